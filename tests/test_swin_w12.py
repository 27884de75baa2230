"""CPU: the window-12 Swin configurations (swin_*_patch4_window12_384). The oracle against the
window-12 goldens (tests/golden/make_golden_swin_w12.py: HuggingFace SwinForImageClassification in
float64), the config names, the host-side validation of the C API, and tools.build_model's name /
size handling. No GPU is touched."""
import ctypes
import os

import numpy as np
import pytest

from edgevisiontransformer_amd import _lib, tools
from edgevisiontransformer_amd.modeling.models.swin import swin_config_from_name
from edgevisiontransformer_amd.weights import (digest, make_images, make_swin_params, swin_config,
                                               swin_param_shapes)
from oracle import swin_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W12_GOLDENS = ["swin_w12_base_micro_b2", "swin_w12_r36_b2", "swin_w12_c96_b2"]


def golden_case_w12(name):
    """As test_swin_oracle.golden_case, with the window the .npz stores."""
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    cfg = swin_config("tiny", image_size=int(z["image_size"]), embed_dim=int(z["embed_dim"]),
                      depths=tuple(int(v) for v in z["depths"]),
                      num_heads=tuple(int(v) for v in z["num_heads"]),
                      num_classes=int(z["num_classes"]), window_size=int(z["window_size"]))
    params = make_swin_params(cfg, seed=int(z["param_seed"]))
    img = make_images(int(z["batch"]), seed=int(z["image_seed"]), image_size=cfg.image_size)
    assert digest(params) == str(z["param_digest"])
    assert digest([img]) == str(z["image_digest"])
    return z, cfg, params, img


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from edgevisiontransformer_amd.build import build
        build()
    return _lib.load_library()


@pytest.mark.parametrize("name", W12_GOLDENS)
def test_oracle_matches_w12_golden(name):
    z, cfg, params, img = golden_case_w12(name)
    assert cfg.window_size == 12
    trace = {}
    out = swin_ref.swin_forward(params, cfg, img, trace=trace)
    assert np.abs(out - z["logits"]).max() < 1e-9
    assert np.abs(trace["embed"][:, :8] - z["embed"]).max() < 1e-12


def test_w12_goldens_reach_what_they_claim():
    _, cfg, _, _ = golden_case_w12("swin_w12_base_micro_b2")
    assert [(cfg.res(i), cfg.window(i), cfg.shift(i, 1)) for i in range(2)] == [(24, 12, 6), (12, 12, 0)]
    assert [cfg.dim(i) for i in range(2)] == [128, 256]
    _, cfg, _, _ = golden_case_w12("swin_w12_r36_b2")
    assert (cfg.res(0), cfg.window(0), cfg.shift(0, 1), cfg.num_stages) == (36, 12, 6, 1)
    _, cfg, _, _ = golden_case_w12("swin_w12_c96_b2")
    assert cfg.dim(0) == 96 and cfg.num_heads == (3, 6) and cfg.window(0) == 12


def test_window12_config_names():
    c = swin_config_from_name("swin_base_patch4_window12_384")
    assert c.embed_dim == 128 and c.depths == (2, 2, 18, 2) and c.num_heads == (4, 8, 16, 32)
    assert c.window_size == 12 and c.image_size == 384
    assert [(c.res(i), c.window(i)) for i in range(4)] == [(96, 12), (48, 12), (24, 12), (12, 12)]
    assert [c.shift(i, 1) for i in range(4)] == [6, 6, 6, 0]
    assert [p for n, p in swin_param_shapes(c) if n == "s2.b0.rpb"] == [(529, 16)]
    for v, e in (("tiny", 96), ("small", 96)):
        c = swin_config_from_name(f"swin_{v}_patch4_window12_384")
        assert (c.embed_dim, c.window_size, c.image_size) == (e, 12, 384)


def _desc(cfg, dtype=1, max_batch=16):
    d = _lib.evt_swin_desc()
    d.image_size, d.patch_size, d.in_chans = cfg.image_size, cfg.patch_size, cfg.in_chans
    d.num_classes, d.embed_dim, d.num_stages = cfg.num_classes, cfg.embed_dim, cfg.num_stages
    for i in range(cfg.num_stages):
        d.depths[i], d.num_heads[i] = cfg.depths[i], cfg.num_heads[i]
    d.window_size, d.mlp_ratio = cfg.window_size, cfg.mlp_ratio
    d.dtype, d.max_batch = dtype, max_batch
    return d


def test_swin_w12_host_validation(lib):
    cfg = swin_config_from_name("swin_base_patch4_window12_384")
    d = _desc(cfg)
    out = ctypes.c_size_t()
    assert lib.evt_swin_query_workspace(ctypes.byref(d), 16, ctypes.byref(out)) == _lib.EVT_OK
    # at least the qkv buffer and the two streams of stage 1 for 16 images in bf16
    assert out.value > 16 * 96 * 96 * 128 * 5 * 2
    assert lib.evt_swin_num_weights(ctypes.byref(d)) == len(swin_param_shapes(cfg))
    # 96 px over three stages at window 12: R = 24, 12, 6 -> the last stage would be 6 x 6
    small = swin_config("base", image_size=96, window_size=12, depths=(2, 2, 2),
                        num_heads=(4, 8, 16))
    d6 = _desc(small)
    assert lib.evt_swin_query_workspace(ctypes.byref(d6), 16, ctypes.byref(out)) == _lib.EVT_EINVAL
    assert b"stage 2" in lib.evt_last_error()
    d8 = _desc(cfg)
    d8.window_size = 8
    assert lib.evt_swin_query_workspace(ctypes.byref(d8), 16, ctypes.byref(out)) == _lib.EVT_EINVAL
    assert b"window_size" in lib.evt_last_error()
    # window 7 at 384 px: 96 is no multiple of 7
    d7 = _desc(cfg)
    d7.window_size = 7
    assert lib.evt_swin_query_workspace(ctypes.byref(d7), 16, ctypes.byref(out)) == _lib.EVT_EINVAL
    assert b"stage 0" in lib.evt_last_error()


def test_swin_w12_max_batch_bound(lib):
    """Stage 1 of Swin-B at 384 px: 9216 tokens x 512 hidden x 2 B = 9 MiB per image in bf16, so
    the FC1 hidden reaches 2^31 bytes at 228 images (2^31 / (9216 * 512 * 2) = 227.6); in fp32
    the same buffer does at 114. The 224 px configurations keep batch 256."""
    cfg = swin_config_from_name("swin_base_patch4_window12_384")
    out = ctypes.c_size_t()
    for dtype, ok, bad in ((1, 227, 228), (0, 113, 114)):
        d = _desc(cfg, dtype=dtype, max_batch=ok)
        assert lib.evt_swin_query_workspace(ctypes.byref(d), ok, ctypes.byref(out)) == _lib.EVT_OK
        d = _desc(cfg, dtype=dtype, max_batch=bad)
        assert lib.evt_swin_query_workspace(ctypes.byref(d), bad, ctypes.byref(out)) == _lib.EVT_EINVAL
        assert b"2^31" in lib.evt_last_error()
    d = _desc(swin_config_from_name("swin_base_patch4_window7_224"), max_batch=256)
    assert lib.evt_swin_query_workspace(ctypes.byref(d), 256, ctypes.byref(out)) == _lib.EVT_OK


def test_python_validation_before_any_device_work():
    from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer
    with pytest.raises(ValueError, match="window_size"):
        SwinTransformer(img_size=384, window_size=8)
    with pytest.raises(ValueError, match="stage 2"):
        SwinTransformer(img_size=96, window_size=12, embed_dim=128, depths=(2, 2, 2),
                        num_heads=(4, 8, 16))
    with pytest.raises(ValueError, match="stage 0"):
        SwinTransformer(img_size=384, window_size=7)


def test_build_model_names_and_sizes(monkeypatch):
    """A full config name carries its own size; refused before any model is built."""
    import edgevisiontransformer_amd.modeling.models.swin as swin_mod
    built = []
    monkeypatch.setattr(swin_mod, "get_swin", lambda name, **kw: built.append((name, kw)) or name)
    assert tools.build_model("swin_base_patch4_window12_384", "bf16", max_batch=16,
                             image_size=384) == "swin_base_patch4_window12_384"
    assert built[-1][1]["max_batch"] == 16 and built[-1][1]["dtype"] == "bf16"
    assert tools.build_model("swin_tiny", "f32") == "swin_tiny_patch4_window7_224"
    n = len(built)
    with pytest.raises(ValueError, match="384"):
        tools.build_model("swin_base_patch4_window12_384", "bf16", image_size=224)
    with pytest.raises(ValueError, match="224"):
        tools.build_model("swin_base_patch4_window7_224", "bf16", image_size=384)
    with pytest.raises(ValueError, match="224"):
        tools.build_model("swin_base", "bf16", image_size=384)
    assert len(built) == n
    shape = tools._input_shape("swin_base_patch4_window12_384", "16,3,384,384")
    assert tools._image_size("swin_base_patch4_window12_384", shape) == 384
