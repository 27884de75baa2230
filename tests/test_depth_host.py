"""CPU: the host side of the depth axis (include/evt_depth.h, modeling/models/depth.py):
`block_stats_reference`, the skip grammar, `drop_blocks`, the importance and selection helpers,
`tools.py --skip`, the header / binding / build lists, and the argument checks of the C ABI that
return before anything touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from edgevisiontransformer_amd import _lib, pruning
from edgevisiontransformer_amd.modeling.models.depth import (DEPTH_STATS, FLT_MIN, IDENTITY_STATS,
                                                             block_stats_reference, checked_skips,
                                                             mask_to_skips, parse_skips)
from edgevisiontransformer_amd.tools import parse_server_args
from edgevisiontransformer_amd.weights import (make_std_vit_params, make_vit_params,
                                               std_vit_param_shapes, vit_config, vit_param_shapes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_stats_reference_properties():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((3 * 5, 16))
    assert DEPTH_STATS == ("cosine", "rel_update", "norm_ratio", "cls_cosine")
    assert np.array_equal(block_stats_reference(a, a, 5), np.tile(IDENTITY_STATS, (3, 1)))
    assert np.allclose(block_stats_reference(a, -a, 5), np.tile((-1.0, 2.0, 1.0, -1.0), (3, 1)))
    s = block_stats_reference(a, 3.0 * a, 5)
    assert np.allclose(s, np.tile((1.0, 2.0, 3.0, 1.0), (3, 1)))
    b = rng.standard_normal(a.shape)
    got = block_stats_reference(a, b, 5)
    assert got.shape == (3, 4) and (np.abs(got[:, [0, 3]]) <= 1).all()
    # per image: image 1 alone is row 1; token 0 is the CLS column
    assert np.array_equal(block_stats_reference(a[5:10], b[5:10], 5)[0], got[1])
    cls = (a[5] * b[5]).sum() / (np.linalg.norm(a[5]) * np.linalg.norm(b[5]))
    assert np.isclose(got[1, 3], cls)
    # orthogonal rows: cosine 0, |b - a| = sqrt(2) |a|
    e = np.zeros((2, 8))
    f = np.zeros((2, 8))
    e[:, 0], f[:, 1] = 2.0, 2.0
    assert np.allclose(block_stats_reference(e, f, 2), [[0.0, np.sqrt(2.0), 1.0, 0.0]])
    # a zero row of a: the FLT_MIN clamp keeps everything finite in fp64
    z = a.copy()
    z[7] = 0.0
    zs = block_stats_reference(z, b, 5)
    assert np.isfinite(zs).all() and zs[1, 2] > 1.0 / FLT_MIN / 5 * 0.1
    # the small update that the three dot products would cancel
    small = a + 2.0 ** -20 * rng.standard_normal(a.shape)
    rel = block_stats_reference(a, small, 5)[:, 1]
    assert (rel > 2.0 ** -22).all() and (rel < 2.0 ** -18).all()
    for bad in ((a, b[:-1], 5), (a, b, 4), (a[0], b[0], 1), (a, b, 0)):
        with pytest.raises(ValueError):
            block_stats_reference(*bad)


def test_skip_grammar():
    assert checked_skips(4, {1: "attn", -1: "ffn", 2: "block"}) == [0, 1, 3, 2]
    assert checked_skips(3, None) == [0, 0, 0] and checked_skips(3, {}) == [0, 0, 0]
    assert checked_skips(3, {0: "attn", -3: "ffn"}) == [3, 0, 0]  # a block named twice gets both
    assert mask_to_skips([0, 1, 3, 2]) == {1: "attn", 2: "block", 3: "ffn"}
    for bad in ({4: "attn"}, {-5: "ffn"}, {0: "mlp"}, {True: "attn"}, {1.5: "attn"}, {"1": "ffn"}):
        with pytest.raises(ValueError):
            checked_skips(4, bad)
    assert parse_skips("5:attn,9:block,-1:ffn") == {5: "attn", 9: "block", -1: "ffn"}
    assert parse_skips("3:attn, 3:ffn,") == {3: "block"}
    assert parse_skips("") == {} and parse_skips(None) == {}
    for bad in ("5", "5:head", "a:attn", "5:attn:ffn"):
        with pytest.raises(ValueError, match="block:attn"):
            parse_skips(bad)


def test_tools_skip_flag():
    args = parse_server_args(["gpu_benchmark", "--model", "deit_base", "--skip", "10:attn,11:block"])
    assert args.skip == {10: "attn", 11: "block"}
    assert parse_server_args(["gpu_benchmark", "--model", "deit_base"]).skip is None
    with pytest.raises(ValueError):
        parse_server_args(["gpu_benchmark", "--model", "deit_base", "--skip", "10:heads"])


@pytest.mark.parametrize("standard", [False, True])
def test_drop_blocks(standard):
    cfg = vit_config(64, 4, 2, 128, image_size=32, patch_size=16, num_classes=5, head_size=32,
                     heads_list=(1, 2, 2, 1), ffn_list=(64, 128, 96, 32))
    make, shapes = (make_std_vit_params, std_vit_param_shapes) if standard else \
        (make_vit_params, vit_param_shapes)
    params = make(cfg, seed=3)
    p2, c2 = pruning.drop_blocks(params, cfg, (1, -1))
    assert c2.depth == 2 and tuple(c2.heads) == (1, 2) and tuple(c2.ffn) == (64, 96)
    assert tuple(c2.head_dim) == (32, 32) and (c2.dim, c2.tokens) == (cfg.dim, cfg.tokens)
    assert sorted(p2) == sorted(n for n, _ in shapes(c2))
    for name, shape in shapes(c2):
        assert tuple(p2[name].shape) == tuple(shape), name
    for new, old in ((0, 0), (1, 2)):
        for name in params:
            if name.startswith(f"l{old}."):
                assert p2[f"l{new}." + name.split(".", 1)[1]] is params[name]
    assert p2["pos"] is params["pos"]
    same, c0 = pruning.drop_blocks(params, cfg, ())
    assert c0 == cfg and sorted(same) == sorted(params)
    none, cn = pruning.drop_blocks(params, cfg, range(4))
    assert cn.depth == 0 and not any(k.startswith("l") and "." in k for k in none)
    for bad in ((4,), (-5,), (1, 1), (1, -3), (True,), (1.0,)):
        with pytest.raises(ValueError):
            pruning.drop_blocks(params, cfg, bad)


def test_importance_and_selection():
    means = [np.array([[0.9, 0.5, 1.1, 0.8], [0.99, 0.05, 1.0, 0.9]]),
             np.array([[0.5, 0.9, 1.2, 0.4], [1.0, 0.0, 1.0, 1.0]])]
    imp = pruning.sublayer_importance_from_stats(means)
    assert np.allclose(imp, [[0.1, 0.01], [0.5, 0.0]])
    assert np.allclose(pruning.sublayer_importance_from_stats(means, kind="rel_update"),
                       [[0.5, 0.05], [0.9, 0.0]])
    batch = [np.stack([m, m]) for m in means]  # [B, 2, 4] is averaged over its images
    assert np.allclose(pruning.sublayer_importance_from_stats(batch), imp)
    for bad in (dict(means=means, kind="norm_ratio"), dict(means=[]), dict(means=[np.zeros((4, 2))])):
        with pytest.raises(ValueError):
            pruning.sublayer_importance_from_stats(**bad)
    assert pruning.sublayers_from_importance(imp, drop=0) == {}
    assert pruning.sublayers_from_importance(imp, drop=1) == {1: "ffn"}
    assert pruning.sublayers_from_importance(imp, drop=2) == {0: "ffn", 1: "ffn"}
    assert pruning.sublayers_from_importance(imp, drop=3) == {0: "block", 1: "ffn"}
    assert pruning.sublayers_from_importance(imp, drop=4) == {0: "block", 1: "block"}
    assert pruning.sublayers_from_importance(imp, drop=1, blocks=(7, 9)) == {9: "ffn"}
    ties = np.zeros((2, 2))  # the earlier block first, attention before FFN
    assert pruning.sublayers_from_importance(ties, drop=1) == {0: "attn"}
    assert pruning.sublayers_from_importance(ties, drop=3) == {0: "block", 1: "attn"}
    for bad in (dict(importance=imp, drop=5), dict(importance=imp, drop=-1),
                dict(importance=imp[:, :1], drop=1), dict(importance=np.full((2, 2), np.nan), drop=1),
                dict(importance=imp, drop=1, blocks=(1,))):
        with pytest.raises(ValueError):
            pruning.sublayers_from_importance(**bad)
    res = {"base": {"acc1": 0.8}, "acc1": [[0.7, 0.8], [float("nan"), 0.85]], "blocks": [0, 3]}
    got = pruning.importance_from_sublayer_ablation(res)
    assert np.allclose(got, [[0.1, 0.0], [0.0, -0.05]])
    assert pruning.sublayers_from_importance(got, drop=1, blocks=res["blocks"]) == {3: "ffn"}
    with pytest.raises(ValueError):
        pruning.importance_from_sublayer_ablation({"base": {"acc1": 0.8}, "acc1": []})


def test_header_binding_and_build_lists():
    txt = open(os.path.join(ROOT, "include", "evt_depth.h")).read()
    declared = sorted(set(re.findall(r"^int\s+(evt_\w+)\(", txt, re.M)))
    assert declared == sorted(_lib.DEPTH_SIGNATURES) and len(declared) == 5
    from edgevisiontransformer_amd.build import HEADERS, SOURCES
    assert '#include "evt_depth.h"' in open(os.path.join(ROOT, "include", "evt.h")).read()
    assert "depth_stats.hip" in SOURCES and any(h.endswith("evt_depth.h") for h in HEADERS)
    for name, value in (("EVT_DEPTH_STATS", _lib.DEPTH_STATS), ("EVT_SKIP_ATTN", _lib.SKIP_ATTN),
                        ("EVT_SKIP_FFN", _lib.SKIP_FFN), ("EVT_DEPTH_FFN", _lib.DEPTH_FFN),
                        ("EVT_DEPTH_CLS_COSINE", _lib.DEPTH_CLS_COSINE)):
        assert re.search(rf"#define {name} {value}\b", txt), name
    assert ctypes.sizeof(_lib.evt_block_stats_args) == 24


def test_c_abi_argument_checks_without_a_device():
    if not os.path.exists(_lib.LIB_PATH):
        from edgevisiontransformer_amd.build import build
        build()
    lib = _lib.load_library()
    for name in _lib.DEPTH_SIGNATURES:
        assert hasattr(lib, name), name
    buf = (ctypes.c_float * 256)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base + (-base) % 16)
    off = ctypes.c_void_p(p.value + 8)
    ok = [1, p, 64, p, 64, 1, 2, 64, p]
    for i, v, msg in ((0, 2, b"dtype"), (5, 0, b"B must"), (6, 0, b"T must"), (6, 4097, b"T must"),
                      (7, 0, b"multiple of 8"), (7, 20, b"multiple of 8"), (2, 32, b"at least D"),
                      (4, 63, b"at least D"), (2, 68, b"16 bytes"), (1, None, b"non-null"),
                      (8, None, b"non-null"), (3, off, b"aligned"), (8, off, b"aligned")):
        args = list(ok)
        args[i] = v
        assert lib.evt_stream_delta_stats(*args, None) == _lib.EVT_EINVAL, (i, v)
        assert msg in lib.evt_last_error(), (i, v, lib.evt_last_error())
    n = ctypes.c_int()
    r = ctypes.byref(n)
    assert lib.evt_block_stats_shape(None, 0, r, r, r) == _lib.EVT_EINVAL
    assert lib.evt_forward_block_stats(None, None, 1, None, None, None) == _lib.EVT_EINVAL
    assert lib.evt_model_set_skips(None, None, 0, None) == _lib.EVT_EINVAL
    assert lib.evt_model_get_skips(None, None, 0, r) == _lib.EVT_EINVAL
