"""CPU: host-side mirror of the reference API (prune encodings, configs, FLOP accounting)."""
import json
import os

import numpy as np
import pytest

from edgevisiontransformer_amd.modeling.models.vit import (_cfg_for, decode_prune_encoding,
                                                           pruned_config)
from edgevisiontransformer_amd.weights import (make_images, make_vit_params, vit_config,
                                               vit_param_shapes)


def test_decode_all():
    assert decode_prune_encoding("all_head12_ffn1.0") == ("all", 12, 1.0)
    assert decode_prune_encoding("all_head2_ffn0.7") == ("all", 2, 0.7)


def test_decode_layerwise():
    s, h, d = decode_prune_encoding("layerwise_h2-d1.0_h3-d0.5_h1-d0.5")
    assert s == "layerwise" and h == [2, 3, 1] and d == [1.0, 0.5, 0.5]


def test_decode_rejects_unknown_setting():
    with pytest.raises(AssertionError):
        decode_prune_encoding("some_head2_ffn0.5")


@pytest.mark.parametrize("thr,width", [(0.1, 76), (0.2, 153), (0.3, 230), (0.4, 307), (0.5, 384),
                                       (0.6, 460), (0.7, 537), (0.8, 614), (0.9, 691)])
def test_prune_benchmark_tiny_widths(thr, width):
    """experiments.py:171-180 builds all_head3_ffn{thr} with int(thr * 768)."""
    cfg = pruned_config(f"all_head3_ffn{thr}", dim=192, depth=12, heads=3, mlp_dim=768)
    assert set(cfg.ffn) == {width} and set(cfg.heads) == {3} and set(cfg.head_dim) == {64}


def test_layerwise_length_must_match_depth():
    with pytest.raises(AssertionError):
        pruned_config("layerwise_h1-d0.5", dim=192, depth=2, heads=3, mlp_dim=768)


def test_gflops_match_baseline_table():
    assert abs(_cfg_for("deit_base").gflop_per_image() - 35.137) < 1e-3
    assert abs(_cfg_for("deit_tiny").gflop_per_image() - 2.509) < 1e-3


def test_gflops_cross_check_reference_counter():
    """The reference's own analytic counter (flops_calculation.py:216-251, includes elementwise)
    lands within 2% of our matmul-only figure. The counter's result for DeiT-base
    (ViTHparams(h=768, l=12, heads=12).get_infer_flops()) is recorded in tests/golden."""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_flops.json")
    with open(golden) as f:
        rec = json.load(f)["deit_base"]
    assert (rec["h"], rec["l"], rec["heads"]) == (768, 12, 12)
    base = rec["infer_flops"] / 1e9
    assert abs(base - 35.295) < 1e-3                                   # 35.295 incl. elementwise
    assert abs(base - _cfg_for("deit_base").gflop_per_image()) / base < 0.02


def test_weights_deterministic_and_shaped():
    cfg = vit_config(128, 2, 2, 256, num_classes=10)
    a, b = make_vit_params(cfg, seed=3), make_vit_params(cfg, seed=3)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    for name, shape in vit_param_shapes(cfg):
        assert a[name].shape == shape and a[name].dtype == np.float32
    assert len(vit_param_shapes(cfg)) == 4 + 11 * cfg.depth + 4
    img = make_images(2, seed=1, image_size=32, layout="NHWC")
    assert img.shape == (2, 32, 32, 3)


def test_t2t_config_and_flops():
    from edgevisiontransformer_amd.modeling.models.t2t_vit import t2t_cfg_for
    from edgevisiontransformer_amd.weights import make_t2t_params, t2t_param_shapes
    c = t2t_cfg_for("t2t_vit_14")
    assert (c.dim, c.depth, c.heads, c.mlp_dim) == (384, 14, 6, 1152)   # t2t_vit.py:147-148
    assert c.grids == (56, 28, 14) and c.tokens == 197 and c.split_dims == (147, 576, 576)
    assert abs(c.gflop_per_image() - 9.567) < 2e-3
    c7 = t2t_cfg_for("t2t_vit_7")
    p = make_t2t_params(c7, seed=0)
    assert [k for k, _ in t2t_param_shapes(c7)] == list(p)
    w = p["p1.w"].astype(np.float64)
    np.testing.assert_allclose(w @ w.T, 32 * np.eye(32), atol=1e-4)    # Orthogonal * sqrt(m)


def test_t2t_rejects_unsupported_tokens_type():
    from edgevisiontransformer_amd.modeling.models.t2t_vit import T2T_ViT
    with pytest.raises(NotImplementedError):
        T2T_ViT(tokens_type="transformer")


def test_default_lanes_policy(monkeypatch):
    """Batch lanes of new T2T-ViT / Swin handles (_lib.default_lanes): two from 128 images in
    bf16, one otherwise; EVT_LANES overrides (the A/B switch)."""
    from edgevisiontransformer_amd import _lib
    monkeypatch.delenv("EVT_LANES", raising=False)
    assert _lib.default_lanes("bf16", 256) == 2
    assert _lib.default_lanes("bf16", _lib.LANES_MIN_BATCH) == 2
    assert _lib.default_lanes("bf16", _lib.LANES_MIN_BATCH - 1) == 1
    assert _lib.default_lanes("f32", 256) == 1
    assert _lib.default_lanes("f32", 256, vit=True) == 2   # ViT: the fp32 path
    assert _lib.default_lanes("bf16", 512, vit=True) == 1
    assert _lib.default_lanes("f32", 64, vit=True) == 1
    monkeypatch.setenv("EVT_LANES", "1")
    assert _lib.default_lanes("bf16", 256) == 1
    monkeypatch.setenv("EVT_LANES", "3")
    assert _lib.default_lanes("f32", 8) == 3
