"""GPU parity of the window-12 Swin path (swin_*_patch4_window12_384): whole forwards against the
HF-produced fp64 goldens (tests/golden/make_golden_swin_w12.py), single-stage one- and two-block
models against the numpy oracle, batch independence / HIP-graph replay / batch lanes bitwise, the
C = 96 model on the GEMM path, and the published 384 px shape in bf16 against fp32.

The window-12 kernels have no op-level entry point (evt_window_attention stays a window-7 op):
they are reached through the model, as here.

Tolerances are those of tests/test_gpu_swin.py: f32 path max-abs <= 1e-3 on logits; bf16 path
max-abs <= 3e-2 and per-row cosine >= 0.9995.
"""
import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import profiling
from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer, get_swin
from edgevisiontransformer_amd.weights import make_images, make_swin_params, swin_config
from oracle import swin_ref
from tests.test_swin_w12 import W12_GOLDENS, golden_case_w12

pytestmark = pytest.mark.gpu


def _model(cfg, dtype, params, gpu, **kw):
    return SwinTransformer(img_size=cfg.image_size, patch_size=cfg.patch_size,
                           num_classes=cfg.num_classes, embed_dim=cfg.embed_dim,
                           depths=cfg.depths, num_heads=cfg.num_heads,
                           window_size=cfg.window_size, dtype=dtype, weights=params, device=gpu,
                           **kw)


def _cos_rows(a, b):
    return (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def _gate(out, ref, dtype, what):
    err = np.abs(out - ref).max()
    print(f"{what} {dtype}: max-abs {err:.3e}")
    if dtype == "f32":
        assert err <= 1e-3, f"{what} f32 max-abs {err:.3e}"
    else:
        assert err <= 3e-2, f"{what} bf16 max-abs {err:.3e}"
        assert _cos_rows(out, ref).min() >= 0.9995


@pytest.mark.parametrize("name", W12_GOLDENS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_swin_w12_golden(gpu, name, dtype):
    z, cfg, params, img = golden_case_w12(name)
    m = _model(cfg, dtype, params, gpu)
    out = m(torch.from_numpy(img).to(gpu)).cpu().numpy().astype(np.float64)
    _gate(out, z["logits"], dtype, name)


@pytest.mark.parametrize("image_size", [96, 144])   # R = 24 (2 x 2 windows), R = 36 (3 x 3)
@pytest.mark.parametrize("depth", [1, 2])           # one W-MSA block; W-MSA + SW-MSA
def test_swin_w12_single_stage_blocks_f32(gpu, image_size, depth):
    """One stage of one or two blocks in f32 against the oracle on the same inputs: nothing after
    the window attention but its own block's proj / MLP and the pooled head, so a wrong bias
    index, region or row map is not averaged away by later stages.

    Measured max-abs error of the f32 path on an MI355X: 1.6e-7 (R = 24, depth 1), 2.9e-7
    (R = 36, depth 1), 3.9e-7 (R = 24, depth 2), 4.6e-7 (R = 36, depth 2): fp32 rounding of
    logits of order 1. The gate is 2e-5, the f32 tolerance of the window-7 kernel test in
    tests/test_gpu_swin.py and 43 times the largest measured error, instead of the 1e-3 of the
    full-model gate."""
    cfg = swin_config("tiny", image_size=image_size, window_size=12, embed_dim=64, depths=(depth,),
                      num_heads=(2,), num_classes=11)
    params = make_swin_params(cfg, seed=41 + depth)
    img = make_images(2, seed=43, image_size=image_size)
    ref = swin_ref.swin_forward(params, cfg, img)
    out = _model(cfg, "f32", params, gpu)(torch.from_numpy(img).to(gpu)).cpu().numpy()
    err = np.abs(out.astype(np.float64) - ref).max()
    print(f"R={image_size // 4} depth={depth} f32: max-abs {err:.3e}")
    assert err <= 2e-5, f"R={image_size // 4} depth={depth} f32 max-abs {err:.3e}"


@pytest.mark.parametrize("image_size", [96, 144])
def test_swin_w12_single_stage_blocks_bf16(gpu, image_size):
    """The bf16 kernel's own sharp check. bf16 rounding (2^-9 relative at every stored
    activation) sits close to what a wrong mask region does to the logits of a seeded model,
    where the residual stream carries mostly the patch embedding. Here both blocks' proj weights
    are scaled by 8, so the window attention's output dominates the stream (and, through the
    final LayerNorm, the logits) while the rounding stays relative: the existing bf16 gate
    (max-abs 3e-2, row cosine 0.9995) then separates the two."""
    cfg = swin_config("tiny", image_size=image_size, window_size=12, embed_dim=64, depths=(2,),
                      num_heads=(2,), num_classes=11)
    params = dict(make_swin_params(cfg, seed=47))
    for j in range(2):
        params[f"s0.b{j}.proj_w"] = params[f"s0.b{j}.proj_w"] * 8.0
        params[f"s0.b{j}.proj_b"] = params[f"s0.b{j}.proj_b"] * 8.0
    img = make_images(2, seed=48, image_size=image_size)
    ref = swin_ref.swin_forward(params, cfg, img)
    out = _model(cfg, "bf16", params, gpu)(torch.from_numpy(img).to(gpu)).cpu().numpy()
    out = out.astype(np.float64)
    print(f"R={image_size // 4} bf16 cos {_cos_rows(out, ref).min():.6f}")
    _gate(out, ref, "bf16", f"R={image_size // 4} depth=2, proj x 8")


def test_swin_w12_batch_independence_and_graph(gpu):
    """Image i's logits do not depend on its batch neighbours (bitwise), and a HIP-graph replay
    reproduces the eager forward bitwise. Both window-12 kernels launch one block per (image,
    window, head), so no block of theirs is ever partial; the odd batch of 5 makes the last
    blocks of the GEMM and row kernels around them partial."""
    cfg = swin_config("base", image_size=96, window_size=12, depths=(2, 2), num_heads=(4, 8),
                      num_classes=19)
    params = make_swin_params(cfg, seed=5)
    img = torch.from_numpy(make_images(5, seed=6, image_size=96)).to(gpu)
    for dtype in ("bf16", "f32"):
        m = _model(cfg, dtype, params, gpu, max_batch=5)
        full = m(img)
        part = m(img[2:4].contiguous())
        assert torch.equal(full[2:4], part), dtype
        logits = torch.empty_like(full)
        m.capture_graph(img, logits)
        m.replay_graph()
        torch.cuda.synchronize()
        assert torch.equal(logits, full), dtype


def test_swin_w12_c96_takes_the_gemm_path(gpu):
    """C = 96 with 3 heads at window 12: logits within the bf16 gate of the golden, and the
    per-role profile shows the unfused path (im2col + patch GEMM, QKV / window attention / proj,
    FC1 / FC2) and none of the fused window-7 kernels (patch embedding without im2col,
    attn_sublayer, mlp)."""
    z, cfg, params, img = golden_case_w12("swin_w12_c96_b2")
    m = _model(cfg, "bf16", params, gpu, max_batch=2)
    x = torch.from_numpy(img).to(gpu)
    out = m(x)
    _gate(out.cpu().numpy().astype(np.float64), z["logits"], "bf16", "swin_w12_c96_b2")
    kt = profiling.kernel_times(m, x, torch.empty_like(out), forwards=1)
    assert "attn_sublayer" not in kt and "mlp" not in kt
    for role in ("patchify", "patch_embed", "qkv", "attention", "out_proj", "fc1", "fc2"):
        assert kt[role]["launches"] >= 1, role
    assert kt["attention"]["launches"] == kt["qkv"]["launches"] == kt["fc1"]["launches"]


def test_swin_base_window12_384_bf16_against_f32(gpu):
    """The published shape: swin_base_patch4_window12_384 on two images, bf16 against f32 (the f32
    path is pinned by the micro goldens) within the bf16 gate."""
    from edgevisiontransformer_amd.modeling.models.swin import swin_config_from_name
    params = make_swin_params(swin_config_from_name("swin_base_patch4_window12_384"), seed=7)
    x = torch.from_numpy(make_images(2, seed=8, image_size=384)).to(gpu)
    out = {}
    for dtype in ("f32", "bf16"):
        m = get_swin("swin_base_patch4_window12_384", dtype=dtype, weights=params, device=gpu,
                     max_batch=2)
        assert [m.cfg.window(i) for i in range(4)] == [12, 12, 12, 12]
        out[dtype] = m(x).cpu().numpy().astype(np.float64)
        m.close()
    assert np.isfinite(out["f32"]).all()
    _gate(out["bf16"], out["f32"], "bf16", "swin_base_patch4_window12_384")


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_swin_w12_lanes_bitwise(gpu, dtype):
    """A two-lane window-12 handle gives the logits of the same handle with one lane, bitwise."""
    cfg = swin_config("base", image_size=96, window_size=12, depths=(2, 2), num_heads=(4, 8),
                      num_classes=19)
    params = make_swin_params(cfg, seed=9)
    img = torch.from_numpy(make_images(5, seed=10, image_size=96)).to(gpu)
    m2 = _model(cfg, dtype, params, gpu, max_batch=5, lanes=2)
    m1 = _model(cfg, dtype, params, gpu, max_batch=5, lanes=1)
    assert m2.lanes() == 2 and m1.lanes() == 1
    assert torch.equal(m2(img), m1(img))
