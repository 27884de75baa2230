"""ViT-L/14 and ViT-H/14 shapes end to end against the numpy oracle (fp64, on the CPU): patch 14
(588-column patch vectors at a stride of 640, evt_patchify_ld) and widths 1280, 1408 and 1536
(10 / 12 LayerNorm statistics slots; heads of 80 and 88 on the generic attention kernels).

Gates: the project's, from tests/test_gpu_model.py and tests/test_std_vit.py - f32 max-abs <= 1e-3;
bf16 max-abs <= 3e-2 (scaled by max|oracle| / 3 where the logits exceed 3) and per-row cosine
>= 0.9995. Plus, bit for bit: one image against its row of a batch, two lanes against one, graph
replay against the eager forward."""
import functools

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import tools
from edgevisiontransformer_amd.modeling.models import vit as vitmod
from edgevisiontransformer_amd.modeling.models.vit import StandardViT, ViT
from edgevisiontransformer_amd.weights import (make_images, make_std_vit_params, make_vit_params,
                                               vit_config)
from oracle import vit_ref
from tests.test_gpu_model import BF16_COS, F32_TOL, _cos_rows
from tests.test_std_vit import _bf16_abs_gate

pytestmark = pytest.mark.gpu


def _gate(out, ref, dtype, what):
    out = np.asarray(out, np.float64)
    err = float(np.abs(out - ref).max())
    cos = float(_cos_rows(out, ref).min())
    print(f"{what} {dtype}: max-abs {err:.3e} (max|oracle| {np.abs(ref).max():.3f}), "
          f"min row cosine {cos:.6f}")
    assert np.isfinite(out).all()
    if dtype == "f32":
        assert err <= F32_TOL, f"{what}: f32 max-abs {err:.3e} > {F32_TOL}"
    else:
        gate = _bf16_abs_gate(ref)
        assert err <= gate and cos >= BF16_COS, \
            f"{what}: bf16 max-abs {err:.3e} (<= {gate:.3e}), min cos {cos:.6f} (>= {BF16_COS})"


@functools.lru_cache(maxsize=None)
def _images(batch, size, seed=91):
    return make_images(batch, seed=seed, image_size=size)


@functools.lru_cache(maxsize=None)
def _reference_case(image, dim, depth, heads, mlp, seed):
    """Seeded parameters and fp64 oracle logits of a reference-semantics ViT at patch 14, B = 2."""
    cfg = vit_config(dim, depth, heads, mlp, image_size=image, patch_size=14)
    params = make_vit_params(cfg, seed=seed)
    return cfg, params, vit_ref.vit_forward(params, cfg, _images(2, image))


@functools.lru_cache(maxsize=None)
def _standard_case(dim, seed):
    """Seeded parameters and fp64 oracle logits of a one-layer StandardViT at 224 / 14, B = 2."""
    cfg = vit_config(dim, 1, 16, 4 * dim, image_size=224, patch_size=14)
    params = make_std_vit_params(cfg, seed=seed)
    return cfg, params, vit_ref.std_vit_forward(params, cfg, _images(2, 224), eps=1e-6)


def _vit(gpu, case, dtype, **kw):
    cfg, params, _ = case
    return ViT(image_size=cfg.image_size, patch_size=14, dim=cfg.dim, depth=cfg.depth,
               heads=cfg.heads[0], mlp_dim=cfg.mlp_dim, dtype=dtype, weights=params, device=gpu, **kw)


CASE_A = (28, 1280, 2, 16, 640, 11)   # 5 tokens, heads of 80
CASE_E = (28, 192, 2, 3, 768, 15)     # patch 14 alone, on a width the goldens pin


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_a_vit_1280_five_tokens(gpu, dtype):
    """One-pass generic attention at h_k = 80, the reference head through split-K at K = 1280."""
    case = _reference_case(*CASE_A)
    assert case[0].head_dim[0] == 80 and case[0].num_patches + 1 == 5
    _gate(_vit(gpu, case, dtype)(_images(2, 28)), case[2], dtype, "ViT 28/14 dim 1280")


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_b_standard_vit_huge_layer(gpu, dtype):
    """224 / 14 = 257 tokens at dim 1280: the streaming generic kernel at h_k = 80, the patch
    embedding's position + statistics epilogue over 10 slots, the LN-folded head at K = 1280."""
    cfg, params, ref = _standard_case(1280, 12)
    m = StandardViT(image_size=224, patch_size=14, dim=1280, depth=1, heads=16, mlp_ratio=4,
                    dtype=dtype, weights=params, device=gpu)
    assert m.cfg.num_patches + 1 == 257 and tuple(m.cfg.ffn) == (5120,)
    _gate(m(_images(2, 224)), ref, dtype, "StandardViT 224/14 dim 1280")


def test_c_standard_vit_large_layer(gpu):
    """ViT-L/14: the tuned streaming kernel (h_k = 64) behind the new patchify."""
    cfg, params, ref = _standard_case(1024, 13)
    m = StandardViT(image_size=224, patch_size=14, dim=1024, depth=1, heads=16, dtype="bf16",
                    weights=params, device=gpu)
    assert tuple(m.cfg.head_dim) == (64,) and tuple(m.cfg.ffn) == (4096,)
    _gate(m(_images(2, 224)), ref, "bf16", "StandardViT 224/14 dim 1024")


@pytest.mark.parametrize("dim,heads", [(1536, 24), (1408, 16)])
def test_d_widest_rows(gpu, dim, heads):
    """12 statistics slots, all used (1536) and the last one empty (1408 = 11 slabs of 128);
    heads of 64 and of 88."""
    case = _reference_case(42, dim, 1, heads, 256, 14)
    assert case[0].num_patches + 1 == 10
    _gate(_vit(gpu, case, "bf16")(_images(2, 42)), case[2], "bf16", f"ViT 42/14 dim {dim}")


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_e_patch14_at_192(gpu, dtype):
    case = _reference_case(*CASE_E)
    m = _vit(gpu, case, dtype)
    img = torch.from_numpy(_images(2, 28)).to(gpu)
    pair = m(img)
    _gate(pair.cpu().numpy(), case[2], dtype, "ViT 28/14 dim 192")
    # image 1 alone: the bits of row 1 of the pair
    one = m(img[1:2])
    torch.cuda.synchronize()
    assert torch.equal(one[0], pair[1])


def test_two_lanes_equal_one(gpu):
    """Case a at 4 images: lane children have their own padded patch matrices."""
    case = _reference_case(*CASE_A)
    img = torch.from_numpy(make_images(4, seed=92, image_size=28)).to(gpu)
    m2 = _vit(gpu, case, "bf16", max_batch=4, lanes=2)
    m1 = _vit(gpu, case, "bf16", max_batch=4, lanes=1)
    assert m2.lanes() == 2 and m1.lanes() == 1
    a, b = m2(img).clone(), m1(img).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_graph_replay_equals_eager(gpu):
    case = _reference_case(*CASE_E)
    m = _vit(gpu, case, "bf16", max_batch=2)
    img = torch.from_numpy(_images(2, 28)).to(gpu)
    eager = m(img).clone()
    logits = torch.empty_like(eager)
    m.capture_graph(img, logits)
    m.replay_graph()
    torch.cuda.synchronize()
    assert torch.equal(logits, eager)
    img.copy_(torch.from_numpy(_images(2, 28, seed=93)).to(gpu))
    m.replay_graph()
    torch.cuda.synchronize()
    assert torch.equal(logits, m(img))


def test_tools_builds_vit_huge(gpu, monkeypatch):
    """tools.build_model by timm name. The 32 layers are 2.5 GB of fp32 parameters to draw on the
    host, so the name is built at depth 2 (the full configuration's shapes are checked on the CPU
    in tests/test_vit_patch14_validation.py)."""
    assert "vit_huge_patch14_224" in tools.STD_VIT_NAMED
    full = vitmod.STD_VIT_NAMED["vit_huge_patch14_224"]
    assert (full["dim"], full["depth"], full["heads"], full["patch_size"]) == (1280, 32, 16, 14)
    monkeypatch.setitem(vitmod.STD_VIT_NAMED, "vit_huge_patch14_224", {**full, "depth": 2})
    m = tools.build_model("vit_huge_patch14_224", "bf16")
    assert isinstance(m, StandardViT) and m.cfg.depth == 2 and m.cfg.head_dim[0] == 80
    assert tuple(m.cfg.ffn) == (5120, 5120) and m.cfg.num_patches + 1 == 257
    out = m(_images(1, 224))
    assert out.shape == (1, 1000) and np.isfinite(out).all()
    with pytest.raises(ValueError):
        tools.build_model("vit_huge_patch14_224", "bf16", prune_encoding="all_head2_ffn0.7")
    m = vitmod.vit_large_patch14_224(depth=1, dtype="bf16", device=gpu)
    assert m.cfg.depth == 1 and m.cfg.dim == 1024 and m.cfg.patch_size == 14
