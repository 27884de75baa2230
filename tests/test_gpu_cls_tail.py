"""GPU: the encoder's CLS tail (include/evt_tail.h): the last block's out-proj, FC1 and FC2 on the
B CLS rows, its attention on query tile 0 (bf16, head size 64), and the full-row block alongside
when a call exports the last token map.

Seeded weights against the fp64 oracles, "f32" and "bf16", at the shapes where this can go wrong:

  ref_192      REFERENCE ViT dim 192, 5 tokens, B = 1, 3 and 130: at 130 the M = B launches have a
               partial second row tile; head size 64, so bf16 runs the CLS-query attention
  std_384_224  STANDARD ViT dim 384 at 224 px, B = 2: the CLS rows sit 197 rows apart and the
               final LayerNorm reads the statistics the tail's FC2 wrote
  std_1408     STANDARD ViT dim 1408, 5 tokens: 12 statistics slots, a partial last column tile
  pruned       ViT_Pruned, layerwise: the last layer's heads (2) and ffn (0.3) differ from the rest
  t2t          T2T-ViT at its smallest configuration (it shares the encoder)

Gates (the project's own): f32 max-abs <= 1e-3 * max(1, max|golden|); bf16 the logits gate of
tests/test_gpu_model.py, max-abs <= 3e-2 and every row's cosine >= 0.9995. Everything else is
exact: evt_model_tail_mode, plain logits == features-forward logits, pooled == tokens[:, 0], a
batch permutation permutes the logits, one image alone gives the bits it gives in a batch, a plain
forward after a features forward is unchanged, a captured graph replays to the eager logits.
"""
import functools

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd.modeling.models.t2t_vit import T2T_ViT
from edgevisiontransformer_amd.modeling.models.vit import (StandardViT, ViT, ViT_Pruned,
                                                           pruned_config)
from edgevisiontransformer_amd.weights import (make_images, make_std_vit_params, make_t2t_params,
                                               make_vit_params, t2t_config, vit_config)
from oracle import t2t_ref, vit_ref
from tests.test_gpu_features import _gate as _row_gate

pytestmark = pytest.mark.gpu

F32_TOL = 1e-3                      # x max(1, max|golden|)
BF16_ABS, BF16_COS = 3e-2, 0.9995   # tests/test_gpu_model.py
PRUNED = "layerwise_h1-d0.5_h3-d1.0_h2-d0.3"
TAIL, TAIL_AND_FULL = 1, 3


def _ref_case(batch):
    geo = dict(dim=192, depth=2, heads=3, mlp_dim=768, image_size=32, patch_size=16, num_classes=16)
    cfg = vit_config(192, 2, 3, 768, image_size=32, patch_size=16, num_classes=16)
    params = make_vit_params(cfg, seed=61)
    img = make_images(batch, seed=62, image_size=32)
    trace = {}
    logits = vit_ref.vit_forward(params, cfg, img, trace=trace)
    make = lambda dtype, lanes, gpu: ViT(dtype=dtype, weights=params, device=gpu,  # noqa: E731
                                         max_batch=batch, lanes=lanes, **geo)
    return dict(make=make, img=img, logits=logits, tokens=trace["l1.ffn"])


def _std_case(dim, heads, depth, image_size, patch_size, batch, seed):
    cfg = vit_config(dim, depth, heads, 4 * dim, image_size=image_size, patch_size=patch_size,
                     num_classes=16)
    params = make_std_vit_params(cfg, seed=seed)
    img = make_images(batch, seed=seed + 1, image_size=image_size)
    make = lambda dtype, lanes, gpu: StandardViT(  # noqa: E731
        image_size=image_size, patch_size=patch_size, num_classes=16, dim=dim, depth=depth,
        heads=heads, dtype=dtype, weights=params, device=gpu, max_batch=batch, lanes=lanes)
    return dict(make=make, img=img, logits=vit_ref.std_vit_forward(params, cfg, img, eps=1e-6))


def _pruned_case():
    geo = dict(dim=192, depth=3, heads=3, mlp_dim=768, image_size=64, patch_size=16, num_classes=16)
    cfg = pruned_config(PRUNED, **geo)
    assert (cfg.heads[-1], cfg.ffn[-1]) != (cfg.heads[0], cfg.ffn[0])
    params = make_vit_params(cfg, seed=65)
    img = make_images(3, seed=66, image_size=64)
    make = lambda dtype, lanes, gpu: ViT_Pruned(  # noqa: E731
        prune_encoding=PRUNED, dtype=dtype, weights=params, device=gpu, max_batch=3, lanes=lanes,
        **geo)
    return dict(make=make, img=img, logits=vit_ref.vit_forward(params, cfg, img))


def _t2t_case():
    args = (256, 2, 4, 2)
    cfg = t2t_config(*args)
    params = make_t2t_params(cfg, seed=67)
    img = make_images(2, seed=68, layout="NHWC")
    make = lambda dtype, lanes, gpu: T2T_ViT(  # noqa: E731
        hidden_size=args[0], depth=args[1], num_heads=args[2], mlp_ratio=args[3], dtype=dtype,
        weights=params, device=gpu, max_batch=2, lanes=lanes)
    return dict(make=make, img=img, logits=t2t_ref.t2t_vit_forward(params, cfg, img))


CASES = {
    "ref_192": lambda: _ref_case(130),
    "std_384_224": lambda: _std_case(384, 6, 2, 224, 16, 2, 63),
    "std_1408": lambda: _std_case(1408, 16, 1, 28, 14, 2, 69),
    "pruned": _pruned_case,
    "t2t": _t2t_case,
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Built once (the fp64 reference is shared by both dtypes and every test) and never modified."""
    return CASES[name]()


def _logits_gate(what, got, ref, dtype):
    got = got.double().cpu().numpy()
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, top = np.abs(got - ref).max(), np.abs(ref).max()
    cos = ((got * ref).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(ref, axis=1))).min()
    print(f"CLS-TAIL {what} {dtype}: max-abs {err:.3e} max|golden| {top:.3f} min row cosine {cos:.6f}")
    if dtype == "f32":
        assert err <= F32_TOL * max(1.0, top), f"{what} f32 max-abs {err:.3e} (max|golden| {top:.3f})"
    else:
        assert err <= BF16_ABS and cos >= BF16_COS, f"{what} bf16 max-abs {err:.3e}, min cos {cos:.6f}"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_cls_tail(gpu, name, dtype):
    c = _case(name)
    m = c["make"](dtype, 1, gpu)
    x = torch.from_numpy(c["img"]).to(gpu)
    b = x.shape[0]
    plain = m(x).clone()
    assert m.tail_mode() == TAIL
    _logits_gate(name, plain, c["logits"], dtype)
    # pooled alone and an attention-map call do not need the last token map
    pooled = m.features(x)["pooled"]
    assert m.tail_mode() == TAIL
    am = m.attention_maps(x, blocks=(-1,), logits=True)
    assert m.tail_mode() == TAIL
    assert torch.equal(am["logits"], plain)
    # tokens, or a tap on the last block, do: the full-row block runs too, and the CLS rows,
    # pooled and the logits are still the tail's
    feat = m.features(x, tokens=True, logits=True)
    assert m.tail_mode() == TAIL_AND_FULL
    assert torch.equal(feat["logits"], plain)
    assert torch.equal(feat["pooled"], feat["tokens"][:, 0])
    assert torch.equal(feat["pooled"], pooled)
    tap = m.features(x, taps=(-1,), logits=True)
    assert m.tail_mode() == TAIL_AND_FULL
    assert torch.equal(tap["logits"], plain) and torch.equal(tap["pooled"], pooled)
    if m.num_blocks > 1:  # a tap on an earlier block alone leaves the last block to the tail
        m.features(x, taps=(0,))
        assert m.tail_mode() == TAIL
    # a plain forward after a features forward is unchanged
    assert torch.equal(m(x), plain) and m.tail_mode() == TAIL
    # a batch permutation permutes the logits
    perm = torch.from_numpy(np.roll(np.arange(b), 1)).to(gpu)
    assert torch.equal(m(x[perm].contiguous()), plain[perm])
    # a captured graph replays to the eager logits
    out = torch.empty_like(plain)
    m.capture_graph(x, out)
    m.replay_graph()
    torch.cuda.synchronize()
    assert torch.equal(out, plain)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_image_alone_is_the_image_in_a_batch(gpu, dtype):
    """B = 1, 3 and 130 on one handle: the M = B launches take the 128x128 kernel at every batch
    (one row tile, then a partial second one at 130), so an image's logits do not depend on the
    batch it came in. The full-size GEMMs of this 5-token model stay on the 128x128 kernel too at
    these batches (at most 36 tiles of 128x128: never more rounds than 256x256 tiles)."""
    c = _case("ref_192")
    m = c["make"](dtype, 1, gpu)
    x = torch.from_numpy(c["img"]).to(gpu)
    full = m(x).clone()
    for lo, n in ((0, 1), (129, 1), (64, 3)):
        part = m(x[lo:lo + n].contiguous())
        assert m.tail_mode() == TAIL
        assert torch.equal(part, full[lo:lo + n]), (lo, n)
        _logits_gate(f"ref_192 B={n}", part, c["logits"][lo:lo + n], dtype)


def test_full_row_block_undisturbed(gpu):
    """B = 130, bf16: every row of `tokens` from a features forward, the 520 non-CLS rows among
    them, passes the per-row gate of tests/test_gpu_features.py against the fp64 oracle."""
    c = _case("ref_192")
    m = c["make"]("bf16", 1, gpu)
    x = torch.from_numpy(c["img"]).to(gpu)
    tokens = m.features(x, tokens=True)["tokens"]
    assert m.tail_mode() == TAIL_AND_FULL
    _row_gate("ref_192 non-CLS tokens", tokens[:, 1:], c["tokens"][:, 1:], "bf16")
    _row_gate("ref_192 CLS tokens", tokens[:, :1], c["tokens"][:, :1], "bf16")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_two_lane_handle(gpu, dtype):
    """Lane children have their own workspace (the tail's hidden rows among it): a two-lane plain
    forward runs the tail in every lane and gives the logits of its own features forward."""
    c = _case("pruned")
    m2 = c["make"](dtype, 2, gpu)
    assert m2.lanes() == 2
    x = torch.from_numpy(c["img"]).to(gpu)
    plain = m2(x).clone()
    assert m2.tail_mode() == TAIL
    _logits_gate("pruned, two lanes", plain, c["logits"], dtype)
    feat = m2.features(x, tokens=True, logits=True)
    assert m2.tail_mode() == TAIL_AND_FULL
    assert torch.equal(feat["logits"], plain)
    assert torch.equal(feat["pooled"], feat["tokens"][:, 0])
    assert torch.equal(m2(x), plain)
