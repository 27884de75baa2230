"""GPU: per-head attention statistics (include/evt_head_stats.h; head_stats_kernel in
csrc/attn_maps.hip).

Op level (evt_attention_head_stats): the cases, inputs, fp64 reference and the derived bound of
tests/_head_stats_probes.py. Each case prints its error as a fraction of the bound
(HEADSTATS-OP ... frac); a fraction above 1 is a finding, the bound is not fitted to the kernel.
qkv sits inside a NaN-filled allocation and the output in a NaN-filled guarded buffer, so a read
past the rows or a write outside [B, H, 4] shows. Bitwise: head-major against token-major, image 0
alone against inside the batch, two launches in a row.

Model level (head_stats / head_stats_into / evt_forward_head_stats): every block, the last one
included, of a small ViT, a pruned ViT with ragged heads, a STANDARD ViT and a T2T-ViT-7 against
`head_stats_reference` in fp64 on `attention_maps(queries="all")` of the same image; the gate is
twice the op-level bound (both sides carry the probabilities' error), evaluated on those maps.

Largest fraction of the bound measured on an MI355X over every op-level case: see DESIGN.md, head
statistics.
"""
import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import Uint8Images, _lib
from edgevisiontransformer_amd.modeling.models.head_stats import (HEAD_STATS, head_stats_reference,
                                                                  patch_distances)
from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer
from edgevisiontransformer_amd.modeling.models.t2t_vit import T2T_ViT
from edgevisiontransformer_amd.modeling.models.vit import StandardViT, ViT, ViT_Pruned
from edgevisiontransformer_amd.weights import make_images, make_swin_params, swin_config
from tests import _head_stats_probes as hp
from tests._ops import TDT, _p, _s
from tests.test_gpu_attention_maps import _op_inputs, _probs
from tests.test_gpu_features import _buffer, _written

pytestmark = pytest.mark.gpu
PAD = 64  # NaN elements before and after qkv
PRUNED = "layerwise_h1-d0.5_h3-d1.0_h2-d0.3"


# ---- op level -------------------------------------------------------------------------------------
def _embed(t, gpu):
    """t on the device inside a NaN-filled allocation, 16-byte aligned: (holder, view)."""
    flat = torch.full((t.numel() + 2 * PAD,), float("nan"), dtype=t.dtype, device=gpu)
    flat[PAD:PAD + t.numel()] = t.reshape(-1).to(gpu)
    return flat, flat[PAD:PAD + t.numel()].view(t.shape)


def _stats(dtype, rows, b, n, h, hd, prefix, gw, gpu, head_major=False):
    """evt_attention_head_stats of float32 host rows [b n, 3 h hd] -> [b, h, 4] on the device."""
    qkv = torch.from_numpy(np.array(rows)).to(TDT[dtype])  # a copy: the shared rows are read-only
    if head_major:  # [B][H][q | k | v][N][64]
        qkv = qkv.view(b, n, 3, h, 64).permute(0, 3, 2, 1, 4).contiguous()
        ldq, sb, sh, ko = 64, 3 * h * n * 64, 3 * n * 64, n * 64
    else:
        ldq, sb, sh, ko = qkv.shape[1], 0, 0, 0
    holder, dev = _embed(qkv, gpu)
    flat, out = _buffer((b, h, 4), gpu)
    _lib.check(_lib.load_library().evt_attention_head_stats(
        _lib.DTYPE[dtype], _p(dev), ldq, sb, sh, ko, b, n, h, hd, hp.ap.scale_of(hd), prefix, gw,
        _p(out), _s()))
    torch.cuda.synchronize()
    assert _written(flat), "NaN left in the output (or read past qkv) or guard words overwritten"
    del holder
    return out


def _in_range(got, n):
    assert np.isfinite(got).all()
    assert (got[..., 0] > 0).all() and (got[..., 0] <= 1).all()
    assert (got[..., 1] >= 0).all() and (got[..., 1] <= np.log(n) * (1 + 2.0 ** -22)).all()
    assert (got[..., 2] >= 0).all()
    assert (got[..., 3] >= 0).all() and (got[..., 3] <= 1).all()


def _op_case(dtype, n, prefix, gw, hd, gpu, b=hp.B, h=hp.H, bitwise=False):
    worst = 0.0
    for kind in hp.INPUTS:
        c = hp.case(kind, n, prefix, gw, hd, dtype, b, h)
        out = _stats(dtype, c["rows"], b, n, h, hd, prefix, gw, gpu)
        got = out.double().cpu().numpy()
        err = np.abs(got - c["ref"])
        frac = (err / c["bound"]).max(axis=(0, 1))
        print(f"HEADSTATS-OP {dtype} N{n} prefix{prefix} grid{gw} hd{hd} {kind}: frac "
              + " ".join(f"{s} {f:.3f}" for s, f in zip(HEAD_STATS, frac))
              + " | err " + " ".join(f"{e:.2e}" for e in err.max(axis=(0, 1))))
        worst = max(worst, frac.max())
        _in_range(got, n)
        if kind == "uniform":  # exactly uniform rows: 1 / N to 2 ulp
            one = np.float32(1.0) / np.float32(n)
            assert (np.abs(got[..., 0] - 1.0 / n) <= 2 * np.spacing(one)).all(), got[..., 0]
        if kind == "perm":     # the mean d(i, pi(i)) over the patch queries, to the 2^-12 leak
            d = patch_distances(n - prefix, gw)
            for i in range(b):
                for j in range(h):
                    pi = c["pi"][i, j]
                    q = np.arange(prefix, n)
                    ok = pi[q] >= prefix
                    want = d[(q - prefix)[ok], (pi[q] - prefix)[ok]].sum() / (n - prefix)
                    assert abs(got[i, j, 2] - want) <= 2.0 ** -12 * d.max() + c["bound"][i, j, 2]
        assert (err <= c["bound"]).all(), f"{kind}: {frac} of the bound"
        if bitwise:
            assert torch.equal(_stats(dtype, c["rows"], b, n, h, hd, prefix, gw, gpu), out), \
                "second launch differs"
            if b > 1:
                alone = _stats(dtype, c["rows"][:n], 1, n, h, hd, prefix, gw, gpu)
                assert torch.equal(alone[0], out[0]), "image 0 alone differs from inside the batch"
            if dtype == "bf16" and hd == 64:
                hm = _stats(dtype, c["rows"], b, n, h, hd, prefix, gw, gpu, head_major=True)
                assert torch.equal(hm, out), "head-major differs from token-major"
    print(f"HEADSTATS-OP-MAX {dtype} N{n} hd{hd}: {worst:.3f}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", hp.CASES, ids=lambda c: "x".join(map(str, c)))
def test_head_stats_op(gpu, case, dtype):
    n, prefix, gw = case
    _op_case(dtype, n, prefix, gw, 64, gpu, bitwise=True)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", hp.HD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_head_stats_op_head_sizes(gpu, case, dtype):
    n, prefix, gw, hd = case
    _op_case(dtype, n, prefix, gw, hd, gpu)


def test_head_stats_op_4096(gpu):
    n, prefix, gw = hp.BIG
    _op_case("bf16", n, prefix, gw, 64, gpu, b=1, h=1)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", [(2, 3, 65, 1, 8, 64), (1, 2, 197, 1, 14, 64), (1, 2, 65, 1, 8, 80)],
                         ids=lambda c: "x".join(map(str, c)))
def test_confidence_is_mean_row_max_of_export(gpu, case, dtype):
    """head_stats_kernel and attn_probs_kernel run one pass 1 (csrc/attn_scores.h), so the
    confidence is bitwise the mean row maximum of the exported map: the maximum's own term is
    2^0 / l, so max_j p_ij is the kernel's 1 / l_i exactly, and a float64 sum of at most 4096 fp32
    values in [2^-12, 1] is exact in any order."""
    b, h, n, prefix, gw, hd = case
    qkv, _ = _op_inputs(b, h, n, hd, dtype, 1.0)
    scale = hp.ap.scale_of(hd)  # the scale _stats hands over
    p = _probs(dtype, qkv, b, n, h, hd, n, gpu, scale=scale).cpu().numpy()
    stats = _stats(dtype, qkv.float().numpy(), b, n, h, hd, prefix, gw, gpu).cpu().numpy()
    want = (p.max(-1).astype(np.float64).sum(-1) / n).astype(np.float32)
    assert np.array_equal(stats[..., 0], want)


# ---- model level ----------------------------------------------------------------------------------
def _vit(dtype, lanes, gpu):
    return ViT(dim=192, depth=3, heads=3, mlp_dim=768, image_size=32, patch_size=4, num_classes=16,
               dtype=dtype, seed=71, device=gpu, max_batch=2, lanes=lanes)


def _pruned(dtype, lanes, gpu):
    return ViT_Pruned(prune_encoding=PRUNED, dim=192, depth=3, heads=3, mlp_dim=768, image_size=64,
                      patch_size=16, num_classes=16, dtype=dtype, seed=72, device=gpu, max_batch=2,
                      lanes=lanes)


def _std(dtype, lanes, gpu):
    return StandardViT(dim=192, depth=2, heads=3, image_size=64, patch_size=8, num_classes=16,
                       dtype=dtype, seed=73, device=gpu, max_batch=2, lanes=lanes)


def _t2t(dtype, lanes, gpu):  # T2T-ViT-7 at 224 px, the smallest size the suite runs T2T-ViT at
    return T2T_ViT(hidden_size=256, depth=7, num_heads=4, mlp_ratio=2, num_classes=16, dtype=dtype,
                   seed=74, device=gpu, max_batch=2, lanes=lanes)


MODELS = {"vit": (_vit, 32, "NCHW"), "pruned": (_pruned, 64, "NCHW"), "std": (_std, 64, "NCHW"),
          "t2t": (_t2t, 224, "NHWC")}


def _image(name, gpu, batch=2):
    _, size, layout = MODELS[name]
    kw = {} if layout == "NCHW" else {"layout": "NHWC"}
    return torch.from_numpy(make_images(batch, seed=75, image_size=size, **kw)).to(gpu)


def _run(m, x, blocks=None, logits=True, pooled=False):
    """head_stats_into on guarded buffers -> {"stats": [...], "logits", "pooled"}."""
    b, gpu = x.shape[0], m.device
    blocks = list(range(m.num_blocks)) if blocks is None else list(blocks)
    bufs = [_buffer((b, m.head_stats_shape(i)[0], 4), gpu) for i in blocks]
    extra = {}
    if logits:
        extra["logits"] = _buffer((b, m.num_classes), gpu)
    if pooled:
        extra["pooled"] = _buffer((b, m.feature_dim), gpu)
    m.head_stats_into(x, blocks=blocks, stat_tensors=[v for _, v in bufs],
                      **{k: v for k, (_, v) in extra.items()})
    torch.cuda.synchronize()
    for flat, _ in bufs + list(extra.values()):
        assert _written(flat), "NaN left in an output or guard words overwritten"
    out = {k: v for k, (_, v) in extra.items()}
    out["stats"] = [v for _, v in bufs]
    return out


def _map_bound(p, prefix, gw):
    """The op-level bound of tests/_head_stats_probes.py from a map [b, h, T, T] alone: y - y_max =
    ln p - ln c_i; |y| is not known from p, so it is taken as |ln p - ln c_i| too (the scores of a
    row are only defined up to a constant; the row maximum at 0)."""
    b, h, n, _ = p.shape
    nkb = -(-n // 64) if n > 64 else 0
    cmax = p.max(-1, keepdims=True)
    with np.errstate(divide="ignore"):
        dy = np.where(p > 0, np.log(cmax) - np.log(np.where(p > 0, p, 1.0)), 0.0)
    eps = (hp.U * (2 + 3 * nkb + 13 * dy)).max(-1)                     # [b, h, T]
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = -np.where(p > 0, p * np.log(p), 0.0).sum(-1)
    lnl = -np.log(cmax[..., 0])
    d = (p[:, :, prefix:, prefix:] * patch_distances(n - prefix, gw)).sum(-1)
    cm = p[:, :, prefix:, :prefix].sum(-1)
    ref = head_stats_reference(p, prefix=prefix, grid_w=gw)
    bound = np.zeros_like(ref)
    ep = eps[:, :, prefix:]
    bound[..., 0] = (2 * eps * cmax[..., 0]).mean(-1)
    bound[..., 1] = (2 * eps * (ent + 1) + 2 * hp.U * lnl
                     + (n + 16) * hp.U * np.maximum(ent - lnl, 0)).mean(-1) + hp.U * np.abs(ref[..., 1])
    bound[..., 2] = ((2 * ep + (n + 16) * hp.U) * d).mean(-1) + hp.U * np.abs(ref[..., 2])
    bound[..., 3] = ((2 * ep + (n + 16) * hp.U) * cm).mean(-1) + hp.U * np.abs(ref[..., 3])
    return ref, bound + hp.ap.TINY


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(MODELS))
def test_model_head_stats(gpu, name, dtype):
    m = MODELS[name][0](dtype, 1, gpu)
    x = _image(name, gpu)
    plain = m(x).clone()
    pooled = m.forward_features(x).clone()
    out = _run(m, x, pooled=True)
    assert torch.equal(out["logits"], plain) and torch.equal(out["pooled"], pooled)
    assert torch.equal(m(x), plain)  # a plain forward after a statistics forward is unchanged
    maps = m.attention_maps(x, blocks=range(m.num_blocks), queries="all")["maps"]
    worst = 0.0
    for i, (s, a) in enumerate(zip(out["stats"], maps)):
        heads, tokens, prefix, gw = m.head_stats_shape(i)
        assert tuple(s.shape) == (x.shape[0], heads, 4) and tuple(a.shape)[1:] == (heads, tokens, tokens)
        got = s.double().cpu().numpy()
        _in_range(got, tokens)
        ref, bound = _map_bound(a.double().cpu().numpy(), prefix, gw)
        frac = (np.abs(got - ref) / (2 * bound)).max(axis=(0, 1))
        print(f"HEADSTATS-MODEL {name} {dtype} block {i}: frac of 2 x bound "
              + " ".join(f"{n_} {f:.3f}" for n_, f in zip(HEAD_STATS, frac)))
        worst = max(worst, frac.max())
        assert (frac <= 1).all(), f"block {i}: {frac} of twice the op-level bound"
    print(f"HEADSTATS-MODEL-MAX {name} {dtype}: {worst:.3f}")
    if name == "pruned":
        assert len({t.shape[1] for t in out["stats"]}) > 1  # ragged heads
    # a second call, a single late block and the order given
    late = m.head_stats(x, blocks=(-1, 0))
    assert list(late) == ["stats"]
    assert torch.equal(late["stats"][0], out["stats"][-1]) and torch.equal(late["stats"][1], out["stats"][0])
    # lanes = 2: the call runs as one lane on the handle's own workspace
    m2 = MODELS[name][0](dtype, 2, gpu)
    assert m2.lanes() == 2
    out2 = _run(m2, x, logits=False)
    assert all(torch.equal(u, v) for u, v in zip(out2["stats"], out["stats"]))


def test_head_stats_numpy_and_uint8(gpu):
    m = _vit("bf16", 1, gpu)
    rng = np.random.default_rng(7)
    u8 = Uint8Images(torch.from_numpy(rng.integers(0, 256, (2, 32, 32, 3), dtype=np.uint8)).to(gpu))
    want = _run(m, u8.to_float("nchw"))
    got = _run(m, u8)
    assert torch.equal(got["logits"], want["logits"])
    assert all(torch.equal(u, v) for u, v in zip(got["stats"], want["stats"]))
    host = m.head_stats(u8.to_float("nchw").cpu().numpy(), logits=True)
    assert isinstance(host["logits"], np.ndarray) and len(host["stats"]) == m.num_blocks
    assert all(np.array_equal(u, v.cpu().numpy()) for u, v in zip(host["stats"], want["stats"]))


def test_head_stats_family_errors(gpu):
    cfg = swin_config("tiny", image_size=56, window_size=7, depths=(2, 2), num_heads=(3, 6),
                      num_classes=11)
    s = SwinTransformer(img_size=56, patch_size=cfg.patch_size, num_classes=11,
                        embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
                        window_size=7, dtype="bf16", weights=make_swin_params(cfg, seed=3),
                        device=gpu, max_batch=1, lanes=1)
    x = torch.zeros((1, 3, 56, 56), device=gpu)
    with pytest.raises(ValueError, match="windowed"):
        s.head_stats(x)
    m8 = ViT(dim=128, depth=2, heads=2, mlp_dim=256, image_size=32, patch_size=16, num_classes=16,
             dtype="mx8", device=gpu, max_batch=1, lanes=1)
    with pytest.raises(ValueError, match="mx8"):
        m8.head_stats(torch.zeros((1, 3, 32, 32), device=gpu))
    # the C ABI refuses both too, before any launch
    import ctypes
    lib = _lib.load_library()
    out = torch.zeros((1, 3, 4), device=gpu)
    a = _lib.evt_head_stats_args()
    a.n_blocks = 1
    a.blocks = (ctypes.c_int32 * 1)(0)
    a.stats = (ctypes.c_void_p * 1)(out.data_ptr())
    for model, img in ((s, x), (m8, torch.zeros((1, 3, 32, 32), device=gpu))):
        args = _lib.evt_image_args()
        args.data = img.data_ptr()
        assert lib.evt_forward_head_stats(ctypes.c_void_p(model._handle), ctypes.byref(args), 1, None,
                                          ctypes.byref(a), None) == _lib.EVT_EINVAL
        h = ctypes.c_int()
        r = ctypes.byref(h)
        assert lib.evt_head_stats_shape(ctypes.c_void_p(model._handle), 0, r, r, r, r) == _lib.EVT_EINVAL
