"""GPU: attention rollout (include/evt_rollout.h; head_mean_kernel in csrc/attn_maps.hip, the
matrix step in csrc/rollout.hip).

Op level (evt_attention_rollout_step): a 3-step chain on the cases, inputs, fp64 reference and the
derived bound of tests/_rollout_probes.py. Each case prints its error as a fraction of the bound
(ROLLOUT-OP ... frac); a fraction above 1 is a finding, the bound is not fitted to the kernels.
qkv sits inside a NaN-filled allocation, r_out and the scratch in NaN-filled guarded buffers of
exactly the stated size, so a read past the rows, or a write outside [B, N, N] or outside the
stated scratch size, shows. Bitwise: head-major against token-major, image 0 alone against inside
the batch, two launches in a row. (No H = 1 against H = 3 check: the mean of three equal heads is
not exact, tests/_rollout_probes.py.)

Model level (attention_rollout / attention_rollout_into / evt_forward_rollout): a small ViT, a
pruned ViT with ragged heads, a STANDARD ViT and a T2T-ViT-7 against `rollout_reference` in fp64 on
`attention_maps(queries="all")` of the same image; the gate is twice the op-level bound (both
sides carry the probabilities' error), evaluated on those maps.

Largest fraction of the bound measured on an MI355X over every op-level case: see DESIGN.md,
attention rollout.
"""
import ctypes

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import Uint8Images, _lib
from edgevisiontransformer_amd.modeling.models.rollout import rollout_reference
from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer
from edgevisiontransformer_amd.modeling.models.vit import ViT
from edgevisiontransformer_amd.weights import make_swin_params, swin_config
from tests import _rollout_probes as rp
from tests._ops import TDT, _p, _s
from tests.test_gpu_attention_maps import _op_inputs, _probs
from tests.test_gpu_features import _buffer, _written
from tests.test_gpu_head_stats import MODELS, _embed, _image

pytestmark = pytest.mark.gpu


# ---- op level -------------------------------------------------------------------------------------
def _chain(dtype, rows, b, n, h, hd, gpu, head_major=False, steps=rp.STEPS):
    """`steps` calls of evt_attention_rollout_step on float32 host rows [b n, 3 h hd] per step ->
    the rollout after every step, [b, n, n] device tensors."""
    lib, outs, r_in = _lib.load_library(), [], None
    for s in range(steps):
        qkv = torch.from_numpy(np.array(rows[s])).to(TDT[dtype])  # a copy: the rows are read-only
        if head_major:  # [B][H][q | k | v][N][64]
            qkv = qkv.view(b, n, 3, h, 64).permute(0, 3, 2, 1, 4).contiguous()
            ldq, sb, sh, ko = 64, 3 * h * n * 64, 3 * n * 64, n * 64
        else:
            ldq, sb, sh, ko = qkv.shape[1], 0, 0, 0
        holder, dev = _embed(qkv, gpu)
        flat, out = _buffer((b, n, n), gpu)
        sflat, scratch = _buffer((b, n, n), gpu)
        _lib.check(lib.evt_attention_rollout_step(
            _lib.DTYPE[dtype], _p(dev), ldq, sb, sh, ko, b, n, h, hd, rp.ap.scale_of(hd),
            _p(r_in) if r_in is not None else None, _p(out), _p(scratch), b * n * n * 4, _s()))
        torch.cuda.synchronize()
        assert _written(flat), "NaN left in r_out (or read past qkv / r_in) or guard words overwritten"
        assert _written(sflat), "NaN left in the scratch or a write past its stated size"
        del holder
        outs.append(out)
        r_in = out
    return outs


def _check(got, ref, bound, what):
    """finite, in [0, 1] and row sums of 1 up to the bound, error inside the bound -> the fraction."""
    assert np.isfinite(got).all(), what
    assert (got >= 0).all() and (got <= 1 + bound).all(), what
    assert (np.abs(got.sum(-1) - 1.0) <= bound.sum(-1) + 1e-15).all(), f"{what}: row sums"
    frac = (np.abs(got - ref) / bound).max()
    return frac


def _op_case(dtype, n, hd, gpu, b=rp.B, h=rp.H, bitwise=False):
    worst = 0.0
    for kind in rp.INPUTS:
        c = rp.case(kind, n, hd, dtype, b, h)
        outs = _chain(dtype, c["rows"], b, n, h, hd, gpu)
        fracs = []
        for s, out in enumerate(outs):
            got = out.double().cpu().numpy()
            fracs.append(_check(got, c["ref"][s], c["bound"][s], f"{kind} step {s}"))
            if kind == "uniform":  # 2^-L I + (1 - 2^-L) / N J
                want = rp.uniform_closed_form(n, s + 1)
                assert (np.abs(got - want) <= c["bound"][s] + 1e-15).all(), f"uniform step {s}"
        err = np.abs(outs[-1].double().cpu().numpy() - c["ref"][-1]).max()
        print(f"ROLLOUT-OP {dtype} N{n} hd{hd} H{h} {kind}: frac "
              + " ".join(f"{f:.3f}" for f in fracs) + f" | err {err:.2e}")
        worst = max(worst, max(fracs))
        assert max(fracs) <= 1, f"{kind}: {fracs} of the bound"
        if bitwise:
            again = _chain(dtype, c["rows"], b, n, h, hd, gpu)
            assert all(torch.equal(u, v) for u, v in zip(again, outs)), "second run differs"
            if b > 1:
                alone = _chain(dtype, [r[:n] for r in c["rows"]], 1, n, h, hd, gpu)
                assert all(torch.equal(u[0], v[0]) for u, v in zip(alone, outs)), \
                    "image 0 alone differs from inside the batch"
            if dtype == "bf16" and hd == 64:
                hm = _chain(dtype, c["rows"], b, n, h, hd, gpu, head_major=True)
                assert all(torch.equal(u, v) for u, v in zip(hm, outs)), \
                    "head-major differs from token-major"
    print(f"ROLLOUT-OP-MAX {dtype} N{n} hd{hd}: {worst:.3f}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("n", rp.NS)
def test_rollout_op(gpu, n, dtype):
    _op_case(dtype, n, 64, gpu, bitwise=True)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", rp.HD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_rollout_op_head_sizes(gpu, case, dtype):
    n, hd = case
    _op_case(dtype, n, hd, gpu)


@pytest.mark.parametrize("n", rp.BIG)
def test_rollout_op_big(gpu, n):
    _op_case("bf16", n, 64, gpu, b=1, h=1)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", [(2, 3, 65, 64), (1, 3, 197, 64), (1, 2, 65, 80), (1, 2, 17, 20)],
                         ids=lambda c: "x".join(map(str, c)))
def test_head_mean_is_head_ordered_sum_of_export(gpu, case, dtype):
    """head_mean_kernel and attn_probs_kernel form their probabilities with one score core
    (csrc/attn_scores.h), so the head mean (the scratch of a step with r_in = NULL holds Abar,
    include/evt_rollout.h) is, bit for bit, the fp32 sum of the exported maps in head order from
    0, times fl(1 / H)."""
    b, h, n, hd = case
    qkv, _ = _op_inputs(b, h, n, hd, dtype, 1.0)
    scale = rp.ap.scale_of(hd)  # one scale for both entry points
    p = _probs(dtype, qkv, b, n, h, hd, n, gpu, scale=scale).cpu().numpy()
    holder, dev = _embed(qkv, gpu)
    flat, out = _buffer((b, n, n), gpu)
    sflat, scratch = _buffer((b, n, n), gpu)
    _lib.check(_lib.load_library().evt_attention_rollout_step(
        _lib.DTYPE[dtype], _p(dev), qkv.shape[1], 0, 0, 0, b, n, h, hd, scale, None,
        _p(out), _p(scratch), b * n * n * 4, _s()))
    torch.cuda.synchronize()
    assert _written(flat) and _written(sflat)
    del holder
    acc = np.zeros((b, n, n), np.float32)
    for i in range(h):
        acc = acc + p[:, i]
    want = acc * (np.float32(1) / np.float32(h))
    assert want.dtype == np.float32 and np.array_equal(scratch.cpu().numpy(), want)


def test_rollout_op_rejects_in_place(gpu):
    n = 5
    c = rp.case("normal", n, 64, "bf16", 1, 1)
    qkv = torch.from_numpy(np.array(c["rows"][0])).to(torch.bfloat16).to(gpu)
    flat, r = _buffer((1, n, n), gpu)
    _, scratch = _buffer((1, n, n), gpu)
    rc = _lib.load_library().evt_attention_rollout_step(
        _lib.DTYPE["bf16"], _p(qkv), qkv.shape[1], 0, 0, 0, 1, n, 1, 64, 0.125, _p(r), _p(r),
        _p(scratch), n * n * 4, _s())
    torch.cuda.synchronize()
    assert rc == _lib.EVT_EINVAL and torch.isnan(r).all()  # nothing launched


# ---- model level ----------------------------------------------------------------------------------
def _run(m, x, queries="all", start=0, logits=False, pooled=False):
    """attention_rollout_into on guarded buffers -> {"rollout", "logits", "pooled"}."""
    b, gpu = x.shape[0], m.device
    t, _ = m.rollout_shape()
    bufs = {"out": _buffer((b, t, t) if queries == "all" else (b, t), gpu)}
    if logits:
        bufs["logits"] = _buffer((b, m.num_classes), gpu)
    if pooled:
        bufs["pooled"] = _buffer((b, m.feature_dim), gpu)
    m.attention_rollout_into(x, queries=queries, start=start, **{k: v for k, (_, v) in bufs.items()})
    torch.cuda.synchronize()
    for flat, _ in bufs.values():
        assert _written(flat), "NaN left in an output or guard words overwritten"
    out = {k: v for k, (_, v) in bufs.items()}
    out["rollout"] = out.pop("out")
    return out


def _map_terms(p):
    """x_i [b, T] of one block (tests/_rollout_probes.py) from its maps [b, h, T, T] alone: the
    scores of a row are only defined up to a constant, so |y| and |y - y_max| are both taken as
    ln c_i - ln p (the row maximum at 0), as the head-statistics model test does."""
    n = p.shape[-1]
    nkb = -(-n // 64) if n > 64 else 0
    cmax = p.max(-1, keepdims=True)
    with np.errstate(divide="ignore"):
        dy = np.where(p > 0, np.log(cmax) - np.log(np.where(p > 0, p, 1.0)), 0.0)
    eps = (rp.U * (2 + 3 * nkb + 13 * dy)).max(-1).max(-2)
    return rp.step_terms(eps, p.shape[1], n)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(MODELS))
def test_model_rollout(gpu, name, dtype):
    m = MODELS[name][0](dtype, 1, gpu)
    x = _image(name, gpu)
    t, depth = m.rollout_shape()
    assert depth == m.num_blocks
    plain = m(x).clone()
    pooled = m.forward_features(x).clone()
    out = _run(m, x, logits=True, pooled=True)
    assert torch.equal(out["logits"], plain) and torch.equal(out["pooled"], pooled)
    assert torch.equal(m(x), plain)  # a plain forward after a rollout forward is unchanged
    maps = [a.double().cpu().numpy()
            for a in m.attention_maps(x, blocks=range(depth), queries="all")["maps"]]
    if name == "pruned":
        assert len({a.shape[1] for a in maps}) > 1  # ragged heads
    xs = [_map_terms(a) for a in maps]
    worst = 0.0
    for start in sorted({0, 1, depth - 1}):
        got_t = out["rollout"] if start == 0 else _run(m, x, start=start)["rollout"]
        got = got_t.double().cpu().numpy()
        ref = rollout_reference(maps, start=start)
        bound = 2 * rp.chain_bound(ref, xs[start:])
        frac = _check(got, ref, bound, f"{name} start {start}")
        print(f"ROLLOUT-MODEL {name} {dtype} start {start}: frac of 2 x bound {frac:.3f}")
        worst = max(worst, frac)
        assert frac <= 1, f"start {start}: {frac} of twice the op-level bound"
        cls = _run(m, x, queries="cls", start=start)["rollout"]
        assert torch.equal(cls, got_t[:, 0]), "queries='cls' is not row 0 of queries='all'"
    print(f"ROLLOUT-MODEL-MAX {name} {dtype}: {worst:.3f}")
    # an image's result is the same alone and at batch position 1
    alone = _run(m, x[1:2])["rollout"]
    assert torch.equal(alone[0], out["rollout"][1])
    # the allocating form, a second call
    again = m.attention_rollout(x, queries="all", logits=True)
    assert sorted(again) == ["logits", "rollout"]
    assert torch.equal(again["rollout"], out["rollout"]) and torch.equal(again["logits"], plain)
    # lanes = 2: the call runs as one lane on the handle's own workspace
    m2 = MODELS[name][0](dtype, 2, gpu)
    assert m2.lanes() == 2
    assert torch.equal(_run(m2, x)["rollout"], out["rollout"])


def test_rollout_numpy_and_uint8(gpu):
    m = MODELS["vit"][0]("bf16", 1, gpu)
    rng = np.random.default_rng(7)
    u8 = Uint8Images(torch.from_numpy(rng.integers(0, 256, (2, 32, 32, 3), dtype=np.uint8)).to(gpu))
    want = _run(m, u8.to_float("nchw"), logits=True)
    got = _run(m, u8, logits=True)
    assert torch.equal(got["logits"], want["logits"]) and torch.equal(got["rollout"], want["rollout"])
    host = m.attention_rollout(u8.to_float("nchw").cpu().numpy(), logits=True)
    assert isinstance(host["logits"], np.ndarray) and host["rollout"].shape == (2, 65)
    assert np.array_equal(host["rollout"], want["rollout"][:, 0].cpu().numpy())
    # the scratch is allocated once per (batch, queries) and kept on the model
    keys = set(m._rollout_scratch_cache)
    assert keys == {(2, _lib.ROLLOUT_ALL), (2, _lib.ROLLOUT_CLS)}
    ptr = m._rollout_scratch_cache[(2, _lib.ROLLOUT_CLS)].data_ptr()
    m.attention_rollout(u8)
    assert m._rollout_scratch_cache[(2, _lib.ROLLOUT_CLS)].data_ptr() == ptr


def test_rollout_under_profile_counts_as_head(gpu):
    """A profiled rollout forward adds EVT_PROF_HEAD launches only (a head mean and a step per
    block from `start` on); the next plain forward's role counts are unchanged."""
    m = MODELS["vit"][0]("bf16", 1, gpu)
    x = _image("vit", gpu)
    lib = _lib.load_library()
    head = _lib.PROF_ROLES.index("head")
    us = (ctypes.c_float * len(_lib.PROF_ROLES))()
    n = (ctypes.c_int * len(_lib.PROF_ROLES))()

    def launches(run):
        _lib.check(lib.evt_model_profile(ctypes.c_void_p(m._handle), 1))
        run()
        torch.cuda.synchronize()
        _lib.check(lib.evt_model_profile_read(ctypes.c_void_p(m._handle), us, n))
        _lib.check(lib.evt_model_profile(ctypes.c_void_p(m._handle), 0))
        return list(n)
    plain = launches(lambda: m(x))
    full = launches(lambda: _run(m, x, logits=True))
    late = launches(lambda: _run(m, x, start=2, logits=True))
    assert full[head] > plain[head] and late[head] > plain[head]
    assert full[head] - plain[head] == 3 * (late[head] - plain[head])  # three blocks against one
    for got in (full, late):
        assert [v for i, v in enumerate(got) if i != head] == [v for i, v in enumerate(plain) if i != head]
    assert launches(lambda: m(x)) == plain


def test_rollout_errors(gpu):
    """Swin and "mx8" raise ValueError; every documented C-level error is EVT_EINVAL with a message
    before any launch: nothing is written."""
    cfg = swin_config("tiny", image_size=56, window_size=7, depths=(2, 2), num_heads=(3, 6),
                      num_classes=11)
    s = SwinTransformer(img_size=56, patch_size=cfg.patch_size, num_classes=11,
                        embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
                        window_size=7, dtype="bf16", weights=make_swin_params(cfg, seed=3),
                        device=gpu, max_batch=1, lanes=1)
    xs = torch.zeros((1, 3, 56, 56), device=gpu)
    with pytest.raises(ValueError, match="window_attention_maps"):
        s.attention_rollout(xs)
    m8 = ViT(dim=128, depth=2, heads=2, mlp_dim=256, image_size=32, patch_size=16, num_classes=16,
             dtype="mx8", device=gpu, max_batch=1, lanes=1)
    x8 = torch.zeros((1, 3, 32, 32), device=gpu)
    with pytest.raises(ValueError, match="mx8"):
        m8.attention_rollout(x8)
    lib = _lib.load_library()
    m = MODELS["vit"][0]("bf16", 1, gpu)
    x = _image("vit", gpu)
    t, depth = m.rollout_shape()
    flat, out = _buffer((2, t, t), gpu)
    need = ctypes.c_size_t()
    _lib.check(lib.evt_rollout_scratch_bytes(ctypes.c_void_p(m._handle), 2, _lib.ROLLOUT_ALL,
                                             ctypes.byref(need)))
    assert 2 * t * t * 4 <= need.value <= 3 * (2 * t * t * 4 + 256)  # at most three buffers
    scratch = torch.zeros(need.value, dtype=torch.uint8, device=gpu)
    tt, dd = ctypes.c_int(), ctypes.c_int()
    _lib.check(lib.evt_rollout_shape(ctypes.c_void_p(m._handle), ctypes.byref(tt), ctypes.byref(dd)))
    assert (tt.value, dd.value) == (t, depth)

    def raw(model=m, img=x, batch=2, null_ro=False, **kw):
        a = _lib.evt_rollout_args()
        a.start, a.mode, a.out = 0, _lib.ROLLOUT_ALL, out.data_ptr()
        a.scratch, a.scratch_bytes = scratch.data_ptr(), need.value
        for k, v in kw.items():
            setattr(a, k, v)
        args = _lib.evt_image_args()
        args.data = img.data_ptr()
        rc = lib.evt_forward_rollout(ctypes.c_void_p(model._handle), ctypes.byref(args), batch, None,
                                     None if null_ro else ctypes.byref(a),
                                     ctypes.c_void_p(_lib.stream_ptr(gpu)))
        return rc, lib.evt_last_error()

    bad = {
        "NULL ro": dict(null_ro=True), "Swin": dict(model=s, img=xs, batch=1),
        "mx8": dict(model=m8, img=x8, batch=1), "start -1": dict(start=-1),
        "start depth": dict(start=depth), "mode 2": dict(mode=2), "NULL out": dict(out=None),
        "NULL scratch": dict(scratch=None), "out misaligned": dict(out=out.data_ptr() + 4),
        "scratch misaligned": dict(scratch=scratch.data_ptr() + 8),
        "scratch too small": dict(scratch_bytes=need.value - 1), "batch 0": dict(batch=0),
        "batch 3": dict(batch=3),
    }
    for what, kw in bad.items():
        rc, msg = raw(**kw)
        assert rc == _lib.EVT_EINVAL and msg, what
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and not scratch.any(), "a refused call wrote something"
    for model in (s, m8):
        assert lib.evt_rollout_shape(ctypes.c_void_p(model._handle), ctypes.byref(tt),
                                     ctypes.byref(dd)) == _lib.EVT_EINVAL
        assert lib.evt_rollout_scratch_bytes(ctypes.c_void_p(model._handle), 1, 0,
                                             ctypes.byref(need)) == _lib.EVT_EINVAL
    rc, _ = raw()  # and the same arguments untouched run
    torch.cuda.synchronize()
    assert rc == 0 and _written(flat)
