"""GPU: per-neuron FFN activation statistics (include/evt_ffn_stats.h; ffn_stats_kernel in
csrc/ffn_stats.hip).

Op level (evt_ffn_neuron_stats): the inputs, fp64 reference and derived bound of
tests/_ffn_stats_probes.py at every width and token count of that module, f32 and bf16. Each case
prints its error as a fraction of the bound (FFNSTATS-OP ... frac); a fraction above 1 is a finding,
the bound is not fitted to the kernel. The matrix has a pitch of F rounded up to 64 with NaN in the
padding columns and sits inside a NaN-filled allocation; the output is a NaN-filled guarded buffer:
a padding column that leaks in, a read that matters past the rows, an unwritten slot or a write
outside [B, F, 4] shows. Exact: `ints` / `onehot` / `signs` to 1 ulp of the correctly rounded
quotient, max_abs bitwise. Bitwise: two launches in a row, image 0 alone against inside the batch.

Model level (ffn_stats / ffn_stats_into / evt_forward_ffn_stats): every block, the last one
included, of a small ViT, a pruned ViT with ragged FFN widths (230 of a 256-column pitch), a
STANDARD ViT and a T2T-ViT-7 against `ffn_stats_reference` of the fp64 CPU forward's hidden
activations gelu(LN2(x) @ fc1_w + fc1_b). Gates per statistic, on max-abs / max(1, max|reference|)
for f32 (<= 1e-3, the project's f32 gate) and max-abs / max|reference| for bf16
(<= BF16_REL_GATE = twice BF16_REL_MEASURED, the practice of tests/test_gpu_features.py).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import Uint8Images, _lib
from edgevisiontransformer_amd.modeling.models.ffn_stats import FFN_STATS, ffn_stats_reference
from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer
from edgevisiontransformer_amd.modeling.models.t2t_vit import T2T_ViT
from edgevisiontransformer_amd.modeling.models.vit import StandardViT, ViT, ViT_Pruned
from edgevisiontransformer_amd.weights import (make_images, make_std_vit_params, make_swin_params,
                                               make_t2t_params, make_vit_params, swin_config)
from oracle import t2t_ref, vit_ref
from tests import _ffn_stats_probes as fp
from tests._ops import TDT, _p, _s
from tests.test_gpu_features import _buffer, _untouched, _written

pytestmark = pytest.mark.gpu
PAD = 64  # NaN elements before and after the hidden matrix
PRUNED = "layerwise_h1-d0.5_h3-d1.0_h2-d0.3"
# bf16, model level: the largest max-abs / max|reference| per statistic (FFN_STATS order) over the
# four models and all their blocks against the fp64 forward, measured on an MI355X (the
# FFNSTATS-MODEL-MAX lines; all four on T2T-ViT-7: blocks 4, 6, 4 and 6; the small ViT reaches
# 3.2e-3 / 3.0e-3 / 3.5e-3 / 6.3e-3, the pruned ViT 4.8e-3 / 4.7e-3 / 5.5e-3 / 5.9e-3, the STANDARD
# ViT 2.5e-3 / 2.0e-3 / 3.4e-3 / 4.6e-3; f32: at most 8.8e-7 against its gate of 1e-3). What it measures is the bf16 forward's error in the hidden activations
# (bf16 weights, activations and the stored value's own 2^-9 rounding), not the reduction's, which
# the op-level bound holds to (T + 16) 2^-24. The gate is twice that (other seeds and widths).
BF16_REL_MEASURED = (5.107e-3, 4.709e-3, 5.876e-3, 6.702e-3)
BF16_REL_GATE = tuple(2 * v for v in BF16_REL_MEASURED)


# ---- op level -------------------------------------------------------------------------------------
def _embed(t, gpu):
    """t on the device inside a NaN-filled allocation, 16-byte aligned: (holder, view)."""
    flat = torch.full((t.numel() + 2 * PAD,), float("nan"), dtype=t.dtype, device=gpu)
    flat[PAD:PAD + t.numel()] = t.reshape(-1).to(gpu)
    return flat, flat[PAD:PAD + t.numel()].view(t.shape)


def _stats(dtype, hidden, gpu):
    """evt_ffn_neuron_stats of float32 host values [b, t, f] -> [b, f, 4] on the device; the rows
    have a pitch of f rounded up to 64, the padding columns hold NaN."""
    b, t, f = hidden.shape
    ld = -(-f // 64) * 64
    rows = torch.full((b * t, ld), float("nan"), dtype=torch.float32)
    rows[:, :f] = torch.from_numpy(np.array(hidden)).reshape(b * t, f)
    holder, dev = _embed(rows.to(TDT[dtype]), gpu)
    flat, out = _buffer((b, f, 4), gpu)
    _lib.check(_lib.load_library().evt_ffn_neuron_stats(_lib.DTYPE[dtype], _p(dev), ld, b, t, f,
                                                        _p(out), _s()))
    torch.cuda.synchronize()
    assert _written(flat), "NaN left in the output (padding or a read past the rows) or guard hit"
    del holder
    return out


def _within_ulp(got32, ref, what):
    want = fp.exact_quotient(ref)
    assert (np.abs(got32.astype(np.float64) - want.astype(np.float64))
            <= np.spacing(np.abs(want)).astype(np.float64)).all(), what


def _op_case(dtype, t, f, gpu, b=fp.B):
    worst = 0.0
    for kind in fp.INPUTS:
        c = fp.case(kind, t, f, dtype, b)
        out = _stats(dtype, c["hidden"], gpu)
        got32 = out.cpu().numpy()
        got = got32.astype(np.float64)
        err = np.abs(got - c["ref"])
        frac = (err / c["bound"]).max(axis=(0, 1))
        print(f"FFNSTATS-OP {dtype} T{t} F{f} {kind}: frac "
              + " ".join(f"{s} {v:.3f}" for s, v in zip(FFN_STATS, frac))
              + " | err " + " ".join(f"{e:.2e}" for e in err.max(axis=(0, 1))))
        worst = max(worst, frac.max())
        assert np.array_equal(got32[..., 3], c["ref"][..., 3].astype(np.float32)), f"{kind}: max_abs"
        if kind != "normal":  # every sum is exact in fp32: the correctly rounded quotient to 1 ulp
            _within_ulp(got32[..., :3], c["ref"][..., :3], f"{kind}: not the rounded quotient")
        if kind == "signs" and t % 2 == 0:
            assert (got32[..., 0] == 0).all(), "signs: the mean of an even T is exactly 0"
        assert (err <= c["bound"]).all(), f"{kind}: {frac} of the bound"
        assert torch.equal(_stats(dtype, c["hidden"], gpu), out), "second launch differs"
        if b > 1:
            alone = _stats(dtype, c["hidden"][:1], gpu)
            assert torch.equal(alone[0], out[0]), "image 0 alone differs from inside the batch"
    print(f"FFNSTATS-OP-MAX {dtype} T{t} F{f}: {worst:.3f}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("f", fp.WIDTHS)
def test_ffn_stats_op(gpu, f, dtype):
    for t in fp.TOKENS:
        _op_case(dtype, t, f, gpu)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ffn_stats_op_4096(gpu, dtype):
    b, t, f = fp.BIG
    _op_case(dtype, t, f, gpu, b=b)


def test_ffn_stats_op_errors_write_nothing(gpu):
    lib = _lib.load_library()
    h = torch.zeros((2 * 5, 64), dtype=torch.bfloat16, device=gpu)
    flat, out = _buffer((2, 60, 4), gpu)
    P = ctypes.c_void_p
    ok = dict(dtype=1, h=h.data_ptr(), ld=64, B=2, T=5, F=60, out=out.data_ptr())
    for kw in (dict(dtype=2), dict(h=None), dict(out=None), dict(B=0), dict(T=0), dict(T=4097),
               dict(F=0), dict(F=65), dict(ld=68), dict(h=h.data_ptr() + 8),
               dict(out=out.data_ptr() + 4)):
        a = {**ok, **kw}
        rc = lib.evt_ffn_neuron_stats(a["dtype"], P(a["h"]), a["ld"], a["B"], a["T"], a["F"],
                                      P(a["out"]), _s())
        assert rc == _lib.EVT_EINVAL and b"ffn_neuron_stats" in lib.evt_last_error(), kw
    torch.cuda.synchronize()
    assert _untouched(flat)


# ---- model level ----------------------------------------------------------------------------------
def std_vit_hidden(params, cfg, img, eps=1e-6, dtype=np.float64):
    """([hidden activations [B, T, F_i] of every block], logits) of the STANDARD forward, written
    after oracle/vit_ref.py's std_vit_forward (x + attn(LN1 x), x + mlp(LN2 x), QKV bias, erf GELU,
    eps 1e-6, final LayerNorm); tests/test_ffn_stats_host.py checks the logits against it."""
    P = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}
    x = vit_ref.patchify_nchw(np.asarray(img, dtype=dtype), cfg.patch_size) @ P["patch_w"] + P["patch_b"]
    b = x.shape[0]
    x = np.concatenate([np.broadcast_to(P["cls"], (b, 1, cfg.dim)), x], axis=1) + P["pos"]
    erf = np.vectorize(math.erf, otypes=[np.float64])
    hidden = []
    for i in range(cfg.depth):
        h, hk = cfg.heads[i], cfg.head_dim[i]
        y = vit_ref.layer_norm(x, P[f"l{i}.ln1_g"], P[f"l{i}.ln1_b"], eps)
        n = y.shape[1]
        qkv = (y @ P[f"l{i}.qkv_w"] + P[f"l{i}.qkv_b"]).reshape(b, n, 3, h, hk).transpose(2, 0, 3, 1, 4)
        att = vit_ref.softmax(np.einsum("bhid,bhjd->bhij", qkv[0], qkv[1]) * hk ** -0.5)
        o = np.einsum("bhij,bhjd->bhid", att, qkv[2]).transpose(0, 2, 1, 3).reshape(b, n, h * hk)
        x = x + o @ P[f"l{i}.out_w"] + P[f"l{i}.out_b"]
        y = vit_ref.layer_norm(x, P[f"l{i}.ln2_g"], P[f"l{i}.ln2_b"], eps)
        z = y @ P[f"l{i}.fc1_w"] + P[f"l{i}.fc1_b"]
        z = 0.5 * z * (1.0 + erf(z / math.sqrt(2.0)))
        hidden.append(z)
        x = x + z @ P[f"l{i}.fc2_w"] + P[f"l{i}.fc2_b"]
    x = vit_ref.layer_norm(x[:, 0], P["norm_g"], P["norm_b"], eps)
    return hidden, x @ P["head_w"] + P["head_b"]


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


# (constructor, image size, layout, parameter seed: the constructor's `seed`)
MODELS = {"vit": (_vit, 32, "NCHW", 71), "pruned": (_pruned, 64, "NCHW", 72),
          "std": (_std, 64, "NCHW", 73), "t2t": (_t2t, 224, "NHWC", 74)}


def _host_image(name, batch=2):
    _, size, layout, _ = MODELS[name]
    kw = {} if layout == "NCHW" else {"layout": "NHWC"}
    return make_images(batch, seed=75, image_size=size, **kw)


_REFERENCES = {}


def _reference(name, cfg):
    """[fp64 [B, F_i, 4] per block] of the model `name` (configuration `cfg`) on its image:
    computed once on the CPU, shared by the f32 and bf16 tests, read-only."""
    if name in _REFERENCES:
        return _REFERENCES[name]
    img, seed = _host_image(name), MODELS[name][3]
    if name == "std":
        hidden, _ = std_vit_hidden(make_std_vit_params(cfg, seed=seed), cfg, img)
    else:
        trace = {}
        if name == "t2t":
            params = make_t2t_params(cfg, seed=seed)
            t2t_ref.t2t_vit_forward(params, cfg, img, trace=trace)
        else:
            params = make_vit_params(cfg, seed=seed)
            vit_ref.vit_forward(params, cfg, img, trace=trace)
        P = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
        hidden = [vit_ref.gelu(trace[f"l{i}.ln2"] @ P[f"l{i}.fc1_w"] + P[f"l{i}.fc1_b"])
                  for i in range(cfg.depth)]
    out = [ffn_stats_reference(h) for h in hidden]
    for a in out:
        a.setflags(write=False)
    _REFERENCES[name] = tuple(out)
    return _REFERENCES[name]


def _run(m, x, blocks=None, logits=True, pooled=False):
    """ffn_stats_into on guarded buffers -> {"stats": [...], "logits", "pooled"}."""
    b, gpu = x.shape[0], m.device
    blocks = list(range(m.num_blocks)) if blocks is None else list(blocks)
    bufs = [_buffer((b, m.ffn_stats_shape(i)[0], 4), gpu) for i in blocks]
    extra = {}
    if logits:
        extra["logits"] = _buffer((b, m.num_classes), gpu)
    if pooled:
        extra["pooled"] = _buffer((b, m.feature_dim), gpu)
    m.ffn_stats_into(x, blocks=blocks, stat_tensors=[v for _, v in bufs],
                     **{k: v for k, (_, v) in extra.items()})
    torch.cuda.synchronize()
    for flat, _ in bufs + list(extra.values()):
        assert _written(flat), "NaN left in an output or guard words overwritten"
    out = {k: v for k, (_, v) in extra.items()}
    out["stats"] = [v for _, v in bufs]
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(MODELS))
def test_model_ffn_stats(gpu, name, dtype):
    m = MODELS[name][0](dtype, 1, gpu)
    x = torch.from_numpy(_host_image(name)).to(gpu)
    plain = m(x).clone()
    pooled = m.forward_features(x).clone()
    out = _run(m, x, pooled=True)  # every block, the last one included
    assert torch.equal(out["logits"], plain) and torch.equal(out["pooled"], pooled)
    assert torch.equal(m(x), plain)  # a plain forward after a statistics forward is unchanged
    ref = _reference(name, m.cfg)
    worst = np.zeros(4)
    for i, (s, r) in enumerate(zip(out["stats"], ref)):
        neurons, tokens = m.ffn_stats_shape(i)
        assert tuple(s.shape) == (x.shape[0], neurons, 4) == r.shape
        got = s.double().cpu().numpy()
        assert np.isfinite(got).all() and (got[..., 1:] >= 0).all()
        err = np.abs(got - r).max(axis=(0, 1))
        top = np.abs(r).max(axis=(0, 1))
        rel = err / (np.maximum(top, 1.0) if dtype == "f32" else top)
        print(f"FFNSTATS-MODEL {name} {dtype} block {i} F{neurons} T{tokens}: rel "
              + " ".join(f"{n_} {v:.3e}" for n_, v in zip(FFN_STATS, rel))
              + " | max|ref| " + " ".join(f"{v:.3f}" for v in top))
        worst = np.maximum(worst, rel)
    print(f"FFNSTATS-MODEL-MAX {name} {dtype}: " + " ".join(f"{v:.3e}" for v in worst))
    gate = (1e-3,) * 4 if dtype == "f32" else BF16_REL_GATE
    assert all(w <= g for w, g in zip(worst, gate)), f"{worst} against the gates {gate}"
    if name == "pruned":
        assert [t.shape[1] for t in out["stats"]] == [384, 768, 230]  # ragged; 230 < its pitch 256
        assert [m.ffn_stats_shape(i) for i in range(3)] == [(384, 17), (768, 17), (230, 17)]
    # a second call, a single late block and the order given; no logits: no classifier head
    late = m.ffn_stats(x, blocks=(-1, 0))
    assert list(late) == ["stats"]
    assert torch.equal(late["stats"][0], out["stats"][-1]) and torch.equal(late["stats"][1], out["stats"][0])
    # the last block alone, with logits and pooled: still bitwise the plain forward's
    last = _run(m, x, blocks=(m.num_blocks - 1,), pooled=True)
    assert torch.equal(last["logits"], plain) and torch.equal(last["pooled"], pooled)
    assert torch.equal(last["stats"][0], out["stats"][-1])
    # a batch permutation permutes the statistics
    flip = _run(m, x.flip(0).contiguous(), logits=False)
    assert all(torch.equal(u.flip(0), v) for u, v in zip(flip["stats"], out["stats"]))
    # lanes = 2: the call runs as one lane on the handle's own workspace
    m2 = MODELS[name][0](dtype, 2, gpu)
    assert m2.lanes() == 2
    out2 = _run(m2, x, logits=False)
    assert all(torch.equal(u, v) for u, v in zip(out2["stats"], out["stats"]))


def test_ffn_stats_numpy_and_uint8(gpu):
    m = _vit("bf16", 1, gpu)
    rng = np.random.default_rng(7)
    u8 = Uint8Images(torch.from_numpy(rng.integers(0, 256, (2, 32, 32, 3), dtype=np.uint8)).to(gpu))
    want = _run(m, u8.to_float("nchw"))
    got = _run(m, u8)
    assert torch.equal(got["logits"], want["logits"])
    assert all(torch.equal(u, v) for u, v in zip(got["stats"], want["stats"]))
    host = m.ffn_stats(u8.to_float("nchw").cpu().numpy(), logits=True)
    assert isinstance(host["logits"], np.ndarray) and len(host["stats"]) == m.num_blocks
    assert all(np.array_equal(u, v.cpu().numpy()) for u, v in zip(host["stats"], want["stats"]))


def test_ffn_stats_under_profile_counts_as_head(gpu):
    """A profiled statistics forward adds EVT_PROF_HEAD launches only, one per requested block, the
    last block included (its full-row and tail launches share their role's event pair, as in a
    features forward with a tap on it); the next plain forward's role counts are unchanged."""
    m = _vit("bf16", 1, gpu)
    x = torch.from_numpy(_host_image("vit")).to(gpu)
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

    others = lambda c: [v for i, v in enumerate(c) if i != head]  # noqa: E731
    plain = launches(lambda: m(x))
    one = launches(lambda: _run(m, x, blocks=(1,)))
    two = launches(lambda: _run(m, x, blocks=(0, 1)))
    assert one[head] == plain[head] + 1 and two[head] == plain[head] + 2
    assert others(one) == others(two) == others(plain)
    tapped = launches(lambda: m.features(x, taps=(-1,), logits=True))
    every = launches(lambda: _run(m, x))
    assert every[head] == plain[head] + 3
    assert others(every) == others(tapped) == others(plain)
    assert launches(lambda: m(x)) == plain


def test_ffn_stats_errors(gpu):
    """Swin and "mx8" raise ValueError; every documented C-level error is EVT_EINVAL with a message
    before any launch: nothing is written."""
    cfg = swin_config("tiny", image_size=56, window_size=7, depths=(2, 2), num_heads=(3, 6),
                      num_classes=11)
    s = SwinTransformer(img_size=56, patch_size=cfg.patch_size, num_classes=11,
                        embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
                        window_size=7, dtype="bf16", weights=make_swin_params(cfg, seed=3),
                        device=gpu, max_batch=1, lanes=1)
    xs = torch.zeros((1, 3, 56, 56), device=gpu)
    with pytest.raises(ValueError, match="fused MLP"):
        s.ffn_stats(xs)
    m8 = ViT(dim=128, depth=2, heads=2, mlp_dim=256, image_size=32, patch_size=16, num_classes=16,
             dtype="mx8", device=gpu, max_batch=1, lanes=1)
    x8 = torch.zeros((1, 3, 32, 32), device=gpu)
    with pytest.raises(ValueError, match="mx8"):
        m8.ffn_stats(x8)
    lib = _lib.load_library()
    m = _vit("bf16", 1, gpu)
    x = torch.from_numpy(_host_image("vit")).to(gpu)
    flats = [_buffer((2, 768, 4), gpu) for _ in range(3)]
    lflat, logits = _buffer((2, m.num_classes), gpu)

    def call(model, img, blocks, ptrs, batch=2, feat=None, n_blocks=None, null_arrays=False):
        a = _lib.evt_ffn_stats_args()
        a.n_blocks = len(blocks) if n_blocks is None else n_blocks
        keep = ((ctypes.c_int32 * max(1, len(blocks)))(*blocks),
                (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs))
        if not null_arrays:
            a.blocks, a.stats = keep
        args = _lib.evt_image_args()
        args.data = img.data_ptr()
        rc = lib.evt_forward_ffn_stats(ctypes.c_void_p(model._handle), ctypes.byref(args), batch,
                                       ctypes.byref(feat) if feat is not None else None,
                                       ctypes.byref(a), _s())
        return rc, lib.evt_last_error()

    ptr = [v.data_ptr() for _, v in flats]
    feat = _lib.evt_features_args()
    feat.logits = logits.data_ptr()
    bad = {
        "swin": dict(model=s, img=xs, blocks=[0], ptrs=ptr[:1], batch=1),
        "mx8": dict(model=m8, img=x8, blocks=[0], ptrs=ptr[:1], batch=1),
        "n_blocks 65": dict(blocks=[0], ptrs=ptr[:1], n_blocks=65),
        "n_blocks negative": dict(blocks=[0], ptrs=ptr[:1], n_blocks=-1),
        "nothing requested": dict(blocks=[], ptrs=[]),
        "NULL arrays": dict(blocks=[0], ptrs=ptr[:1], null_arrays=True),
        "NULL stats pointer": dict(blocks=[0, 1], ptrs=[ptr[0], None]),
        "block out of range": dict(blocks=[0, 3], ptrs=ptr[:2]),
        "block negative": dict(blocks=[-1], ptrs=ptr[:1]),
        "blocks not increasing": dict(blocks=[1, 0], ptrs=ptr[:2]),
        "blocks repeated": dict(blocks=[1, 1], ptrs=ptr[:2]),
        "stats misaligned": dict(blocks=[0], ptrs=[ptr[0] + 4]),
        "batch over max_batch": dict(blocks=[0], ptrs=ptr[:1], batch=3),
        "batch 0": dict(blocks=[0], ptrs=ptr[:1], batch=0),
        "with feat, a bad block": dict(blocks=[5], ptrs=ptr[:1], feat=feat),
    }
    for what, kw in bad.items():
        kw = {"model": m, "img": x, **kw}
        rc, msg = call(**kw)
        assert rc == _lib.EVT_EINVAL and msg, what
    h = ctypes.c_int()
    r = ctypes.byref(h)
    for model, blk in ((s, 0), (m8, 0), (m, 3), (m, -1)):
        assert lib.evt_ffn_stats_shape(ctypes.c_void_p(model._handle), blk, r, r) == _lib.EVT_EINVAL
    nn, tt = ctypes.c_int(), ctypes.c_int()
    _lib.check(lib.evt_ffn_stats_shape(ctypes.c_void_p(m._handle), 2, ctypes.byref(nn), ctypes.byref(tt)))
    assert (nn.value, tt.value) == (768, 65) == m.ffn_stats_shape(2)
    torch.cuda.synchronize()
    assert all(_untouched(f) for f, _ in flats) and _untouched(lflat)
    # the Python layer's own checks
    for kw in (dict(blocks=(3,)), dict(blocks=(0, 0))):
        with pytest.raises(ValueError):
            m.ffn_stats(x, **kw)
    with pytest.raises(ValueError):
        m.ffn_stats_into(x, blocks=(0,), stat_tensors=(torch.empty((2, 767, 4), device=gpu),))
