"""GPU: Swin window attention maps (include/evt_window_attention.h; csrc/attn_maps.hip).

Op level (evt_window_attention_probs): q and k rounded to the dtype first, the reference the fp64
softmax of those same values with the bias and the region mask (tests/_window_probs_ref.py), at
the shapes where the kernels can go wrong: 2 x 2 windows with and without the shift (all four mask
types), a single window, 3 x 3 windows (interior ones), both window sizes, a row stride past 3 C
and scores past +-88. Three probes pin what random inputs blur: the bias table lookup (q = k = 0,
a table that is distinct per relative offset and head), the region mask (the set of exact zeros)
and the gather geometry (one-hot q / k rows numbered by raster token). Outputs are NaN-prefilled
with guard words; qkv sits inside a NaN-filled allocation, so a read past its rows shows as NaN.

Model level (window_attention_maps / window_attention_maps_into / evt_forward_window_attention):
every block of a fused stage-1 model (bf16, C = 96), the same in f32, an unfused window-7 model
and a window-12 model against the fp64 oracle, and the bitwise properties of the call.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import Uint8Images, _lib
from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer
from edgevisiontransformer_amd.modeling.models.vit import ViT
from edgevisiontransformer_amd.weights import (make_images, make_swin_params, make_vit_params,
                                               swin_config, vit_config)
from oracle import swin_ref
from tests._ops import TDT, _p, _s
from tests._window_probs_ref import bias_and_mask, model_window_probs, window_probs
from tests.test_gpu_features import GUARD, _buffer, _cos_rows, _untouched, _written

pytestmark = pytest.mark.gpu

# Op level, against the fp64 reference on the same (rounded) q and k, over every case and probe
# below, measured on an MI355X on the first run of this file: largest max-abs error and largest
# |sum_k p - 1| of a row, per dtype. The gates are twice that (other seeds and shapes; the
# arithmetic is deterministic, so not device differences). The max-abs maxima are the x6 cases'
# (scores past +-88: the rounding of the log2-domain score is 1e-5 there; with unit-variance q and
# k the largest are 2.868e-7 f32 and 1.457e-7 bf16). The f32 row-sum maximum is the geometry
# probe's: the thread-per-query fp32 kernel adds a row's terms in key order, and 48 terms of
# e^-11.3 added one by one to a sum near 1 each lose the same fraction of an ulp (random inputs:
# at most 6.107e-7); the bf16 kernel sums four keys per lane first (at most 2.261e-7).
OP_ERR_MEASURED = {"f32": 8.073e-6, "bf16": 2.764e-6}
OP_ROWSUM_MEASURED = {"f32": 2.062e-6, "bf16": 2.261e-7}
# Model level, bf16: largest max-abs error of a map against the fp64 oracle over every case and
# block below, measured on the same run: 2.314e-3 (w7_c64 block 1; the fused stage-1 blocks of
# tiny_56: 9.979e-4 and 1.924e-3; lowest row cosine 0.999954, gate 0.9995; f32: at most 2.049e-7,
# gate 1e-3). The gate is twice the measured value.
MODEL_BF16_ERR_MEASURED = 2.314e-3
PAD = 64  # NaN elements before and after qkv


# ---- op level ---------------------------------------------------------------------------------
OP_CASES = [  # (B, R, w, H, shift, extra columns of a qkv row)
    (2, 14, 7, 3, 0, 0), (2, 14, 7, 3, 3, 0), (2, 7, 7, 1, 0, 0), (2, 21, 7, 2, 3, 0),
    (2, 24, 12, 2, 0, 0), (2, 24, 12, 2, 6, 0), (2, 12, 12, 4, 0, 0), (2, 14, 7, 3, 3, 16),
]
PROBE_CASES = [(2, 14, 7, 3, 0), (2, 14, 7, 3, 3), (2, 24, 12, 2, 0), (2, 24, 12, 2, 6)]
_id = lambda c: "x".join(map(str, c))  # noqa: E731


def _embed(t, gpu):
    """t on the device inside a NaN-filled allocation, 16-byte aligned: (holder, view)."""
    flat = torch.full((t.numel() + 2 * PAD,), float("nan"), dtype=t.dtype, device=gpu)
    flat[PAD:PAD + t.numel()] = t.reshape(-1).to(gpu)
    return flat, flat[PAD:PAD + t.numel()].view(t.shape)


@functools.lru_cache(maxsize=None)
def _op_inputs(B, R, w, H, shift, extra, dtype, gain):
    """(qkv [B*R*R, 3*32*H + extra] rounded to the dtype, on the host; rpb [(2w-1)^2, H] fp32;
    the fp64 reference [B, nW, H, N, N])."""
    rng = np.random.default_rng(10000 * R + 100 * shift + 10 * H + w + extra)
    qkv = torch.from_numpy(rng.standard_normal((B * R * R, 96 * H + extra)).astype(np.float32) * gain)
    qkv = qkv.to(TDT[dtype])
    rpb = (rng.standard_normal(((2 * w - 1) ** 2, H)) * 0.5).astype(np.float32)
    return qkv, rpb, window_probs(qkv.double().numpy(), rpb, R, w, H, shift)


def _probs(dtype, qkv, rpb, B, R, w, H, shift, gpu):
    """evt_window_attention_probs into a guarded NaN-filled buffer -> [B, nW, H, N, N]."""
    holder, dev = _embed(qkv, gpu)
    table = torch.from_numpy(np.ascontiguousarray(rpb, dtype=np.float32)).to(gpu)
    flat, out = _buffer((B, (R // w) ** 2, H, w * w, w * w), gpu)
    _lib.check(_lib.load_library().evt_window_attention_probs(
        _lib.DTYPE[dtype], _p(dev), qkv.shape[1], _p(table), B, R, w, 32 * H, H, shift, _p(out),
        _s()))
    torch.cuda.synchronize()
    assert _written(flat), "NaN left in the output (or read past qkv) or guard words overwritten"
    del holder
    return out


def _gate(what, dtype, out, ref):
    assert bool(torch.isfinite(out).all()) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    got = out.double().cpu().numpy()
    err = np.abs(got - ref).max()
    rs = np.abs(got.sum(-1) - 1.0).max()
    print(f"WINMAPS-OP {what} {dtype}: max-abs {err:.3e} rowsum {rs:.3e}")
    assert err <= 2 * OP_ERR_MEASURED[dtype], f"max-abs {err:.3e}"
    assert rs <= 2 * OP_ROWSUM_MEASURED[dtype], f"|sum p - 1| {rs:.3e}"
    return got


def _mask_probe(got, R, w, H, shift):
    """The exact zeros are the pairs in different regions: per window, the oracle's shift_mask."""
    _, masked = bias_and_mask(np.zeros(((2 * w - 1) ** 2, H)), R, w, H, shift)
    assert np.array_equal(got == 0.0, np.broadcast_to(masked[None, :, None], got.shape))
    nwx = R // w
    for win in range(nwx * nwx):  # the three masked window types, and type 0
        edge = shift > 0 and (win // nwx == nwx - 1 or win % nwx == nwx - 1)
        assert bool(masked[win].any()) == edge, win
    if not shift:
        assert not (got == 0.0).any()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", OP_CASES, ids=_id)
def test_window_attention_probs(gpu, case, dtype):
    B, R, w, H, shift, extra = case
    qkv, rpb, ref = _op_inputs(B, R, w, H, shift, extra, dtype, 1.0)
    out = _probs(dtype, qkv, rpb, B, R, w, H, shift, gpu)
    got = _gate(_id(case), dtype, out, ref)
    _mask_probe(got, R, w, H, shift)
    assert torch.equal(_probs(dtype, qkv, rpb, B, R, w, H, shift, gpu), out), "second launch differs"
    perm = torch.from_numpy(np.roll(np.arange(B), 1))  # a permuted batch: the output, permuted
    qp = qkv.view(B, R * R, -1)[perm].reshape(B * R * R, -1).contiguous()
    assert torch.equal(_probs(dtype, qp, rpb, B, R, w, H, shift, gpu), out[perm.to(gpu)])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", [(2, 14, 7, 3, 3, 0), (2, 24, 12, 2, 6, 0)], ids=_id)
def test_window_attention_probs_large_scores(gpu, case, dtype):
    """q and k scaled by 6: the scores reach past +-88, where exp without the max subtraction
    overflows fp32. Same gate."""
    B, R, w, H, shift, extra = case
    qkv, rpb, ref = _op_inputs(B, R, w, H, shift, extra, dtype, 6.0)
    x = qkv.double().numpy().reshape(B, R * R, 3, H, 32)
    s = np.einsum("bihd,bjhd->bhij", x[:, :, 0], x[:, :, 1]) * 32 ** -0.5
    assert s.max() > 88.0 and s.min() < -88.0
    _gate(_id(case) + " x6", dtype, _probs(dtype, qkv, rpb, B, R, w, H, shift, gpu), ref)


@pytest.mark.parametrize("case", [(2, 24, 12, 2, 6, 0), (2, 12, 12, 4, 0, 0)], ids=_id)
def test_window12_store_forms_agree(gpu, monkeypatch, case):
    """The dword store form of the bf16 window-12 kernel (EVT_WINDOW_MAPS_STORE=dword, kept for
    the measurement) writes the bits of the launched 16-byte form."""
    B, R, w, H, shift, extra = case
    qkv, rpb, _ = _op_inputs(B, R, w, H, shift, extra, "bf16", 1.0)
    want = _probs("bf16", qkv, rpb, B, R, w, H, shift, gpu)
    monkeypatch.setenv("EVT_WINDOW_MAPS_STORE", "dword")
    got = _probs("bf16", qkv, rpb, B, R, w, H, shift, gpu)
    monkeypatch.delenv("EVT_WINDOW_MAPS_STORE")
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", PROBE_CASES, ids=_id)
def test_bias_probe(gpu, case, dtype):
    """q = k = 0 and rpb[r, h] = (r + h) / 16 (exact in fp32, distinct per relative offset and
    head): the map is softmax(rpb[rel] + mask); two swapped keys or a wrong head differ by far
    more than the gate."""
    B, R, w, H, shift = case
    qkv = torch.zeros((B * R * R, 96 * H), dtype=TDT[dtype])
    r = np.arange((2 * w - 1) ** 2)
    rpb = ((r[:, None] + np.arange(H)[None, :]) / 16.0).astype(np.float32)
    ref = window_probs(qkv.double().numpy(), rpb, R, w, H, shift)
    got = _gate("bias " + _id(case), dtype, _probs(dtype, qkv, rpb, B, R, w, H, shift, gpu), ref)
    _mask_probe(got, R, w, H, shift)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", PROBE_CASES + [(2, 21, 7, 2, 3)], ids=_id)
def test_geometry_probe(gpu, case, dtype):
    """rpb = 0, q and k rows one_hot(raster token % 32) * 8 in every head: keys of the query's own
    residue outweigh the others by e^(64 * 0.177), so a row gathered from the wrong raster
    position or the wrong shift is visible."""
    B, R, w, H, shift = case
    tok = np.arange(R * R) % 32
    hot = np.zeros((R * R, 32), np.float32)
    hot[np.arange(R * R), tok] = 8.0
    row = np.concatenate([np.tile(hot, (1, H)), np.tile(hot, (1, H)), np.zeros((R * R, 32 * H))], 1)
    qkv = torch.from_numpy(np.tile(row, (B, 1)).astype(np.float32)).to(TDT[dtype])
    rpb = np.zeros(((2 * w - 1) ** 2, H), np.float32)
    ref = window_probs(qkv.double().numpy(), rpb, R, w, H, shift)
    _gate("geometry " + _id(case), dtype, _probs(dtype, qkv, rpb, B, R, w, H, shift, gpu), ref)


# ---- model level ------------------------------------------------------------------------------
def _swin_case(variant, image_size, window, heads, seed, **kw):
    cfg = swin_config(variant, image_size=image_size, window_size=window, depths=(2, 2),
                      num_heads=heads, num_classes=11, **kw)
    params = make_swin_params(cfg, seed=seed)
    img = make_images(2, seed=seed + 1, image_size=image_size)
    trace = {}
    swin_ref.swin_forward(params, cfg, img, trace=trace)
    ref = [model_window_probs(params, cfg, img, i, trace=trace) for i in range(sum(cfg.depths))]
    make = lambda dtype, lanes, gpu: SwinTransformer(  # noqa: E731
        img_size=cfg.image_size, patch_size=cfg.patch_size, num_classes=cfg.num_classes,
        embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
        window_size=cfg.window_size, dtype=dtype, weights=params, device=gpu, max_batch=2,
        lanes=lanes)
    return dict(make=make, img=img, ref=ref, cfg=cfg)


CASES = {
    # stage 1 (C = 96, 3 heads): the fused sublayer in bf16, shifted 2 x 2 windows; stage 2: one
    "tiny_56": lambda: _swin_case("tiny", 56, 7, (3, 6), 21),
    "w7_c64": lambda: _swin_case("tiny", 56, 7, (2, 4), 23, embed_dim=64),  # the unfused w = 7 path
    "base_w12": lambda: _swin_case("base", 96, 12, (4, 8), 25),
}
MODEL_RUNS = [("tiny_56", "bf16"), ("tiny_56", "f32"), ("w7_c64", "bf16"), ("base_w12", "bf16"),
              ("base_w12", "f32")]


@functools.lru_cache(maxsize=None)
def _case(name):
    """Built once (the fp64 reference is shared by both dtypes) and never modified."""
    return CASES[name]()


def _run(m, x, blocks=None, logits=True, pooled=False):
    """window_attention_maps_into on guarded buffers -> {"maps": [...], "logits", "pooled"}."""
    b, gpu = x.shape[0], m.device
    blocks = list(range(m.num_blocks)) if blocks is None else list(blocks)
    bufs = [_buffer(m._window_map_shape(b, i), gpu) for i in blocks]
    extra = {}
    if logits:
        extra["logits"] = _buffer((b, m.num_classes), gpu)
    if pooled:
        extra["pooled"] = _buffer((b, m.feature_dim), gpu)
    m.window_attention_maps_into(x, blocks=blocks, map_tensors=[v for _, v in bufs],
                                 **{k: v for k, (_, v) in extra.items()})
    torch.cuda.synchronize()
    for flat, _ in bufs + list(extra.values()):
        assert _written(flat), "NaN left in an output or guard words overwritten"
    out = {k: v for k, (_, v) in extra.items()}
    out["maps"] = [v for _, v in bufs]
    return out


@pytest.mark.parametrize("name,dtype", MODEL_RUNS, ids=lambda v: str(v))
def test_model_window_maps(gpu, name, dtype):
    c = _case(name)
    m = c["make"](dtype, 1, gpu)
    x = torch.from_numpy(c["img"]).to(gpu)
    plain = m(x).clone()
    pooled = m.forward_features(x).clone()
    full = _run(m, x, pooled=True)
    assert torch.equal(full["logits"], plain) and torch.equal(full["pooled"], pooled)
    assert torch.equal(m(x), plain)  # a plain forward after a maps forward is unchanged
    worst = 0.0
    for i, (a, r) in enumerate(zip(full["maps"], c["ref"])):
        assert tuple(a.shape) == r.shape == (2, *m.window_attn_shape(i), m.window_attn_shape(i)[2])
        assert bool(torch.isfinite(a).all()) and float(a.min()) >= 0.0 and float(a.max()) <= 1.0
        got = a.double().cpu().numpy()
        assert np.array_equal(got == 0.0, r == 0.0), f"block {i}: the masked pairs differ"
        err, cos = np.abs(got - r).max(), _cos_rows(got, r).min()
        print(f"WINMAPS-MODEL {name} {dtype} block {i}: max-abs {err:.3e} min row cosine {cos:.6f}")
        worst = max(worst, err)
        if dtype == "f32":
            assert err <= 1e-3, f"block {i} f32 max-abs {err:.3e}"
        else:
            assert cos >= 0.9995, f"block {i} bf16 row cosine {cos:.6f}"
            assert err <= 2 * MODEL_BF16_ERR_MEASURED, f"block {i} bf16 max-abs {err:.3e}"
    print(f"WINMAPS-MODEL-MAX {name} {dtype}: {worst:.3e}")
    # lanes = 2: the call runs as one lane on the handle's own workspace
    m2 = c["make"](dtype, 2, gpu)
    assert m2.lanes() == 2
    out2 = _run(m2, x, logits=False)
    assert all(torch.equal(u, v) for u, v in zip(out2["maps"], full["maps"]))


@pytest.mark.parametrize("name", ["tiny_56", "base_w12"])
def test_window_maps_exact_properties(gpu, name):
    """bf16 (tiny_56: the fused stage 1): a repeated call, a permuted batch, blocks (0, 1) against
    each alone, window_attention_maps against _into, numpy in / out and the order given."""
    c = _case(name)
    m = c["make"]("bf16", 1, gpu)
    x = torch.from_numpy(c["img"]).to(gpu)
    full = _run(m, x)
    again = _run(m, x)
    assert torch.equal(again["logits"], full["logits"])
    assert all(torch.equal(u, v) for u, v in zip(again["maps"], full["maps"]))
    perm = torch.tensor([1, 0], device=gpu)
    rolled = _run(m, x[perm].contiguous())
    assert all(torch.equal(u, v[perm]) for u, v in zip(rolled["maps"], full["maps"]))
    both = _run(m, x, blocks=(0, 1), logits=False)["maps"]
    for i in (0, 1):
        alone = _run(m, x, blocks=(i,), logits=False)["maps"][0]
        assert torch.equal(alone, both[i]) and torch.equal(alone, full["maps"][i])
    dev = m.window_attention_maps(x)  # defaults: the last block, device tensors
    assert isinstance(dev["maps"][0], torch.Tensor) and list(dev) == ["maps"]
    assert torch.equal(dev["maps"][0], full["maps"][-1])
    host = m.window_attention_maps(c["img"], blocks=(-1, 0), logits=True, pooled=True)
    assert all(isinstance(v, np.ndarray) for v in host["maps"])
    assert np.array_equal(host["maps"][0], full["maps"][-1].cpu().numpy())
    assert np.array_equal(host["maps"][1], full["maps"][0].cpu().numpy())
    assert np.array_equal(host["logits"], full["logits"].cpu().numpy())
    assert np.array_equal(host["pooled"], m.forward_features(c["img"]))
    # the map says which raster tokens it relates: window_token_index is a permutation of them
    idx = m.window_token_index(1)
    assert idx.shape == full["maps"][1].shape[1:4:2] and len(np.unique(idx)) == idx.size


def test_window_maps_with_features_through_feat(gpu):
    """evt_forward_window_attention with a full `feat` (logits, pooled, tokens, a tap): every
    feature output is bitwise that of features(), the map that of a maps-only call."""
    c = _case("tiny_56")
    m = c["make"]("bf16", 1, gpu)
    x = torch.from_numpy(c["img"]).to(gpu)
    want = m.features(x, tokens=True, taps=(1,), logits=True)
    maps = _run(m, x, blocks=(1,), logits=False)["maps"]
    b, (f, t, geo) = x.shape[0], m._feature_geometry()
    bufs = {"logits": _buffer((b, m.num_classes), gpu), "pooled": _buffer((b, f), gpu),
            "tokens": _buffer((b, t, f), gpu), "tap": _buffer((b, *geo[1]), gpu),
            "map": _buffer(m._window_map_shape(b, 1), gpu)}
    feat = _lib.evt_features_args()
    feat.logits, feat.pooled, feat.tokens = (bufs[k][1].data_ptr() for k in ("logits", "pooled", "tokens"))
    feat.n_taps = 1
    feat.tap_blocks = (ctypes.c_int32 * 1)(1)
    feat.taps = (ctypes.c_void_p * 1)(bufs["tap"][1].data_ptr())
    a = _lib.evt_attn_args()
    a.n_maps, a.queries = 1, _lib.ATTN_ALL
    a.blocks = (ctypes.c_int32 * 1)(1)
    a.maps = (ctypes.c_void_p * 1)(bufs["map"][1].data_ptr())
    img = _lib.evt_image_args()
    img.data = x.data_ptr()
    _lib.check(_lib.load_library().evt_forward_window_attention(
        ctypes.c_void_p(m._handle), ctypes.byref(img), b, ctypes.byref(feat), ctypes.byref(a),
        ctypes.c_void_p(_lib.stream_ptr(m.device))))
    torch.cuda.synchronize()
    assert all(_written(flat) for flat, _ in bufs.values())
    for k in ("logits", "pooled", "tokens"):
        assert torch.equal(bufs[k][1], want[k]), k
    assert torch.equal(bufs["tap"][1], want["taps"][0])
    assert torch.equal(bufs["map"][1], maps[0])


def test_window_maps_uint8_images(gpu):
    """A Uint8Images batch gives bitwise the maps and logits of its to_float image."""
    c = _case("tiny_56")
    m = c["make"]("bf16", 1, gpu)
    rng = np.random.default_rng(7)
    u8 = Uint8Images(torch.from_numpy(rng.integers(0, 256, (2, 56, 56, 3), dtype=np.uint8)).to(gpu))
    want = _run(m, u8.to_float("nchw"))
    got = _run(m, u8)
    assert torch.equal(got["logits"], want["logits"])
    assert all(torch.equal(u, v) for u, v in zip(got["maps"], want["maps"]))


def test_window_maps_under_profile_count_as_head(gpu):
    """A profiled maps forward adds EVT_PROF_HEAD launches only (fused block: the QKV GEMM and the
    export; otherwise the export); the next plain forward's role counts are unchanged."""
    c = _case("tiny_56")
    m = c["make"]("bf16", 1, gpu)
    x = torch.from_numpy(c["img"]).to(gpu)
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
    maps = launches(lambda: _run(m, x))
    assert maps[head] == plain[head] + 2 * 2 + 2  # two fused blocks, two GEMM-path blocks
    assert [v for i, v in enumerate(maps) if i != head] == [v for i, v in enumerate(plain) if i != head]
    assert launches(lambda: m(x)) == plain


def _raw(m, x, attn, feat=None, batch=None, img=None):
    lib = _lib.load_library()
    if img is None:
        img = _lib.evt_image_args()
        img.data = x.data_ptr()
    rc = lib.evt_forward_window_attention(ctypes.c_void_p(m._handle), ctypes.byref(img),
                                          x.shape[0] if batch is None else batch,
                                          ctypes.byref(feat) if feat is not None else None,
                                          ctypes.byref(attn) if attn is not None else None,
                                          ctypes.c_void_p(_lib.stream_ptr(m.device)))
    return rc, lib.evt_last_error()


def test_window_maps_error_cases(gpu):
    """Every documented C-level error is EVT_EINVAL with a message, before any launch: nothing is
    written. A ViT handle is refused with a message naming evt_forward_attention, and the old
    entry points keep refusing Swin."""
    c = _case("tiny_56")
    m = c["make"]("bf16", 1, gpu)
    x = torch.from_numpy(c["img"]).to(gpu)
    b = x.shape[0]
    f0, map0 = _buffer(m._window_map_shape(b, 0), gpu)
    f1, map1 = _buffer(m._window_map_shape(b, 1), gpu)
    fl, logits = _buffer((b, m.num_classes), gpu)
    idx = lambda *v: (ctypes.c_int32 * len(v))(*v)  # noqa: E731
    ptr = lambda *t: (ctypes.c_void_p * len(t))(*[u.data_ptr() if u is not None else None  # noqa: E731
                                                  for u in t])

    def args(blocks=None, maps=None, n_maps=None, queries=_lib.ATTN_ALL):
        a = _lib.evt_attn_args()
        a.n_maps = (len(blocks) if blocks is not None else 0) if n_maps is None else n_maps
        if blocks is not None:
            a.blocks = blocks
        if maps is not None:
            a.maps = maps
        a.queries = queries
        return a
    good = lambda: args(idx(0), ptr(map0))  # noqa: E731
    empty_feat, feat = _lib.evt_features_args(), _lib.evt_features_args()
    feat.logits = logits.data_ptr()
    bad_img, bad_fmt = _lib.evt_image_args(), _lib.evt_image_args()
    bad_fmt.data, bad_fmt.format = x.data_ptr(), 9
    bad = {
        "n_maps -1": dict(attn=args(n_maps=-1)),
        "n_maps 65": dict(attn=args(idx(*range(65)), ptr(*([map0] * 65)))),
        "n_maps 0, no feat": dict(attn=args()),
        "n_maps 0, feat without outputs": dict(attn=args(), feat=empty_feat),
        "maps with a feat without outputs": dict(attn=good(), feat=empty_feat),
        "NULL arrays": dict(attn=args(n_maps=1)),
        "NULL map pointer": dict(attn=args(idx(0), ptr(None))),
        "block out of range": dict(attn=args(idx(4), ptr(map0))),
        "negative block": dict(attn=args(idx(-1), ptr(map0))),
        "blocks not increasing": dict(attn=args(idx(1, 0), ptr(map1, map0))),
        "block named twice": dict(attn=args(idx(0, 0), ptr(map0, map1))),
        "queries CLS": dict(attn=args(idx(0), ptr(map0), queries=_lib.ATTN_CLS)),
        "queries 2": dict(attn=args(idx(0), ptr(map0), queries=2)),
        "map misaligned": dict(attn=args(idx(0), ptr(f0[1:1 + map0.numel()]))),
        "batch 0": dict(attn=good(), batch=0),
        "batch > max_batch": dict(attn=good(), batch=b + 1),
        "batch > max_batch with feat": dict(attn=good(), feat=feat, batch=b + 1),
        "NULL attn": dict(attn=None),
        "NULL image data": dict(attn=good(), img=bad_img),
        "unknown image format": dict(attn=good(), img=bad_fmt),
    }
    for what, kw in bad.items():
        rc, msg = _raw(m, x, **kw)
        assert rc == _lib.EVT_EINVAL and msg, what
    lib = _lib.load_library()
    assert lib.evt_forward_window_attention(ctypes.c_void_p(m._handle), None, b, None,
                                            ctypes.byref(good()), None) == _lib.EVT_EINVAL
    nw, h, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    shape = lambda mm, i: lib.evt_window_attn_map_shape(  # noqa: E731
        ctypes.c_void_p(mm._handle), i, ctypes.byref(nw), ctypes.byref(h), ctypes.byref(t))
    for i in range(m.num_blocks):
        assert shape(m, i) == 0 and (nw.value, h.value, t.value) == m.window_attn_shape(i)
    assert shape(m, 4) == _lib.EVT_EINVAL and shape(m, -1) == _lib.EVT_EINVAL
    # the old entry points keep refusing Swin
    with pytest.raises(ValueError, match="windowed"):
        m.attention_maps(x)
    img = _lib.evt_image_args()
    img.data = x.data_ptr()
    cls = args(idx(0), ptr(map0), queries=_lib.ATTN_CLS)
    assert lib.evt_forward_attention(ctypes.c_void_p(m._handle), ctypes.byref(img), b, None,
                                     ctypes.byref(cls), None) == _lib.EVT_EINVAL
    assert b"Swin" in lib.evt_last_error()
    # a ViT handle: its maps are evt_forward_attention's
    geo = dict(dim=128, depth=2, heads=2, mlp_dim=256, image_size=32, patch_size=16, num_classes=16)
    mv = ViT(dtype="bf16", device=gpu, max_batch=2, lanes=1,
             weights=make_vit_params(vit_config(128, 2, 2, 256, image_size=32, patch_size=16,
                                                num_classes=16), seed=51), **geo)
    xv = torch.from_numpy(make_images(2, seed=52, image_size=32)).to(gpu)
    with pytest.raises(ValueError, match="attention_maps"):
        mv.window_attention_maps(xv)
    rc, msg = _raw(mv, xv, good())
    assert rc == _lib.EVT_EINVAL and b"evt_forward_attention" in msg
    assert shape(mv, 0) == _lib.EVT_EINVAL
    torch.cuda.synchronize()
    assert all(_untouched(f) for f in (f0, f1, fl))
    assert GUARD > 0
