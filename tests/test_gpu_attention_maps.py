"""GPU: attention-map outputs (include/evt_attention_maps.h; csrc/attn_maps.hip).

Op level (evt_attention_probs): q and k rounded to the dtype first, the reference the fp64 softmax
of those same values, at the shapes where the kernel (one 16-query tile per wave, 64-key blocks,
rows stored through a per-wave LDS tile) can go wrong: fewer tokens than a tile, exactly a tile, a
tile + 1, 197 / 257 / 577 tokens (rows that start 16-byte aligned one time in four), head sizes
padded to 32 / 96 / 128 (50x32, 65x80, 33x128, 21x20) and 4096 keys in CLS mode. Outputs are
NaN-prefilled with guard words; qkv sits inside a NaN-filled allocation, so a read past the last
row shows as NaN. The kernel's second store form (16-byte stores of each row's aligned body,
EVT_ATTN_MAPS_STORE=wide, kept for the measurement) must give the same bits.

Model level (attention_maps / attention_maps_into / evt_forward_attention): every block of a
REFERENCE, a STANDARD (head-major QKV in bf16), a pruned (heads differ per block), a T2T and a
290-token ViT against the fp64 oracle, both dtypes, both `queries` modes.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import Uint8Images, _lib
from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer
from edgevisiontransformer_amd.modeling.models.t2t_vit import T2T_ViT
from edgevisiontransformer_amd.modeling.models.vit import (StandardViT, ViT, ViT_Pruned,
                                                           pruned_config)
from edgevisiontransformer_amd.weights import (make_images, make_std_vit_params, make_swin_params,
                                               make_t2t_params, make_vit_params, swin_config,
                                               t2t_config, vit_config)
from oracle import t2t_ref, vit_ref
from tests._ops import TDT, _p, _s
from tests.test_gpu_features import GUARD, _buffer, _cos_rows, _untouched, _written

pytestmark = pytest.mark.gpu

# Op level, against the fp64 softmax of the same (rounded) q and k, over every case below
# (the x6 case included), measured on an MI355X on the first run of this file: largest max-abs
# error and largest |sum_j p - 1| of a row. The gates are twice that (other seeds and shapes; the
# arithmetic is deterministic, so not device differences).
# Both maxima are the x6 case's (scores past +-88: the rounding of (s - m) c is 1e-5 there); with
# unit-variance q and k the largest are 1.750e-7 (f32) and 7.851e-8 (bf16).
OP_ERR_MEASURED = {"f32": 7.842e-6, "bf16": 3.341e-6}
OP_ROWSUM_MEASURED = {"f32": 1.772e-7, "bf16": 1.602e-7}
# Model level, bf16: largest max-abs error of a map against the fp64 oracle over every case,
# block and mode below, measured on the same run: 2.790e-3 (pruned, block 0; per case 2.3e-4 ..
# 2.8e-3; lowest row cosine 0.999962, gate 0.9995; f32: at most 2.813e-7, gate 1e-3). The gate is
# twice the measured value, for the same reason.
MODEL_BF16_ERR_MEASURED = 2.790e-3
PRUNED = "layerwise_h1-d0.5_h3-d1.0_h2-d0.3"
PAD = 64  # NaN elements before and after qkv


# ---- op level ---------------------------------------------------------------------------------
OP_CASES = [  # (B, H, N, h_k, modes)
    (2, 3, 5, 64, "both"), (1, 2, 16, 64, "both"), (2, 2, 17, 64, "both"),
    (2, 3, 197, 64, "both"), (1, 2, 257, 64, "both"), (1, 1, 577, 64, "both"),
    (2, 2, 50, 32, "both"), (1, 2, 65, 80, "both"), (1, 1, 33, 128, "both"),
    (1, 2, 21, 20, "both"), (1, 1, 4096, 64, "cls"),
]
HEAD_MAJOR = {(2, 3, 197, 64), (1, 2, 257, 64)}  # both layouts (bf16, h_k = 64)


def _embed(t, gpu):
    """t on the device inside a NaN-filled allocation, 16-byte aligned: (holder, view)."""
    flat = torch.full((t.numel() + 2 * PAD,), float("nan"), dtype=t.dtype, device=gpu)
    flat[PAD:PAD + t.numel()] = t.reshape(-1).to(gpu)
    return flat, flat[PAD:PAD + t.numel()].view(t.shape)


@functools.lru_cache(maxsize=None)
def _op_inputs(B, H, N, hd, dtype, gain):
    """(qkv [B*N, 3*H*hd] rounded to the dtype, on the host; fp64 reference [B, H, N, N] or, past
    1024 tokens, its CLS rows [B, H, 1, N])."""
    rng = np.random.default_rng(1000 * N + 10 * hd + H + B)
    qkv = torch.from_numpy(rng.standard_normal((B * N, 3 * H * hd)).astype(np.float32) * gain)
    qkv = qkv.to(TDT[dtype])
    x = qkv.double().numpy().reshape(B, N, 3, H, hd).transpose(2, 0, 3, 1, 4)
    q = x[0] if N <= 1024 else x[0][:, :, :1]
    ref = vit_ref.softmax(np.einsum("bhid,bhjd->bhij", q, x[1]) * hd ** -0.5)
    return qkv, ref


def _probs(dtype, qkv, B, N, H, hd, nq, gpu, head_major=False, scale=None):
    """evt_attention_probs into a guarded NaN-filled buffer -> [B, H, nq, N]. scale: hd^-0.5
    unless given."""
    scale = hd ** -0.5 if scale is None else scale
    if head_major:  # [B][H][q | k | v][N][64]
        qkv = qkv.view(B, N, 3, H, 64).permute(0, 3, 2, 1, 4).contiguous()
        ldq, sb, sh, ko = 64, 3 * H * N * 64, 3 * N * 64, N * 64
    else:
        ldq, sb, sh, ko = qkv.shape[1], 0, 0, 0
    holder, dev = _embed(qkv, gpu)
    flat, out = _buffer((B, H, nq, N), gpu)
    _lib.check(_lib.load_library().evt_attention_probs(
        _lib.DTYPE[dtype], _p(dev), ldq, sb, sh, ko, B, N, H, hd, scale, nq, _p(out), _s()))
    torch.cuda.synchronize()
    assert _written(flat), "NaN left in the output (or read past qkv) or guard words overwritten"
    del holder
    return out


def _op_check(dtype, B, H, N, hd, modes, gpu, gain=1.0):
    qkv, ref = _op_inputs(B, H, N, hd, dtype, gain)
    cls = _probs(dtype, qkv, B, N, H, hd, 1, gpu)
    outs = [cls]
    if modes == "both":
        full = _probs(dtype, qkv, B, N, H, hd, N, gpu)
        assert torch.equal(cls[:, :, 0], full[:, :, 0]), "CLS output differs from ALL[:, :, 0]"
        outs.append(full)
    for o in outs:
        assert bool(torch.isfinite(o).all()) and float(o.min()) >= 0.0 and float(o.max()) <= 1.0
    nq = outs[-1].shape[2]
    if dtype == "bf16" and (B, H, N, hd) in HEAD_MAJOR:
        assert torch.equal(_probs(dtype, qkv, B, N, H, hd, nq, gpu, head_major=True), outs[-1]), \
            "head-major differs from token-major"
    assert torch.equal(_probs(dtype, qkv, B, N, H, hd, nq, gpu), outs[-1]), "second launch differs"
    if B > 1:  # a permuted batch gives the same output, permuted
        perm = np.roll(np.arange(B), 1)
        qp = qkv.view(B, N, -1)[torch.from_numpy(perm)].reshape(B * N, -1).contiguous()
        assert torch.equal(_probs(dtype, qp, B, N, H, hd, nq, gpu), outs[-1][torch.from_numpy(perm).to(gpu)])
    got = outs[-1].double().cpu().numpy()
    err = np.abs(got - ref[:, :, :nq]).max()
    rs = np.abs(got.sum(-1) - 1.0).max()
    print(f"ATTNMAPS-OP {dtype} B{B} H{H} N{N} hd{hd} gain{gain:g}: max-abs {err:.3e} "
          f"rowsum {rs:.3e}")
    assert err <= 2 * OP_ERR_MEASURED[dtype], f"max-abs {err:.3e}"
    assert rs <= 2 * OP_ROWSUM_MEASURED[dtype], f"|sum p - 1| {rs:.3e}"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", OP_CASES, ids=lambda c: "x".join(map(str, c[:4])))
def test_attention_probs(gpu, case, dtype):
    B, H, N, hd, modes = case
    _op_check(dtype, B, H, N, hd, modes, gpu)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_attention_probs_large_scores(gpu, dtype):
    """q and k scaled by 6: the scores reach past +-88, where exp without the max subtraction
    overflows fp32. Same gate."""
    qkv, _ = _op_inputs(2, 3, 197, 64, dtype, 6.0)
    x = qkv.double().numpy().reshape(2, 197, 3, 3, 64)
    s = np.einsum("bihd,bjhd->bhij", x[:, :, 0], x[:, :, 1]) / 8.0
    assert s.max() > 88.0 and s.min() < -88.0
    _op_check(dtype, 2, 3, 197, 64, "both", gpu, gain=6.0)


@pytest.mark.parametrize("shape", [(2, 3, 197, 64), (1, 2, 16, 64), (1, 2, 65, 80)],
                         ids=lambda c: "x".join(map(str, c)))
def test_attention_probs_store_forms_agree(gpu, monkeypatch, shape):
    """The wide store form (aligned 16-byte body, peeled edges) writes the bits of the launched
    dword form: 197 and 65 tokens have rows at every alignment, 16 only aligned ones."""
    B, H, N, hd = shape
    for dtype in ("f32", "bf16"):
        qkv, _ = _op_inputs(B, H, N, hd, dtype, 1.0)
        want = _probs(dtype, qkv, B, N, H, hd, N, gpu)
        monkeypatch.setenv("EVT_ATTN_MAPS_STORE", "wide")
        got = _probs(dtype, qkv, B, N, H, hd, N, gpu)
        monkeypatch.delenv("EVT_ATTN_MAPS_STORE")
        assert torch.equal(got, want)


# ---- model level ------------------------------------------------------------------------------
def _probs64(qkv, b, n, h, hk):
    x = qkv.reshape(b, n, 3, h, hk).transpose(2, 0, 3, 1, 4)
    return vit_ref.softmax(np.einsum("bhid,bhjd->bhij", x[0], x[1]) * hk ** -0.5)


def _std_maps(params, cfg, img, eps=1e-6):
    """fp64 attention probabilities of every block of the STANDARD ViT: std_vit_forward's loop
    (oracle/vit_ref.py) built from the oracle's own layer_norm / softmax, keeping `att`."""
    import math

    from scipy.special import erf
    ln = vit_ref.layer_norm
    P = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    x = vit_ref.patchify_nchw(np.asarray(img, dtype=np.float64), cfg.patch_size) @ P["patch_w"] \
        + P["patch_b"]
    b = x.shape[0]
    x = np.concatenate([np.broadcast_to(P["cls"], (b, 1, cfg.dim)), x], axis=1) + P["pos"]
    maps = []
    for i in range(cfg.depth):
        h, hk = cfg.heads[i], cfg.head_dim[i]
        n = x.shape[1]
        qkv = ln(x, P[f"l{i}.ln1_g"], P[f"l{i}.ln1_b"], eps) @ P[f"l{i}.qkv_w"] + P[f"l{i}.qkv_b"]
        att = _probs64(qkv, b, n, h, hk)
        maps.append(att)
        v = qkv.reshape(b, n, 3, h, hk).transpose(2, 0, 3, 1, 4)[2]
        o = np.einsum("bhij,bhjd->bhid", att, v).transpose(0, 2, 1, 3).reshape(b, n, h * hk)
        x = x + o @ P[f"l{i}.out_w"] + P[f"l{i}.out_b"]
        z = ln(x, P[f"l{i}.ln2_g"], P[f"l{i}.ln2_b"], eps) @ P[f"l{i}.fc1_w"] + P[f"l{i}.fc1_b"]
        x = x + (0.5 * z * (1.0 + erf(z / math.sqrt(2.0)))) @ P[f"l{i}.fc2_w"] + P[f"l{i}.fc2_b"]
    return maps


def _trace_maps(trace, params, heads, hks):
    """From the oracle's trace of a REFERENCE ViT / T2T-ViT: softmax of LN1(x) @ qkv_w."""
    maps = []
    for i, (h, hk) in enumerate(zip(heads, hks)):
        y = trace[f"l{i}.ln1"]
        maps.append(_probs64(y @ np.asarray(params[f"l{i}.qkv_w"], np.float64), y.shape[0],
                             y.shape[1], h, hk))
    return maps


def _ref_case(batch=2, **geo):
    cfg = vit_config(geo["dim"], geo["depth"], geo["heads"], geo["mlp_dim"],
                     image_size=geo["image_size"], patch_size=geo["patch_size"], num_classes=16)
    params = make_vit_params(cfg, seed=61)
    img = make_images(batch, seed=62, image_size=cfg.image_size)
    trace = {}
    vit_ref.vit_forward(params, cfg, img, trace=trace)
    make = lambda dtype, lanes, gpu: ViT(dtype=dtype, weights=params, device=gpu,  # noqa: E731
                                         max_batch=batch, lanes=lanes, num_classes=16, **geo)
    return dict(make=make, img=img, ref=_trace_maps(trace, params, cfg.heads, cfg.head_dim))


def _std_case():
    cfg = vit_config(384, 2, 6, 1536, image_size=224, patch_size=16, num_classes=16)
    params = make_std_vit_params(cfg, seed=63)
    img = make_images(2, seed=64, image_size=224)
    make = lambda dtype, lanes, gpu: StandardViT(  # noqa: E731
        image_size=224, patch_size=16, num_classes=16, dim=384, depth=2, heads=6, dtype=dtype,
        weights=params, device=gpu, max_batch=2, lanes=lanes)
    return dict(make=make, img=img, ref=_std_maps(params, cfg, img))


def _pruned_case():
    geo = dict(dim=192, depth=3, heads=3, mlp_dim=768, image_size=64, patch_size=16, num_classes=16)
    cfg = pruned_config(PRUNED, **geo)
    params = make_vit_params(cfg, seed=65)
    img = make_images(2, seed=66, image_size=64)
    trace = {}
    vit_ref.vit_forward(params, cfg, img, trace=trace)
    make = lambda dtype, lanes, gpu: ViT_Pruned(  # noqa: E731
        prune_encoding=PRUNED, dtype=dtype, weights=params, device=gpu, max_batch=2, lanes=lanes,
        **geo)
    assert len(set(cfg.heads)) > 1
    return dict(make=make, img=img, ref=_trace_maps(trace, params, cfg.heads, cfg.head_dim))


def _t2t_case():
    args = (256, 2, 4, 2)
    cfg = t2t_config(*args)
    params = make_t2t_params(cfg, seed=67)
    img = make_images(2, seed=68, layout="NHWC")
    trace = {}
    t2t_ref.t2t_vit_forward(params, cfg, img, trace=trace)
    make = lambda dtype, lanes, gpu: T2T_ViT(  # noqa: E731
        hidden_size=args[0], depth=args[1], num_heads=args[2], mlp_ratio=args[3], dtype=dtype,
        weights=params, device=gpu, max_batch=2, lanes=lanes)
    return dict(make=make, img=img, ref=_trace_maps(trace, params, [cfg.heads] * cfg.depth,
                                                    [cfg.dim // cfg.heads] * cfg.depth))


CASES = {
    "vit_ref_192": lambda: _ref_case(dim=192, depth=2, heads=3, mlp_dim=768, image_size=32,
                                     patch_size=16),
    "std_384_224": _std_case,
    "pruned": _pruned_case,
    "t2t": _t2t_case,
    "vit_290": lambda: _ref_case(dim=128, depth=2, heads=2, mlp_dim=256, image_size=272,
                                 patch_size=16),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Built once (the fp64 reference is shared by both dtypes) and never modified."""
    return CASES[name]()


def _run(m, x, queries, blocks=None, logits=True, pooled=False):
    """attention_maps_into on guarded buffers -> {"maps": [...], "logits", "pooled"}."""
    b, gpu = x.shape[0], m.device
    blocks = list(range(m.num_blocks)) if blocks is None else list(blocks)
    q = _lib.ATTN_ALL if queries == "all" else _lib.ATTN_CLS
    bufs = [_buffer(m._map_shape(b, i, q), gpu) for i in blocks]
    extra = {}
    if logits:
        extra["logits"] = _buffer((b, m.num_classes), gpu)
    if pooled:
        extra["pooled"] = _buffer((b, m.feature_dim), gpu)
    m.attention_maps_into(x, blocks=blocks, map_tensors=[v for _, v in bufs], queries=queries,
                          **{k: v for k, (_, v) in extra.items()})
    torch.cuda.synchronize()
    for flat, _ in bufs + list(extra.values()):
        assert _written(flat), "NaN left in an output or guard words overwritten"
    out = {k: v for k, (_, v) in extra.items()}
    out["maps"] = [v for _, v in bufs]
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_model_maps(gpu, name, dtype):
    c = _case(name)
    m = c["make"](dtype, 1, gpu)
    x = torch.from_numpy(c["img"]).to(gpu)
    plain = m(x).clone()
    pooled = m.forward_features(x).clone()
    full = _run(m, x, "all", pooled=True)
    cls = _run(m, x, "cls")
    assert torch.equal(full["logits"], plain) and torch.equal(cls["logits"], plain)
    assert torch.equal(full["pooled"], pooled)
    assert torch.equal(m(x), plain)  # a plain forward after a maps forward is unchanged
    worst = 0.0
    for i, (a, r) in enumerate(zip(full["maps"], c["ref"])):
        assert tuple(a.shape) == r.shape == (x.shape[0], *m.attn_shape(i), m.attn_shape(i)[1])
        assert torch.equal(cls["maps"][i], a[:, :, 0]), f"block {i}: CLS differs from ALL[:, :, 0]"
        assert bool(torch.isfinite(a).all()) and float(a.min()) >= 0.0 and float(a.max()) <= 1.0
        got = a.double().cpu().numpy()
        err, cos = np.abs(got - r).max(), _cos_rows(got, r).min()
        print(f"ATTNMAPS-MODEL {name} {dtype} block {i}: max-abs {err:.3e} min row cosine {cos:.6f}")
        worst = max(worst, err)
        if dtype == "f32":
            assert err <= 1e-3, f"block {i} f32 max-abs {err:.3e}"
        else:
            assert cos >= 0.9995, f"block {i} bf16 row cosine {cos:.6f}"
            assert err <= 2 * MODEL_BF16_ERR_MEASURED, f"block {i} bf16 max-abs {err:.3e}"
    print(f"ATTNMAPS-MODEL-MAX {name} {dtype}: {worst:.3e}")
    # lanes = 2: the call runs as one lane on the handle's own workspace
    m2 = c["make"](dtype, 2, gpu)
    assert m2.lanes() == 2
    out2 = _run(m2, x, "all", logits=False)
    assert all(torch.equal(u, v) for u, v in zip(out2["maps"], full["maps"]))


def test_model_maps_head_major_layout(gpu, monkeypatch):
    """The model's QKV GEMM stores head-major only from the batch at which it takes the persistent
    kernel (2 images do not reach it): at 20 images of std_384_224 in bf16 both layers do
    (asserted), and the maps are bitwise those of an EVT_QKV_LAYOUT=token handle."""
    c = _case("std_384_224")
    x = torch.from_numpy(make_images(20, seed=69, image_size=224)).to(gpu)

    def build():
        m = c["make"]("bf16", 1, gpu)
        m._build(20)
        return m
    mh = build()
    hm = _run(mh, x, "all")
    assert mh.qkv_headmajor_layers() == mh.num_blocks
    monkeypatch.setenv("EVT_QKV_LAYOUT", "token")
    mt = build()
    tok = _run(mt, x, "all")
    assert mt.qkv_headmajor_layers() == 0
    assert torch.equal(hm["logits"], tok["logits"])
    assert all(torch.equal(u, v) for u, v in zip(hm["maps"], tok["maps"]))
    assert all(torch.equal(u, v[:, :, 0]) for u, v in zip(_run(mh, x, "cls")["maps"], hm["maps"]))


def test_maps_numpy_order_and_single_block(gpu):
    """numpy in, numpy out; maps come back in the order given, negative indices resolved; a
    single late block equals that block of the all-blocks call."""
    c = _case("pruned")
    m = c["make"]("f32", 1, gpu)
    out = m.attention_maps(c["img"], blocks=(-1, 0), queries="all", logits=True)
    assert isinstance(out["logits"], np.ndarray) and all(isinstance(v, np.ndarray) for v in out["maps"])
    assert [v.shape[1] for v in out["maps"]] == [m.attn_shape(2)[0], m.attn_shape(0)[0]]
    x = torch.from_numpy(c["img"]).to(gpu)
    full = _run(m, x, "all")
    assert np.array_equal(out["maps"][0], full["maps"][2].cpu().numpy())
    assert np.array_equal(out["maps"][1], full["maps"][0].cpu().numpy())
    assert np.array_equal(out["logits"], m(c["img"]))
    dev = m.attention_maps(x)  # defaults: the last block's CLS rows, device tensors
    assert isinstance(dev["maps"][0], torch.Tensor) and list(dev) == ["maps"]
    assert torch.equal(dev["maps"][0], full["maps"][2][:, :, 0])


def test_maps_with_features_through_feat(gpu):
    """evt_forward_attention with a full `feat` (logits, pooled, tokens, a tap): every feature
    output is bitwise that of features(), the maps those of a maps-only call."""
    c = _case("vit_ref_192")
    m = c["make"]("bf16", 1, gpu)
    x = torch.from_numpy(c["img"]).to(gpu)
    want = m.features(x, tokens=True, taps=(1,), logits=True)
    maps = _run(m, x, "cls", logits=False)["maps"]
    b, (f, t, geo) = x.shape[0], m._feature_geometry()
    bufs = {"logits": _buffer((b, m.num_classes), gpu), "pooled": _buffer((b, f), gpu),
            "tokens": _buffer((b, t, f), gpu), "tap": _buffer((b, *geo[1]), gpu),
            "map": _buffer(m._map_shape(b, 0, _lib.ATTN_CLS), gpu)}
    feat = _lib.evt_features_args()
    feat.logits, feat.pooled, feat.tokens = (bufs[k][1].data_ptr() for k in ("logits", "pooled", "tokens"))
    feat.n_taps = 1
    feat.tap_blocks = (ctypes.c_int32 * 1)(1)
    feat.taps = (ctypes.c_void_p * 1)(bufs["tap"][1].data_ptr())
    a = _lib.evt_attn_args()
    a.n_maps, a.queries = 1, _lib.ATTN_CLS
    a.blocks = (ctypes.c_int32 * 1)(0)
    a.maps = (ctypes.c_void_p * 1)(bufs["map"][1].data_ptr())
    img = _lib.evt_image_args()
    img.data = x.data_ptr()
    _lib.check(_lib.load_library().evt_forward_attention(
        ctypes.c_void_p(m._handle), ctypes.byref(img), b, ctypes.byref(feat), ctypes.byref(a),
        ctypes.c_void_p(_lib.stream_ptr(m.device))))
    torch.cuda.synchronize()
    assert all(_written(flat) for flat, _ in bufs.values())
    for k in ("logits", "pooled", "tokens"):
        assert torch.equal(bufs[k][1], want[k]), k
    assert torch.equal(bufs["tap"][1], want["taps"][0])
    assert torch.equal(bufs["map"][1], maps[0])


def test_maps_uint8_images(gpu):
    """A Uint8Images batch gives bitwise the maps and logits of its to_float image."""
    c = _case("vit_ref_192")
    m = c["make"]("bf16", 1, gpu)
    rng = np.random.default_rng(7)
    u8 = Uint8Images(torch.from_numpy(rng.integers(0, 256, (2, 32, 32, 3), dtype=np.uint8)).to(gpu))
    want = _run(m, u8.to_float("nchw"), "all")
    got = _run(m, u8, "all")
    assert torch.equal(got["logits"], want["logits"])
    assert all(torch.equal(u, v) for u, v in zip(got["maps"], want["maps"]))
    host = m.attention_maps(Uint8Images(u8.data.cpu().numpy()), blocks=(0, 1), queries="all")
    assert all(np.array_equal(u, v.cpu().numpy()) for u, v in zip(host["maps"], want["maps"]))


def test_maps_under_profile_count_as_head(gpu):
    """A profiled maps forward adds EVT_PROF_HEAD launches only; the next plain forward's role
    counts are unchanged."""
    c = _case("vit_ref_192")
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
    maps = launches(lambda: _run(m, x, "all"))
    assert maps[head] == plain[head] + 2  # one export per block
    assert [v for i, v in enumerate(maps) if i != head] == [v for i, v in enumerate(plain) if i != head]
    assert launches(lambda: m(x)) == plain


def _raw(m, x, attn, feat=None, batch=None, img=None):
    lib = _lib.load_library()
    if img is None:
        img = _lib.evt_image_args()
        img.data = x.data_ptr()
    rc = lib.evt_forward_attention(ctypes.c_void_p(m._handle), ctypes.byref(img),
                                   x.shape[0] if batch is None else batch,
                                   ctypes.byref(feat) if feat is not None else None,
                                   ctypes.byref(attn) if attn is not None else None,
                                   ctypes.c_void_p(_lib.stream_ptr(m.device)))
    return rc, lib.evt_last_error()


def test_maps_error_cases(gpu):
    """Swin and MX8 raise ValueError on the host; every documented C-level error is EVT_EINVAL
    with a message, before any launch: nothing is written."""
    c = _case("vit_ref_192")
    m = c["make"]("bf16", 1, gpu)
    x = torch.from_numpy(c["img"]).to(gpu)
    b = x.shape[0]
    f0, map0 = _buffer(m._map_shape(b, 0, _lib.ATTN_CLS), gpu)
    f1, map1 = _buffer(m._map_shape(b, 1, _lib.ATTN_CLS), gpu)
    fl, logits = _buffer((b, 16), gpu)
    idx = lambda *v: (ctypes.c_int32 * len(v))(*v)  # noqa: E731
    ptr = lambda *t: (ctypes.c_void_p * len(t))(*[u.data_ptr() if u is not None else None  # noqa: E731
                                                  for u in t])

    def args(blocks=None, maps=None, n_maps=None, queries=0):
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
        "block out of range": dict(attn=args(idx(2), ptr(map0))),
        "negative block": dict(attn=args(idx(-1), ptr(map0))),
        "blocks not increasing": dict(attn=args(idx(1, 0), ptr(map1, map0))),
        "block named twice": dict(attn=args(idx(0, 0), ptr(map0, map1))),
        "queries 2": dict(attn=args(idx(0), ptr(map0), queries=2)),
        "queries -1": dict(attn=args(idx(0), ptr(map0), queries=-1)),
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
    assert lib.evt_forward_attention(ctypes.c_void_p(m._handle), None, b, None, ctypes.byref(good()),
                                     None) == _lib.EVT_EINVAL
    h, t = ctypes.c_int(), ctypes.c_int()
    for i in range(m.num_blocks):
        assert lib.evt_attn_map_shape(ctypes.c_void_p(m._handle), i, ctypes.byref(h), ctypes.byref(t)) == 0
        assert (h.value, t.value) == m.attn_shape(i)
    assert lib.evt_attn_map_shape(ctypes.c_void_p(m._handle), 2, ctypes.byref(h),
                                  ctypes.byref(t)) == _lib.EVT_EINVAL
    # Swin: a different object
    cfg = swin_config("tiny", image_size=56, window_size=7, depths=(2, 2), num_heads=(3, 6),
                      num_classes=11)
    ms = SwinTransformer(img_size=56, patch_size=cfg.patch_size, num_classes=11,
                         embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
                         window_size=7, dtype="bf16", weights=make_swin_params(cfg, seed=3),
                         device=gpu, max_batch=2, lanes=1)
    xs = torch.from_numpy(make_images(2, seed=4, image_size=56)).to(gpu)
    with pytest.raises(ValueError, match="windowed"):
        ms.attention_maps(xs)
    rc, msg = _raw(ms, xs, good())
    assert rc == _lib.EVT_EINVAL and b"Swin" in msg
    assert lib.evt_attn_map_shape(ctypes.c_void_p(ms._handle), 0, ctypes.byref(h),
                                  ctypes.byref(t)) == _lib.EVT_EINVAL
    # MX8: as taps
    geo = dict(dim=128, depth=2, heads=2, mlp_dim=256, image_size=32, patch_size=16, num_classes=16)
    m8 = ViT(dtype="mx8", device=gpu, max_batch=3, lanes=1,
             weights=make_vit_params(vit_config(128, 2, 2, 256, image_size=32, patch_size=16,
                                                num_classes=16), seed=51), **geo)
    with pytest.raises(ValueError, match="mx8"):
        m8.attention_maps(x)
    rc, msg = _raw(m8, x, good())
    assert rc == _lib.EVT_EINVAL and b"MX8" in msg
    torch.cuda.synchronize()
    assert all(_untouched(f) for f in (f0, f1, fl))
    assert GUARD > 0
