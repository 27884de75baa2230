"""GPU: the depth axis (include/evt_depth.h; csrc/depth_stats.hip, run_encoder's skips).

Op level (evt_stream_delta_stats) against `block_stats_reference` in fp64 on the same stored
values. The gate is derived, not tuned: a dot product of D fp32 terms carries at most D 2^-24
relative to |a||b|, so each per-token cosine and ratio, and with them their means, is gated at
8 D 2^-24 absolute plus the same relative. (The kernel's order, D / 64 or D / 128 terms per lane
and a 4-step butterfly, has a smaller bound; the wider one of the issue is kept.) Each case prints
its error as a fraction of the gate (DEPTH-OP ... frac). a and b sit at pitches above D inside
NaN-filled allocations and the output between guard words.

Model level: `block_stats` against the op on operands recovered from taps (a skipped sublayer makes
a block's tap the other sublayer's output), against the fp64 forward of tests/_depth_ref.py, and
the bitwise claims (logits, pooled, lanes, layout, uint8, graph replay, batch position). Taps give
a sublayer's operands only while the block's other sublayer is skipped (the stream between the two
sublayers has no tap), so the bitwise comparison with the op always runs under a skip; the unskipped
model's statistics are held to the fp64 forward at the derived gate, not to the bit. Skips: a model with whole
blocks skipped is bitwise a fresh model of `drop_blocks`; single sublayers against the fp64 forward
with that sublayer absent.

Largest fractions measured on an MI355X: DESIGN.md, "Depth axis".
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import Uint8Images, _lib
from edgevisiontransformer_amd.evaluate import sublayer_ablation
from edgevisiontransformer_amd.modeling.models.depth import (DEPTH_STATS, IDENTITY_STATS,
                                                             block_stats_reference)
from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer
from edgevisiontransformer_amd.modeling.models.t2t_vit import T2T_ViT
from edgevisiontransformer_amd.modeling.models.vit import StandardViT, ViT, pruned_config
from edgevisiontransformer_amd.pruning import drop_blocks
from edgevisiontransformer_amd.weights import (make_images, make_std_vit_params, make_swin_params,
                                               make_vit_params, swin_config, vit_config)
from tests import _depth_ref
from tests._ops import TDT, _p, _s

pytestmark = pytest.mark.gpu
F32_TOL = 1e-3                      # x max(1, max|golden|)
BF16_ABS, BF16_COS = 3e-2, 0.9995   # tests/test_gpu_model.py
PRUNED = "layerwise_h1-d0.5_h3-d1.0_h2-d0.3_h3-d0.5"
GUARD, GUARD_VALUE = 16, 12345.0
SHAPES = [(1, 1, 8), (2, 2, 8), (3, 64, 64), (2, 65, 200), (2, 197, 192), (1, 257, 1536),
          (1, 4096, 64)]
KINDS = ("random", "same", "negated", "zero_row", "small_update")


def gate(D, ref):
    """8 D 2^-24 absolute plus the same relative (module docstring)."""
    return 8.0 * D * 2.0 ** -24 * (1.0 + np.abs(ref))


# ---- op level -------------------------------------------------------------------------------------
def _inputs(kind, B, T, D, dtype):
    """(a, b) float32 [B T, D], exactly representable in `dtype`."""
    rng = np.random.default_rng(1000 * T + D + len(kind))
    rnd = lambda v: torch.from_numpy(v.astype(np.float32)).to(TDT[dtype]).float().numpy()  # noqa: E731
    a = rnd(rng.standard_normal((B * T, D)))
    if kind == "random":
        b = rnd(rng.standard_normal((B * T, D)))
    elif kind == "same":
        b = a.copy()
    elif kind == "negated":
        b = -a
    elif kind == "zero_row":  # |b_t| / FLT_MIN must stay finite in fp32: |b_t| about 2^-20
        b = rnd(rng.standard_normal((B * T, D)))
        r = (B * T) // 2
        a[r] = 0.0
        b[r] = rnd(b[r] * 2.0 ** -20 / np.sqrt(D))
    else:  # the element-wise difference does not cancel
        b = rnd(a + 2.0 ** -7 * rng.standard_normal((B * T, D)).astype(np.float32))
    return a, b


def _strided(rows, ld, dtype, gpu):
    """rows [R, D] on the device at pitch ld inside a NaN-filled allocation: (holder, pointer)."""
    r, d = rows.shape
    flat = torch.full((r * ld + 64,), float("nan"), dtype=TDT[dtype], device=gpu)
    view = flat[32:32 + r * ld].view(r, ld)
    view[:, :d] = torch.from_numpy(rows).to(TDT[dtype]).to(gpu)
    return flat, view


def _op(dtype, a, b, B, T, D, gpu, pad=(24, 8)):
    ha, va = _strided(a, D + pad[0], dtype, gpu)
    hb, vb = _strided(b, D + pad[1], dtype, gpu)
    flat = torch.full((GUARD + B * 4 + GUARD,), GUARD_VALUE, dtype=torch.float32, device=gpu)
    flat[GUARD:GUARD + B * 4] = float("nan")
    out = flat[GUARD:GUARD + B * 4].view(B, 4)
    _lib.check(_lib.load_library().evt_stream_delta_stats(
        _lib.DTYPE[dtype], _p(va), D + pad[0], _p(vb), D + pad[1], B, T, D, _p(out), _s()))
    torch.cuda.synchronize()
    assert bool((flat[:GUARD] == GUARD_VALUE).all()) and bool((flat[-GUARD:] == GUARD_VALUE).all()), \
        "guard words around out overwritten"
    assert not bool(torch.isnan(out).any()), "NaN in the output (unwritten, or read past the rows)"
    del ha, hb
    return out.clone()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_against_reference(gpu, shape, dtype):
    B, T, D = shape
    worst = 0.0
    for kind in KINDS:
        a, b = _inputs(kind, B, T, D, dtype)
        out = _op(dtype, a, b, B, T, D, gpu)
        got = out.double().cpu().numpy()
        ref = block_stats_reference(a, b, T)
        assert np.isfinite(got).all(), (kind, got)
        frac = (np.abs(got - ref) / gate(D, ref)).max(axis=0)
        print(f"DEPTH-OP {dtype} B{B} T{T} D{D} {kind}: frac "
              + " ".join(f"{s} {f:.4f}" for s, f in zip(DEPTH_STATS, frac)))
        worst = max(worst, frac.max())
        if kind == "same":
            assert (got == np.array(IDENTITY_STATS)).all(), got
        if kind == "negated":
            assert (got == np.array([-1.0, 2.0, 1.0, -1.0])).all(), got
        assert (frac <= 1).all(), f"{kind}: {frac} of the gate"
        assert torch.equal(_op(dtype, a, b, B, T, D, gpu), out), "second launch differs"
        if B > 1:
            i = B - 1
            alone = _op(dtype, a[i * T:(i + 1) * T], b[i * T:(i + 1) * T], 1, T, D, gpu)
            assert torch.equal(alone[0], out[i]), "an image alone differs from inside the batch"
    print(f"DEPTH-OP-MAX {dtype} B{B} T{T} D{D}: {worst:.4f}")


def test_op_argument_errors(gpu):
    lib = _lib.load_library()
    x = torch.zeros((64, 64), device=gpu)
    out = torch.zeros((4, 4), device=gpu)
    ok = dict(dtype=0, a=_p(x), lda=64, b=_p(x), ldb=64, B=2, T=4, D=64, out=_p(out))
    call = lambda **kw: lib.evt_stream_delta_stats(*{**ok, **kw}.values(), _s())  # noqa: E731
    assert call() == 0
    off = ctypes.c_void_p(x.data_ptr() + 4)
    for kw, msg in ((dict(B=0), b"B must"), (dict(T=0), b"T must"), (dict(T=4097), b"T must"),
                    (dict(D=4), b"multiple of 8"), (dict(D=12), b"multiple of 8"),
                    (dict(lda=56), b"at least D"), (dict(ldb=32), b"at least D"),
                    (dict(lda=66), b"16 bytes"), (dict(a=off), b"aligned"), (dict(out=None), b"non-null"),
                    (dict(dtype=2), b"dtype")):
        assert call(**kw) == _lib.EVT_EINVAL, kw
        assert msg in lib.evt_last_error(), (kw, lib.evt_last_error())
    torch.cuda.synchronize()


# ---- models ---------------------------------------------------------------------------------------
def _ref_case():
    geo = dict(dim=192, depth=4, heads=3, mlp_dim=768, image_size=32, patch_size=8, num_classes=16)
    cfg = vit_config(192, 4, 3, 768, image_size=32, patch_size=8, num_classes=16)
    return dict(cfg=cfg, params=make_vit_params(cfg, seed=81), geo=geo, cls=ViT, standard=False,
                img=make_images(2, seed=82, image_size=32))


def _pruned_case():
    geo = dict(dim=192, depth=4, heads=3, mlp_dim=768, image_size=64, patch_size=16, num_classes=16)
    cfg = pruned_config(PRUNED, **geo)
    return dict(cfg=cfg, params=make_vit_params(cfg, seed=83), geo=geo, cls=ViT, standard=False,
                img=make_images(2, seed=84, image_size=64))


def _std_case():
    geo = dict(dim=192, depth=4, heads=3, image_size=64, patch_size=8, num_classes=16)
    cfg = vit_config(192, 4, 3, 768, image_size=64, patch_size=8, num_classes=16)
    return dict(cfg=cfg, params=make_std_vit_params(cfg, seed=85), geo=geo, cls=StandardViT,
                standard=True, img=make_images(2, seed=86, image_size=64))


CASES = {"vit": _ref_case, "pruned": _pruned_case, "std": _std_case}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Built once, shared by every test, never modified."""
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def _ref_forward(name, mask):
    c = _case(name)
    return _depth_ref.forward(c["params"], c["cfg"], c["img"], list(mask), standard=c["standard"])


def _make(name, dtype, gpu, lanes=1, params=None, cfg=None, max_batch=2):
    c = _case(name)
    cfg = c["cfg"] if cfg is None else cfg
    geo = {**c["geo"], "depth": cfg.depth}
    kw = {} if c["standard"] else {"_cfg": cfg}
    return c["cls"](dtype=dtype, weights=c["params"] if params is None else params, device=gpu,
                    max_batch=max_batch, lanes=lanes, **geo, **kw)


def _img(name, gpu):
    return torch.from_numpy(_case(name)["img"]).to(gpu)


def _outputs(m, x):
    """Everything a forward gives: logits, pooled, tokens and top-5."""
    f = m.features(x, tokens=True, logits=True)
    top = m.classify(x, topk=5)
    torch.cuda.synchronize()
    return [m(x).clone(), f["logits"], f["pooled"], f["tokens"], top["indices"], top["values"]]


def _same(u, v):
    return all(torch.equal(a, b) for a, b in zip(u, v))


def _logits_gate(what, got, ref, dtype):
    got = got.double().cpu().numpy()
    err, top = np.abs(got - ref).max(), np.abs(ref).max()
    cos = ((got * ref).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(ref, axis=1))).min()
    print(f"DEPTH-SKIP {what} {dtype}: max-abs {err:.3e} max|golden| {top:.3f} min row cosine {cos:.6f}")
    if dtype == "f32":
        assert err <= F32_TOL * max(1.0, top), f"{what} f32 max-abs {err:.3e} (max|golden| {top:.3f})"
    else:
        assert err <= BF16_ABS and cos >= BF16_COS, f"{what} bf16 max-abs {err:.3e}, min cos {cos:.6f}"


def _stored(tap, dtype):
    """A tap [B, T, D] (fp32 export of the stored stream) -> float32 rows [B T, D]; the export is
    exact, so these are the stored values."""
    t = tap.to(TDT[dtype]).float()
    assert torch.equal(t, tap)
    return t.reshape(-1, t.shape[-1]).cpu().numpy()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_block_stats_model(gpu, name, dtype):
    c = _case(name)
    m = _make(name, dtype, gpu)
    x = _img(name, gpu)
    depth, T, D = c["cfg"].depth, c["cfg"].tokens, c["cfg"].dim
    assert m.block_stats_shape(-1) == (2, 4, T)
    plain, pooled = m(x).clone(), m.forward_features(x).clone()
    out = m.block_stats(x, logits=True, pooled=True)
    torch.cuda.synchronize()
    assert m.tail_mode() == 3
    assert torch.equal(out["logits"], plain) and torch.equal(out["pooled"], pooled)
    assert torch.equal(m(x), plain) and m.tail_mode() == 1
    stats = out["stats"]
    assert len(stats) == depth and all(tuple(s.shape) == (2, 2, 4) for s in stats)
    # against the fp64 forward. f32: the op gate. bf16: plus the rounding of the operands, each
    # element of a and b within 2^-9 relative, so |da| <= 2^-9 |a|, |db| <= 2^-9 |b|: the cosine
    # moves by at most 2^-8, |b| / |a| by 2^-8 of itself and |b - a| / |a| by 2^-9 (1 + |b| / |a| +
    # |b - a| / |a|), to first order; 2^-8 (1 + ratio + rel_update) covers the three.
    _, streams = _ref_forward(name, (0,) * depth)
    worst = 0.0
    for i in range(depth):
        for sub in range(2):
            a, b = (v.reshape(-1, D) for v in streams[i][sub])
            ref = block_stats_reference(a, b, T)
            g = gate(D, ref)
            if dtype == "bf16":
                g = g + 2.0 ** -8 * (1.0 + ref[:, 2:3] + ref[:, 1:2])
            got = stats[i][:, sub].double().cpu().numpy()
            frac = (np.abs(got - ref) / g).max(axis=0)
            print(f"DEPTH-MODEL {name} {dtype} block {i} {('attn', 'ffn')[sub]}: got {got[0]} ref "
                  f"{ref[0]} frac " + " ".join(f"{f:.3f}" for f in frac))
            worst = max(worst, frac.max())
    print(f"DEPTH-MODEL-MAX {name} {dtype}: {worst:.3f}")
    assert worst <= 1, f"{worst} of the gate"
    # where taps give the operands: with the FFN of block i skipped, tap i - 1 and tap i are the
    # attention sublayer's input and output, with the attention skipped the FFN's (bitwise the op).
    # The last block's CLS rows in the tap are the tail's, the statistics read the full-row
    # launch's: its token-0 values are held to the gate, not to the bit.
    for i in range(1, depth):
        for sub, other in ((0, "ffn"), (1, "attn")):
            with m.skipping({i: other}):
                taps = m.features(x, taps=(i - 1, i))["taps"]
                got = m.block_stats(x, blocks=(i,))["stats"][0]
            a, b = _stored(taps[0], dtype), _stored(taps[1], dtype)
            want = _op(dtype, a, b, 2, T, D, gpu, pad=(0, 0))
            assert torch.equal(got[:, 1 - sub], torch.tensor(IDENTITY_STATS, device=gpu).expand(2, 4))
            if i < depth - 1:
                assert torch.equal(got[:, sub], want), (i, sub)
            else:
                ref = want.double().cpu().numpy()
                g = gate(D, ref) + (2.0 ** -8 * (1.0 + ref[:, 2:3] + ref[:, 1:2])
                                    if dtype == "bf16" else 0.0)
                assert (np.abs(got[:, sub].double().cpu().numpy() - ref) <= g).all(), (i, sub)
    assert not m.skipped()
    # order given, a second call, lanes 2, token-major QKV, uint8 input, batch position
    late = m.block_stats(x, blocks=(-1, 0))["stats"]
    assert torch.equal(late[0], stats[-1]) and torch.equal(late[1], stats[0])
    m2 = _make(name, dtype, gpu, lanes=2)
    assert m2.lanes() == 2
    assert _same(m2.block_stats(x)["stats"], stats)
    one = m.block_stats(x[1:2])["stats"]
    assert all(torch.equal(u[0], v[1]) for u, v in zip(one, stats))


def test_block_stats_head_major_layout(gpu, monkeypatch):
    """The QKV GEMM stores head-major only from the batch at which it takes the persistent kernel:
    20 images of a 384-wide StandardViT at 224 px reach it in both layers (asserted). Statistics and
    logits, without and with a skip, are bitwise those of an EVT_QKV_LAYOUT=token handle."""
    cfg = vit_config(384, 2, 6, 1536, image_size=224, patch_size=16, num_classes=16)
    params = make_std_vit_params(cfg, seed=63)
    x = torch.from_numpy(make_images(20, seed=69, image_size=224)).to(gpu)
    build = lambda: StandardViT(image_size=224, patch_size=16, num_classes=16, dim=384, depth=2,  # noqa: E731
                                heads=6, dtype="bf16", weights=params, device=gpu, max_batch=20, lanes=1)

    def run(m):
        out = [m.block_stats(x, logits=True)]
        assert m.qkv_headmajor_layers() == hm_layers
        m.skip_sublayers({1: "ffn"})
        out.append(m.block_stats(x, logits=True))
        return [[o["logits"]] + o["stats"] for o in out]

    hm_layers = 2
    head = run(build())
    monkeypatch.setenv("EVT_QKV_LAYOUT", "token")
    mt = build()
    monkeypatch.delenv("EVT_QKV_LAYOUT")
    hm_layers = 0
    token = run(mt)
    assert all(_same(u, v) for u, v in zip(head, token))


def test_block_stats_uint8_graph(gpu):
    m = _make("vit", "bf16", gpu)
    x = _img("vit", gpu)
    stats = m.block_stats(x)["stats"]
    rng = np.random.default_rng(7)
    u8 = Uint8Images(torch.from_numpy(rng.integers(0, 256, (2, 32, 32, 3), dtype=np.uint8)).to(gpu))
    want = m.block_stats(u8.to_float("nchw"), logits=True)
    got = m.block_stats(u8, logits=True)
    assert torch.equal(got["logits"], want["logits"]) and _same(got["stats"], want["stats"])
    host = m.block_stats(x.cpu().numpy())
    assert all(np.array_equal(u, v.cpu().numpy()) for u, v in zip(host["stats"], stats))
    # a captured graph stays the logits forward; statistics calls around its replays do not disturb it
    logits = torch.empty((2, 16), device=gpu)
    m.capture_graph(x, logits)
    m.replay_graph()
    torch.cuda.synchronize()
    first = logits.clone()
    assert _same(m.block_stats(x)["stats"], stats)
    m.replay_graph()
    torch.cuda.synchronize()
    assert torch.equal(logits, first) and torch.equal(first, m(x))
    with pytest.raises(ValueError, match="before evt_graph_capture"):
        m.skip_sublayers({0: "attn"})
    assert not m.skipped()
    # a statistics forward captured into a graph of the caller's and replayed on new images, without
    # a skip and with one (whose identity rows are a copy node)
    for skips in ({}, {1: "ffn", 3: "attn"}):
        mg = _make("vit", "bf16", gpu)
        mg.skip_sublayers(skips)
        x2 = torch.flip(x, dims=(0,)).contiguous()
        want = mg.block_stats(x2, logits=True)
        xin, lg = x.clone(), torch.empty((2, 16), device=gpu)
        bufs = [torch.empty((2, 2, 4), device=gpu) for _ in range(4)]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            mg.block_stats_into(xin, blocks=range(4), stat_tensors=bufs, logits=lg)
        xin.copy_(x2)
        for t in bufs + [lg]:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(lg, want["logits"]) and _same(bufs, want["stats"]), skips
    # the library's own graph, captured under a skip mask, replays the skipped forward
    ms = _make("vit", "bf16", gpu)
    ms.skip_sublayers({1: "attn", 2: "block"})
    eager = ms(x).clone()
    ms.capture_graph(x, logits)
    logits.fill_(float("nan"))
    ms.replay_graph()
    torch.cuda.synchronize()
    assert torch.equal(logits, eager) and not torch.equal(eager, first)
    with pytest.raises(ValueError, match="before evt_graph_capture"):
        ms.clear_skips()
    assert ms.skipped() == {1: "attn", 2: "block"}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_skipped_blocks_are_dropped_blocks(gpu, name, dtype):
    c = _case(name)
    m = _make(name, dtype, gpu)
    x = _img(name, gpu)
    base = _outputs(m, x)
    for S in ((1,), (3,), (1, 2), (2, 3)):  # a middle block, the last block, two adjacent blocks
        m.skip_sublayers({b: "block" for b in S})
        assert m.skipped() == {b: "block" for b in S}
        got = _outputs(m, x)
        p2, c2 = drop_blocks(c["params"], c["cfg"], S)
        fresh = _make(name, dtype, gpu, params=p2, cfg=c2)
        assert _same(got, _outputs(fresh, x)), f"blocks {S} skipped differ from the dropped model"
        assert _same(got, _outputs(m, x)), "second call differs"
        assert m.tail_mode() == 1
        # a skipped block's tap is its input
        taps = m.features(x, taps=(S[0] - 1, S[0]))["taps"]
        assert torch.equal(taps[0], taps[1])
        m2 = _make(name, dtype, gpu, lanes=2)
        m2.skip_sublayers({b: "block" for b in S})
        assert torch.equal(m2(x), got[0]), "lanes 2 differ"
        m.clear_skips()
        assert _same(_outputs(m, x), base), "clearing does not restore the unskipped outputs"
    # the mask stays with the mirror across a handle rebuild
    m.skip_sublayers({1: "block"})
    small = m(x[:1]).clone()
    x3 = torch.cat([x, x[:1]])
    big = m(x3)
    assert m._max_batch == 3 and m.skipped() == {1: "block"}
    assert torch.equal(big[:1], small) and torch.equal(big[2:], small)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_single_sublayer_skips(gpu, name, dtype):
    c = _case(name)
    m = _make(name, dtype, gpu)
    x = _img(name, gpu)
    depth = c["cfg"].depth
    for block in (1, depth - 1):
        for what, bit in (("attn", 1), ("ffn", 2)):
            mask = [0] * depth
            mask[block] = bit
            ref, _ = _ref_forward(name, tuple(mask))
            with m.skipping({block: what}):
                _logits_gate(f"{name} block {block} {what}", m(x), ref, dtype)
                ident = m.block_stats(x, blocks=(block,))["stats"][0][:, bit - 1]
            assert torch.equal(ident, torch.tensor(IDENTITY_STATS, device=gpu).expand(2, 4))
    assert not m.skipped()


def test_skips_profile_work_counts_what_runs(gpu):
    m = _make("vit", "bf16", gpu)
    x = _img("vit", gpu)
    lib = _lib.load_library()

    def work():
        _lib.check(lib.evt_model_profile(m._ptr(), 1))
        m(x)
        torch.cuda.synchronize()
        us, n = (ctypes.c_float * 16)(), (ctypes.c_int * 16)()
        gf, gb = (ctypes.c_double * 16)(), (ctypes.c_double * 16)()
        _lib.check(lib.evt_model_profile_read(m._ptr(), us, n))
        _lib.check(lib.evt_model_profile_work(m._ptr(), gf, gb))
        _lib.check(lib.evt_model_profile(m._ptr(), 0))
        roles = {r: i for i, r in enumerate(_lib.PROF_ROLES)}
        return {r: (n[i], gf[i]) for r, i in roles.items()}

    full = work()
    m.skip_sublayers({1: "attn", 3: "ffn"})
    part = work()
    for role in ("qkv", "attention", "out_proj", "fc1", "fc2"):
        assert part[role][0] == full[role][0] - 1, role
        assert abs(part[role][1] - 0.75 * full[role][1]) <= 1e-9 * full[role][1], role
    assert part["patch_embed"] == full["patch_embed"]


def test_skips_compose_with_gates_and_token_schedule(gpu):
    c = _case("vit")
    m = _make("vit", "bf16", gpu)
    x = _img("vit", gpu)
    base = m(x).clone()
    g = np.array([1.0, 0.0, 0.5], dtype=np.float32)
    m.set_head_gates({1: g, 2: g})
    m.set_ffn_gates({2: np.linspace(0.0, 1.0, 768, dtype=np.float32)})
    gated = m(x).clone()
    m.set_token_pruning({0: 9})
    both = m(x).clone()
    m.skip_sublayers({2: "block"})
    got = m(x).clone()
    # the same from the other side: the dropped model with block 1's gates and the schedule
    p2, c2 = drop_blocks(c["params"], c["cfg"], (2,))
    fresh = _make("vit", "bf16", gpu, params=p2, cfg=c2)
    fresh.set_head_gates({1: g})
    fresh.set_token_pruning({0: 9})
    assert torch.equal(got, fresh(x))
    # the gates of the skipped block are kept and act again once the skip is cleared
    assert np.array_equal(m.head_gates()[2], g)
    m.clear_skips()
    assert torch.equal(m(x), both)
    m.set_token_pruning(None)
    assert torch.equal(m(x), gated)
    m.clear_gates()
    assert torch.equal(m(x), base)


def test_refusals(gpu):
    m = _make("vit", "bf16", gpu)
    x = _img("vit", gpu)
    m.skip_sublayers({1: "attn", 2: "ffn", -1: "block"})
    for fn in (lambda: m.attention_maps(x, blocks=(1,)), lambda: m.head_stats(x, blocks=(0, 1)),
               lambda: m.attention_rollout(x), lambda: m.attention_rollout(x, start=3),
               lambda: m.ffn_stats(x, blocks=(2,)), lambda: m.ffn_stats(x, blocks=(3,)),
               lambda: m.set_token_pruning({1: 8}),   # its attention is skipped
               lambda: m.set_token_pruning({2: 8})):  # the last block that runs
        with pytest.raises(ValueError, match="skip"):
            fn()
    assert m.token_schedule() == []
    # what is not skipped still works
    m.attention_maps(x, blocks=(0, 2))
    m.head_stats(x, blocks=(2,))
    m.ffn_stats(x, blocks=(0, 1))
    m.set_token_pruning({0: 8})
    with pytest.raises(ValueError, match="token schedule"):
        m.block_stats(x)
    # a schedule first, then a mask that does not fit it
    m.clear_skips()
    for bad in ({0: "attn"}, {1: "block", 2: "block", 3: "block"}):
        with pytest.raises(ValueError, match="token schedule"):
            m.skip_sublayers(bad)
    assert not m.skipped()
    m.set_token_pruning(None)
    with pytest.raises(ValueError, match="attn"):
        m.skip_sublayers({0: "mlp"})
    with pytest.raises(ValueError, match="outside"):
        m.skip_sublayers({4: "attn"})
    with pytest.raises(ValueError, match="every block"):
        m.skip_sublayers({b: "block" for b in range(4)})
    assert not m.skipped()
    # an exception inside the body: the previous mask comes back
    m.skip_sublayers({0: "ffn"})
    with pytest.raises(RuntimeError):
        with m.skipping({1: "attn"}):
            assert m.skipped() == {1: "attn"}
            raise RuntimeError("body")
    assert m.skipped() == {0: "ffn"}
    # while the stream is capturing: refused, by name, and the mask and the model stay as they were
    lib = _lib.load_library()
    before = m(x).clone()
    buf = torch.zeros(8, device=gpu)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        buf.add_(1.0)
        with pytest.raises(ValueError, match="capturing"):
            m.skip_sublayers({1: "attn"})
        with pytest.raises(ValueError, match="capturing"):
            m.clear_skips()
        cap = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        one = (ctypes.c_uint8 * 4)(0, 1, 0, 0)
        assert lib.evt_model_set_skips(m._ptr(), one, 4, cap) == _lib.EVT_EINVAL
        assert "capturing" in _lib.last_error()
        assert lib.evt_model_set_skips(m._ptr(), None, 0, cap) == _lib.EVT_EINVAL
        assert "capturing" in _lib.last_error()
    torch.cuda.synchronize()
    assert m.skipped() == {0: "ffn"} and torch.equal(m(x), before)
    # the C ABI: a mask of another depth, bits beyond the two
    four = (ctypes.c_uint8 * 4)(0, 4, 0, 0)
    assert lib.evt_model_set_skips(m._ptr(), four, 3, None) == _lib.EVT_EINVAL
    assert lib.evt_model_set_skips(m._ptr(), four, 4, None) == _lib.EVT_EINVAL
    back = (ctypes.c_uint8 * 4)()
    n = ctypes.c_int()
    assert lib.evt_model_get_skips(m._ptr(), back, 4, ctypes.byref(n)) == 0
    assert n.value == 4 and list(back) == [2, 0, 0, 0]
    # the families without a depth axis
    cfg = swin_config("tiny", image_size=56, window_size=7, depths=(2, 2), num_heads=(3, 6),
                      num_classes=11)
    s = SwinTransformer(img_size=56, patch_size=cfg.patch_size, num_classes=11,
                        embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
                        window_size=7, dtype="bf16", weights=make_swin_params(cfg, seed=3),
                        device=gpu, max_batch=1, lanes=1)
    t = T2T_ViT(hidden_size=256, depth=2, num_heads=4, mlp_ratio=2, num_classes=16, dtype="bf16",
                seed=74, device=gpu, max_batch=1, lanes=1)
    m8 = ViT(dim=128, depth=2, heads=2, mlp_dim=256, image_size=32, patch_size=16, num_classes=16,
             dtype="mx8", device=gpu, max_batch=1, lanes=1)
    for model, img in ((s, torch.zeros((1, 3, 56, 56), device=gpu)),
                       (t, torch.zeros((1, 224, 224, 3), device=gpu)),
                       (m8, torch.zeros((1, 3, 32, 32), device=gpu))):
        with pytest.raises(ValueError):
            model.block_stats(img)
        with pytest.raises(ValueError):
            model.skip_sublayers({0: "attn"})
        with pytest.raises(ValueError):  # refused before the base pass (an empty loader would pass it)
            sublayer_ablation(model, [])
        one = (ctypes.c_uint8 * 8)(1)
        assert lib.evt_model_set_skips(model._ptr(), one, 2, None) == _lib.EVT_EINVAL
        d = ctypes.c_int()
        assert lib.evt_block_stats_shape(model._ptr(), 0, ctypes.byref(d), ctypes.byref(d),
                                         ctypes.byref(d)) == _lib.EVT_EINVAL


def test_sublayer_ablation_equals_manual_runs(gpu):
    from edgevisiontransformer_amd.evaluate import evaluate
    m = _make("vit", "bf16", gpu)
    rng = np.random.default_rng(11)
    loader = [(make_images(2, seed=90 + i, image_size=32), rng.integers(0, 16, 2)) for i in range(2)]
    m.skip_sublayers({0: "ffn"})
    res = sublayer_ablation(m, loader, topk=3, blocks=(0, 3))
    assert res["blocks"] == [0, 3] and m.skipped() == {0: "ffn"}
    assert res["base"] == evaluate(m, loader, topk=3)
    assert np.isnan(res["acc1"][0][1]) and np.isnan(res["acck"][0][1])
    for row, block in enumerate((0, 3)):
        for col, what in enumerate(("attn", "ffn")):
            if (block, what) == (0, "ffn"):
                continue
            skips = {0: "block"} if block == 0 else {0: "ffn", 3: what}
            with m.skipping(skips):
                r = evaluate(m, loader, topk=3)
            assert (res["acc1"][row][col], res["acck"][row][col]) == (r["acc1"], r["acck"])
