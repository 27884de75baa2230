"""GPU: token pruning (include/evt_token_pruning.h; csrc/token_pruning.hip, encoder.cpp).

Op level. evt_token_scores is bitwise the head-ordered fp32 sum of the CLS rows evt_attention_probs
exports (both qkv layouts, both dtypes, head sizes 8 / 64 / 80); evt_token_select equals
`select_tokens_reference` exactly on random, tied, constant, signed-zero and NaN scores at every
slot and wave edge up to 4096 tokens; evt_token_gather is a bitwise row and statistics copy for
widths that are and are not multiples of 64. Inputs and outputs sit inside sentinel-filled
allocations: a read or a write outside shows.

Model level (set_token_pruning / token_pruning_outputs / evt_forward_token_pruning) on the tiny
models of tests/test_gpu_head_stats.py and a 290-token ViT whose schedule crosses 256 tokens and
lands on 64. Three independent claims (tests/_token_pruning_ref.py): the scores are within H times
the attention-map gate of the fp64 reference's, the kept table is exactly the stable top-K of the
exported scores, and the logits pass the project's gates against the reference that keeps the
device's rows. Bitwise: K = T - 1 everywhere is the unscheduled forward; one image alone, lanes,
the QKV layout, graph replay, uint8 input and a second call change nothing; clearing the schedule
restores the unscheduled logits.
"""
import ctypes

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import Uint8Images, _lib
from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer
from edgevisiontransformer_amd.modeling.models.token_pruning import select_tokens_reference
from edgevisiontransformer_amd.modeling.models.vit import ViT
from edgevisiontransformer_amd.weights import (make_images, make_std_vit_params, make_swin_params,
                                               make_vit_params, swin_config)
from tests import _token_pruning_ref as tref
from tests._ops import TDT, _p, _s
from tests.test_gpu_attention_maps import MODEL_BF16_ERR_MEASURED, _op_inputs, _probs
from tests.test_gpu_features import _cos_rows
from tests.test_gpu_head_stats import _pruned, _std, _t2t, _vit
from tests.test_gpu_model import BF16_ABS, BF16_COS, F32_TOL

pytestmark = pytest.mark.gpu
PAD = 64  # sentinel elements before and after every op-level buffer
INT_SENTINEL = -7


def _guarded(shape, dtype, gpu, src=None):
    """A [shape] view inside a sentinel-filled (NaN, or -7 for integers) allocation; 16-byte
    aligned for every dtype used here (PAD elements of >= 2 bytes... 64 * 2 = 128 bytes)."""
    n = int(np.prod(shape))
    fill = INT_SENTINEL if dtype == torch.int32 else float("nan")
    flat = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=gpu)
    view = flat[PAD:PAD + n].view(*shape)
    if src is not None:
        view.copy_(src.to(gpu))
    return flat, view


def _is_sentinel(t):
    return t == INT_SENTINEL if t.dtype == torch.int32 else torch.isnan(t)


def _intact(flat, filled=True):
    """Both pads untouched; with `filled`, no sentinel left inside."""
    ok = bool(_is_sentinel(flat[:PAD]).all()) and bool(_is_sentinel(flat[-PAD:]).all())
    return ok and (not filled or not bool(_is_sentinel(flat[PAD:-PAD]).any()))


# ---- op level: scores -----------------------------------------------------------------------------
def _scores(dtype, qkv, b, n, h, hd, gpu, head_major=False):
    if head_major:  # [B][H][q | k | v][N][64]
        qkv = qkv.view(b, n, 3, h, 64).permute(0, 3, 2, 1, 4).contiguous()
        ldq, sb, sh, ko = 64, 3 * h * n * 64, 3 * n * 64, n * 64
    else:
        ldq, sb, sh, ko = qkv.shape[1], 0, 0, 0
    holder, dev = _guarded(qkv.shape, qkv.dtype, gpu, qkv)
    flat, out = _guarded((b, n), torch.float32, gpu)
    _lib.check(_lib.load_library().evt_token_scores(
        _lib.DTYPE[dtype], _p(dev), ldq, sb, sh, ko, b, n, h, hd, hd ** -0.5, _p(out), _s()))
    torch.cuda.synchronize()
    assert _intact(flat), "NaN left in the scores (or read past qkv) or a write outside them"
    del holder
    return out


def _head_sum(p):
    """sum_h p[:, h] in fp32, heads added in index order starting from 0."""
    acc = torch.zeros_like(p[:, 0])
    for h in range(p.shape[1]):
        acc = acc + p[:, h]
    return acc


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", [(2, 3, 65, 64), (2, 2, 257, 64), (1, 2, 64, 80), (1, 1, 2, 8)],
                         ids=lambda c: "x".join(map(str, c)))
def test_scores_are_head_ordered_sum_of_export(gpu, case, dtype):
    b, h, n, hd = case
    qkv, _ = _op_inputs(b, h, n, hd, dtype, 1.0)
    p = _probs(dtype, qkv, b, n, h, hd, 1, gpu)  # [B, H, 1, N]
    want = _head_sum(p[:, :, 0, :])
    got = _scores(dtype, qkv, b, n, h, hd, gpu)
    assert torch.equal(got, want)
    assert torch.equal(_scores(dtype, qkv, b, n, h, hd, gpu), got), "second launch differs"
    if b > 1:
        alone = _scores(dtype, qkv[:n].contiguous(), 1, n, h, hd, gpu)
        assert torch.equal(alone[0], got[0]), "image 0 alone differs from inside the batch"
    if dtype == "bf16" and hd == 64:
        assert torch.equal(_scores(dtype, qkv, b, n, h, hd, gpu, head_major=True), got), \
            "head-major differs from token-major"


# ---- op level: select -----------------------------------------------------------------------------
def _select_inputs(n):
    rng = np.random.default_rng(500 + n)
    nan = np.float32("nan")
    rnd = rng.standard_normal((2, n)).astype(np.float32)
    ties = np.stack([np.resize(rng.standard_normal(8).astype(np.float32), n) for _ in range(2)])
    zeros = np.where(rng.random((2, n)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    zeros[:, ::7] = rng.standard_normal(zeros[:, ::7].shape).astype(np.float32)
    some_nan = rnd.copy()
    some_nan[rng.random((2, n)) < 0.3] = nan
    some_nan[1, n // 2:] = nan
    return {"random": rnd, "ties": ties, "equal": np.full((2, n), 0.125, dtype=np.float32),
            "zeros": zeros, "nan": some_nan}


@pytest.mark.parametrize("n", [2, 64, 65, 257, 4096])
def test_select_is_the_reference(gpu, n):
    lib = _lib.load_library()
    for kind, s in _select_inputs(n).items():
        holder, dev = _guarded(s.shape, torch.float32, gpu, torch.from_numpy(s))
        for k in sorted({1, max(1, n // 2), max(1, n - 2), n - 1}):
            flat, kept = _guarded((2, k + 1), torch.int32, gpu)
            _lib.check(lib.evt_token_select(_p(dev), 2, n, k, _p(kept), _s()))
            torch.cuda.synchronize()
            assert _intact(flat), f"{kind} K={k}: an entry not written, or a write outside kept"
            assert np.array_equal(kept.cpu().numpy(), select_tokens_reference(s, k)), (kind, k)
        del holder


# ---- op level: gather -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("d", [64, 192, 200])
def test_gather_is_a_bitwise_copy(gpu, d, dtype):
    lib = _lib.load_library()
    b, t, k1, slots = 2, 65, 17, 2
    rng = np.random.default_rng(d)
    x = torch.from_numpy(rng.standard_normal((b * t, d)).astype(np.float32)).to(TDT[dtype])
    st = torch.from_numpy(rng.standard_normal((b * t, slots, 2)).astype(np.float32))
    kept = np.stack([np.concatenate([[0], np.sort(rng.choice(np.arange(1, t), k1 - 1, False))])
                     for _ in range(b)]).astype(np.int32)
    hx, dx = _guarded(x.shape, x.dtype, gpu, x)
    hs, ds = _guarded(st.shape, torch.float32, gpu, st)
    hk, dk = _guarded(kept.shape, torch.int32, gpu, torch.from_numpy(kept))
    fo, out = _guarded((b * k1, d), x.dtype, gpu)
    fs, sout = _guarded((b * k1, slots, 2), torch.float32, gpu)
    _lib.check(lib.evt_token_gather(_lib.DTYPE[dtype], _p(dx), _p(out), _p(ds), _p(sout), slots,
                                    _p(dk), b, t, k1, d, _s()))
    torch.cuda.synchronize()
    assert _intact(fo) and _intact(fs), "a row not written, or a write outside the destination"
    assert _intact(hx) and _intact(hs) and _intact(hk), "the gather wrote to a source"
    rows = (np.arange(b)[:, None] * t + kept).reshape(-1)
    assert torch.equal(out.cpu().view(torch.int16 if dtype == "bf16" else torch.int32),
                       x[rows].view(torch.int16 if dtype == "bf16" else torch.int32))
    assert torch.equal(sout.cpu(), st[rows])
    # rows alone (no statistics), then the refusals: in place, and a destination inside the source
    fo2, out2 = _guarded((b * k1, d), x.dtype, gpu)
    _lib.check(lib.evt_token_gather(_lib.DTYPE[dtype], _p(dx), _p(out2), None, None, 0, _p(dk), b,
                                    t, k1, d, _s()))
    torch.cuda.synchronize()
    assert _intact(fo2) and torch.equal(out2, out)
    for dst in (dx, dx[t:]):
        assert lib.evt_token_gather(_lib.DTYPE[dtype], _p(dx), _p(dst), None, None, 0, _p(dk), b,
                                    t, k1, d, _s()) == _lib.EVT_EINVAL
        assert "overlap" in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(dx.cpu().view(torch.int16 if dtype == "bf16" else torch.int32),
                       x.view(torch.int16 if dtype == "bf16" else torch.int32))


# ---- model level ----------------------------------------------------------------------------------
def _wide(dtype, lanes, gpu):  # 290 tokens: 290 -> 256 -> 64 crosses the streaming / one-pass edge
    return ViT(dim=128, depth=3, heads=2, mlp_dim=256, image_size=68, patch_size=4, num_classes=16,
               dtype=dtype, seed=76, device=gpu, max_batch=2, lanes=lanes)


# name -> (factory, image size, schedule, parameter generator, seed, standard semantics)
CASES = {"vit": (_vit, 32, {0: 40, 1: 17}, make_vit_params, 71, False),
         "std": (_std, 64, {0: 0.5}, make_std_vit_params, 73, True),
         "pruned": (_pruned, 64, {1: 8}, make_vit_params, 72, False),
         "wide": (_wide, 68, {0: 255, 1: 63}, make_vit_params, 76, False)}


def _image(name, gpu, batch=2):
    return torch.from_numpy(make_images(batch, seed=75, image_size=CASES[name][1])).to(gpu)


def _outputs(m, x, pooled=False):
    out = m.token_pruning_outputs(x, logits=True, pooled=pooled)
    torch.cuda.synchronize()
    return out


def _same(a, b):
    return torch.equal(a["logits"], b["logits"]) and \
        all(torch.equal(u, v) for u, v in zip(a["scores"], b["scores"])) and \
        all(torch.equal(u, v) for u, v in zip(a["kept"], b["kept"]))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_model_token_pruning(gpu, name, dtype):
    make, _, schedule, gen, seed, standard = CASES[name]
    m = make(dtype, 1, gpu)
    x = _image(name, gpu)
    cfg, depth = m.cfg, m.cfg.depth
    plain, pooled = m(x).clone(), m.forward_features(x).clone()
    ws = m.allocated_workspace_bytes()
    first = min(schedule)
    cls_map = m.attention_maps(x, blocks=(first,), queries="cls")["maps"][0]  # [B, H, T]

    # identity: every patch token kept after every block that can be scheduled
    m.set_token_pruning({l: 1.0 for l in range(depth - 1)})
    ident = _outputs(m, x, pooled=True)
    assert torch.equal(ident["logits"], plain) and torch.equal(ident["pooled"], pooled)
    ar = torch.arange(cfg.tokens, dtype=torch.int32, device=gpu).expand(x.shape[0], -1)
    assert all(torch.equal(k, ar) for k in ident["kept"])
    assert torch.equal(ident["token_index"], ar.long())

    m.set_token_pruning(schedule)
    sched = m.token_schedule()
    assert m.allocated_workspace_bytes() == ws
    assert [m.tokens_at(b_) for b_, _, _, _ in sched] == [t for _, _, t, _ in sched]
    assert m.tokens_at(-1) == sched[-1][3]
    out = _outputs(m, x, pooled=True)
    assert torch.isfinite(out["logits"]).all() and torch.isfinite(out["pooled"]).all()

    # selection: exactly the stable top-K of the exported scores
    kept = [k.cpu().numpy() for k in out["kept"]]
    for (blk, k, t_in, t_out), s, kk in zip(sched, out["scores"], kept):
        assert tuple(s.shape) == (x.shape[0], t_in) and kk.shape == (x.shape[0], t_out)
        assert np.array_equal(kk, select_tokens_reference(s.cpu().numpy(), k)), f"block {blk}"
    index = np.broadcast_to(np.arange(cfg.tokens), (x.shape[0], cfg.tokens))
    for kk in kept:
        index = np.take_along_axis(index, kk.astype(np.int64), axis=1)
    assert np.array_equal(out["token_index"].cpu().numpy(), index)

    # scores: the first scheduled block sees the unscheduled stream, so bitwise the exported maps'
    assert torch.equal(out["scores"][0], _head_sum(cls_map))
    # ... and every block's are within H gates of one exported probability of the fp64 reference's
    ref_logits, ref_scores = tref.forward(gen(cfg, seed=seed), cfg, x.cpu().numpy(), sched, kept,
                                          standard=standard)
    gate = 1e-3 if dtype == "f32" else 2 * MODEL_BF16_ERR_MEASURED
    for (blk, _, _, _), s, r in zip(sched, out["scores"], ref_scores):
        err = np.abs(s.double().cpu().numpy() - r).max()
        heads = cfg.heads[blk]
        print(f"TOKENPRUNE-SCORES {name} {dtype} block {blk}: max-abs {err:.3e} "
              f"(gate {heads} x {gate:.3e})")
        assert err <= heads * gate, f"block {blk}: {err:.3e}"

    # logits: the project's gates against the reference that keeps the device's rows
    got = out["logits"].double().cpu().numpy()
    err, cos = np.abs(got - ref_logits).max(), _cos_rows(got, ref_logits).min()
    print(f"TOKENPRUNE-LOGITS {name} {dtype}: max-abs {err:.3e} min cos {cos:.6f}")
    if dtype == "f32":
        assert err <= F32_TOL, f"f32 max-abs {err:.3e}"
    else:
        assert err <= BF16_ABS and cos >= BF16_COS, f"bf16 max-abs {err:.3e}, min cos {cos:.6f}"

    # bitwise: the plain forwards run the same schedule; a second call; one image alone
    assert torch.equal(m(x), out["logits"])
    assert torch.equal(m.forward_features(x), out["pooled"])
    assert _same(_outputs(m, x), out)
    alone = _outputs(m, x[:1].contiguous())
    assert torch.equal(alone["logits"][0], out["logits"][0])
    assert all(torch.equal(u[0], v[0]) for u, v in zip(alone["scores"], out["scores"]))
    assert all(torch.equal(u[0], v[0]) for u, v in zip(alone["kept"], out["kept"]))

    # clearing restores the unscheduled forward
    m.set_token_pruning(None)
    assert m.token_schedule() == [] and m.tokens_at(-1) == cfg.tokens
    assert torch.equal(m(x), plain) and m.allocated_workspace_bytes() == ws
    assert torch.equal(m.attention_maps(x, blocks=(first,), queries="cls")["maps"][0], cls_map)


@pytest.mark.parametrize("name", ["vit", "wide"])
def test_lanes_layout_and_graph(gpu, name, monkeypatch):
    make, _, schedule, *_ = CASES[name]
    x = _image(name, gpu)
    m = make("bf16", 1, gpu)
    m.set_token_pruning(schedule)
    out = _outputs(m, x)
    # lanes = 2: the plain forward splits the batch, the exporting forward runs as one lane
    m2 = make("bf16", 2, gpu)
    m2.set_token_pruning(schedule)
    assert m2.lanes() == 2
    assert torch.equal(m2(x), out["logits"]) and _same(_outputs(m2, x), out)
    # a schedule set before the lanes is inherited by them (the constructor keyword)
    m3 = ViT(**_CTOR[name], dtype="bf16", device=gpu, max_batch=2, lanes=2, token_keep=schedule)
    assert m3.token_schedule() == m.token_schedule() and torch.equal(m3(x), out["logits"])
    # token-major QKV
    monkeypatch.setenv("EVT_QKV_LAYOUT", "token")
    mt = make("bf16", 1, gpu)
    monkeypatch.delenv("EVT_QKV_LAYOUT")
    mt.set_token_pruning(schedule)
    assert _same(_outputs(mt, x), out) and mt.qkv_headmajor_layers() == 0
    # graph replay, and no schedule change once a graph is captured
    xin, logits = x.clone(), torch.empty_like(out["logits"])
    m.capture_graph(xin, logits)
    m.replay_graph()
    torch.cuda.synchronize()
    assert torch.equal(logits, out["logits"])
    with pytest.raises(ValueError, match="before evt_graph_capture"):
        m.set_token_pruning({0: 8})
    assert m.token_schedule() == out_schedule(m, schedule)


_CTOR = {"vit": dict(dim=192, depth=3, heads=3, mlp_dim=768, image_size=32, patch_size=4,
                     num_classes=16, seed=71),
         "wide": dict(dim=128, depth=3, heads=2, mlp_dim=256, image_size=68, patch_size=4,
                      num_classes=16, seed=76)}


def out_schedule(m, schedule):
    from edgevisiontransformer_amd.modeling.models.token_pruning import schedule_tokens
    return schedule_tokens(m.cfg.tokens, m.cfg.depth, schedule)


def test_uint8_numpy_profile_and_rebuild(gpu):
    m = _vit("bf16", 1, gpu)
    schedule = CASES["vit"][2]
    m.set_token_pruning(schedule)
    rng = np.random.default_rng(7)
    u8 = Uint8Images(torch.from_numpy(rng.integers(0, 256, (2, 32, 32, 3), dtype=np.uint8)).to(gpu))
    xf = u8.to_float("nchw")
    want = _outputs(m, xf)
    assert _same(_outputs(m, u8), want) and torch.equal(m(u8), want["logits"])
    host = m.token_pruning_outputs(xf.cpu().numpy())
    assert isinstance(host["logits"], np.ndarray) and isinstance(host["kept"][0], np.ndarray)
    assert np.array_equal(host["logits"], want["logits"].cpu().numpy())
    assert np.array_equal(host["token_index"], want["token_index"].cpu().numpy())
    assert torch.equal(m.classify(xf, topk=3, logits=True)["logits"], want["logits"])

    # profiling: three launches per scheduled block, all under EVT_PROF_HEAD
    lib = _lib.load_library()
    head = _lib.PROF_ROLES.index("head")
    us = (ctypes.c_float * len(_lib.PROF_ROLES))()
    n = (ctypes.c_int * len(_lib.PROF_ROLES))()

    def launches():
        _lib.check(lib.evt_model_profile(ctypes.c_void_p(m._handle), 1))
        got = m(xf)
        torch.cuda.synchronize()
        _lib.check(lib.evt_model_profile_read(ctypes.c_void_p(m._handle), us, n))
        _lib.check(lib.evt_model_profile(ctypes.c_void_p(m._handle), 0))
        return list(n), got
    with_s, got = launches()
    assert torch.equal(got, want["logits"])
    m.set_token_pruning(None)
    without, _ = launches()
    assert with_s[head] == without[head] + 3 * len(schedule)
    assert [v for i, v in enumerate(with_s) if i != head] == \
        [v for i, v in enumerate(without) if i != head]

    # the schedule survives a rebuild of the handle for a larger batch
    small = ViT(**_CTOR["vit"], dtype="bf16", device=gpu, max_batch=1, lanes=1, token_keep=schedule)
    assert torch.equal(small(xf), want["logits"])  # batch 2 > max_batch 1: _fit rebuilds
    cnt = ctypes.c_int()
    blocks, keep = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    _lib.check(lib.evt_model_token_schedule(small._ptr(), ctypes.byref(cnt), blocks, keep, 4))
    assert (cnt.value, list(blocks[:2]), list(keep[:2])) == (2, [0, 1], [40, 17])
    t = ctypes.c_int()
    _lib.check(lib.evt_model_tokens_at(small._ptr(), 2, ctypes.byref(t)))
    assert t.value == 18


def test_refusals(gpu):
    m = _vit("bf16", 1, gpu)
    x = _image("vit", gpu)
    with pytest.raises(ValueError, match="no token schedule"):
        m.token_pruning_outputs(x)
    m.set_token_pruning(CASES["vit"][2])
    for call in (lambda: m.attention_maps(x), lambda: m.head_stats(x),
                 lambda: m.attention_rollout(x), lambda: m.ffn_stats(x),
                 lambda: m.features(x, tokens=True), lambda: m.features(x, taps=(0,))):
        with pytest.raises(ValueError, match="token schedule"):
            call()
    assert tuple(m.forward_features(x).shape) == (2, m.feature_dim)  # pooled stays available
    for bad in ({2: 8}, {0: 65}, {0: 40, 1: 41}, {0: 0}):
        with pytest.raises(ValueError):
            m.set_token_pruning(bad)
    assert m.token_schedule() == out_schedule(m, CASES["vit"][2])
    # the C ABI: its own range checks, the export list's length, a features forward with tokens
    lib = _lib.load_library()
    one = lambda v: (ctypes.c_int32 * 1)(v)  # noqa: E731
    two = lambda a, b: (ctypes.c_int32 * 2)(a, b)  # noqa: E731
    E = _lib.EVT_EINVAL
    assert lib.evt_model_set_token_schedule(m._ptr(), 1, one(2), one(8), None) == E
    assert lib.evt_model_set_token_schedule(m._ptr(), 1, one(0), one(65), None) == E
    assert lib.evt_model_set_token_schedule(m._ptr(), 2, two(1, 0), two(8, 8), None) == E
    assert "ascending" in _lib.last_error()
    assert lib.evt_model_set_token_schedule(m._ptr(), 1, None, None, None) == E
    assert lib.evt_model_set_token_schedule(m._ptr(), 65, one(0), one(8), None) == E
    args = _lib.evt_image_args()
    args.data = x.data_ptr()
    logits = torch.empty((2, 16), device=gpu)
    feat = _lib.evt_features_args()
    feat.logits = logits.data_ptr()
    tp = _lib.evt_token_pruning_args()
    tp.n_blocks = 1
    assert lib.evt_forward_token_pruning(m._ptr(), ctypes.byref(args), 2, ctypes.byref(feat),
                                         ctypes.byref(tp), None) == E
    tok = torch.empty((2, 65, 192), device=gpu)
    feat.tokens = tok.data_ptr()
    assert lib.evt_forward_token_pruning(m._ptr(), ctypes.byref(args), 2, ctypes.byref(feat), None,
                                         None) == E
    assert "token schedule" in _lib.last_error()
    # the other families and mx8
    cfg = swin_config("tiny", image_size=56, window_size=7, depths=(2, 2), num_heads=(3, 6),
                      num_classes=11)
    sw = SwinTransformer(img_size=56, patch_size=cfg.patch_size, num_classes=11,
                         embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
                         window_size=7, dtype="bf16", weights=make_swin_params(cfg, seed=3),
                         device=gpu, max_batch=1, lanes=1)
    m8 = ViT(dim=128, depth=2, heads=2, mlp_dim=256, image_size=32, patch_size=16, num_classes=16,
             dtype="mx8", device=gpu, max_batch=1, lanes=1)
    t2t = _t2t("bf16", 1, gpu)
    for model in (sw, m8, t2t):
        with pytest.raises(ValueError):
            model.set_token_pruning({0: 2})
        assert lib.evt_model_set_token_schedule(model._ptr(), 1, one(0), one(2), None) == E
    with pytest.raises(ValueError, match="mx8"):
        ViT(dim=128, depth=2, heads=2, mlp_dim=256, image_size=32, patch_size=16, num_classes=16,
            dtype="mx8", device=gpu, max_batch=1, lanes=1, token_keep={0: 2})
