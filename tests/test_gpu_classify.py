"""GPU: classification outputs (include/evt_classify.h; the classify kernel of csrc/features.hip).

Op level (evt_classify) against `classify_reference` (numpy fp64 on the same fp32 logits) at the
smallest shapes at which the kernel (one wave per row, 4-class chunks per lane, four rows per
block) can go wrong. Every case runs twice, with the logits 16-byte aligned and one float past
that (rows then start at every 4-byte phase; padding columns and the surroundings are NaN, so a
read outside a row shows in the probabilities), and both runs must give the same bits. Indices,
ranks, LOGIT values and counters are exact. Probabilities and lse are gated by the fp32 error
bound of the formula (u = 2^-24):

    |p - p64|     <= (C + 2 |l_i - m| + 16) u p64 + 1e-37
    |lse - lse64| <= (C + 16) u + 2 u |lse64|

(a length-C positive sum in any order: (C - 1) u; the rounded l_i - m: u |l_i - m| into exp, twice
for its two roundings; a few ulp for exp, the scale and the divide). Measured on an MI355X on the
first run of this file, largest error / bound over every case here: see DESIGN.md, "Classification
outputs".

Model level: classify / classify_into / classify_logits / evaluate on small models of each family.
"""
import ctypes

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import Uint8Images, _lib, evaluate
from edgevisiontransformer_amd.modeling.models.classify import classify_reference
from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer
from edgevisiontransformer_amd.modeling.models.t2t_vit import T2T_ViT
from edgevisiontransformer_amd.modeling.models.vit import ViT
from edgevisiontransformer_amd.weights import (make_images, make_swin_params, make_t2t_params,
                                               make_vit_params, swin_config, t2t_config,
                                               vit_config)
from tests._ops import _p, _s

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 64
SENT_I, SENT_F = -77, 7.25  # what the outputs hold before a call


# ---- guarded outputs ------------------------------------------------------------------------------
def _buf(shape, dtype, gpu):
    n = int(np.prod(shape))
    flat = torch.full((n + GUARD,), SENT_F if dtype == torch.float32 else SENT_I, dtype=dtype,
                      device=gpu)
    return flat, flat[:n].view(*shape)


def _guard_ok(flat, n):
    return bool((flat[n:] == (SENT_F if flat.dtype == torch.float32 else SENT_I)).all())


def _untouched(flat):
    return _guard_ok(flat, 0)


def _place(logits, ldl, shift, gpu):
    """logits [B, C] on the device as rows ldl apart, starting `shift` floats past a 16-byte
    aligned address, everything around them NaN: (holder, pointer tensor)."""
    b, c = logits.shape
    flat = torch.full((GUARD + shift + b * ldl + GUARD,), float("nan"), device=gpu)
    assert flat.data_ptr() % 16 == 0
    view = flat[GUARD + shift:GUARD + shift + b * ldl].view(b, ldl)
    view[:, :c] = torch.from_numpy(logits).to(gpu)
    return flat, view


def _classify(view, c, k, values, gpu, labels=None, counters=None, want=("indices", "vals", "lse")):
    """evt_classify into guarded, sentinel-filled buffers -> dict of numpy arrays."""
    b, ldl = view.shape
    a = _lib.evt_classify_args()
    a.k, a.values = k, values
    bufs = {}
    for name, shape, dt in (("indices", (b, k), torch.int32), ("vals", (b, k), torch.float32),
                            ("lse", (b,), torch.float32)):
        if name in want:
            bufs[name] = _buf(shape, dt, gpu)
            setattr(a, name, bufs[name][1].data_ptr())
    if labels is not None:
        y = torch.from_numpy(np.asarray(labels, np.int32)).to(gpu)
        bufs["rank"] = _buf((b,), torch.int32, gpu)
        a.labels, a.rank = y.data_ptr(), bufs["rank"][1].data_ptr()
        if counters is not None:
            a.counters = counters.data_ptr()
    _lib.check(_lib.load_library().evt_classify(_p(view), ldl, b, c, ctypes.byref(a), _s()))
    torch.cuda.synchronize()
    out = {}
    for name, (flat, t) in bufs.items():
        assert _guard_ok(flat, t.numel()), f"{name}: guard words overwritten"
        out[name] = t.cpu().numpy()
    return out


def _gate_probs(what, got, ref, logits):
    """The error-bound gates of the module docstring on finite rows; prints the largest ratio."""
    c = logits.shape[1]
    l64 = logits.astype(np.float64)
    m = l64.max(1, keepdims=True)
    li = np.take_along_axis(l64, ref["indices"].astype(np.int64), 1)
    # a -inf entry has p64 == 0 exactly: its relative term is 0 (not inf * 0)
    rel = np.where(ref["prob"] > 0, (c + 2 * np.abs(li - m) + 16) * U, 0.0) * ref["prob"]
    bound = rel + 1e-37
    err = np.abs(got["vals"].astype(np.float64) - ref["prob"])
    lbound = (c + 16) * U + 2 * U * np.abs(ref["lse"])
    lerr = np.abs(got["lse"].astype(np.float64) - ref["lse"])
    print(f"CLASSIFY {what}: max p err/bound {np.max(err / bound):.3f} (max rel err "
          f"{np.max(np.where(ref['prob'] > 1e-30, err / np.maximum(ref['prob'], 1e-30), 0)) / U:.2f}"
          f" u), max lse err/bound "
          f"{np.max(lerr / lbound):.4f} (max abs {lerr.max() / U:.2f} u)")
    assert np.isfinite(got["vals"]).all() and np.isfinite(got["lse"]).all()
    assert (err <= bound).all(), f"p error {np.max(err / bound):.3f} of the bound"
    assert (lerr <= lbound).all(), f"lse error {np.max(lerr / lbound):.3f} of the bound"
    if got["vals"].shape[1] == c:  # k = C: the probabilities of a row sum to 1
        sbound = rel.sum(1) + 1e-37
        serr = np.abs(got["vals"].astype(np.float64).sum(1) - 1.0)
        print(f"CLASSIFY {what}: max |sum p - 1| {serr.max():.3e} (bound {sbound.min():.3e})")
        assert (serr <= sbound).all()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b, perm=None):
    assert a.keys() == b.keys()
    for key in a:
        v = b[key] if perm is None else b[key][perm]
        assert np.array_equal(_bits(a[key]), _bits(v)), f"{key} differs"


# ---- op level: shapes -----------------------------------------------------------------------------
OP_CASES = [(1, 1, 1, 1), (5, 3, 3, 3), (3, 10, 10, 10), (5, 63, 64, 5), (5, 64, 64, 32),
            (5, 65, 72, 32), (130, 1000, 1000, 5), (7, 1003, 1008, 5), (3, 4099, 4099, 8),
            (2, 21841, 21841, 5)]


def _labels(rng, b, c):
    y = rng.integers(0, c, b)
    if b >= 3:
        y[1], y[2] = -1, c  # no label; out of range
    return y.astype(np.int32)


@pytest.mark.parametrize("case", OP_CASES, ids=lambda c: "x".join(map(str, c)))
def test_classify_op(gpu, case):
    B, C, ldl, k = case
    rng = np.random.default_rng(C * 131 + B)
    logits = (rng.standard_normal((B, C)) * 3).astype(np.float32)
    y = _labels(rng, B, C)
    ref = classify_reference(logits, k, labels=y)
    outs = []
    for shift in (0, 1):
        holder, view = _place(logits, ldl, shift, gpu)
        counters = torch.tensor([10, 20, 30], dtype=torch.int64, device=gpu)
        got = _classify(view, C, k, _lib.CLASSIFY_PROB, gpu, labels=y, counters=counters)
        lg = _classify(view, C, k, _lib.CLASSIFY_LOGIT, gpu, labels=y, counters=counters)
        # two accumulating calls into the same buffer
        assert counters.cpu().numpy().tolist() == (np.array([10, 20, 30]) + 2 * ref["counters"]).tolist()
        assert np.array_equal(got["indices"], ref["indices"])
        assert np.array_equal(got["rank"], ref["rank"])
        assert np.array_equal(lg["indices"], ref["indices"]) and np.array_equal(lg["rank"], ref["rank"])
        assert np.array_equal(_bits(lg["vals"]), _bits(ref["logit"]))
        assert np.array_equal(_bits(lg["lse"]), _bits(got["lse"]))
        _gate_probs(f"B{B} C{C} ldl{ldl} k{k} shift{shift}", got, ref, logits)
        _same_bits(got, _classify(view, C, k, _lib.CLASSIFY_PROB, gpu, labels=y))  # repeated
        outs.append(got)
        if B > 1:  # a permuted batch gives the same rows, permuted
            perm = np.roll(np.arange(B), 1)
            h2, v2 = _place(logits[perm], ldl, shift, gpu)
            _same_bits(_classify(v2, C, k, _lib.CLASSIFY_PROB, gpu, labels=y[perm]), got, perm)
        # each output alone gives the bits it has among the others
        for name in ("indices", "vals", "lse"):
            alone = _classify(view, C, k, _lib.CLASSIFY_PROB, gpu, want=(name,))
            assert np.array_equal(_bits(alone[name]), _bits(got[name])), name
        del holder
    _same_bits(outs[0], outs[1])  # the bits do not depend on the rows' alignment


# ---- op level: adversarial rows -------------------------------------------------------------------
def _adversarial(C):
    rng = np.random.default_rng(9)
    base = (rng.standard_normal(C) * 2).astype(np.float32)
    rows, labels = {}, {}
    rows["all equal"], labels["all equal"] = np.full(C, 0.75, np.float32), 3
    r = base.copy()
    r[[0, 63, 64, 65, C - 1]] = 9.0  # above everything else
    rows["repeated top"], labels["repeated top"] = r, 64  # a tie that includes the label
    r = base.copy()
    r[[0, 63, 64, 65, C - 1]] = -9.0  # below everything else
    rows["repeated bottom"], labels["repeated bottom"] = r, C - 1
    r = -np.abs(base) - 1
    r[[2, 70, 5, 64]] = [0.0, -0.0, -0.0, 0.0]
    rows["signed zeros"], labels["signed zeros"] = r.astype(np.float32), 64
    r = np.full(C, -np.inf, np.float32)
    r[77] = 1.25
    rows["all but one -inf"], labels["all but one -inf"] = r, 0
    r = base.copy()
    r[0], r[100] = np.nan, np.nan
    rows["NaN at class 0"], labels["NaN at class 0"] = r, 0
    r = base.copy()
    r[5], r[6] = np.inf, -np.inf
    rows["+inf and -inf"], labels["+inf and -inf"] = r, 6
    rows["magnitudes of 1e4"] = (rng.standard_normal(C) * 1e4).astype(np.float32)
    labels["magnitudes of 1e4"] = -1
    rows["label C"], labels["label C"] = base.copy(), C
    return rows, labels


def test_classify_adversarial_rows(gpu):
    C, k = 130, 8
    rows, labels = _adversarial(C)
    names = list(rows)
    logits = np.stack([rows[n] for n in names])
    y = np.array([labels[n] for n in names], np.int32)
    ref = classify_reference(logits, k, labels=y)
    assert ref["indices"][0].tolist() == list(range(k))  # all equal: 0 .. k-1
    assert ref["indices"][1][:5].tolist() == [0, 63, 64, 65, C - 1] and ref["rank"][1] == 2
    assert ref["indices"][3][:4].tolist() == [2, 5, 64, 70]  # -0.0 == +0.0: by index
    assert ref["rank"][5] == C - 2 and ref["rank"][8] == -1  # NaN last, by index
    for shift in (0, 1):
        holder, view = _place(logits, C + 2, shift, gpu)
        counters = torch.zeros(3, dtype=torch.int64, device=gpu)
        got = _classify(view, C, k, _lib.CLASSIFY_PROB, gpu, labels=y, counters=counters)
        lg = _classify(view, C, k, _lib.CLASSIFY_LOGIT, gpu, labels=y)
        for i, n in enumerate(names):
            assert got["indices"][i].tolist() == ref["indices"][i].tolist(), n
            assert got["rank"][i] == ref["rank"][i], n
            assert np.array_equal(_bits(lg["vals"][i]), _bits(ref["logit"][i])), n
        assert counters.cpu().numpy().tolist() == ref["counters"].tolist()
        finite = [i for i, n in enumerate(names) if np.isfinite(ref["prob"][i]).all()
                  and np.isfinite(ref["lse"][i])]
        assert {names[i] for i in finite} >= {"all equal", "repeated top", "signed zeros",
                                              "all but one -inf", "magnitudes of 1e4"}
        sub = lambda d: {key: v[finite] for key, v in d.items() if key != "counters"}  # noqa: E731
        _gate_probs(f"adversarial shift{shift}", sub(got), sub(ref), logits[finite])
        i = names.index("all but one -inf")  # exactly 0 at the -inf entries, 1 at the finite one
        assert got["vals"][i].tolist() == [1.0] + [0.0] * (k - 1) and got["lse"][i] == 1.25
        del holder


def test_classify_wide_spread_k_equals_c(gpu):
    """Logits spread over +-60 with k = C = 10: the small probabilities are far below one ulp of
    the large ones; the relative bound holds for each."""
    rng = np.random.default_rng(3)
    logits = rng.uniform(-60, 60, (6, 10)).astype(np.float32)
    logits[0] = np.linspace(-60, 60, 10)
    ref = classify_reference(logits, 10)
    for shift in (0, 1):
        holder, view = _place(logits, 10, shift, gpu)
        got = _classify(view, 10, 10, _lib.CLASSIFY_PROB, gpu)
        assert np.array_equal(got["indices"], ref["indices"])
        _gate_probs(f"spread shift{shift}", got, ref, logits)
        del holder


# ---- model level ----------------------------------------------------------------------------------
GEO = dict(dim=128, depth=2, heads=2, mlp_dim=256, image_size=32, patch_size=16, num_classes=16)
LANES_BATCH = 130  # >= _lib.LANES_MIN_BATCH, not a multiple of 4


def _vit(dtype, gpu, max_batch, lanes=None):
    cfg = vit_config(128, 2, 2, 256, image_size=32, patch_size=16, num_classes=16)
    return ViT(dtype=dtype, device=gpu, max_batch=max_batch, lanes=lanes,
               weights=make_vit_params(cfg, seed=51), **GEO)


def _check_model(m, x, k, what):
    """classify(x) against classify_reference(model(x)); -> the classify output (tensors)."""
    b = x.shape[0]
    plain = m(x)
    ref_logits = plain.cpu().numpy()
    rng = np.random.default_rng(b)
    y = rng.integers(-1, m.cfg.num_classes + 1, b)
    ref = classify_reference(ref_logits, k, labels=y)
    out = m.classify(x, topk=k, labels=y, logits=True)
    assert torch.equal(out["logits"], plain), "logits differ from model(img)"
    got = {"indices": out["indices"].cpu().numpy(), "vals": out["values"].cpu().numpy(),
           "lse": out["lse"].cpu().numpy(), "rank": out["rank"].cpu().numpy()}
    assert got["indices"].dtype == np.int32 and got["rank"].dtype == np.int32
    assert np.array_equal(got["indices"], ref["indices"]) and np.array_equal(got["rank"], ref["rank"])
    _gate_probs(what, got, ref, ref_logits)
    lg = m.classify(x, topk=k, values="logit")
    assert "rank" not in lg and "logits" not in lg
    assert np.array_equal(_bits(lg["values"].cpu().numpy()), _bits(ref["logit"]))
    assert torch.equal(lg["indices"], out["indices"]) and torch.equal(lg["lse"], out["lse"])
    # the op on the forward's logits gives the bits of the forward-integrated call
    idx = torch.empty((b, k), dtype=torch.int32, device=x.device)
    val, lse = torch.empty((b, k), device=x.device), torch.empty(b, device=x.device)
    m.classify_logits(plain, indices=idx, values_out=val, lse=lse, topk=k)
    assert torch.equal(idx, out["indices"]) and torch.equal(val, out["values"])
    assert torch.equal(lse, out["lse"])
    return out


@pytest.mark.parametrize("dtype", ["bf16", "f32", "mx8"])
def test_classify_vit(gpu, dtype):
    x = torch.from_numpy(make_images(LANES_BATCH, seed=52, image_size=32)).to(gpu)
    m = _vit(dtype, gpu, 3, lanes=1)
    for b in (1, 3):
        _check_model(m, x[:b].contiguous(), 5, f"vit {dtype} bs{b}")
    # numpy in, numpy out
    host = m.classify(x[:3].cpu().numpy(), topk=16, labels=[0, -1, 5])
    assert all(isinstance(v, np.ndarray) for v in host.values())
    assert sorted(host["indices"][0].tolist()) == list(range(16)) and host["rank"][1] == -1
    del m
    # batch lanes: the default policy gives an fp32 ViT two lanes from 128 images and a bf16 or
    # mx8 one none; bf16 gets two by hand
    m = _vit(dtype, gpu, LANES_BATCH, lanes=2 if dtype == "bf16" else None)
    assert m.lanes() == (1 if dtype == "mx8" else 2)
    _check_model(m, x, 5, f"vit {dtype} bs{LANES_BATCH} lanes {m.lanes()}")


def test_classify_t2t_and_swin(gpu):
    args = (256, 2, 4, 2)
    t = T2T_ViT(hidden_size=args[0], depth=args[1], num_heads=args[2], mlp_ratio=args[3],
                dtype="bf16", weights=make_t2t_params(t2t_config(*args), seed=67), device=gpu,
                max_batch=3, lanes=1)
    xt = torch.from_numpy(make_images(3, seed=68, layout="NHWC")).to(gpu)
    _check_model(t, xt, 5, "t2t bf16 bs3")  # C = 1000
    cfg = swin_config("tiny", image_size=56, window_size=7, depths=(2, 2), num_heads=(3, 6),
                      num_classes=11)
    s = SwinTransformer(img_size=56, patch_size=cfg.patch_size, num_classes=11,
                        embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
                        window_size=7, dtype="bf16", weights=make_swin_params(cfg, seed=3),
                        device=gpu, max_batch=3, lanes=1)
    xs = torch.from_numpy(make_images(3, seed=4, image_size=56)).to(gpu)
    _check_model(s, xs, 11, "swin bf16 bs3")  # k = C


def test_classify_uint8_images(gpu):
    """A Uint8Images batch gives bitwise the outputs of its to_float image."""
    m = _vit("bf16", gpu, 3, lanes=1)
    rng = np.random.default_rng(7)
    u8 = Uint8Images(torch.from_numpy(rng.integers(0, 256, (3, 32, 32, 3), dtype=np.uint8)).to(gpu))
    want = m.classify(u8.to_float("nchw"), topk=5, labels=[1, 2, 3], logits=True)
    got = m.classify(u8, topk=5, labels=[1, 2, 3], logits=True)
    assert got.keys() == want.keys() and all(torch.equal(got[k], want[k]) for k in got)
    host = m.classify(Uint8Images(u8.data.cpu().numpy()), topk=5)
    assert np.array_equal(host["indices"], want["indices"].cpu().numpy())
    assert np.array_equal(_bits(host["values"]), _bits(want["values"].cpu().numpy()))


def test_classify_logits_after_graph_replay(gpu):
    m = _vit("bf16", gpu, 3, lanes=1)
    x = torch.from_numpy(make_images(3, seed=52, image_size=32)).to(gpu)
    y = torch.tensor([3, -1, 0], dtype=torch.int32, device=gpu)
    eager = m.classify(x, topk=5, labels=y, logits=True)
    buf = torch.zeros((3, 16), device=gpu)
    m.capture_graph(x, buf)
    m.replay_graph()
    idx = torch.empty((3, 5), dtype=torch.int32, device=gpu)
    val, lse = torch.empty((3, 5), device=gpu), torch.empty(3, device=gpu)
    rank = torch.empty(3, dtype=torch.int32, device=gpu)
    counters = torch.zeros(3, dtype=torch.int64, device=gpu)
    m.classify_logits(buf, indices=idx, values_out=val, lse=lse, labels=y, rank=rank,
                      counters=counters, topk=5)
    assert torch.equal(buf, eager["logits"])
    assert torch.equal(idx, eager["indices"]) and torch.equal(val, eager["values"])
    assert torch.equal(lse, eager["lse"]) and torch.equal(rank, eager["rank"])
    r = eager["rank"].cpu().numpy()
    assert counters.cpu().tolist() == [2, int(((r >= 0) & (r < 1)).sum()), int(((r >= 0) & (r < 5)).sum())]


def test_classify_under_profile_counts_as_head(gpu):
    """A profiled classify forward adds one EVT_PROF_HEAD launch and nothing else."""
    m = _vit("bf16", gpu, 3, lanes=1)
    x = torch.from_numpy(make_images(3, seed=52, image_size=32)).to(gpu)
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
    cls = launches(lambda: m.classify(x))
    assert cls[head] == plain[head] + 1
    assert [v for i, v in enumerate(cls) if i != head] == [v for i, v in enumerate(plain) if i != head]
    assert launches(lambda: m(x)) == plain


def test_forward_classify_error_cases(gpu):
    """Every documented error is EVT_EINVAL with a message before any launch: the sentinel-filled
    outputs (the logits among them) stay as they were."""
    m = _vit("bf16", gpu, 3, lanes=1)
    x = torch.from_numpy(make_images(3, seed=52, image_size=32)).to(gpu)
    b, lib = 3, _lib.load_library()
    fl, logits = _buf((b, 16), torch.float32, gpu)
    fi, idx = _buf((b, 5), torch.int32, gpu)
    fv, val = _buf((b, 5), torch.float32, gpu)
    fs, lse = _buf((b,), torch.float32, gpu)
    fr, rank = _buf((b,), torch.int32, gpu)
    fc = torch.full((4,), SENT_I, dtype=torch.int64, device=gpu)
    y = torch.zeros(b, dtype=torch.int32, device=gpu)

    def raw(batch=b, img="ok", feat="ok", cls="ok", **f):
        a = _lib.evt_classify_args()
        a.k, a.values, a.indices, a.vals, a.lse = 5, 0, idx.data_ptr(), val.data_ptr(), lse.data_ptr()
        for name, v in f.items():
            setattr(a, name, v)
        ft = _lib.evt_features_args()
        if feat == "ok":
            ft.logits = logits.data_ptr()
        elif feat == "misaligned":
            ft.logits = logits.data_ptr() + 2
        im = _lib.evt_image_args()
        im.data, im.format = (x.data_ptr(), 9 if img == "format" else 0) if img != "null data" else (None, 0)
        rc = lib.evt_forward_classify(
            ctypes.c_void_p(m._handle), None if img is None else ctypes.byref(im), batch,
            None if feat is None else ctypes.byref(ft), None if cls is None else ctypes.byref(a),
            ctypes.c_void_p(_lib.stream_ptr(m.device)))
        return rc, lib.evt_last_error()

    bad = {
        "NULL cls": dict(cls=None), "NULL feat": dict(feat=None), "NULL logits": dict(feat="none"),
        "logits misaligned": dict(feat="misaligned"),
        "NULL image": dict(img=None), "NULL image data": dict(img="null data"),
        "unknown image format": dict(img="format"),
        "k 0": dict(k=0), "k > C": dict(k=17), "k 33": dict(k=33), "values 2": dict(values=2),
        "no output": dict(indices=None, vals=None, lse=None),
        "labels alone": dict(indices=None, vals=None, lse=None, labels=y.data_ptr()),
        "rank without labels": dict(rank=rank.data_ptr()),
        "counters without labels": dict(counters=fc.data_ptr()),
        "indices misaligned": dict(indices=idx.data_ptr() + 2),
        "vals misaligned": dict(vals=val.data_ptr() + 1),
        "lse misaligned": dict(lse=lse.data_ptr() + 2),
        "labels misaligned": dict(labels=y.data_ptr() + 2),
        "rank misaligned": dict(labels=y.data_ptr(), rank=rank.data_ptr() + 2),
        "counters 4-byte aligned": dict(labels=y.data_ptr(), counters=fc.data_ptr() + 4),
        "batch 0": dict(batch=0), "batch > max_batch": dict(batch=b + 1),
    }
    for what, kw in bad.items():
        rc, msg = raw(**kw)
        assert rc == _lib.EVT_EINVAL and msg, what
    # op level on device memory: ldl < C, batch 0
    a = _lib.evt_classify_args()
    a.k, a.indices = 5, idx.data_ptr()
    good = torch.zeros((b, 16), device=gpu)
    for ldl, batch in ((15, b), (16, 0)):
        assert lib.evt_classify(_p(good), ldl, batch, 16, ctypes.byref(a), _s()) == _lib.EVT_EINVAL
        assert b"classify" in lib.evt_last_error()
    torch.cuda.synchronize()
    assert all(_untouched(f) for f in (fl, fi, fv, fs, fr, fc))
    # and the valid call fills them
    rc, msg = raw(labels=y.data_ptr(), rank=rank.data_ptr(), counters=fc.data_ptr())
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert torch.equal(logits, m(x)) and fc.cpu().tolist()[0] == SENT_I + b and fc[3] == SENT_I
    assert not (idx == SENT_I).any() and not (rank == SENT_I).any()
    # the Python layer's own checks
    with pytest.raises(ValueError, match="topk"):
        m.classify(x, topk=17)
    with pytest.raises(ValueError, match="labels"):
        m.classify(x, labels=[0, 1])
    with pytest.raises(ValueError, match="labels"):
        m.classify(x, labels=[0.0, 1.0, 2.0])


def test_evaluate_end_to_end(gpu):
    """Three batches (fp32 tensor, numpy, a short Uint8Images one); the labels come from the
    model's own order: rows 0-4 its argmax, rows 5-7 its second class, the rest its third. Every
    label is among the top 3, so seen = 11, top1 = 5, topk = 11 exactly."""
    m = _vit("bf16", gpu, 4, lanes=1)
    x = torch.from_numpy(make_images(8, seed=52, image_size=32)).to(gpu)
    rng = np.random.default_rng(11)
    u8 = Uint8Images(torch.from_numpy(rng.integers(0, 256, (3, 32, 32, 3), dtype=np.uint8)).to(gpu))
    batches = [x[:4].contiguous(), x[4:].cpu().numpy(), u8]
    place = [0] * 5 + [1] * 3 + [2] * 3
    loader, row = [], 0
    for imgs in batches:
        order = classify_reference(np.asarray(m(imgs).cpu() if not isinstance(imgs, np.ndarray)
                                              else m(imgs)), 3)["indices"]
        y = [int(order[i, place[row + i]]) for i in range(order.shape[0])]
        loader.append((imgs, torch.tensor(y) if len(loader) == 0 else y))
        row += order.shape[0]
    lines = []
    res = evaluate(m, loader, topk=3, log=lines.append)
    assert (res["seen"], res["top1"], res["topk"]) == (11, 5, 11)
    assert res["acc1"] == 5 / 11 and res["acck"] == 1.0
    assert len(lines) == 4 and lines[-1] == f"Summary model accuracy is {5 / 11 * 100: .2f}%"
    assert evaluate(m, loader, topk=1) == dict(seen=11, top1=5, topk=5, acc1=5 / 11, acck=5 / 11)
