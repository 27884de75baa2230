"""GPU: the TokenPerformer kernels on token-exact probes at every chunk, tile and span edge
(tests/_performer_probes.py: the probes, the fp64 reference, the derivation of the error bound;
tests/test_performer_probes_host.py: the same cases' sensitivity on the CPU).

test_performer_core (tests/test_gpu_t2t.py) gates random inputs at 3e-2 / 2e-4 of the output scale,
which one lost, doubled or cross-image token among T stays inside. Here every case is a probe on
which such a fault is >= 4 x the derived per-element bound, through evt_performer (bf16, f32) and
evt_performer_ex (bf16: kqv_perm 0 / 1, with and without tstats; include/evt_performer.h).

Every launch: a hostile neighbour image in both image orders (the probe image's bits must not
depend on the order), ldq in {192, 200} and ldo in {64, 72} with NaN input padding and sentinel
output padding, NaN guard rows around kqv, sentinel guard rows around out and tstats, and a
scratch of exactly evt_performer_scratch floats, NaN before the call, with a canary behind it.

Each family prints `PERFPROBE <family>: max err/bound ...` when the module ends (-s shows it);
the figures of the first MI355X run are in DESIGN.md, "Performer probes".
"""
import collections
import functools

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import _lib
from edgevisiontransformer_amd.weights import make_t2t_params, t2t_config
from oracle import t2t_ref
from tests import _ops
from tests import _performer_probes as pp
from tests._ops import TDT, _p, _s

pytestmark = pytest.mark.gpu

G = 8                    # guard rows on either side
SENT = 7.0               # output / tstats sentinel
CANARY = 12345.0
N_CANARY = 64
RATIO = collections.defaultdict(lambda: [0.0, 0])   # family -> [largest err / bound, cases]


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam in sorted(RATIO):
        print(f"\nPERFPROBE {fam}: max err/bound {RATIO[fam][0]:.3f} ({RATIO[fam][1]} cases)", end="")
    print()


def _note(family, ratio):
    RATIO[family][0] = max(RATIO[family][0], float(ratio))
    RATIO[family][1] += 1


def _cus(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count


_DEV_W = {}


def _weights(gpu, P=None):
    """Device pointers' tensors in evt_performer's order; P = None: the probe weights."""
    if P is not None:
        return [torch.from_numpy(np.ascontiguousarray(P["p1." + n], np.float32)).to(gpu)
                for n in pp.WEIGHT_ORDER]
    key = str(gpu)
    if key not in _DEV_W:
        w = pp.weights()
        _DEV_W[key] = [torch.from_numpy(np.ascontiguousarray(w[n])).to(gpu) for n in pp.WEIGHT_ORDER]
    return _DEV_W[key]


def _run(gpu, entry, dtype, rows, B, T, ldq, ldo, perm=0, tstats=False, ws=None):
    """One launch with every guard in place; rows [B T, 192] fp64 in reference order. Returns the
    [B T, 64] output tensor (a copy) and the [B T, 2] statistics (or None)."""
    lib = _lib.load_library()
    tdt, n = TDT[dtype], B * T
    assert rows.shape == (n, 192)
    kq = torch.full((n + 2 * G, ldq), float("nan"), dtype=tdt, device=gpu)
    data = pp.permute_rows(rows) if perm else rows
    kq[G:G + n, :192] = torch.from_numpy(data.astype(np.float32)).to(gpu).to(tdt)
    out = torch.full((n + 2 * G, ldo), SENT, dtype=tdt, device=gpu)
    ts = torch.full((n + 2 * G, 2), SENT, device=gpu) if tstats else None
    nf = int(lib.evt_performer_scratch(B, T))
    assert nf == pp.scratch_floats(B, T)
    part = torch.full((nf + N_CANARY,), float("nan"), device=gpu)
    part[nf:] = CANARY
    w = ws if ws is not None else _weights(gpu)
    args = [_lib.DTYPE[dtype], _p(kq[G:]), ldq, B, T, *[_p(t) for t in w], _p(part), _p(out[G:]), ldo]
    if entry == "ex":
        _lib.check(lib.evt_performer_ex(*args, perm, _p(ts[G:]) if tstats else None, _s()))
    else:
        _lib.check(lib.evt_performer(*args, _s()))
    torch.cuda.synchronize()
    assert torch.all(out[:G] == SENT) and torch.all(out[G + n:] == SENT), "out guard rows written"
    assert torch.all(out[G:G + n, 64:] == SENT), "out padding columns written"
    assert torch.all(part[nf:] == CANARY), "write past evt_performer_scratch floats"
    assert not torch.isnan(part[:nf]).any(), "scratch not fully written"
    if tstats:
        assert torch.all(ts[:G] == SENT) and torch.all(ts[G + n:] == SENT), "tstats guard rows written"
    return out[G:G + n, :64].clone(), (ts[G:G + n].clone() if tstats else None)


def _f64(t):
    return t.double().cpu().numpy()


def _pair(case, order):
    """rows of (hostile, probe) for order 0, (probe, hostile) for order 1; probe row slice."""
    r = case["rows"]
    T = r[0].shape[0]
    if order == 0:
        return np.concatenate([r[1], r[0]]), slice(T, 2 * T), slice(0, T)
    return np.concatenate([r[0], r[1]]), slice(0, T), slice(T, 2 * T)


def _gate(family, got, case, bounds, ps, hs, what):
    assert np.all(np.isfinite(got)), f"{what}: non-finite output"
    rp = (np.abs(got[ps] - case["refs"][0]["out"]) / bounds[0]).max()
    rh = (np.abs(got[hs] - case["refs"][1]["out"]) / bounds[1]).max()
    print(f"PERFPROBE {family} {what}: probe err/bound {rp:.3f}, neighbour {rh:.3f}")
    assert rp <= 1.0, f"{what}: probe image err / bound {rp:.3f}"
    assert rh <= 1.0, f"{what}: neighbour image err / bound {rh:.3f}"
    _note(family, rp)


def _check_tstats(out, ts, what):
    """(sum, sumsq) of every token against the fp64 sums of the stored bf16 output."""
    o = _f64(out)
    want = np.stack([o.sum(-1), (o * o).sum(-1)], -1)
    r = (np.abs(_f64(ts) - want) / pp.tstats_bound(o)).max()
    assert r <= 1.0, f"{what}: tstats err / bound {r:.3f}"
    return r


CASES = [c for c in pp.probe_cases() if c[1] in pp.PROBE_T]


@pytest.mark.parametrize("probe,T,dtype", CASES, ids=_ids(CASES))
def test_performer_probe(gpu, probe, T, dtype):
    """evt_performer: performer_kv_kernel, performer_reduce_kernel and performer_out16_kernel
    (bf16) / performer_out_kernel (f32) in reference column order."""
    case, bounds = pp.case(probe, T), pp.bounds(probe, T, dtype)
    ldq, ldo = pp.ld_of(T)
    bits = []
    for order in (0, 1):
        rows, ps, hs = _pair(case, order)
        out, _ = _run(gpu, "performer", dtype, rows, 2, T, ldq, ldo)
        _gate(f"evt_performer {dtype}", _f64(out), case, bounds, ps, hs, f"order {order}")
        bits.append(out[ps])
    assert torch.equal(bits[0], bits[1]), "the probe image's bits depend on the image order"


EX_CASES = [(p, t) for t in pp.PROBE_T for p in pp.PROBES]


@pytest.mark.parametrize("probe,T", EX_CASES, ids=_ids(EX_CASES))
def test_performer_ex_probe(gpu, probe, T):
    """evt_performer_ex (bf16): the model's path (kqv_perm = 1 on kqv_col-permuted columns, 16-B
    loads, the kv kernel's raw prefetch, tstats) against the reference order, bit for bit."""
    case, bounds = pp.case(probe, T), pp.bounds(probe, T, "bf16")
    ldq, ldo = 200, pp.ld_of(T)[1]          # the permuted path needs ldq % 8 == 0
    bits = []
    for order in (0, 1):
        rows, ps, hs = _pair(case, order)
        plain, _ = _run(gpu, "performer", "bf16", rows, 2, T, ldq, ldo)
        for perm in (0, 1):
            for with_ts in (False, True):
                what = f"order {order} kqv_perm {perm} tstats {int(with_ts)}"
                out, ts = _run(gpu, "ex", "bf16", rows, 2, T, ldq, ldo, perm=perm, tstats=with_ts)
                assert torch.equal(out, plain), f"{what}: out differs from evt_performer's bits"
                if with_ts:
                    _note("tstats", _check_tstats(out, ts, what))
        _gate(f"evt_performer_ex bf16", _f64(out), case, bounds, ps, hs, f"order {order}")
        bits.append(out[ps])
    assert torch.equal(bits[0], bits[1]), "the probe image's bits depend on the image order"


# ---- the out pass with more than one round per wave ---------------------------------------------
MULTI = [("performer", "bf16"), ("performer", "f32"), ("ex", "bf16")]
SHAPES = [(100, 112), (200, 80)]        # (T, span): B = 4 CUs, B = ceil(4 CUs / 3)


def _multi_B(T, cus):
    return 4 * cus if T == 100 else (4 * cus + 2) // 3


@functools.lru_cache(maxsize=None)
def _multi_batch(T, B):
    """[B, T, 64] x 3: the class probe at 0 and B - 1, the count probe in the middle, a hostile
    image next to the first and the last, seeded {-1, 0, +1} images elsewhere; the fp64 reference."""
    k, q, v = (a.copy() for a in pp.fill_kqv(B, T, seed=T + B))
    where = {0: "class", B // 2: "count", B - 1: "class"}
    for i, probe in where.items():
        k[i], q[i], v[i] = pp.case(probe, T)["kqv"][0]
    for i in (1, B - 2):
        k[i], q[i], v[i] = pp.case("class", T)["kqv"][1]
    ref = pp.core(k, q, v)
    rows = pp.to_rows(k, q, v).reshape(B * T, 192)
    return rows, ref, where


@functools.lru_cache(maxsize=None)
def _multi_bound(T, B, dtype):
    return pp.error_bound(_multi_batch(T, B)[1], dtype)


@pytest.mark.parametrize("T,span", SHAPES)
@pytest.mark.parametrize("entry,dtype", MULTI)
def test_out_pass_rounds(gpu, entry, dtype, T, span):
    """span > 64: the `t0 += 64` loop of the out kernels, the prefetch of the next tile and the
    partly valid tile of the second round (T = 100, span 112: three waves run a second round, the
    fourth none). The probe images' rows equal, bit for bit, the rows they give alone (B = 1,
    span 64): a token's arithmetic does not depend on its workgroup."""
    cus = _cus(gpu)
    B = _multi_B(T, cus)
    assert pp.span_of(T, B, cus) == span and span > 64, "the case went vacuous on this device"
    assert pp.span_of(T, 1, cus) == 64
    rows, ref, where = _multi_batch(T, B)
    ldq, ldo = 200, 72
    kw = dict(perm=1, tstats=True) if entry == "ex" else {}
    out, ts = _run(gpu, entry, dtype, rows, B, T, ldq, ldo, **kw)
    got = _f64(out).reshape(B, T, 64)
    assert np.all(np.isfinite(got))
    ratio = np.abs(got - ref["out"]) / _multi_bound(T, B, dtype)
    per_image = ratio.reshape(B, -1).max(1)
    fam = f"out pass span {span} {entry} {dtype}"
    print(f"PERFPROBE {fam}: probes {[round(float(per_image[i]), 3) for i in where]}, "
          f"all images {per_image.max():.3f}")
    assert per_image.max() <= 1.0, f"image {per_image.argmax()}: err / bound {per_image.max():.3f}"
    _note(fam, per_image.max())
    if ts is not None:
        _note("tstats", _check_tstats(out, ts, fam))
    for i in where:
        one, ts1 = _run(gpu, entry, dtype, rows[i * T:(i + 1) * T], 1, T, ldq, ldo, **kw)
        assert torch.equal(one, out[i * T:(i + 1) * T]), f"image {i}: bits depend on the span"
        if ts is not None:
            assert torch.equal(ts1, ts[i * T:(i + 1) * T]), f"image {i}: tstats depend on the span"


# ---- evt_unfold_stats -----------------------------------------------------------------------------
def _gather(ts, R):
    """fp64 soft-split (k 3, s 2, p 1) gather of [B, R, R, 2] -> ([B, OW, OW, 2], its sum of |.|)."""
    OW = (R + 1) // 2
    pad = np.pad(ts.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    s, a = np.zeros((ts.shape[0], OW, OW, 2)), np.zeros((ts.shape[0], OW, OW, 2))
    for kh in range(3):
        for kw in range(3):
            win = pad[:, kh:kh + 2 * OW - 1:2, kw:kw + 2 * OW - 1:2]
            s, a = s + win, a + np.abs(win)
    return s, a


def _unfold_stats(gpu, ts, R, nslots):
    lib = _lib.load_library()
    B, OW = ts.shape[0], (R + 1) // 2
    rows = B * OW * OW
    src = torch.full((B * R * R + 2 * G, 2), float("nan"), device=gpu)
    src[G:G + B * R * R] = torch.from_numpy(ts.reshape(-1, 2)).to(gpu)
    dst = torch.full((rows + 2 * G, nslots, 2), SENT, device=gpu)
    _lib.check(lib.evt_unfold_stats(_p(src[G:]), B, R, _p(dst[G:]), nslots, _s()))
    torch.cuda.synchronize()
    assert torch.all(dst[:G] == SENT) and torch.all(dst[G + rows:] == SENT), "dst guard rows written"
    got = dst[G:G + rows].cpu().numpy()
    assert not got[:, 1:].any(), "slots >= 1 must be zero"
    return got[:, 0].astype(np.float64).reshape(B, OW, OW, 2)


@pytest.mark.parametrize("R", [2, 4, 6, 12])
def test_unfold_stats(gpu, R):
    """unfold_stats_kernel: slot 0 = the fp64 gather of the <= 9 source tokens within 9 u of their
    absolute sum, with a hostile second image (1e6 x) in both orders."""
    rng = np.random.default_rng(R)
    img = rng.standard_normal((2, R, R, 2)).astype(np.float32)
    img[1] *= 1e6
    for order in (0, 1):
        ts = img if order else img[::-1].copy()
        want, mag = _gather(ts, R)
        got = _unfold_stats(gpu, ts, R, 3)
        r = (np.abs(got - want) / (9 * pp.U * mag + pp.TINY)).max()
        assert r <= 1.0, f"order {order}: err / bound {r:.3f}"
        _note("evt_unfold_stats", r)


@pytest.mark.parametrize("R", [2, 4, 6, 12])
def test_unfold_stats_against_unfold(gpu, R):
    """For a bf16 map [2, R, R, 64]: the statistics gathered from per-token (sum, sumsq) equal the
    row statistics evt_unfold (k 3, s 2, p 1, ldo 576) computes from the gathered rows itself.
    Bounds: the token statistics are fp64 sums rounded to fp32 (u), the gather 9 u, evt_unfold's
    fp32 sum of a 576-element row (576 additions in some order, a rounded square each) 577 u, all
    of the absolute sum of the row."""
    lib = _lib.load_library()
    rng = np.random.default_rng(100 + R)
    x = rng.standard_normal((2, R, R, 64)).astype(np.float32)
    x[1] *= 64.0
    xb = torch.from_numpy(x).to(gpu).to(torch.bfloat16)
    xd = xb.double().cpu().numpy()
    ts = np.stack([xd.sum(-1), (xd * xd).sum(-1)], -1).astype(np.float32)
    _, mag = _gather(np.stack([np.abs(xd).sum(-1), (xd * xd).sum(-1)], -1), R)
    OW, nslots = (R + 1) // 2, 6
    rows = 2 * OW * OW
    got = _unfold_stats(gpu, ts, R, nslots).reshape(rows, 2)
    urows = torch.full((rows, 576), SENT, dtype=torch.bfloat16, device=gpu)
    ustats = torch.full((rows, nslots, 2), SENT, device=gpu)
    _lib.check(lib.evt_unfold(_lib.DTYPE["bf16"], 0, _p(xb), 2, R, R, 64, 3, 2, 1, _p(urows), 576,
                              _p(ustats), nslots, _s()))
    torch.cuda.synchronize()
    ref = t2t_ref.unfold_nhwc(xd, 3, 2, 1).reshape(rows, 576)
    assert np.array_equal(_f64(urows), ref)
    us = ustats.cpu().numpy().astype(np.float64)
    assert not us[:, 1:].any()
    r = (np.abs(got - us[:, 0]) / ((9 + 1 + 577) * pp.U * mag.reshape(rows, 2) + pp.TINY)).max()
    assert r <= 1.0, f"gathered against evt_unfold's statistics: err / bound {r:.3f}"
    _note("evt_unfold_stats vs evt_unfold", r)


# ---- random inputs, seeded weights: LN2 and the FFN at the new edges ----------------------------
@functools.lru_cache(maxsize=None)
def _seeded_params():
    return make_t2t_params(t2t_config(256, 1, 4, 2), seed=21)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("T,big", [(197, False), (393, False), (100, True)])
def test_performer_core_at_the_edges(gpu, dtype, T, big):
    """test_performer_core's check (tests/test_gpu_t2t.py; 2e-4 of the output scale in f32, 3e-2
    in bf16) at two chunks of 99, three of 131 and at B = 4 CUs, T = 100 (span 112)."""
    P = _seeded_params()
    B = 4 * _cus(gpu) if big else 2
    rng = np.random.default_rng(T)
    kqv = rng.standard_normal((B, T, 192)).astype(np.float32)
    kqv = torch.from_numpy(kqv).to(TDT[dtype]).double().numpy()
    ref = t2t_ref.performer_core(kqv, {k: v.astype(np.float64) for k, v in P.items()}, "p1.")
    out, _ = _run(gpu, "performer", dtype, kqv.reshape(B * T, 192), B, T, *pp.ld_of(T),
                  ws=_weights(gpu, P))
    got = _f64(out).reshape(B, T, 64)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    tol = 2e-4 if dtype == "f32" else 3e-2
    print(f"PERFPROBE random {dtype} T={T} B={B}: rel err {err:.2e}")
    assert err <= tol, f"performer {dtype} T={T} B={B}: rel err {err:.2e} > {tol}"
