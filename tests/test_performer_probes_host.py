"""CPU checks of tests/_performer_probes.py for every case tests/test_gpu_performer_probes.py runs:

  * the conditions on the reference: every input exact in bf16, exponents exact and in range, the
    count probe's y = S_n / (T + 1e-8), the class probe's weight on keys of another class
    <= 2^-12 per query, and across the cases every k / q / v feature and random feature in use;
  * sensitivity: every applicable mutation (a token lost or doubled in kptv, ksum or both, a
    clamped row counted, a chunk partial skipped or doubled, v swapped or shifted against kp,
    output rows swapped, a token of the other image) exceeds the bound by >= 4 x at some element,
    and every mutation that exists at T is seen by a case at T, in bf16 and in f32;
  * sanity: a legal re-evaluation (fp32, the kernels' rounding points, another summation order)
    stays within the bound, for both images of a case and for the fill images;
  * include/evt_performer.h = its binding = the exported symbols.
"""
import os
import re

import numpy as np
import pytest

from edgevisiontransformer_amd import _lib
from tests import _performer_probes as pp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = pp.probe_cases()


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


def _ratios(probe, T, dtype):
    c = pp.case(probe, T)
    ref, bound = c["refs"][0]["out"], pp.bounds(probe, T, dtype)[0]
    return {name: (np.abs(pp.mutated(c["kqv"][0], c["kqv"][1], name) - ref) / bound).max()
            for name in pp.MUTATIONS if pp.applicable((probe, T, dtype), name)}


def _check_inputs(kqv, ref):
    for z in kqv:
        assert np.array_equal(pp.bf16_round(z), z)
    for x in (ref["xk"], ref["xq"]):
        assert np.array_equal(np.round(2 * x), 2 * x) and np.abs(x).max() <= 80.0
    assert np.all(np.isfinite(ref["out"]))


@pytest.mark.parametrize("probe,T,dtype", CASES, ids=_ids(CASES))
def test_probe(probe, T, dtype):
    c = pp.case(probe, T)
    for kqv, ref in zip(c["kqv"], c["refs"]):
        _check_inputs(kqv, ref)
    ref = c["refs"][0]
    if probe == "count":
        s = np.bincount(np.arange(T) % 64, minlength=64)
        assert np.all(ref["kp"] == pp.C64) and np.all(ref["qp"] == pp.C64)
        np.testing.assert_allclose(ref["y"], np.broadcast_to(s / (T + 1e-8), (T, 64)), rtol=1e-14)
    else:
        kc, qc, Kc = pp.class_maps(T)
        assert set(kc) == set(qc) == set(range(Kc))
        if Kc >= 2:
            assert (kc == kc[T - 1]).sum() == 2
        p = (ref["qp"] @ ref["kp"].T) / (ref["D"] + 1e-8)[:, None]
        leak = (p * (kc[None, :] != qc[:, None])).sum(1)
        assert leak.max() <= pp.LEAK, f"weight on keys of another class {leak.max():.3e}"
    assert np.abs(c["refs"][1]["out"] - 128.0).max() <= 1e-4      # the neighbour: 64 + 64 (1e-8 / D aside)
    for name, r in _ratios(probe, T, dtype).items():
        assert r >= 4.0, f"{name}: err / bound {r:.2f}"
    for img in (0, 1):
        got = pp.emulate(*c["kqv"][img], dtype)
        r = (np.abs(got - c["refs"][img]["out"]) / pp.bounds(probe, T, dtype)[img]).max()
        assert r <= 1.0, f"image {img}: re-evaluated err / bound {r:.3f}"


@pytest.mark.parametrize("dtype", pp.DTYPES)
@pytest.mark.parametrize("T", pp.PROBE_T + (200,))
def test_every_mutation_is_seen_at_every_T(T, dtype):
    for name in pp.MUTATIONS:
        if pp.structural(T, name):
            assert any(pp.applicable((p, T, dtype), name) for p in pp.PROBES), name


def test_every_mutation_exists_somewhere():
    for name in pp.MUTATIONS:
        assert any(pp.structural(T, name) for T in pp.PROBE_T), name


def test_every_feature_carries_signal():
    k = q = v = np.zeros(64, bool)
    rf = np.zeros(32, bool)
    for T in pp.PROBE_T:
        (kk, qq, vv), ref = pp.case("class", T)["kqv"][0], pp.case("class", T)["refs"][0]
        k, q, v = k | (kk != 0).any(0), q | (qq != 0).any(0), v | (vv != 0).any(0)
        rf |= (ref["xk"] == 0).any(0) & (ref["xq"] == 0).any(0)
    assert k.all() and q.all() and v.all() and rf.all()
    assert (pp.case("count", 393)["kqv"][0][2] != 0).any(0).all()


@pytest.mark.parametrize("dtype", pp.DTYPES)
@pytest.mark.parametrize("T", pp.MULTI_T)
def test_fill_images(T, dtype):
    k, q, v = pp.fill_kqv(3, T, seed=T)
    ref = pp.core(k, q, v)
    bound = pp.error_bound(ref, dtype)
    for i in range(3):
        _check_inputs((k[i], q[i], v[i]), {key: ref[key][i] for key in ("xk", "xq", "out")})
        r = (np.abs(pp.emulate(k[i], q[i], v[i], dtype) - ref["out"][i]) / bound[i]).max()
        assert r <= 1.0, f"fill image {i}: re-evaluated err / bound {r:.3f}"
    # batched and per-image evaluation of the reference and the bound agree
    one = pp.core(k[1], q[1], v[1])
    assert np.array_equal(one["out"], ref["out"][1])
    np.testing.assert_allclose(pp.error_bound(one, dtype), bound[1], rtol=1e-12)


def test_layout_and_span():
    assert [pp.layout(T) for T in (1, 196, 197, 392, 393, 3136)] == [
        (1, 1), (1, 196), (2, 99), (2, 196), (3, 131), (16, 196)]
    assert pp.span_of(100, 2, 256) == 64 and pp.span_of(100, 1024, 256) == 112
    assert pp.span_of(200, (4 * 256 + 2) // 3, 256) == 80
    assert pp.span_of(3136, 256, 256) == 784 and pp.span_of(784, 256, 256) == 208
    assert sorted(pp.kqv_col(f) for f in range(64)) == list(range(64))
    assert [pp.kqv_col(f) for f in (0, 3, 4, 16, 20, 63)] == [0, 3, 16, 4, 20, 63]


def test_reference_is_the_oracle():
    """`core` with the probe weights equals oracle/t2t_ref.py performer_core."""
    from oracle import t2t_ref
    P = {"p." + n: a.astype(np.float64) for n, a in pp.weights().items()}
    for probe, T in (("count", 65), ("class", 197)):
        c = pp.case(probe, T)
        ref = t2t_ref.performer_core(np.stack(c["rows"]), P, "p.")
        for img in (0, 1):
            assert np.abs(ref[img] - c["refs"][img]["out"]).max() <= 1e-12


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from edgevisiontransformer_amd.build import build
        build()
    return _lib.load_library()


def test_header_binding_and_exports_agree(lib):
    txt = open(os.path.join(REPO, "include", "evt_performer.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t|const char\*)\s+(evt_\w+)\(", txt, re.M)))
    assert declared == sorted(_lib.PERFORMER_SIGNATURES) == ["evt_performer_ex", "evt_unfold_stats"]
    assert not set(declared) & set(_lib.SIGNATURES)
    assert '#include "evt_performer.h"' in open(os.path.join(REPO, "include", "evt.h")).read()
    from edgevisiontransformer_amd import build
    assert any(h.endswith("evt_performer.h") for h in build.HEADERS)
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.PERFORMER_SIGNATURES[name][1]
    # evt_performer's arguments, then (kqv_perm, tstats), then the stream
    perf, ex = _lib.SIGNATURES["evt_performer"][1], _lib.PERFORMER_SIGNATURES["evt_performer_ex"][1]
    assert ex[:len(perf) - 1] == perf[:-1] and len(ex) == len(perf) + 2
    assert lib.evt_performer_scratch(3, 393) == pp.scratch_floats(3, 393)
    assert lib.evt_performer_scratch(2, 196) == pp.scratch_floats(2, 196)
