"""CPU checks of tests/_attn_probes.py for every case tests/test_gpu_attn_probes.py runs:

  * the condition on the reference: the permutation probe's fp64 softmax keeps >= 1 - 2^-12 on
    key pi(i) of every query, and the uniform probe's weights are exactly 1 / N;
  * sensitivity: every applicable mutation of the reference (a dropped, doubled or unmasked key,
    two V rows swapped, a skipped key block) exceeds the error bound by >= 4 x at some element, so
    the bound cannot be vacuous;
  * sanity: a legal re-evaluation (fp32, reversed summation order, bf16 P and output where the
    kernel has them) stays within the bound.
"""
import numpy as np
import pytest

from tests import _attn_probes as ap


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


TOKEN_CASES = ap.attention_cases() + [c for c in ap.hd_cases() if c[2] != 64] + ap.mx8_cases()


def _token_bound(case, img, n, hd, dtype):
    ref = case["refs"][img]
    b = ap.rows_of(ap.error_bound(ref, dtype, n, hd), n)
    if dtype == "mx8":
        b = b + ap.mx8_step(ap.rows_of(ref["o"], n))
    return b


def _check_condition(probe, ref, target):
    p = ref["p"]
    if probe == "uniform":
        assert np.all(ref["y"] == 0.0) and np.all(p == 1.0 / p.shape[-1])
        return
    hit = np.take_along_axis(p, target[..., None], -1)[..., 0]
    assert hit.min() >= 1.0 - ap.LEAK, f"weight on pi(i): {hit.min()}"
    assert np.abs(ref["yqk"]).max() < 80.0


@pytest.mark.parametrize("probe,n,hd,dtype", TOKEN_CASES, ids=_ids(TOKEN_CASES))
def test_token_probe(probe, n, hd, dtype):
    case = ap.token_case(probe, n, hd)
    ref, ins = case["refs"][0], case["ins"][0]
    _check_condition(probe, ref, case["pi"])
    bound = _token_bound(case, 0, n, hd, dtype)
    o64 = ap.rows_of(ref["o"], n)
    for name in ap.applicable(probe, n):
        ratio = (np.abs(ap.rows_of(ap.mutated(ins, name), n) - o64) / bound).max()
        assert ratio >= 4.0, f"{name}: err / bound {ratio:.2f}"
    if dtype != "mx8":  # the quantiser is a step function: its gate is not a rounding bound
        for img in (0, 1):
            got = ap.rows_of(ap.reordered(case["ins"][img], dtype), n)
            r = (np.abs(got - ap.rows_of(case["refs"][img]["o"], n)) /
                 _token_bound(case, img, n, hd, dtype)).max()
            assert r <= 1.0, f"image {img}: reordered err / bound {r:.3f}"


@pytest.mark.parametrize("n", ap.MX8_N)
def test_mx8_uniform_cannot_see_a_key(n):
    """Why the uniform probe is not run on evt_attention_mx8: a lost or doubled key moves its
    outputs by about 1 / N, below 4 x the E4M3 step of the block."""
    case = ap.token_case("uniform", n, 64)
    bound = _token_bound(case, 0, n, 64, "mx8")
    o64 = ap.rows_of(case["refs"][0]["o"], n)
    worst = min((np.abs(ap.rows_of(ap.mutated(case["ins"][0], m), n) - o64) / bound).max()
                for m in ap.applicable("uniform", n))
    assert worst < 4.0


WINDOW_CASES = ap.window_cases()


@pytest.mark.parametrize("probe,R,shift,dtype", WINDOW_CASES, ids=_ids(WINDOW_CASES))
def test_window_probe(probe, R, shift, dtype):
    case = ap.window_case(probe, R, shift)
    ref, ins = case["refs"][0], case["ins"][0]
    if probe == "perm":
        # key pi(i): the one key of the query's group that carries its code
        target = np.einsum("gid,gjd->gij", ins[0], ins[1]).argmax(-1)
        _check_condition(probe, ref, target)
    else:  # equal weights over the keys of the query's own region
        p = ref["p"]
        cnt = (p > 1e-30).sum(-1, keepdims=True)
        assert np.all(np.abs(np.where(p > 1e-30, p * cnt, 1.0) - 1.0) < 1e-12)
    bound = ap.error_bound(ref, dtype, 49, 32)
    muts = {m: ap.mutated(ins, m) for m in ap.applicable(probe, 49)}
    if shift and probe == "uniform":  # (pi stays inside a region: its probe cannot see this one)
        muts["mask_ignored"] = ap.core(*case["unmasked"])["o"]
    for name, o in muts.items():
        ratio = (np.abs(o - ref["o"]) / bound).max()
        assert ratio >= 4.0, f"{name}: err / bound {ratio:.2f}"
    for img in (0, 1):
        r = (np.abs(ap.reordered(case["ins"][img], dtype) - case["refs"][img]["o"]) /
             ap.error_bound(case["refs"][img], dtype, 49, 32)).max()
        assert r <= 1.0, f"image {img}: reordered err / bound {r:.3f}"


def test_window_reference_is_the_oracle_core():
    """The grouped reference of the window probes equals `_oracle_core` (tests/test_gpu_swin.py)
    on the same rows, bias table and shift."""
    from tests.test_gpu_swin import _oracle_core as oracle
    for probe, R, shift, _ in ap.window_cases()[:4]:
        case = ap.window_case(probe, R, shift)
        mine = ap.window_rows(case["refs"][0]["o"], case["win"], R * R)
        ref = oracle(case["rows"][0], R, ap.H, shift, case["rpb"])
        assert np.abs(mine - ref).max() <= 1e-12
