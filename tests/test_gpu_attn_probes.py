"""GPU: the attention kernels on key-exact probes at every tile boundary (tests/_attn_probes.py:
the probes, the fp64 reference, the derivation of the error bound and the N -> kernel map beside
the case lists; tests/test_attn_probes_host.py: the same cases' sensitivity on the CPU).

The random-input tests (test_attention, test_attention_any_head_size, test_long_attention*) gate
the bf16 kernels at 2e-2, which one lost or doubled key among N stays inside. Here every case is a
probe on which such a fault is far above the bound

    |o - o64| <= u_out |o64| + r_P + (N + hd + 8) 2^-24 a + E + tiny

and runs with a hostile neighbour image (B = 2, H = 2) in both image orders: the probe image's
output bits must not depend on the order, the rows after B N of the qkv allocation are NaN (the
output must be finite), and both images are gated by the bound. evt_attention_hd writes into a
padded pitch whose extra columns must keep their sentinel.

Each family prints `ATTNPROBE <family>: max err/bound ...` when the module ends (-s shows it);
the figures of the first MI355X run are in DESIGN.md, "Attention probes".
"""
import collections

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import _lib
from oracle import mx8_ref
from tests import _attn_probes as ap
from tests import _ops
from tests._ops import TDT, _p, _s

pytestmark = pytest.mark.gpu

H = ap.H
GUARD_ROWS = 8
RATIO = collections.defaultdict(lambda: [0.0, 0])   # family -> [largest err / bound, cases]


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam in sorted(RATIO):
        print(f"\nATTNPROBE {fam}: max err/bound {RATIO[fam][0]:.3f} ({RATIO[fam][1]} cases)", end="")
    print()


def _device_qkv(rows, order, tdt, gpu):
    """Both images as one qkv allocation followed by NaN guard rows. order 0: (hostile, probe),
    order 1: (probe, hostile). Returns the view of the B N valid rows (it keeps the storage)."""
    x = np.concatenate([rows[1], rows[0]] if order == 0 else [rows[0], rows[1]])
    t = torch.full((x.shape[0] + GUARD_ROWS, x.shape[1]), float("nan"), dtype=tdt, device=gpu)
    t[: x.shape[0]] = torch.from_numpy(x).to(tdt)
    return t[: x.shape[0]]


def _gate(family, outs, bits, refs, bounds, n):
    """outs[order]: [2 n, cols] fp64 of both images; bits[order]: tensors whose equality is the
    bitwise one; refs / bounds [image]: [n, cols] (image 0 the probe)."""
    for order in (0, 1):
        assert np.all(np.isfinite(outs[order])), f"order {order}: non-finite output"
    sl = [slice(n, 2 * n), slice(0, n)]                  # the probe image's rows per order
    for a, b in zip(bits[0], bits[1]):
        assert torch.equal(a[sl[0]], b[sl[1]]), "the probe image's bits depend on the image order"
    worst = 0.0
    for order in (0, 1):
        hs = sl[1 - order]                               # the hostile image's rows
        rp = (np.abs(outs[order][sl[order]] - refs[0]) / bounds[0]).max()
        rh = (np.abs(outs[order][hs] - refs[1]) / bounds[1]).max()
        worst = max(worst, rp)
        print(f"ATTNPROBE {family} order {order}: probe err/bound {rp:.3f}, neighbour {rh:.3f}")
        assert rp <= 1.0, f"order {order}: probe image err / bound {rp:.3f}"
        assert rh <= 1.0, f"order {order}: neighbour image err / bound {rh:.3f}"
    RATIO[family][0] = max(RATIO[family][0], worst)
    RATIO[family][1] += 1


def _token_refs(case, n, hd, dtype):
    refs = [ap.rows_of(r["o"], n) for r in case["refs"]]
    bounds = [ap.rows_of(ap.error_bound(r, dtype, n, hd), n) for r in case["refs"]]
    return refs, bounds


def _bitview(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


ATTN_CASES = ap.attention_cases()


@pytest.mark.parametrize("probe,n,hd,dtype", ATTN_CASES, ids=_ids(ATTN_CASES))
def test_attention_probe(gpu, probe, n, hd, dtype):
    """evt_attention (head size 64): the tuned one-pass kernels up to 256 tokens, the streaming
    kernels past them; N on both sides of every kernel, key-block and query-block boundary."""
    case = ap.token_case(probe, n, 64)
    outs, bits = [], []
    for order in (0, 1):
        qkv = _device_qkv(case["rows"], order, TDT[dtype], gpu)
        out = _ops.attention(dtype, qkv, 2, n, H, scale=0.125)
        torch.cuda.synchronize()
        outs.append(out.double().cpu().numpy())
        bits.append([_bitview(out)])
    fam = f"evt_attention {dtype} {'one-pass' if n <= 256 else 'streaming'}"
    _gate(fam, outs, bits, *_token_refs(case, n, 64, dtype), n)


HD_CASES = ap.hd_cases()


@pytest.mark.parametrize("probe,n,hd,dtype", HD_CASES, ids=_ids(HD_CASES))
def test_attention_hd_probe(gpu, probe, n, hd, dtype):
    """evt_attention_hd: the generic kernels (NKT 4 / 8 / 13 / 16 x DP 32 / 64 / 96 / 128, the
    element-wise paths of head sizes 10 and 100) and their streaming forms, into a padded pitch."""
    case = ap.token_case(probe, n, hd)
    outs, bits = [], []
    for order in (0, 1):
        qkv = _device_qkv(case["rows"], order, TDT[dtype], gpu)
        full = torch.full((2 * n, H * hd + 8), 7.0, dtype=TDT[dtype], device=gpu)
        out = full[:, : H * hd]
        _ops.attention_hd(dtype, qkv, 2, n, H, hd, scale=ap.scale_of(hd), out=out)
        torch.cuda.synchronize()
        assert torch.all(full[:, H * hd:] == 7.0), "columns past H * h_k must stay untouched"
        outs.append(out.double().cpu().numpy())
        bits.append([_bitview(out)])
    fam = f"evt_attention_hd {dtype} {'one-pass' if n <= 256 else 'streaming'}"
    _gate(fam, outs, bits, *_token_refs(case, n, hd, dtype), n)


MX8_CASES = ap.mx8_cases()


@pytest.mark.parametrize("probe,n,hd,dtype", MX8_CASES, ids=_ids(MX8_CASES))
def test_attention_mx8_probe(gpu, probe, n, hd, dtype):
    """evt_attention_mx8: the bf16 one-pass kernels with the MX8 epilogue, dequantised with the
    quantiser's oracle; the gate is the bound plus the block's quantisation allowance
    (_attn_probes.mx8_step). Bytes and scale bytes must not depend on the image order."""
    case = ap.token_case(probe, n, 64)
    outs, bits = [], []
    for order in (0, 1):
        qkv = _device_qkv(case["rows"], order, torch.bfloat16, gpu)
        q, s = _ops.attention_mx8(qkv, 2, n, H)
        torch.cuda.synchronize()
        sb = mx8_ref.dwords_to_scales(s.cpu().numpy().view(np.uint32), 2 * n)[:, : H * 2]
        outs.append(mx8_ref.dequantize(q.cpu().numpy()[:, : H * 64], sb))
        bits.append([q[:, : H * 64].contiguous(), torch.from_numpy(sb.copy())])
    refs, bounds = _token_refs(case, n, 64, "mx8")
    bounds = [b + ap.mx8_step(r) for b, r in zip(bounds, refs)]
    _gate("evt_attention_mx8", outs, bits, refs, bounds, n)


WINDOW_CASES = ap.window_cases()


@pytest.mark.parametrize("probe,R,shift,dtype", WINDOW_CASES, ids=_ids(WINDOW_CASES))
def test_window_attention_probe(gpu, probe, R, shift, dtype):
    """evt_window_attention (window 7, head size 32): W-MSA and SW-MSA; the permutation stays
    inside each (window, mask region) group and the bias is a small integer table, the uniform
    probe has a zero bias and sees a masked key that is counted."""
    case = ap.window_case(probe, R, shift)
    T, C = R * R, 32 * H
    rpb = torch.from_numpy(case["rpb"].astype(np.float32)).to(gpu)
    outs, bits = [], []
    for order in (0, 1):
        qkv = _device_qkv(case["rows"], order, TDT[dtype], gpu)
        out = torch.full((2 * T, C), float("nan"), dtype=TDT[dtype], device=gpu)
        _lib.check(_lib.load_library().evt_window_attention(
            _lib.DTYPE[dtype], _p(qkv), qkv.stride(0), _p(out), out.stride(0), _p(rpb), 2, R, C, H,
            shift, _s()))
        torch.cuda.synchronize()
        outs.append(out.double().cpu().numpy())
        bits.append([_bitview(out)])
    refs = [ap.window_rows(r["o"], case["win"], T) for r in case["refs"]]
    bounds = [ap.window_rows(ap.error_bound(r, dtype, 49, 32), case["win"], T) for r in case["refs"]]
    _gate(f"evt_window_attention {dtype}", outs, bits, refs, bounds, T)
