"""Inputs, fp64 reference and error bound of the FFN-statistics tests (include/evt_ffn_stats.h).

Pure numpy; no GPU. tests/test_ffn_stats_host.py checks this module on the CPU,
tests/test_gpu_ffn_stats.py runs the cases on the kernel (ffn_stats_kernel, csrc/ffn_stats.hip).

Inputs (hidden: [B, T, F] fp32 values that are exact in the dtype under test)
------
ints    seeded integers in [-8, 8]: every sum (at most 4096 * 64) is an integer below 2^24, exact
        in fp32 in any order. Statistics 0-2 must equal the correctly rounded quotient sum / T to
        1 ulp, max_abs bitwise.
onehot  column j is zero except at token j % T, where it holds (j % 251 + 1) / 4 (a multiple of 1/4
        up to 63: exact in bf16). mean = mean_abs = v / T, mean_sq = v^2 / T, max_abs = v: a skipped
        or doubled row, or a column landing in another output slot, shows in all of them.
signs   column j is c_j (-1)^(t + j), c_j = (j % 61 + 3) / 8: mean_abs = c_j and max_abs = c_j
        exactly, mean_sq = c_j^2; the mean is exactly 0 for even T and +-c_j / T for odd T (every
        partial sum, in any order, is a small integer multiple of c_j or c_j^2: exact in fp32).
normal  seeded N(0, 1), rounded to the dtype under test before the reference sees it.

Reference: `ffn_stats_reference` (fp64) of the same, already rounded, values.

Bound (u = 2^-24, the unit roundoff of fp32)
-----
The stored values are exact inputs of the reduction (bf16 -> fp32 is exact). For one column let
S = sum_t x_t of T fp32 terms x_t, added in fp32 in any order and any grouping (the kernel: four
interleaved chains of ceil(T / 4) terms, then three more additions). Every term passes through at
most T - 1 additions, each of relative error at most u, so

    |fl(S) - S| <= ((1 + u)^(T - 1) - 1) sum |x_t| <= 1.001 (T - 1) u sum |x_t|      (T <= 4096).

  mean      x_t = a_t: the sum, then one correctly rounded division by T (1 u more):
            (1.001 (T - 1) + 1.001) u mean_abs <= (T + 16) u mean_abs.
  mean_abs  x_t = |a_t| (exact): the same, (T + 16) u mean_abs.
  mean_sq   x_t = a_t^2: exact for bf16 (an 8-bit significand squared), and for f32 formed inside
            the fused multiply-add of the accumulation, which rounds once (the one rounding already
            counted for that addition). A kernel that rounded the product on its own would add 1 u:
            (1.001 T + 1.001) u mean_sq <= (T + 16) u mean_sq covers both.
  max_abs   a maximum of stored values: 0.

Plus tiny = 1e-37 throughout (a reference of exactly 0 allows no error: `signs` at even T). The 16
is head-room for the 1.001 factors at T = 4096 (4.1) and the division, not a fitted constant; no
constant here was measured.
"""
from __future__ import annotations

import numpy as np

from edgevisiontransformer_amd.modeling.models.ffn_stats import ffn_stats_reference

U = 2.0 ** -24
TINY = 1e-37
B = 2
INPUTS = ("ints", "onehot", "signs", "normal")
# F: each side of a lane's 16-byte vector (f32: 4, bf16: 8), of 64 columns (the padded pitch of the
# tests, ld = F rounded up to 64), of a workgroup's column slab = one wave's 1 KiB row (f32: 256,
# bf16: 512), several slabs with a ragged tail (1544 = 3 * 512 + 8 = 6 * 256 + 8), and 200 (a
# pruned model's width: no multiple of 64)
WIDTHS = (1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 200, 255, 256, 257, 511, 512, 513, 1544)
# T: fewer rows than the four waves, each side of the wave split (4) and of the four-row unroll of a
# wave (16 | 17), and DeiT's 197
TOKENS = (1, 3, 4, 5, 17, 197)
BIG = (1, 4096, 64)   # (B, T, F)


def bf16_round(x) -> np.ndarray:
    """fp32 values rounded to the nearest bf16 (ties to even), as fp32."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    bits = a.view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).reshape(a.shape)


def round_to(x, dtype: str) -> np.ndarray:
    a = np.asarray(x, dtype=np.float32)
    return bf16_round(a) if dtype == "bf16" else a


def hidden(kind: str, b: int, t: int, f: int, dtype: str) -> np.ndarray:
    """The [b, t, f] fp32 input of `kind`, every value exact in `dtype`."""
    rng = np.random.default_rng(1000 * t + f + {"ints": 1, "normal": 2}.get(kind, 0) * 7919)
    j = np.arange(f)
    tt = np.arange(t)
    if kind == "ints":
        a = rng.integers(-8, 9, size=(b, t, f)).astype(np.float32)
    elif kind == "onehot":
        a = np.zeros((b, t, f), np.float32)
        a[:, j % t, j] = ((j % 251 + 1) / 4.0).astype(np.float32)
    elif kind == "signs":
        c = ((j % 61 + 3) / 8.0).astype(np.float32)
        a = np.broadcast_to(c[None, :] * (1.0 - 2.0 * ((tt[:, None] + j[None, :]) % 2)),
                            (b, t, f)).astype(np.float32)
    elif kind == "normal":
        a = rng.standard_normal((b, t, f), dtype=np.float32)
    else:
        raise ValueError(kind)
    r = round_to(a, dtype)
    if kind != "normal":
        assert np.array_equal(r, a), f"{kind}: not exact in {dtype}"
    return r


def bound(ref: np.ndarray, t: int) -> np.ndarray:
    """The module docstring's bound for a reference [..., F, 4] over `t` tokens."""
    out = np.empty_like(ref)
    out[..., 0] = out[..., 1] = (t + 16) * U * ref[..., 1]
    out[..., 2] = (t + 16) * U * ref[..., 2]
    out[..., 3] = 0.0
    return out + TINY


def case(kind: str, t: int, f: int, dtype: str, b: int = B) -> dict:
    a = hidden(kind, b, t, f, dtype)
    ref = ffn_stats_reference(a)
    return {"hidden": a, "ref": ref, "bound": bound(ref, t)}


def exact_quotient(ref: np.ndarray) -> np.ndarray:
    """fp32 nearest of the fp64 statistics (for inputs whose sums are exact in fp32 the fp64 value
    is sum / T to 2^-53, so this is the correctly rounded quotient)."""
    return ref.astype(np.float32)
