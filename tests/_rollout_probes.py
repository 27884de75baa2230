"""Inputs, fp64 reference and error bound of the attention-rollout tests (include/evt_rollout.h).

Pure numpy (torch only for the bf16 rounding); no GPU. tests/test_rollout_host.py checks this
module on the CPU, tests/test_gpu_rollout.py runs the cases on the kernels.

Inputs
------
A chain of STEPS = 3 rollout steps. Step s has its own q and k, [B, H, N, hd]: the `uniform`, `perm`
and `normal` inputs of tests/_head_stats_probes.py, drawn once for STEPS * B images from that
module's stream and cut into STEPS groups of B, so the steps are independent draws (v is never
read and is zero).

uniform  every probability is exactly 1 / N in every head and step: Abar = J / N and the rollout
         after L steps is 2^-L I + (1 - 2^-L) / N J, whatever N. A skipped or doubled row, column
         or k of the matrix step moves an element by about 1 / N.
perm     Abar is, to the 2^-12 leak, the mean of H permutation matrices, different in every step:
         the chain is a product of sparse matrices in which a wrong row-to-column map at any tile
         or chunk edge is an O(1 / H) error.
normal   seeded standard-normal q and k, rounded to the dtype under test first.

Reference: the contract in fp64 (softmax of the same, already rounded, q and k; `rollout_reference`
of edgevisiontransformer_amd.modeling.models.rollout on those probabilities).

Bound (u = 2^-24). Every quantity is non-negative, so nothing cancels and every error stays
relative to its element. tests/_attn_probes.py derives the relative error eps_ij of one
unnormalised weight of these kernels' exp2 path,

    eps_ij = u (2 + 3 nkb + 6 (|y_ij| + |y_i,max|) + 7 |y_ij - y_i,max|)

(y the natural-log scores, nkb = ceil(N / 64) blocks for N > 64 and 0 up to 64 keys: the head mean
forms l_i block by block like attn_probs_kernel); a probability moves by at most 2 eps_i,
eps_i = max_j eps_ij. One step computes, for row i,

    R_out[i][j] = 0.5 (R_in[i][j] + sum_k Abar[i][k] R_in[k][j]),   Abar[i][k] = (sum_h p_h[i][k]) fl(1 / H)

  p_h[i][k]       2 eps_i (the largest over the heads)
  the head sum    H - 1 fp32 additions of non-negative terms: (H - 1) u
  times fl(1 / H) the rounded reciprocal and the product: 2 u (exact for H a power of two)
  the product     a k-ordered fmaf chain from 0 over T terms (the exact fp32 MFMA: one rounding
                  per term, the products unrounded): T u, in any order
  + R_in[i][j]    one addition: u. In the first step R_in = I, the sum is Abar itself and this is
                  where the diagonal's + 1 rounds (off the diagonal the + 0 is exact)
  times 0.5       exact (an underflow is inside tiny)

so a step adds at most x_i = 2 eps_i + (H + T + c) u relative to each element of row i with
c = 2: (H - 1) + 2 + T + 1. R_in[k][j] carries the error of ITS row k of the steps before, so the
relative error of row i after a step is at most E_i = x_i + max_k E_k(before): over L steps the
terms add to first order. The neglected products of these terms are closed rigorously by
prod (1 + a) - 1 <= X / (1 - X), X their sum: bound = ref E / (1 - E) + tiny, tiny = 1e-37. (E is
below 1e-3 in every case here, so the closure changes the bound by less than a part in 1000.)
Every constant is derived; none was measured.

Row sums: the reference's rows sum to 1, so a row of the result sums to 1 within the sum of its
elements' bounds. The mean of H identical heads is not exact (p + p + p rounds, and so does the
product with fl(1 / 3)), so there is no H = 1 against H = 3 bitwise check.
"""
from __future__ import annotations

import functools

import numpy as np

from edgevisiontransformer_amd.modeling.models.rollout import rollout_reference
from tests import _attn_probes as ap
from tests import _head_stats_probes as hp

U = ap.U
TINY = ap.TINY
B, H, STEPS = 2, 3, 3
C = 2  # the c of a step's (H + T + c) u (module docstring)
# N: each side of the 16-query tile (16 | 17), of the 64-key block, the 64-query group and the step
# kernel's 64 x 64 tile (64 | 65; 128 | 129 two tiles), of its 32-token k chunk (32 | 33), 5 tokens
# in one tile, two and more groups (129, 197, 257)
NS = (5, 16, 17, 32, 33, 64, 65, 128, 129, 197, 257)
HD_CASES = tuple((n, hd) for hd in (32, 80, 128) for n in (65, 197))
BIG = (577, 1025)   # B = 1, H = 1, bf16
INPUTS = hp.INPUTS


def softmax64(q, k, scale):
    """(p, y) fp64 of [..., N, hd] q and k."""
    y = np.einsum("...id,...jd->...ij", q, k) * scale
    e = np.exp(y - y.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True), y


def step_terms(eps_rows, heads, n):
    """x_i of the module docstring from eps_i [..., N] (already the largest over the heads)."""
    return 2.0 * eps_rows + (heads + n + C) * U


def chain_bound(ref, xs):
    """bound [..., N, N] of a chain whose steps have the per-row terms xs[s] [..., N]."""
    e = np.zeros_like(xs[0])
    for x in xs:
        e = x + e.max(-1, keepdims=True)
    assert (e < 0.5).all()
    return ref * (e / (1.0 - e))[..., None] + TINY


def eps_rows(y, n):
    """eps_i [..., N]: the largest eps_ij over the keys and the heads (axis -3) of scores y."""
    nkb = -(-n // 64) if n > 64 else 0
    ymax = y.max(-1, keepdims=True)
    eps = U * (2 + 3 * nkb + 6 * (np.abs(y) + np.abs(ymax)) + 7 * np.abs(y - ymax))
    return eps.max(-1).max(-2)


@functools.lru_cache(maxsize=None)
def case(kind, n, hd, dtype, b=B, h=H):
    """Everything a test needs of one case, built once and shared (read-only): rows[s] (float32
    [b n, 3 h hd], exactly representable in `dtype`), ref[s] and bound[s] [b, n, n] after steps
    0 .. s, maps[s] the fp64 probabilities [b, h, n, n]."""
    exact = kind != "normal"   # integer and power-of-two values: the same in both dtypes
    q, k, _ = hp.inputs(kind, n, hd, "f32" if exact else dtype, STEPS * b, h)
    scale = ap.scale_of(hd)
    rows, maps, xs, refs, bounds = [], [], [], [], []
    for s in range(STEPS):
        qs, ks = q[s * b:(s + 1) * b], k[s * b:(s + 1) * b]
        p, y = softmax64(qs, ks, scale)
        rows.append(hp.qkv_rows(qs, ks))
        maps.append(p)
        xs.append(step_terms(eps_rows(y, n), h, n))
        refs.append(rollout_reference(maps))
        bounds.append(chain_bound(refs[-1], xs))
    for a in rows + maps + refs + bounds:
        a.setflags(write=False)
    return dict(rows=rows, maps=maps, ref=refs, bound=bounds)


def uniform_closed_form(n, steps):
    return 2.0 ** -steps * np.eye(n) + (1.0 - 2.0 ** -steps) / n * np.ones((n, n))


def fp32_chain(maps):
    """The chain re-evaluated in numpy float32 from the fp64 probabilities rounded to fp32: head sum
    in index order, times fl(1 / H), fp32 matrix product, the + and the halving."""
    r = None
    for p in maps:
        p32 = p.astype(np.float32)
        acc = np.zeros_like(p32[..., 0, :, :])
        for hh in range(p32.shape[-3]):
            acc = acc + p32[..., hh, :, :]
        abar = acc * (np.float32(1.0) / np.float32(p32.shape[-3]))
        if r is None:
            r = np.float32(0.5) * (abar + np.eye(abar.shape[-1], dtype=np.float32))
        else:
            r = np.float32(0.5) * (r + np.matmul(abar, r))
    return r
