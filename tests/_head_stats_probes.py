"""Inputs, fp64 reference and error bound of the head-statistics tests (include/evt_head_stats.h).

Pure numpy (torch only for the bf16 rounding); no GPU. tests/test_head_stats_host.py checks this
module on the CPU, tests/test_gpu_head_stats.py runs the cases on the kernel.

Inputs (q, k: [B, H, N, hd]; v is never read and is zero)
------
uniform  q = 0, k small random integers: every score is 0, every probability exactly 1 / N.
         confidence = 1 / N, entropy = ln N, cls_mass = prefix / N, distance = the grid's mean
         pairwise distance times (N - prefix) / N. A skipped or doubled key or query moves them by
         about 1 / N; confidence is checked to 2 ulp.
perm     the permutation probe of tests/_attn_probes.py (its codes, its S_PERM, its derangement):
         q_i = s c_i, k_pi(i) = s c_i, so query i keeps >= 1 - 2^-12 on key pi(i) and `distance`
         is, to that leak, the mean d(i, pi(i)): a wrong key-to-cell map at any block edge shows.
         Beyond the 600 codes of that module's pool the same greedy rule (every pairwise dot
         product below hd / 2) is continued on the same stream.
normal   seeded standard-normal q and k, rounded to the dtype under test first.

Reference: `head_stats_reference` (fp64) of the same, already rounded, q and k.

Bound (u = 2^-24). tests/_attn_probes.py derives the relative error eps_ij of one unnormalised
weight e_ij against the others of its row for these kernels' exp2 path; without a bias it is

    eps_ij = u (2 + 3 nkb + 6 (|y_ij| + |y_i,max|) + 7 |y_ij - y_i,max|)

with y the natural-log scores and nkb the number of 64-key blocks the row sum streams over.
head_stats_kernel (as attn_probs_kernel) forms l_i block by block at every N, so nkb = ceil(N / 64)
for N > 64 and 0 up to 64 keys. eps_i = max_j eps_ij. A probability e_ij / l_i moves by at most
2 eps_i relative (numerator and denominator). Per query i, with c_i = max_j p_ij, H_i its entropy,
D_i = sum_{j >= prefix} p_ij d_ij and C_i = sum_{j < prefix} p_ij of the reference:

  confidence  1 / l_i: 2 eps_i c_i.
  entropy     H_i = ln l_i + A_i, A_i = sum_j p_ij (y_i,max - y_ij) >= 0. ln l_i moves by eps_i (l's
              relative error) and by logf's 2 u |ln l_i|; in A_i each p moves by 2 eps_i, each
              exponent t_ij ln 2 by at most eps_ij (the exponent error is part of eps), and the fp32
              sum of N terms in any order, the product and the division add (N + 16) u A_i:
              2 eps_i (H_i + 1) + 2 u ln l_i + (N + 16) u (H_i - ln l_i)      (A_i <= H_i).
  distance    2 eps_i D_i + (N + 16) u D_i: d_ij is the correctly formed sqrt of an exact small
              integer (v_sqrt_f32: 1 ulp = 2 u, inside the 16), N additions in any order.
  cls_mass    2 eps_i C_i + (N + 16) u C_i.

The statistic is the mean of the per-query values; the kernel adds them in fp64 and rounds the mean
to fp32 once, which adds u |value| to `entropy`, `distance` and `cls_mass` (confidence's 2 eps_i >=
4 u already holds it). Plus tiny = 1e-37. Every constant is derived; none was measured.
"""
from __future__ import annotations

import functools

import numpy as np

from edgevisiontransformer_amd.modeling.models.head_stats import head_stats_reference
from tests import _attn_probes as ap

U = ap.U
B, H = 2, 3
# (N, prefix, grid_w): each side of the 16-query tile (16 | 17), the 64-key block and 64-query group
# (64 | 65), two and more groups (129, 197, 257), 5 tokens in one tile, a rectangular grid
# (257: 16 x 16; 129: 16 columns x 8 rows; 1025: 32 x 32), prefix 0 and 1
CASES = ((5, 1, 2), (16, 0, 4), (17, 1, 4), (64, 0, 8), (65, 1, 8), (129, 1, 16),
         (197, 1, 14), (257, 1, 16), (577, 1, 24), (1025, 1, 32))
HD_CASES = tuple((n, p, g, hd) for hd in (32, 80, 128) for (n, p, g) in ((65, 1, 8), (197, 1, 14)))
BIG = (4096, 0, 64)   # B = 1, H = 1, bf16
INPUTS = ("uniform", "perm", "normal")


def _bf16(x):
    return ap.bf16_round(x)


@functools.lru_cache(maxsize=None)
def codes(n, hd):
    """n codes in {-1, +1}^hd, every pairwise dot product below hd / 2: _attn_probes' pool, and
    past its 600 the same greedy rule on a stream of its own."""
    pool = ap.codes(min(n, 600), hd)
    if n <= 600:
        return pool
    out = np.zeros((n, hd))
    out[:600] = pool
    rng = np.random.default_rng(5000 + hd)
    m = 600
    while m < n:
        for c in rng.integers(0, 2, (4096, hd)) * 2.0 - 1.0:
            if (out[:m] @ c).max() < hd / 2:
                out[m] = c
                m += 1
                if m == n:
                    break
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def inputs(kind, n, hd, dtype, b=B, h=H):
    """(q, k) fp64 [b, h, n, hd], already exactly representable in `dtype`; pi [b, h, n] or None."""
    rng = np.random.default_rng(31 * n + hd + {"uniform": 0, "perm": 1, "normal": 2}[kind])
    pi = None
    if kind == "uniform":
        q = np.zeros((b, h, n, hd))
        k = rng.integers(-3, 4, (b, h, n, hd)).astype(np.float64)
    elif kind == "perm":
        c = codes(n, hd)
        q = np.broadcast_to(ap.S_PERM * c, (b, h, n, hd)).copy()
        k = np.zeros((b, h, n, hd))
        pi = np.stack([[ap.derangement(n, rng) for _ in range(h)] for _ in range(b)])
        for i in range(b):
            for j in range(h):
                k[i, j, pi[i, j]] = ap.S_PERM * c
    else:
        q, k = (rng.standard_normal((b, h, n, hd)).astype(np.float32).astype(np.float64)
                for _ in range(2))
        if dtype == "bf16":
            q, k = _bf16(q), _bf16(k)
    q.setflags(write=False)
    k.setflags(write=False)
    return q, k, pi


def qkv_rows(q, k):
    """[b, h, n, hd] x 2 -> float32 rows [b n, 3 h hd], columns (qkv, h, d); v = 0."""
    b, h, n, hd = q.shape
    x = np.stack([q, k, np.zeros_like(q)], axis=2)          # [b, h, 3, n, hd]
    return np.ascontiguousarray(x.transpose(0, 3, 2, 1, 4).reshape(b * n, 3 * h * hd), np.float32)


def reference_and_bound(q, k, prefix, grid_w):
    """(ref [b, h, 4] fp64, bound [b, h, 4]) by the module docstring, one (image, head) at a time
    (N = 4096 is 128 MB of fp64 per matrix)."""
    b, h, n, hd = q.shape
    scale = ap.scale_of(hd)
    nkb = -(-n // 64) if n > 64 else 0
    ref, bound = np.zeros((b, h, 4)), np.zeros((b, h, 4))
    for i in range(b):
        for j in range(h):
            y = (q[i, j] @ k[i, j].T) * scale
            ymax = y.max(-1, keepdims=True)
            e = np.exp(y - ymax)
            l = e.sum(-1, keepdims=True)
            p = e / l
            r = head_stats_reference(p, prefix=prefix, grid_w=grid_w)
            eps = (U * (2 + 3 * nkb + 6 * (np.abs(y) + np.abs(ymax)) + 7 * np.abs(y - ymax))).max(-1)
            lnl = np.log(l[:, 0])
            with np.errstate(divide="ignore", invalid="ignore"):
                ent = -np.where(p > 0, p * np.log(p), 0.0).sum(-1)
            d = _dist_rows(p, prefix, grid_w)
            cm = p[:, :prefix].sum(-1)
            pq = slice(prefix, None)
            bound[i, j, 0] = (2 * eps * p.max(-1)).mean()
            bound[i, j, 1] = (2 * eps * (ent + 1) + 2 * U * lnl
                              + (n + 16) * U * np.maximum(ent - lnl, 0.0)).mean() + U * abs(r[1])
            bound[i, j, 2] = ((2 * eps[pq] + (n + 16) * U) * d).mean() + U * abs(r[2])
            bound[i, j, 3] = ((2 * eps[pq] + (n + 16) * U) * cm[pq]).mean() + U * abs(r[3])
            ref[i, j] = r
    return ref, bound + ap.TINY


def _dist_rows(p, prefix, grid_w):
    """D_i of the patch queries: sum_{j >= prefix} p_ij d_ij, [n - prefix]."""
    from edgevisiontransformer_amd.modeling.models.head_stats import patch_distances
    return (p[prefix:, prefix:] * patch_distances(p.shape[-1] - prefix, grid_w)).sum(-1)


@functools.lru_cache(maxsize=None)
def case(kind, n, prefix, grid_w, hd, dtype, b=B, h=H):
    """Everything a test needs of one case, built once and shared: rows (float32, exactly
    representable in `dtype`), ref, bound, pi."""
    exact = kind != "normal"   # integer and power-of-two values: the same in both dtypes
    q, k, pi = inputs(kind, n, hd, "f32" if exact else dtype, b, h)
    ref, bound = _ref_cached(kind, n, prefix, grid_w, hd, "f32" if exact else dtype, b, h)
    rows = qkv_rows(q, k)
    rows.setflags(write=False)
    return dict(rows=rows, ref=ref, bound=bound, pi=pi, q=q, k=k)


@functools.lru_cache(maxsize=None)
def _ref_cached(kind, n, prefix, grid_w, hd, dtype, b, h):
    q, k, _ = inputs(kind, n, hd, dtype, b, h)
    ref, bound = reference_and_bound(q, k, prefix, grid_w)
    ref.setflags(write=False)
    bound.setflags(write=False)
    return ref, bound
