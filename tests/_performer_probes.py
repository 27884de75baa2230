"""Token-exact probe inputs for the TokenPerformer kernels, their fp64 reference and its error bound.

Pure numpy (torch only for the bf16 rounding); no GPU. tests/test_performer_probes_host.py checks
this module on the CPU, tests/test_gpu_performer_probes.py runs the same cases on the kernels of
csrc/t2t.hip (performer_kv_kernel, performer_reduce_kernel, performer_out_kernel,
performer_out16_kernel).

The op takes its weights as arguments, so the probes choose them (`weights`): out_w = I, out_b = 0,
fc2_w = 0, fc2_b = 0, so that out = y2 + (0 . h1 + 0) = v + y exactly as far as the FFN goes (LN2
and FC1 are finite and multiplied by zero), and the random-feature matrix w [32][64] has
w[m][m] = w[m][m + 32] = 2 and zeros elsewhere. Every probe value is a small integer or a power
of two, exact in bf16 and f32; w . k and |k|^2 / 2 are integers below 2^24, so the exponent
x = w . k - |k|^2 / 2 of prm_exp is exact in the kernels whatever their summation order.

Probes (one image of T tokens each, rows (k | q | v) of 64 features)
------
count    k = q = 0: every kp, qp is c = 1 / sqrt(32), ksum[m] = T c, D = T, and with
         v[t] = e_(t mod 64), y[t][n] = S_n / (T + 1e-8) for every token, S_n the number of tokens
         with t mod 64 = n. A token lost from or doubled in kptv (or both sums), a chunk partial
         counted wrongly or a clamped row counted as valid moves feature n of every row by about
         1 / S_n of its value. It cannot see a fault in ksum alone beyond T = 1 in bf16 (1 / T of
         the value), two tokens' v swapped or shifted (equal weights), or a chunk partial skipped
         or doubled (a chunk holds nearly the same share of every feature): `applicable`.
class    token class a < Kc selects random feature a: k = 4 (e_a + e_(a+32)) gives x = 16 - 16 = 0
         for m = a and x = -16 for the others, so the weight of a key of another class is
         2 e^-16 of a matching one (the leak, asserted <= 2^-12 per query on the reference). The
         classes of k and of q come from two different seeded maps, so they cross every tile,
         chunk and span edge; v[t] is a random {+-1, +-2} vector. Row t reads back the mean v of
         the k class that q_t selects: a kp / v mis-pairing in the transposed LDS tiles, a wrong
         lane-to-token map, a shifted tile or swapped output rows is an O(1) error. Kc =
         min(32, T // 2) classes (from T = 64 on all 32 random features and all 64 k / q features
         carry signal), every class has a key and a query, and the last token's class has exactly
         two keys (the other one seeded): what makes a token lost or doubled in ksum alone, a
         relative 1 / (class size) of y, visible in bf16.
hostile  the neighbour image of every case: k = 0 (full weight on every random feature), the
         probe's q, v = 64 everywhere: out = 128 exactly, and a token or partial read across the
         image boundary moves the probe's outputs by tens. Run in both image orders.
fill     (multi-round cases) k, q, v drawn from {-1, 0, +1}; exponents in [-36, 4].

Reference: `core`, fp64, which also returns the intermediates the bound needs.

Bound per output element, derived from csrc/t2t.hip; u = 2^-24 (fp32 round to nearest), h = 2^-8
(bf16 round to nearest, as in _attn_probes.py; h = 0 for the f32 kernels). Reference quantities:
x the exponents, kp, qp, ksum, kptv, D, y = N / (D + 1e-8), out = v + y; A[n][m] = sum_t |v_tn|
kp_tm, a_tn = sum_m qp_tm A[n][m] / (D_t + 1e-8) (the weighted mean of |v|, = |y| when v >= 0).

  e(x) = u (5 + 2 |x|): prm_tile's `__expf(acc - zd) * inv_sqrt_m`. acc - zd is exact (above).
         __expf is v_exp_f32 of x log2(e): the rounded constant and the rounded product move the
         exponent by 2 u |x| log2(e), i.e. the result by 2 u |x| relative; v_exp_f32 is 1 ulp
         = 2 u; the product with inv_sqrt_m u, and inv_sqrt_m = 1.0f / sqrtf(32.0f) is two correctly
         rounded operations, 2 u. (The accurate expf, 1 ulp, is inside the same figure.)
  ksum   fp32 kp summed per lane over the tiles, over 16 lanes, 4 waves and the chunks, in fp32:
         at most T + 8 additions of positive terms in some order, (T + 8) u ksum, plus the exp
         error sum_t kp e(x). ksum is not rounded to bf16 and D uses the fp32 qp.
  kptv   tmma<bf16> rounds kp (h) and v (exact) to bf16 and accumulates in fp32 on the MFMA; we
         take the MFMA's sum as fp32 additions in some order (as _attn_probes.py does for P.V):
         (h + (T + 8) u) A + sum_t |v| kp e(x). The out16 kernel rounds the summed kptv to bf16
         for LDS: h more. The f32 kernels keep fp32 throughout.
  D      32 products and additions in fp32 and two shuffles, (34 u) D; + 1e-8f (u), the reciprocal
         (u; 2 u if the compiler takes v_rcp_f32) and `acc * rden` (u): 4 u.
  N      chain16<bf16> rounds qp to bf16 (h) against the bf16 kptv; 32 terms on the MFMA, 34 u.
  y      altogether  dy = (3 h + (T + 42) u) a + E_N + |y| ((T + 46) u + E_D) with the exp terms
             E_N = sum_m qp (sum_t |v| kp e(x_k) + A e(x_q)) / (D + 1e-8)
             E_D = sum_m qp (ksum e(x_q) + sum_t kp e(x_k)) / (D + 1e-8).
  out    attn_output: chain16<bf16> rounds y to bf16 (h |y|) and multiplies by out_w = I (1.0 and
         0.0 are exact, the sum has one non-zero term); `acc + bo + v` one fp32 addition
         (u |out|); the FFN adds exactly 0; the bf16 store h |out|.

    |got - out| <= (1 + 8 h) (h |out| + u |out| + h |y| + dy) + 1e-37

The factor 1 + 8 h covers the products of the (at most 8) relative errors of size h that the
first-order sum leaves out. Every constant is derived; none was measured.

`emulate` is a legal re-evaluation: fp32 with the kernels' rounding points and numpy's own
summation order over the reversed token axis. The host test holds it to the bound.

Mutations (`MUTATIONS`): deliberately wrong fp64 Performers, as index lists (which kp and which v
enter kptv, which kp enter ksum), an output row permutation and extra tokens of the other image.
`applicable(case, name)` says which mutation a case (probe, T, dtype) can see and why not;
`structural(T, name)` which exist at T at all (a swap needs two tokens, a chunk partial two
chunks, ...). The host test asserts that every mutation that exists at T is seen by a case at T.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
HB = 2.0 ** -8
TINY = 1e-37
LEAK = 2.0 ** -12
HS, M = 64, 32
C64 = 1.0 / math.sqrt(M)

# ---- the cases the GPU file runs (the host file checks every one of them) -----------------------
# performer_launch: nchunk = ceil(T / 196), chunk = ceil(T / nchunk); kv tiles of 16 tokens, 4 waves
# (64 tokens a round); out pass span >= 64.  T -> (nchunk, chunk): 1..196 one chunk | 197: 2 x 99 |
# 392: 2 x 196 | 393: 3 x 131 (chunk starts 131, 262: no multiple of 16).
PROBE_T = (1, 15, 16, 17, 63, 64, 65, 100, 195, 196, 197, 392, 393)
MULTI_T = (100, 200)          # the multi-round out pass (B from the CU count, GPU file)
PROBES = ("count", "class")
DTYPES = ("bf16", "f32")
LDS = ((192, 64), (200, 72), (192, 72), (200, 64))   # (ldq, ldo), cycled over PROBE_T


def probe_cases():
    return [(p, t, dt) for dt in DTYPES for t in PROBE_T + (200,) for p in PROBES]


def ld_of(T):
    return LDS[(PROBE_T + (200,)).index(T) % len(LDS)]


def layout(T):
    """(nchunk, chunk) of performer_launch."""
    nchunk = (T + 195) // 196
    return nchunk, (T + nchunk - 1) // nchunk


def span_of(T, B, cus):
    """Tokens per output workgroup, performer_launch's formula."""
    per_img = max(1, (4 * cus + B - 1) // B)
    return max(64, ((T + per_img - 1) // per_img + 15) & ~15)


def scratch_floats(B, T):
    return B * (layout(T)[0] + 1) * (HS * M + M)


def kqv_col(f):
    """Column of feature f inside its 64 block on the permuted path (t2t.hip kqv_col)."""
    return 16 * ((f >> 2) & 3) + 4 * (f >> 4) + (f & 3)


def permute_rows(rows):
    """[..., 192] rows in reference order -> the order kqv_perm = 1 expects."""
    out = np.empty_like(rows)
    for blk in range(3):
        for f in range(HS):
            out[..., blk * HS + kqv_col(f)] = rows[..., blk * HS + f]
    return out


def bf16_round(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).double().numpy()


def _w():
    w = np.zeros((M, HS))
    w[np.arange(M), np.arange(M)] = 2.0
    w[np.arange(M), np.arange(M) + M] = 2.0
    return w


W = _w()
W.setflags(write=False)


def weights():
    """fp32 weights of the probes in evt_performer's argument order (Keras layouts)."""
    z, one = np.zeros(HS, np.float32), np.ones(HS, np.float32)
    eye = np.eye(HS, dtype=np.float32)
    return dict(w=W.astype(np.float32), out_w=eye, out_b=z, ln2_g=one, ln2_b=z,
                fc1_w=0.5 * eye, fc1_b=z, fc2_w=np.zeros((HS, HS), np.float32), fc2_b=z)


WEIGHT_ORDER = ("w", "out_w", "out_b", "ln2_g", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")


# ---- probe inputs --------------------------------------------------------------------------------
def class_maps(T):
    """(k class, q class) [T] each, Kc: every class has a key and a query, the last token's k
    class (class 0) has exactly two keys when Kc >= 2."""
    Kc = min(M, max(1, T // 2))
    rng = np.random.default_rng(5000 + T)
    if Kc == 1:
        return np.zeros(T, int), np.zeros(T, int), 1
    kc = rng.integers(1, Kc, T)
    partner = int(rng.integers(0, max(1, T - 17))) if T > 18 else 0
    free = np.array([t for t in rng.permutation(T) if t not in (T - 1, partner)])
    kc[free[: Kc - 1]] = np.arange(1, Kc)
    kc[[T - 1, partner]] = 0
    qc = rng.integers(0, Kc, T)
    qc[rng.permutation(T)[:Kc]] = np.arange(Kc)
    return kc, qc, Kc


def probe_kqv(probe, T):
    """(k, q, v) [T, 64] of the probe image."""
    k, q, v = np.zeros((T, HS)), np.zeros((T, HS)), np.zeros((T, HS))
    if probe == "count":
        v[np.arange(T), np.arange(T) % HS] = 1.0
        return k, q, v
    kc, qc, _ = class_maps(T)
    t = np.arange(T)
    k[t, kc] = k[t, kc + M] = 4.0
    q[t, qc] = q[t, qc + M] = 4.0
    v = np.random.default_rng(6000 + T).choice([-2.0, -1.0, 1.0, 2.0], (T, HS))
    return k, q, v


def hostile_kqv(q):
    return np.zeros_like(q), q.copy(), np.full_like(q, 64.0)


def fill_kqv(n, T, seed):
    """n fill images [n, T, 64] x 3 from {-1, 0, +1}."""
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(-1, 2, (n, T, HS)).astype(np.float64) for _ in range(3))


def to_rows(k, q, v):
    return np.concatenate([k, q, v], axis=-1)


# ---- reference and bound -------------------------------------------------------------------------
def _exponent(z):
    return z @ W.T - (z * z).sum(-1, keepdims=True) / 2


def _tn_tm(x, y):        # [.., T, n], [.., T, m] -> [.., n, m], summed over the tokens
    return np.matmul(np.swapaxes(x, -1, -2), y)


def _tm_nm(x, y):        # [.., T, m], [.., n, m] -> [.., T, n]
    return np.matmul(x, np.swapaxes(y, -1, -2))


def _tm_m(x, y):         # [.., T, m], [.., m] -> [.., T]
    return np.matmul(x, y[..., None])[..., 0]


def core(k, q, v):
    """fp64 Performer on [..., T, 64] inputs with the probe weights: out = v + y."""
    xk, xq = _exponent(k), _exponent(q)
    kp, qp = C64 * np.exp(xk), C64 * np.exp(xq)
    ksum = kp.sum(-2)
    kptv = _tn_tm(v, kp)
    D = _tm_m(qp, ksum)
    N = _tm_nm(qp, kptv)
    y = N / (D + 1e-8)[..., None]
    return dict(out=v + y, y=y, D=D, kp=kp, qp=qp, xk=xk, xq=xq, ksum=ksum, kptv=kptv, v=v)


def error_bound(ref, dtype):
    """The module docstring's bound for every output element of `ref` (a `core` result)."""
    h = HB if dtype == "bf16" else 0.0
    kp, qp, xk, xq, y, out = ref["kp"], ref["qp"], ref["xk"], ref["xq"], ref["y"], ref["out"]
    T = kp.shape[-2]
    ek, eq = U * (5 + 2 * np.abs(xk)), U * (5 + 2 * np.abs(xq))
    av = np.abs(ref["v"])
    Dp = (ref["D"] + 1e-8)[..., None]
    A, Ae = _tn_tm(av, kp), _tn_tm(av, kp * ek)
    a = _tm_nm(qp, A) / Dp
    e_n = (_tm_nm(qp, Ae) + _tm_nm(qp * eq, A)) / Dp
    e_d = (_tm_m(qp * eq, ref["ksum"]) + _tm_m(qp, (kp * ek).sum(-2)))[..., None] / Dp
    dy = (3 * h + (T + 42) * U) * a + e_n + np.abs(y) * ((T + 46) * U + e_d)
    return (1 + 8 * HB) * (h * np.abs(out) + U * np.abs(out) + h * np.abs(y) + dy) + TINY


def tstats_bound(stored):
    """[.., 64] stored outputs (fp64 of the bf16 values) -> the bound of the kernel's fp32
    (sum, sumsq): 64 additions each in some order (the squares of bf16 values are exact)."""
    return np.stack([64 * U * np.abs(stored).sum(-1), 64 * U * (stored * stored).sum(-1)], -1) + TINY


def emulate(k, q, v, dtype):
    """A legal evaluation: fp32 with the kernels' rounding points, the token axis reversed and
    numpy's summation order."""
    f = np.float32
    rb = (lambda x: bf16_round(x).astype(f)) if dtype == "bf16" else (lambda x: x)
    c = f(1.0) / np.sqrt(f(M))
    kp = (np.exp(_exponent(k).astype(f)) * c).astype(f)[::-1].copy()
    qp = (np.exp(_exponent(q).astype(f)) * c).astype(f)
    vr = v.astype(f)[::-1].copy()
    ksum = kp.sum(0, dtype=f)
    kptv = rb(np.matmul(vr.T.copy(), rb(kp)).astype(f))              # [64, 32]
    D = (np.matmul(qp[:, ::-1].copy(), ksum[::-1].copy()).astype(f) + f(1e-8)).astype(f)
    N = np.matmul(rb(qp), kptv.T.copy()).astype(f)
    y = (N * (f(1.0) / D)[:, None]).astype(f)
    y2 = (rb(y) + v.astype(f)).astype(f)
    return rb(y2).astype(np.float64)


# ---- mutations -----------------------------------------------------------------------------------
def _swap16(n):
    idx = np.arange(n)
    for t in range(0, n - 1, 16):
        idx[t], idx[t + 1] = idx[t + 1], idx[t]
    return idx


def _last_chunk(T):
    nchunk, chunk = layout(T)
    t_lo = (nchunk - 1) * chunk
    return t_lo, (-(T - t_lo)) % 16       # first row, lanes past the chunk in its last tile


def _mut(T, kp=None, v=None, ks=None, rows=None, extra=0):
    a = np.arange(T)
    return dict(kp=a if kp is None else kp, v=a if v is None else v, ks=a if ks is None else ks,
                rows=a if rows is None else rows, extra=extra)


def _chunk1(T):
    _, chunk = layout(T)
    return np.arange(chunk, min(T, 2 * chunk))


MUTATIONS = {
    "drop_kptv": lambda T: _mut(T, kp=np.arange(T - 1), v=np.arange(T - 1)),
    "drop_ksum": lambda T: _mut(T, ks=np.arange(T - 1)),
    "drop_both": lambda T: _mut(T, kp=np.arange(T - 1), v=np.arange(T - 1), ks=np.arange(T - 1)),
    "double_kptv": lambda T: _mut(T, kp=np.r_[np.arange(T), T - 1], v=np.r_[np.arange(T), T - 1]),
    "double_ksum": lambda T: _mut(T, ks=np.r_[np.arange(T), T - 1]),
    "double_both": lambda T: _mut(T, *(np.r_[np.arange(T), T - 1],) * 3),
    # the rows past the last chunk load the chunk's first row: counted instead of zeroed
    "clamped_valid": lambda T: _mut(T, *(np.r_[np.arange(T), np.full(_last_chunk(T)[1], _last_chunk(T)[0])],) * 3),
    "skip_partial": lambda T: _mut(T, *(np.setdiff1d(np.arange(T), _chunk1(T)),) * 3),
    "double_partial": lambda T: _mut(T, *(np.r_[np.arange(T), _chunk1(T)],) * 3),
    "swap_v": lambda T: _mut(T, v=_swap16(T)),
    "shift_tile": lambda T: _mut(T, v=(np.arange(T) + 16) % T),
    "swap_rows": lambda T: _mut(T, rows=_swap16(T)),
    "other_image": lambda T: _mut(T, extra=1),
}


def structural(T, name):
    """Whether the fault `name` exists at T tokens at all."""
    if name in ("drop_kptv", "drop_ksum", "drop_both", "double_kptv", "double_ksum", "other_image"):
        return True
    if name == "double_both":          # the only token doubled in both sums: the same Performer
        return T >= 2
    if name == "clamped_valid":        # needs a lane past the chunk, and a second token (as above)
        return T >= 2 and _last_chunk(T)[1] > 0
    if name in ("skip_partial", "double_partial"):
        return layout(T)[0] >= 2
    if name == "shift_tile":
        return T > 16
    return T >= 2                      # swap_v, swap_rows


def applicable(case, name):
    """Whether the case (probe, T, dtype) sees the mutation `name` (module docstring, Probes)."""
    probe, T, dtype = case
    if not structural(T, name):
        return False
    if probe == "count":
        if name in ("swap_v", "shift_tile", "skip_partial", "double_partial"):
            return False               # equal weights; a chunk's share of every feature
        if name in ("drop_ksum", "double_ksum"):
            return dtype == "f32" or T == 1     # 1 / T of the value against 5 h
        return True
    Kc = class_maps(T)[2]
    if name in ("swap_v", "shift_tile"):
        return Kc >= 2                 # one class: every key has the same weight
    if name == "clamped_valid":
        # the doubled row must share its class: the last chunk's first token does from Kc = 32 on
        # (about T / 32 keys a class); below, the count probe sees it
        kc = class_maps(T)[0]
        return (kc == kc[_last_chunk(T)[0]]).sum() >= 2
    return True


def mutated(kqv, other, name):
    """fp64 output of the wrong Performer `name` on the image kqv = (k, q, v); other = the
    neighbour image's (k, q, v)."""
    k, q, v = kqv
    T = k.shape[0]
    m = MUTATIONS[name](T)
    kp, qp = C64 * np.exp(_exponent(k)), C64 * np.exp(_exponent(q))
    kptv = v[m["v"]].T @ kp[m["kp"]]
    ksum = kp[m["ks"]].sum(0)
    if m["extra"]:
        okp = C64 * np.exp(_exponent(other[0][: m["extra"]]))
        kptv = kptv + other[2][: m["extra"]].T @ okp
        ksum = ksum + okp.sum(0)
    y = (qp @ kptv.T) / (qp @ ksum + 1e-8)[:, None]
    return (v + y)[m["rows"]]


# ---- cases ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(probe, T):
    """The probe image and its hostile neighbour: kqv [2] of (k, q, v), rows [2][T, 192], `core`
    results and (on demand, `bounds`) their bounds. Shared by every test; arrays are read-only."""
    k, q, v = probe_kqv(probe, T)
    kqv = [(k, q, v), hostile_kqv(q)]
    refs = [core(*x) for x in kqv]
    rows = [to_rows(*x) for x in kqv]
    for a in rows + [z for x in kqv for z in x] + [r[key] for r in refs for key in r]:
        a.setflags(write=False)
    return dict(kqv=kqv, refs=refs, rows=rows)


@functools.lru_cache(maxsize=None)
def bounds(probe, T, dtype):
    out = [error_bound(r, dtype) for r in case(probe, T)["refs"]]
    for a in out:
        a.setflags(write=False)
    return out
