"""Key-exact probe inputs for the attention kernels, their fp64 reference and its error bound.

Pure numpy (torch only for the bf16 rounding); no GPU. tests/test_attn_probes_host.py checks this
module on the CPU, tests/test_gpu_attn_probes.py runs the same cases on the kernels.

Layout: that of `_attn_ref_hd` (tests/test_gpu_ops.py): qkv rows are tokens, columns (qkv, h, d).
Every probe value is a small integer or a power of two, so it is exact in bf16, f32 and E4M3, and
every q.k product sum is an exact fp32 integer: the kernels' raw scores carry no rounding.

Probes
------
uniform       q = 0, k random integers, v in {-1, +1}. Every score is 0, every unnormalised weight
              is 2^0 = 1 in a kernel that subtracts the maximum, o_id = (n+ - n-) / N. A lost,
              doubled or wrongly unmasked key moves an output by about 1 / N.
permutation   (head size >= 32) token i has a code c_i in {-1, +1}^hd; q_i = s c_i,
              k_pi(i) = s c_i, v_j a random {+-1, +-2} vector, pi a fixed derangement (seeded; it
              maps across every tile boundary). Query i reads back v_pi(i): a swapped row, a wrong
              tile offset or lane-to-key map is an O(1) error. s = 2: the matching score is
              4 sqrt(hd) (22.6 at hd 32 .. 45.3 at hd 128, below 80). The codes are drawn greedily
              with every pairwise dot product below hd / 2, which is what keeps the reference's
              weight on key pi(i) >= 1 - 2^-12 (asserted on the reference by the host test for
              every case; doubling s is not open at hd 32, where 16 sqrt(32) = 90.5 > 80, so the
              condition is met by the choice of codes). N = 1 has no derangement, and head sizes
              10 and 24 cannot separate the keys: uniform only there.
hostile       B = 2. The other image has k = 4 x the codes and v = 64 everywhere: a key read
              across the image boundary moves an output by tens. Run in both image orders.

Reference: `core` (fp64 softmax attention on [G, n, hd] groups, optional additive bias), which
also returns the softmax matrix p and the scores the bound needs.

Bound per output element (p, o64 from the reference, a = sum_j p_j |v_jd|, u = 2^-24):

    |o - o64| <= u_out |o64| + r_P + (N + hd + 8) u a + E + tiny

  u_out  2^-8 for a bf16 output, 2^-24 for an fp32 one (and for the MX8 output, which is quantised
         from the fp32 value; its gate adds the block's quantisation step, `mx8_step`).
         bf16 keeps 8 significand bits (7 stored), so round-to-nearest is off by up to half an
         ulp = 2^-8 of the binade: 1 / 15 = 0.066667 rounds to 0.066895, 2^-8.2 relative. A
         2^-9 (half of that, the figure first proposed for this gate) fails an exactly computed,
         correctly rounded output, which test_attn_probes_host.py shows with its re-evaluation.
  r_P    the bf16 rounding of the P operand in the bf16 kernels: 2^-8 sum_{j: s_j != m} p_j |v_jd|.
         This is sum_j |bf16(e_j) - e_j| |v_jd| / sum_j e_j (e_j = exp(s_j - m)) with each
         |bf16(e) - e| replaced by its upper limit 2^-8 e for every key but the row maxima: the
         kernel rounds
         its own e_j (off by the relative eps_j below, and in the streaming kernels taken against
         the running maximum and rescaled later), not the reference's, and a value next to a
         rounding boundary can round the other way. A key at the row maximum has e = 1 up to
         eps_j, which rounds to 1. So r_P is exactly 0 in the uniform probe and below
         2^-8 2^-12 2 in the permutation probe; 0 for the fp32 kernels.
  (N + hd + 8) u a: N fp32 additions in the row sum and in P.V in any order, the score's hd
         additions (exact on these inputs), and 1 / l, its product and slack.
  E      the kernels' exp2 path, per key (the issue's e_exp a with e_exp taken per key and weighed
         by p_j; never more than 2 max_j(eps_j) a):
             E = sum_j p_j eps_j (|v_jd| + |o64_d|) / (1 - max eps)
         (numerator and denominator of the softmax each move by sum_j p_j eps_j). eps_j is the
         relative error of key j's weight against the other keys of its row. Derived from
         attention.hip / swin.hip, y = natural-log score, y_qk its q.k part, b its bias part:
           * __builtin_amdgcn_exp2f is v_exp_f32, 1 ulp = 2 u relative; exp2f (the fp32 kernels)
             is the same instruction plus a denormal range fix: 2 u.
           * c = scale * log2(e) in fp32: the rounded constant (u), the product (u) and, for the
             window kernels' literal 32^-0.5, the rounded scale (u): |dc| <= 3 u relative, which
             moves the exponent of key j by at most 3 u |y_qk,j| log2(e).
           * the exponent s c + mo (mo = -m c rounded; FMA or not): u |y_qk| log2(e) for each of
             the two products and u |t| for the sum; the window kernels add the rounded bias
             b log2(e) (u |b|) and subtract the maximum afterwards (u |t|). In the fp32 kernels
             the error of mo is common to the row and cancels, in the bf16 kernels P is rounded
             and l is not, so it does not: both are covered by charging key j with its own and
             the row maximum's terms, 6 u (|y_qk,j| + |b_j| + |y_qk,max| + |b_max|) together with
             dc, in natural-log units (d 2^t / 2^t = ln 2 dt).
           * u |y_j - y_max| for the rounding of the difference.
           * streaming kernels (N > 256, nkb = ceil(N / 64) blocks): a key's weight is taken
             against the running maximum and multiplied by at most nkb - 1 factors
             2^((m_old - m_new) c), each 2 u (exp2) + u (the product) and 6 u |dy| for its
             exponent; the |dy| telescope to at most |y_j - y_max|: 3 nkb u + 6 u |y_j - y_max|.
         Together  eps_j = u (2 + 3 nkb + 6 (|y_qk,j| + |b_j| + |y_qk,max| + |b_max|)
                             + 7 |y_j - y_max|),  nkb = 0 up to 256 keys.
         In the uniform probe with a zero bias this is 2 u.
  tiny   1e-37.
Every constant above is derived; none was measured.

Mutations (`MUTATIONS`): fp64 outputs of deliberately wrong attentions, as key index lists for
K (and the bias columns) and for V. `past_n` reads the row a clamped load reads (row N - 1), as
the kernels' staging does, so it equals `double_last`; both are kept because they name different
faults. `swap_v` leaves the uniform probe unchanged (equal weights), a doubled key leaves the
permutation probe unchanged (the one query that reads it gets (v + v) / 2) and `skip_block` needs
N > 256: `applicable` says which mutation a case can see.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import mx8_ref, swin_ref

U = 2.0 ** -24
TINY = 1e-37
S_PERM = 2.0         # q / k magnitude of the permutation probe
LEAK = 2.0 ** -12    # the reference keeps >= 1 - LEAK on key pi(i)
H = 2

# ---- the cases the GPU file runs (the host file checks every one of them) -----------------------
# evt_attention, head size 64. N -> kernel (attention_launch):
#   bf16: 1..64 NKT 4 | 65..128 NKT 8 (launch_nkt<8>) | 129..192 NKT 12 | 193..208 NKT 13 (half
#         PV step: 193 leaves one valid key in it, 208 fills it) | 209..224 NKT 14 | 225..256
#         NKT 16 | 257.. attn_long_bf16_kernel (64-key blocks: 320 | 321, 384 | 385; 128 queries
#         per workgroup: 256 | 257, 384 | 385; 577: 10 key blocks, 5 query blocks)
#   f32:  1..64 NKT 4 | 65..128 NKT 8 | 129..224 NKT 14 | 225..256 NKT 16 | 257.. attn_long_f32
#         (64-key blocks, 64 queries per workgroup: 320 | 321, 384 | 385)
ATTN_N = (1, 15, 16, 17, 63, 64, 65, 100, 127, 128, 129, 191, 192, 193, 207, 208, 209, 223, 224,
          225, 255, 256, 257, 319, 320, 321, 384, 385, 577)
# evt_attention_hd. N -> generic kernel (attention_gen_launch): 1..64 NKT 4 | 65..128 NKT 8 |
# 129..208 NKT 13 | 209..256 NKT 16 | 257.. attn_long_gen_bf16 / attn_long_f32 (64 | 64);
# head size -> DP 32 (10, 24, 32) | 64 (48) | 96 (72, 96) | 128 (100, 128); fp32: one feature
# group up to 64, two above.
HD_N = (17, 64, 65, 128, 129, 208, 209, 256, 257, 321)
HD_BOTH = (32, 48, 72, 96, 100, 128)   # the condition on the reference holds: both probes
HD_UNIFORM = (10, 24)                  # keys cannot be separated below 32 features
# evt_attention_mx8 (bf16 in, the NKT 4 / 8 / 12 / 13 / 16 bf16 kernels with the MX8 epilogue).
# The uniform probe is not run here: its outputs are multiples of 1 / N below the block's E4M3
# step (2^-3 of the block maximum), so no mutation reaches 4 x the gate (checked by
# test_attn_probes_host.py::test_mx8_uniform_cannot_see_a_key).
MX8_N = (64, 65, 128, 129, 193, 208, 256)
# evt_window_attention (window 7, head size 32): W-MSA and SW-MSA at the smallest R with shifted
# windows. The window-12 kernels have no op-level entry point (they are reached through the
# model only, tests/test_gpu_swin_w12.py), so they have no probe here.
WINDOW_RS = ((14, 0), (14, 3))
DTYPES = ("bf16", "f32")


def attention_cases():
    return [(probe, n, 64, dt) for dt in DTYPES for n in ATTN_N for probe in ("uniform", "perm")
            if not (probe == "perm" and n == 1)]


def hd_cases():
    out = []
    for dt in DTYPES:
        for hd in sorted(HD_BOTH + HD_UNIFORM):
            for n in HD_N:
                out.append(("uniform", n, hd, dt))
                if hd in HD_BOTH:
                    out.append(("perm", n, hd, dt))
    return out


def mx8_cases():
    return [("perm", n, 64, "mx8") for n in MX8_N]


def window_cases():
    return [(probe, r, s, dt) for dt in DTYPES for (r, s) in WINDOW_RS
            for probe in ("uniform", "perm")]


# ---- building blocks -----------------------------------------------------------------------------
def bf16_round(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).double().numpy()


@functools.lru_cache(maxsize=None)
def _code_pool(hd):
    """Up to 600 codes in {-1, +1}^hd, every pairwise dot product below hd / 2 (greedy over a
    seeded stream, so a prefix of the pool is a valid set too)."""
    rng = np.random.default_rng(1000 + hd)
    pool = np.zeros((600, hd))
    n = 0
    while n < 600:
        for c in rng.integers(0, 2, (4096, hd)) * 2.0 - 1.0:
            if n == 0 or (pool[:n] @ c).max() < hd / 2:
                pool[n] = c
                n += 1
                if n == 600:
                    break
    pool.setflags(write=False)
    return pool


def codes(n, hd):
    if hd >= 32:
        return _code_pool(hd)[:n]
    return np.random.default_rng(1000 + hd).integers(0, 2, (600, hd))[:n] * 2.0 - 1.0


def derangement(n, rng):
    """A permutation of range(n) without fixed points (n >= 2)."""
    while True:
        pi = rng.permutation(n)
        if not np.any(pi == np.arange(n)):
            return pi


def to_rows(q, k, v):
    """[H, n, hd] each -> qkv rows [n, 3 H hd], columns (qkv, h, d)."""
    x = np.stack([q, k, v])                       # [3, H, n, hd]
    return x.transpose(2, 0, 1, 3).reshape(q.shape[1], -1)


def from_rows(o, hd):
    """output rows [n, H hd] -> [H, n, hd]."""
    n = o.shape[0]
    return o.reshape(n, -1, hd).transpose(1, 0, 2)


def _probe_qkv(probe, n, hd, seed):
    """(q, k, v) [H, n, hd] of the probe image, pi [H, n] (None for the uniform probe)."""
    rng = np.random.default_rng(seed)
    if probe == "uniform":
        q = np.zeros((H, n, hd))
        k = rng.integers(-3, 4, (H, n, hd)).astype(np.float64)
        v = rng.integers(0, 2, (H, n, hd)) * 2.0 - 1.0
        return q, k, v, None
    c = codes(n, hd)
    q = np.broadcast_to(S_PERM * c, (H, n, hd)).copy()
    k = np.zeros((H, n, hd))
    pi = np.stack([derangement(n, rng) for _ in range(H)])
    for h in range(H):
        k[h, pi[h]] = S_PERM * c
    v = rng.choice([-2.0, -1.0, 1.0, 2.0], (H, n, hd))
    return q, k, v, pi


def _hostile_qkv(q, n, hd):
    """The neighbour image: the probe's queries, k = 4 x the codes, v = 64."""
    k = np.broadcast_to(4.0 * codes(n, hd), (H, n, hd)).copy()
    return q.copy(), k, np.full((H, n, hd), 64.0)


def core(q, k, v, scale, bias=None):
    """fp64 softmax attention on groups: q, k, v [G, n, hd], additive bias [G, nq, nk] or None."""
    yqk = np.einsum("gid,gjd->gij", q, k) * scale
    y = yqk if bias is None else yqk + bias
    e = np.exp(y - y.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    return dict(o=p @ v, p=p, y=y, yqk=yqk, bias=bias, v=v)


def error_bound(ref, dtype, n_keys, hd):
    """The module docstring's bound for every output element of `ref` (a `core` result).
    dtype: 'bf16' | 'f32' | 'mx8' (bf16 kernel, fp32 value before the quantiser)."""
    p, y, yqk, v, o = ref["p"], ref["y"], ref["yqk"], np.abs(ref["v"]), np.abs(ref["o"])
    b = np.zeros_like(y) if ref["bias"] is None else np.abs(ref["bias"])
    nkb = -(-n_keys // 64) if n_keys > 256 else 0
    ymax = y.max(-1, keepdims=True)
    jm = y.argmax(-1)[..., None]
    lin = np.abs(yqk) + b
    eps = U * (2 + 3 * nkb + 6 * (lin + np.take_along_axis(lin, jm, -1)) + 7 * np.abs(y - ymax))
    w = p * eps
    e_term = (w @ v + w.sum(-1, keepdims=True) * o) / (1.0 - eps.max())
    a = p @ v
    u_out = 2.0 ** -8 if dtype == "bf16" else U
    r_p = 0.0 if dtype == "f32" else 2.0 ** -8 * ((p * (y != ymax)) @ v)
    return u_out * o + r_p + (n_keys + hd + 8) * U * a + e_term + TINY


def mx8_step(o_rows):
    """[rows, K] fp64 reference output -> per element, the quantisation allowance of its
    32-element block, from the block scale X = 2^(s - 127) of the quantiser's oracle
    (oracle/mx8_ref.py): two E4M3 steps of the block's top binade, 2 x 32 X. One step covers
    round-to-nearest (16 X) and a device block maximum on the other side of a power of two (the
    scale one binade off: 16 X' = 32 X, or the clamp of (448, 512) X' to 448 X' = 32 X); the
    second covers the OCP clamp of (448, 512) X to 448 X at the reference's own scale (64 X)."""
    _, sb = mx8_ref.quantize(o_rows.astype(np.float32))
    x = np.exp2(sb.astype(np.float64) - 127.0)
    return np.repeat(64.0 * x, 32, axis=1)


# ---- mutations: (key index list for K / bias, key index list for V) ------------------------------
def _swap16(n):
    idx = np.arange(n)
    for t in range(0, n - 1, 16):
        idx[t], idx[t + 1] = idx[t + 1], idx[t]
    return idx


MUTATIONS = {
    "drop_last": lambda n: (np.arange(n - 1),) * 2,
    "double_last": lambda n: (np.r_[np.arange(n), n - 1],) * 2,
    "past_n": lambda n: (np.r_[np.arange(n), min(n, n - 1)],) * 2,   # the clamped row
    "swap_v": lambda n: (np.arange(n), _swap16(n)),
    "skip_block": lambda n: (np.r_[np.arange(64), np.arange(128, n)],) * 2,   # block b = 1
}


def applicable(probe, n):
    if n < 2:
        return []
    names = ["drop_last"]
    names += ["swap_v"] if probe == "perm" else ["double_last", "past_n"]
    if n > 256:
        names.append("skip_block")
    return names


def mutated(ref_in, name):
    """fp64 output of the wrong attention `name` on the inputs (q, k, v, scale, bias)."""
    q, k, v, scale, bias = ref_in
    kidx, vidx = MUTATIONS[name](k.shape[1])
    return core(q, k[:, kidx], v[:, vidx], scale, None if bias is None else bias[:, :, kidx])["o"]


def reordered(ref_in, dtype):
    """A legal evaluation: fp32 throughout, the key axis summed in reverse order; for the bf16
    kernels P and the output rounded to bf16 as they do."""
    q, k, v, scale, bias = ref_in
    f = np.float32
    y = np.matmul(q.astype(f)[..., ::-1].copy(), k.astype(f)[..., ::-1].copy().transpose(0, 2, 1))
    y = (y * f(scale)).astype(f)
    if bias is not None:
        y = (y + bias.astype(f)).astype(f)
    e = np.exp((y - y.max(-1, keepdims=True)).astype(f)).astype(f)[..., ::-1].copy()
    l = e.sum(-1, keepdims=True, dtype=f)
    pn = e if dtype == "f32" else bf16_round(e).astype(f)
    o = (np.matmul(pn, v.astype(f)[:, ::-1].copy()) / l).astype(f)
    return (bf16_round(o) if dtype == "bf16" else o).astype(np.float64)


# ---- token attention (evt_attention, evt_attention_hd, evt_attention_mx8) ------------------------
def scale_of(hd):
    """The fp32 scale the entry points are handed (hd^-0.5; exactly 0.125 at 64)."""
    return float(np.float32(hd ** -0.5))


@functools.lru_cache(maxsize=None)
def token_case(probe, n, hd):
    """The probe and its hostile neighbour: rows [2][n, 3 H hd] (index 0 the probe image), the
    reference inputs and `core` results of both, pi. Shared by every test; arrays are read-only."""
    q, k, v, pi = _probe_qkv(probe, n, hd, seed=7 * n + hd)
    hq, hk, hv = _hostile_qkv(q, n, hd)
    scale = scale_of(hd)
    ins = [(q, k, v, scale, None), (hq, hk, hv, scale, None)]
    refs = [core(*x) for x in ins]
    rows = [to_rows(q, k, v), to_rows(hq, hk, hv)]
    for a in rows + [q, k, v, hq, hk, hv] + [r[key] for r in refs for key in ("o", "p", "y", "yqk")]:
        a.setflags(write=False)
    return dict(rows=rows, ins=ins, refs=refs, pi=pi)


def rows_of(o, n):
    """[H, n, hd] -> output rows [n, H hd]."""
    return o.transpose(1, 0, 2).reshape(n, -1)


# ---- window attention (evt_window_attention: window 7, head size 32) -----------------------------
def window_index(R, shift, w=7):
    """[nW, w w]: the raster row of each window token (with the cyclic shift)."""
    idx = np.arange(R * R).reshape(R, R)
    if shift:
        idx = np.roll(idx, (-shift, -shift), axis=(0, 1))
    nw = R // w
    return idx.reshape(nw, w, nw, w).transpose(0, 2, 1, 3).reshape(nw * nw, w * w)


@functools.lru_cache(maxsize=None)
def window_case(probe, R, shift):
    """As token_case for one R x R image: rows [2][R R, 3 C], the relative-position table
    [169, H] (zero for the uniform probe, integers in -2 .. 2 otherwise), grouped reference inputs
    (G = windows x heads) with the bias and mask of the oracle, `core` results, and the same
    inputs without the shift mask (the 'mask ignored' mutation)."""
    hd, w, T = 32, 7, R * R
    rng = np.random.default_rng(100 * R + shift)
    win = window_index(R, shift)                                     # [nW, 49]
    nW = win.shape[0]
    mask = swin_ref.shift_mask(R, R, w, shift) if shift else np.zeros((nW, 49, 49))
    label = np.argmax(mask == 0, axis=-1)                            # [nW, 49] region of a token
    rpb = np.zeros((169, H)) if probe == "uniform" else rng.integers(-2, 3, (169, H)).astype(float)
    if probe == "uniform":
        q = np.zeros((H, T, hd))
        k = rng.integers(-3, 4, (H, T, hd)).astype(np.float64)
        v = rng.integers(0, 2, (H, T, hd)) * 2.0 - 1.0
    else:
        c = codes(T, hd)
        q = np.broadcast_to(S_PERM * c, (H, T, hd)).copy()
        k = np.zeros((H, T, hd))
        for h in range(H):
            for wi in range(nW):
                for lab in np.unique(label[wi]):
                    members = win[wi][label[wi] == lab]              # raster rows of one group
                    k[h, members[derangement(len(members), rng)]] = S_PERM * c[members]
        v = rng.choice([-2.0, -1.0, 1.0, 2.0], (H, T, hd))
    hq, hk, hv = _hostile_qkv(q, T, hd)
    bias = rpb[swin_ref.relative_position_index(w).reshape(-1)].reshape(49, 49, H).transpose(2, 0, 1)

    def grouped(x):                                                  # [H, T, hd] -> [nW H, 49, hd]
        return x[:, win].transpose(1, 0, 2, 3).reshape(nW * H, 49, hd)

    gb = (bias[None] + mask[:, None]).reshape(nW * H, 49, 49)
    gb0 = np.broadcast_to(bias[None], (nW, H, 49, 49)).reshape(nW * H, 49, 49)
    scale = hd ** -0.5
    ins = [(grouped(q), grouped(k), grouped(v), scale, gb),
           (grouped(hq), grouped(hk), grouped(hv), scale, gb)]
    refs = [core(*x) for x in ins]
    unmasked = (grouped(q), grouped(k), grouped(v), scale, gb0)
    return dict(rows=[to_rows(q, k, v), to_rows(hq, hk, hv)], rpb=rpb, ins=ins, refs=refs,
                unmasked=unmasked, win=win, nW=nW)


def window_rows(o, win, T):
    """grouped output [nW H, 49, hd] -> raster rows [T, H hd]."""
    nW = win.shape[0]
    o = o.reshape(nW, H, 49, -1)
    out = np.zeros((T, H * o.shape[-1]))
    for h in range(H):
        out[win.reshape(-1), h * o.shape[-1]:(h + 1) * o.shape[-1]] = o[:, h].reshape(nW * 49, -1)
    return out
