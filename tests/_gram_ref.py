"""Inputs, fp64 references and the error bound of the activation-Gram tests (include/evt_gram.h).

Pure numpy; no GPU. tests/test_gram_host.py checks this module on the CPU, tests/test_gpu_gram.py
runs the cases on the kernels (gram_kernel / gram_reduce_kernel, csrc/gram.hip).

Shapes. The kernel as built has 128-wide tiles (both dtypes), stages rows in pieces of 64 (bf16) or
32 (fp32) and, for the narrow matrices here (fewer than 256 tiles), splits the rows into chunks of
a multiple of 64 rows once the matrix has 512 of them (csrc/evt_internal.h gram_plan):

    WIDTHS  8, 120 / 128 / 136 (one tile, at and above its edge), 256 / 264 (two and three tiles,
            off-diagonal tiles), 776 (seven tiles: 28 workgroups per chunk)
    ROWS    1, 2, 31 / 32 / 33 and 63 / 64 / 65 (the fp32 and bf16 piece), 197, 511 / 512 / 513
            (one chunk, two chunks of 256, 320 + 193), 788 (three chunks)

each with ld = F and ld = F + 24, the padding columns NaN.

Bound. An fp32 sum of R terms in any order is within R 2^-24 sum |terms| of the exact sum (first
order); the gate is 8 times that, per element, against the fp64 result of the stored (rounded)
values. Products of bf16 values are exact in fp32; an fp32 product is rounded once, inside the fused
multiply-add, which the same bound covers.
"""
import math

import numpy as np

from oracle import vit_ref

TILE = 128
PIECE = {"bf16": 64, "f32": 32}
WIDTHS = (8, 120, 128, 136, 256, 264, 776)
ROWS = (1, 2, 31, 32, 33, 63, 64, 65, 197, 511, 512, 513, 788)
BIG = (16 * 197, 3072)
PAD_COLS = 24
MARGIN = 8.0


def round_to(values, dtype):
    """float32 values rounded to the storage dtype ("bf16": round to nearest even), as float32."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    if dtype == "f32":
        return v
    u = v.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def normal(rows, width, dtype, seed):
    """A random matrix with a nonzero mean and columns of different scales, rounded to dtype."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((rows, width)) * (0.25 + rng.random(width)) + 0.3
    return round_to(a, dtype)


def reference(a):
    """fp64 Gram, column sums and the per-element gates of the stored values a [R, F]."""
    x = np.asarray(a, dtype=np.float64)
    mag = np.abs(x)
    scale = MARGIN * x.shape[0] * 2.0 ** -24
    return {"gram": x.T @ x, "sum": x.sum(0), "gram_gate": scale * (mag.T @ mag),
            "sum_gate": scale * mag.sum(0)}


def edge_columns(width):
    """Every column next to a tile edge, and the first and last one."""
    cols = {0, width - 1}
    for e in range(TILE, width + 1, TILE):
        cols.update(c for c in (e - 1, e, e + 1) if 0 <= c < width)
    return sorted(cols)


def probe_single(rows, width):
    """Row r has one nonzero, (-1)^r (1 + r % 2) at column r % width: a diagonal integer Gram."""
    a = np.zeros((rows, width), dtype=np.float32)
    r = np.arange(rows)
    a[r, r % width] = np.where(r % 2, -2.0, 1.0)
    return a


def probe_pairs(width, repeat=3):
    """Rows with two nonzeros (1 at column i, 2 at column j, i < j; or a single 2 when i == j) that
    walk every pair of edge columns, hence every tile pair, `repeat` times."""
    cols = edge_columns(width)
    pairs = [(i, j) for i in cols for j in cols if i <= j]
    a = np.zeros((len(pairs) * repeat, width), dtype=np.float32)
    for r in range(a.shape[0]):
        i, j = pairs[r % len(pairs)]
        a[r, i] = 1.0
        a[r, j] = 2.0
    return a


def probe_dense(rows, width, seed):
    """Dense small integers in [-2, 2]: every partial sum stays below 2^24, so any order is exact."""
    assert 4 * rows < 2 ** 24
    return np.random.default_rng(seed).integers(-2, 3, (rows, width)).astype(np.float32)


def exact(a):
    """The integer Gram and sums of an integer-valued matrix, as the float32 they must be."""
    x = np.asarray(a, dtype=np.float64)  # integers far below 2^53: the fp64 products and sums are exact
    assert np.array_equal(x, np.rint(x))
    g, s = x.T @ x, x.sum(0)
    assert np.abs(g).max() < 2 ** 24 and np.abs(s).max() < 2 ** 24
    return g.astype(np.float32), s.astype(np.float32)


# ---- model level: the rows the Grams are formed of, from the fp64 forwards ----------------------
def _context(y, qkv_w, qkv_b, heads, hk):
    b, n, _ = y.shape
    qkv = y @ qkv_w + (0.0 if qkv_b is None else qkv_b)
    qkv = qkv.reshape(b, n, 3, heads, hk).transpose(2, 0, 3, 1, 4)
    att = vit_ref.softmax(np.einsum("bhid,bhjd->bhij", qkv[0], qkv[1]) * hk ** -0.5)
    return np.einsum("bhij,bhjd->bhid", att, qkv[2]).transpose(0, 2, 1, 3).reshape(b, n, heads * hk)


def vit_rows(params, cfg, img):
    """(FC1 outputs [B, T, F_i], attention contexts [B, T, heads_i * head_dim_i], logits) of every
    block of the reference-semantics forward (oracle/vit_ref.py vit_forward and its trace)."""
    trace = {}
    logits = vit_ref.vit_forward(params, cfg, img, trace=trace)
    P = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    hidden = [vit_ref.gelu(trace[f"l{i}.ln2"] @ P[f"l{i}.fc1_w"] + P[f"l{i}.fc1_b"])
              for i in range(cfg.depth)]
    ctx = [_context(trace[f"l{i}.ln1"], P[f"l{i}.qkv_w"], None, cfg.heads[i], cfg.head_dim[i])
           for i in range(cfg.depth)]
    return hidden, ctx, logits


def t2t_rows(params, cfg, img):
    """(FC1 outputs, attention contexts) of every backbone block of the fp64 T2T-ViT forward (its
    encoder blocks are vit_ref's: no QKV bias, head size dim // heads)."""
    from oracle import t2t_ref
    trace = {}
    t2t_ref.t2t_vit_forward(params, cfg, img, trace=trace)
    P = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    hidden = [vit_ref.gelu(trace[f"l{i}.ln2"] @ P[f"l{i}.fc1_w"] + P[f"l{i}.fc1_b"])
              for i in range(cfg.depth)]
    ctx = [_context(trace[f"l{i}.ln1"], P[f"l{i}.qkv_w"], None, cfg.heads, cfg.dim // cfg.heads)
           for i in range(cfg.depth)]
    return hidden, ctx


def std_vit_rows(params, cfg, img, eps=1e-6, dtype=np.float64):
    """(FC1 outputs, attention contexts, logits) of the STANDARD forward: std_vit_hidden of
    tests/test_gpu_ffn_stats.py (x + attn(LN1 x), x + mlp(LN2 x), QKV bias, erf GELU, eps 1e-6,
    final LayerNorm) that also keeps the attention context."""
    P = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}
    x = vit_ref.patchify_nchw(np.asarray(img, dtype=dtype), cfg.patch_size) @ P["patch_w"] + P["patch_b"]
    b = x.shape[0]
    x = np.concatenate([np.broadcast_to(P["cls"], (b, 1, cfg.dim)), x], axis=1) + P["pos"]
    erf = np.vectorize(math.erf, otypes=[np.float64])
    hidden, ctx = [], []
    for i in range(cfg.depth):
        y = vit_ref.layer_norm(x, P[f"l{i}.ln1_g"], P[f"l{i}.ln1_b"], eps)
        o = _context(y, P[f"l{i}.qkv_w"], P[f"l{i}.qkv_b"], cfg.heads[i], cfg.head_dim[i])
        ctx.append(o)
        x = x + o @ P[f"l{i}.out_w"] + P[f"l{i}.out_b"]
        y = vit_ref.layer_norm(x, P[f"l{i}.ln2_g"], P[f"l{i}.ln2_b"], eps)
        z = y @ P[f"l{i}.fc1_w"] + P[f"l{i}.fc1_b"]
        z = 0.5 * z * (1.0 + erf(z / math.sqrt(2.0)))
        hidden.append(z)
        x = x + z @ P[f"l{i}.fc2_w"] + P[f"l{i}.fc2_b"]
    x = vit_ref.layer_norm(x[:, 0], P["norm_g"], P["norm_b"], eps)
    return hidden, ctx, x @ P["head_w"] + P["head_b"]
