"""The fp64 teacher-forced reference of the token-pruning tests (include/evt_token_pruning.h).

It is the oracle's forward (`oracle.vit_ref`: its layer_norm, softmax, gelu, patchify and
feed_forward, reference and standard semantics) with one change: after each scheduled block it
records its OWN score (the head sum of the CLS row of its own softmax) and then keeps the rows the
DEVICE's `kept` table names. Near-ties in the score therefore cannot flip a test, and correctness
splits into three independent claims: the scores are close to the reference's, the selection is
exact given the scores, and the forward is close to the reference given the selection.
"""
import math

import numpy as np

from oracle import vit_ref


def _attention(y, qkv_w, qkv_b, heads, hk):
    """(probabilities [B, h, N, N], attention output [B, N, h hk]) of LayerNorm'd rows y."""
    b, n, _ = y.shape
    qkv = y @ qkv_w
    if qkv_b is not None:
        qkv = qkv + qkv_b
    qkv = qkv.reshape(b, n, 3, heads, hk).transpose(2, 0, 3, 1, 4)
    p = vit_ref.softmax(np.einsum("bhid,bhjd->bhij", qkv[0], qkv[1]) * hk ** -0.5)
    o = np.einsum("bhij,bhjd->bhid", p, qkv[2]).transpose(0, 2, 1, 3).reshape(b, n, heads * hk)
    return p, o


def forward(params, cfg, img, schedule, kept, standard=False, eps=1e-6):
    """(logits [B, classes], scores: one [B, T_l] per scheduled block) in fp64. schedule:
    [(block, K, T_in, T_out)]; kept: the device's tables, one int array [B, 1 + K] per entry."""
    P = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    x = vit_ref.patchify_nchw(np.asarray(img, dtype=np.float64), cfg.patch_size)
    x = x @ P["patch_w"] + P["patch_b"]
    b = x.shape[0]
    x = np.concatenate([np.broadcast_to(P["cls"].reshape(1, 1, -1), (b, 1, cfg.dim)), x], 1) + P["pos"]
    at = {blk: (i, k) for i, (blk, k, _, _) in enumerate(schedule)}
    scores = []
    for i in range(cfg.depth):
        h, hk = cfg.heads[i], cfg.head_dim[i]
        if standard:
            y = vit_ref.layer_norm(x, P[f"l{i}.ln1_g"], P[f"l{i}.ln1_b"], eps)
            p, o = _attention(y, P[f"l{i}.qkv_w"], P[f"l{i}.qkv_b"], h, hk)
            x = x + o @ P[f"l{i}.out_w"] + P[f"l{i}.out_b"]
            y = vit_ref.layer_norm(x, P[f"l{i}.ln2_g"], P[f"l{i}.ln2_b"], eps)
            from scipy.special import erf
            z = y @ P[f"l{i}.fc1_w"] + P[f"l{i}.fc1_b"]
            z = 0.5 * z * (1.0 + erf(z / math.sqrt(2.0)))
            x = x + z @ P[f"l{i}.fc2_w"] + P[f"l{i}.fc2_b"]
        else:
            y = vit_ref.layer_norm(x, P[f"l{i}.ln1_g"], P[f"l{i}.ln1_b"])
            p, o = _attention(y, P[f"l{i}.qkv_w"], None, h, hk)
            x = o @ P[f"l{i}.out_w"] + P[f"l{i}.out_b"] + y
            y = vit_ref.layer_norm(x, P[f"l{i}.ln2_g"], P[f"l{i}.ln2_b"])
            x = vit_ref.feed_forward(y, P[f"l{i}.fc1_w"], P[f"l{i}.fc1_b"], P[f"l{i}.fc2_w"],
                                     P[f"l{i}.fc2_b"]) + y
        if i in at:
            e, k = at[i]
            scores.append(p[:, :, 0, :].sum(1))
            idx = np.asarray(kept[e], dtype=np.int64)
            assert idx.shape == (b, k + 1)
            x = np.take_along_axis(x, idx[:, :, None], axis=1)
    if standard:
        t = vit_ref.layer_norm(x[:, 0], P["norm_g"], P["norm_b"], eps)
        return t @ P["head_w"] + P["head_b"], scores
    t = vit_ref.gelu(x[:, 0] @ P["head1_w"] + P["head1_b"])
    return t @ P["head2_w"] + P["head2_b"], scores
