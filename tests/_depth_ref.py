"""The fp64 reference of the depth tests (include/evt_depth.h): the oracle's forward
(`oracle.vit_ref`: its layer_norm, softmax, gelu, patchify and feed_forward, reference and standard
semantics) with a skip mask, keeping every sublayer's input and output rows.

A skipped sublayer is absent: the stream passes through, its LayerNorm included. `forward` returns
the logits and, per block, the pair (attention sublayer, FFN sublayer) of (input, output) streams
[B, T, D]; a skipped sublayer's pair is (x, x).
"""
import math

import numpy as np

from oracle import vit_ref
from tests._token_pruning_ref import _attention

SKIP_ATTN, SKIP_FFN = 1, 2


def forward(params, cfg, img, mask=None, standard=False, eps=1e-6):
    P = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    mask = [0] * cfg.depth if mask is None else list(mask)
    x = vit_ref.patchify_nchw(np.asarray(img, dtype=np.float64), cfg.patch_size)
    x = x @ P["patch_w"] + P["patch_b"]
    b = x.shape[0]
    x = np.concatenate([np.broadcast_to(P["cls"].reshape(1, 1, -1), (b, 1, cfg.dim)), x], 1) + P["pos"]
    streams = []
    for i in range(cfg.depth):
        h, hk = cfg.heads[i], cfg.head_dim[i]
        x_in = x
        if not mask[i] & SKIP_ATTN:
            if standard:
                y = vit_ref.layer_norm(x, P[f"l{i}.ln1_g"], P[f"l{i}.ln1_b"], eps)
                _, o = _attention(y, P[f"l{i}.qkv_w"], P[f"l{i}.qkv_b"], h, hk)
                x = x + o @ P[f"l{i}.out_w"] + P[f"l{i}.out_b"]
            else:
                y = vit_ref.layer_norm(x, P[f"l{i}.ln1_g"], P[f"l{i}.ln1_b"])
                _, o = _attention(y, P[f"l{i}.qkv_w"], None, h, hk)
                x = o @ P[f"l{i}.out_w"] + P[f"l{i}.out_b"] + y
        xm = x
        if not mask[i] & SKIP_FFN:
            if standard:
                from scipy.special import erf
                y = vit_ref.layer_norm(x, P[f"l{i}.ln2_g"], P[f"l{i}.ln2_b"], eps)
                z = y @ P[f"l{i}.fc1_w"] + P[f"l{i}.fc1_b"]
                z = 0.5 * z * (1.0 + erf(z / math.sqrt(2.0)))
                x = x + z @ P[f"l{i}.fc2_w"] + P[f"l{i}.fc2_b"]
            else:
                y = vit_ref.layer_norm(x, P[f"l{i}.ln2_g"], P[f"l{i}.ln2_b"])
                x = vit_ref.feed_forward(y, P[f"l{i}.fc1_w"], P[f"l{i}.fc1_b"], P[f"l{i}.fc2_w"],
                                         P[f"l{i}.fc2_b"]) + y
        streams.append(((x_in, xm), (xm, x)))
    if standard:
        t = vit_ref.layer_norm(x[:, 0], P["norm_g"], P["norm_b"], eps)
        return t @ P["head_w"] + P["head_b"], streams
    t = vit_ref.gelu(x[:, 0] @ P["head1_w"] + P["head1_b"])
    return t @ P["head2_w"] + P["head2_b"], streams
