"""fp64 numpy reference of the Swin window attention maps (include/evt_window_attention.h), built
from oracle/swin_ref.py's layer_norm, softmax, relative_position_index, shift_mask and
patch_merge; test infrastructure only.

Masked pairs (shift_mask != 0: query and key in different SW-MSA regions) are set to exactly 0 and
the row is renormalised over the rest: the scores of such pairs are -inf here where the oracle's
window_attention adds -100. The two forms differ by at most e^-100 < 1e-40 per entry.
"""
import numpy as np

from oracle import swin_ref


def window_partition(x, R, w, shift):
    """x [B, R*R, C] raster rows -> [B, nW, N, C] in the shifted frame (oracle window_attention)."""
    b, _, c = x.shape
    x = x.reshape(b, R, R, c)
    if shift:
        x = np.roll(x, (-shift, -shift), axis=(1, 2))
    nw = R // w
    return x.reshape(b, nw, w, nw, w, c).transpose(0, 1, 3, 2, 4, 5).reshape(b, nw * nw, w * w, c)


def bias_and_mask(rpb, R, w, H, shift):
    """(bias [H, N, N], masked [nW, N, N] bool) of a block."""
    n = w * w
    rpb = np.asarray(rpb, np.float64)
    bias = rpb[swin_ref.relative_position_index(w).reshape(-1)].reshape(n, n, H).transpose(2, 0, 1)
    nw = (R // w) ** 2
    masked = swin_ref.shift_mask(R, R, w, shift) != 0 if shift else np.zeros((nw, n, n), bool)
    return bias, masked


def window_probs(qkv, rpb, R, w, H, shift):
    """qkv [B*R*R, >= 3*32*H] (columns (qkv h d), head size 32; any float dtype, read as fp64), rpb
    [(2w-1)^2, H] -> fp64 [B, nW, H, N, N]."""
    c = 32 * H
    qkv = np.asarray(qkv, np.float64)[:, :3 * c]
    b = qkv.shape[0] // (R * R)
    win = window_partition(qkv.reshape(b, R * R, 3 * c), R, w, shift)
    win = win.reshape(b, -1, w * w, 3, H, 32)
    q, k = (win[..., i, :, :].transpose(0, 1, 3, 2, 4) for i in range(2))  # [B, nW, H, N, 32]
    att = np.einsum("bwhid,bwhjd->bwhij", q, k) * 32 ** -0.5
    bias, masked = bias_and_mask(rpb, R, w, H, shift)
    att = att + bias[None, None]
    att = np.where(masked[None, :, None], -np.inf, att)
    return swin_ref.softmax(att)


def model_window_probs(params, cfg, img, block, trace=None):
    """fp64 [B, nW, H, N, N] of block `block` (numbered over the stages) of the Swin model: the
    block's input from swin_forward's trace ("embed" for block 0, the previous block's output
    otherwise, through patch_merge at a stage's first block), LN1, the QKV projection, window_probs.
    `trace`: a trace of swin_forward(params, cfg, img) to reuse."""
    if trace is None:
        trace = {}
        swin_ref.swin_forward(params, cfg, img, trace=trace)
    names = [(i, j) for i in range(cfg.num_stages) for j in range(cfg.depths[i])]
    i, j = names[block]
    x = trace["embed"] if block == 0 else trace["s%d.b%d" % names[block - 1]]
    P = lambda k: np.asarray(params[k], np.float64)  # noqa: E731
    if j == 0 and i > 0:
        x = swin_ref.patch_merge(x, cfg.res(i - 1), P(f"s{i}.merge_g"), P(f"s{i}.merge_b"),
                                 P(f"s{i}.merge_w"))
    pre = f"s{i}.b{j}."
    y = swin_ref.layer_norm(x, P(pre + "ln1_g"), P(pre + "ln1_b"))
    qkv = y @ P(pre + "qkv_w") + P(pre + "qkv_b")
    return window_probs(qkv.reshape(-1, qkv.shape[-1]), P(pre + "rpb"), cfg.res(i), cfg.window(i),
                        cfg.num_heads[i], cfg.shift(i, j))
