"""Per-head attention statistics of the model mirrors: the binding of include/evt_head_stats.h.

    out = model.head_stats(img)                 # every block
    out["stats"]                                # list of [B, H_i, 4], HEAD_STATS order
    out = model.head_stats(img, blocks=(-1, 0), logits=True)
    model.head_stats_into(img, blocks=(3, 11), stat_tensors=(a, b))
    model.head_stats_shape(-1)                  # (heads, tokens, prefix, grid_w) of a block

Four numbers per (image, head), fp32 whatever the model's dtype, reduced on the device from the
softmax probabilities p[b, h, i, j] of the chosen encoder blocks (the values `attention_maps`
exports), without storing a map:

    confidence  mean over the T queries of max_j p_ij (Voita et al.: a forward-only pruning score)
    entropy     mean over the T queries of -sum_j p_ij ln p_ij, in nats
    distance    mean over the patch queries of sum_{patch j} p_ij d(i, j), d the Euclidean distance
                of the two patches in patch units (not renormalised over the patch keys)
    cls_mass    mean over the patch queries of the probability they give the CLS token

They come from the same forward that produces the logits (one more kernel per requested block),
so `logits=True` / `pooled=True` return bitwise what `model(img)` / `forward_features(img)`
return. ViT (reference and standard, pruned or not) and T2T_ViT have them; Swin and "mx8" models
raise ValueError, as for `attention_maps`.

`head_stats_reference` is the same contract in numpy fp64, from probabilities or from q and k.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ... import _lib
from .features import resolve_taps
from .window_attention_maps import WindowAttentionMaps

HEAD_STATS = ("confidence", "entropy", "distance", "cls_mass")


def patch_distances(n_patches: int, grid_w: int) -> np.ndarray:
    """[n, n] fp64 Euclidean distances of the cells of a row-major grid of `grid_w` columns."""
    if grid_w < 1 or n_patches < 0 or n_patches % grid_w:
        raise ValueError(f"{n_patches} patches are not a grid of {grid_w} columns")
    r = np.arange(n_patches)
    y, x = (r // grid_w).astype(np.float64), (r % grid_w).astype(np.float64)
    return np.sqrt((y[:, None] - y[None, :]) ** 2 + (x[:, None] - x[None, :]) ** 2)


def head_stats_reference(p_or_qk, *, prefix: int = 1, grid_w: Optional[int] = None,
                         scale: Optional[float] = None) -> np.ndarray:
    """The contract of include/evt_head_stats.h in numpy fp64: [..., 4] in HEAD_STATS order, from
    a probability array [..., T, T] (indexed [query, key]) or from a pair (q, k) of [..., T, d]
    arrays (scale: d^-0.5 unless given). `grid_w`: columns of the patch grid behind tokens
    prefix .. T - 1 (default: a square grid)."""
    if isinstance(p_or_qk, (tuple, list)):
        q, k = (np.asarray(a, dtype=np.float64) for a in p_or_qk)
        s = np.einsum("...id,...jd->...ij", q, k) * (q.shape[-1] ** -0.5 if scale is None else scale)
        e = np.exp(s - s.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
    else:
        p = np.asarray(p_or_qk, dtype=np.float64)
    t = p.shape[-1]
    if p.ndim < 2 or p.shape[-2] != t:
        raise ValueError(f"probabilities must be [..., T, T], got {p.shape}")
    if not 0 <= prefix < t:
        raise ValueError(f"prefix must be in [0, {t})")
    if grid_w is None:
        grid_w = int(round((t - prefix) ** 0.5))
    d = patch_distances(t - prefix, grid_w)
    with np.errstate(divide="ignore", invalid="ignore"):
        plogp = np.where(p > 0, p * np.log(p), 0.0)
    out = np.empty(p.shape[:-2] + (4,))
    out[..., 0] = p.max(-1).mean(-1)
    out[..., 1] = -plogp.sum(-1).mean(-1)
    out[..., 2] = (p[..., prefix:, prefix:] * d).sum(-1).mean(-1)
    out[..., 3] = p[..., prefix:, :prefix].sum(-1).mean(-1)
    return out


class HeadStats(WindowAttentionMaps):
    """What ViT, T2T_ViT and SwinTransformer derive from (through Classification): the head
    statistics on top of the attention maps. The blocks are those of `_attn_geometry()` (Swin and
    "mx8" raise there); the model class provides `_patch_grid_w()`."""

    def _patch_grid_w(self) -> int:
        raise ValueError(f"{type(self).__name__} has no head statistics")

    def head_stats_shape(self, block: int) -> Tuple[int, int, int, int]:
        """(heads, tokens per image, prefix, grid_w) of `block` (negative: from the last)."""
        geo = self._attn_blocks()
        h, t = geo[resolve_taps((block,), len(geo))[0]]
        return h, t, 1, self._patch_grid_w()

    def head_stats_into(self, img, *, blocks: Sequence[int], stat_tensors: Sequence[torch.Tensor],
                        logits: torch.Tensor = None, pooled: torch.Tensor = None) -> None:
        """Enqueue one forward of a device-resident batch (fp32 in the model's layout, or a
        `Uint8Images`) that fills `stat_tensors[i]` [B, H, 4] with the statistics of block
        `blocks[i]` and the given `logits` [B, num_classes] / `pooled` [B, F] tensors; no
        allocation, no synchronisation (evt_forward_head_stats)."""
        geo = self._attn_blocks()
        idx = resolve_taps(blocks, len(geo))
        b = img.shape[0]
        keep = self._block_list(idx, stat_tensors, lambda i: (b, geo[i][0], _lib.HEAD_STATS),
                                "stat_tensors", "block")
        feat = self._feat_args(b, logits=logits, pooled=pooled)
        if not (idx or feat[1]):
            raise ValueError("no output requested")
        a = _lib.evt_head_stats_args()
        a.n_blocks = len(idx)
        if idx:
            a.blocks, a.stats = keep
        self._analysis_forward("evt_forward_head_stats", img, feat, a)

    def head_stats(self, img, blocks: Optional[Sequence[int]] = None, logits: bool = False,
                   pooled: bool = False) -> Dict[str, object]:
        """{"stats": [one [B, H_i, 4] per block, in the order given]} plus the requested "logits" /
        "pooled"; `blocks=None`: every block. numpy in, numpy out; a device tensor (or a device
        `Uint8Images`) gives device tensors."""
        geo = self._attn_blocks()
        idx = resolve_taps(range(len(geo)) if blocks is None else blocks, len(geo))
        return self._block_outputs(
            img, "stats", idx, lambda b, i: (b, geo[i][0], _lib.HEAD_STATS),
            lambda x, t, **kw: self.head_stats_into(x, blocks=idx, stat_tensors=t, **kw),
            logits=logits, pooled=pooled)
