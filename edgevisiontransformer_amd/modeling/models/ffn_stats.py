"""Per-neuron FFN activation statistics of the model mirrors: the binding of
include/evt_ffn_stats.h.

    out = model.ffn_stats(img)                  # every block
    out["stats"]                                # list of [B, F_i, 4], FFN_STATS order
    out = model.ffn_stats(img, blocks=(-1, 0), logits=True)
    model.ffn_stats_into(img, blocks=(3, 11), stat_tensors=(a, b))
    model.ffn_stats_shape(-1)                   # (neurons, tokens) of a block

Four numbers per (image, FFN neuron), fp32 whatever the model's dtype, reduced on the device from
the hidden activations a[b, t, j] FC1 stores for FC2 (the GELU output, rounded to the model's
dtype), over the T tokens of the image, without exporting the [B T, F] matrix:

    mean      sum_t a / T
    mean_abs  sum_t |a| / T
    mean_sq   sum_t a^2 / T     (times ||fc2_w[j, :]||^2: the neuron's output energy)
    max_abs   max_t |a|         (exact: one of the stored values)

They come from the same forward that produces the logits (one more kernel per requested block,
between FC1 and FC2), so `logits=True` / `pooled=True` return bitwise what `model(img)` /
`forward_features(img)` return. ViT (reference and standard, pruned or not) and T2T_ViT have them;
Swin (its fused MLP never stores the hidden rows) and "mx8" models (theirs are kept quantised)
raise ValueError.

`ffn_stats_reference` is the same contract in numpy fp64, from a hidden matrix.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ... import _lib
from .features import resolve_taps
from .rollout import AttentionRollout

FFN_STATS = ("mean", "mean_abs", "mean_sq", "max_abs")


def ffn_stats_reference(hidden) -> np.ndarray:
    """The contract of include/evt_ffn_stats.h in numpy fp64: hidden activations [..., T, F] ->
    [..., F, 4] in FFN_STATS order, reduced over the T axis."""
    a = np.asarray(hidden, dtype=np.float64)
    if a.ndim < 2 or a.shape[-2] < 1:
        raise ValueError(f"hidden must be [..., T >= 1, F], got {a.shape}")
    mag = np.abs(a)
    return np.stack([a.mean(-2), mag.mean(-2), (a * a).mean(-2), mag.max(-2)], axis=-1)


class FFNStats(AttentionRollout):
    """What ViT, T2T_ViT and SwinTransformer derive from (through Classification): the FFN neuron
    statistics on top of the attention outputs. The model class provides `_ffn_geometry()` ->
    [(neurons, tokens) per encoder block], or leaves the default, which raises (Swin)."""

    def _ffn_geometry(self) -> List[Tuple[int, int]]:
        raise ValueError(f"{type(self).__name__} has no FFN statistics: its fused MLP does not "
                         "store the hidden activations")

    def _ffn_blocks(self) -> List[Tuple[int, int]]:
        if getattr(self, "dtype", None) == "mx8":
            raise ValueError("FFN statistics are not available on an 'mx8' model: its hidden "
                             "activations are kept quantised")
        return self._ffn_geometry()

    def ffn_stats_shape(self, block: int) -> Tuple[int, int]:
        """(FFN neurons, tokens per image) of `block` (negative: from the last). Host only."""
        geo = self._ffn_blocks()
        return geo[resolve_taps((block,), len(geo))[0]]

    def ffn_stats_into(self, img, *, blocks: Sequence[int], stat_tensors: Sequence[torch.Tensor],
                       logits: torch.Tensor = None, pooled: torch.Tensor = None) -> None:
        """Enqueue one forward of a device-resident batch (fp32 in the model's layout, or a
        `Uint8Images`) that fills `stat_tensors[i]` [B, F, 4] with the statistics of block
        `blocks[i]` and the given `logits` [B, num_classes] / `pooled` [B, features] tensors; no
        allocation, no synchronisation (evt_forward_ffn_stats)."""
        geo = self._ffn_blocks()
        idx = resolve_taps(blocks, len(geo))
        b = img.shape[0]
        keep = self._block_list(idx, stat_tensors, lambda i: (b, geo[i][0], _lib.FFN_STATS),
                                "stat_tensors", "block")
        feat = self._feat_args(b, logits=logits, pooled=pooled)
        if not (idx or feat[1]):
            raise ValueError("no output requested")
        a = _lib.evt_ffn_stats_args()
        a.n_blocks = len(idx)
        if idx:
            a.blocks, a.stats = keep
        self._analysis_forward("evt_forward_ffn_stats", img, feat, a)

    def ffn_stats(self, img, blocks: Optional[Sequence[int]] = None, logits: bool = False,
                  pooled: bool = False) -> Dict[str, object]:
        """{"stats": [one [B, F_i, 4] per block, in the order given]} plus the requested "logits" /
        "pooled"; `blocks=None`: every block. numpy in, numpy out; a device tensor (or a device
        `Uint8Images`) gives device tensors."""
        geo = self._ffn_blocks()
        idx = resolve_taps(range(len(geo)) if blocks is None else blocks, len(geo))
        return self._block_outputs(
            img, "stats", idx, lambda b, i: (b, geo[i][0], _lib.FFN_STATS),
            lambda x, t, **kw: self.ffn_stats_into(x, blocks=idx, stat_tensors=t, **kw),
            logits=logits, pooled=pooled)
