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

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ... import _lib
from ...images import Uint8Images
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
        if len(stat_tensors) != len(idx):
            raise ValueError("stat_tensors needs one tensor per block")
        b = img.shape[0]
        order = sorted(range(len(idx)), key=idx.__getitem__)  # the C ABI wants them rising
        ptrs = [self._feature_tensor(f"stat_tensors[{i}]", stat_tensors[i],
                                     (b, geo[idx[i]][0], _lib.FFN_STATS)) for i in order]
        feat = _lib.evt_features_args()
        feat.logits = self._feature_tensor("logits", logits, (b, self.num_classes))
        feat.pooled = self._feature_tensor("pooled", pooled, (b, self.feature_dim))
        if not (idx or feat.logits or feat.pooled):
            raise ValueError("no output requested")
        a = _lib.evt_ffn_stats_args()
        a.n_blocks = len(idx)
        keep = ((ctypes.c_int32 * max(1, len(idx)))(*[idx[i] for i in order]),
                (ctypes.c_void_p * max(1, len(idx)))(*ptrs))
        if idx:
            a.blocks, a.stats = keep
        if isinstance(img, Uint8Images):
            args = img.image_args()
        else:
            args = _lib.evt_image_args()
            args.data, args.format = img.data_ptr(), 0  # EVT_IMG_F32
        self._fit(img)
        _lib.check(_lib.load_library().evt_forward_ffn_stats(
            self._ptr(), ctypes.byref(args), b,
            ctypes.byref(feat) if (feat.logits or feat.pooled) else None, ctypes.byref(a),
            self._stream()))

    def ffn_stats(self, img, blocks: Optional[Sequence[int]] = None, logits: bool = False,
                  pooled: bool = False) -> Dict[str, object]:
        """{"stats": [one [B, F_i, 4] per block, in the order given]} plus the requested "logits" /
        "pooled"; `blocks=None`: every block. numpy in, numpy out; a device tensor (or a device
        `Uint8Images`) gives device tensors."""
        geo = self._ffn_blocks()
        idx = resolve_taps(range(len(geo)) if blocks is None else blocks, len(geo))
        x, was_numpy = self._checked_image(img)
        b = x.shape[0]
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)  # noqa: E731
        out: Dict[str, object] = {"stats": [new(b, geo[i][0], _lib.FFN_STATS) for i in idx]}
        if logits:
            out["logits"] = new(b, self.num_classes)
        if pooled:
            out["pooled"] = new(b, self.feature_dim)
        with torch.cuda.device(self.device):
            self.ffn_stats_into(x, blocks=idx, stat_tensors=out["stats"],
                                logits=out.get("logits"), pooled=out.get("pooled"))
        if was_numpy:  # .cpu() waits for the stream, as __call__ does
            out = {k: [v.cpu().numpy() for v in val] if isinstance(val, list) else val.cpu().numpy()
                   for k, val in out.items()}
        return out
