"""Attention rollout of the model mirrors: the binding of include/evt_rollout.h.

    out = model.attention_rollout(img)                    # {"rollout": [B, T]}, the CLS row
    sal = out["rollout"][:, 1:].reshape(B, grid, grid)    # the usual saliency map
    out = model.attention_rollout(img, queries="all", start=4, logits=True)   # [B, T, T]
    model.attention_rollout_into(img, out=t, queries="cls")
    model.rollout_shape()                                 # (tokens, blocks)

Attention rollout (Abnar & Zuidema, 2020) with mean head fusion and residual weight 0.5: with
p_l[b, h] the softmax probabilities of encoder block l (the values `attention_maps` exports),

    Abar_l = mean_h p_l[b, h]      Ahat_l = 0.5 (Abar_l + I)      R_l = Ahat_l @ R_{l-1},  R_{start-1} = I

and the result is R_{depth-1}, indexed [image, query, source token]; `queries="cls"` is bitwise
`queries="all"`[:, 0]. Everything is fp32 on the device whatever the model's dtype, no per-head
map is stored, and it comes from the same forward that produces the logits, so `logits=True` /
`pooled=True` return bitwise what `model(img)` / `forward_features(img)` return. Rows are
non-negative and sum to 1. ViT (reference and standard, pruned or not) and T2T_ViT have it; Swin
(its windows do not compose this way: `window_attention_maps` gives the per-window maps) and "mx8"
models raise ValueError.

The scratch the C ABI asks of its caller (up to three [B, T, T] fp32 buffers) is allocated here once
per (batch, queries) and kept on the model object; it goes with the model.

`rollout_reference` is the same contract in numpy fp64, from per-block probability arrays.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from ... import _lib
from .features import resolve_taps
from .head_stats import HeadStats

MODES = {"cls": _lib.ROLLOUT_CLS, "all": _lib.ROLLOUT_ALL}


def resolve_mode(queries) -> int:
    """EVT_ROLLOUT_CLS / EVT_ROLLOUT_ALL of a `queries=` argument ("cls" / "all" or the constant)."""
    if isinstance(queries, str) and queries in MODES:
        return MODES[queries]
    if not isinstance(queries, (str, bool)) and queries in (_lib.ROLLOUT_CLS, _lib.ROLLOUT_ALL):
        return int(queries)
    raise ValueError(f"queries must be 'cls' or 'all', got {queries!r}")


def rollout_reference(maps: Sequence, start: int = 0) -> np.ndarray:
    """The contract of include/evt_rollout.h in numpy fp64: [..., T, T] (indexed [query, source])
    from `maps`, one probability array [..., H_l, T, T] per encoder block (H_l may differ), over
    blocks start .. len(maps) - 1 (negative `start`: from the last)."""
    maps = list(maps)
    if not maps:
        raise ValueError("rollout_reference needs at least one block's maps")
    start = resolve_taps((start,), len(maps))[0]
    r = None
    for a in maps[start:]:
        p = np.asarray(a, dtype=np.float64)
        if p.ndim < 3 or p.shape[-1] != p.shape[-2]:
            raise ValueError(f"maps must be [..., H, T, T], got {p.shape}")
        t = p.shape[-1]
        if r is not None and r.shape[-1] != t:
            raise ValueError("every block must have the same number of tokens")
        ahat = 0.5 * (p.mean(axis=-3) + np.eye(t))
        r = ahat if r is None else ahat @ r
    return r


class AttentionRollout(HeadStats):
    """What ViT, T2T_ViT and SwinTransformer derive from (through Classification): attention
    rollout on top of the head statistics and attention maps. The blocks are those of
    `_attn_geometry()`; Swin and "mx8" raise."""

    def _rollout_blocks(self):
        if getattr(self, "dtype", None) == "mx8":
            raise ValueError("attention rollout is not available on an 'mx8' model")
        try:
            return self._attn_geometry()
        except ValueError as e:
            raise ValueError(f"{type(self).__name__} has no attention rollout: its windowed "
                             "attention does not compose across blocks this way "
                             "(window_attention_maps gives the per-window maps)") from e

    def rollout_shape(self) -> Tuple[int, int]:
        """(tokens per image, encoder blocks). Host only."""
        geo = self._rollout_blocks()
        return geo[0][1], len(geo)

    def _rollout_scratch(self, b: int, mode: int) -> torch.Tensor:
        """The call's scratch: allocated once per (batch, mode), kept on the model."""
        cache = self.__dict__.setdefault("_rollout_scratch_cache", {})
        t = cache.get((b, mode))
        if t is None:
            n = ctypes.c_size_t()
            _lib.check(_lib.load_library().evt_rollout_scratch_bytes(self._ptr(), b, mode,
                                                                     ctypes.byref(n)))
            t = cache[(b, mode)] = torch.empty(n.value, dtype=torch.uint8, device=self.device)
        return t

    def attention_rollout_into(self, img, *, out: torch.Tensor, queries="cls", start: int = 0,
                               logits: torch.Tensor = None, pooled: torch.Tensor = None) -> None:
        """Enqueue one forward of a device-resident batch (fp32 in the model's layout, or a
        `Uint8Images`) that fills `out` ([B, T] for queries="cls", [B, T, T] for "all") with the
        rollout over blocks start .. depth - 1 and the given `logits` [B, num_classes] / `pooled`
        [B, F] tensors; no synchronisation, and no allocation after the first call of a (batch,
        queries) (evt_forward_rollout)."""
        t, depth = self.rollout_shape()
        mode = resolve_mode(queries)
        a = _lib.evt_rollout_args()
        a.start, a.mode = resolve_taps((start,), depth)[0], mode
        b = img.shape[0]
        if out is None:
            raise ValueError("out must be a tensor")
        a.out = self._feature_tensor("out", out, (b, t, t) if mode == _lib.ROLLOUT_ALL else (b, t))
        feat = self._feat_args(b, logits=logits, pooled=pooled)
        self._fit(img)  # the handle sizes the scratch
        with torch.cuda.device(self.device):
            scratch = self._rollout_scratch(b, mode)
        a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
        self._analysis_forward("evt_forward_rollout", img, feat, a)

    def attention_rollout(self, img, queries="cls", start: int = 0, logits: bool = False,
                          pooled: bool = False) -> Dict[str, object]:
        """{"rollout": [B, T] or [B, T, T]} plus the requested "logits" / "pooled". numpy in, numpy
        out; a device tensor (or a device `Uint8Images`) gives device tensors."""
        t, depth = self.rollout_shape()
        mode = resolve_mode(queries)
        start = resolve_taps((start,), depth)[0]
        out = self._block_outputs(  # a list of one: the rollout
            img, "rollout", (0,), lambda b, _: (b, t, t) if mode == _lib.ROLLOUT_ALL else (b, t),
            lambda x, r, **kw: self.attention_rollout_into(x, out=r[0], queries=mode, start=start,
                                                           **kw),
            logits=logits, pooled=pooled)
        out["rollout"] = out["rollout"][0]
        return out
