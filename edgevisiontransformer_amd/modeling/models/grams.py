"""Activation Grams of the model mirrors: the binding of include/evt_gram.h.

    out = model.activation_grams(img)                       # every block's FFN hidden activations
    out["gram"], out["sum"], out["rows"]                    # [[F_i, F_i]], [[F_i]], B * T
    out = model.activation_grams(img, blocks=(-1, 0), what="attn", logits=True)
    model.activation_grams_into(img, blocks=(3, 11), what="ffn", gram_tensors=(g3, g11),
                                sum_tensors=(s3, s11))
    model.gram_shape(-1, "attn")                            # (width, tokens) of a block

Second moments of the matrix H a pruned layer's consumer reads, fp32 whatever the model's dtype,
formed on the device without exporting H (620 MB per block at DeiT-base and 512 images):

    what="ffn"    H = the FC1 output FC2 multiplies, [B T, F_i]
    what="attn"   H = the attention context the out-projection multiplies, [B T, heads_i * head_dim_i]

    gram = H^T H  (both triangles, bitwise symmetric)        sum = the column sums of H

All B T token rows of the batch enter one Gram: it is a statistic of the batch, not of an image.
`pruning.reconstruct_linear` turns the Grams of a calibration set (`evaluate.collect_grams`) into
least-squares repaired FC2 / out-projection weights. They come from the same forward that produces
the logits (one or two more launches per requested block), so `logits=True` / `pooled=True` return
bitwise what `model(img)` / `forward_features(img)` return. ViT (reference and standard, pruned or
not) and T2T_ViT have them; Swin and "mx8" models raise ValueError, and so does a model with a
token schedule or a request for a skipped sublayer.

The scratch the C ABI asks of its caller (the fp32 partial tiles of the row chunks) is allocated
here once per size and kept on the model object; it goes with the model.

`gram_reference` is the same contract in numpy fp64, from a hidden matrix.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ... import _lib
from .features import resolve_taps
from .ffn_stats import FFNStats

WHAT = {"ffn": _lib.GRAM_FFN, "attn": _lib.GRAM_ATTN}


def resolve_what(what) -> int:
    """EVT_GRAM_FFN / EVT_GRAM_ATTN of a `what=` argument ("ffn" / "attn" or the constant)."""
    if isinstance(what, str) and what in WHAT:
        return WHAT[what]
    if not isinstance(what, (str, bool)) and what in (_lib.GRAM_FFN, _lib.GRAM_ATTN):
        return int(what)
    raise ValueError(f"what must be 'ffn' or 'attn', got {what!r}")


def gram_reference(hidden) -> Dict[str, object]:
    """The contract of include/evt_gram.h in numpy fp64: a matrix [..., F] (every leading axis is
    rows) -> {"gram": [F, F], "sum": [F], "rows": R}."""
    a = np.asarray(hidden, dtype=np.float64)
    if a.ndim < 2 or a.shape[-1] < 1 or a.size == 0:
        raise ValueError(f"hidden must be [..., R >= 1, F >= 1], got {a.shape}")
    a = a.reshape(-1, a.shape[-1])
    return {"gram": a.T @ a, "sum": a.sum(0), "rows": a.shape[0]}


class ActivationGrams(FFNStats):
    """What ViT, T2T_ViT and SwinTransformer derive from (through Classification): the activation
    Grams on top of the FFN statistics. The model class provides `_ffn_geometry()` and
    `_attn_context_geometry()` -> [(width, tokens) per encoder block], or leaves the defaults, which
    raise (Swin)."""

    def _attn_context_geometry(self) -> List[Tuple[int, int]]:
        raise ValueError(f"{type(self).__name__} has no activation Grams: its window attention "
                         "does not store the context rows of a block")

    def _gram_blocks(self, what: int) -> List[Tuple[int, int]]:
        if getattr(self, "dtype", None) == "mx8":
            raise ValueError("activation Grams are not available on an 'mx8' model: its hidden and "
                             "attention rows are kept quantised")
        try:
            return self._ffn_geometry() if what == _lib.GRAM_FFN else self._attn_context_geometry()
        except ValueError as e:
            raise ValueError(f"{type(self).__name__} has no activation Grams: its fused kernels do "
                             "not store the rows a Gram is formed of") from e

    def gram_shape(self, block: int, what="ffn") -> Tuple[int, int]:
        """(width of the Gram, tokens per image) of `block` (negative: from the last). Host only."""
        geo = self._gram_blocks(resolve_what(what))
        return geo[resolve_taps((block,), len(geo))[0]]

    def _gram_scratch(self, need: int) -> Optional[torch.Tensor]:
        """The call's scratch: grown to the largest size asked for, kept on the model."""
        if not need:
            return None
        t = self.__dict__.get("_gram_scratch_buf")
        if t is None or t.numel() < need:
            t = self.__dict__["_gram_scratch_buf"] = torch.empty(need, dtype=torch.uint8,
                                                                 device=self.device)
        return t

    def activation_grams_into(self, img, *, blocks: Sequence[int], what="ffn",
                              gram_tensors: Sequence[torch.Tensor],
                              sum_tensors: Sequence[torch.Tensor], logits: torch.Tensor = None,
                              pooled: torch.Tensor = None) -> None:
        """Enqueue one forward of a device-resident batch (fp32 in the model's layout, or a
        `Uint8Images`) that fills `gram_tensors[i]` [F, F] and `sum_tensors[i]` [F] with the Gram
        and column sums of block `blocks[i]` over all B T rows of the batch, and the given `logits`
        [B, num_classes] / `pooled` [B, features] tensors; no synchronisation, and no allocation
        after the first call of a size (evt_forward_grams)."""
        which = resolve_what(what)
        geo = self._gram_blocks(which)
        idx = resolve_taps(blocks, len(geo))
        b = img.shape[0]
        keep_g = self._block_list(idx, gram_tensors, lambda i: (geo[i][0], geo[i][0]),
                                  "gram_tensors", "block")
        keep_s = self._block_list(idx, sum_tensors, lambda i: (geo[i][0],), "sum_tensors", "block")
        feat = self._feat_args(b, logits=logits, pooled=pooled)
        if not (idx or feat[1]):
            raise ValueError("no output requested")
        a = _lib.evt_gram_args()
        a.n_blocks, a.which = len(idx), which
        if idx:
            a.blocks, a.grams = keep_g
            a.sums = keep_s[1]
            lib, need = _lib.load_library(), 0
            for i in idx:
                n = ctypes.c_size_t()
                _lib.check(lib.evt_gram_scratch_bytes(b * geo[i][1], geo[i][0], ctypes.byref(n)))
                need = max(need, n.value)
            self._fit(img)
            with torch.cuda.device(self.device):
                scratch = self._gram_scratch(need)
            if scratch is not None:
                a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
        self._analysis_forward("evt_forward_grams", img, feat, a)

    def activation_grams(self, img, blocks: Optional[Sequence[int]] = None, what="ffn",
                         logits: bool = False, pooled: bool = False) -> Dict[str, object]:
        """{"gram": [one [F_i, F_i] per block, in the order given], "sum": [one [F_i] per block],
        "rows": B * T} plus the requested "logits" / "pooled"; `blocks=None`: every block. numpy
        in, numpy out; a device tensor (or a device `Uint8Images`) gives device tensors."""
        which = resolve_what(what)
        geo = self._gram_blocks(which)
        idx = resolve_taps(range(len(geo)) if blocks is None else blocks, len(geo))
        out = self._block_outputs(
            img, ("gram", "sum"), idx,
            (lambda b, i: (geo[i][0], geo[i][0]), lambda b, i: (geo[i][0],)),
            lambda x, g, s, **kw: self.activation_grams_into(x, blocks=idx, what=which,
                                                             gram_tensors=g, sum_tensors=s, **kw),
            logits=logits, pooled=pooled)
        out["rows"] = img.shape[0] * geo[0][1]
        return out
