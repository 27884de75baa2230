"""Attention-map outputs of the model mirrors: the binding of include/evt_attention_maps.h.

    out = model.attention_maps(img, blocks=(-1,), queries="cls")   # DINO-style CLS maps
    out["maps"]                       # list of [B, H_i, T] (queries="all": [B, H_i, T, T])
    out = model.attention_maps(img, blocks=range(model.num_blocks), queries="all", logits=True)
    model.attention_maps_into(img, blocks=(3, 11), map_tensors=(a, b), queries="cls")
    model.attn_shape(-1)              # (heads, tokens) of a block

The maps are the softmax probabilities of the chosen encoder blocks, fp32 whatever the model's
dtype, indexed [image, head, (query,) key]; `queries="cls"` is bitwise `queries="all"`[:, :, 0].
They come from the same forward that produces the logits (one more kernel per requested block,
right after the block's attention kernel), so `logits=True` / `pooled=True` return bitwise what
`model(img)` / `forward_features(img)` return. ViT (reference and standard, pruned or not) and
T2T_ViT have them; Swin's windowed, biased attention and "mx8" models raise ValueError.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import torch

from ... import _lib
from .features import FeatureOutputs, resolve_taps

QUERIES = {"cls": _lib.ATTN_CLS, "all": _lib.ATTN_ALL}


def resolve_queries(queries) -> int:
    """EVT_ATTN_CLS / EVT_ATTN_ALL of a `queries=` argument ("cls" / "all" or the constant)."""
    if isinstance(queries, str) and queries in QUERIES:
        return QUERIES[queries]
    if not isinstance(queries, (str, bool)) and queries in (_lib.ATTN_CLS, _lib.ATTN_ALL):
        return int(queries)
    raise ValueError(f"queries must be 'cls' or 'all', got {queries!r}")


class AttentionMaps(FeatureOutputs):
    """What ViT, T2T_ViT and SwinTransformer derive from: the attention maps on top of the feature
    outputs (features.py). The model class provides `_attn_geometry()` -> [(heads, tokens) per
    encoder block], or leaves the default, which raises (Swin)."""

    def _attn_geometry(self) -> List[Tuple[int, int]]:
        raise ValueError(f"{type(self).__name__} has no attention maps: its windowed, biased "
                         "attention is a different object")

    def _attn_blocks(self) -> List[Tuple[int, int]]:
        if getattr(self, "dtype", None) == "mx8":
            raise ValueError("attention maps are not available on an 'mx8' model")
        return self._attn_geometry()

    def attn_shape(self, block: int) -> Tuple[int, int]:
        """(heads, tokens per image) of the map of `block` (negative: from the last)."""
        geo = self._attn_blocks()
        return geo[resolve_taps((block,), len(geo))[0]]

    def _map_shape(self, b: int, block: int, q: int) -> Tuple[int, ...]:
        h, t = self._attn_blocks()[block]
        return (b, h, t, t) if q == _lib.ATTN_ALL else (b, h, t)

    def attention_maps_into(self, img, *, blocks: Sequence[int],
                            map_tensors: Sequence[torch.Tensor], queries="cls",
                            logits: torch.Tensor = None, pooled: torch.Tensor = None) -> None:
        """Enqueue one forward of a device-resident batch (fp32 in the model's layout, or a
        `Uint8Images`) that fills `map_tensors[i]` with the map of block `blocks[i]` and the given
        `logits` [B, num_classes] / `pooled` [B, F] tensors; no allocation, no synchronisation
        (evt_forward_attention)."""
        idx = resolve_taps(blocks, len(self._attn_blocks()))
        q = resolve_queries(queries)
        b = img.shape[0]
        keep = self._block_list(idx, map_tensors, lambda i: self._map_shape(b, i, q),
                                "map_tensors", "block")
        feat = self._feat_args(b, logits=logits, pooled=pooled)
        if not (idx or feat[1]):
            raise ValueError("no output requested")
        a = _lib.evt_attn_args()
        a.n_maps, a.queries = len(idx), q
        if idx:
            a.blocks, a.maps = keep
        self._analysis_forward("evt_forward_attention", img, feat, a)

    def attention_maps(self, img, *, blocks: Sequence[int] = (-1,), queries="cls",
                       logits: bool = False, pooled: bool = False) -> Dict[str, object]:
        """{"maps": [one per block, in the order given]} plus the requested "logits" / "pooled".
        numpy in, numpy out; a device tensor (or a device `Uint8Images`) gives device tensors."""
        idx = resolve_taps(blocks, len(self._attn_blocks()))
        q = resolve_queries(queries)
        return self._block_outputs(
            img, "maps", idx, lambda b, i: self._map_shape(b, i, q),
            lambda x, t, **kw: self.attention_maps_into(x, blocks=idx, map_tensors=t, queries=q, **kw),
            logits=logits, pooled=pooled)
