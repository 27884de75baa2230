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

import ctypes
from typing import Dict, List, Sequence, Tuple

import torch

from ... import _lib
from ...images import Uint8Images
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
        geo = self._attn_blocks()
        idx = resolve_taps(blocks, len(geo))
        q = resolve_queries(queries)
        if len(map_tensors) != len(idx):
            raise ValueError("map_tensors needs one tensor per block")
        b = img.shape[0]
        order = sorted(range(len(idx)), key=idx.__getitem__)  # the C ABI wants them rising
        ptrs = [self._feature_tensor(f"map_tensors[{i}]", map_tensors[i],
                                     self._map_shape(b, idx[i], q)) for i in order]
        feat = _lib.evt_features_args()
        feat.logits = self._feature_tensor("logits", logits, (b, self.num_classes))
        feat.pooled = self._feature_tensor("pooled", pooled, (b, self.feature_dim))
        if not (idx or feat.logits or feat.pooled):
            raise ValueError("no output requested")
        a = _lib.evt_attn_args()
        a.n_maps, a.queries = len(idx), q
        keep = ((ctypes.c_int32 * max(1, len(idx)))(*[idx[i] for i in order]),
                (ctypes.c_void_p * max(1, len(idx)))(*ptrs))
        if idx:
            a.blocks, a.maps = keep
        if isinstance(img, Uint8Images):
            args = img.image_args()
        else:
            args = _lib.evt_image_args()
            args.data, args.format = img.data_ptr(), 0  # EVT_IMG_F32
        self._fit(img)
        _lib.check(_lib.load_library().evt_forward_attention(
            self._ptr(), ctypes.byref(args), b,
            ctypes.byref(feat) if (feat.logits or feat.pooled) else None, ctypes.byref(a),
            self._stream()))

    def attention_maps(self, img, *, blocks: Sequence[int] = (-1,), queries="cls",
                       logits: bool = False, pooled: bool = False) -> Dict[str, object]:
        """{"maps": [one per block, in the order given]} plus the requested "logits" / "pooled".
        numpy in, numpy out; a device tensor (or a device `Uint8Images`) gives device tensors."""
        geo = self._attn_blocks()
        idx = resolve_taps(blocks, len(geo))
        q = resolve_queries(queries)
        x, was_numpy = self._checked_image(img)
        b = x.shape[0]
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)  # noqa: E731
        out: Dict[str, object] = {"maps": [new(*self._map_shape(b, i, q)) for i in idx]}
        if logits:
            out["logits"] = new(b, self.num_classes)
        if pooled:
            out["pooled"] = new(b, self.feature_dim)
        with torch.cuda.device(self.device):
            self.attention_maps_into(x, blocks=idx, map_tensors=out["maps"], queries=q,
                                     logits=out.get("logits"), pooled=out.get("pooled"))
        if was_numpy:  # .cpu() waits for the stream, as __call__ does
            out = {k: [v.cpu().numpy() for v in val] if isinstance(val, list) else val.cpu().numpy()
                   for k, val in out.items()}
        return out
