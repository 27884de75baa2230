"""Window attention maps of SwinTransformer: the binding of include/evt_window_attention.h.

    out = model.window_attention_maps(img, blocks=(-1,))       # the last block's windows
    out["maps"]                        # list of [B, nW, H_i, N, N] fp32, N = window * window
    out = model.window_attention_maps(img, blocks=range(model.num_blocks), logits=True)
    model.window_attention_maps_into(img, blocks=(0, 1), map_tensors=(a, b))
    model.window_attn_shape(-1)        # (windows, heads, tokens per window) of a block
    idx = model.window_token_index(1)  # [nW, N] raster tokens: maps[b, w, h, q, k] is attention
                                       # from token idx[w, q] to token idx[w, k]

The maps are the softmax probabilities of the chosen blocks' windows, relative position bias and
SW-MSA mask included (a query / key pair in different regions of a shifted window is exactly 0),
fp32 whatever the model's dtype, indexed [image, window, head, query, key] with the windows and
their tokens in the shifted frame (`window_token_index` maps them back to raster tokens). They come
from the same forward that produces the logits, so `logits=True` / `pooled=True` return bitwise
what `model(img)` / `forward_features(img)` return. ViT and T2T_ViT raise ValueError: their maps
are `attention_maps`.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from ... import _lib
from .attention_maps import AttentionMaps
from .features import resolve_taps


def window_token_index(res: int, window: int, shift: int) -> np.ndarray:
    """int64 [nW, N]: the raster token (y * res + x) of every window-local token of a res x res
    token map cut into window x window windows after a cyclic shift by -shift along both axes
    (host only)."""
    if window <= 0 or res <= 0 or res % window or not 0 <= shift < window:
        raise ValueError(f"bad window geometry: resolution {res}, window {window}, shift {shift}")
    nw = res // window
    wy, wx, i, j = np.meshgrid(np.arange(nw), np.arange(nw), np.arange(window), np.arange(window),
                               indexing="ij")
    y, x = (wy * window + i + shift) % res, (wx * window + j + shift) % res
    return (y * res + x).reshape(nw * nw, window * window).astype(np.int64)


class WindowAttentionMaps(AttentionMaps):
    """What ViT, T2T_ViT and SwinTransformer derive from: the window attention maps on top of the
    attention maps (attention_maps.py). The model class provides `_window_geometry()` ->
    [(resolution, window, shift, heads) per block], or leaves the default, which raises (ViT,
    T2T_ViT)."""

    def _window_geometry(self) -> List[Tuple[int, int, int, int]]:
        raise ValueError(f"{type(self).__name__} has no window attention maps: its attention is "
                         "global, use attention_maps")

    def window_attn_shape(self, block: int) -> Tuple[int, int, int]:
        """(windows per image, heads, tokens per window) of the map of `block` (negative: from the
        last)."""
        geo = self._window_geometry()
        r, w, _, h = geo[resolve_taps((block,), len(geo))[0]]
        return (r // w) ** 2, h, w * w

    def window_token_index(self, block: int) -> np.ndarray:
        """int64 numpy [nW, N]: the raster token (y * R + x, the block's shift included) of every
        window-local token of `block`, so maps[b, w, h, q, k] is the attention from token
        idx[w, q] to token idx[w, k]. Host only."""
        geo = self._window_geometry()
        r, w, s, _ = geo[resolve_taps((block,), len(geo))[0]]
        return window_token_index(r, w, s)

    def _window_map_shape(self, b: int, block: int) -> Tuple[int, ...]:
        r, w, _, h = self._window_geometry()[block]
        return (b, (r // w) ** 2, h, w * w, w * w)

    def window_attention_maps_into(self, img, *, blocks: Sequence[int],
                                   map_tensors: Sequence[torch.Tensor],
                                   logits: torch.Tensor = None,
                                   pooled: torch.Tensor = None) -> None:
        """Enqueue one forward of a device-resident batch (fp32 NCHW, or a `Uint8Images`) that
        fills `map_tensors[i]` with the window map of block `blocks[i]` and the given `logits`
        [B, num_classes] / `pooled` [B, F] tensors; no allocation, no synchronisation
        (evt_forward_window_attention)."""
        idx = resolve_taps(blocks, len(self._window_geometry()))
        b = img.shape[0]
        keep = self._block_list(idx, map_tensors, lambda i: self._window_map_shape(b, i),
                                "map_tensors", "block")
        feat = self._feat_args(b, logits=logits, pooled=pooled)
        if not (idx or feat[1]):
            raise ValueError("no output requested")
        a = _lib.evt_attn_args()
        a.n_maps, a.queries = len(idx), _lib.ATTN_ALL
        if idx:
            a.blocks, a.maps = keep
        self._analysis_forward("evt_forward_window_attention", img, feat, a)

    def window_attention_maps(self, img, *, blocks: Sequence[int] = (-1,), logits: bool = False,
                              pooled: bool = False) -> Dict[str, object]:
        """{"maps": [one [B, nW, H, N, N] per block, in the order given]} plus the requested
        "logits" / "pooled". numpy in, numpy out; a device tensor (or a device `Uint8Images`)
        gives device tensors."""
        idx = resolve_taps(blocks, len(self._window_geometry()))
        return self._block_outputs(
            img, "maps", idx, self._window_map_shape,
            lambda x, t, **kw: self.window_attention_maps_into(x, blocks=idx, map_tensors=t, **kw),
            logits=logits, pooled=pooled)
