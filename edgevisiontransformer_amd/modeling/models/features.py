"""Feature outputs of the model mirrors: the binding of include/evt_features.h.

The models of this package are mostly used as backbones; besides `model(img)` (logits) every
mirror class offers

    emb = model.forward_features(img)                  # [B, F]: what the classifier reads
    out = model.features(img, tokens=True, taps=(3, 7, -1))
    out["pooled"], out["tokens"], out["taps"]          # [B, F], [B, T, F], list of [B, T_i, C_i]
    model.features_into(img, pooled=p, tokens=t)       # preallocated device tensors, no allocation

`forward_features` is the reference name and meaning (`T2T_ViT.forward_features`, reference
t2t_vit.py:120-130: LayerNorm then the CLS token; microsoft `SwinTransformer.forward_features`:
LayerNorm, token mean). Per family (the table in include/evt_features.h): a REFERENCE `ViT` has no
final LayerNorm, so its pooled / tokens are the last block's output as it stands; `StandardViT`
and `T2T_ViT` give LN(x); Swin gives the token mean of LN(x) and the last stage's LN(x) map.
A tap is the residual stream after a block (negative indices count from the last one);
`tap_norm=True` passes the taps through the final LayerNorm (StandardViT and T2T_ViT only).
Everything comes back fp32, whatever the model's dtype.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from ... import _lib
from ...images import Uint8Images
from ._handle import ModelHandle

MAX_TAPS = 64  # include/evt_features.h: n_taps 0..64


def resolve_taps(taps: Sequence[int], num_blocks: int, *, tap_norm: bool = False,
                 tap_norm_ok: bool = True) -> List[int]:
    """Block indices of a `taps=` argument, in the order given (host only, no device call).

    Negative indices count from the last block. ValueError: an index outside [-num_blocks,
    num_blocks), a block named twice, more than 64 taps, or `tap_norm` on a model whose taps
    cannot take the final LayerNorm (`tap_norm_ok` False: REFERENCE ViT, Swin)."""
    if tap_norm and not tap_norm_ok:
        raise ValueError("tap_norm=True needs a final LayerNorm of the taps' width: StandardViT and "
                         "T2T_ViT have one; a reference ViT has none, Swin stage widths differ")
    out = []
    for t in taps:
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)):
            raise ValueError(f"tap indices must be integers, got {t!r}")
        i = int(t) + num_blocks if t < 0 else int(t)
        if not 0 <= i < num_blocks:
            raise ValueError(f"tap {int(t)} is outside the model's {num_blocks} blocks")
        if i in out:
            raise ValueError(f"block {i} is tapped twice")
        out.append(i)
    if len(out) > MAX_TAPS:
        raise ValueError(f"at most {MAX_TAPS} taps per call")
    return out


def outputs_to_numpy(out: Dict[str, object]) -> Dict[str, object]:
    """The host copy of a dict of device tensors and lists of them (.cpu() waits for the stream,
    as `__call__` does)."""
    return {k: [t.cpu().numpy() for t in v] if isinstance(v, list) else v.cpu().numpy()
            for k, v in out.items()}


class FeatureOutputs(ModelHandle):
    """What ViT, T2T_ViT and SwinTransformer derive from: the feature outputs on top of the handle
    plumbing (_handle.py). The model class provides `_feature_geometry()` -> (F, T, [(tokens,
    width) per block]), `_image_dims()` -> the [1:] shape of its input, and `_TAP_NORM_OK`."""

    _TAP_NORM_OK = False

    @property
    def feature_dim(self) -> int:
        """F: the width of `forward_features(img)` and of the final token map."""
        return self._feature_geometry()[0]

    @property
    def num_blocks(self) -> int:
        """Blocks a tap can name (Swin: numbered consecutively over the stages)."""
        return len(self._feature_geometry()[2])

    def tap_shape(self, block: int) -> Tuple[int, int]:
        """(tokens per image, width) of the tap after `block` (negative: from the last)."""
        return self._feature_geometry()[2][resolve_taps((block,), self.num_blocks)[0]]

    def _feature_tensor(self, name: str, t, shape) -> int:
        if t is None:
            return 0
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() \
                or t.device != self.device or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be a contiguous float32 tensor of shape {tuple(shape)} "
                             f"on {self.device}")
        return t.data_ptr()

    # -- what the per-block outputs share (the analysis forwards of the classes on top of this one) --
    def _feat_shapes(self, b: int) -> Dict[str, Tuple[int, ...]]:
        f, t, _ = self._feature_geometry()
        return {"logits": (b, self.cfg.num_classes), "pooled": (b, f), "tokens": (b, t, f)}

    def _feat_args(self, b: int, **tensors):
        """(the evt_features_args of the fp32 device tensors `logits` [b, num_classes] / `pooled`
        [b, F] / `tokens` [b, T, F] given, None: not asked for, checked in the order given; whether
        any of them is set)."""
        a, shapes = _lib.evt_features_args(), self._feat_shapes(b)
        for name, t in tensors.items():
            setattr(a, name, self._feature_tensor(name, t, shapes[name]))
        return a, bool(a.logits or a.pooled or a.tokens)

    def _block_list(self, blocks: Sequence[int], tensors: Sequence[torch.Tensor], shape, name: str,
                    per: str):
        """The block and pointer arrays of a per-block output list for the C ABI, which wants the
        blocks rising: `tensors[i]` (of `shape(blocks[i])`, named `name[i]` in an error) is the
        output of block `blocks[i]`, in the caller's order; ValueError(f"{name} needs one tensor per
        {per}") on another count. The caller keeps the arrays alive until after the call."""
        if len(tensors) != len(blocks):
            raise ValueError(f"{name} needs one tensor per {per}")
        order = sorted(range(len(blocks)), key=blocks.__getitem__)
        ptrs = [self._feature_tensor(f"{name}[{i}]", tensors[i], shape(blocks[i])) for i in order]
        n = max(1, len(blocks))  # (ctypes: no zero-length arrays to point at)
        return (ctypes.c_int32 * n)(*[blocks[i] for i in order]), (ctypes.c_void_p * n)(*ptrs)

    def _analysis_forward(self, fn: str, img, feat, args) -> None:
        """The analysis forward `fn` (evt_forward_attention, ...) of a device-resident batch (fp32 in
        the model's layout, or a `Uint8Images`) with the outputs `feat` = `_feat_args(...)` and the
        entry point's own `args`."""
        image = self._image_args(img)
        b = self._fit(img)
        _lib.check(getattr(_lib.load_library(), fn)(
            self._ptr(), ctypes.byref(image), b, ctypes.byref(feat[0]) if feat[1] else None,
            ctypes.byref(args), self._stream()))

    def _block_outputs(self, img, key, blocks: Sequence[int], shape, into,
                       **want: bool) -> Dict[str, object]:
        """What the allocating wrappers share: {key: [one fp32 tensor of `shape(b, block)` per block
        of `blocks`]} plus the "logits" / "pooled" / "tokens" asked for in `want`, filled by
        `into(x, tensors, logits=..., ...)` on the model's device. numpy in, numpy out. With a tuple
        of keys and as many shape functions there is one list per key, and `into` gets the lists in
        that order: `into(x, tensors_0, tensors_1, ..., logits=..., ...)`."""
        keys, shapes_of = ((key,), (shape,)) if isinstance(key, str) else (tuple(key), tuple(shape))
        x, was_numpy = self._checked_image(img)
        b = x.shape[0]
        new = lambda shape: torch.empty(shape, dtype=torch.float32, device=self.device)  # noqa: E731
        out: Dict[str, object] = {k: [new(f(b, i)) for i in blocks] for k, f in zip(keys, shapes_of)}
        shapes = self._feat_shapes(b)
        out.update({k: new(shapes[k]) for k, wanted in want.items() if wanted})
        with torch.cuda.device(self.device):
            into(x, *[out[k] for k in keys], **{k: out.get(k) for k in want})
        return outputs_to_numpy(out) if was_numpy else out

    def features_into(self, img: torch.Tensor, *, pooled: torch.Tensor = None,
                      tokens: torch.Tensor = None, logits: torch.Tensor = None,
                      taps: Sequence[int] = (), tap_tensors: Sequence[torch.Tensor] = (),
                      tap_norm: bool = False) -> None:
        """Enqueue one forward of a device-resident batch that fills the given fp32 device tensors
        (`pooled` [B, F], `tokens` [B, T, F], `logits` [B, num_classes], `tap_tensors[i]` the tap
        after block `taps[i]`); no allocation, no synchronisation (evt_forward_features)."""
        blocks = resolve_taps(taps, self.num_blocks, tap_norm=tap_norm,
                              tap_norm_ok=self._TAP_NORM_OK)
        b, geo = img.shape[0], self._feature_geometry()[2]
        keep = self._block_list(blocks, tap_tensors, lambda i: (b, *geo[i]), "tap_tensors", "tap")
        a, any_set = self._feat_args(b, pooled=pooled, tokens=tokens, logits=logits)
        if not (any_set or blocks):
            raise ValueError("no output requested")
        a.n_taps, a.tap_norm = len(blocks), int(bool(tap_norm))
        if blocks:
            a.tap_blocks, a.taps = keep
        if isinstance(img, Uint8Images):  # device-resident uint8 NHWC (include/evt_image.h)
            return self._forward_image(img, a)
        self._fit(img)
        _lib.check(_lib.load_library().evt_forward_features(
            self._ptr(), ctypes.c_void_p(img.data_ptr()), b, ctypes.byref(a), self._stream()))

    def features(self, img, *, tokens: bool = False, taps: Sequence[int] = (),
                 tap_norm: bool = False, logits: bool = False) -> Dict[str, object]:
        """{"pooled": [B, F]} plus the requested "tokens" [B, T, F], "logits" and "taps" (a list in
        the order given). numpy in, numpy out; a device tensor gives device tensors."""
        blocks = resolve_taps(taps, self.num_blocks, tap_norm=tap_norm,
                              tap_norm_ok=self._TAP_NORM_OK)
        geo = self._feature_geometry()[2]
        out = self._block_outputs(
            img, "taps", blocks, lambda b, i: (b, *geo[i]),
            lambda x, t, **kw: self.features_into(x, taps=blocks, tap_tensors=t, tap_norm=tap_norm,
                                                  **kw),
            pooled=True, tokens=tokens, logits=logits)
        tapped = out.pop("taps")  # last, and only when asked for
        if blocks:
            out["taps"] = tapped
        return out

    def forward_features(self, img):
        """Pooled features [B, F]: the vector the classifier reads (reference
        `T2T_ViT.forward_features`, microsoft `SwinTransformer.forward_features`)."""
        return self.features(img)["pooled"]
