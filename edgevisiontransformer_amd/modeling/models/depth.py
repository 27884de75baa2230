"""The depth axis of the ViT mirrors: the binding of include/evt_depth.h.

    out = model.block_stats(img)                   # every block
    out["stats"]                                   # list of [B, 2, 4]: [image, ("attn", "ffn"), DEPTH_STATS]
    model.block_stats_into(img, blocks=(3, 11), stat_tensors=(a, b))
    means = collect_block_stats(model, loader)     # dataset means, fp64, one [2, 4] per block

    model.skip_sublayers({5: "attn", 9: "block", -1: "ffn"})
    with model.skipping({10: "attn", 11: "attn"}):    # the previous mask comes back on exit
        acc = evaluate(model, loader)
    model.skipped(); model.clear_skips()

Statistics: how much a sublayer changes the token stream, reduced on the device from the
sublayer's input rows a and output rows b as stored in the model's dtype, per image over its T
tokens, in fp32 (`block_stats_reference` is the contract in numpy fp64):

    cosine      mean_t  a_t . b_t / max(|a_t| |b_t|, FLT_MIN)
    rel_update  mean_t  |b_t - a_t| / max(|a_t|, FLT_MIN)
    norm_ratio  mean_t  |b_t| / max(|a_t|, FLT_MIN)
    cls_cosine  the cosine of token 0

They come from the forward that produces the logits (two more kernels per requested sublayer), so
`logits=True` / `pooled=True` return bitwise what `model(img)` / `forward_features(img)` return.

Skips: a skipped sublayer is absent from the forward. The stream passes through unchanged, the
sublayer's LayerNorm goes with it, and none of its kernels is launched, so the forward gets faster.
A model with whole blocks skipped is bitwise a fresh model of `pruning.drop_blocks(params, cfg,
blocks)`. A skipped sublayer reports the identity statistics (1, 0, 1, 1). The mask stays with the
model across handle rebuilds; gates of a skipped sublayer are kept and act again after the skip is
cleared. `attention_maps`, `head_stats`, `attention_rollout` and a token-schedule entry on a block
whose attention is skipped, and `ffn_stats` of a block whose FFN is skipped, raise ValueError.

ViT, ViT_Pruned and StandardViT in "f32" and "bf16" have both; T2T_ViT, SwinTransformer and "mx8"
models raise ValueError, and so does `block_stats` while a token schedule is set.
"""
from __future__ import annotations

import contextlib
import ctypes
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from ... import _lib
from .features import resolve_taps
from .gates import StructuredGates

DEPTH_STATS = ("cosine", "rel_update", "norm_ratio", "cls_cosine")
SUBLAYERS = ("attn", "ffn")
SKIP_BITS = {"attn": _lib.SKIP_ATTN, "ffn": _lib.SKIP_FFN, "block": _lib.SKIP_ATTN | _lib.SKIP_FFN}
SKIP_NAMES = {v: k for k, v in SKIP_BITS.items()}
IDENTITY_STATS = (1.0, 0.0, 1.0, 1.0)
FLT_MIN = float(np.finfo(np.float32).tiny)


def block_stats_reference(a, b, T: int) -> np.ndarray:
    """The contract of include/evt_depth.h in numpy fp64: row matrices a, b [B * T, D] (row b T + t
    is token t of image b) -> [B, 4] in DEPTH_STATS order."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.ndim != 2 or a.shape != b.shape or T < 1 or a.shape[0] % T:
        raise ValueError(f"a and b must be [B * T, D] with T = {T}, got {a.shape} and {b.shape}")
    na, nb = np.sqrt((a * a).sum(-1)), np.sqrt((b * b).sum(-1))
    d = b - a
    cos = (a * b).sum(-1) / np.maximum(na * nb, FLT_MIN)
    rel = np.sqrt((d * d).sum(-1)) / np.maximum(na, FLT_MIN)
    ratio = nb / np.maximum(na, FLT_MIN)
    cos, rel, ratio = (v.reshape(-1, T) for v in (cos, rel, ratio))
    return np.stack([cos.mean(-1), rel.mean(-1), ratio.mean(-1), cos[:, 0]], axis=-1)


def checked_skips(depth: int, skips: Optional[Mapping[int, str]]) -> List[int]:
    """`{block: "attn" | "ffn" | "block"}` on a model of `depth` blocks -> the mask, one byte per
    block (bit 0 attention, bit 1 FFN). Negative blocks count from the last; a block named twice
    gets both. ValueError: a block out of range or another word."""
    mask = [0] * depth
    for block, what in (skips or {}).items():
        if isinstance(block, bool) or not isinstance(block, (int, np.integer)):
            raise ValueError(f"skip blocks must be integers, got {block!r}")
        i = int(block) + depth if block < 0 else int(block)
        if not 0 <= i < depth:
            raise ValueError(f"block {block} is outside the model's {depth} blocks")
        if what not in SKIP_BITS:
            raise ValueError(f'block {block}: a skip is "attn", "ffn" or "block", got {what!r}')
        mask[i] |= SKIP_BITS[what]
    return mask


def mask_to_skips(mask: Sequence[int]) -> Dict[int, str]:
    """The mask -> `{block: "attn" | "ffn" | "block"}` of its non-zero entries."""
    return {i: SKIP_NAMES[int(v)] for i, v in enumerate(mask) if v}


def parse_skips(spec: Optional[str]) -> Dict[int, str]:
    """'5:attn,9:block,-1:ffn' -> {5: "attn", 9: "block", -1: "ffn"} (tools.py --skip). A block
    named with both sublayers becomes "block"."""
    out: Dict[int, str] = {}
    for part in (spec or "").split(","):
        if not part.strip():
            continue
        try:
            b, what = part.split(":")
            block, what = int(b), what.strip()
        except ValueError:
            raise ValueError(f"skip entries are block:attn|ffn|block, got {part!r}") from None
        if what not in SKIP_BITS:
            raise ValueError(f"skip entries are block:attn|ffn|block, got {part!r}")
        bits = SKIP_BITS[what] | SKIP_BITS.get(out.get(block, ""), 0)
        out[block] = SKIP_NAMES[bits]
    return out


class DepthAxis(StructuredGates):
    """What ViT, T2T_ViT and SwinTransformer derive from: the stream statistics and the sublayer
    skips on top of everything else. A class that supports them sets `_DEPTH_OK`."""

    _DEPTH_OK = False
    _skip_mask: Optional[List[int]] = None  # one byte per block; None: no skips

    def _depth_refused(self, what: str) -> None:
        if not self._DEPTH_OK:
            raise ValueError(f"{type(self).__name__} has no {what}: the depth axis is ViT's (ViT, "
                             "ViT_Pruned, StandardViT)")
        if getattr(self, "dtype", None) == "mx8":
            raise ValueError(f"{what} is not available on an 'mx8' model")

    @staticmethod
    def _einval(fn, *args, **kw):
        try:
            return fn(*args, **kw)
        except _lib.EvtError as e:
            if e.code == _lib.EVT_EINVAL:
                raise ValueError(str(e)) from e
            raise

    # -- statistics -----------------------------------------------------------------------------
    def block_stats_shape(self, block: int) -> Tuple[int, int, int]:
        """(sublayers, statistics, tokens per image) of `block` (negative: from the last): (2, 4,
        T). Host only."""
        self._depth_refused("block statistics")
        resolve_taps((block,), self.cfg.depth)
        return len(SUBLAYERS), _lib.DEPTH_STATS, self.cfg.tokens

    def block_stats_into(self, img, *, blocks: Sequence[int], stat_tensors: Sequence[torch.Tensor],
                         logits: torch.Tensor = None, pooled: torch.Tensor = None) -> None:
        """Enqueue one forward of a device-resident batch (fp32 in the model's layout, or a
        `Uint8Images`) that fills `stat_tensors[i]` [B, 2, 4] with the statistics of block
        `blocks[i]` and the given `logits` / `pooled` tensors; no allocation, no synchronisation
        (evt_forward_block_stats)."""
        self._depth_refused("block statistics")
        idx = resolve_taps(blocks, self.cfg.depth)
        b = img.shape[0]
        keep = self._block_list(idx, stat_tensors,
                                lambda i: (b, len(SUBLAYERS), _lib.DEPTH_STATS), "stat_tensors",
                                "block")
        feat = self._feat_args(b, logits=logits, pooled=pooled)
        if not (idx or feat[1]):
            raise ValueError("no output requested")
        a = _lib.evt_block_stats_args()
        a.n_blocks = len(idx)
        if idx:
            a.blocks, a.stats = keep
        try:
            self._analysis_forward("evt_forward_block_stats", img, feat, a)
        except _lib.EvtError as e:
            if e.code == _lib.EVT_EINVAL and "token schedule" in str(e):
                raise ValueError(str(e)) from e
            raise

    def block_stats(self, img, blocks: Optional[Sequence[int]] = None, logits: bool = False,
                    pooled: bool = False) -> Dict[str, object]:
        """{"stats": [one [B, 2, 4] per block, in the order given]} plus the requested "logits" /
        "pooled"; `blocks=None`: every block. numpy in, numpy out; a device tensor (or a device
        `Uint8Images`) gives device tensors."""
        self._depth_refused("block statistics")
        idx = resolve_taps(range(self.cfg.depth) if blocks is None else blocks, self.cfg.depth)
        return self._block_outputs(
            img, "stats", idx, lambda b, i: (b, len(SUBLAYERS), _lib.DEPTH_STATS),
            lambda x, t, **kw: self.block_stats_into(x, blocks=idx, stat_tensors=t, **kw),
            logits=logits, pooled=pooled)

    # -- skips ----------------------------------------------------------------------------------
    def _send_skips(self, mask: Optional[List[int]]) -> None:
        arr = (ctypes.c_uint8 * len(mask))(*mask) if mask else None
        with torch.cuda.device(self.device):
            self._einval(lambda: _lib.check(_lib.load_library().evt_model_set_skips(
                self._ptr(), arr, len(mask) if mask else 0, self._stream())))

    def _set_skip_mask(self, mask: Optional[List[int]]) -> None:
        mask = mask if mask and any(mask) else None
        if getattr(self, "_handle", None):
            self._send_skips(mask)  # a refusal leaves the mirror's mask as it was
        self._skip_mask = mask

    def skip_sublayers(self, skips: Optional[Mapping[int, str]]) -> None:
        """`{block: "attn" | "ffn" | "block"}`: the mask becomes exactly this (None or {}: no
        skips)."""
        if not skips and self._skip_mask is None:
            return
        self._depth_refused("sublayer skipping")
        self._set_skip_mask(checked_skips(self.cfg.depth, skips))

    def skipped(self) -> Dict[int, str]:
        """`{block: "attn" | "ffn" | "block"}` of the current mask ({}: none). Host only."""
        return mask_to_skips(self._skip_mask or [])

    def clear_skips(self) -> None:
        self.skip_sublayers(None)

    @contextlib.contextmanager
    def skipping(self, skips: Optional[Mapping[int, str]]):
        """Set the given skips for the body of the `with`; on exit, also on an exception, the mask
        is the one from before."""
        before = list(self._skip_mask) if self._skip_mask else None
        try:
            self.skip_sublayers(skips)
            yield self
        finally:
            if (self._skip_mask or None) != before:
                self._set_skip_mask(before)

    def _build(self, max_batch: int) -> None:
        super()._build(max_batch)
        if self._skip_mask:  # a rebuilt handle starts without skips
            self._send_skips(self._skip_mask)

    # -- what a skip refuses, with the library's message -----------------------------------------
    def _skip_refused(self, fn, *args, **kw):
        try:
            return fn(*args, **kw)
        except _lib.EvtError as e:
            if self._skip_mask and e.code == _lib.EVT_EINVAL and "skipped" in str(e):
                raise ValueError(str(e)) from e
            raise

    def attention_maps_into(self, *a, **kw):
        return self._skip_refused(super().attention_maps_into, *a, **kw)

    def head_stats_into(self, *a, **kw):
        return self._skip_refused(super().head_stats_into, *a, **kw)

    def attention_rollout_into(self, *a, **kw):
        return self._skip_refused(super().attention_rollout_into, *a, **kw)

    def ffn_stats_into(self, *a, **kw):
        return self._skip_refused(super().ffn_stats_into, *a, **kw)

    def activation_grams_into(self, *a, **kw):
        return self._skip_refused(super().activation_grams_into, *a, **kw)


def collect_block_stats(model, loader) -> List[np.ndarray]:
    """Dataset means of `model.block_stats` over `loader` (batches of images, or (images, labels)
    pairs): one fp64 [2, 4] array per block, every image weighted equally."""
    sums: Optional[List[np.ndarray]] = None
    n = 0
    for batch in loader:
        img = batch[0] if isinstance(batch, (tuple, list)) else batch
        stats = model.block_stats(img)["stats"]
        stats = [s.double().cpu().numpy() if isinstance(s, torch.Tensor) else
                 np.asarray(s, dtype=np.float64) for s in stats]
        if sums is None:
            sums = [np.zeros(s.shape[1:], dtype=np.float64) for s in stats]
        for acc, s in zip(sums, stats):
            acc += s.sum(0)
        n += stats[0].shape[0]
    if not n:
        raise ValueError("collect_block_stats: the loader gave no images")
    return [s / n for s in sums]
