"""Structured gates of the ViT mirrors: the binding of include/evt_gates.h.

    model.mask_heads({3: [1, 5]})                       # the reference's name: heads 1, 5 of block 3 off
    model.set_head_gates({3: xi})                       # real-valued gates, one per head of block 3
    model.mask_ffn({7: dead}); model.set_ffn_gates({7: g})
    with model.gated(heads={-1: g}):                    # the previous gates come back on exit
        acc = evaluate(model, loader)
    model.head_gates(); model.ffn_gates(); model.clear_gates()

A head gate multiplies that head's slice of the attention output before the out-projection, an FFN
gate one column of the hidden activation before FC2. The library applies them to the packed
out-projection / FC2 weights when they are set (one small kernel per block and role); the forward
is the one the model ran before, and a captured graph picks the gates up on its next replay.

The contract is `gates_reference`: a gated model is bitwise a fresh model created from the
parameters it returns. What a block's own gates do not change: `attention_maps`, `head_stats` and
`attention_rollout` of block l do not depend on block l's head gates (they are statistics of the
probabilities the block computed), `ffn_stats` of block l does not depend on block l's FFN gates
(what FC1 stored). Later blocks see the gated stream.

A `{block: ...}` argument sets the blocks it names and leaves the others as they are; negative
blocks count from the last. Gates stay with the model across handle rebuilds. ViT, ViT_Pruned (per
block head / neuron counts) and StandardViT in "f32" and "bf16" have them; T2T_ViT,
SwinTransformer and "mx8" models raise ValueError.
"""
from __future__ import annotations

import contextlib
import ctypes
from typing import Dict, Iterable, List, Mapping, Optional, Sequence

import numpy as np
import torch

from ... import _lib
from .token_pruning import TokenPruning

ROLES = ("head", "ffn")


def bf16_round(a) -> np.ndarray:
    """float32 -> the nearest bf16 value (ties to even), as float32: the rounding the library packs
    a "bf16" model's weights with. Finite input."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


def _block_index(block, depth: int) -> int:
    if isinstance(block, bool) or not isinstance(block, (int, np.integer)):
        raise ValueError(f"gate blocks must be integers, got {block!r}")
    i = int(block) + depth if block < 0 else int(block)
    if not 0 <= i < depth:
        raise ValueError(f"block {block} is outside the model's {depth} blocks")
    return i


def _counts(cfg, role: str) -> List[int]:
    return [int(v) for v in list(cfg.heads if role == "head" else cfg.ffn)[:cfg.depth]]


def checked_gates(cfg, role: str, gates: Optional[Mapping[int, Sequence[float]]]) -> Dict[int, np.ndarray]:
    """`{block: gates}` of `role` ("head" / "ffn") on a model of config `cfg` -> {block index:
    float32 [count]}, validated as evt_model_set_head_gates / _ffn_gates validate: integer blocks
    in [-depth, depth) named once, one finite gate per head / neuron of the block."""
    counts, out = _counts(cfg, role), {}
    what = "heads" if role == "head" else "FFN neurons"
    for block, g in (gates or {}).items():
        i = _block_index(block, cfg.depth)
        if i in out:
            raise ValueError(f"block {i} is named twice")
        a = np.asarray(g, dtype=np.float32)
        if a.ndim != 1 or a.shape[0] != counts[i]:
            raise ValueError(f"block {i} has {counts[i]} {what}, got gates of shape {a.shape}")
        if not np.isfinite(a).all():
            raise ValueError(f"block {i}: gates must be finite (no NaN or infinity)")
        out[i] = np.ascontiguousarray(a)
    return out


def mask_to_gates(cfg, role: str, masked: Optional[Mapping[int, Iterable[int]]]) -> Dict[int, np.ndarray]:
    """`{block: [indices]}` -> binary `{block index: gates}`: 0 at the named heads / neurons, 1
    elsewhere. ValueError: a block or an index out of range."""
    counts, out = _counts(cfg, role), {}
    for block, idx in (masked or {}).items():
        i = _block_index(block, cfg.depth)
        if i in out:
            raise ValueError(f"block {i} is named twice")
        g = np.ones(counts[i], dtype=np.float32)
        for j in idx:
            if isinstance(j, bool) or not isinstance(j, (int, np.integer)) or not 0 <= j < counts[i]:
                raise ValueError(f"block {i}: index {j!r} is outside [0, {counts[i]})")
            g[int(j)] = 0.0
        out[i] = g
    return out


def gates_reference(params: Mapping[str, np.ndarray], cfg, head_gates=None, ffn_gates=None,
                    dtype: str = "f32") -> Dict[str, np.ndarray]:
    """The gated parameter dict of the contract, in numpy: `params` with row h * head_dim + d of
    `l{i}.out_w` multiplied by head_gates[i][h] and row j of `l{i}.fc2_w` by ffn_gates[i][j] (both
    `{block: gates}`, validated as `set_head_gates` does). The product is fp32, of the value the
    loader stores: the fp32 weight for dtype "f32", the bf16-rounded weight for "bf16". A fresh
    model of `dtype` created from the result is bitwise the gated model; the fp64 oracle takes it
    too. Arrays that are not gated are the input's own."""
    if dtype not in ("f32", "bf16"):
        raise ValueError(f'dtype must be "f32" or "bf16", got {dtype!r}')
    out = dict(params)
    hd = [int(v) for v in cfg.head_dim]
    for role, given, key in (("head", head_gates, "out_w"), ("ffn", ffn_gates, "fc2_w")):
        for i, g in checked_gates(cfg, role, given).items():
            w = np.asarray(params[f"l{i}.{key}"], dtype=np.float32)
            rows = np.repeat(g, hd[i]) if role == "head" else g
            if w.ndim != 2 or w.shape[0] != rows.shape[0]:
                raise ValueError(f"l{i}.{key} has shape {w.shape}, the gates cover {rows.shape[0]} rows")
            if dtype == "bf16":
                w = bf16_round(w)
            out[f"l{i}.{key}"] = np.ascontiguousarray(w * rows[:, None], dtype=np.float32)
    return out


def parse_mask_heads(spec: Optional[str]) -> Dict[int, List[int]]:
    """'3:1,3:5,7:0' -> {3: [1, 5], 7: [0]}: the reference's `--attention_mask_heads layer:head`
    list (0-based here, as every block index of this package)."""
    out: Dict[int, List[int]] = {}
    for part in (spec or "").split(","):
        if not part.strip():
            continue
        try:
            b, h = part.split(":")
            out.setdefault(int(b), []).append(int(h))
        except ValueError:
            raise ValueError(f"mask_heads entries are block:head, got {part!r}") from None
    return out


class StructuredGates(TokenPruning):
    """What ViT, T2T_ViT and SwinTransformer derive from: head and FFN gates on top of everything
    else. A class that supports them sets `_GATES_OK`; the others refuse."""

    _GATES_OK = False
    _gates: Optional[Dict[str, Dict[int, np.ndarray]]] = None  # role -> {block index: gates}

    def _gate_state(self) -> Dict[str, Dict[int, np.ndarray]]:
        if self._gates is None:
            self._gates = {r: {} for r in ROLES}
        return self._gates

    def _gates_refused(self) -> None:
        if not self._GATES_OK:
            raise ValueError(f"{type(self).__name__} has no structured gates: head and FFN gates "
                             "are ViT's (ViT, ViT_Pruned, StandardViT)")
        if getattr(self, "dtype", None) == "mx8":
            raise ValueError("structured gates are not available on an 'mx8' model: its "
                             "block-scaled weights would need requantising")

    def _send_gates(self, role: str, block: int, g: np.ndarray) -> None:
        fn = getattr(_lib.load_library(), f"evt_model_set_{role}_gates")
        with torch.cuda.device(self.device):
            try:
                _lib.check(fn(self._ptr(), block, g.ctypes.data_as(_lib._PF), g.shape[0],
                              self._stream()))
            except _lib.EvtError as e:
                if e.code == _lib.EVT_EINVAL:
                    raise ValueError(str(e)) from e
                raise

    def _set_gates(self, role: str, gates: Dict[int, np.ndarray]) -> None:
        state = self._gate_state()[role]
        for i, g in gates.items():
            if getattr(self, "_handle", None):
                self._send_gates(role, i, g)  # a refusal leaves the record of this block as it was
            state[i] = g.copy()

    # -- setting --------------------------------------------------------------------------------
    def set_head_gates(self, gates: Optional[Mapping[int, Sequence[float]]]) -> None:
        """`{block: [one gate per head]}`: any finite floats. The blocks not named keep theirs."""
        if not gates:
            return
        self._gates_refused()
        self._set_gates("head", checked_gates(self.cfg, "head", gates))

    def set_ffn_gates(self, gates: Optional[Mapping[int, Sequence[float]]]) -> None:
        """`{block: [one gate per FFN neuron]}`: any finite floats."""
        if not gates:
            return
        self._gates_refused()
        self._set_gates("ffn", checked_gates(self.cfg, "ffn", gates))

    def mask_heads(self, heads: Optional[Mapping[int, Iterable[int]]]) -> None:
        """`{block: [heads]}` (the reference's `mask_heads(to_prune)`): gate 0 for the named heads
        of each named block, 1 for its others."""
        if not heads:
            return
        self._gates_refused()
        self._set_gates("head", mask_to_gates(self.cfg, "head", heads))

    def mask_ffn(self, neurons: Optional[Mapping[int, Iterable[int]]]) -> None:
        """`{block: [neurons]}`: gate 0 for the named FFN neurons of each named block."""
        if not neurons:
            return
        self._gates_refused()
        self._set_gates("ffn", mask_to_gates(self.cfg, "ffn", neurons))

    def clear_gates(self) -> None:
        """Every gate back to 1; the packed weights are restored bitwise."""
        had = self._gates is not None and any(self._gates[r] for r in ROLES)
        self._gates = None
        if had and getattr(self, "_handle", None):
            with torch.cuda.device(self.device):
                try:
                    _lib.check(_lib.load_library().evt_model_clear_gates(self._ptr(), self._stream()))
                except _lib.EvtError as e:
                    if e.code == _lib.EVT_EINVAL:
                        raise ValueError(str(e)) from e
                    raise

    # -- reading (host only) --------------------------------------------------------------------
    def _read_gates(self, role: str) -> List[np.ndarray]:
        self._gates_refused()
        state = self._gate_state()[role]
        return [state[i].copy() if i in state else np.ones(n, dtype=np.float32)
                for i, n in enumerate(_counts(self.cfg, role))]

    def head_gates(self) -> List[np.ndarray]:
        """One float32 [H_i] array per block (1 where none was set)."""
        return self._read_gates("head")

    def ffn_gates(self) -> List[np.ndarray]:
        """One float32 [F_i] array per block."""
        return self._read_gates("ffn")

    @contextlib.contextmanager
    def gated(self, heads: Optional[Mapping[int, Sequence[float]]] = None,
              ffn: Optional[Mapping[int, Sequence[float]]] = None):
        """Set the given gates for the body of the `with`; on exit, also on an exception, every
        block the body's gates touched (through `heads` / `ffn` or by calls inside the body) is
        back at the gates it had before."""
        before = {r: {i: g.copy() for i, g in self._gate_state()[r].items()} for r in ROLES}
        try:
            self.set_head_gates(heads)
            self.set_ffn_gates(ffn)
            yield self
        finally:
            now = self._gate_state()
            for r in ROLES:
                counts = _counts(self.cfg, r)
                back = {i: before[r].get(i, np.ones(counts[i], dtype=np.float32))
                        for i, g in now[r].items()
                        if i not in before[r] or not np.array_equal(g, before[r][i])}
                back.update({i: g for i, g in before[r].items() if i not in now[r]})
                self._set_gates(r, back)
                now[r].clear()
                now[r].update(before[r])

    def _build(self, max_batch: int) -> None:
        super()._build(max_batch)
        for r in ROLES:  # a rebuilt handle starts ungated
            for i, g in (self._gates or {}).get(r, {}).items():
                if (g != 1.0).any():
                    self._send_gates(r, i, g)
