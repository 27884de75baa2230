"""Token pruning of the ViT mirrors: the binding of include/evt_token_pruning.h.

    model = get_deit_base(dtype="bf16", token_keep={3: 0.7, 6: 0.7, 9: 0.7})
    logits = model(img)                                   # 197 -> 139 -> 98 -> 69 tokens per image
    model.set_token_pruning({3: 100, 6: 0.5})             # counts or rates; None / {} clears
    model.token_schedule()                                # [(block, K, T_in, T_out), ...]
    out = model.token_pruning_outputs(img)                # scores, kept, token_index, logits

After a scheduled block the stream keeps the CLS token and the K patch tokens the CLS token attends
to most (the head sum of the CLS row of the block's attention, EViT's score); later blocks, the CLS
tail and the head run on 1 + K tokens per image. A rate in (0, 1] means K = ceil(rate * (T - 1)) of
the block's T - 1 patch tokens, EViT's rule. The selection is `select_tokens_reference`: the stable
top-K (`np.argsort(-s, kind="stable")`), returned ascending so raster order is preserved. Nothing
changes for a model without a schedule.

With a schedule the logits forwards (`model(img)`, `forward_into`, `classify`, graph capture,
`forward_features`) run the scheduled forward; what reads every token of a block
(`attention_maps`, `head_stats`, `attention_rollout`, `ffn_stats`, `features(tokens=True / taps=)`)
raises ValueError until the schedule is cleared. ViT, ViT_Pruned and StandardViT in "f32" and "bf16"
have it; T2T_ViT, SwinTransformer and "mx8" models raise ValueError.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from ... import _lib
from .classify import Classification
from .features import outputs_to_numpy

Keep = Union[int, float]


def select_tokens_reference(scores, keep: int) -> np.ndarray:
    """The selection contract in numpy: `scores` [..., T] (entry 0 is the CLS token's) ->
    int32 [..., 1 + keep]: 0, then the `keep` patch tokens j >= 1 that come first in
    `np.argsort(-s, kind="stable")` (larger first; ties, and -0.0 against +0.0, to the lower index;
    NaN last), in ascending order."""
    s = np.asarray(scores)
    t = s.shape[-1]
    if not 1 <= keep <= t - 1:
        raise ValueError(f"keep must be in [1, {t - 1}], got {keep}")
    flat = s.reshape(-1, t)
    out = np.zeros((flat.shape[0], keep + 1), dtype=np.int32)
    for r, row in enumerate(flat):
        order = np.argsort(-row[1:], kind="stable")[:keep] + 1
        out[r, 1:] = np.sort(order)
    return out.reshape(*s.shape[:-1], keep + 1)


def _resolve_keep(keep: Keep, patches: int) -> int:
    if isinstance(keep, bool) or not isinstance(keep, (int, float, np.integer, np.floating)):
        raise ValueError(f"keep must be an int (a count) or a float in (0, 1] (a rate), got {keep!r}")
    if isinstance(keep, (float, np.floating)):
        if not 0.0 < keep <= 1.0:
            raise ValueError(f"a keep rate must be in (0, 1], got {keep}")
        return max(1, int(math.ceil(float(keep) * patches - 1e-9)))  # 0.1 * 30 is 3, not 4
    return int(keep)


def schedule_tokens(tokens: int, depth: int,
                    schedule: Optional[Mapping[int, Keep]]) -> List[Tuple[int, int, int, int]]:
    """[(block, K, T_in, T_out)] of a `{block: keep}` schedule on a model of `tokens` tokens per
    image and `depth` blocks, rates resolved (K = ceil(rate * (T_in - 1))), blocks ascending. The
    ValueErrors mirror evt_model_set_token_schedule: a block outside [0, depth - 1), a K outside
    [1, T_in - 1], more than 64 entries."""
    out: List[Tuple[int, int, int, int]] = []
    t = int(tokens)
    items = sorted((schedule or {}).items(), key=lambda kv: kv[0])
    if len(items) > _lib.TOKEN_SCHEDULE_MAX:
        raise ValueError(f"at most {_lib.TOKEN_SCHEDULE_MAX} scheduled blocks")
    for block, keep in items:
        if isinstance(block, bool) or not isinstance(block, (int, np.integer)):
            raise ValueError(f"schedule blocks must be integers, got {block!r}")
        if not 0 <= block < depth - 1:
            raise ValueError(f"block {block} is outside [0, depth - 1 = {depth - 1}): the last "
                             "block's output is the CLS token's alone")
        k = _resolve_keep(keep, t - 1)
        if not 1 <= k <= t - 1:
            raise ValueError(f"keep {k} after block {block} is outside [1, {t - 1}], the block's "
                             "patch tokens")
        out.append((int(block), k, t, k + 1))
        t = k + 1
    return out


def tokens_per_block(tokens: int, depth: int, schedule) -> List[int]:
    """T_l for l = 0 .. depth - 1: the tokens per image block l runs on under `schedule`."""
    t, out, sched = int(tokens), [], {b: t_out for b, _, _, t_out in
                                      schedule_tokens(tokens, depth, schedule)}
    for l in range(depth):
        out.append(t)
        t = sched.get(l, t)
    return out


def scheduled_gflop_per_image(cfg, schedule) -> float:
    """`ViTConfig.gflop_per_image` with block l on its T_l tokens (the matmul FLOPs the scheduled
    forward needs; the scores, the selection and the gather are not matmuls)."""
    p, d = cfg.num_patches, cfg.dim
    f = 2.0 * p * cfg.patch_dim * d
    for i, n in enumerate(tokens_per_block(cfg.tokens, cfg.depth, schedule)):
        inner = cfg.heads[i] * cfg.head_dim[i]
        f += 2.0 * n * d * 3 * inner + 2.0 * 2 * n * n * inner + 2.0 * n * inner * d
        f += 2.0 * 2 * n * d * cfg.ffn[i]
    f += 2.0 * d * cfg.mlp_dim + 2.0 * cfg.mlp_dim * cfg.num_classes
    return f / 1e9


def parse_token_keep(spec: Optional[str]) -> Dict[int, Keep]:
    """'3:0.7,6:0.7,9:100' -> {3: 0.7, 6: 0.7, 9: 100} (a value with a '.' is a rate)."""
    out: Dict[int, Keep] = {}
    for part in (spec or "").split(","):
        if not part.strip():
            continue
        try:
            b, k = part.split(":")
            out[int(b)] = float(k) if "." in k else int(k)
        except ValueError:
            raise ValueError(f"token_keep entries are block:keep, got {part!r}") from None
    return out


class TokenPruning(Classification):
    """What ViT, T2T_ViT and SwinTransformer derive from: token schedules on top of everything
    else. A class that supports them sets `_TOKEN_PRUNING_OK`; the others refuse."""

    _TOKEN_PRUNING_OK = False
    _token_keep: Optional[Dict[int, Keep]] = None

    # -- the schedule ---------------------------------------------------------------------------
    def _resolved_schedule(self, schedule) -> List[Tuple[int, int, int, int]]:
        if not schedule:
            return []
        if not self._TOKEN_PRUNING_OK:
            raise ValueError(f"{type(self).__name__} has no token pruning: token schedules are "
                             "ViT's (ViT, ViT_Pruned, StandardViT)")
        if getattr(self, "dtype", None) == "mx8":
            raise ValueError("token pruning is not available on an 'mx8' model")
        return schedule_tokens(self.cfg.tokens, self.cfg.depth, schedule)

    def _apply_token_schedule(self) -> None:
        """Hand the stored schedule to the handle (set_token_pruning, and _build after it has
        recreated the handle)."""
        sched = self._resolved_schedule(self._token_keep)
        n = len(sched)
        blocks = (ctypes.c_int32 * max(1, n))(*[s[0] for s in sched])
        keep = (ctypes.c_int32 * max(1, n))(*[s[1] for s in sched])
        _lib.check(_lib.load_library().evt_model_set_token_schedule(
            self._ptr(), n, blocks, keep, self._stream()))

    def set_token_pruning(self, schedule: Optional[Mapping[int, Keep]]) -> None:
        """Set the schedule `{block: keep}` (keep: an int count, or a float rate in (0, 1]);
        None or {} clears it. It stays with the model across handle rebuilds."""
        self._resolved_schedule(schedule)  # the ValueErrors, before anything changes
        old = self._token_keep
        self._token_keep = dict(schedule) if schedule else None
        if getattr(self, "_handle", None):
            try:
                self._apply_token_schedule()
            except _lib.EvtError as e:
                self._token_keep = old
                raise ValueError(str(e)) from e

    def _build(self, max_batch: int) -> None:
        super()._build(max_batch)
        if self._token_keep:
            self._apply_token_schedule()

    def token_schedule(self) -> List[Tuple[int, int, int, int]]:
        """[(block, K, T_in, T_out)] of the current schedule ([]: none). Host only."""
        return self._resolved_schedule(self._token_keep)

    def tokens_at(self, block: int) -> int:
        """Tokens per image block `block` runs on (negative: from the last). Host only."""
        depth = self.cfg.depth
        i = block + depth if block < 0 else block
        if not 0 <= i < depth:
            raise ValueError(f"block {block} is outside the model's {depth} blocks")
        return tokens_per_block(self.cfg.tokens, depth, self._token_keep)[i]

    # -- what reads every token of a block refuses, with the library's message ------------------
    def _refused(self, fn, *args, **kw):
        try:
            return fn(*args, **kw)
        except _lib.EvtError as e:
            if self._token_keep and e.code == _lib.EVT_EINVAL and "token schedule" in str(e):
                raise ValueError(str(e)) from e
            raise

    def features_into(self, *a, **kw):
        return self._refused(super().features_into, *a, **kw)

    def attention_maps_into(self, *a, **kw):
        return self._refused(super().attention_maps_into, *a, **kw)

    def head_stats_into(self, *a, **kw):
        return self._refused(super().head_stats_into, *a, **kw)

    def attention_rollout_into(self, *a, **kw):
        return self._refused(super().attention_rollout_into, *a, **kw)

    def ffn_stats_into(self, *a, **kw):
        return self._refused(super().ffn_stats_into, *a, **kw)

    def activation_grams_into(self, *a, **kw):
        return self._refused(super().activation_grams_into, *a, **kw)

    # -- the scheduled forward with its exports -------------------------------------------------
    def _int32_tensor(self, name: str, t, shape) -> int:
        if t is None:
            return 0
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or not t.is_contiguous() \
                or t.device != self.device or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be a contiguous int32 tensor of shape {tuple(shape)} "
                             f"on {self.device}")
        return t.data_ptr()

    def token_pruning_outputs_into(self, img, *, scores: Sequence[torch.Tensor] = (),
                                   kept: Sequence[torch.Tensor] = (), logits: torch.Tensor = None,
                                   pooled: torch.Tensor = None) -> None:
        """Enqueue the scheduled forward of a device-resident batch (fp32 in the model's layout, or
        a `Uint8Images`) into `logits` [B, num_classes] / `pooled` [B, F] and, per scheduled block
        in schedule order, `scores[i]` fp32 [B, T_in] and `kept[i]` int32 [B, 1 + K] (either list
        may be empty, an entry None); no allocation, no synchronisation
        (evt_forward_token_pruning)."""
        sched = self.token_schedule()
        if not sched:
            raise ValueError("the model has no token schedule (set_token_pruning first)")
        n, b = len(sched), img.shape[0]
        for name, seq in (("scores", scores), ("kept", kept)):
            if len(seq) not in (0, n):
                raise ValueError(f"{name} needs one tensor per scheduled block ({n}) or none")
        a = _lib.evt_token_pruning_args()
        a.n_blocks = n
        sp = (ctypes.c_void_p * n)(*[self._feature_tensor(f"scores[{i}]", t, (b, sched[i][2]))
                                     for i, t in enumerate(scores)] or [None] * n)
        kp = (ctypes.c_void_p * n)(*[self._int32_tensor(f"kept[{i}]", t, (b, sched[i][3]))
                                     for i, t in enumerate(kept)] or [None] * n)
        a.scores, a.kept = sp, kp
        feat = self._feat_args(b, logits=logits, pooled=pooled)
        if not feat[1]:
            raise ValueError("no output requested: logits and pooled are None")
        self._analysis_forward("evt_forward_token_pruning", img, feat, a)

    def token_pruning_outputs(self, img, logits: bool = True, pooled: bool = False) -> Dict[str, object]:
        """{"scores": [fp32 [B, T_in] per scheduled block], "kept": [int32 [B, 1 + K] per block],
        "token_index": int64 [B, T_final], the original token id of every surviving row} plus the
        requested "logits" / "pooled". numpy in, numpy out; a device tensor (or a device
        `Uint8Images`) gives device tensors."""
        sched = self.token_schedule()
        if not sched:
            raise ValueError("the model has no token schedule (set_token_pruning first)")
        if not (logits or pooled):
            raise ValueError("no output requested: logits and pooled are False")
        x, was_numpy = self._checked_image(img)
        b = x.shape[0]
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)  # noqa: E731
        out: Dict[str, object] = {
            "scores": [new((b, s[2]), torch.float32) for s in sched],
            "kept": [new((b, s[3]), torch.int32) for s in sched]}
        if logits:
            out["logits"] = new((b, self.num_classes), torch.float32)
        if pooled:
            out["pooled"] = new((b, self.feature_dim), torch.float32)
        with torch.cuda.device(self.device):
            self.token_pruning_outputs_into(x, scores=out["scores"], kept=out["kept"],
                                            logits=out.get("logits"), pooled=out.get("pooled"))
            # the kept tables composed: row r of the final stream is original token index[r]
            index = torch.arange(sched[0][2], device=self.device).expand(b, -1)
            for k in out["kept"]:
                index = torch.gather(index, 1, k.long())
            out["token_index"] = index.contiguous()
        return outputs_to_numpy(out) if was_numpy else out
