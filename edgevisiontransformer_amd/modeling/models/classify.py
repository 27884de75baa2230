"""Classification outputs of the model mirrors: the binding of include/evt_classify.h.

    out = model.classify(img, topk=5)                  # {"indices": [B, 5] int32, "values": [B, 5]
    out["indices"][:, 0]                               #  fp32 probabilities, "lse": [B]}; argmax
    out = model.classify(img, topk=5, labels=y, logits=True)    # + "rank" [B] int32, "logits"
    model.classify_into(img, logits=l, indices=i, labels=y, counters=c, topk=5)   # no allocation
    model.classify_logits(l, topk=5, values="logit")   # the kernel alone, e.g. after replay_graph()
    classify_reference(l, 5, labels=y)                 # the contract in numpy fp64 (no device)

One kernel after the forward turns the logits into the ordered top-k classes (l_i > l_j first, ties
and -0.0 / +0.0 by the lower index, NaN last: numpy's argsort(-l, kind="stable"), whose first
element is argmax), their softmax probabilities (or the logits themselves), the log-sum-exp and,
with labels, each label's rank (0 = top-1; a label outside [0, C), e.g. -1, gives -1 and is not
counted) and three device counters `int64[3] += (valid labels, top-1 hits, top-k hits)`, so a loop
over a dataset reads three integers at its end (evaluate.py). Every family and dtype has it.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from ... import _lib
from .features import outputs_to_numpy
from .grams import ActivationGrams

VALUES = {"prob": _lib.CLASSIFY_PROB, "logit": _lib.CLASSIFY_LOGIT}
MAX_CLASSES = 1 << 20


def resolve_values(values) -> int:
    """EVT_CLASSIFY_PROB / EVT_CLASSIFY_LOGIT of a `values=` argument ("prob" / "logit" or the
    constant)."""
    if isinstance(values, str) and values in VALUES:
        return VALUES[values]
    if not isinstance(values, (str, bool)) and values in (_lib.CLASSIFY_PROB, _lib.CLASSIFY_LOGIT):
        return int(values)
    raise ValueError(f"values must be 'prob' or 'logit', got {values!r}")


def resolve_topk(topk, num_classes: int) -> int:
    """k of a `topk=` argument: an integer in [1, min(num_classes, 32)]."""
    kmax = min(int(num_classes), _lib.CLASSIFY_MAX_K)
    if isinstance(topk, bool) or not isinstance(topk, (int, np.integer)) or not 1 <= topk <= kmax:
        raise ValueError(f"topk must be an integer in [1, min(num_classes, "
                         f"{_lib.CLASSIFY_MAX_K}) = {kmax}], got {topk!r}")
    return int(topk)


def classify_reference(logits, k: int, labels=None) -> Dict[str, np.ndarray]:
    """The contract of include/evt_classify.h on the host, in numpy fp64: of `logits` [B, C] (read
    as the fp32 values they are) {"indices" [B, k] int32, "logit" [B, k] fp32 (bitwise copies),
    "prob" [B, k] fp64, "lse" [B] fp64} and, with `labels` [B], {"rank" [B] int32, "counters"
    int64[3] = (valid labels, rank < 1, rank < k)}. The oracle of the tests; works without a
    device."""
    l32 = np.ascontiguousarray(np.asarray(logits, dtype=np.float32))
    if l32.ndim != 2 or l32.shape[0] < 1 or not 1 <= l32.shape[1] <= MAX_CLASSES:
        raise ValueError("logits must be [B >= 1, 1 <= C <= 2^20]")
    b, c = l32.shape
    k = resolve_topk(k, c)
    l64 = l32.astype(np.float64)
    # -l: descending values, -0.0 == +0.0, NaN last; stable: ties by the lower index
    order = np.argsort(-l64, axis=1, kind="stable")
    idx = order[:, :k]
    with np.errstate(all="ignore"):
        m = np.max(l64, axis=1, keepdims=True)
        e = np.exp(l64 - m)
        s = e.sum(axis=1, keepdims=True)
        out = {"indices": idx.astype(np.int32), "logit": np.take_along_axis(l32, idx, axis=1),
               "prob": np.take_along_axis(e, idx, axis=1) / s, "lse": (m + np.log(s))[:, 0]}
    if labels is not None:
        y = np.asarray(labels).astype(np.int64).reshape(-1)
        if y.shape[0] != b:
            raise ValueError("labels must hold one label per row")
        valid = (y >= 0) & (y < c)
        pos = np.empty_like(order)
        np.put_along_axis(pos, order, np.broadcast_to(np.arange(c), (b, c)), axis=1)
        rank = np.where(valid, pos[np.arange(b), np.where(valid, y, 0)], -1).astype(np.int32)
        out["rank"] = rank
        out["counters"] = np.array([valid.sum(), (valid & (rank < 1)).sum(),
                                    (valid & (rank < k)).sum()], dtype=np.int64)
    return out


class Classification(ActivationGrams):
    """What ViT, T2T_ViT and SwinTransformer derive from: the classification outputs on top of the
    FFN statistics, attention rollout, head statistics, attention maps and feature outputs. Needs nothing of the
    model class but `cfg.num_classes`."""

    def _int_tensor(self, name: str, t, shape, dtype) -> int:
        if t is None:
            return 0
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() \
                or t.device != self.device or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be a contiguous {str(dtype).replace('torch.', '')} "
                             f"tensor of shape {tuple(shape)} on {self.device}")
        return t.data_ptr()

    def _classify_args(self, b: int, c: int, topk, values, indices, values_out, lse, labels, rank,
                       counters) -> _lib.evt_classify_args:
        """The checked evt_classify_args of a batch of `b` rows of `c` classes (host only)."""
        a = _lib.evt_classify_args()
        a.k, a.values = resolve_topk(topk, c), resolve_values(values)
        a.indices = self._int_tensor("indices", indices, (b, a.k), torch.int32)
        a.vals = self._feature_tensor("values_out", values_out, (b, a.k))
        a.lse = self._feature_tensor("lse", lse, (b,))
        a.labels = self._int_tensor("labels", labels, (b,), torch.int32)
        a.rank = self._int_tensor("rank", rank, (b,), torch.int32)
        a.counters = self._int_tensor("counters", counters, (3,), torch.int64)
        if not (a.indices or a.vals or a.lse or a.rank or a.counters):
            raise ValueError("no output requested: give indices, values_out, lse, rank or counters")
        if (a.rank or a.counters) and not a.labels:
            raise ValueError("rank and counters need labels")
        return a

    def classify_into(self, img, *, logits: torch.Tensor, indices: torch.Tensor = None,
                      values_out: torch.Tensor = None, lse: torch.Tensor = None,
                      labels: torch.Tensor = None, rank: torch.Tensor = None,
                      counters: torch.Tensor = None, topk: int, values="prob") -> None:
        """Enqueue one forward of a device-resident batch (fp32 in the model's layout, or a
        `Uint8Images`) into `logits` [B, num_classes] and the classify kernel on them: `indices`
        [B, topk] int32, `values_out` [B, topk] and `lse` [B] fp32, and with `labels` [B] int32
        `rank` [B] int32 and `counters` int64[3] (added to). No allocation, no synchronisation
        (evt_forward_classify)."""
        b = img.shape[0]
        if logits is None:
            raise ValueError("logits is required: the caller owns the buffer the kernel reads")
        feat = self._feat_args(b, logits=logits)
        a = self._classify_args(b, self.cfg.num_classes, topk, values, indices, values_out, lse,
                                labels, rank, counters)
        self._analysis_forward("evt_forward_classify", img, feat, a)

    def classify_logits(self, logits: torch.Tensor, *, indices: torch.Tensor = None,
                        values_out: torch.Tensor = None, lse: torch.Tensor = None,
                        labels: torch.Tensor = None, rank: torch.Tensor = None,
                        counters: torch.Tensor = None, topk: int, values="prob") -> None:
        """The kernel alone on an existing device logits tensor [B, C] (for example the buffer of
        `capture_graph` after `replay_graph()`), on the current stream (evt_classify)."""
        if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 \
                or logits.dim() != 2 or not logits.is_contiguous() or logits.device != self.device \
                or logits.shape[0] < 1 or not 1 <= logits.shape[1] <= MAX_CLASSES:
            raise ValueError(f"logits must be a contiguous float32 [B, C] tensor on {self.device}")
        b, c = logits.shape
        a = self._classify_args(b, c, topk, values, indices, values_out, lse, labels, rank, counters)
        _lib.check(_lib.load_library().evt_classify(
            ctypes.c_void_p(logits.data_ptr()), c, b, c, ctypes.byref(a), self._stream()))

    def classify(self, img, topk: int = 5, values="prob", labels=None,
                 logits: bool = False) -> Dict[str, object]:
        """{"indices" [B, topk] int32, "values" [B, topk] fp32 (probabilities, or with
        values="logit" the logits), "lse" [B]} plus "rank" [B] int32 with `labels` [B] (any
        integer array or tensor) and "logits" [B, num_classes] on request (bitwise `model(img)`).
        numpy in, numpy out; a device tensor (or a device `Uint8Images`) gives device tensors."""
        k, v = resolve_topk(topk, self.cfg.num_classes), resolve_values(values)
        x, was_numpy = self._checked_image(img)
        b = x.shape[0]
        y: Optional[torch.Tensor] = None
        if labels is not None:
            y = torch.as_tensor(np.asarray(labels) if not isinstance(labels, torch.Tensor)
                                else labels).reshape(-1)
            if y.shape[0] != b or y.dtype.is_floating_point or y.dtype == torch.bool:
                raise ValueError(f"labels must be {b} integers, one per image")
            y = y.to(device=self.device, dtype=torch.int32).contiguous()
        new = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=self.device)  # noqa: E731
        lg = new((b, self.cfg.num_classes))
        out: Dict[str, object] = {"indices": new((b, k), torch.int32), "values": new((b, k)),
                                  "lse": new((b,))}
        if y is not None:
            out["rank"] = new((b,), torch.int32)
        with torch.cuda.device(self.device):
            self.classify_into(x, logits=lg, indices=out["indices"], values_out=out["values"],
                               lse=out["lse"], labels=y, rank=out.get("rank"), topk=k, values=v)
        if logits:
            out["logits"] = lg
        return outputs_to_numpy(out) if was_numpy else out
