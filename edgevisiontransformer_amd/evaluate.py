"""Accuracy of a model over a dataset: the mirror of the reference's `evaluate_torch(model,
data_loader, device)` (utils.py:785-813: argmax of the logits against the target, correct / total).

    from edgevisiontransformer_amd import evaluate, EvalTransform
    res = evaluate(model, loader, topk=5)                       # fp32 batches or Uint8Images
    res = evaluate(model, loader, transform=EvalTransform(224), log=print)   # decoded uint8 images
    res["acc1"], res["acck"], res["seen"], res["top1"], res["topk"]

`loader` is any iterable of (images, target). The hits are counted on the device (the classify
kernel's int64[3] counters, include/evt_classify.h): the loop enqueues one forward + classify per
batch and reads three integers once at its end; only with `log` does it read them after every
batch, for the reference's progress lines. A target outside [0, num_classes) (-1: unlabelled) is not
counted. The counters are sums, so the results of several ranks or shards add up.
"""
from __future__ import annotations

import contextlib
from datetime import datetime
from typing import Callable, Dict, Iterable, Optional

import numpy as np

from .images import Uint8Images


def _device_batch(model, images, transform):
    """The device-resident batch `classify_into` takes, of one loader item."""
    import torch
    if transform is not None and not isinstance(images, (Uint8Images, torch.Tensor, np.ndarray)):
        images = transform(images, model.device)  # a list of decoded uint8 HWC images
    x, _ = model._checked_image(images)
    return x


def _device_labels(target, batch: int, device):
    import torch
    y = target if isinstance(target, torch.Tensor) else torch.as_tensor(np.asarray(target))
    y = y.reshape(-1)
    if y.shape[0] != batch or y.dtype.is_floating_point or y.dtype == torch.bool:
        raise ValueError(f"target must be {batch} integers, one per image")
    return y.to(device=device, dtype=torch.int32).contiguous()


def evaluate(model, loader: Iterable, topk: int = 5, transform=None,
             log: Optional[Callable[[str], None]] = None) -> Dict[str, float]:
    """Top-1 and top-`topk` accuracy of `model` over `loader`, an iterable of (images, target):
    images an fp32 batch in the model's layout, a `Uint8Images` or, with `transform=
    EvalTransform(...)`, a list of decoded uint8 HWC arrays; target [B] integers. Returns {"seen",
    "top1", "topk"} (integers) and {"acc1" = top1 / seen, "acck"}; "acc1" is what the reference's
    evaluate_torch returns. `log` (e.g. print) gets the reference's progress line per batch and
    its summary line."""
    import torch
    device = model.device
    on_device = torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext()
    counters = torch.zeros(3, dtype=torch.int64, device=device)
    logits = None
    before = (0, 0, 0)
    for images, target in loader:
        x = _device_batch(model, images, transform)
        b = x.shape[0]
        y = _device_labels(target, b, device)
        if logits is None or logits.shape[0] < b:  # one buffer for the loop; a short last batch
            logits = torch.empty((b, model.cfg.num_classes), dtype=torch.float32, device=device)
        with on_device:
            model.classify_into(x, logits=logits[:b], labels=y, counters=counters, topk=topk)
        if log is not None:
            now = tuple(int(v) for v in counters.cpu())
            n, hit = now[0] - before[0], now[1] - before[1]
            cur = hit / n * 100 if n else 0.0
            log(f'[{datetime.now().strftime("D%m%d %H:%M:%S")} {now[0]: 5d}]  '
                f'Cur Accuracy: {cur: .2f}% Total Accuracy: {_ratio(now[1], now[0]) * 100: .2f}%')
            before = now
    seen, top1, topn = (int(v) for v in counters.cpu())
    res = {"seen": seen, "top1": top1, "topk": topn, "acc1": _ratio(top1, seen),
           "acck": _ratio(topn, seen)}
    if log is not None:
        log(f'Summary model accuracy is {res["acc1"] * 100: .2f}%')
    return res


def _ratio(a: int, b: int) -> float:
    return a / b if b else 0.0


def head_ablation(model, loader: Iterable, topk: int = 5, transform=None, blocks=None,
                  log: Optional[Callable[[str], None]] = None) -> Dict[str, object]:
    """The head-ablation sweep of the reference's `are_16_heads/heads_ablation.sh` (`--attention_
    mask_heads layer:head` over every head) on the loaded model: {"base": `evaluate`'s result with
    the model's current gates, "acc1": [[top-1 accuracy with head h of block l masked] per head]
    per block, "acck": the same for top-`topk`, "blocks": the block indices of the rows}.
    `blocks=None` sweeps every block (negative indices and any order as `head_stats`); a pruned
    model's rows have its per-block head counts.

    One head at a time is gated to 0 on top of the gates the model already has (`mask_heads`
    semantics on that one head: modeling/models/gates.py), and the whole loader is counted by
    `evaluate` on the device. `loader` is re-iterated once per mask and once for the base: give a
    list (or anything that can be iterated again), not a one-shot generator; nothing is
    materialised here. The model's gates are back as they were at the end, also on an exception.
    `log` gets one line per mask."""
    from .modeling.models.features import resolve_taps
    nb = model.num_blocks
    idx = resolve_taps(range(nb) if blocks is None else blocks, nb)
    res: Dict[str, object] = {"base": evaluate(model, loader, topk=topk, transform=transform),
                              "acc1": [], "acck": [], "blocks": list(idx)}
    for l in idx:
        mine = model.head_gates()[l]
        row1, rowk = [], []
        for h in range(mine.shape[0]):
            g = mine.copy()
            g[h] = 0.0
            with model.gated(heads={l: g}):
                r = evaluate(model, loader, topk=topk, transform=transform)
            if r["seen"] != res["base"]["seen"]:
                raise ValueError("head_ablation: the loader gave a different number of images on a "
                                 "later pass (it must be re-iterable)")
            row1.append(r["acc1"])
            rowk.append(r["acck"])
            if log is not None:
                log(f"head_ablation block {l} head {h}: acc1 {r['acc1'] * 100:.2f}% "
                    f"(base {res['base']['acc1'] * 100:.2f}%)")
        res["acc1"].append(row1)
        res["acck"].append(rowk)
    return res


def sublayer_ablation(model, loader: Iterable, topk: int = 5, transform=None, blocks=None,
                      log: Optional[Callable[[str], None]] = None) -> Dict[str, object]:
    """The depth twin of `head_ablation`: {"base": `evaluate`'s result with the model's current
    skips, "acc1": [[top-1 accuracy with the attention sublayer of block l skipped, ... with its
    FFN sublayer skipped] per block], "acck": the same for top-`topk`, "blocks": the block indices
    of the rows}. `blocks=None` sweeps every block (negative indices and any order as
    `block_stats`). A sublayer the model skips already is NaN: there is nothing left to ablate.

    One sublayer at a time is skipped on top of the skips the model already has
    (modeling/models/depth.py: its kernels are not launched), and the whole loader is counted by
    `evaluate` on the device. `loader` is re-iterated once per sublayer and once for the base: give
    a list (or anything that can be iterated again), not a one-shot generator; nothing is
    materialised here. The model's skips are back as they were at the end, also on an exception.
    `log` gets one line per sublayer."""
    from .modeling.models.depth import SKIP_BITS, SKIP_NAMES, SUBLAYERS
    from .modeling.models.features import resolve_taps
    model.block_stats_shape(0)  # a model without a depth axis: ValueError before any pass
    nb = model.num_blocks
    idx = resolve_taps(range(nb) if blocks is None else blocks, nb)
    res: Dict[str, object] = {"base": evaluate(model, loader, topk=topk, transform=transform),
                              "acc1": [], "acck": [], "blocks": list(idx)}
    for l in idx:
        row1, rowk = [], []
        for sub in SUBLAYERS:
            mine = model.skipped()
            have = SKIP_BITS.get(mine.get(l, ""), 0)
            if have & SKIP_BITS[sub]:
                row1.append(float("nan"))
                rowk.append(float("nan"))
                continue
            with model.skipping({**mine, l: SKIP_NAMES[have | SKIP_BITS[sub]]}):
                r = evaluate(model, loader, topk=topk, transform=transform)
            if r["seen"] != res["base"]["seen"]:
                raise ValueError("sublayer_ablation: the loader gave a different number of images "
                                 "on a later pass (it must be re-iterable)")
            row1.append(r["acc1"])
            rowk.append(r["acck"])
            if log is not None:
                log(f"sublayer_ablation block {l} {sub}: acc1 {r['acc1'] * 100:.2f}% "
                    f"(base {res['base']['acc1'] * 100:.2f}%)")
        res["acc1"].append(row1)
        res["acck"].append(rowk)
    return res


def collect_head_stats(model, loader: Iterable, transform=None, blocks=None):
    """Dataset means of the per-head attention statistics (modeling/models/head_stats.py): one
    fp64 [H_i, 4] array per block (`blocks=None`: every block; negative indices and any order as
    `head_stats`), columns in HEAD_STATS order (confidence, entropy, distance, cls_mass).

    `loader` yields what `evaluate` takes: (images, target) tuples, of which the target is not
    read, or the images alone. Each batch's [B, H_i, 4] is summed over its images (a torch sum
    over the batch axis) into a per-block fp64 device tensor that lives for the whole loop; the
    host reads once, at the end. Every image weighs the same, whatever its batch's size."""
    import torch

    from .modeling.models.features import resolve_taps
    device = model.device
    on_device = torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext()
    nb = model.num_blocks
    idx = resolve_taps(range(nb) if blocks is None else blocks, nb)
    heads = [model.head_stats_shape(i)[0] for i in idx]
    sums = [torch.zeros((h, 4), dtype=torch.float64, device=device) for h in heads]
    bufs, seen = None, 0
    for item in loader:
        images = item[0] if isinstance(item, tuple) else item
        x = _device_batch(model, images, transform)
        b = x.shape[0]
        if bufs is None or bufs[0].shape[0] < b:  # one set of buffers for the loop
            bufs = [torch.empty((b, h, 4), dtype=torch.float32, device=device) for h in heads]
        views = [t[:b] for t in bufs]
        with on_device:
            model.head_stats_into(x, blocks=idx, stat_tensors=views)
            for s, v in zip(sums, views):
                s += v.sum(dim=0, dtype=torch.float64)
        seen += b
    if not seen:
        raise ValueError("collect_head_stats: the loader gave no images")
    return [(s / seen).cpu().numpy() for s in sums]


def collect_ffn_stats(model, loader: Iterable, transform=None, blocks=None):
    """Dataset statistics of the FFN neurons (modeling/models/ffn_stats.py): one fp64 [F_i, 4]
    array per block (`blocks=None`: every block; negative indices and any order as `ffn_stats`),
    columns in FFN_STATS order. mean, mean_abs and mean_sq are the means over the dataset's images
    of the per-image values (every image has the same number of tokens, so they are the means over
    all tokens of the dataset); max_abs is the maximum over the dataset.

    `loader` yields what `evaluate` takes: (images, target) tuples, of which the target is not
    read, or the images alone. Each batch's [B, F_i, 4] is reduced over its images on the device
    (an fp64 sum of columns 0-2, a maximum of column 3) into per-block fp64 device tensors that
    live for the whole loop; the host reads once, at the end. Every image weighs the same, whatever
    its batch's size."""
    import torch

    from .modeling.models.features import resolve_taps
    device = model.device
    on_device = torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext()
    nb = model.num_blocks
    idx = resolve_taps(range(nb) if blocks is None else blocks, nb)
    widths = [model.ffn_stats_shape(i)[0] for i in idx]
    sums = [torch.zeros((f, 3), dtype=torch.float64, device=device) for f in widths]
    tops = [torch.zeros((f,), dtype=torch.float64, device=device) for f in widths]
    bufs, seen = None, 0
    for item in loader:
        images = item[0] if isinstance(item, tuple) else item
        x = _device_batch(model, images, transform)
        b = x.shape[0]
        if bufs is None or bufs[0].shape[0] < b:  # one set of buffers for the loop
            bufs = [torch.empty((b, f, 4), dtype=torch.float32, device=device) for f in widths]
        views = [t[:b] for t in bufs]
        with on_device:
            model.ffn_stats_into(x, blocks=idx, stat_tensors=views)
            for s, top, v in zip(sums, tops, views):
                s += v[:, :, :3].sum(dim=0, dtype=torch.float64)
                torch.maximum(top, v[:, :, 3].amax(dim=0).double(), out=top)
        seen += b
    if not seen:
        raise ValueError("collect_ffn_stats: the loader gave no images")
    return [torch.cat([s / seen, top[:, None]], dim=1).cpu().numpy() for s, top in zip(sums, tops)]


def collect_grams(model, loader: Iterable, what="ffn", blocks=None, transform=None):
    """Dataset Grams of the activations a pruned layer's consumer reads (modeling/models/grams.py):
    {"gram": [one fp64 [F_i, F_i] per block], "sum": [one fp64 [F_i] per block], "rows": the token
    rows seen}, numpy, for `pruning.reconstruct_vit_params`. `what`: "ffn" (the FC1 output, for
    FC2) or "attn" (the attention context, for the out-projection); `blocks=None`: every block
    (negative indices and any order as `activation_grams`).

    `loader` yields what `evaluate` takes: (images, target) tuples, of which the target is not
    read, or the images alone. Each batch's fp32 Gram and column sums are added into per-block
    fp64 device tensors that live for the whole loop, as do the fp32 buffers of a call; the host
    reads once, at the end. Every token row weighs the same, whatever its batch's size."""
    import torch

    from .modeling.models.features import resolve_taps
    device = model.device
    on_device = torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext()
    nb = model.num_blocks
    idx = resolve_taps(range(nb) if blocks is None else blocks, nb)
    geo = [model.gram_shape(i, what) for i in idx]
    grams = [torch.zeros((f, f), dtype=torch.float64, device=device) for f, _ in geo]
    sums = [torch.zeros((f,), dtype=torch.float64, device=device) for f, _ in geo]
    gbuf = [torch.empty((f, f), dtype=torch.float32, device=device) for f, _ in geo]
    sbuf = [torch.empty((f,), dtype=torch.float32, device=device) for f, _ in geo]
    rows = 0
    for item in loader:
        images = item[0] if isinstance(item, tuple) else item
        x = _device_batch(model, images, transform)
        with on_device:
            model.activation_grams_into(x, blocks=idx, what=what, gram_tensors=gbuf,
                                        sum_tensors=sbuf)
            for g, s, gb, sb in zip(grams, sums, gbuf, sbuf):
                g += gb
                s += sb
        rows += x.shape[0] * geo[0][1] if geo else 0
    if not rows:
        raise ValueError("collect_grams: the loader gave no images (or no block was asked for)")
    return {"gram": [g.cpu().numpy() for g in grams], "sum": [s.cpu().numpy() for s in sums],
            "rows": rows}
