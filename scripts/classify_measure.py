"""The classify kernel (csrc/features.hip, include/evt_classify.h) on one MI355X:

  * the kernel alone (evt_classify on random logits; indices, probabilities and lse, with and
    without labels / rank / counters): us per launch at [64, 1000] and [512, 1000] (DeiT-base's
    logits, k = 5) and at [64, 21841] and [512, 21841] (ImageNet-21k);
  * beside it, in the same process, `torch.topk(torch.softmax(logits, -1), 5)` on the same logits;
  * the whole forward, DeiT-base bf16 at 64 and 512 images: `classify_into` (forward + classify
    with labels and counters) over `forward_into`, and, with --parent-lib (a libevt_hip.so built
    from the parent commit), that library's plain forward, alternating: each measurement is a
    fresh child process, parent / this / parent / this ...

    python scripts/classify_measure.py [--parent-lib PATH] [--out profiles/classify_measure.json]

Recorded, not gated. Every step runs under its own time limit (an alarm with the default action in
this process, a timeout on each child): a step that overruns it ends the run there and nothing
further is started on the GPU. Medians over REPS repetitions after WARMUP warm-up calls.
"""
import argparse
import ctypes
import json
import os
import signal
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from edgevisiontransformer_amd import _lib  # noqa: E402

WARMUP, REPS, ROUNDS = 5, 30, 3
KW = dict(dim=768, depth=12, heads=12, patch_size=16)


def event_us(fn):
    t = []
    for i in range(WARMUP + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= WARMUP:
            t.append(a.elapsed_time(b) * 1e3)
    return statistics.median(t)


def host_ms(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def kernel(batch, classes, dev, k=5):
    lib = _lib.load_library()
    logits = torch.randn((batch, classes), device=dev) * 3
    idx = torch.empty((batch, k), dtype=torch.int32, device=dev)
    val, lse = torch.empty((batch, k), device=dev), torch.empty(batch, device=dev)
    y = torch.randint(0, classes, (batch,), dtype=torch.int32, device=dev)
    rank = torch.empty(batch, dtype=torch.int32, device=dev)
    counters = torch.zeros(3, dtype=torch.int64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    a = _lib.evt_classify_args()
    a.k, a.values = k, _lib.CLASSIFY_PROB
    a.indices, a.vals, a.lse = idx.data_ptr(), val.data_ptr(), lse.data_ptr()
    run = lambda: _lib.check(lib.evt_classify(ctypes.c_void_p(logits.data_ptr()), classes, batch,  # noqa: E731
                                              classes, ctypes.byref(a), stream))
    res = {"topk_probs_lse_us": round(event_us(run), 1)}
    a.labels, a.rank, a.counters = y.data_ptr(), rank.data_ptr(), counters.data_ptr()
    res["with_labels_rank_counters_us"] = round(event_us(run), 1)
    res["torch_softmax_topk_us"] = round(event_us(
        lambda: torch.topk(torch.softmax(logits, -1), k)), 1)
    res["logits_mbytes"] = round(logits.numel() * 4 / 1e6, 2)
    return res


def forward(batch, dev, with_classify):
    """This process's library (EVT_LIB may name another): ms of the plain forward and, when the
    library has it, of forward + classify."""
    from edgevisiontransformer_amd.modeling.models import vit as vitmod
    from edgevisiontransformer_amd.weights import std_vit_param_shapes, vit_config
    cfg = vit_config(KW["dim"], KW["depth"], KW["heads"], 4 * KW["dim"], patch_size=16)
    rng = np.random.default_rng(0)
    params = {n: np.ones(s, np.float32) if n.endswith("_g")
              else rng.standard_normal(s, dtype=np.float32) * np.float32(0.02)
              for n, s in std_vit_param_shapes(cfg)}
    m = vitmod.StandardViT(**KW, dtype="bf16", weights=params, max_batch=batch)
    img = torch.randn((batch, 3, 224, 224), device=dev)
    logits = torch.empty((batch, m.num_classes), device=dev)
    res = {"forward_ms": round(host_ms(lambda: m.forward_into(img, logits)), 4)}
    if with_classify:
        idx = torch.empty((batch, 5), dtype=torch.int32, device=dev)
        val = torch.empty((batch, 5), device=dev)
        y = torch.randint(0, m.num_classes, (batch,), dtype=torch.int32, device=dev)
        counters = torch.zeros(3, dtype=torch.int64, device=dev)
        res["classify_ms"] = round(host_ms(lambda: m.classify_into(
            img, logits=logits, indices=idx, values_out=val, labels=y, counters=counters,
            topk=5)), 4)
    m.close()
    return res


def child(batch, lib_path, seconds):
    """One forward measurement in a fresh process (its own library)."""
    env = dict(os.environ)
    if lib_path:
        env["EVT_LIB"] = lib_path
    else:
        env.pop("EVT_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(batch)]
    if not lib_path:
        cmd.append("--with-classify")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=seconds)
    if r.returncode != 0:
        sys.exit(f"child failed ({r.returncode}); nothing further is started:\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "classify_measure.json"))
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--step-seconds", type=int, default=150)
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--with-classify", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    _lib.ensure_device(dev.index or 0)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    if a.child:
        signal.alarm(a.step_seconds)
        print(json.dumps(forward(a.child, dev, a.with_classify)), flush=True)
        return
    res = {"warmup": WARMUP, "reps": REPS, "k": 5, "kernel": {}, "forward": {}}
    for batch, classes in ((64, 1000), (512, 1000), (64, 21841), (512, 21841)):
        signal.alarm(a.step_seconds)
        res["kernel"][f"bs{batch}_c{classes}"] = r = kernel(batch, classes, dev)
        signal.alarm(0)
        print(f"kernel bs{batch} C{classes}: {r}", file=sys.stderr, flush=True)
    parent = os.path.abspath(a.parent_lib) if a.parent_lib else ""
    for batch in (64, 512):
        rounds = []
        for _ in range(ROUNDS):
            r = {}
            if parent:
                r["parent_forward_ms"] = child(batch, parent, a.step_seconds)["forward_ms"]
            r.update(child(batch, "", a.step_seconds))
            rounds.append(r)
            print(f"forward bs{batch}: {r}", file=sys.stderr, flush=True)
        med = {key: round(statistics.median(x[key] for x in rounds), 4) for key in rounds[0]}
        med["classify_over_forward"] = round(med["classify_ms"] / med["forward_ms"], 4)
        res["forward"][f"bs{batch}"] = {"model": "deit_base_patch16_224 bf16", "rounds": rounds,
                                        "median": med}
    line = json.dumps(res, indent=1)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
