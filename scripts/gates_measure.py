"""Structured gates (include/evt_gates.h) on one MI355X, DeiT-base in bf16:

  * the gate kernel on its own (evt_gate_weights, HIP events per launch) at the out-projection
    shape [768][768] and the FC2 shape [768][3072], with the bandwidth it reaches (the pristine
    weight read once, the weight written once, the gate vector read once);
  * one head-gate set and one FFN-gate set through the model (`set_head_gates` / `set_ffn_gates` of
    one block, a host clock around the call and a synchronise): the first set of a role, which
    allocates and fills its pristine copy, apart from the later ones;
  * the whole forward at 512 images on ONE handle: ungated, all-ones gates written by the kernel,
    and binary gates (every second head and every second FFN neuron of every block off), the three
    alternated within every round; the forward runs the same kernels on the same shapes in all
    three, so the ratios say whether a gate costs anything after it is set;
  * a one-block head-ablation sweep at 64 images (`head_ablation(blocks=(6,))`: the base pass and
    one pass per head, 13 passes), in images per second, the gate sets included;
  * with --parent-lib: bench.py's default line with this tree's library and with the library of
    the parent commit (EVT_LIB), alternated, each run a process of its own.

    python scripts/gates_measure.py [--out profiles/gates_measure.json]
                                    [--parent-lib /path/to/parent/libevt_hip.so]

Recorded, not gated. Every step runs under its own time limit, an alarm with the default action: a
step that overruns it, hung in a device wait included, ends the process there and nothing further
is started on the GPU. Medians and min-max over REPS launches or ROUNDS alternated rounds after
warm-up. The values are random (they do not change the work).
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
from edgevisiontransformer_amd.evaluate import head_ablation  # noqa: E402
from edgevisiontransformer_amd.modeling.models import vit as vitmod  # noqa: E402

WARMUP, REPS, ROUNDS, CALLS = 5, 30, 15, 3
SHAPES = {"out_proj": (768, 768), "fc2": (768, 3072)}  # (rows, kpad) of DeiT-base


def spread(v, digits=1):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits),
            "max": round(max(v), digits)}


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
    return t


def kernel(dev):
    lib = _lib.load_library()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {}
    for name, (rows, kpad) in SHAPES.items():
        w0 = torch.randn((rows, kpad), device=dev).to(torch.bfloat16)
        w = torch.empty_like(w0)
        g = torch.rand((kpad,), device=dev)
        us = event_us(lambda: _lib.check(lib.evt_gate_weights(1, p(w0), p(w), p(g), rows, kpad,
                                                             stream)))
        nbytes = 2 * rows * kpad * 2 + kpad * 4
        res[name] = {"rows": rows, "kpad": kpad, "bytes": nbytes, "us": spread(us, 2),
                     "tbytes_per_s": round(nbytes / statistics.median(us) / 1e6, 3)}
    return res


def sets(dev):
    m = vitmod.get_deit_base(dtype="bf16", max_batch=1)
    rng = np.random.default_rng(0)
    res = {}
    for role, n, fn in (("head", 12, m.set_head_gates), ("ffn", 3072, m.set_ffn_gates)):
        ms = []
        for i in range(1 + WARMUP + REPS):
            g = rng.random(n).astype(np.float32)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn({6: g})
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        res[role] = {"first_set_ms": round(ms[0], 3), "set_ms": spread(ms[1 + WARMUP:], 4)}
    m.close()
    return res


def forward(batch, dev):
    m = vitmod.get_deit_base(dtype="bf16", max_batch=batch)
    img = torch.randn((batch, 3, 224, 224), device=dev)
    logits = torch.empty((batch, m.num_classes), device=dev)
    half_h, half_f = np.arange(12) % 2, np.arange(3072) % 2
    variants = {"ungated": None,
                "all_ones": ({b: np.ones(12) for b in range(12)}, {b: np.ones(3072) for b in range(12)}),
                "binary": ({b: half_h for b in range(12)}, {b: half_f for b in range(12)})}
    m.set_head_gates(variants["binary"][0])  # the pristine copies exist from here on
    m.set_ffn_gates(variants["binary"][1])

    def gate(name):
        if variants[name] is None:
            m.clear_gates()
        else:
            m.set_head_gates(variants[name][0])
            m.set_ffn_gates(variants[name][1])
        torch.cuda.synchronize()

    def run():
        for _ in range(CALLS):
            m.forward_into(img, logits)
        torch.cuda.synchronize()

    for name in variants:
        gate(name)
        for _ in range(WARMUP):
            run()
    ms = {k: [] for k in variants}
    for _ in range(ROUNDS):  # alternated: every round times each variant once
        for k in variants:
            gate(k)
            t0 = time.perf_counter()
            run()
            ms[k].append((time.perf_counter() - t0) * 1e3 / CALLS)
    base = statistics.median(ms["ungated"])
    res = {k: {"ms": spread(v, 3), "images_per_s": round(batch / statistics.median(v) * 1e3, 1),
               "time_over_ungated": round(statistics.median(v) / base, 4)} for k, v in ms.items()}
    m.close()
    return res


def sweep(batch, dev):
    m = vitmod.get_deit_base(dtype="bf16", max_batch=batch)
    loader = [(torch.randn((batch, 3, 224, 224), device=dev),
               torch.randint(0, m.num_classes, (batch,), device=dev))]
    head_ablation(m, loader, blocks=(6,))  # warm-up: the pristine copy of block 6 exists after it
    ms = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = head_ablation(m, loader, blocks=(6,))
        ms.append((time.perf_counter() - t0) * 1e3)
    passes = 1 + len(res["acc1"][0])
    m.close()
    return {"batch": batch, "block": 6, "passes": passes, "sweep_ms": spread(ms, 2),
            "images_per_s": round(passes * batch / statistics.median(ms) * 1e3, 1)}


def bench_ab(parent_lib, rounds, seconds):
    """bench.py's default line, this tree's library and the parent's alternated."""
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "20",
           "--warmup", "5"]
    vals = {"this": [], "parent": []}
    for _ in range(rounds):
        for who in ("parent", "this"):
            env = dict(os.environ)
            if who == "parent":
                env["EVT_LIB"] = parent_lib
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=seconds)
            if r.returncode != 0:  # nothing further on the GPU
                raise SystemExit(f"bench.py ({who}) ended with {r.returncode}:\n{r.stderr[-2000:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            vals[who].append(json.loads(line)["value"])
    res = {k + "_images_per_s": {**spread(v), "runs": [round(x, 1) for x in v]}
           for k, v in vals.items()}
    res["rounds"] = rounds
    res["this_over_parent"] = round(statistics.median(vals["this"]) /
                                    statistics.median(vals["parent"]), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gates_measure.json"))
    ap.add_argument("--step-seconds", type=int, default=150)
    ap.add_argument("--parent-lib", default="", help="libevt_hip.so built from the parent commit")
    ap.add_argument("--bench-rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    _lib.ensure_device(dev.index or 0)
    res = {"dtype": "bf16", "model": "deit_base (reference semantics)", "warmup": WARMUP,
           "reps": REPS, "rounds": ROUNDS, "calls_per_round": CALLS}
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    for name, step in (("kernel", lambda: kernel(dev)), ("model_set", lambda: sets(dev)),
                       ("forward_bs512", lambda: forward(512, dev)),
                       ("ablation_sweep_bs64", lambda: sweep(64, dev))):
        signal.alarm(a.step_seconds)
        res[name] = step()
        signal.alarm(0)
        print(f"{name}: {res[name]}", file=sys.stderr, flush=True)
    if a.parent_lib:
        torch.cuda.empty_cache()
        res["bench_default_line"] = bench_ab(os.path.abspath(a.parent_lib), a.bench_rounds,
                                             a.step_seconds)
    line = json.dumps(res, indent=1)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
