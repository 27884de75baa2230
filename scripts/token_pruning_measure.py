"""Token pruning (include/evt_token_pruning.h) on one MI355X, DeiT-base in bf16 at 512 and 64 images:

  * the whole forward to logits, unscheduled against the schedules {3: .7, 6: .7, 9: .7} and
    {3: .5, 6: .5, 9: .5} on the SAME handle (the schedule set and cleared between the timed
    groups), the three alternated within every round; beside each time ratio the matmul-FLOP ratio
    `scheduled_gflop_per_image / gflop_per_image`, so the gap between work saved and time saved
    shows;
  * the three kernels on their own at the first scheduled block's shape (197 tokens, 12 heads of
    64, keep 138): evt_token_scores, evt_token_select, evt_token_gather, HIP events per launch;
  * with --parent-lib: bench.py's default line with this tree's library and with the library of
    the parent commit (EVT_LIB), alternated, each run a process of its own.

    python scripts/token_pruning_measure.py [--out profiles/token_pruning_measure.json]
                                            [--parent-lib /path/to/parent/libevt_hip.so]

Recorded, not gated, with one condition the script reports as `scheduled_faster_at_512`: the 0.7
schedule at 512 images must be faster than the unscheduled forward of the same run. Every step runs
under its own time limit, an alarm with the default action: a step that overruns it, hung in a
device wait included, ends the process there and nothing further is started on the GPU. Medians
and min-max over REPS launches (HIP events) or ROUNDS alternated rounds (host clock around a
synchronise) after warm-up. The values are random (they do not change the work).
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

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from edgevisiontransformer_amd import _lib  # noqa: E402
from edgevisiontransformer_amd.modeling.models import vit as vitmod  # noqa: E402
from edgevisiontransformer_amd.modeling.models.token_pruning import (  # noqa: E402
    schedule_tokens, scheduled_gflop_per_image)

WARMUP, REPS, ROUNDS, CALLS = 5, 30, 15, 3
T, H, HD, D, KEEP = 197, 12, 64, 768, 138
SCHEDULES = {"keep_0.7": {3: 0.7, 6: 0.7, 9: 0.7}, "keep_0.5": {3: 0.5, 6: 0.5, 9: 0.5}}


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


def kernels(batch, dev):
    lib = _lib.load_library()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    qkv = torch.randn((batch * T, 3 * H * HD), device=dev).to(torch.bfloat16)
    scores = torch.empty((batch, T), device=dev)
    kept = torch.empty((batch, KEEP + 1), dtype=torch.int32, device=dev)
    x = torch.randn((batch * T, D), device=dev).to(torch.bfloat16)
    y = torch.empty((batch * (KEEP + 1), D), dtype=torch.bfloat16, device=dev)
    slots = 2 * ((D + 255) // 256)
    sx = torch.randn((batch * T, slots, 2), device=dev)
    sy = torch.empty((batch * (KEEP + 1), slots, 2), device=dev)
    res = {
        "scores_us": spread(event_us(lambda: _lib.check(lib.evt_token_scores(
            1, p(qkv), 3 * H * HD, 0, 0, 0, batch, T, H, HD, HD ** -0.5, p(scores), stream)))),
        "select_us": spread(event_us(lambda: _lib.check(lib.evt_token_select(
            p(scores), batch, T, KEEP, p(kept), stream)))),
        "gather_us": spread(event_us(lambda: _lib.check(lib.evt_token_gather(
            1, p(x), p(y), p(sx), p(sy), slots, p(kept), batch, T, KEEP + 1, D, stream)))),
    }
    nbytes = 2 * batch * (KEEP + 1) * (D * 2 + slots * 8)
    res["gather_tbytes_per_s"] = round(nbytes / res["gather_us"]["median"] / 1e6, 3)
    return res


def forward(batch, dev):
    m = vitmod.get_deit_base(dtype="bf16", max_batch=batch)
    img = torch.randn((batch, 3, 224, 224), device=dev)
    logits = torch.empty((batch, m.num_classes), device=dev)
    names = ["unscheduled"] + list(SCHEDULES)

    def run(name):
        m.set_token_pruning(SCHEDULES.get(name))  # host only: the same handle, the same workspace
        for _ in range(CALLS):
            m.forward_into(img, logits)
        torch.cuda.synchronize()

    for name in names:
        for _ in range(WARMUP):
            run(name)
    ms = {k: [] for k in names}
    for _ in range(ROUNDS):  # alternated: every round times each variant once
        for k in names:
            m.set_token_pruning(SCHEDULES.get(k))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(k)
            ms[k].append((time.perf_counter() - t0) * 1e3 / CALLS)
    base, g0 = statistics.median(ms["unscheduled"]), m.cfg.gflop_per_image()
    res = {"unscheduled_ms": spread(ms["unscheduled"], 3),
           "unscheduled_images_per_s": round(batch / base * 1e3, 1)}
    for k, sched in SCHEDULES.items():
        med = statistics.median(ms[k])
        res[k] = {"tokens": [t for _, _, _, t in schedule_tokens(m.cfg.tokens, m.cfg.depth, sched)],
                  "ms": spread(ms[k], 3), "images_per_s": round(batch / med * 1e3, 1),
                  "time_over_unscheduled": round(med / base, 4),
                  "gflop_over_unscheduled": round(scheduled_gflop_per_image(m.cfg, sched) / g0, 4)}
    m.close()
    return res


def bench_ab(parent_lib, rounds, seconds):
    """bench.py's default line, this tree's library and the parent's alternated."""
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "20",
           "--warmup", "5"]
    vals = {"this": [], "parent": []}
    for _ in range(rounds):
        for who in ("this", "parent"):
            env = dict(os.environ)
            if who == "parent":
                env["EVT_LIB"] = parent_lib
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=seconds)
            if r.returncode != 0:  # nothing further on the GPU
                raise SystemExit(f"bench.py ({who}) ended with {r.returncode}:\n{r.stderr[-2000:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            vals[who].append(json.loads(line)["value"])
    res = {k + "_images_per_s": spread(v) for k, v in vals.items()}
    res["rounds"] = rounds
    res["this_over_parent"] = round(statistics.median(vals["this"]) /
                                    statistics.median(vals["parent"]), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "token_pruning_measure.json"))
    ap.add_argument("--step-seconds", type=int, default=150)
    ap.add_argument("--parent-lib", default="", help="libevt_hip.so built from the parent commit")
    ap.add_argument("--bench-rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    _lib.ensure_device(dev.index or 0)
    res = {"dtype": "bf16", "model": "deit_base (reference semantics)", "tokens": T,
           "kernel_shape": {"tokens": T, "heads": H, "head_dim": HD, "dim": D, "keep": KEEP},
           "warmup": WARMUP, "reps": REPS, "rounds": ROUNDS, "calls_per_round": CALLS, "cases": {}}
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    for batch in (512, 64):
        signal.alarm(a.step_seconds)
        r = {"kernels": kernels(batch, dev)}
        signal.alarm(a.step_seconds)
        r["forward"] = forward(batch, dev)
        signal.alarm(0)
        res["cases"][f"bs{batch}"] = r
        print(f"bs{batch}: {r}", file=sys.stderr, flush=True)
    res["scheduled_faster_at_512"] = \
        res["cases"]["bs512"]["forward"]["keep_0.7"]["time_over_unscheduled"] < 1.0
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
