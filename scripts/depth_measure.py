"""The depth axis (include/evt_depth.h) on one MI355X, DeiT-base in bf16, at 512 and 64 images:

  * the stream-delta kernel on its own (evt_stream_delta_stats on two [B 197, 768] bf16 matrices,
    HIP events per call; above 16 tokens that is its two launches and the pool allocation of the
    op-level entry point) against the bytes it must move, 2 B T D elements read once;
  * the same reduction written in torch on the same tensors;
  * the forward with the statistics of all 24 sublayers against the plain forward;
  * the forward with the last two attention sublayers skipped, and with the last block skipped,
    against the unskipped forward, with the matmul-FLOP ratio beside each; one handle, the variants
    alternated within every round;
  * with --parent-lib: bench.py's default line with this tree's library and with the library of
    the parent commit (EVT_LIB), alternated, each run a process of its own.

    python scripts/depth_measure.py [--out profiles/depth_measure.json]
                                    [--parent-lib /path/to/parent/libevt_hip.so]

Recorded, not gated. Every step runs under its own time limit, an alarm with the default action: a
step that overruns it, hung in a device wait included, ends the process there and nothing further
is started on the GPU. Medians and min-max over REPS calls or ROUNDS alternated rounds after
warm-up. The values are random (they do not change the work).
"""
import argparse
import ctypes
import dataclasses
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

WARMUP, REPS, ROUNDS, CALLS = 5, 30, 15, 3
T, D = 197, 768
SKIPS = {"unskipped": {}, "last_two_attn": {10: "attn", 11: "attn"}, "last_block": {11: "block"}}


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


def torch_stats(a, b, batch):
    a, b = a.float(), b.float()
    na, nb = a.norm(dim=-1), b.norm(dim=-1)
    tiny = torch.finfo(torch.float32).tiny
    cos = ((a * b).sum(-1) / (na * nb).clamp_min(tiny)).view(batch, T)
    rel = ((b - a).norm(dim=-1) / na.clamp_min(tiny)).view(batch, T)
    ratio = (nb / na.clamp_min(tiny)).view(batch, T)
    return torch.stack([cos.mean(1), rel.mean(1), ratio.mean(1), cos[:, 0]], dim=1)


def kernel(batch, dev):
    lib = _lib.load_library()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    a = torch.randn((batch * T, D), device=dev).to(torch.bfloat16)
    b = (a.float() + 0.3 * torch.randn((batch * T, D), device=dev)).to(torch.bfloat16)
    out = torch.empty((batch, 4), device=dev)
    us = event_us(lambda: _lib.check(lib.evt_stream_delta_stats(1, p(a), D, p(b), D, batch, T, D,
                                                                p(out), stream)))
    ref = torch_stats(a, b, batch)
    tus = event_us(lambda: torch_stats(a, b, batch))
    nbytes = 2 * batch * T * D * 2 + batch * 16
    return {"bytes": nbytes, "us": spread(us, 2),
            "tbytes_per_s": round(nbytes / statistics.median(us) / 1e6, 3), "torch_us": spread(tus, 2),
            "torch_over_kernel": round(statistics.median(tus) / statistics.median(us), 2),
            "max_abs_diff_to_torch": float((out - ref).abs().max())}


def timed(variants, select, run):
    for k in variants:
        select(k)
        for _ in range(WARMUP):
            run(k)
    ms = {k: [] for k in variants}
    for _ in range(ROUNDS):  # alternated: every round times each variant once
        for k in variants:
            select(k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(k)
            ms[k].append((time.perf_counter() - t0) * 1e3 / CALLS)
    return ms


def forward(batch, dev):
    m = vitmod.get_deit_base(dtype="bf16", max_batch=batch)
    img = torch.randn((batch, 3, 224, 224), device=dev)
    logits = torch.empty((batch, m.num_classes), device=dev)
    stats = [torch.empty((batch, 2, 4), device=dev) for _ in range(12)]
    res = {}

    def run_stats(k):
        for _ in range(CALLS):
            if k == "plain":
                m.forward_into(img, logits)
            else:
                m.block_stats_into(img, blocks=range(12), stat_tensors=stats, logits=logits)
        torch.cuda.synchronize()

    ms = timed(("plain", "all_24_sublayers"), lambda k: None, run_stats)
    base = statistics.median(ms["plain"])
    res["statistics"] = {k: {"ms": spread(v, 3), "time_over_plain": round(statistics.median(v) / base, 4)}
                         for k, v in ms.items()}

    def select(k):
        m.skip_sublayers(SKIPS[k])
        torch.cuda.synchronize()

    def run(k):
        for _ in range(CALLS):
            m.forward_into(img, logits)
        torch.cuda.synchronize()

    ms = timed(tuple(SKIPS), select, run)
    m.clear_skips()
    base = statistics.median(ms["unskipped"])
    full = m.cfg.gflop_per_image()
    res["skips"] = {}
    for k, v in ms.items():
        bits = {b: w for b, w in SKIPS[k].items()}
        cfg = m.cfg
        # matmul FLOPs of what still runs: a block without attention keeps its FFN and the reverse
        heads = [0 if bits.get(i) in ("attn", "block") else h for i, h in enumerate(cfg.heads)]
        ffn = [0 if bits.get(i) in ("ffn", "block") else f for i, f in enumerate(cfg.ffn)]
        left = dataclasses.replace(cfg, heads=tuple(heads), ffn=tuple(ffn)).gflop_per_image()
        res["skips"][k] = {"ms": spread(v, 3), "images_per_s": round(batch / statistics.median(v) * 1e3, 1),
                           "time_over_unskipped": round(statistics.median(v) / base, 4),
                           "matmul_flop_over_unskipped": round(left / full, 4)}
    m.close()
    return res


def bench_ab(parent_lib, rounds, seconds):
    """bench.py's default line, this tree's library and the parent's alternated."""
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "20",
           "--warmup", "5"]
    vals = {"this": [], "parent": []}
    for i in range(rounds):
        for who in (("parent", "this"), ("this", "parent"))[i % 2]:  # who goes first alternates too
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_measure.json"))
    ap.add_argument("--step-seconds", type=int, default=150)
    ap.add_argument("--parent-lib", default="", help="libevt_hip.so built from the parent commit")
    ap.add_argument("--bench-rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    _lib.ensure_device(dev.index or 0)
    res = {"dtype": "bf16", "model": "deit_base (reference semantics)", "warmup": WARMUP,
           "reps": REPS, "rounds": ROUNDS, "calls_per_round": CALLS}
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    for name, step in (("kernel_bs512", lambda: kernel(512, dev)), ("kernel_bs64", lambda: kernel(64, dev)),
                       ("forward_bs512", lambda: forward(512, dev)),
                       ("forward_bs64", lambda: forward(64, dev))):
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
