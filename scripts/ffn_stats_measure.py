"""The FFN-statistics kernel (ffn_stats_kernel, csrc/ffn_stats.hip) on one MI355X, DeiT-base in
bf16 at 512 and 64 images:

  * the kernel for one block (evt_ffn_neuron_stats on a random [B * 197, 3072] bf16 matrix): time
    per launch and the achieved bytes/s (the matrix read once plus the 16 bytes per neuron
    written), against the same reduction written in torch on the same tensor, in the same process;
  * the whole forward: `ffn_stats_into` for the last block and for all 12 blocks against the plain
    forward to logits, the three alternated within every round;
  * with --parent-lib: bench.py's default line with this tree's library and with the library of
    the parent commit (EVT_LIB), alternated, each run a process of its own.

    python scripts/ffn_stats_measure.py [--out profiles/ffn_stats_measure.json]
                                        [--parent-lib /path/to/parent/libevt_hip.so]

Recorded, not gated. Every step runs under its own time limit, an alarm with the default action
(bench.py: the child's timeout): a step that overruns it, hung in a device wait included, ends the
process there and nothing further is started on the GPU. Medians and min-max over REPS launches
(HIP events) or ROUNDS alternated rounds (host clock around a synchronise) after warm-up. The
values are random (they do not change the work).
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
from edgevisiontransformer_amd.modeling.models import vit as vitmod  # noqa: E402
from edgevisiontransformer_amd.weights import std_vit_param_shapes, vit_config  # noqa: E402

WARMUP, REPS, ROUNDS, CALLS = 5, 30, 15, 3
T, F = 197, 3072
KW = dict(dim=768, depth=12, heads=12, patch_size=16)


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


def torch_stats(h, batch):
    x = h.view(batch, T, F).float()
    mag = x.abs()
    return torch.stack([x.mean(1), mag.mean(1), (x * x).mean(1), mag.amax(1)], dim=-1)


def kernel(batch, dev):
    lib = _lib.load_library()
    h = torch.randn((batch * T, F), device=dev).to(torch.bfloat16)
    out = torch.empty((batch, F, 4), device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    k = event_us(lambda: _lib.check(lib.evt_ffn_neuron_stats(
        1, ctypes.c_void_p(h.data_ptr()), F, batch, T, F, ctypes.c_void_p(out.data_ptr()), stream)))
    ref = torch_stats(h, batch)
    agree = float((out - ref).abs().max() / ref.abs().max())
    tt = event_us(lambda: torch_stats(h, batch))
    nbytes = h.numel() * 2 + out.numel() * 4
    med = statistics.median(k)
    return {"kernel_us": spread(k), "torch_us": spread(tt), "bytes": nbytes,
            "kernel_tbytes_per_s": round(nbytes / med / 1e6, 3),
            "torch_over_kernel": round(statistics.median(tt) / med, 2),
            "max_abs_diff_to_torch_over_max": agree}


def forward(batch, dev):
    cfg = vit_config(KW["dim"], KW["depth"], KW["heads"], 4 * KW["dim"], patch_size=16)
    rng = np.random.default_rng(0)
    params = {n: np.ones(s, np.float32) if n.endswith("_g")
              else rng.standard_normal(s, dtype=np.float32) * np.float32(0.02)
              for n, s in std_vit_param_shapes(cfg)}
    m = vitmod.StandardViT(**KW, dtype="bf16", weights=params, max_batch=batch)
    img = torch.randn((batch, 3, 224, 224), device=dev)
    logits = torch.empty((batch, m.num_classes), device=dev)
    stats = [torch.empty((batch, F, 4), device=dev) for _ in range(12)]
    variants = {
        "forward": lambda: m.forward_into(img, logits),
        "last_block": lambda: m.ffn_stats_into(img, blocks=(11,), stat_tensors=stats[11:],
                                               logits=logits),
        "all_12_blocks": lambda: m.ffn_stats_into(img, blocks=range(12), stat_tensors=stats,
                                                  logits=logits),
    }
    for fn in variants.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(ROUNDS):  # alternated: every round times each variant once
        for k, fn in variants.items():
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / CALLS)
    m.close()
    res = {k + "_ms": spread(v, 3) for k, v in ms.items()}
    base = statistics.median(ms["forward"])
    res["last_block_over_forward"] = round(statistics.median(ms["last_block"]) / base, 4)
    res["all_12_over_forward"] = round(statistics.median(ms["all_12_blocks"]) / base, 4)
    res["per_block_us"] = round((statistics.median(ms["all_12_blocks"]) - base) / 12 * 1e3, 1)
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ffn_stats_measure.json"))
    ap.add_argument("--step-seconds", type=int, default=150)
    ap.add_argument("--parent-lib", default="", help="libevt_hip.so built from the parent commit")
    ap.add_argument("--bench-rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    _lib.ensure_device(dev.index or 0)
    res = {"dtype": "bf16", "model": "deit_base_patch16_224", "tokens": T, "neurons": F,
           "warmup": WARMUP, "reps": REPS, "rounds": ROUNDS, "calls_per_round": CALLS, "cases": {}}
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    for batch in (512, 64):
        signal.alarm(a.step_seconds)
        r = {"kernel": kernel(batch, dev)}
        signal.alarm(a.step_seconds)
        r["forward"] = forward(batch, dev)
        signal.alarm(0)
        res["cases"][f"bs{batch}"] = r
        print(f"bs{batch}: {r}", file=sys.stderr, flush=True)
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
