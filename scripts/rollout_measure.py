"""Attention rollout (include/evt_rollout.h) on one MI355X, DeiT-base in bf16 at 64 and 512 images:

  (a) the rollout forward (`attention_rollout_into`, queries="cls" and "all", all 12 blocks)
      against the plain forward to logits (`forward_into`), alternated in the same process;
  (b) at 64 images, the rollout forward against what could be done without it:
      `attention_maps_into` of all 12 blocks (queries="all") into preallocated tensors, then a
      torch fp32 head mean and `bmm` chain. At 512 images the twelve maps alone are 11.4 GB; (b) is
      not run there and the result says so;
  (c) one block's two launches (evt_attention_rollout_step: the head mean and the matrix step) on
      random q / k in the head-major layout the model's QKV GEMM stores at these batches, against
      the EVT_ATTN_ALL export of the same block.

    python scripts/rollout_measure.py [--out profiles/rollout_measure.json]

Recorded, not gated. One process; every step runs under its own time limit, an alarm with the
default action: a step that overruns it, hung in a device wait included, ends the process there
and nothing further is started on the GPU. Forward times: ROUNDS rounds that run every variant
once each in turn after WARMUP warm-up rounds, a host clock around work that ends in a device
synchronise; the median and the (min, max) over the rounds are recorded. Kernel times: HIP events.
The values are random (they do not change the work).
"""
import argparse
import ctypes
import json
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from edgevisiontransformer_amd import _lib  # noqa: E402
from edgevisiontransformer_amd.modeling.models import vit as vitmod  # noqa: E402
from edgevisiontransformer_amd.weights import std_vit_param_shapes, vit_config  # noqa: E402

WARMUP, ROUNDS, REPS = 3, 15, 20
H, T, HD, DEPTH = 12, 197, 64, 12
KW = dict(dim=768, depth=DEPTH, heads=H, patch_size=16)


def alternated(fns):
    """{name: {"ms", "min", "max"}} of the callables, one call each per round, in turn."""
    t = {k: [] for k in fns}
    for r in range(WARMUP + ROUNDS):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= WARMUP:
                t[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"ms": round(statistics.median(v), 3), "min": round(min(v), 3),
                "max": round(max(v), 3)} for k, v in t.items()}


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
    return round(statistics.median(t), 1)


def kernel(batch, dev):
    lib = _lib.load_library()
    qkv = torch.randn((batch, H, 3, T, HD), device=dev).to(torch.bfloat16)  # head-major
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    layout = (ctypes.c_void_p(qkv.data_ptr()), 64, 3 * H * T * 64, 3 * T * 64, T * 64, batch, T, H,
              HD, HD ** -0.5)
    r0, r1, scratch = (torch.rand((batch, T, T), device=dev) for _ in range(3))
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    first = event_us(lambda: _lib.check(lib.evt_attention_rollout_step(
        1, *layout, None, p(r1), p(scratch), scratch.numel() * 4, stream)))
    step = event_us(lambda: _lib.check(lib.evt_attention_rollout_step(
        1, *layout, p(r0), p(r1), p(scratch), scratch.numel() * 4, stream)))
    if batch <= 64:
        full = torch.empty((batch, H, T, T), device=dev)
        maps = event_us(lambda: _lib.check(lib.evt_attention_probs(1, *layout, T, p(full), stream)))
    else:
        maps = None
    # the step's share: the first form runs the head mean and an elementwise kernel
    return {"head_mean_plus_first_us": first, "head_mean_plus_step_us": step,
            "step_minus_first_us": round(step - first, 1), "maps_all_us": maps,
            "step_gflop": round(2.0 * batch * T ** 3 / 1e9, 2)}


def forward(batch, dev):
    cfg = vit_config(KW["dim"], KW["depth"], KW["heads"], 4 * KW["dim"], patch_size=16)
    rng = np.random.default_rng(0)
    params = {n: np.ones(s, np.float32) if n.endswith("_g")
              else rng.standard_normal(s, dtype=np.float32) * np.float32(0.02)
              for n, s in std_vit_param_shapes(cfg)}
    m = vitmod.StandardViT(**KW, dtype="bf16", weights=params, max_batch=batch)
    img = torch.randn((batch, 3, 224, 224), device=dev)
    logits = torch.empty((batch, m.num_classes), device=dev)
    cls = torch.empty((batch, T), device=dev)
    full = torch.empty((batch, T, T), device=dev)
    fns = {
        "forward": lambda: m.forward_into(img, logits),
        "rollout_cls": lambda: m.attention_rollout_into(img, out=cls, queries="cls", logits=logits),
        "rollout_all": lambda: m.attention_rollout_into(img, out=full, queries="all", logits=logits),
    }
    res = {}
    if batch <= 64:
        maps = [torch.empty((batch, H, T, T), device=dev) for _ in range(DEPTH)]
        eye = torch.eye(T, device=dev)
        bufs = [torch.empty((batch, T, T), device=dev) for _ in range(3)]

        def today():
            m.attention_maps_into(img, blocks=range(DEPTH), map_tensors=maps, queries="all",
                                  logits=logits)
            r = None
            for i, a in enumerate(maps):
                ahat = bufs[2]
                torch.mean(a, dim=1, out=ahat)
                ahat.add_(eye).mul_(0.5)
                if r is None:
                    r = bufs[0].copy_(ahat)
                else:
                    r = torch.bmm(ahat, r, out=bufs[i & 1])
            return r
        fns["maps_plus_torch_chain"] = today
        # the two agree (fp32 against fp32, different summation orders)
        m.attention_rollout_into(img, out=full, queries="all")
        res["max_abs_diff_vs_torch_chain"] = float((today() - full).abs().max())
    else:
        res["maps_plus_torch_chain"] = ("not run: the twelve [512, 12, 197, 197] fp32 maps alone "
                                        "are 11.4 GB")
    res.update(alternated(fns))
    f = res["forward"]["ms"]
    for k in ("rollout_cls", "rollout_all"):
        res[k]["over_forward"] = round(res[k]["ms"] / f, 4)
    if batch <= 64:
        res["maps_plus_torch_chain"]["over_forward"] = round(res["maps_plus_torch_chain"]["ms"] / f, 4)
        res["rollout_all"]["over_maps_plus_torch_chain"] = round(
            res["rollout_all"]["ms"] / res["maps_plus_torch_chain"]["ms"], 4)
    res["headmajor_layers"] = m.qkv_headmajor_layers()
    res["scratch_mbytes"] = round(m._rollout_scratch_cache[(batch, _lib.ROLLOUT_ALL)].numel() / 1e6, 1)
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "rollout_measure.json"))
    ap.add_argument("--step-seconds", type=int, default=150)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    _lib.ensure_device(dev.index or 0)
    res = {"dtype": "bf16", "model": "deit_base_patch16_224", "warmup": WARMUP, "rounds": ROUNDS,
           "kernel_reps": REPS, "cases": {}}
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    for batch in (64, 512):
        signal.alarm(a.step_seconds)
        r = {"kernel": kernel(batch, dev)}
        signal.alarm(a.step_seconds)
        r["forward"] = forward(batch, dev)
        signal.alarm(0)
        res["cases"][f"bs{batch}"] = r
        print(f"bs{batch}: {r}", file=sys.stderr, flush=True)
    line = json.dumps(res, indent=1)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
