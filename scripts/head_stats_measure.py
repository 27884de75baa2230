"""The head-statistics kernel (head_stats_kernel, csrc/attn_maps.hip) on one MI355X, DeiT-base in
bf16 at 64 and 512 images:

  * the kernel for one block (evt_attention_head_stats on random q / k in the head-major layout
    the model's QKV GEMM stores at these batches) against the EVT_ATTN_ALL export of the same
    block (evt_attention_probs, nq = T) in the same process: time per launch and the ratio. The
    expectation to confirm or refute: the statistics cost less than the full map, because they
    write 16 bytes per head where the export writes 4 T^2;
  * the whole forward: `head_stats_into` for all 12 blocks over the plain forward to logits.

    python scripts/head_stats_measure.py [--out profiles/head_stats_measure.json]

Recorded, not gated. One process; every step runs under its own time limit, an alarm with the
default action: a step that overruns it, hung in a device wait included, ends the process there
and nothing further is started on the GPU. Medians over REPS repetitions after WARMUP warm-up
calls, HIP events around each launch. The values are random (they do not change the work).
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

WARMUP, REPS = 5, 30
H, T, HD, GRID = 12, 197, 64, 14
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


def kernel(batch, dev):
    lib = _lib.load_library()
    qkv = torch.randn((batch, H, 3, T, HD), device=dev).to(torch.bfloat16)  # head-major
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    layout = (ctypes.c_void_p(qkv.data_ptr()), 64, 3 * H * T * 64, 3 * T * 64, T * 64, batch, T, H,
              HD, HD ** -0.5)
    stats = torch.empty((batch, H, 4), device=dev)
    full = torch.empty((batch, H, T, T), device=dev)
    s_us = event_us(lambda: _lib.check(lib.evt_attention_head_stats(
        1, *layout, 1, GRID, ctypes.c_void_p(stats.data_ptr()), stream)))
    m_us = event_us(lambda: _lib.check(lib.evt_attention_probs(
        1, *layout, T, ctypes.c_void_p(full.data_ptr()), stream)))
    return {"head_stats_us": round(s_us, 1), "maps_all_us": round(m_us, 1),
            "stats_over_maps": round(s_us / m_us, 3), "stats_out_bytes": stats.numel() * 4,
            "maps_out_mbytes": round(full.numel() * 4 / 1e6, 1)}


def forward(batch, dev):
    cfg = vit_config(KW["dim"], KW["depth"], KW["heads"], 4 * KW["dim"], patch_size=16)
    rng = np.random.default_rng(0)
    params = {n: np.ones(s, np.float32) if n.endswith("_g")
              else rng.standard_normal(s, dtype=np.float32) * np.float32(0.02)
              for n, s in std_vit_param_shapes(cfg)}
    m = vitmod.StandardViT(**KW, dtype="bf16", weights=params, max_batch=batch)
    img = torch.randn((batch, 3, 224, 224), device=dev)
    logits = torch.empty((batch, m.num_classes), device=dev)
    stats = [torch.empty((batch, H, 4), device=dev) for _ in range(12)]
    plain = host_ms(lambda: m.forward_into(img, logits))
    every = host_ms(lambda: m.head_stats_into(img, blocks=range(12), stat_tensors=stats,
                                              logits=logits))
    hm = m.qkv_headmajor_layers()
    m.close()
    return {"forward_ms": round(plain, 3), "headmajor_layers": hm,
            "stats_12_blocks_ms": round(every, 3), "stats_12_over_forward": round(every / plain, 4),
            "per_block_us": round((every - plain) / 12 * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "head_stats_measure.json"))
    ap.add_argument("--step-seconds", type=int, default=150)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    _lib.ensure_device(dev.index or 0)
    res = {"dtype": "bf16", "model": "deit_base_patch16_224", "warmup": WARMUP, "reps": REPS,
           "cases": {}}
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
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
