"""The attention-map export (csrc/attn_maps.hip) on one MI355X, DeiT-base in bf16 at 64 and 512
images:

  * the export kernel alone (evt_attention_probs on random q / k in the head-major layout the
    model's QKV GEMM stores at these batches), in CLS and in ALL mode, with both store forms
    (EVT_ATTN_MAPS_STORE=wide / dword): time per launch, TB/s of the bytes it must move (ALL: the
    B H T^2 fp32 written + q and k read once; CLS: k and the CLS rows read, B H T written) and that
    figure as a fraction of ROOF_TBPS, the HBM rate a streaming kernel reaches on this part;
  * beside it, in the same process, `torch.softmax((q @ k.transpose(-1, -2)).float() * scale, -1)`
    on the same q / k (ALL) and the same expression for the CLS row (CLS);
  * the whole forward: `attention_maps_into` for the last block and for all 12 blocks in CLS
    mode, and for the last block in ALL mode, over the plain forward to logits.

    python scripts/attention_maps_measure.py [--out profiles/attention_maps_measure.json]

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
ROOF_TBPS = 6.3  # achievable HBM3E rate of a streaming kernel on MI355X (8.0 peak)
H, T, HD = 12, 197, 64
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
    res = {}
    for mode, nq in (("cls", 1), ("all", T)):
        out = torch.empty((batch, H, nq, T), device=dev)
        moved = out.numel() * 4 + batch * H * (T + nq) * HD * 2
        r = {"out_mbytes": round(out.numel() * 4 / 1e6, 1), "moved_gbytes": round(moved / 1e9, 4)}
        for store in ("wide", "dword"):
            os.environ["EVT_ATTN_MAPS_STORE"] = store
            us = event_us(lambda: _lib.check(lib.evt_attention_probs(
                1, ctypes.c_void_p(qkv.data_ptr()), 64, 3 * H * T * 64, 3 * T * 64, T * 64, batch,
                T, H, HD, HD ** -0.5, nq, ctypes.c_void_p(out.data_ptr()), stream)))
            tbps = moved / (us * 1e-6) / 1e12
            r[store] = {"us": round(us, 1), "tbps": round(tbps, 3),
                        "of_roof": round(tbps / ROOF_TBPS, 3)}
        os.environ.pop("EVT_ATTN_MAPS_STORE")
        q, k = qkv[:, :, 0, :nq], qkv[:, :, 1]
        us = event_us(lambda: torch.softmax((q @ k.transpose(-1, -2)).float() * HD ** -0.5, -1))
        r["torch_us"] = round(us, 1)
        res[mode] = r
        del out
    return res


def forward(batch, dev):
    cfg = vit_config(KW["dim"], KW["depth"], KW["heads"], 4 * KW["dim"], patch_size=16)
    rng = np.random.default_rng(0)
    params = {n: np.ones(s, np.float32) if n.endswith("_g")
              else rng.standard_normal(s, dtype=np.float32) * np.float32(0.02)
              for n, s in std_vit_param_shapes(cfg)}
    m = vitmod.StandardViT(**KW, dtype="bf16", weights=params, max_batch=batch)
    img = torch.randn((batch, 3, 224, 224), device=dev)
    logits = torch.empty((batch, m.num_classes), device=dev)
    cls = [torch.empty((batch, H, T), device=dev) for _ in range(12)]
    plain = host_ms(lambda: m.forward_into(img, logits))
    last = host_ms(lambda: m.attention_maps_into(img, blocks=(-1,), map_tensors=cls[:1],
                                                 logits=logits))
    every = host_ms(lambda: m.attention_maps_into(img, blocks=range(12), map_tensors=cls,
                                                  logits=logits))
    full = torch.empty((batch, H, T, T), device=dev)
    last_all = host_ms(lambda: m.attention_maps_into(img, blocks=(-1,), map_tensors=[full],
                                                     queries="all", logits=logits))
    hm = m.qkv_headmajor_layers()
    m.close()
    return {"forward_ms": round(plain, 3), "headmajor_layers": hm,
            "cls_last_block_ms": round(last, 3), "cls_last_over_forward": round(last / plain, 4),
            "cls_12_blocks_ms": round(every, 3), "cls_12_over_forward": round(every / plain, 4),
            "all_last_block_ms": round(last_all, 3), "all_last_over_forward": round(last_all / plain, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "attention_maps_measure.json"))
    ap.add_argument("--step-seconds", type=int, default=150)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    _lib.ensure_device(dev.index or 0)
    res = {"dtype": "bf16", "model": "deit_base_patch16_224", "warmup": WARMUP, "reps": REPS,
           "roof_tbps": ROOF_TBPS, "cases": {}}
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
