"""Swin-B at 384 px (swin_base_patch4_window12_384) on one MI355X: images/s, the per-role device
times of a forward (evt_model_profile), and the stage-1 window-attention launch of the window-12
kernel beside the window-7 kernel's (Swin-B at 224 px) in the same process.

    python scripts/swin384_measure.py [--batches 64,16] [--out FILE]

The stage-1 figures come from single-stage models of the stage-1 shape (embed 128, 4 heads, two
blocks): 96 x 96 tokens at window 12, 56 x 56 at window 7. Bytes per launch are the QKV read plus
the O write (4 x rows x C x 2 B); MFMA work is 4 x rows x w^2 x C FLOP.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from edgevisiontransformer_amd import profiling  # noqa: E402
from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer, get_swin  # noqa: E402

PEAK_TFLOPS, PEAK_GBPS = 2500.0, 8000.0


def images_per_s(m, batch, size, steps=20, warmup=5):
    img = torch.randn((batch, 3, size, size), device=m.device, dtype=torch.float32)
    logits = torch.empty((batch, m.num_classes), dtype=torch.float32, device=m.device)
    for _ in range(warmup):
        m.forward_into(img, logits)
    torch.cuda.synchronize()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        m.forward_into(img, logits)
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    t.sort()
    return batch / t[len(t) // 2], img, logits


def stage1_attention(window, size, batch):
    m = SwinTransformer(img_size=size, embed_dim=128, depths=(2,), num_heads=(4,),
                        window_size=window, num_classes=8, dtype="bf16", seed=0, max_batch=batch)
    _, img, logits = images_per_s(m, batch, size, steps=3, warmup=2)
    kt = profiling.kernel_times(m, img, logits, forwards=10)["attention"]
    us = kt["us_per_launch"]
    gb = kt["gbytes"] / kt["launches"]
    gf = kt["gflop"] / kt["launches"]
    m.close()
    return {"window": window, "tokens_per_image": (size // 4) ** 2, "batch": batch,
            "us_per_launch": round(us, 1), "gbytes_per_launch": round(gb, 4),
            "hbm_frac": round(gb / (us * 1e-6) / PEAK_GBPS, 4),
            "tflops": round(gf / (us * 1e-6) / 1e3, 1),
            "mfma_frac": round(gf / (us * 1e-6) / 1e3 / PEAK_TFLOPS, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    here = os.path.dirname(os.path.abspath(__file__))
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=here,
                                capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    res = {"model": "swin_base_patch4_window12_384", "dtype": "bf16", "commit": commit or None,
           "images_per_s": {}, "roles": {}}
    for b in [int(x) for x in a.batches.split(",")]:
        m = get_swin("swin_base_patch4_window12_384", dtype="bf16", seed=0, max_batch=b)
        ips, img, logits = images_per_s(m, b, 384)
        res["images_per_s"][str(b)] = round(ips, 1)
        kt = profiling.kernel_times(m, img, logits, forwards=5)
        res["roles"][str(b)] = profiling.roofline_table(kt, PEAK_TFLOPS, PEAK_GBPS)
        m.close()
    b0 = int(a.batches.split(",")[0])
    res["stage1_attention"] = [stage1_attention(12, 384, b0), stage1_attention(7, 224, b0)]
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
