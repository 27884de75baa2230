"""Per-role device times of one forward of a named DeiT at a given image size
(evt_model_profile through edgevisiontransformer_amd.profiling.kernel_times).

    python scripts/long_model_profile.py --model deit_base --batch 64 --image_size 384 [--out FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from edgevisiontransformer_amd import profiling, tools  # noqa: E402
from edgevisiontransformer_amd.weights import make_images  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="deit_base")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--image_size", type=int, default=384)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    m = tools.build_model(a.model, a.dtype, max_batch=a.batch, image_size=a.image_size)
    img = torch.from_numpy(make_images(a.batch, seed=1, image_size=a.image_size)).to(m.device)
    logits = torch.empty((a.batch, m.num_classes), dtype=torch.float32, device=m.device)
    for _ in range(3):
        m.forward_into(img, logits)
    torch.cuda.synchronize()
    kt = profiling.kernel_times(m, img, logits, forwards=5)
    table = profiling.roofline_table(kt, peak_tflops=2500.0, peak_gbps=8000.0)
    res = {"model": a.model, "batch": a.batch, "image_size": a.image_size, "dtype": a.dtype,
           "qkv_headmajor_layers": m.qkv_headmajor_layers(),
           "us_per_forward": round(sum(v["us"] for v in table.values()), 1), "roles": table}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
