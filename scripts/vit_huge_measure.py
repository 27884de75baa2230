"""ViT-H/14 and ViT-L/14 (vit_huge_patch14_224, vit_large_patch14_224; StandardViT, bf16) on one
MI355X: images/s, the per-role device times of a forward (evt_model_profile), and the two figures
that decide follow-up work:

  * the achieved HBM bandwidth of the patch-14 patchify kernel (patchify_ld_kernel) beside the
    patch-16 one's (patchify_cm_kernel, vit_large_patch16_224 at the same width and batch) in the
    same process, as a ratio;
  * the attention role's share of the ViT-H forward (head size 80 on the generic streaming kernel)
    beside the QKV role's.

    python scripts/vit_huge_measure.py [--out FILE] [--step-seconds 120]

One process. Every step (a model built, timed and profiled) runs under its own time limit, an
alarm with the default action: a step that overruns it, hung in a device wait included, ends the
process there (killed by SIGALRM) and nothing further is started on the GPU. The weights are
small random numbers drawn in fp32 (the values do not change the work).
"""
import argparse
import json
import os
import signal
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from edgevisiontransformer_amd import profiling  # noqa: E402
from edgevisiontransformer_amd.modeling.models import vit as vitmod  # noqa: E402
from edgevisiontransformer_amd.weights import std_vit_param_shapes, vit_config  # noqa: E402

PEAK_TFLOPS, PEAK_GBPS = 2500.0, 8000.0


def fast_params(name, depth=None):
    """fp32 N(0, 0.02) weights (LayerNorm gammas 1) for a STD_VIT_NAMED configuration."""
    kw = dict(vitmod.STD_VIT_NAMED[name])
    if depth is not None:
        kw["depth"] = depth
    cfg = vit_config(kw["dim"], kw["depth"], kw["heads"], 4 * kw["dim"],
                     patch_size=kw["patch_size"])
    rng = np.random.default_rng(0)
    p = {}
    for pname, shape in std_vit_param_shapes(cfg):
        if pname.endswith("_g"):
            p[pname] = np.ones(shape, np.float32)
        else:
            p[pname] = rng.standard_normal(shape, dtype=np.float32) * np.float32(0.02)
    return kw, p


def images_per_s(m, batch, steps=20, warmup=5):
    img = torch.randn((batch, 3, 224, 224), device=m.device, dtype=torch.float32)
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


def measure(name, batches, depth=None):
    """One handle sized for the largest batch; images/s and the role table per batch."""
    kw, params = fast_params(name, depth)
    m = vitmod.StandardViT(**kw, dtype="bf16", weights=params, max_batch=max(batches))
    del params
    out = {"depth": kw["depth"], "images_per_s": {}, "roles": {}}
    for b in batches:
        ips, img, logits = images_per_s(m, b)
        out["images_per_s"][str(b)] = round(ips, 1)
        kt = profiling.kernel_times(m, img, logits, forwards=5)
        out["roles"][str(b)] = profiling.roofline_table(kt, PEAK_TFLOPS, PEAK_GBPS)
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-seconds", type=int, default=120)
    a = ap.parse_args()
    here = os.path.dirname(os.path.abspath(__file__))
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=here,
                                capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    res = {"dtype": "bf16", "commit": commit or None, "models": {}}
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    steps = [("vit_huge_patch14_224", [64, 16], None),
             ("vit_large_patch14_224", [64], None),
             # the patch-16 patchify of the same width and batch (one layer is enough)
             ("vit_large_patch16_224", [64], 1)]
    for name, batches, depth in steps:
        signal.alarm(a.step_seconds)
        res["models"][name] = measure(name, batches, depth)
        signal.alarm(0)
        print(f"{name}: {res['models'][name]['images_per_s']}", file=sys.stderr, flush=True)
    r = res["models"]
    p14 = r["vit_large_patch14_224"]["roles"]["64"]["patchify"]
    p16 = r["vit_large_patch16_224"]["roles"]["64"]["patchify"]
    res["patchify"] = {"patch14_gbps": p14["gbps"], "patch14_us": p14["us"],
                       "patch16_gbps": p16["gbps"], "patch16_us": p16["us"],
                       "ratio_patch14_over_patch16": round(p14["gbps"] / p16["gbps"], 3)}
    h = r["vit_huge_patch14_224"]["roles"]["64"]
    total = sum(v["us"] for v in h.values())
    res["vit_huge_bs64"] = {"forward_us": round(total, 1),
                            "attention_share": round(h["attention"]["us"] / total, 4),
                            "qkv_share": round(h["qkv"]["us"] / total, 4),
                            "patchify_share": round(h["patchify"]["us"] / total, 5),
                            "attention_over_qkv": round(h["attention"]["us"] / h["qkv"]["us"], 3)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
