"""The stream-export kernel (csrc/features.hip) and the feature forwards on one MI355X, bf16:

  * the export kernel's device time and achieved GB/s writing the normalised token map of
    DeiT-base (deit_base_patch16_224) at 512 and at 64 images and of ViT-H/14 at 64: a profiled
    features forward that asks for the tokens alone launches nothing else under the "head" role
    (no logits: no head GEMM), so that role's event pair brackets the one export launch;
  * beside each, `x.float()` on a bf16 tensor of the same shape in the same process (torch events
    around the one cast kernel), which moves the same bytes: 2 read + 4 written per element;
  * the whole-forward time of `features(tokens=True)` (pooled + tokens) against the plain
    forward to logits (host clock around a call that ends in a device synchronise).

    python scripts/features_measure.py [--out profiles/features_measure.json]

Recorded, not gated. One process; every step runs under its own time limit, an alarm with the
default action: a step that overruns it, hung in a device wait included, ends the process there
and nothing further is started on the GPU. Medians over REPS repetitions after WARMUP warm-up
calls of every shape. The weights are small random numbers (the values do not change the work).
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
CASES = [  # (label, StandardViT keywords, images)
    ("deit_base_bs512", dict(dim=768, depth=12, heads=12, patch_size=16), 512),
    ("deit_base_bs64", dict(dim=768, depth=12, heads=12, patch_size=16), 64),
    ("vit_huge_patch14_bs64", dict(vitmod.STD_VIT_NAMED["vit_huge_patch14_224"]), 64),
]


def fast_params(kw):
    cfg = vit_config(kw["dim"], kw["depth"], kw["heads"], 4 * kw["dim"], patch_size=kw["patch_size"])
    rng = np.random.default_rng(0)
    return {n: np.ones(s, np.float32) if n.endswith("_g")
            else rng.standard_normal(s, dtype=np.float32) * np.float32(0.02)
            for n, s in std_vit_param_shapes(cfg)}


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


def export_us(m, img, tokens):
    """Median device time of the tokens export launch (the only "head" launch of the forward)."""
    lib, h = _lib.load_library(), ctypes.c_void_p(m._handle)
    head = _lib.PROF_ROLES.index("head")
    us = (ctypes.c_float * len(_lib.PROF_ROLES))()
    n = (ctypes.c_int * len(_lib.PROF_ROLES))()
    _lib.check(lib.evt_model_profile(h, 1))
    t = []
    for i in range(WARMUP + REPS):
        m.features_into(img, tokens=tokens)
        _lib.check(lib.evt_model_profile_read(h, us, n))
        assert n[head] == 1, n[head]
        if i >= WARMUP:
            t.append(us[head])
    _lib.check(lib.evt_model_profile(h, 0))
    return statistics.median(t)


def cast_us(shape, device):
    x = torch.randn(shape, device=device).to(torch.bfloat16)
    t = []
    for i in range(WARMUP + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        y = x.float()
        b.record()
        b.synchronize()
        if i >= WARMUP:
            t.append(a.elapsed_time(b) * 1e3)
        del y
    return statistics.median(t)


def measure(kw, batch):
    m = vitmod.StandardViT(**kw, dtype="bf16", weights=fast_params(kw), max_batch=batch)
    dev = m.device
    img = torch.randn((batch, 3, 224, 224), device=dev)
    f, t, _ = m._feature_geometry()
    logits = torch.empty((batch, m.num_classes), device=dev)
    pooled = torch.empty((batch, f), device=dev)
    tokens = torch.empty((batch, t, f), device=dev)
    gb = batch * t * f * 6 / 1e9  # bf16 read + fp32 written
    ex, ca = export_us(m, img, tokens), cast_us((batch, t, f), dev)
    plain = host_ms(lambda: m.forward_into(img, logits))
    feat = host_ms(lambda: m.features_into(img, pooled=pooled, tokens=tokens))
    m.close()
    return {"tokens_shape": [batch, t, f], "gbytes": round(gb, 4),
            "export_us": round(ex, 1), "export_gbps": round(gb / (ex * 1e-6), 1),
            "cast_us": round(ca, 1), "cast_gbps": round(gb / (ca * 1e-6), 1),
            "export_over_cast": round(ex / ca, 3),
            "forward_ms": round(plain, 3), "features_tokens_ms": round(feat, 3),
            "features_over_forward": round(feat / plain, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "features_measure.json"))
    ap.add_argument("--step-seconds", type=int, default=150)
    a = ap.parse_args()
    res = {"dtype": "bf16", "warmup": WARMUP, "reps": REPS, "cases": {}}
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    for label, kw, batch in CASES:
        signal.alarm(a.step_seconds)
        res["cases"][label] = measure(kw, batch)
        signal.alarm(0)
        print(f"{label}: {res['cases'][label]}", file=sys.stderr, flush=True)
    line = json.dumps(res, indent=1)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
