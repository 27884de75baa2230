"""uint8 against fp32 image input (include/evt_image.h) on one MI355X, bf16 models:

  DeiT-base bs512, T2T-ViT-14 bs256, Swin-T bs256 (the fused stem), each run with its native fp32
  input and with a `Uint8Images` of the same pixels, the two alternated call by call:

  * the whole-forward time (host clock around `forward_into` that ends in a device synchronise);
  * the first-stage role time from evt_model_profile (patchify for ViT, t2t_unfold for T2T-ViT,
    patch_embed for Swin-T, whose fused stem reads the image), profiled forwards in a second pass;
  * the pinned-host to device copy time of each input (torch events around one `copy_`);
  * the fp32 side's repeat-to-repeat spread: the measurement is taken ROUNDS times and the spread
    is (max - min) / median of the per-round fp32 medians.

    python scripts/uint8_input_measure.py [--out profiles/uint8_input_measure.json]
                                          [--parent parent.json]

Recorded, not gated. The expectation (not a fixed number): the uint8 forward is no slower than the
fp32 forward beyond that spread, since the first kernel reads a quarter of the bytes and writes
the same. On a checkout without `Uint8Images` (the parent commit) the script measures the fp32
side alone; `--parent` copies such a result into the output under "parent", which shows whether
sharing the gather code with the uint8 loaders changed the fp32 first-stage times.

One process; every model runs under its own time limit, an alarm with the default action: a step
that overruns it, hung in a device wait included, ends the process there and nothing further is
started on the GPU.
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
from edgevisiontransformer_amd import _lib, tools  # noqa: E402

try:
    from edgevisiontransformer_amd import Uint8Images
except ImportError:  # the parent commit: fp32 side only
    Uint8Images = None

WARMUP, REPS, ROUNDS = 5, 20, 3
CASES = [  # (label, model name, batch, native layout, first-stage role)
    ("deit_base_bs512", "deit_base", 512, "nchw", "patchify"),
    ("t2t_vit_14_bs256", "t2t_vit_14", 256, "nhwc", "t2t_unfold"),
    ("swin_tiny_bs256", "swin_tiny", 256, "nchw", "patch_embed"),
]


def forward_ms(m, inputs, logits):
    """Per input kind, the per-round medians of the host-clocked forward; the kinds alternate."""
    for _ in range(WARMUP):
        for x in inputs.values():
            m.forward_into(x, logits)
    torch.cuda.synchronize()
    rounds = {k: [] for k in inputs}
    for _ in range(ROUNDS):
        t = {k: [] for k in inputs}
        for _ in range(REPS):
            for k, x in inputs.items():
                t0 = time.perf_counter()
                m.forward_into(x, logits)
                torch.cuda.synchronize()
                t[k].append((time.perf_counter() - t0) * 1e3)
        for k in inputs:
            rounds[k].append(statistics.median(t[k]))
    return rounds


def role_us(m, inputs, logits, role):
    """Per input kind, the median device time of the first-stage role (profiled forwards)."""
    lib, h = _lib.load_library(), ctypes.c_void_p(m._handle)
    idx = _lib.PROF_ROLES.index(role)
    us = (ctypes.c_float * len(_lib.PROF_ROLES))()
    n = (ctypes.c_int * len(_lib.PROF_ROLES))()
    _lib.check(lib.evt_model_profile(h, 1))
    t = {k: [] for k in inputs}
    for i in range(WARMUP + REPS):
        for k, x in inputs.items():
            m.forward_into(x, logits)
            _lib.check(lib.evt_model_profile_read(h, us, n))
            if i >= WARMUP:
                t[k].append(us[idx])
    _lib.check(lib.evt_model_profile(h, 0))
    return {k: statistics.median(v) for k, v in t.items()}


def copy_us(dev_tensor):
    """Median time of one pinned-host to device copy of a tensor of this shape and dtype."""
    host = torch.empty(dev_tensor.shape, dtype=dev_tensor.dtype).pin_memory()
    t = []
    for i in range(WARMUP + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dev_tensor.copy_(host, non_blocking=True)
        b.record()
        b.synchronize()
        if i >= WARMUP:
            t.append(a.elapsed_time(b) * 1e3)
    return statistics.median(t)


def measure(name, batch, layout, role):
    m = tools.build_model(name, "bf16", max_batch=batch)
    dev = m.device
    bytes_ = np.random.default_rng(0).integers(0, 256, size=(batch, 224, 224, 3), dtype=np.uint8)
    inputs = {}
    if Uint8Images is not None:
        u8 = Uint8Images(torch.from_numpy(bytes_)).to(dev)
        inputs["fp32"] = u8.to_float(layout)
        inputs["uint8"] = u8
    else:  # the same pixel values, normalised on the host
        mean, std = np.float32([0.485, 0.456, 0.406]), np.float32([0.229, 0.224, 0.225])
        f = (bytes_.astype(np.float32) / np.float32(255) - mean) / std
        inputs["fp32"] = torch.from_numpy(
            np.ascontiguousarray(f.transpose(0, 3, 1, 2)) if layout == "nchw" else f).to(dev)
    logits = torch.empty((batch, m.num_classes), device=dev)
    rounds = forward_ms(m, inputs, logits)
    roles = role_us(m, inputs, logits, role)
    res = {"batch": batch, "first_stage_role": role, "lanes": m.lanes()}
    for k, x in inputs.items():
        t = x.data if k == "uint8" else x
        res[k] = {"input_mbytes": round(t.numel() * t.element_size() / 1e6, 1),
                  "forward_ms_rounds": [round(v, 3) for v in rounds[k]],
                  "forward_ms": round(statistics.median(rounds[k]), 3),
                  "first_stage_us": round(roles[k], 1),
                  "h2d_copy_us": round(copy_us(t), 1)}
    f = rounds["fp32"]
    res["fp32_spread"] = round((max(f) - min(f)) / statistics.median(f), 4)
    if "uint8" in res:
        res["uint8_over_fp32_forward"] = round(res["uint8"]["forward_ms"] / res["fp32"]["forward_ms"], 4)
        res["uint8_over_fp32_first_stage"] = round(
            res["uint8"]["first_stage_us"] / res["fp32"]["first_stage_us"], 4)
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "uint8_input_measure.json"))
    ap.add_argument("--parent", default=None,
                    help="a result of this script on the parent commit (fp32 only), copied in")
    ap.add_argument("--step-seconds", type=int, default=240)
    a = ap.parse_args()
    res = {"dtype": "bf16", "warmup": WARMUP, "reps": REPS, "rounds": ROUNDS,
           "uint8": Uint8Images is not None, "cases": {}}
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    for label, name, batch, layout, role in CASES:
        signal.alarm(a.step_seconds)
        res["cases"][label] = measure(name, batch, layout, role)
        signal.alarm(0)
        print(f"{label}: {res['cases'][label]}", file=sys.stderr, flush=True)
    if a.parent:
        with open(a.parent) as f:
            parent = json.load(f)
        res["parent"] = {k: {"first_stage_us": v["fp32"]["first_stage_us"],
                             "forward_ms": v["fp32"]["forward_ms"],
                             "fp32_spread": v["fp32_spread"]}
                         for k, v in parent["cases"].items()}
    line = json.dumps(res, indent=1)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
