"""The uint8 eval transform (include/evt_preprocess.h) on one MI355X, one process, device events,
medians:

  (a) evt_resize_crop_u8 (through `EvalTransform.into`) on 512 and 64 resident images of
      500 x 375 x 3 -> Resize(256) -> 224, per call and per image, and as GB/s of (the input bytes
      the crop window's taps need + the output bytes);
  (b) the vendor-stack comparator on a float batch of the same shape:
      torch.nn.functional.interpolate(mode="bicubic", antialias=True) + the crop. Time only; it is
      not bit-equal to Pillow;
  (c) Pillow on one CPU core on the same images (resize + crop of one decoded image), for the
      "cores needed to feed one GPU" figure; skipped where Pillow is not installed;
  (d) DeiT-base bs512 and Swin-T bs256 bf16 uint8 forwards with and without the transform in front,
      alternated call by call: the share of the forward it costs.

    python scripts/resize_measure.py [--out profiles/resize_measure.json]

Recorded, not gated. One process; every step runs under its own time limit, an alarm with the
default action: a step that overruns it, hung in a device wait included, ends the process there and
nothing further is started on the GPU.
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from edgevisiontransformer_amd import EvalTransform, Uint8Images, _lib, tools  # noqa: E402
from edgevisiontransformer_amd.images import resize_coefficients, resize_geometry  # noqa: E402

WARMUP, REPS = 5, 30
H, W, C, S = 500, 375, 3, 224


def event_ms(fn, reps=REPS):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return statistics.median(t)


def needed_input_bytes(pre):
    """Bytes of one H x W image inside the tap windows of the crop's columns and rows."""
    oh, ow, top, left = resize_geometry(H, W, pre.resize, S)
    bh, _ = resize_coefficients(W, ow, pre.interpolation, left, S)
    bv, _ = resize_coefficients(H, oh, pre.interpolation, top, S)
    cols = int(bh[-1].sum() - bh[0, 0])
    rows = int(bv[-1].sum() - bv[0, 0])
    return rows * cols * C


def transform_alone(dev, batch):
    pre = EvalTransform(S)
    raw = list(torch.from_numpy(np.random.default_rng(batch).integers(
        0, 256, size=(batch, H, W, C), dtype=np.uint8)).to(dev))
    out = torch.empty((batch, S, S, C), dtype=torch.uint8, device=dev)
    ms = event_ms(lambda: pre.into(raw, out))
    moved = batch * (needed_input_bytes(pre) + S * S * C)
    res = {"batch": batch, "ms_per_call": round(ms, 4), "us_per_image": round(ms * 1e3 / batch, 3),
           "images_per_s": round(batch / ms * 1e3), "needed_gbytes_per_s": round(moved / ms / 1e6, 1),
           "launches_per_call": -(-batch // _lib.RESIZE_CHUNK)}
    # (b) the same shape in float through torch
    f = torch.stack(raw).permute(0, 3, 1, 2).float().contiguous()
    oh, ow, top, left = resize_geometry(H, W, pre.resize, S)

    def vendor():
        r = torch.nn.functional.interpolate(f, size=(oh, ow), mode="bicubic", antialias=True,
                                            align_corners=False)
        return r[:, :, top:top + S, left:left + S].contiguous()
    vms = event_ms(vendor, reps=10)
    res["torch_interpolate_ms_per_call"] = round(vms, 4)
    res["torch_over_ours"] = round(vms / ms, 2)
    pre.close()
    return res


def pillow_one_core():
    try:
        from PIL import Image
    except ImportError:
        return None
    torch.set_num_threads(1)
    pre = EvalTransform(S)
    oh, ow, top, left = resize_geometry(H, W, pre.resize, S)
    imgs = [Image.fromarray(np.random.default_rng(i).integers(0, 256, size=(H, W, C), dtype=np.uint8))
            for i in range(8)]
    t = []
    for i in range(5 + 40):
        im = imgs[i % len(imgs)]
        t0 = time.perf_counter()
        np.asarray(im.resize((ow, oh), Image.BICUBIC))[top:top + S, left:left + S].copy()
        t.append((time.perf_counter() - t0) * 1e3)
    ms = statistics.median(t[5:])
    return {"ms_per_image": round(ms, 4), "images_per_s_per_core": round(1e3 / ms, 1)}


def forward_share(name, batch):
    m = tools.build_model(name, "bf16", max_batch=batch)
    dev = m.device
    pre = EvalTransform(S)
    raw = list(torch.from_numpy(np.random.default_rng(1).integers(
        0, 256, size=(batch, H, W, C), dtype=np.uint8)).to(dev))
    u8 = pre(raw, dev)
    logits = torch.empty((batch, m.num_classes), device=dev)

    def plain():
        m.forward_into(u8, logits)

    def with_transform():
        pre.into(raw, u8.data)
        m.forward_into(u8, logits)
    for _ in range(WARMUP):
        plain()
        with_transform()
    torch.cuda.synchronize()
    t = {"forward": [], "transform_and_forward": []}
    for _ in range(REPS):
        for key, fn in (("forward", plain), ("transform_and_forward", with_transform)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[key].append((time.perf_counter() - t0) * 1e3)
    res = {k: round(statistics.median(v), 3) for k, v in t.items()}
    res["batch"] = batch
    res["transform_share_of_forward"] = round(res["transform_and_forward"] / res["forward"] - 1, 4)
    res["forward_images_per_s"] = round(batch / res["forward"] * 1e3)
    pre.close()
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "resize_measure.json"))
    ap.add_argument("--step-seconds", type=int, default=120)
    a = ap.parse_args()
    _lib.ensure_device(0)
    dev = torch.device("cuda", 0)
    res = {"image": [H, W, C], "crop": S, "resize": EvalTransform(S).resize, "warmup": WARMUP,
           "reps": REPS}
    signal.signal(signal.SIGALRM, signal.SIG_DFL)

    def step(key, fn, *args):
        signal.alarm(a.step_seconds)
        res[key] = fn(*args)
        signal.alarm(0)
        print(f"{key}: {res[key]}", file=sys.stderr, flush=True)
    step("transform_bs512", transform_alone, dev, 512)
    step("transform_bs64", transform_alone, dev, 64)
    step("pillow_one_core", pillow_one_core)
    step("deit_base_bs512", forward_share, "deit_base", 512)
    step("swin_tiny_bs256", forward_share, "swin_tiny", 256)
    if res["pillow_one_core"]:
        per_core = res["pillow_one_core"]["images_per_s_per_core"]
        for key in ("deit_base_bs512", "swin_tiny_bs256"):
            res[key]["pillow_cores_to_feed_it"] = round(res[key]["forward_images_per_s"] / per_core, 1)
    line = json.dumps(res, indent=1)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
