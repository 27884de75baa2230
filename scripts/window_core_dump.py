"""Seeded outputs of every kernel built on csrc/window_scores.h, as .npy files, for a bitwise
comparison of two builds of the library (run it from each tree, then `--compare`):

    python scripts/window_core_dump.py DIR
    python scripts/window_core_dump.py --compare DIR_A DIR_B [--out profiles/window_core_compare.json]

  * evt_window_attention (w = 7), bf16 and f32: (R, H, shift, B) = (14, 3, 0, 2), (14, 3, 3, 2)
    (all four window types of a 2 x 2 grid), (7, 3, 0, 1) (3 pairs in a 4-pair block), (21, 4, 3, 1)
    (3 x 3 grid); ldo = C rounded up to 64, so pad columns exist;
  * window 12: a one-stage Swin (embed 128, 4 heads, depth 2: W-MSA + SW-MSA) at 96 and 144 px, both
    dtypes, batch 2: logits and the last block's tap;
  * the fused C = 96 sublayer: a one-stage 3-head window-7 depth-2 bf16 model at 56 px, batch 3
    (one window per block), and at 224 px with enough images that the windows exceed the grid cap of
    2 x CU count (blocks loop, the next-window prefetch runs);
  * evt_window_attention_probs: w = 7 at R = 14, shift 3 and w = 12 at R = 24, shift 6; H = 3,
    B = 2, both dtypes.

The comparison is numpy.array_equal per array; the exit status is 1 if any differs.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def dump(dirname):
    import torch
    from edgevisiontransformer_amd import _lib
    from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer
    from edgevisiontransformer_amd.weights import make_images, make_swin_params, swin_config

    os.makedirs(dirname, exist_ok=True)
    gpu = torch.device("cuda", 0)
    lib = _lib.load_library()
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16}
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

    def save(name, t):
        a = t.float().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        np.save(os.path.join(dirname, name + ".npy"), a)
        print(name, a.shape, flush=True)

    for dtype in ("bf16", "f32"):
        for R, H, shift, B in [(14, 3, 0, 2), (14, 3, 3, 2), (7, 3, 0, 1), (21, 4, 3, 1)]:
            rng = np.random.default_rng(100 * R + shift)
            C = 32 * H
            ldo = (C + 63) // 64 * 64
            qkv = torch.from_numpy(rng.standard_normal((B * R * R, 3 * C)).astype(np.float32))
            rpb = torch.from_numpy((rng.standard_normal((169, H)) * 0.5).astype(np.float32)).to(gpu)
            qkv = qkv.to(gpu).to(tdt[dtype])
            out = torch.full((B * R * R, ldo), float("nan"), dtype=tdt[dtype], device=gpu)
            _lib.check(lib.evt_window_attention(_lib.DTYPE[dtype], p(qkv), 3 * C, p(out), ldo, p(rpb),
                                                B, R, C, H, shift, stream()))
            torch.cuda.synchronize()
            save(f"attn7_{dtype}_R{R}_H{H}_s{shift}_B{B}", out)
        for w, R, shift in [(7, 14, 3), (12, 24, 6)]:
            H, B, N = 3, 2, w * w
            rng = np.random.default_rng(1000 * w + R)
            qkv = torch.from_numpy(rng.standard_normal((B * R * R, 96 * H)).astype(np.float32))
            qkv = qkv.to(gpu).to(tdt[dtype])
            rpb = torch.from_numpy((rng.standard_normal(((2 * w - 1) ** 2, H)) * 0.5).astype(np.float32)).to(gpu)
            out = torch.full((B, (R // w) ** 2, H, N, N), float("nan"), dtype=torch.float32, device=gpu)
            _lib.check(lib.evt_window_attention_probs(_lib.DTYPE[dtype], p(qkv), qkv.shape[1], p(rpb), B,
                                                      R, w, 32 * H, H, shift, p(out), stream()))
            torch.cuda.synchronize()
            save(f"probs{w}_{dtype}_R{R}_s{shift}", out)

    def model(dtype, image_size, window, embed, heads, batch, tag):
        cfg = swin_config("tiny", image_size=image_size, window_size=window, embed_dim=embed,
                          depths=(2,), num_heads=(heads,), num_classes=11)
        m = SwinTransformer(img_size=cfg.image_size, patch_size=cfg.patch_size, num_classes=cfg.num_classes,
                            embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
                            window_size=cfg.window_size, dtype=dtype, weights=make_swin_params(cfg, seed=7),
                            device=gpu, max_batch=batch)
        img = torch.from_numpy(make_images(batch, seed=8, image_size=image_size)).to(gpu)
        out = m.features(img, taps=(1,), logits=True)
        torch.cuda.synchronize()
        save(f"{tag}_logits", out["logits"])
        save(f"{tag}_tap1", out["taps"][0])

    for dtype in ("bf16", "f32"):
        for size in (96, 144):
            model(dtype, size, 12, 128, 4, 2, f"w12_{dtype}_{size}")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    batch = 9
    while batch * 64 <= 2 * cus:  # 64 windows per 224 px image: more windows than the grid cap
        batch += 1
    print(f"CUs {cus}: fused sublayer at 224 px with batch {batch} = {batch * 64} windows, grid cap "
          f"{2 * cus}", flush=True)
    model("bf16", 56, 7, 96, 3, 3, "fused96_56_B3")
    model("bf16", 224, 7, 96, 3, batch, "fused96_224")


def compare(a, b, out):
    names = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
    res = {}
    for f in names:
        pb = os.path.join(b, f)
        res[f[:-4]] = os.path.exists(pb) and bool(np.array_equal(np.load(os.path.join(a, f)), np.load(pb),
                                                                 equal_nan=True))
    missing = sorted(f[:-4] for f in os.listdir(b) if f.endswith(".npy") and f not in names)
    doc = {"equal": res, "only_in_second": missing, "all_equal": all(res.values()) and not missing}
    print(json.dumps(doc, indent=1))
    if out:
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0 if doc["all_equal"] and names else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("dirs", nargs="+")
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.dirs[0], a.dirs[1], a.out))
    dump(a.dirs[0])
