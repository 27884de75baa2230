"""The Swin window attention-map export (csrc/attn_maps.hip) on one MI355X, bf16:

  * the export alone (evt_window_attention_probs on random qkv rows: the table expansion, a few
    microseconds, and the export kernel) at Swin-T with 256 images, stages 1 to 4 (window 7,
    shifted), and at Swin-B 384 px with 64 images, stage 1 (window 12, shifted; both store forms,
    EVT_WINDOW_MAPS_STORE=wide / dword): time per call, TB/s of the bytes it must move (the q and
    k columns read once + the fp32 map written) and that figure as a fraction of ROOF_TBPS, the
    HBM rate a streaming kernel reaches on this part;
  * beside it, in the same process, the same probabilities written in torch from the same qkv
    (roll, window partition, q k^T, bias, mask, softmax in fp32);
  * the whole forward of Swin-T at 256 images: `window_attention_maps_into` for the last block and
    for all 12 blocks over the plain forward to logits.

    python scripts/window_attention_maps_measure.py [--out profiles/window_attention_maps_measure.json]

Recorded, not gated. One process; every step runs under its own time limit, an alarm with the
default action: a step that overruns it, hung in a device wait included, ends the process there
and nothing further is started on the GPU. Medians over REPS repetitions after WARMUP warm-up
calls, HIP events around each call. The values are random (they do not change the work).
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
from edgevisiontransformer_amd.modeling.models.swin import get_swin  # noqa: E402
from edgevisiontransformer_amd.modeling.models.window_attention_maps import window_token_index  # noqa: E402

WARMUP, REPS = 3, 15
ROOF_TBPS = 6.3  # achievable HBM3E rate of a streaming kernel on MI355X (8.0 peak)
LAUNCHES = [  # (name, images, R, window, heads, shift)
    ("swin_t bs256 stage 1", 256, 56, 7, 3, 3), ("swin_t bs256 stage 2", 256, 28, 7, 6, 3),
    ("swin_t bs256 stage 3", 256, 14, 7, 12, 3), ("swin_t bs256 stage 4", 256, 7, 7, 24, 0),
    ("swin_b 384 bs64 stage 1", 64, 96, 12, 4, 6),
]


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


def torch_probs(qkv, rpb, B, R, w, H, shift, dev):
    """The same map in torch: [B, nW, H, N, N] fp32 from the bf16 qkv rows."""
    n, nw, C = w * w, R // w, 32 * H
    idx = torch.from_numpy(window_token_index(R, w, shift)).to(dev)  # [nW, N]
    ys, xs = np.meshgrid(np.arange(w), np.arange(w), indexing="ij")
    rel = ((ys.reshape(-1)[:, None] - ys.reshape(-1)[None, :] + w - 1) * (2 * w - 1) +
           xs.reshape(-1)[:, None] - xs.reshape(-1)[None, :] + w - 1)
    bias = rpb[torch.from_numpy(rel.reshape(-1)).to(dev)].view(n, n, H).permute(2, 0, 1)
    reg = (np.arange(R) >= R - w).astype(np.int64) + (np.arange(R) >= R - shift) if shift else \
        np.zeros(R, np.int64)
    reg = torch.from_numpy(reg[:, None] * 3 + reg[None, :]).to(dev)  # regions of the shifted frame
    rw = reg.view(nw, w, nw, w).permute(0, 2, 1, 3).reshape(nw * nw, n)
    mask = rw[:, :, None] != rw[:, None, :]  # [nW, N, N]

    def run():
        x = qkv.view(B, R * R, 3, H, 32)[:, idx]  # [B, nW, N, 3, H, 32]
        q, k = x[:, :, :, 0].permute(0, 1, 3, 2, 4), x[:, :, :, 1].permute(0, 1, 3, 2, 4)
        att = (q @ k.transpose(-1, -2)).float() * 32 ** -0.5 + bias
        att = att.masked_fill(mask[None, :, None], float("-inf"))
        return torch.softmax(att, -1)
    return run


def kernel(name, B, R, w, H, shift, dev):
    lib = _lib.load_library()
    C = 32 * H
    qkv = torch.randn((B * R * R, 3 * C), device=dev).to(torch.bfloat16)
    rpb = torch.randn(((2 * w - 1) ** 2, H), device=dev) * 0.5
    nwin, n = (R // w) ** 2, w * w
    out = torch.empty((B, nwin, H, n, n), device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    moved = out.numel() * 4 + B * R * R * 2 * C * 2
    r = {"out_mbytes": round(out.numel() * 4 / 1e6, 1), "moved_gbytes": round(moved / 1e9, 4)}

    def call():
        _lib.check(lib.evt_window_attention_probs(
            _lib.DTYPE["bf16"], ctypes.c_void_p(qkv.data_ptr()), 3 * C,
            ctypes.c_void_p(rpb.data_ptr()), B, R, w, C, H, shift, ctypes.c_void_p(out.data_ptr()),
            stream))
    for store in (("wide", "dword") if w == 12 else ("dword",)):
        os.environ["EVT_WINDOW_MAPS_STORE"] = store
        us = event_us(call)
        r[store] = {"us": round(us, 1), "tbps": round(moved / us / 1e6, 3),
                    "of_roof": round(moved / us / 1e6 / ROOF_TBPS, 3)}
    os.environ.pop("EVT_WINDOW_MAPS_STORE", None)
    ref = torch_probs(qkv, rpb, B, R, w, H, shift, dev)
    got = ref()
    r["max_abs_vs_torch"] = float((got - out).abs().max())  # (the last call: the dword form)
    del got
    r["torch_us"] = round(event_us(ref), 1)
    return r


def forward(dev):
    B = 256
    m = get_swin("swin_tiny_patch4_window7_224", dtype="bf16", device=dev, max_batch=B)
    x = torch.randn((B, 3, 224, 224), device=dev)
    logits = torch.empty((B, m.num_classes), device=dev)
    r = {"plain_ms": round(host_ms(lambda: m(x)), 3)}
    for what, blocks in (("last_block", [m.num_blocks - 1]), ("all_blocks", list(range(m.num_blocks)))):
        maps = [torch.empty(m._window_map_shape(B, i), device=dev) for i in blocks]
        ms = host_ms(lambda: m.window_attention_maps_into(x, blocks=blocks, map_tensors=maps,
                                                          logits=logits))
        r[what] = {"ms": round(ms, 3), "map_gbytes": round(sum(t.numel() for t in maps) * 4 / 1e9, 3),
                   "over_plain_ms": round(ms - r["plain_ms"], 3)}
        del maps
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "window_attention_maps_measure.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: no device, nothing measured")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "roof_tbps": ROOF_TBPS, "warmup": WARMUP,
           "reps": REPS, "kernel": {}}
    for name, *shape in LAUNCHES:
        signal.alarm(120)
        res["kernel"][name] = kernel(name, *shape, dev)
        signal.alarm(0)
        print(name, json.dumps(res["kernel"][name]), flush=True)
    signal.alarm(180)
    res["forward_swin_t_bs256"] = forward(dev)
    signal.alarm(0)
    print("forward", json.dumps(res["forward_swin_t_bs256"]), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
