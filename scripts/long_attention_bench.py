"""The streaming attention kernel (more than 256 tokens per image) against torch's
scaled_dot_product_attention on the same tensors, same device, same run.

    python scripts/long_attention_bench.py [--out FILE] [--B 64] [--H 12] [--N 577]

Product: evt_attention, bf16, token-major qkv [B*N][3*H*64] -> out [B*N][H*64] (the layout
transform is part of neither side: SDPA gets contiguous q, k, v [B][H][N][64], its best case).
HIP events on torch's current stream after warm-up; the two sides alternate, 7 rounds of 20
launches each, median round. TFLOP/s from the algorithmic 4 B H N^2 64 FLOP. The script fails
if the outputs disagree beyond the bf16 op tolerance (2e-2): faster and different is not faster."""
import argparse
import ctypes
import json
import os
import sys

import torch
import torch.nn.functional as F
from torch.nn.attention import SDPBackend, sdpa_kernel

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from edgevisiontransformer_amd import _lib  # noqa: E402


def rounds(fns, n_rounds=7, launches=20):
    """Median per-launch milliseconds of each fn; the fns alternate round by round."""
    for fn in fns:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(n_rounds):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[i].append(e0.elapsed_time(e1) / launches)
    return [sorted(t)[len(t) // 2] for t in ts], [[round(x * 1e3, 1) for x in t] for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--H", type=int, default=12)
    ap.add_argument("--N", type=int, default=577)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, H, N, DH = a.B, a.H, a.N, 64
    _lib.ensure_device(0)
    lib = _lib.load_library()
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn((B * N, 3 * H * DH), generator=g, device="cuda").bfloat16()
    out = torch.empty((B * N, H * DH), dtype=torch.bfloat16, device="cuda")
    scale = DH ** -0.5
    q, k, v = (qkv.view(B, N, 3, H, DH)[:, :, i].permute(0, 2, 1, 3).contiguous() for i in range(3))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def product():
        _lib.check(lib.evt_attention(1, ctypes.c_void_p(qkv.data_ptr()), 3 * H * DH,
                                     ctypes.c_void_p(out.data_ptr()), H * DH, B, N, H,
                                     ctypes.c_float(scale), stream))

    def flash():
        return F.scaled_dot_product_attention(q, k, v, scale=scale)

    flops = 4.0 * B * H * N * N * DH
    res = {"shape": {"B": B, "H": H, "N": N, "head": DH, "dtype": "bf16"},
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "gflop": round(flops * 1e-9, 2)}
    with sdpa_kernel([SDPBackend.FLASH_ATTENTION]):
        o = flash()
        product()
        torch.cuda.synchronize()
        ref = out.view(B, N, H, DH).permute(0, 2, 1, 3).float()
        diff = float((o.float() - ref).abs().max())
        (t_prod, t_flash), (r_prod, r_flash) = rounds([product, flash])
    res["product"] = {"us": round(t_prod * 1e3, 1), "TFLOP/s": round(flops / t_prod / 1e9, 1),
                      "rounds_us": r_prod}
    res["sdpa_flash"] = {"us": round(t_flash * 1e3, 1), "TFLOP/s": round(flops / t_flash / 1e9, 1),
                         "rounds_us": r_flash}
    res["maxdiff_product_vs_flash"] = diff
    res["product_over_flash_time"] = round(t_prod / t_flash, 3)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    assert diff <= 2e-2 * (1.0 + float(ref.abs().max())), f"outputs disagree: {diff}"


if __name__ == "__main__":
    main()
