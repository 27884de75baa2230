"""The activation-Gram kernel (gram_kernel / gram_reduce_kernel, csrc/gram.hip) on one MI355X,
DeiT-base shapes in bf16. No target is fixed in advance; the script records medians and min-max of

  * the kernel alone (evt_gram) at R = 512 * 197 and 64 * 197, F = 3072 and 768, against torch on
    the same tensor in the same run, the variants alternated round by round: `h.T @ h` with an fp32
    output (`torch.mm(h.T, h, out_dtype=torch.float32)`; when this torch build refuses that, the
    entry says so and nothing stands in for it), the bf16-output product cast up, and
    `h.float().T @ h.float()`;
  * the whole forward: `activation_grams_into` for one block and for all 12 blocks against the plain
    forward, in alternated rounds;
  * `bench.py` at its default configuration, this build against another build given as
    `--parent-lib` (run through EVT_LIB), alternated, each child process under a time limit.

Timing: device events around a window of back-to-back calls that is sized, from one timed call, to
last about `--window-ms`; every variant is warmed first; each figure is the per-call time of one
window, and the spread is that of the windows (one per round). The calls of a window re-read the
same tensor: the 19 MB and 77 MB matrices (R = 64 * 197) can be served from the 256 MB last-level
cache, the 155 MB and 620 MB ones stream from HBM, as in the forward.

    python scripts/gram_measure.py [--out profiles/gram_measure.json] [--parent-lib path/to/.so]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from edgevisiontransformer_amd import _lib  # noqa: E402
from edgevisiontransformer_amd.modeling.models.vit import get_deit_base  # noqa: E402


def _window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def alternated(variants, rounds, window_ms):
    """{name: [ms per call, one window per round]}: every variant warmed (two calls), its window
    sized from one timed call, then `rounds` rounds that run each variant's window in turn."""
    calls = {}
    for name, fn in variants.items():
        fn()
        fn()
        torch.cuda.synchronize()
        calls[name] = max(3, min(2000, int(window_ms / max(_window(fn, 1), 1e-3))))
    ms = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            ms[name].append(_window(fn, calls[name]))
    return ms, calls


def summary(ms, calls=None):
    out = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
           "windows": len(ms)}
    if calls is not None:
        out["calls_per_window"] = calls
    return out


def kernel_cases(dev, rounds, window_ms):
    lib, out = _lib.load_library(), {}
    s = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    P = ctypes.c_void_p
    for rows in (512 * 197, 64 * 197):
        for f in (3072, 768):
            h = (torch.randn((rows, f), device=dev) * 0.5).to(torch.bfloat16)
            hf = h.float()
            g = torch.empty((f, f), device=dev)
            sm = torch.empty((f,), device=dev)
            n = ctypes.c_size_t()
            _lib.check(lib.evt_gram_scratch_bytes(rows, f, ctypes.byref(n)))
            scratch = torch.empty(max(n.value, 16), dtype=torch.uint8, device=dev)

            def ours():
                _lib.check(lib.evt_gram(_lib.DTYPE["bf16"], P(h.data_ptr()), f, rows, f,
                                        P(g.data_ptr()), P(sm.data_ptr()), P(scratch.data_ptr()),
                                        n.value, s()))

            variants = {"gram_kernel": ours,
                        "torch_bf16_out_bf16_cast_fp32": lambda: (h.T @ h).float(),
                        "torch_fp32_operands": lambda: hf.T @ hf}
            note = None
            try:
                torch.mm(h.T, h, out_dtype=torch.float32)
                variants["torch_bf16_out_fp32"] = lambda: torch.mm(h.T, h, out_dtype=torch.float32)
            except (TypeError, RuntimeError) as e:
                note = f"not measured: this torch refuses mm(out_dtype=float32): {str(e)[:120]}"
            ms, calls = alternated(variants, rounds, window_ms)
            flop = 2.0 * rows * f * f
            case = {k: summary(v, calls[k]) for k, v in ms.items()}
            for v in case.values():
                v["tflops_at_median"] = flop / v["median_ms"] / 1e9
            if note:
                case["torch_bf16_out_fp32"] = note
            ours()
            torch.cuda.synchronize()
            ref = hf.double().T @ hf.double()
            case["max_abs_err_over_max_abs_ref"] = {
                "gram_kernel": ((g.double() - ref).abs().max() / ref.abs().max()).item(),
                "torch_bf16_out_bf16_cast_fp32":
                    (((h.T @ h).double() - ref).abs().max() / ref.abs().max()).item()}
            case.update(flop=flop, matrix_bytes=rows * f * 2, scratch_bytes=n.value)
            out[f"R{rows}_F{f}"] = case
            del h, hf, g, sm, scratch, ref
    return out


def forward_cases(dev, batch, rounds, window_ms):
    m = get_deit_base(dtype="bf16", device=dev, max_batch=batch)
    img = torch.randn((batch, 3, 224, 224), device=dev)
    logits = torch.empty((batch, 1000), device=dev)
    grams = [torch.empty((3072, 3072), device=dev) for _ in range(12)]
    sums = [torch.empty((3072,), device=dev) for _ in range(12)]
    agram = [torch.empty((768, 768), device=dev) for _ in range(12)]
    asum = [torch.empty((768,), device=dev) for _ in range(12)]
    runs = {
        "plain": lambda: m.forward_into(img, logits),
        "ffn_one_block": lambda: m.activation_grams_into(
            img, blocks=(5,), gram_tensors=grams[:1], sum_tensors=sums[:1], logits=logits),
        "ffn_all_12_blocks": lambda: m.activation_grams_into(
            img, blocks=range(12), gram_tensors=grams, sum_tensors=sums, logits=logits),
        "attn_all_12_blocks": lambda: m.activation_grams_into(
            img, blocks=range(12), what="attn", gram_tensors=agram, sum_tensors=asum, logits=logits),
    }
    ms, calls = alternated(runs, rounds, window_ms)
    out = {"batch": batch, **{k: summary(v, calls[k]) for k, v in ms.items()}}
    for k in runs:
        out[k]["images_per_s_at_median"] = batch / out[k]["median_ms"] * 1e3
    return out


def bench_ab(parent_lib, rounds, limit_s):
    """bench.py, this build and the parent's alternated; a child that fails or runs past its limit
    ends the comparison (nothing more is started on the device)."""
    def run(env):
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1"],
                           capture_output=True, text=True, env={**os.environ, **env},
                           timeout=limit_s, check=True)
        return json.loads(r.stdout.strip().splitlines()[-1])["value"]
    out = {"this": [], "parent": [], "unit": "images/s"}
    try:
        for _ in range(rounds):
            out["parent"].append(run({"EVT_LIB": os.path.abspath(parent_lib)}))
            out["this"].append(run({}))
    except (subprocess.TimeoutExpired, subprocess.CalledProcessError) as e:
        out["stopped"] = f"{type(e).__name__}: {str(e)[:200]}"
        return out
    out["this_median"] = statistics.median(out["this"])
    out["parent_median"] = statistics.median(out["parent"])
    out["this_median_inside_parent_min_max"] = (min(out["parent"]) <= out["this_median"]
                                                <= max(out["parent"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gram_measure.json"))
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=150.0)
    ap.add_argument("--bench-rounds", type=int, default=4)
    ap.add_argument("--bench-limit-s", type=float, default=300.0)
    ap.add_argument("--parent-lib", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gram_measure.py needs the GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    _lib.ensure_device(0)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "rounds": a.rounds, "window_ms": a.window_ms,
           "kernel": kernel_cases(dev, a.rounds, a.window_ms),
           "forward": forward_cases(dev, a.batch, a.rounds, a.window_ms)}
    torch.cuda.empty_cache()
    res["bench"] = (bench_ab(a.parent_lib, a.bench_rounds, a.bench_limit_s) if a.parent_lib
                    else "not measured: no --parent-lib given")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
