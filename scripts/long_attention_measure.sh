#!/bin/bash
# The measurements DESIGN.md quotes for attention beyond 256 tokens, on one MI355X, in one run:
#   1. the bf16 streaming kernel against torch SDPA (flash) at B 64, H 12, N 577, head 64
#   2. the gpu_benchmark line of DeiT-base at 64 x 3 x 384 x 384
#   3. the per-role profile of that forward
# Results are appended to $OUT (default long_attention_results.txt); summaries worth keeping are
# copied into profiles/ by hand. Every GPU step has its own time limit; the first failure stops
# the script (pipefail: a step that fails in front of its tee fails the chain).
set -u
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-long_attention_results.txt}
export PYTHONDONTWRITEBYTECODE=1
timeout -k 10 240 python -u scripts/long_attention_bench.py --out "$OUT" &&
timeout -k 10 300 python -u -m edgevisiontransformer_amd.tools gpu_benchmark --model deit_base \
    --input_shape 64,3,384,384 --io_binding --num_runs 30 --warmup_runs 10 --precision 3 | tee -a "$OUT" &&
timeout -k 10 300 python -u scripts/long_model_profile.py --model deit_base --batch 64 \
    --image_size 384 --out "$OUT"
