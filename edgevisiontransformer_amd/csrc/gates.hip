// Structured gates (include/evt_gates.h): the one launch that runs when the gates of a block's
// heads or FFN neurons change (model.cpp set_gates) and the op-level entry point of the tests.
//
//   w[n][k] = round_dtype(g[k] * w0[n][k])      n < rows, k < kpad
//
// over a packed Dense weight [rows][kpad] (DenseW::w, K contiguous, kpad a multiple of 64): w0 is
// the pristine copy, g the fp32 gate of every K column (a head's gate repeated over its head_dim
// columns, or one per FFN neuron; 1 in the K padding). The product is one fp32 multiply and the
// rounding is from_f32<T> (common.h), the conversion pack_kernel (gemm.hip) packs a weight with:
// the result is bitwise what make_dense stores for the weight fl(g[k] * w0[n][k]). 0 * a negative
// weight is -0.0 here and there.
//
// A thread per 16-byte chunk (4 fp32 / 8 bf16 elements), grid-stride over at most GATE_MAX_BLOCKS
// workgroups: a chunk never crosses a row since kpad * sizeof(T) is a multiple of 16, and its gates
// are 16 or 32 contiguous bytes of g, which stays in L2 (kpad floats). Plain vector loads, one
// 16-byte store through the common.h helper, no atomics: one result whatever the timing. The
// kernel is bandwidth bound and small (DeiT-base: 1.2 MB out-proj, 4.7 MB FC2, read once and
// written once).
#include <algorithm>
#include <cstdint>

#include "common.h"
#include "evt_internal.h"

namespace evt {

namespace {

constexpr int GATE_MAX_BLOCKS = 2048;  // 256 CUs x 8 workgroups; the rest is the grid stride

template <typename T>
__global__ __launch_bounds__(256) void gate_weights_kernel(const u32x4* __restrict__ w0,
                                                           u32x4* __restrict__ w,
                                                           const float* __restrict__ g, int cpr,
                                                           int64_t total) {
  constexpr int E = 16 / (int)sizeof(T);  // elements of a chunk
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < total; c += step) {
    const int cc = (int)(c % cpr);  // the chunk's place in its row
    const u32x4 v = w0[c];
    const float* gp = g + cc * E;
    if constexpr (E == 4) {
      const f32x4 x = __builtin_bit_cast(f32x4, v), gv = *(const f32x4*)gp;
      const f32x4 o = {gv[0] * x[0], gv[1] * x[1], gv[2] * x[2], gv[3] * x[3]};
      store_f32x4((float*)(w + c), o);
    } else {
      const bf16x8 x = __builtin_bit_cast(bf16x8, v);
      const f32x4 g0 = *(const f32x4*)gp, g1 = *(const f32x4*)(gp + 4);
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = from_f32<bf16>(g0[j] * to_f32(x[j]));
        o[4 + j] = from_f32<bf16>(g1[j] * to_f32(x[4 + j]));
      }
      store_bf16x8((bf16*)(w + c), o);
    }
  }
}

}  // namespace

hipError_t gate_weights_launch(int dtype, const void* w0, void* w, const float* g, int rows,
                               int kpad, hipStream_t s) {
  if (rows == 0) return hipSuccess;
  if ((dtype != DT_BF16 && dtype != DT_F32) || !w0 || !w || !g || rows < 0 || kpad < PAD_K ||
      kpad % PAD_K || (((uintptr_t)w0 | (uintptr_t)w | (uintptr_t)g) & 15))
    return hipErrorInvalidValue;
  const int cpr = kpad / (dtype == DT_BF16 ? 8 : 4);
  const int64_t total = (int64_t)rows * cpr;
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, GATE_MAX_BLOCKS);
  if (dtype == DT_BF16)
    hipLaunchKernelGGL(gate_weights_kernel<bf16>, dim3(grid), dim3(256), 0, s, (const u32x4*)w0,
                       (u32x4*)w, g, cpr, total);
  else
    hipLaunchKernelGGL(gate_weights_kernel<float>, dim3(grid), dim3(256), 0, s, (const u32x4*)w0,
                       (u32x4*)w, g, cpr, total);
  return hipGetLastError();
}

}  // namespace evt
