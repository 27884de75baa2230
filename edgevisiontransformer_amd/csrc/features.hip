// Stream export: rows of the token stream (bf16 or fp32, in the workspace) -> caller-owned fp32,
// optionally through the model's final LayerNorm. The kernel behind evt_forward_features
// (include/evt_features.h): the pooled vector, the token map and the block taps.
//
// The logits path never materialises the final LayerNorm (gamma / beta are folded into the head
// weights and only the CLS rows are normalised, inside the head GEMM's epilogue), so the feature
// outputs need a pass of their own: read x[row * row_step] (width D at stride ldx; row_step = 1
// every token, row_step = T the CLS rows, the way the heads set lda = T * D), normalise, write a
// contiguous [rows, D] fp32 matrix. Padding columns [D, ldx) of a Swin stage buffer are not read.
//
// One wave64 per row, four rows per 256-thread block, grid-stride over rows. A lane loads 16 B per
// step (8 bf16 or 4 fp32) and keeps its at most 1536 / 64 = 24 values in registers. The statistics
// are the two-pass form on the values as stored: the mean, then the centred sum of squares, each
// with a butterfly wave reduction (every lane ends with the same bits). The slot statistics the
// GEMM epilogues write (ws.sx) are sums of the fp32 values BEFORE the stream's bf16 rounding and
// give E[x^2] - mean^2; the features are what a user compares against LayerNorm(x) of the stream,
// so they are computed from the stream itself. A row's arithmetic depends on its D values and on
// nothing else in the launch: pooled == tokens[:, 0] bitwise, and so is any batch permutation.
#include <algorithm>

#include "common.h"
#include "evt_internal.h"

namespace evt {

namespace {

constexpr int EXPORT_MAX_D = 1536;

__device__ __forceinline__ void load_chunk(const float* p, float (&v)[4]) {
  const f32x4 q = *(const f32x4*)p;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = q[j];
}
__device__ __forceinline__ void load_chunk(const bf16* p, float (&v)[8]) {
  const bf16x8 q = *(const bf16x8*)p;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (float)q[j];
}

// V = elements of one 16-B load; STEPS * 64 * V = EXPORT_MAX_D. D % 8 == 0, so the chunk count
// D / V is whole for both types and every chunk is 16-B aligned on both sides.
template <typename T, bool NORM>
__global__ __launch_bounds__(256) void export_rows_kernel(const T* __restrict__ x, int64_t ldx,
                                                          int64_t row_step, float* __restrict__ out,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, int rows,
                                                          int D, float eps) {
  constexpr int V = 16 / (int)sizeof(T);
  constexpr int STEPS = EXPORT_MAX_D / (64 * V);
  const int lane = threadIdx.x & 63;
  const int nch = D / V;
  for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += gridDim.x * 4) {
    const T* xr = x + (int64_t)row * row_step * ldx;
    float v[STEPS][V];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < STEPS; ++i) {
      const int c = i * 64 + lane;
      if (c < nch) {
        load_chunk(xr + c * V, v[i]);
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) v[i][j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < V; ++j) s += v[i][j];
    }
    float mean = 0.f, rstd = 1.f;
    if (NORM) {
      const float inv_d = 1.0f / (float)D;
      mean = wave_sum(s) * inv_d;
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < STEPS; ++i) {
        if (i * 64 + lane < nch) {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float d = v[i][j] - mean;
            q += d * d;
          }
        }
      }
      rstd = rsqrtf(wave_sum(q) * inv_d + eps);
    }
    float* yr = out + (int64_t)row * D;
#pragma unroll
    for (int i = 0; i < STEPS; ++i) {
      const int c = i * 64 + lane;
      if (c < nch) {
#pragma unroll
        for (int h = 0; h < V / 4; ++h) {
          const int col = c * V + h * 4;
          f32x4 o = {v[i][h * 4 + 0], v[i][h * 4 + 1], v[i][h * 4 + 2], v[i][h * 4 + 3]};
          if (NORM) o = (o - mean) * rstd * load4(gamma + col) + load4(beta + col);
          store_f32x4(yr + col, o);
        }
      }
    }
  }
}

}  // namespace

hipError_t export_rows_launch(int dtype, const void* x, int64_t ldx, int64_t row_step, float* out,
                              const float* gamma, const float* beta, int rows, int D, float eps,
                              hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  const bool norm = gamma != nullptr;
  if (!x || !out || D <= 0 || D % 8 || D > EXPORT_MAX_D || ldx < D || ldx % 8 || row_step < 1 ||
      (norm && !beta) || (((uintptr_t)x | (uintptr_t)out) & 15))
    return hipErrorInvalidValue;
  // memory bound: at most 8 blocks per CU, the rest of the rows by the grid stride
  const int grid = std::min((rows + 3) / 4, device_cus() * 8);
#define EVT_EXPORT(T, N)                                                                         \
  hipLaunchKernelGGL((export_rows_kernel<T, N>), dim3(grid), dim3(256), 0, s, (const T*)x, ldx, \
                     row_step, out, gamma, beta, rows, D, eps)
  if (dtype == DT_BF16) {
    if (norm) EVT_EXPORT(bf16, true); else EVT_EXPORT(bf16, false);
  } else {
    if (norm) EVT_EXPORT(float, true); else EVT_EXPORT(float, false);
  }
#undef EVT_EXPORT
  return hipGetLastError();
}

}  // namespace evt
