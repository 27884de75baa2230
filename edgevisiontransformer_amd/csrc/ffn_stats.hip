// FFN neuron statistics (include/evt_ffn_stats.h): a column reduction of the hidden matrix FC1
// stores, h[b T + t][j] (row-major, row pitch ld, model dtype), to four fp32 numbers per (image,
// neuron):
//
//   out[b][j] = (sum_t a / T, sum_t |a| / T, sum_t a^2 / T, max_t |a|)        a = h[b T + t][j]
//
// ffn_stats_kernel. A workgroup (4 waves) owns one image and one slab of 64 * V consecutive columns,
// V = 16 bytes of elements (8 bf16, 4 f32): a lane owns one 16-byte vector of V columns, so a wave
// reads a row of the slab as one coalesced 1 KiB load. Wave w takes rows t = w, w + 4, ... in rising
// order, four loads in flight per lane, and keeps V x 4 fp32 accumulators in registers (a^2 is formed
// inside the fused multiply-add: one rounding per term; for bf16 the product is exact anyway). The
// four waves' partials meet in LDS as [wave][statistic][column] and are combined in wave order
// ((p0 + p1) + p2) + p3 by the thread that then stores the column: thread i stores columns i,
// i + 256, ..., each as one 16-byte store, a wave writing 1 KiB of consecutive output. The order of
// every sum is fixed by (T, column) alone: a result is bitwise reproducible and does not depend on
// the batch. No atomics, no scratch memory.
//
// Edges. A lane whose first column is >= F loads nothing: ld is a multiple of V and >= F, so every
// vector that is loaded lies inside its row's pitch. The vector that straddles F loads up to V - 1
// padding columns (ld > F), whatever they hold; their accumulators reach LDS but no store: only
// columns < F are written. Rows are exactly the T of the image; with T < 4 the idle waves
// contribute their zero partials (x + 0 = x, max(x, 0) = x for x >= 0). Row and output offsets are
// 64-bit (B T ld passes 2^31 elements at DeiT-base bs512 x 6).
#include "common.h"
#include "evt_internal.h"

namespace evt {

namespace {

constexpr int WAVES = 4, UNROLL = 4;

template <typename T> struct FfnVec;
template <> struct FfnVec<bf16> { static constexpr int V = 8; typedef bf16x8 type; };
template <> struct FfnVec<float> { static constexpr int V = 4; typedef f32x4 type; };

template <typename T>
__global__ __launch_bounds__(64 * WAVES) void ffn_stats_kernel(const T* __restrict__ h, int64_t ld,
                                                               int tokens, int F, int slabs,
                                                               float* __restrict__ out) {
  constexpr int V = FfnVec<T>::V, SLAB = 64 * V;
  typedef typename FfnVec<T>::type vec_t;
  __shared__ float part[WAVES][4][SLAB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / slabs, c0 = (blockIdx.x - b * slabs) * SLAB;
  const int col = c0 + lane * V;

  float sum[V], sab[V], ssq[V], mab[V];
#pragma unroll
  for (int e = 0; e < V; ++e) sum[e] = sab[e] = ssq[e] = mab[e] = 0.f;

  if (col < F) {
    const T* src = h + ((int64_t)b * tokens) * ld + col;
    for (int t0 = wave; t0 < tokens; t0 += WAVES * UNROLL) {
      vec_t v[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int t = t0 + u * WAVES;  // wave-uniform
        if (t < tokens) v[u] = *(const vec_t*)(src + (int64_t)t * ld);
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        if (t0 + u * WAVES < tokens) {
#pragma unroll
          for (int e = 0; e < V; ++e) {
            const float a = (float)v[u][e];
            sum[e] += a;
            sab[e] += fabsf(a);
            ssq[e] = __fmaf_rn(a, a, ssq[e]);
            mab[e] = fmaxf(mab[e], fabsf(a));
          }
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) {
    part[wave][0][lane * V + e] = sum[e];
    part[wave][1][lane * V + e] = sab[e];
    part[wave][2][lane * V + e] = ssq[e];
    part[wave][3][lane * V + e] = mab[e];
  }
  __syncthreads();

  const float n = (float)tokens;
  float* dst = out + (int64_t)b * F * 4;
#pragma unroll
  for (int c = tid; c < SLAB; c += 64 * WAVES) {
    if (c0 + c < F) {
      float r[4];
#pragma unroll
      for (int s = 0; s < 3; ++s)
        r[s] = ((part[0][s][c] + part[1][s][c]) + part[2][s][c]) + part[3][s][c];
      r[3] = fmaxf(fmaxf(fmaxf(part[0][3][c], part[1][3][c]), part[2][3][c]), part[3][3][c]);
      store_f32x4(dst + (int64_t)(c0 + c) * 4, f32x4{r[0] / n, r[1] / n, r[2] / n, r[3]});
    }
  }
}

}  // namespace

hipError_t ffn_stats_launch(int dtype, const void* h, int64_t ld, int B, int T, int F, float* out,
                            hipStream_t s) {
  if (B <= 0) return hipSuccess;
  const int V = dtype == DT_BF16 ? 8 : 4;
  if ((dtype != DT_BF16 && dtype != DT_F32) || !h || !out || T < 1 || T > FFN_STATS_MAX_TOKENS ||
      F < 1 || ld < F || ld % V || (((uintptr_t)h | (uintptr_t)out) & 15))
    return hipErrorInvalidValue;
  const int slabs = (F + 64 * V - 1) / (64 * V);
  if ((int64_t)B * slabs > INT32_MAX) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(B * slabs)), block(64 * WAVES);
  if (dtype == DT_BF16)
    hipLaunchKernelGGL(ffn_stats_kernel<bf16>, grid, block, 0, s, (const bf16*)h, ld, T, F,
                       slabs, out);
  else
    hipLaunchKernelGGL(ffn_stats_kernel<float>, grid, block, 0, s, (const float*)h, ld, T, F,
                       slabs, out);
  return hipGetLastError();
}

}  // namespace evt
