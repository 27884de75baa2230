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

// ---- classification outputs (include/evt_classify.h) --------------------------------------------
//
// logits [B, C] (fp32, rows ldl apart, 4-byte aligned) -> the ordered top-k classes, their
// probabilities or logits, the log-sum-exp, the label's rank and the hit counters.
//
// The order of the header (l_i > l_j, ties and -0.0 / +0.0 by index, NaN last) is the descending
// order of one 64-bit integer per class: the usual monotone map of the float's bits (zeros folded
// to +0, NaN to 0, below -inf) in the high word and ~index in the low word. Every class of a row
// has a different key, so the j-th class is the largest key below the (j-1)-th: selection keeps no
// state but the previous winner, integer maxima are exact in any order, and the rank of a label is
// the number of keys above its own. All of it is integer work: it does not depend on the float
// mode the file is compiled with.
//
// One wave64 per row, four rows per 256-thread block, grid-stride over rows, as above. A lane owns
// the 4-class chunks lane, lane + 64, ... of its row whatever the row's alignment (one 16-byte load
// when the row start is 16-byte aligned and the chunk is whole, dword loads otherwise): the order
// in which a lane adds its exponentials is a function of C alone, so a row gives the same bits at
// any batch position. Round 0 of the selection finds the row maximum m; the sum of exp(l - m) is
// then one more pass over the (L1 / L2 resident) row with m exact, which needs no running-max
// rescaling and no guard beyond m itself: exp(-inf - m) is exactly 0 for a finite m. k + 1 reads
// of the row (+ 1 with labels), the same as an online first pass followed by k rounds.
constexpr unsigned long long CLS_NO_KEY = ~0ull;  // above every key (no class has index 2^32-1)

__device__ __forceinline__ unsigned long long cls_key(unsigned bits, int idx) {
  unsigned k;
  if ((bits & 0x7fffffffu) > 0x7f800000u) k = 0u;            // NaN: after -inf
  else if ((bits << 1) == 0u) k = 0x80000000u;               // -0.0 == +0.0
  else k = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  return ((unsigned long long)k << 32) | (unsigned)(~(unsigned)idx);
}
__device__ __forceinline__ int cls_key_index(unsigned long long key) {
  return (int)(~(unsigned)(key & 0xffffffffu));
}

// f(class, bits) for every class of the lane's chunks, in rising class order
template <typename F>
__device__ __forceinline__ void cls_scan(const unsigned* __restrict__ row, int C, bool al16,
                                         int lane, F&& f) {
  const int nch = (C + 3) >> 2;
  for (int ch = lane; ch < nch; ch += 64) {
    const int c0 = ch * 4;
    if (al16 && c0 + 3 < C) {
      const u32x4 q = *(const u32x4*)(row + c0);
#pragma unroll
      for (int j = 0; j < 4; ++j) f(c0 + j, q[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < C) f(c0 + j, row[c0 + j]);
    }
  }
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void classify_kernel(
    const float* __restrict__ logits, int64_t ldl, int B, int C, int k, int values,
    int* __restrict__ indices, float* __restrict__ vals, float* __restrict__ lse,
    const int* __restrict__ labels, int* __restrict__ rank,
    unsigned long long* __restrict__ counters) {
  __shared__ int hits[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool want_sum = lse != nullptr || (vals != nullptr && values == CLS_PROB);
  int n_valid = 0, n_top1 = 0, n_topk = 0;  // of this wave's rows (wave-uniform)
  for (int b = blockIdx.x * 4 + wave; b < B; b += gridDim.x * 4) {
    const float* rowf = logits + (int64_t)b * ldl;
    const unsigned* row = (const unsigned*)rowf;
    const bool al16 = ((uintptr_t)row & 15) == 0;
    // selection: lane j keeps the j-th key
    unsigned long long prev = CLS_NO_KEY, mine = 0ull;
    float m = 0.f, s = 1.f;
    for (int j = 0; j < k; ++j) {
      unsigned long long best = 0ull;
      cls_scan(row, C, al16, lane, [&](int c, unsigned bits) {
        const unsigned long long key = cls_key(bits, c);
        if (key < prev && key > best) best = key;
      });
      prev = wave_max_u64(best);
      if (lane == j) mine = prev;
      if (j == 0 && want_sum) {
        m = rowf[cls_key_index(prev)];
        float acc = 0.f;
        cls_scan(row, C, al16, lane,
                 [&](int, unsigned bits) { acc += expf(__uint_as_float(bits) - m); });
        s = wave_sum(acc);
      }
    }
    if (lane < k && (indices || vals)) {
      const int c = cls_key_index(mine);
      const int64_t o = (int64_t)b * k + lane;
      if (indices) indices[o] = c;
      if (vals) {
        const float l = rowf[c];
        vals[o] = values == CLS_LOGIT ? l : expf(l - m) / s;
      }
    }
    if (lse && lane == 0) lse[b] = m + logf(s);
    if (labels) {
      const int y = labels[b];
      int r = -1;
      if (y >= 0 && y < C) {
        const unsigned long long ky = cls_key(row[y], y);
        int above = 0;
        cls_scan(row, C, al16, lane,
                 [&](int c, unsigned bits) { above += cls_key(bits, c) > ky ? 1 : 0; });
        r = wave_sum_i32(above);
        n_valid += 1;
        n_top1 += r < 1 ? 1 : 0;
        n_topk += r < k ? 1 : 0;
      }
      if (rank && lane == 0) rank[b] = r;
    }
  }
  if (counters) {  // one 64-bit integer add per block and counter (exact, order-independent)
    if (lane == 0) {
      hits[wave][0] = n_valid;
      hits[wave][1] = n_top1;
      hits[wave][2] = n_topk;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      const int n = hits[0][threadIdx.x] + hits[1][threadIdx.x] + hits[2][threadIdx.x] +
                    hits[3][threadIdx.x];
      if (n) atomicAdd(counters + threadIdx.x, (unsigned long long)n);
    }
  }
}

}  // namespace

hipError_t classify_launch(const float* logits, int64_t ldl, int B, int C,
                           const ClassifyParams& a, hipStream_t s) {
  if (!logits || B < 1 || C < 1 || C > (1 << 20) || ldl < C || a.k < 1 || a.k > C ||
      a.k > CLS_MAX_K ||
      (a.values != CLS_PROB && a.values != CLS_LOGIT) ||
      ((a.rank || a.counters) && !a.labels) ||
      (((uintptr_t)logits | (uintptr_t)a.indices | (uintptr_t)a.vals | (uintptr_t)a.lse |
        (uintptr_t)a.labels | (uintptr_t)a.rank) & 3) || ((uintptr_t)a.counters & 7))
    return hipErrorInvalidValue;
  const int grid = std::min((B + 3) / 4, device_cus() * 8);
  hipLaunchKernelGGL(classify_kernel, dim3(grid), dim3(256), 0, s, logits, ldl, B, C, a.k,
                     a.values, a.indices, a.vals, a.lse, a.labels, a.rank,
                     (unsigned long long*)a.counters);
  return hipGetLastError();
}

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
