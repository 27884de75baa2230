// Stream-delta statistics (include/evt_depth.h): how much a sublayer changed the token stream. a
// and b are row-major matrices of B T rows of D elements (model dtype, row pitches lda / ldb), row
// b T + t being token t of image b before and after the sublayer. Per token, in fp32,
//
//   dot = a_t . b_t     na2 = |a_t|^2     nb2 = |b_t|^2     dd = sum_i (b_ti - a_ti)^2
//
// (the difference element by element: formed from the three dot products it would cancel for a
// small update) and from them
//
//   cosine     dot / max(sqrt(na2 nb2), FLT_MIN)
//   rel_update sqrt(dd) / max(sqrt(na2), FLT_MIN)
//   norm_ratio sqrt(nb2) / max(sqrt(na2), FLT_MIN)
//
// out[b] = (mean_t cosine, mean_t rel_update, mean_t norm_ratio, cosine of token 0), fp32.
// sqrt(na2 nb2) is taken in fp64 (the product of two floats is exact there, and it neither
// overflows nor underflows), so b = a gives dot / sqrt(dot^2) = 1 exactly and b = -a gives -1.
//
// stream_delta_kernel. A bandwidth kernel: 2 B T D elements read once. A workgroup (4 waves) owns
// CHUNK = 16 consecutive tokens of one image; a token belongs to one 16-lane group of a wave, whose
// lane l reads the 16-byte vectors l, l + 16, ... of the token's two rows (a group reads 256
// contiguous bytes of each row per load, two vectors of each row in flight per lane) and keeps the
// four sums in registers; a 4-step butterfly inside the group leaves every lane with the row's sums
// (x + y == y + x bit for bit, so every lane holds the same bits). Lane 0 of the group forms the
// token's three values and puts them into LDS; thread 0 adds the chunk's 16 tokens in token order.
// How a token is summed depends on D alone and how tokens are combined on T alone: a result is
// bitwise reproducible and does not depend on the batch or on the image's place in it. No atomics,
// no scratch memory, LDS only for the 16 tokens' values.
//
// An image of more than CHUNK tokens is split over ceil(T / CHUNK) workgroups (13 at T = 197: one
// workgroup per image would leave three quarters of the CUs idle at 64 images); each stores its
// partial sums as one 16-byte vector into `part` [B][chunks][4], and stream_delta_finish_kernel, one
// thread per image, adds them in chunk order, divides by T and stores the image's 16 bytes. With
// T <= CHUNK the first kernel stores the result itself (the same arithmetic: one partial, / T).
//
// Edges. Tokens past T in the last chunk and lanes past D / V load nothing and contribute +0.
// Row and output offsets are 64-bit.
#include <float.h>

#include "common.h"
#include "evt_internal.h"

namespace evt {

namespace {

constexpr int WAVES = 4, GROUP = 16, CHUNK = WAVES * (64 / GROUP);
static_assert(CHUNK == STREAM_DELTA_CHUNK, "evt_internal.h sizes the partials by it");

template <typename T> struct DeltaVec;
template <> struct DeltaVec<bf16> { static constexpr int V = 8; typedef bf16x8 type; };
template <> struct DeltaVec<float> { static constexpr int V = 4; typedef f32x4 type; };

template <typename T, typename Vec>
__device__ __forceinline__ void delta_acc(const Vec& va, const Vec& vb, float& dot, float& na2,
                                          float& nb2, float& dd) {
#pragma unroll
  for (int e = 0; e < DeltaVec<T>::V; ++e) {
    const float x = (float)va[e], y = (float)vb[e], d = y - x;
    dot = __fmaf_rn(x, y, dot);
    na2 = __fmaf_rn(x, x, na2);
    nb2 = __fmaf_rn(y, y, nb2);
    dd = __fmaf_rn(d, d, dd);
  }
}

template <typename T>
__global__ __launch_bounds__(64 * WAVES) void stream_delta_kernel(
    const T* __restrict__ a, int64_t lda, const T* __restrict__ b, int64_t ldb, int tokens, int D,
    int chunks, float* __restrict__ out, int64_t ldo, float* __restrict__ part) {
  constexpr int V = DeltaVec<T>::V;
  typedef typename DeltaVec<T>::type vec_t;
  __shared__ float tok[CHUNK][4];
  const int tid = threadIdx.x, gl = tid & (GROUP - 1), slot = tid / GROUP;
  const int img = blockIdx.x / chunks, ch = blockIdx.x - img * chunks;
  const int t = ch * CHUNK + slot;

  float dot = 0.f, na2 = 0.f, nb2 = 0.f, dd = 0.f;
  if (t < tokens) {
    const int64_t row = (int64_t)img * tokens + t;
    const T* pa = a + row * lda;
    const T* pb = b + row * ldb;
    const int nv = D / V;
    for (int i = gl; i < nv; i += 2 * GROUP) {
      const bool two = i + GROUP < nv;
      const vec_t a0 = *(const vec_t*)(pa + (int64_t)i * V);
      const vec_t b0 = *(const vec_t*)(pb + (int64_t)i * V);
      vec_t a1 = a0, b1 = b0;
      if (two) {
        a1 = *(const vec_t*)(pa + (int64_t)(i + GROUP) * V);
        b1 = *(const vec_t*)(pb + (int64_t)(i + GROUP) * V);
      }
      delta_acc<T>(a0, b0, dot, na2, nb2, dd);
      if (two) delta_acc<T>(a1, b1, dot, na2, nb2, dd);
    }
  }
#pragma unroll
  for (int o = GROUP / 2; o > 0; o >>= 1) {
    dot += __shfl_xor(dot, o, 64);
    na2 += __shfl_xor(na2, o, 64);
    nb2 += __shfl_xor(nb2, o, 64);
    dd += __shfl_xor(dd, o, 64);
  }
  if (gl == 0) {
    float c = 0.f, r = 0.f, n = 0.f;
    if (t < tokens) {
      const float na = fmaxf(sqrtf(na2), FLT_MIN);
      const float den = fmaxf((float)sqrt((double)na2 * (double)nb2), FLT_MIN);
      c = dot / den;
      r = sqrtf(dd) / na;
      n = sqrtf(nb2) / na;
    }
    tok[slot][0] = c;
    tok[slot][1] = r;
    tok[slot][2] = n;
  }
  __syncthreads();
  if (tid == 0) {
    float s0 = tok[0][0], s1 = tok[0][1], s2 = tok[0][2];
#pragma unroll
    for (int k = 1; k < CHUNK; ++k) {
      s0 += tok[k][0];
      s1 += tok[k][1];
      s2 += tok[k][2];
    }
    if (chunks == 1) {
      const float n = (float)tokens;
      store_f32x4(out + (int64_t)img * ldo, f32x4{s0 / n, s1 / n, s2 / n, tok[0][0]});
    } else {  // token 0 is slot 0 of chunk 0
      store_f32x4(part + ((int64_t)img * chunks + ch) * 4,
                  f32x4{s0, s1, s2, ch == 0 ? tok[0][0] : 0.f});
    }
  }
}

__global__ __launch_bounds__(64) void stream_delta_finish_kernel(const float* __restrict__ part,
                                                                 int B, int tokens, int chunks,
                                                                 float* __restrict__ out,
                                                                 int64_t ldo) {
  const int img = blockIdx.x * 64 + threadIdx.x;
  if (img >= B) return;
  const float* p = part + (int64_t)img * chunks * 4;
  f32x4 s = *(const f32x4*)p;
  for (int c = 1; c < chunks; ++c) {
    const f32x4 v = *(const f32x4*)(p + (int64_t)c * 4);
    s[0] += v[0];
    s[1] += v[1];
    s[2] += v[2];
  }
  const float n = (float)tokens;
  store_f32x4(out + (int64_t)img * ldo, f32x4{s[0] / n, s[1] / n, s[2] / n, s[3]});
}

}  // namespace

hipError_t stream_delta_launch(int dtype, const void* a, int64_t lda, const void* b, int64_t ldb,
                               int B, int T, int D, float* out, int64_t ldo, float* part,
                               hipStream_t s) {
  const int V = dtype == DT_BF16 ? 8 : 4;
  if ((dtype != DT_BF16 && dtype != DT_F32) || !a || !b || !out || B < 1 || T < 1 ||
      T > STREAM_DELTA_MAX_TOKENS || D < 8 || D % 8 || lda < D || ldb < D || lda % V || ldb % V ||
      ldo < 4 || ldo % 4 || (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out | (uintptr_t)part) & 15))
    return hipErrorInvalidValue;
  const int chunks = (T + CHUNK - 1) / CHUNK;
  if (chunks > 1 && !part) return hipErrorInvalidValue;
  if ((int64_t)B * chunks > INT32_MAX) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(B * chunks)), block(64 * WAVES);
  if (dtype == DT_BF16)
    hipLaunchKernelGGL(stream_delta_kernel<bf16>, grid, block, 0, s, (const bf16*)a, lda,
                       (const bf16*)b, ldb, T, D, chunks, out, ldo, part);
  else
    hipLaunchKernelGGL(stream_delta_kernel<float>, grid, block, 0, s, (const float*)a, lda,
                       (const float*)b, ldb, T, D, chunks, out, ldo, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || chunks == 1) return e;
  hipLaunchKernelGGL(stream_delta_finish_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s,
                     part, B, T, chunks, out, ldo);
  return hipGetLastError();
}

}  // namespace evt
