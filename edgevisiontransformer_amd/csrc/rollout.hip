// Attention rollout (include/evt_rollout.h): the batched fp32 matrix step
//
//   R_out[b] = 0.5 (R_in[b] + Abar[b] @ R_in[b])          Abar, R_in: [B][N][N] fp32
//
// of Abar = the head mean of a block's attention probabilities (head_mean_kernel, attn_maps.hip)
// and the rollout so far. With Ahat = 0.5 (Abar + I) this is Ahat @ R_in; the identity's share is
// added as R_in itself, so no N x N identity is ever formed or multiplied. The first step has
// R_in = I: rollout_first_kernel reads no R_in and writes 0.5 (Abar + I).
//
// rollout_step_kernel. A workgroup (4 waves) owns a 64 x 64 tile of one image's R_out, a wave a
// 32 x 32 quadrant as 2 x 2 tiles of the exact v_mfma_f32_16x16x4_f32 (fp32 operands, fp32
// accumulator: a k-ordered fmaf chain, one rounding per term; four independent accumulators per
// wave cover the instruction's 40-cycle dependent latency). K runs over 32-token chunks: the 64 x 32
// piece of Abar and the 32 x 64 piece of R_in go through registers into LDS (the loads of chunk
// i + 1 are issued before the MFMAs of chunk i), Abar rows padded to 36 floats (16-B aligned, one
// ds_read_b128 gives a lane its four k of a 16-k group), R_in rows to 68 (the lane groups of a
// ds_read_b32 land 16 banks apart). Within a 16-k group lane group g takes k = 4 g + e in MFMA
// e = 0 .. 3, for the A and the B operand alike: a fixed order, so a result is bitwise reproducible
// and does not depend on the batch position.
//
// N is arbitrary (197, 257, 577 are no tile multiples, and rows start 16-B aligned one time in
// four, so every global access of the step kernel is one float). A row, column or k past N is
// never read: its LDS element is a literal 0 (0 * 0 adds +0 to a non-negative sum), and never
// written. nq = N stores every row; nq = 1 launches the first tile row only, loads row 0 of Abar
// alone and stores row 0 [B][N]: MFMA rows are independent, so it is bitwise row 0 of the nq = N
// result.
//
// Epilogue: the accumulators go through LDS (the operand tiles' space, 64 x 68 floats) so that a wave
// reads R_in and writes R_out by row segments, a lane per float, 256 contiguous bytes per wave
// instruction. R_in and R_out must not overlap: every row of R_in is an operand of every tile.
// All image, row and output offsets are 64-bit (B N^2 passes 2^31 at ordinary sizes).
#include "common.h"
#include "evt_internal.h"

namespace evt {

namespace {

constexpr int TM = 64, TN = 64, TK = 32;
constexpr int AS = TK + 4;  // floats per LDS row of the Abar tile
constexpr int RS = TN + 4;  // floats per LDS row of the R_in tile and of the result tile
static_assert(TM * AS + TK * RS >= TM * RS, "the result tile overlays the operand tiles");

__global__ __launch_bounds__(256) void rollout_step_kernel(const float* __restrict__ abar,
                                                           const float* __restrict__ r_in,
                                                           float* __restrict__ r_out, int N, int nq,
                                                           int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(16))) float smem[TM * AS + TK * RS];
  float* As = smem;            // [64 rows][AS]: Abar[m0 + row][k0 + k]
  float* Rs = smem + TM * AS;  // [32 k][RS]:    R_in[k0 + k][n0 + col]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c16 = lane & 15;
  const int wr = wave >> 1, wc = wave & 1;
  const int per = tiles_m * tiles_n;
  const int b = blockIdx.x / per, t = blockIdx.x - b * per;
  const int m0 = (t / tiles_n) * TM, n0 = (t % tiles_n) * TN;
  const float* A = abar + (int64_t)b * N * N;
  const float* R = r_in + (int64_t)b * N * N;

  // this thread's 8 + 8 elements of a chunk: Abar (row i * 8 + tid / 32, k tid % 32) and R_in
  // (k i * 4 + tid / 64, column tid % 64); rows >= nq of Abar are not needed and not read
  float ra[8], rr[8];
  const int ar = tid >> 5, ak = tid & 31, rk = tid >> 6, rc = tid & 63;
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = m0 + i * 8 + ar, k = k0 + ak;
      ra[i] = (row < nq && k < N) ? A[(int64_t)row * N + k] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = k0 + i * 4 + rk, col = n0 + rc;
      rr[i] = (k < N && col < N) ? R[(int64_t)k * N + col] : 0.f;
    }
  };

  f32x4 acc[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  load(0);
  for (int k0 = 0; k0 < N; k0 += TK) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      As[(i * 8 + ar) * AS + ak] = ra[i];
      Rs[(i * 4 + rk) * RS + rc] = rr[i];
    }
    __syncthreads();
    if (k0 + TK < N) load(k0 + TK);  // in flight under the MFMAs below
#pragma unroll
    for (int kg = 0; kg < TK / 16; ++kg) {
      f32x4 a[2];
      float bv[2][4];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
        a[mt] = *(const f32x4*)(As + (32 * wr + 16 * mt + c16) * AS + 16 * kg + 4 * g);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          bv[nt][e] = Rs[(16 * kg + 4 * g + e) * RS + 32 * wc + 16 * nt + c16];
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][e], bv[nt][e], acc[mt][nt], 0, 0, 0);
    }
    __syncthreads();  // every wave is done with the chunk before the next one (or the result) lands
  }

  // acc[mt][nt][j] = (Abar @ R_in)[m0 + 32 wr + 16 mt + 4 g + j][n0 + 32 wc + 16 nt + c16]
  float* Cs = smem;  // [64][RS]
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        Cs[(32 * wr + 16 * mt + 4 * g + j) * RS + 32 * wc + 16 * nt + c16] = acc[mt][nt][j];
  __syncthreads();
  const int col = n0 + lane;
  float* O = r_out + (int64_t)b * nq * N;
  for (int r = 0; r < 16; ++r) {
    const int row = m0 + 16 * wave + r;
    if (row >= nq) break;  // wave-uniform
    if (col < N) {
      const int64_t e = (int64_t)row * N + col;
      O[e] = 0.5f * (R[e] + Cs[(16 * wave + r) * RS + lane]);
    }
  }
}

// R_in = I: r_out[b][i][j] = 0.5 (abar[b][i][j] + (i == j)), i < nq. One workgroup per row. VEC: N
// is a multiple of 4 and both bases are 16-B aligned, so every row is: 16-B loads and stores (the
// same values, element by element, as the dword form).
template <bool VEC>
__global__ __launch_bounds__(256) void rollout_first_kernel(const float* __restrict__ abar,
                                                            float* __restrict__ r_out, int N,
                                                            int nq) {
  const int64_t bi = blockIdx.x;  // b * nq + i
  const int64_t b = bi / nq;
  const int i = (int)(bi - b * nq);
  const float* src = abar + (b * N + i) * N;
  float* dst = r_out + bi * N;
  if constexpr (VEC) {
    for (int j = 4 * threadIdx.x; j < N; j += 4 * 256) {
      f32x4 v = *(const f32x4*)(src + j);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = 0.5f * (v[e] + (i == j + e ? 1.f : 0.f));
      store_f32x4(dst + j, v);
    }
  } else {
    for (int j = threadIdx.x; j < N; j += 256) dst[j] = 0.5f * (src[j] + (i == j ? 1.f : 0.f));
  }
}

}  // namespace

hipError_t rollout_step_launch(const float* abar, const float* r_in, float* r_out, int B, int N,
                               int nq, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (!abar || !r_out || N <= 0 || N > EVT_ATTN_MAX_TOKENS || (nq != 1 && nq != N))
    return hipErrorInvalidValue;
  if (!r_in) {
    if ((int64_t)B * nq > INT32_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(B * nq)), block(256);
    if (N % 4 == 0 && !(((uintptr_t)abar | (uintptr_t)r_out) & 15))
      hipLaunchKernelGGL(rollout_first_kernel<true>, grid, block, 0, s, abar, r_out, N, nq);
    else
      hipLaunchKernelGGL(rollout_first_kernel<false>, grid, block, 0, s, abar, r_out, N, nq);
    return hipGetLastError();
  }
  const int tiles_m = (nq + TM - 1) / TM, tiles_n = (N + TN - 1) / TN;
  if ((int64_t)B * tiles_m * tiles_n > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rollout_step_kernel, dim3((unsigned)(B * tiles_m * tiles_n)), dim3(256), 0, s,
                     abar, r_in, r_out, N, nq, tiles_m, tiles_n);
  return hipGetLastError();
}

}  // namespace evt
