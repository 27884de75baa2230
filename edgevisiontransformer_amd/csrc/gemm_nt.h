// ---------------------------------------------------------------------------------------------
// 128x128 tile kernel (bf16 and f32): 256 threads = 4 waves in 2 (m) x 2 (n), 64x64 per wave,
// 2-stage glds double buffer (64 KiB), two blocks per CU.
// ---------------------------------------------------------------------------------------------
#pragma once
#include "gemm_epi.h"

namespace evt {

namespace {

template <typename T, int FL>
__global__ __launch_bounds__(256, 2) void gemm_nt_kernel(GemmParams p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_BYTES];
  if (gridDim.y > 1) {  // split-K (gemm_splitk_launch): this block's K range and partial C
    const int z = blockIdx.y;
    p.A = (const T*)p.A + (int64_t)z * p.ks_chunk;
    p.W = (const T*)p.W + (int64_t)z * p.ks_chunk;
    p.K = p.ks_chunk;
    p.C = (float*)p.C + (int64_t)z * p.ks_stride;
  }

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably uniform -> SGPR math
  const int wm = wave & 1, wn = wave >> 1;
  const int wgid = xcd_remap(blockIdx.x, gridDim.x);
  const int tm = wgid / p.ntiles, tn = wgid - tm * p.ntiles;
  const int m0 = tm * GEMM_BM, n0 = tn * GEMM_BN;

  // ---- staging: wave stages rows [wave*32, wave*32+32) of both tiles ----
  const int srow = lane >> 3, sslot = lane & 7;
  const int64_t lda_b = p.lda * (int64_t)sizeof(T), ldw_b = p.ldw * (int64_t)sizeof(T);
  const int arow0 = m0 + wave * 32 + srow;
  const char* a_base = (const char*)p.A + ((sslot ^ srow) * 16);
  const char* w_base = (const char*)p.W + (int64_t)(n0 + wave * 32 + srow) * ldw_b + ((sslot ^ srow) * 16);
  auto stage = [&](int kt, int buf) {
    EVT_LDS char* base = (EVT_LDS char*)smem + buf * STAGE_BYTES;
    const int64_t koff = (int64_t)kt * ROWB;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gm = min(arow0 + i * 8, p.M - 1);
      glds16(a_base + gm * lda_b + koff, base + (wave * 32 + i * 8) * ROWB);
      glds16(w_base + (i * 8) * ldw_b + koff, base + TILE_BYTES + (wave * 32 + i * 8) * ROWB);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = p.K * (int)sizeof(T) / ROWB;
  stage(0, 0);
  const int frow = lane & 15, fsw = lane & 7, fg = lane >> 4;
  // f32 with EPI_LNIN: the A fragments are centred (x - mu, mu from the row's statistics) before
  // the product. The folded form r acc - r mu colsum subtracts two fp32 sums of ~|mu| |colsum|
  // whose rounding (a few 1e-6 over K = 768) r then multiplies: up to 1 / sqrt(eps) = 316 on a
  // constant row, 2e-3 against the 1e-3 this path promises. bf16 keeps the folded form (the
  // products are exact in fp32 there and its tolerance is 100 times wider). Columns past K are
  // zero in Wp, so the -mu they pick up contributes nothing.
  constexpr bool CENTER = std::is_same<T, float>::value && (FL & EPI_LNIN) != 0;
  float amu[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (CENTER) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int mr = min(m0 + wm * 64 + mt * 16 + frow, p.M - 1);
      float r_unused;
      ln_coef(p.stats_in, p.nslots, (int64_t)mr * (p.stats_step > 1 ? p.stats_step : 1), p.inv_d,
              p.eps, amu[mt], r_unused);
    }
  }
  for (int kt = 0; kt < nk; ++kt) {
    wait_vmcnt0();
    __syncthreads();
    if (kt + 1 < nk) stage(kt + 1, (kt + 1) & 1);
    const EVT_LDS char* As = (const EVT_LDS char*)smem + (kt & 1) * STAGE_BYTES;
    const EVT_LDS char* Ws = As + TILE_BYTES;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int coff = ((fg + 4 * kk) ^ fsw) * 16;
      u32x4 a[4], w[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
        a[mt] = *(const EVT_LDS u32x4*)(As + (wm * 64 + mt * 16 + frow) * ROWB + coff);
      if constexpr (CENTER) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
          a[mt] = __builtin_bit_cast(u32x4, __builtin_bit_cast(f32x4, a[mt]) - amu[mt]);
      }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        w[nt] = *(const EVT_LDS u32x4*)(Ws + (wn * 64 + nt * 16 + frow) * ROWB + coff);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) Mma<T>::run(w[nt], a[mt], acc[nt][mt]);
    }
  }

  // ---- stage the 128x128 fp32 tile (exactly the 64 KiB of LDS), then row-major epilogue ----
  __syncthreads();
  EVT_LDS char* stg = (EVT_LDS char*)smem;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int row = wm * 64 + mt * 16 + frow;
      *(EVT_LDS f32x4*)(stg + stg_off(row, wn * 16 + nt * 4 + fg)) = acc[nt][mt];
    }
  __syncthreads();
  const bool interior = p.vec_ok && (n0 + GEMM_BN <= p.N) && (m0 + GEMM_BM <= p.M);
  epi_rows<T, FL>(p, stg, m0, n0 + (lane & 31) * 4, n0 + (lane & 15) * 8, wave * 32, lane,
                  n0 / 128, interior);
}

}  // namespace

}  // namespace evt
