// ---------------------------------------------------------------------------------------------
// Large-tile bf16 kernel: 256x256 output tile, BK = 64, 512 threads = 8 waves in 2 (m) x 4 (n),
// each wave a 128 (m) x 64 (n) sub-tile = 8 x 4 MFMA tiles (128 fp32 accumulators per lane).
// 128 KiB LDS (2 buffers x {A 32 KiB, W 32 KiB}), one block per CU; one barrier per K-tile.
// VAR 6 (default): after the barrier, k-step-0 fragments are read, the 8 DMA pieces of the next
// K-tile are spread between the first 16 MFMAs and the k-step-1 reads between the next 12
// (sched_group_barrier), so the DMA issue and LDS latency hide under MFMA issue.
// VAR 0: the same without the explicit issue order (kept for A/B measurements).
// ---------------------------------------------------------------------------------------------
#pragma once
#include "gemm_big8.h"

namespace evt {

namespace {

// Epilogue of the 256x256 kernels: two passes staged through the (idle) 128 KiB of LDS; in
// pass h every wave hands over its column tiles nt = 2h, 2h+1 (half of its accumulators die per
// pass) and all 8 waves then stream 32 rows each of the staged 256 x 128 slab. Stats slot of
// pass h: 2*tn + h. The wave's 128 x 64 sub-tile is rows wm*128.., columns wn*64...
template <int FL>
__device__ __forceinline__ void big_epilogue(const GemmParams& p, char* smem, f32x4 (&acc)[4][8],
                                             int wm, int wn, int m0, int n0, int tn, int wave,
                                             int lane) {
  EVT_LDS char* stg = (EVT_LDS char*)smem;
  const bool interior = p.vec_ok && (n0 + BIG_BN <= p.N) && (m0 + BIG_BM <= p.M);
  const int c = lane & 31, frow = lane & 15, fg = lane >> 4;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    __builtin_amdgcn_s_barrier();  // previous readers of the staging area are done
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int mt = 0; mt < 8; ++mt) {
        const int row = wm * 128 + mt * 16 + frow;
        *(EVT_LDS f32x4*)(stg + stg_off(row, wn * 8 + t * 4 + fg)) = acc[2 * h + t][mt];
      }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
    // staged chunk c holds global columns n0 + (c>>3)*64 + h*32 + (c&7)*4 .. +3
    // (8-column layout: lane chunks 2 c8, 2 c8 + 1 -> n0 + (c8>>2)*64 + h*32 + (c8&3)*8 .. +7)
    const int c8 = lane & 15;
    epi_rows<bf16, FL, true>(p, stg, m0, n0 + (c >> 3) * 64 + h * 32 + (c & 7) * 4,
                       n0 + (c8 >> 2) * 64 + h * 32 + (c8 & 3) * 8, wave * 32, lane, 2 * tn + h,
                       interior);
    __builtin_amdgcn_s_waitcnt(0xC07F);
  }
}

template <int FL, int VAR>
__global__ __launch_bounds__(512, 2) void gemm_big_kernel(GemmParams p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * BIG_STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably uniform -> SGPR math
  // VAR 8 pairs the two waves of a SIMD across the wave groups wm = 0 / 1 (waves w, w + 4)
  const int wm = VAR == 8 ? wave >> 2 : wave & 1, wn = VAR == 8 ? wave & 3 : wave >> 1;
  const int wgid = xcd_remap(blockIdx.x, gridDim.x);
  const int tm = wgid / p.ntiles, tn = wgid - tm * p.ntiles;
  const int m0 = tm * BIG_BM, n0 = tn * BIG_BN;

  const int srow = lane >> 3, sslot = lane & 7;
  const int64_t lda_b = p.lda * 2, ldw_b = p.ldw * 2;
  // Addresses are recomputed per stage (a few VALU ops) instead of held in 16 VGPRs.
  const int arow0 = m0 + wave * 32 + srow;
  const char* a_base = (const char*)p.A + ((sslot ^ srow) * 16);
  const char* w_base = (const char*)p.W + (int64_t)(n0 + wave * 32 + srow) * ldw_b + ((sslot ^ srow) * 16);
  auto stage = [&](int kt, int buf) {
    EVT_LDS char* base = (EVT_LDS char*)smem + buf * BIG_STAGE;
    const int64_t koff = (int64_t)kt * ROWB;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gm = min(arow0 + i * 8, p.M - 1);
      glds16(a_base + gm * lda_b + koff, base + (wave * 32 + i * 8) * ROWB);
      glds16(w_base + (i * 8) * ldw_b + koff, base + BIG_TILE + (wave * 32 + i * 8) * ROWB);
    }
  };

  f32x4 acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = p.K / 64;
  const int frow = lane & 15, fsw = lane & 7, fg = lane >> 4;
  auto read_step = [&](int kt, int ks, u32x4 (&a)[8], u32x4 (&w)[4]) {
    const EVT_LDS char* As = (const EVT_LDS char*)smem + (kt & 1) * BIG_STAGE;
    const EVT_LDS char* Ws = As + BIG_TILE;
    const int coff = ((fg + 4 * ks) ^ fsw) * 16;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
      w[nt] = *(const EVT_LDS u32x4*)(Ws + (wn * 64 + nt * 16 + frow) * ROWB + coff);
#pragma unroll
    for (int mt = 0; mt < 8; ++mt)
      a[mt] = *(const EVT_LDS u32x4*)(As + (wm * 128 + mt * 16 + frow) * ROWB + coff);
  };
  auto mfma_step = [&](const u32x4 (&a)[8], const u32x4 (&w)[4]) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int mt = 0; mt < 8; ++mt) Mma<bf16>::run(w[nt], a[mt], acc[nt][mt]);
  };
  if constexpr (VAR == 8) {
    big8_prologue(p, smem, wave, lane, m0, n0, nk);
    big8_loop<0>(p, smem, acc, wave, lane, wm, wn, m0, n0, nk);
  } else {
  stage(0, 0);
  if constexpr (VAR == 6) {
    auto tile = [&](int kt, bool dma) {
      wait_vmcnt0();
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      u32x4 a0[8], w0[4], a1[8], w1[4];
      read_step(kt, 0, a0, w0);
      if (dma) stage(kt + 1, (kt + 1) & 1);
      read_step(kt, 1, a1, w1);
      mfma_step(a0, w0);
      mfma_step(a1, w1);
      __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);  // DS read
      if (dma) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // MFMA
          __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);  // VMEM (glds)
        }
      } else {
        __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
      }
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 36, 0);
      __builtin_amdgcn_sched_barrier(0);
    };
    for (int kt = 0; kt + 1 < nk; ++kt) tile(kt, true);
    tile(nk - 1, false);
  } else {
    for (int kt = 0; kt < nk; ++kt) {
      wait_vmcnt0();
      __builtin_amdgcn_s_barrier();
      if (kt + 1 < nk) stage(kt + 1, (kt + 1) & 1);
      u32x4 a[8], w[4];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        read_step(kt, ks, a, w);
        mfma_step(a, w);
      }
    }
  }
  }

  big_epilogue<FL>(p, smem, acc, wm, wn, m0, n0, tn, wave, lane);
}

}  // namespace

}  // namespace evt
