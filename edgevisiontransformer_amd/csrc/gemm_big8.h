// ---------------------------------------------------------------------------------------------
// 8-phase ping-pong main loop (VAR 8 of gemm_big_kernel, and gemm_pers_kernel).
// Four phases per K-tile. Each K-tile buffer is split into four 16 KiB regions: j = 0 A rows of
// m-half 0 (of both wm), 1 W rows of n-half 0 (of all wn), 2 W n-half 1, 3 A m-half 1, read in
// phases 1 / 1 / 2 / 3 of the tile (the wave's 128 x 64 sub-tile is done as four 64 x 32
// quadrants, B n-half 0 stays in registers for the 4th). Region s = 4 T + j is DMA'd (2 glds
// per lane) in global phase s - 6, i.e. into the buffer still being read, two or more phases
// after the region's last read (WAR), and retired by a counted vmcnt before the first barrier
// of the phase preceding its first read (RAW): every DMA gets about one K-tile of flight time
// and 8 glds per lane stay in flight. Wave group wm = 1 runs one barrier behind group 0, so
// while one group issues MFMAs (at raised priority) the other issues ds_reads and DMAs on the
// same SIMD (waves w and w + 4 share a SIMD).
// ---------------------------------------------------------------------------------------------
#pragma once
#include "gemm_epi.h"

namespace evt {

namespace {

// 256 x 256 tile of gemm_big_kernel / gemm_pers_kernel; 64 KiB K-tile stages for every geometry
constexpr int BIG_BM = 256, BIG_BN = 256;
constexpr int BIG_TILE = BIG_BM * ROWB;       // 32 KiB per operand
constexpr int BIG_STAGE = 2 * BIG_TILE;       // 64 KiB per K-tile

struct NoOp {
  __device__ void operator()() const {}
};

template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ void big8_bar() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
}

// Params types of the EPI_GATHER / EPI_SPLIT instantiations: the A loader gathers (the type
// selects the loader at compile time; every other GEMM keeps the plain one): Swin PatchMerging
// (gmode 1) / the T2T soft split (gmode 2).
struct MergeParams : GemmParams {};
struct UnfoldParams : GemmParams {};
// 128 x 384 tiles (gemm_p384_kernel): the params type selects the tile geometry at compile time
struct P384Params : GemmParams {};

// Tile geometry of the 8-phase main loop by params type: BM x BN block tile, 8 waves as 2 (wm) x 4
// (wn), each wave (BM / 2) x (BN / 4) = MF x NF fragments of 16 x 16. The K-tile's LDS stage is
// A (BM rows) then W (BN rows) of 128 B, 64 KiB for both geometries; its four DMA regions are the
// A m-halves (AI instructions per wave) and the W n-halves (WI per wave), AI + WI = 4.
template <typename P>
struct GeoOf {
  static constexpr int BM = 256, BN = 256, MF = 8, NF = 4;
};
template <>
struct GeoOf<P384Params> {
  static constexpr int BM = 128, BN = 384, MF = 4, NF = 6;
};
template <typename P>
struct Geo : GeoOf<P> {
  using G = GeoOf<P>;
  static constexpr int WR = G::BM / 2, WC = G::BN / 4;  // wave tile rows / columns
  static constexpr int MH = G::MF / 2, NH = G::NF / 2;  // fragments per m-half / n-half
  static constexpr int A_TILE = G::BM * ROWB;
  static constexpr int AI = G::BM / 128, WI = G::BN / 128;  // DMA instructions per wave per region
  static_assert(A_TILE + G::BN * ROWB == BIG_STAGE && AI + WI == 4, "64 KiB K-tile stages");
};

// EPI_GATHER A address (Swin PatchMerging, reference SwinTransformer PatchMerging.forward:
// x0 | x1 | x2 | x3 = x[0::2, 0::2] | x[1::2, 0::2] | x[0::2, 1::2] | x[1::2, 1::2]): GEMM row gm
// is token (b, y, x) of the R/2 grid, element k = q C + c is channel c of source token
// (2y + (q & 1), 2x + (q >> 1)) of the R-grid stream. Divisions by float reciprocals (exact for
// gm < 2^22 with the half-unit offset, as pos_img).
// gmode 2 (T2T soft_split1, tf_Unfold k 3 s 2 p 1 of the 64-channel token map, t2t_vit.py:72):
// element k = (3 kh + kw) 64 + c is channel c of source token (2y - 1 + kh, 2x - 1 + kw), or of a
// zero row outside the map.
template <int MODE>
__device__ __forceinline__ const char* gather_addr(const GemmParams& p, int gm, int k) {
  const int OW = p.gOW;
  const int b = (int)(((float)gm + 0.5f) * p.g_inv_rr);
  const int r = gm - b * OW * OW;
  const int y = (int)(((float)r + 0.5f) * p.g_inv_r);
  const int x = r - y * OW;
  if constexpr (MODE == 2) {
    const int win = k >> 6, c = k & 63;
    const int kh = (win * 11) >> 5, kw = win - 3 * kh;  // win / 3 for win < 9
    const int iy = 2 * y - 1 + kh, ix = 2 * x - 1 + kw;
    if (iy < 0 || iy >= p.gR || ix < 0 || ix >= p.gR) return (const char*)p.gzero + c * 2;
    const int64_t src = ((int64_t)b * p.gR + iy) * p.gR + ix;
    return (const char*)p.A + (src * p.lda + c) * 2;
  }
  const int q = (k >= p.gC) + (k >= 2 * p.gC) + (k >= 3 * p.gC);
  const int c = k - q * p.gC;
  const int64_t src = ((int64_t)b * p.gR + 2 * y + (q & 1)) * p.gR + 2 * x + (q >> 1);
  return (const char*)p.A + (src * p.lda + c) * 2;
}

// DMA region j of K-tile T into buffer (T ^ par) & 1 (par: the buffer parity of the tile's
// K-tile 0; persistent kernel with an odd K-tile count: alternates from tile to tile).
template <typename P>
__device__ __forceinline__ void big8_stage(const P& p, char* smem, int wave, int lane,
                                           int m0, int n0, int T, int j, int par = 0) {
  typedef Geo<P> Gm;
  const int srow = lane >> 3, sslot = lane & 7;
  EVT_LDS char* base = (EVT_LDS char*)smem + ((T ^ par) & 1) * BIG_STAGE;
  // the lane's swizzled 16-B chunk. Computed here, ahead of every branch: hipcc 7.2 orders the
  // gathered loaders' address arithmetic by this position (re-check the ISA before moving it)
  const uint32_t swz = (uint32_t)((sslot ^ srow) << 4);
  if constexpr (Gm::BM != 256) {
    // general geometry: a K-tile's 8 DMA instructions per wave in the region order of the 256 x 256
    // one (A m-half 0, W n-half 0, W n-half 1, A m-half 1: AI, WI, WI, AI instructions), issued
    // two per phase: "j" is the pair (0, 1: the first half of that order, 2, 3: the second), so
    // unequal regions (1 + 3 + 3 + 1 for 128 x 384) still spread evenly over the phases
    auto a_ins = [&](int h, int i) {  // A m-half h, instruction i of AI: rows wm*WR + h*WR/2 + ..
      const int g = wave * Gm::AI + i, gpw = Gm::WR / 16;
      const int row = (g / gpw) * Gm::WR + h * (Gm::WR / 2) + (g % gpw) * 8;
      const int gm = min(m0 + row + srow, p.M - 1);
      glds16s((const char*)p.A + (int64_t)m0 * (p.lda * 2) + T * ROWB,
              (uint32_t)((gm - m0) * (p.lda * 2)) + swz, base + row * ROWB);
    };
    auto w_ins = [&](int h, int i) {  // W n-half h, instruction i of WI: rows wn*WC + h*WC/2 + ..
      const int g = wave * Gm::WI + i, gpw = Gm::WC / 16;
      const int row = (g / gpw) * Gm::WC + h * (Gm::WC / 2) + (g % gpw) * 8;
      glds16s((const char*)p.W + (int64_t)n0 * (p.ldw * 2) + T * ROWB,
              (uint32_t)((row + srow) * (p.ldw * 2)) + swz,
              base + Gm::A_TILE + row * ROWB);
    };
    auto ins = [&](int q) {  // instruction q (0..7) of the K-tile's sequence
      if (q < Gm::AI) a_ins(0, q);
      else if (q < Gm::AI + Gm::WI) w_ins(0, q - Gm::AI);
      else if (q < Gm::AI + 2 * Gm::WI) w_ins(1, q - Gm::AI - Gm::WI);
      else a_ins(1, q - Gm::AI - 2 * Gm::WI);
    };
    ins(2 * j);
    ins(2 * j + 1);
    return;
  }
  if constexpr (!std::is_same<P, MergeParams>::value && !std::is_same<P, UnfoldParams>::value) {
    // the wave's two pieces of the region are 8 rows = 1 KiB apart in LDS: one M0 for both, the
    // second at instruction offset 1024 (applied to the LDS and the global address alike; the
    // SGPR base moves down 1 KiB so that no lane offset goes negative)
    const int r = wave * 16;
    if (j == 0 || j == 3) {
      const int row = (r & 63) + ((r >> 6) << 7) + (j == 3 ? 64 : 0);
      const int gm0 = min(m0 + row + srow, p.M - 1), gm1 = min(m0 + row + 8 + srow, p.M - 1);
      glds16s_pair(((const char*)p.A - 1024 + (int64_t)m0 * (p.lda * 2)) + T * ROWB,
                   (uint32_t)((gm0 - m0) * (p.lda * 2)) + swz + 1024,
                   (uint32_t)((gm1 - m0) * (p.lda * 2)) + swz, base + row * ROWB);
    } else {
      const int row = ((r >> 5) << 6) + (r & 31) + (j == 2 ? 32 : 0);
      glds16s_pair(((const char*)p.W - 1024 + (int64_t)n0 * (p.ldw * 2)) + T * ROWB,
                   (uint32_t)((row + srow) * (p.ldw * 2)) + swz + 1024,
                   (uint32_t)((row + 8 + srow) * (p.ldw * 2)) + swz,
                   base + BIG_TILE + row * ROWB);
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = (wave * 2 + i) * 8;  // region row of this wave-instruction (8 rows)
    if (j == 0 || j == 3) {
      const int row = (r & 63) + ((r >> 6) << 7) + (j == 3 ? 64 : 0);
      const int gm = min(m0 + row + srow, p.M - 1);
      if constexpr (std::is_same<P, MergeParams>::value)
        glds16(gather_addr<1>(p, gm, T * 64 + ((sslot ^ srow) << 3)), base + row * ROWB);
      else if constexpr (std::is_same<P, UnfoldParams>::value)
        glds16(gather_addr<2>(p, gm, T * 64 + ((sslot ^ srow) << 3)), base + row * ROWB);
      else  // SGPR base = the tile's first row at K-tile T, 32-bit lane offsets (glds16s)
        glds16s((const char*)p.A + (int64_t)m0 * (p.lda * 2) + T * ROWB,
                (uint32_t)((gm - m0) * (p.lda * 2)) + swz, base + row * ROWB);
    } else {
      const int row = ((r >> 5) << 6) + (r & 31) + (j == 2 ? 32 : 0);
      glds16s((const char*)p.W + (int64_t)n0 * (p.ldw * 2) + T * ROWB,
              (uint32_t)((row + srow) * (p.ldw * 2)) + swz,
              base + BIG_TILE + row * ROWB);
    }
  }
}

__device__ __forceinline__ int big8_npro(int nk) { return min(6, 4 * nk); }

template <typename P>
__device__ __forceinline__ void big8_prologue(const P& p, char* smem, int wave, int lane,
                                              int m0, int n0, int nk, int par = 0) {
  // regions s = 0..5 (tile 0, then regions 0 / 1 of tile 1); only 0..3 when nk == 1
#pragma unroll
  for (int s = 0; s < 4; ++s) big8_stage(p, smem, wave, lane, m0, n0, 0, s, par);
  if (nk >= 2) {
    big8_stage(p, smem, wave, lane, m0, n0, 1, 0, par);
    big8_stage(p, smem, wave, lane, m0, n0, 1, 1, par);
  }
}

// One K-tile. MODE 0 steady (all DMAs, waits 8), 1 second-to-last tile, 2 last tile. X is
// added to every wait of the tile: the number of VMEM instructions each wave is known to have
// issued after the prologue DMAs (gemm_pers_kernel's epilogue stores; first K-tile only).
// cont (persistent kernel, even nk): the last 1.5 K-tiles' DMA slots, idle otherwise, carry the
// NEXT tile's prologue (its K-tiles 0 and 1 are this tile's K-tiles nk and nk + 1 of one continuous
// stream: same buffers, same WAR distances, the steady-state waits), at (nm0, nn0).
// OPEN (last K-tile of a persistent-kernel tile): wave group 1 skips the barrier that closes its
// final MFMA phase and group 0 the resync barrier after the loop, so group 0 starts its epilogue
// while group 1 still issues its last 16 MFMAs (the two barriers cancel in every wave's count).
// ph3: issues X3 further VMEM loads at the start of phase 3 (added to that phase's wait).
template <int MODE, int X, bool OPEN = false, int X3 = 0, typename Ph3 = NoOp,
          typename P = GemmParams>
__device__ __forceinline__ void big8_ktile(const P& p, char* smem,
                                           f32x4 (&acc)[GeoOf<P>::NF][GeoOf<P>::MF],
                                           int wave, int lane, int wm, int wn, int m0, int n0,
                                           int t, bool cont = false, int nm0 = 0, int nn0 = 0,
                                           Ph3 ph3 = {}, int par = 0, int npar = 0) {
  typedef Geo<P> Gm;
  constexpr int MH = Gm::MH, NH = Gm::NH;
  const int frow = lane & 15, fsw = lane & 7, fg = lane >> 4;
  const EVT_LDS char* As = (const EVT_LDS char*)smem + ((t ^ par) & 1) * BIG_STAGE;
  const EVT_LDS char* Ws = As + Gm::A_TILE;
  auto rd = [&](const EVT_LDS char* S, int row, int ks) {
    return *(const EVT_LDS u32x4*)(S + row * ROWB + (((fg + 4 * ks) ^ fsw) << 4));
  };
  u32x4 af[MH][2], bf0[NH][2], bf1[NH][2];
#pragma unroll
  for (int ph = 0; ph < 4; ++ph) {
    // the phase's fragment reads, then its DMA issue (the DMA regions are >= 2 phases from any
    // read here; issuing the DMA first measured 0.7 % slower, round 3)
    if (ph == 0) {
#pragma unroll
      for (int nt = 0; nt < NH; ++nt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) bf0[nt][ks] = rd(Ws, wn * Gm::WC + nt * 16 + frow, ks);
#pragma unroll
      for (int mt = 0; mt < MH; ++mt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) af[mt][ks] = rd(As, wm * Gm::WR + mt * 16 + frow, ks);
    } else if (ph == 1) {
#pragma unroll
      for (int nt = 0; nt < NH; ++nt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          bf1[nt][ks] = rd(Ws, wn * Gm::WC + Gm::WC / 2 + nt * 16 + frow, ks);
    } else if (ph == 2) {
#pragma unroll
      for (int mt = 0; mt < MH; ++mt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          af[mt][ks] = rd(As, wm * Gm::WR + Gm::WR / 2 + mt * 16 + frow, ks);
    }
    if (ph == 3) ph3();
    // DMA of region s = 4 t + ph + 6
    if (MODE == 0 || (MODE == 1 && ph < 2)) {
      if (ph < 2) big8_stage(p, smem, wave, lane, m0, n0, t + 1, ph + 2, par);
      else big8_stage(p, smem, wave, lane, m0, n0, t + 2, ph - 2, par);
    } else if (cont) {  // MODE 1 phases 2, 3 and MODE 2: the next tile's regions, in order
      const int s6 = (MODE == 1 ? ph - 2 : ph + 2);  // 0..5: (K-tile 0, regions 0-3), (1, 0-1)
      big8_stage(p, smem, wave, lane, nm0, nn0, s6 >> 2, s6 & 3, npar);
    }
    // retire what the next phase reads (phases 4, 1, 2 precede reading phases). W0: after phase 0
    // the W n-half-1 region must have landed; its last instruction is followed by 8 younger ones
    // in the 256 x 256 order, by 7 in the paired order of the 128 x 384 geometry (big8_stage)
    constexpr int W0 = Gm::WI == 3 ? 7 : 8;
    if (ph != 2) {
      if (MODE == 0 || cont) {  // (cont: the steady-state DMA pattern continues)
        if (ph == 3) wait_vm<8 + X + X3>();
        else if (ph == 0) wait_vm<W0 + X>();
        else wait_vm<8 + X>();
      } else if (MODE == 1) {
        if (ph == 3) wait_vm<4 + X>();
        else if (ph == 0) wait_vm<W0 + X>();
        else wait_vm<8 + X>();
      } else if (ph == 0) {
        wait_vm<Gm::AI + X>();  // the last K-tile's A m-half-1 region (j3) follows
      } else if (ph == 1) {
        wait_vm<0 + X>();
      }
    }
    big8_bar();
    __builtin_amdgcn_sched_barrier(0);
    const int mb = (ph >= 2) ? MH : 0, nb = (ph == 1 || ph == 2) ? NH : 0;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int nt = 0; nt < NH; ++nt)
#pragma unroll
        for (int mt = 0; mt < MH; ++mt)
          Mma<bf16>::run(nb ? bf1[nt][ks] : bf0[nt][ks], af[mt][ks], acc[nb + nt][mb + mt]);
    if (!(OPEN && MODE == 2 && ph == 3 && wm == 1)) big8_bar();
  }
}

// Two-phase schedule (big8_loop<..., KT2 = true>: the LN-folded FC1 + GELU kernels only): per
// K-tile and wave group two MFMA bursts of 32 (n-halves 0 and 1 of m-half 0, then of m-half 1)
// instead of four of 16 (FC1 -1.5 %; the instances with residual or head-major epilogues spill
// with it, profiles/r05_gemm_two_phase_ab.txt). The region stream keeps the order of
// big8_prologue; regions 0..2 of K-tile T are issued in phase 1 of K-tile T - 2, region 3 in phase
// 0 of K-tile T - 1 (one K-tile of flight each), 8 glds per lane younger at every wait; K-tile 1's
// region 2 waits for K-tile 0's phase 0 (the epilogue's scratch is in it: with cont, the previous
// tile's last K-tile issues the next tile's (0, 0..3), (1, 0..1) like big8_prologue). WAR: a
// region is overwritten one barrier after its last read, so every wave retires its fragment reads
// (lgkmcnt 0) before its opening barrier.
template <int MODE, int X, bool OPEN = false, int X3 = 0, typename Ph3 = NoOp,
          typename P = GemmParams>
__device__ __forceinline__ void big8_ktile2(const P& p, char* smem,
                                            f32x4 (&acc)[GeoOf<P>::NF][GeoOf<P>::MF],
                                            int wave, int lane, int wm, int wn, int m0, int n0,
                                            int t, bool cont = false, int nm0 = 0, int nn0 = 0,
                                            Ph3 ph3 = {}, int par = 0, int npar = 0) {
  typedef Geo<P> Gm;
  constexpr int MH = Gm::MH, NH = Gm::NH;
  // phase 0 reads regions 0..2 (and, 128 x 384, the first instruction of region 3): 8 younger
  // glds after region 2, 7 after that instruction (big8_stage's paired order)
  constexpr int W0 = Gm::WI == 3 ? 7 : 8;
  const int frow = lane & 15, fsw = lane & 7, fg = lane >> 4;
  const EVT_LDS char* As = (const EVT_LDS char*)smem + ((t ^ par) & 1) * BIG_STAGE;
  const EVT_LDS char* Ws = As + Gm::A_TILE;
  auto rd = [&](const EVT_LDS char* S, int row, int ks) {
    return *(const EVT_LDS u32x4*)(S + row * ROWB + (((fg + 4 * ks) ^ fsw) << 4));
  };
  u32x4 af[MH][2], bf0[NH][2], bf1[NH][2];
#pragma unroll
  for (int ph = 0; ph < 2; ++ph) {
    // the DMA first: its address arithmetic then overlaps dead fragment registers (issued after
    // the reads it spilled in the out-proj / QKV instantiations)
    if (MODE == 0 || (MODE == 1 && ph == 0)) {
      if (ph == 0) {
        if (t == 0) big8_stage(p, smem, wave, lane, m0, n0, 1, 2, par);
        big8_stage(p, smem, wave, lane, m0, n0, t + 1, 3, par);
      } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) big8_stage(p, smem, wave, lane, m0, n0, t + 2, j, par);
      }
    } else if (cont) {  // the next tile's regions: (0, 0..2) | (0, 3), (1, 0..1)
      if (ph == 0) {
        big8_stage(p, smem, wave, lane, nm0, nn0, 0, 3, npar);
      } else {
#pragma unroll
        for (int j = 0; j < (MODE == 1 ? 3 : 2); ++j)
          big8_stage(p, smem, wave, lane, nm0, nn0, MODE == 1 ? 0 : 1, j, npar);
      }
    }
    if (ph == 0) {
#pragma unroll
      for (int nt = 0; nt < NH; ++nt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) bf0[nt][ks] = rd(Ws, wn * Gm::WC + nt * 16 + frow, ks);
#pragma unroll
      for (int mt = 0; mt < MH; ++mt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) af[mt][ks] = rd(As, wm * Gm::WR + mt * 16 + frow, ks);
#pragma unroll
      for (int nt = 0; nt < NH; ++nt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          bf1[nt][ks] = rd(Ws, wn * Gm::WC + Gm::WC / 2 + nt * 16 + frow, ks);
    } else {
#pragma unroll
      for (int mt = 0; mt < MH; ++mt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          af[mt][ks] = rd(As, wm * Gm::WR + Gm::WR / 2 + mt * 16 + frow, ks);
    }
    // retire what the next phase reads: region 3 after phase 0 (X: younger, issued before the
    // K-tile), the next K-tile's regions 0..2 after phase 1 (X older than those)
    if (ph == 0) {
      if (MODE != 2 || cont) wait_vm<8 + X>();
      else wait_vm<0 + X>();
    } else if (MODE == 0 || (MODE == 1 && cont)) {
      wait_vm<W0>();
    } else if (MODE == 1) {
      wait_vm<W0 - 6>();
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    big8_bar();
    __builtin_amdgcn_sched_barrier(0);
    const int mb = ph ? MH : 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int nb = (ph ^ h) ? NH : 0;  // phase 0: n-half 0 then 1; phase 1: 1 then 0
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int nt = 0; nt < NH; ++nt)
#pragma unroll
          for (int mt = 0; mt < MH; ++mt)
            Mma<bf16>::run(nb ? bf1[nt][ks] : bf0[nt][ks], af[mt][ks], acc[nb + nt][mb + mt]);
      // the X3 loads once the n-half-1 fragments are dead (their registers)
      if (ph == 1 && h == 0) ph3();
    }
    if (!(OPEN && MODE == 2 && ph == 1 && wm == 1)) big8_bar();
  }
}

// one K-tile of either schedule
template <bool KT2, int MODE, int X, bool OPEN = false, int X3 = 0, typename Ph3 = NoOp,
          typename P = GemmParams>
__device__ __forceinline__ void big8_kt(const P& p, char* smem,
                                        f32x4 (&acc)[GeoOf<P>::NF][GeoOf<P>::MF], int wave,
                                        int lane, int wm, int wn, int m0, int n0, int t,
                                        bool cont = false, int nm0 = 0, int nn0 = 0, Ph3 ph3 = {},
                                        int par = 0, int npar = 0) {
  if constexpr (KT2)
    big8_ktile2<MODE, X, OPEN, X3>(p, smem, acc, wave, lane, wm, wn, m0, n0, t, cont, nm0, nn0,
                                   ph3, par, npar);
  else
    big8_ktile<MODE, X, OPEN, X3>(p, smem, acc, wave, lane, wm, wn, m0, n0, t, cont, nm0, nn0,
                                  ph3, par, npar);
}

// Main loop over the nk K-tiles after big8_prologue (whose DMAs may be followed by X further
// VMEM instructions per wave, or by a vmcnt(0)). Ends with every wave past a common barrier.
// pre1: run by wave group 1 in the slot where it waits one barrier for group 0 (per-tile LDS
// setup work that is then off the critical path); mid: after K-tile 0 (nk >= 3 only).
// last: issues LX further VMEM loads per wave just before the last K-tile (added to its waits:
// they are younger than every DMA that tile waits for); last3: LX3 more at the start of the last
// K-tile's phase 3.
// after: called with t after every steady-state K-tile t (1 <= t <= nk - 3); the persistent
// kernel's wide-row statistics rounds hang on it (pers_run).
template <int X, bool OPEN = false, typename Pre1 = NoOp, typename Mid = NoOp, int LX = 0,
          typename Last = NoOp, int LX3 = 0, typename Last3 = NoOp, typename P = GemmParams,
          bool KT2 = false, bool U2 = false, typename After = NoOp>
__device__ __forceinline__ void big8_loop(const P& p, char* smem,
                                          f32x4 (&acc)[GeoOf<P>::NF][GeoOf<P>::MF],
                                          int wave, int lane, int wm, int wn, int m0, int n0,
                                          int nk, bool cont = false, int nm0 = 0, int nn0 = 0,
                                          Pre1 pre1 = {}, Mid mid = {}, Last last = {},
                                          Last3 last3 = {}, int par = 0, After after = {}) {
  constexpr bool AFTER = !std::is_same<After, NoOp>::value;
  // K-tile t of this tile sits in buffer (t ^ par) & 1; the next tile (cont) starts at the parity
  // of stream K-tile nk
  const int npar = par ^ (nk & 1);
  if constexpr (KT2) {
    // phase 0 reads regions 0..2 (big8_ktile2): younger are (0, 3) and (1, 0..1)
    constexpr int W0 = Geo<P>::WI == 3 ? 7 : 8;
    if (nk >= 2) wait_vm<W0 - 2 + X>();
    else wait_vm<W0 - 6 + X>();
  } else {
    if (nk >= 2) wait_vm<8 + X>();
    else wait_vm<4 + X>();
  }
  big8_bar();
  if (wm == 1) {
    pre1();
    big8_bar();
  }
  if (nk >= 3) {
    big8_kt<KT2, 0, X>(p, smem, acc, wave, lane, wm, wn, m0, n0, 0, false, 0, 0, {}, par, 0);
    mid();
    int t = 1;
    // U2: two K-tiles per iteration: t is odd in the first, even in the second, so each one's
    // buffer parity (t ^ par) & 1 and region addresses are loop-invariant (round 6: SALU 42 -> 18.5
    // and VALU 6 -> 2 per K-tile; QKV 315.4 -> 310.9 µs, FC2 386.4 -> 377.7, DeiT-base +0.9 %,
    // profiles/r06_unroll2_ab.txt); not where the doubled body spills (pers_run)
    if constexpr (U2) {
      for (; t + 3 < nk; t += 2) {
        big8_kt<KT2, 0, 0>(p, smem, acc, wave, lane, wm, wn, m0, n0, t, false, 0, 0, {}, par, 0);
        if constexpr (AFTER) after(t);
        big8_kt<KT2, 0, 0>(p, smem, acc, wave, lane, wm, wn, m0, n0, t + 1, false, 0, 0, {}, par, 0);
        if constexpr (AFTER) after(t + 1);
      }
    }
    for (; t + 2 < nk; ++t) {
      big8_kt<KT2, 0, 0>(p, smem, acc, wave, lane, wm, wn, m0, n0, t, false, 0, 0, {}, par, 0);
      if constexpr (AFTER) after(t);
    }
    big8_kt<KT2, 1, 0>(p, smem, acc, wave, lane, wm, wn, m0, n0, t, cont, nm0, nn0, {}, par, npar);
    last();
    big8_kt<KT2, 2, LX, OPEN, LX3>(p, smem, acc, wave, lane, wm, wn, m0, n0, t + 1, cont, nm0, nn0,
                                 last3, par, npar);
  } else if (nk == 2) {
    big8_kt<KT2, 1, X>(p, smem, acc, wave, lane, wm, wn, m0, n0, 0, cont, nm0, nn0, {}, par, npar);
    last();
    big8_kt<KT2, 2, LX, OPEN, LX3>(p, smem, acc, wave, lane, wm, wn, m0, n0, 1, cont, nm0, nn0, last3,
                                 par, npar);
  } else {
    last();
    big8_kt<KT2, 2, X + LX, OPEN, LX3>(p, smem, acc, wave, lane, wm, wn, m0, n0, 0, false, 0, 0,
                                     last3, par);
  }
  if (!OPEN && wm == 0) big8_bar();
}

}  // namespace

}  // namespace evt
