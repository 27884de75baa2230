// ---------------------------------------------------------------------------------------------
// Persistent 256x256 kernel with the epilogue in registers (bf16 output; FL without POS /
// OUT_F32). One block per CU walks its tiles (XCD-aware: in every round an XCD takes a
// contiguous range of logical tiles); per tile:
//   main loop (big8_loop) -> LayerNorm coefficients / column vectors into LDS ->
//   DMA of the NEXT tile's prologue (and its statistics / column vectors) ->
//   epilogue of this tile straight from the accumulators, overlapping those DMAs ->
//   the next main loop starts while this tile's output stores drain.
// The accumulators are converted in the MFMA layout (lane: token row mt*16 + (lane & 15),
// features 4 (lane >> 4) + j), then v_permlane16_swap pairs fragments (2k, 2k+1) so that every
// lane holds 8 consecutive features of one row: 16-B residual loads and 16-B output stores,
// no LDS staging of the tile. Row statistics (EPI_STATS): 64-column partials per wave, the two
// waves of a 128-column slab combined in a fixed order (slot 2 tn + slab, as the staged
// epilogue). Every interior tile issues its 16 output stores per wave after the next tile's
// prologue DMAs, which is what the first K-tile's counted waits (X = 16) assume; an edge tile
// drains with vmcnt(0) instead.
// ---------------------------------------------------------------------------------------------
#pragma once
#include "gemm_big8.h"

namespace evt {

namespace {

constexpr int PERS_RAW = 2 * BIG_STAGE;         // raw LN statistics of the tile rows [256][<=8] f32x2
constexpr int PERS_COLRAW = PERS_RAW + 16384;   // DMA'd column vectors [3][256] f32
constexpr int PERS_COEF = PERS_COLRAW + 3072;   // LayerNorm (mu, r) per tile row [256] f32x2
constexpr int PERS_COLB = PERS_COEF + 2048;     // column vectors of the tile being finished
constexpr int PERS_PART = PERS_COLB + 3072;     // odd-wn waves' row partials [2][256] f32x2
constexpr int PERS_LDS = PERS_PART + 4096;
constexpr int PERS_LDS_ALL = PERS_LDS + 16;
constexpr int PERS_X = 16;                      // output stores per wave per interior tile
// Wide LayerNorm rows (10 or 12 statistics slots, widths 1025..1536: the WIDE instantiations):
// PERS_RAW holds 8 slots per row, so the statistics are staged in two DMA rounds. Round 0 (slots
// 0..7, after K-tile 0 of the previous tile, where the one-round DMA sits) is summed per row in
// slot order into PERS_ACC after K-tile 2; round 1 (slots 8.., [256][nslots - 8] at PERS_RAW)
// is issued after K-tile 3, and the next tile's coefficients continue the sums from PERS_ACC in
// the same slot order, so (s1, s2) are the sequential sums ln_coef forms. Both rounds are
// followed by whole steady-state K-tiles (nk >= 8, use_pers): every counted wait of those K-tiles
// leaves at most 8 DMAs in flight per wave, all younger, and they add VMEM instructions only where
// X = 0 (waits there get stricter, never weaker); the first K-tile's X is unchanged.
constexpr int PERS_ACC = PERS_LDS_ALL;          // partial (s1, s2) of slots 0..7 [256] f32x2
constexpr int PERS_LDS_WIDE = PERS_ACC + 2048;
constexpr int PERS_WIDE_MIN_NK = 8;
static_assert(PERS_LDS_WIDE <= 160 * 1024, "LDS of one workgroup");

template <int FL>
struct PersFlags {
  static constexpr bool ln = (FL & (EPI_LNIN | EPI_RESLN)) != 0;
  // column vector slots: 0 bias, 1 colsum (LNIN) or rgamma (RESLN), 2 rbeta (RESLN)
  static constexpr bool v0 = (FL & EPI_BIAS) != 0;
  static constexpr bool v1 = (FL & (EPI_LNIN | EPI_RESLN)) != 0;
  static constexpr bool v2 = (FL & EPI_RESLN) != 0;
  static_assert(!((FL & EPI_LNIN) && (FL & EPI_RESLN)), "one LayerNorm source per GEMM");
  static_assert(!(FL & EPI_RESLN) || ((FL & EPI_BIAS) && (FL & EPI_RESID)),
                "RESLN: the residual LayerNorm's beta is folded into the bias add");
  static_assert(!(FL & EPI_OUT_F32), "persistent kernel: bf16 outputs");
  // EPI_POS (patch embedding): + pos[t + 1][n] from a bf16 copy of the table in p.resid (pitch
  // p.ldr), row remap b*P + t -> b*(P+1) + 1 + t of the outputs and their statistics
  static_assert(!(FL & EPI_POS) || !(FL & (EPI_RESID | EPI_LNIN)), "POS: its own residual form");
};

// DMA the tile's LN statistics rows and column vectors into LDS (before its prologue DMAs).
// WIDE: round 0 = slots 0..7 of every row ([256][8], the one-round image) and the column vectors,
// round 1 = slots 8..nslots-1 ([256][nslots - 8]).
template <int FL, bool WIDE = false>
__device__ __forceinline__ void pers_coop_dma(const GemmParams& p, char* smem, int wave, int lane,
                                              int m0, int n0, int round = 0) {
  typedef PersFlags<FL> F;
  asm volatile("" : "+v"(lane));
  if constexpr (F::ln && WIDE) {
    const float* st = (FL & EPI_LNIN) ? p.stats_in : p.rstats;
    const int cpr = round ? (p.nslots >> 1) - 4 : 4;  // 16-B chunks per row in this round: 1, 2 / 4
    const int nch = 256 * cpr;
    for (int c = wave * 64; c < nch; c += 512) {
      const int cl = c + lane, r = cpr == 4 ? cl >> 2 : (cpr == 2 ? cl >> 1 : cl), q = cl - r * cpr;
      const int64_t row = min(m0 + r, p.M - 1);
      glds16(st + row * (2 * p.nslots) + (round ? 16 : 0) + 4 * q,
             (EVT_LDS char*)smem + PERS_RAW + c * 16);
    }
    if (round) return;
  } else if constexpr (F::ln) {
    const float* st = (FL & EPI_LNIN) ? p.stats_in : p.rstats;
    const int half = p.nslots >> 1;  // 16-B chunks per row
    const int nch = 256 * half;
    const int64_t c0 = (int64_t)m0 * half, clast = (int64_t)p.M * half - 1;
    for (int c = wave * 64; c < nch; c += 512)
      glds16(st + 4 * min(c0 + c + lane, clast), (EVT_LDS char*)smem + PERS_RAW + c * 16);
  }
  const float* v = nullptr;
  if (wave == 0 && F::v0) v = p.bias;
  if (wave == 1 && (FL & EPI_LNIN)) v = p.colsum;
  if (wave == 1 && (FL & EPI_RESLN)) v = p.rgamma;
  if (wave == 2 && F::v2) v = p.rbeta;
  if (v) glds16(v + min(n0 + 4 * lane, p.N - 4), (EVT_LDS char*)smem + PERS_COLRAW + wave * 1024);
}

// WIDE: (s1, s2) over the staged slots 0..7 of every tile row, in slot order, into PERS_ACC
// (threads 0..255); the reads are retired on return, so a barrier later round 1 may overwrite them.
__device__ __forceinline__ void pers_wide_reduce(char* smem, int tid) {
  asm volatile("" : "+v"(tid));
  if (tid < 256) {
    const EVT_LDS f32x2* st = (const EVT_LDS f32x2*)(smem + PERS_RAW) + tid * 8;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const f32x2 v = st[j];
      s1 += v[0];
      s2 += v[1];
    }
    ((EVT_LDS f32x2*)(smem + PERS_ACC))[tid] = f32x2{s1, s2};
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// Per-row LayerNorm coefficients (as ln_coef) and a copy of the column vectors for the epilogue.
template <int FL, bool WIDE = false>
__device__ __forceinline__ void pers_coef(const GemmParams& p, char* smem, int tid) {
  typedef PersFlags<FL> F;
  asm volatile("" : "+v"(tid));
  if (tid < 256) {
    if constexpr (F::ln) {
      const int ns = WIDE ? p.nslots - 8 : p.nslots;
      const EVT_LDS f32x2* st = (const EVT_LDS f32x2*)(smem + PERS_RAW) + tid * ns;
      float s1 = 0.f, s2 = 0.f;
      if constexpr (WIDE) {  // slots 0..7 summed by pers_wide_reduce; 8.. continue the same chain
        const f32x2 a = ((const EVT_LDS f32x2*)(smem + PERS_ACC))[tid];
        s1 = a[0];
        s2 = a[1];
      }
      for (int j = 0; j < ns; ++j) {
        const f32x2 v = st[j];
        s1 += v[0];
        s2 += v[1];
      }
      const float mu = s1 * p.inv_d;
      const float r = rsqrtf(fmaxf(s2 * p.inv_d - mu * mu, 0.f) + p.eps);
      ((EVT_LDS f32x2*)(smem + PERS_COEF))[tid] = f32x2{mu, r};
    }
    const EVT_LDS float* src = (const EVT_LDS float*)(smem + PERS_COLRAW);
    EVT_LDS float* dst = (EVT_LDS float*)(smem + PERS_COLB);
    if (F::v0) dst[tid] = src[tid];
    if (F::v1) dst[256 + tid] = src[256 + tid];
    if (F::v2) dst[512 + tid] = src[512 + tid];
  }
}

__device__ __forceinline__ f32x4 lds4(const EVT_LDS float* p) { return *(const EVT_LDS f32x4*)p; }

// v_permlane16_swap_b32 on (x, y): odd 16-lane rows of x <-> even rows of y. Written on scalars:
// applied in place to vector elements (v[j] = swap(...)[0] in a loop) hipcc 7.2 miscompiles the
// builtin (it reuses element 0 for every j).
__device__ __forceinline__ float swp16(float x, float y, float& yo) {
  const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, x),
                                                  __builtin_bit_cast(unsigned, y), false, false);
  yo = __builtin_bit_cast(float, (unsigned)r[1]);
  return __builtin_bit_cast(float, (unsigned)r[0]);
}
__device__ __forceinline__ void swap_rows16(f32x4& a, f32x4& b) {
  float y0, y1, y2, y3;
  const float x0 = swp16(a[0], b[0], y0), x1 = swp16(a[1], b[1], y1);
  const float x2 = swp16(a[2], b[2], y2), x3 = swp16(a[3], b[3], y3);
  a = f32x4{x0, x1, x2, x3};
  b = f32x4{y0, y1, y2, y3};
}

// Buffer resource of one tile's rows of an output / residual matrix [M][ld] (bf16): base = the
// tile's first element (m0, n0), num_records = the bytes to the end of the tile's last valid row,
// so rows past M are dropped (stores) / read as 0 (loads) by the hardware range check instead of
// per-lane branches. m0 / n0 go through readfirstlane and every input stays 32-bit: a 64-bit
// min/max in the byte count is lowered to VALU, and hipcc then no longer proves the descriptor
// wave-uniform and wraps every buffer op in a waterfall loop (guide T20).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const void* mat, int64_t ld, int M,
                                                           int m0, int n0) {
  m0 = __builtin_amdgcn_readfirstlane(m0);
  n0 = __builtin_amdgcn_readfirstlane(n0);
  const int nr = (min(M - m0, 256) * (int)ld - n0) * 2;  // ld < 2^22: a tile spans < 2 GB
  return __builtin_amdgcn_make_buffer_rsrc((char*)const_cast<void*>(mat) + ((int64_t)m0 * ld + n0) * 2,
                                           0, nr, 0x00020000);
}

// EPI_POS row arithmetic: image of patch row m (m / P, exact in fp32 for m < 2^22 with the
// half-row offset) and its token row in the stream, b*(P+1) + 1 + t = m + m/P + 1.
__device__ __forceinline__ int pos_img(int m, int P) {
  return (int)(((float)m + 0.5f) * (1.0f / (float)P));
}
__device__ __forceinline__ int pos_orow(int m, int P) { return m + pos_img(m, P) + 1; }

// Epilogue of one 256 x 256 tile straight from the accumulators (VALU-bound: every instruction
// here is paid with the MFMA pipe idle, so the arithmetic is in packed form throughout):
//   LNIN   r (acc - mu colsum) + c      2 v_pk_fma per column pair
//   BIAS   acc + bias (+ beta of the residual LayerNorm when RESLN: folded into one add)
//   RESLN  + gamma (r resid - r mu)     2 v_pk_fma per pair on the unpacked bf16 residual
//   STATS  (sum, sumsq) of the stored bf16 values with v_dot2c_f32_bf16 (2 per stored dword)
// Residual loads and output stores go through tile buffer resources (SGPR base per tile, lane
// offsets tile-invariant, row offsets in SGPRs): no per-store 64-bit address arithmetic and no
// exec-mask branches for the M edge.
// Residual of the first ER row pairs (the epilogue's rr[0 .. ER-1]), issued before the tile's last
// K-tile so that part of the residual fetch is in flight under its MFMAs (ER = 1: the most that
// fits in 256 VGPRs without spilling).
template <int K0, int K1>
__device__ __forceinline__ void pers_resid_early(const GemmParams& p, int wm, int wn, int lane,
                                                 int m0, int n0, u32x4 (&rre)[2][4]) {
  const int frow = lane & 15, fg = lane >> 4;
  const int rl = wm * 128 + (fg & 1) * 16 + frow, cl = wn * 64 + (fg >> 1) * 8;
  const __amdgpu_buffer_rsrc_t rs = tile_rsrc(p.resid, p.ldr, p.M, m0, n0);
  const int vo = (rl * (int)p.ldr + cl) * 2;
#pragma unroll
  for (int k = K0; k < K1; ++k) {
    const int so = __builtin_amdgcn_readfirstlane(32 * k * (int)p.ldr * 2);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
      rre[k][nt] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo + 32 * nt, so, 0));
  }
}

// PADN: the output width N is not a multiple of the tile (Swin / pruned widths): column groups
// entirely past N skip their epilogue VALU work. Compiled out otherwise (the check alone cost
// 2-4 % on the DeiT shapes, measured in one process).
template <int FL, bool PADN = true, int ER = 0>
__device__ __forceinline__ void pers_epilogue(const GemmParams& p, char* smem, f32x4 (&acc)[4][8],
                                              int wave, int wm, int wn, int m0, int n0, int tn,
                                              int lane, bool interior,
                                              const u32x4 (*rre)[4] = nullptr, int spar = 0) {
  asm volatile("" : "+v"(lane));  // keep lane-derived addresses out of the persistent loop (VGPRs)
  const int frow = lane & 15, fg = lane >> 4;
  const EVT_LDS f32x2* coef = (const EVT_LDS f32x2*)(smem + PERS_COEF);
  const EVT_LDS float* colb = (const EVT_LDS float*)(smem + PERS_COLB);
  auto padskip = [&](int nt) { return PADN && !interior && n0 + wn * 64 + nt * 16 >= p.N; };
  // 1. MFMA layout: row wm*128 + mt*16 + frow, columns wn*64 + nt*16 + 4 fg + j
  if constexpr ((FL & EPI_LNIN) != 0) {
    f32x4 b4[4], c4[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int c = wn * 64 + nt * 16 + 4 * fg;
      b4[nt] = (FL & EPI_BIAS) ? lds4(colb + c) : f32x4{0.f, 0.f, 0.f, 0.f};
      c4[nt] = lds4(colb + 256 + c);
    }
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
      const f32x2 cf = coef[wm * 128 + mt * 16 + frow];
      const f32x2 nmu = {-cf[0], -cf[0]}, rr = {cf[1], cf[1]};
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        if (padskip(nt)) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          f32x2 a = {acc[nt][mt][2 * h], acc[nt][mt][2 * h + 1]};
          const f32x2 cs = {c4[nt][2 * h], c4[nt][2 * h + 1]}, bb = {b4[nt][2 * h], b4[nt][2 * h + 1]};
          a = __builtin_elementwise_fma(cs, nmu, a);
          a = __builtin_elementwise_fma(a, rr, bb);
          acc[nt][mt][2 * h] = a[0];
          acc[nt][mt][2 * h + 1] = a[1];
        }
      }
    }
  } else if constexpr ((FL & EPI_BIAS) != 0) {
    f32x4 b4[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int c = wn * 64 + nt * 16 + 4 * fg;
      b4[nt] = lds4(colb + c);
      if (FL & EPI_RESLN) b4[nt] += lds4(colb + 512 + c);  // + beta of LN(resid)
    }
#pragma unroll
    for (int mt = 0; mt < 8; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        if (padskip(nt)) continue;
        acc[nt][mt] += b4[nt];
      }
  }
  if constexpr ((FL & (EPI_GELU | EPI_GELU_ERF)) != 0) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      // column group past N (padding of the packed width): wave-uniform skip of the VALU work
      if (padskip(nt)) continue;
#pragma unroll
      for (int mt = 0; mt < 8; ++mt) acc[nt][mt] = gelu4(acc[nt][mt], (FL & EPI_GELU) ? 0 : 2);
    }
  }
  // 2. store layout: pair (2k, 2k+1) -> lane row wm*128 + (2k + (fg & 1))*16 + frow, columns
  //    wn*64 + nt*16 + (fg >> 1)*8 + [acc[nt][2k][0..3], acc[nt][2k+1][0..3]]
  //    (no residual / position / statistics: the values are packed to bf16 first and the swap
  //    moves 2 dwords per pair instead of 4; the same elements, bitwise the same stores)
  constexpr bool PACK_FIRST = (FL & (EPI_RESID | EPI_POS | EPI_STATS)) == 0;
  if constexpr (!PACK_FIRST) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int k = 0; k < 4; ++k) swap_rows16(acc[nt][2 * k], acc[nt][2 * k + 1]);
  }
  const int rl = wm * 128 + (fg & 1) * 16 + frow;  // + 32 k
  const int cl = wn * 64 + (fg >> 1) * 8;           // + 16 nt
  bool cok[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) cok[nt] = !PADN || interior || n0 + cl + 16 * nt < p.N;
  // 3. residual (16-B buffer loads in the store layout, all issued up front), bf16 stores and the
  //    row statistics of the stored values; nt-major so each column-vector slice is read once
  u32x4 rr[4][4];
  if constexpr ((FL & EPI_RESID) != 0) {
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc(p.resid, p.ldr, p.M, m0, n0);
    const int vo = (rl * (int)p.ldr + cl) * 2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int so = __builtin_amdgcn_readfirstlane(32 * k * (int)p.ldr * 2);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        rr[k][nt] = k < ER ? rre[k][nt]
                           : __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo + 32 * nt, so, 0));
    }
  } else if constexpr ((FL & EPI_POS) != 0) {  // pos[t + 1][n0 + cl + 16 nt ..] (bf16 table)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.resid), 0, (p.P + 1) * (int)p.ldr * 2, 0x00020000);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int m = min(m0 + rl + 32 * k, p.M - 1);
      const int t = m - pos_img(m, p.P) * p.P;
      const int vo = ((t + 1) * (int)p.ldr + n0 + cl) * 2;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        rr[k][nt] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo + 32 * nt, 0, 0));
    }
  }
  f32x2 rc[4], st[4];
  u32x4 ov[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    rc[k] = (FL & EPI_RESLN) ? coef[rl + 32 * k] : f32x2{0.f, 0.f};
    st[k] = f32x2{0.f, 0.f};
  }
  const bf16x2 one2 = {(bf16)1.0f, (bf16)1.0f};
  if constexpr (PACK_FIRST) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const f32x4 x = acc[nt][2 * k], y = acc[nt][2 * k + 1];
        const u32x2 xa = __builtin_bit_cast(u32x2, bf16x4{(bf16)x[0], (bf16)x[1], (bf16)x[2], (bf16)x[3]});
        const u32x2 ya = __builtin_bit_cast(u32x2, bf16x4{(bf16)y[0], (bf16)y[1], (bf16)y[2], (bf16)y[3]});
        unsigned x0 = xa[0], x1 = xa[1], y0 = ya[0], y1 = ya[1];
        permlane16_swap(x0, y0);
        permlane16_swap(x1, y1);
        ov[k][nt] = u32x4{x0, x1, y0, y1};
      }
  }
#pragma unroll
  for (int nt = 0; nt < 4 && !PACK_FIRST; ++nt) {
    const int c = cl + 16 * nt;
    f32x4 g[2];
    if (FL & EPI_RESLN) {
#pragma unroll
      for (int h = 0; h < 2; ++h) g[h] = lds4(colb + 256 + c + 4 * h);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      f32x4 v[2] = {acc[nt][2 * k], acc[nt][2 * k + 1]};
      if constexpr ((FL & (EPI_RESID | EPI_POS)) != 0) {
        const bf16x8 r8 = __builtin_bit_cast(bf16x8, rr[k][nt]);
        const f32x2 rrow = {rc[k][1], rc[k][1]}, nrm = {-rc[k][1] * rc[k][0], -rc[k][1] * rc[k][0]};
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const f32x2 rv = {(float)r8[4 * h + 2 * q], (float)r8[4 * h + 2 * q + 1]};
            f32x2 a = {v[h][2 * q], v[h][2 * q + 1]};
            if (FL & EPI_RESLN) {  // + gamma (r resid - r mu)   (beta already in the bias)
              const f32x2 t = __builtin_elementwise_fma(rrow, rv, nrm);
              a = __builtin_elementwise_fma(f32x2{g[h][2 * q], g[h][2 * q + 1]}, t, a);
            } else {
              a += rv;
            }
            v[h][2 * q] = a[0];
            v[h][2 * q + 1] = a[1];
          }
      }
      const bf16x8 o = {(bf16)v[0][0], (bf16)v[0][1], (bf16)v[0][2], (bf16)v[0][3],
                        (bf16)v[1][0], (bf16)v[1][1], (bf16)v[1][2], (bf16)v[1][3]};
      ov[k][nt] = __builtin_bit_cast(u32x4, o);
      if (FL & EPI_STATS) {
        if (cok[nt]) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            // (from the bf16x8, not bit_cast(bf16x2, ov[k][nt][e]): hipcc 7.2 then feeds word 0
            // to all four dot2s)
            const bf16x2 w = {o[2 * e], o[2 * e + 1]};
            st[k][0] = __builtin_amdgcn_fdot2_f32_bf16(w, one2, st[k][0], false);
            st[k][1] = __builtin_amdgcn_fdot2_f32_bf16(w, w, st[k][1], false);
          }
        }
      }
    }
  }
  // 4. output: per row pair k, the wave's 32 x 64 block goes through its private 4 KiB of LDS
  //    (free during the epilogue: buffer-1 regions 2 / 3 are only DMA'd in the next tile's
  //    phases 1 / 2) and leaves as whole 128-B row segments, 8 rows per store instruction
  {
    const int w = wave;
    // spar: buffer parity of the next tile, whose K-tile 1 (regions 2 / 3 still unloaded) sits in
    // buffer 1 ^ spar
    EVT_LDS char* scr = (EVT_LDS char*)smem - spar * BIG_STAGE +
                        (w < 4 ? (96 + 4 + 8 * w) * 1024 : (72 + (w - 4) * 4 + ((w - 4) >> 1) * 8) * 1024);
    const int wrow = (fg & 1) * 16 + frow;               // store-layout row within the pair
    const int rrow = lane >> 3, rch = lane & 7;          // row-layout lane: row i*8 + rrow, chunk
    const bool rcol_ok = !PADN || interior || n0 + wn * 64 + rch * 8 < p.N;
    __amdgpu_buffer_rsrc_t cs;
    int vo = ((wm * 128 + rrow) * (int)p.ldc + wn * 64 + rch * 8) * 2, orow0 = 0;
    // EPI_HM: this wave's 64 columns are one (part, head) of q | k | v; row m = (b, t) goes to
    // (((b H + h) 3 + part) P + t) 64 + ... of the whole buffer (rows past M land past its end)
    // (lane row base = m0 + wm 128 + rrow as image b0, token t0; the stored rows are base + 8 j,
    // j < 16, at most one image boundary past it for P >= 128, else pos_img per row)
    int hm_b0 = 0, hm_t0 = 0, hm_col = 0, hm_HP = 0, hm_r0 = 0, hm_wrap = 0;
    if constexpr ((FL & EPI_HM) != 0) {
      const int inner = p.N / 3, c0 = n0 + wn * 64;
      const int part = __builtin_amdgcn_readfirstlane(c0 / inner);
      const int h = __builtin_amdgcn_readfirstlane((c0 - part * inner) >> 6);
      hm_HP = 3 * (inner >> 6) * p.P;                      // rows of one image's slices
      hm_col = ((3 * h + part) * p.P * 64 + rch * 8) * 2;  // + ((b 3 H P + t) 64) 2
      const int base = m0 + wm * 128 + rrow;
      hm_b0 = pos_img(base, p.P);
      hm_t0 = base - hm_b0 * p.P;
      hm_r0 = (hm_b0 * hm_HP + hm_t0) * 128 + hm_col;  // the lane's first row; + 8 j rows: + 1 KiB j
      hm_wrap = (hm_HP - p.P) * 128;                   // past the image's last token: the next image
      cs = __builtin_amdgcn_make_buffer_rsrc(p.C, 0, p.M * p.N * 2, 0x00020000);
    } else if constexpr ((FL & EPI_POS) != 0) {  // output rows b*(P+1) + 1 + t, base at tile row 0
      orow0 = __builtin_amdgcn_readfirstlane(pos_orow(m0, p.P));
      const int olast = pos_orow(min(m0 + BIG_BM, p.M) - 1, p.P);
      const int nr = ((olast + 1 - orow0) * (int)p.ldc - n0) * 2;
      cs = __builtin_amdgcn_make_buffer_rsrc((char*)p.C + ((int64_t)orow0 * p.ldc + n0) * 2, 0,
                                             nr, 0x00020000);
    } else {
      cs = tile_rsrc(p.C, p.ldc, p.M, m0, n0);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int ch = 2 * nt + (fg >> 1);
        *(EVT_LDS u32x4*)(scr + wrow * 128 + ((ch ^ (wrow & 7)) << 4)) = ov[k][nt];
      }
      asm volatile("" ::: "memory");  // (a wave's LDS operations execute in order)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = i * 8 + rrow;
        const u32x4 v = *(const EVT_LDS u32x4*)(scr + r * 128 + ((rch ^ (r & 7)) << 4));
        bool keep = rcol_ok;  // (a mutable copy: hipcc 7.2 schedules the epilogue differently without)
        int so = __builtin_amdgcn_readfirstlane((32 * k + 8 * i) * (int)p.ldc * 2), svo = vo;
        if constexpr ((FL & EPI_HM) != 0) {  // per-lane head-major row
          if (p.P >= 128) {  // row offset 8 j (< P): one compare / select per store, j in soffset
            so = __builtin_amdgcn_readfirstlane((32 * k + 8 * i) * 128);
            svo = hm_r0 + (hm_t0 + 32 * k + 8 * i >= p.P ? hm_wrap : 0);
          } else {
            const int m = m0 + wm * 128 + 32 * k + 8 * i + rrow;
            const int b = pos_img(m, p.P), t = m - b * p.P;
            so = 0;
            svo = (b * hm_HP + t) * 128 + hm_col;
          }
        } else if constexpr ((FL & EPI_POS) != 0) {  // per-lane remapped row (rows past M: beyond nr)
          so = 0;
          svo = ((pos_orow(m0 + wm * 128 + 32 * k + 8 * i + rrow, p.P) - orow0) * (int)p.ldc +
                 wn * 64 + rch * 8) * 2;
        }
        if (keep)  // nontemporal (aux nt): whole lines streamed past L2
          buffer_store_b128<2>(v, cs, svo, so);
      }
      asm volatile("" ::: "memory");
    }
  }
  if constexpr ((FL & EPI_STATS) != 0) {
    // lanes fg and fg ^ 2 hold the two 32-column halves of the same row
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      st[k][0] += __shfl_xor(st[k][0], 32, 64);
      st[k][1] += __shfl_xor(st[k][1], 32, 64);
    }
    EVT_LDS f32x2* part = (EVT_LDS f32x2*)(smem + PERS_PART) + (wn >> 1) * 256;
    if ((wn & 1) && lane < 32) {
#pragma unroll
      for (int k = 0; k < 4; ++k) part[rl + 32 * k] = st[k];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    big8_bar();
    if (!(wn & 1) && lane < 32) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int m = m0 + rl + 32 * k;
        const f32x2 o = part[rl + 32 * k];
        const int sm = (FL & EPI_POS) ? pos_orow(m, p.P) : m;
        if (interior || m < p.M)
          *(f32x2*)(p.stats_out + 2 * ((int64_t)p.nslots * sm + 2 * tn + (wn >> 1))) = st[k] + o;
      }
    }
  }
}

// Logical walk index -> output tile of the persistent 256 x 256 kernel. Walk index t of round
// r = t / G runs on XCD x of its round slot (blocks b and b + 8 share an XCD; the start index of
// block b is x (G / 8) + (b >> 3), x = b & 7). One group (xgroups <= 1): the rounds sweep the tiles
// m-panel-major, so an XCD's 32 tiles of a round span every weight panel of a wide GEMM (FC1: all
// 12, 4.7 MB, more than its 4 MB L2, fetched again from beyond L2 every round). xgroups = g: the
// XCDs form g groups of 8 / g, group k owns weight panels [k ntiles / g, (k + 1) ntiles / g) for
// the whole launch and walks the m-panels of that slice in the same m-major order, so the slice
// (FC1, g = 2: 2.4 MB) can stay in its XCDs' L2 across rounds while the A panels stream (each A
// panel then read by g XCD groups). Returns whether t names a tile. Which tile a block runs never
// changes a tile's arithmetic (bitwise the same outputs for every xgroups).
__device__ __forceinline__ bool pers_tile(int t, int G, int ntiles, int xgroups, int total, int& tm,
                                          int& tn) {
  if (xgroups <= 1) {
    tm = t / ntiles;
    tn = t - tm * ntiles;
    return t < total;
  }
  const int q = G >> 3, r = t / G, w = t - r * G, x = w / q, l = w - x * q;
  const int xs = 8 / xgroups, k = x / xs, j = (r * xs + (x - k * xs)) * q + l;
  const int ntg = ntiles / xgroups;
  tm = j / ntg;
  tn = k * ntg + (j - tm * ntg);
  return j < total / xgroups;
}

// The persistent tile walk of one GEMM from logical tile `tile` in steps of gridDim.x.
template <int FL, bool PADN, typename P = GemmParams, bool WIDE = false>
__device__ __forceinline__ void pers_run(const P& p, int total, int tile, char* smem) {
  // a quarter of the residual before the last K-tile (out-proj 160 -> 153 us)
  constexpr int ER = (FL & EPI_RESID) ? 2 : 0;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int G = gridDim.x;
  const int nk = p.K / 64;
  const int xg = p.xgroups;
  // the two-phase K-tile for the LN-folded FC1 + GELU kernels (big8_ktile2)
  // (round 6, with the SGPR-base DMA: the two-phase K-tile on every non-residual instance, where
  // it no longer spills, measured equal to this rule: QKV 311.8 vs 311.9 us, r6c A/B)
  constexpr bool KT2 = (FL & EPI_LNIN) && (FL & (EPI_GELU | EPI_GELU_ERF)) &&
                       !(FL & (EPI_RESID | EPI_HM | EPI_STATS | EPI_GATHER | EPI_SPLIT));
  // the two-K-tile steady loop (big8_loop U2) where its doubled body does not spill: not the
  // gathered loaders (Swin PatchMerging, T2T soft splits), the Swin plain-residual epilogue or the
  // column-padded (PADN) instances
  constexpr bool U2 = !PADN && !(FL & (EPI_GATHER | EPI_SPLIT)) &&
                      !((FL & EPI_RESID) && !(FL & EPI_RESLN));
  int tm, tn;
  pers_tile(tile, G, p.ntiles, xg, total, tm, tn);
  pers_coop_dma<FL, WIDE>(p, smem, wave, lane, tm * BIG_BM, tn * BIG_BN);
  if constexpr (WIDE) {  // the first tile's two statistics rounds, drained one after the other
    wait_vmcnt0();
    big8_bar();
    pers_wide_reduce(smem, tid);
    big8_bar();
    pers_coop_dma<FL, WIDE>(p, smem, wave, lane, tm * BIG_BM, tn * BIG_BN, 1);
  }
  big8_prologue(p, smem, wave, lane, tm * BIG_BM, tn * BIG_BN, nk);
  wait_vmcnt0();  // the first K-tile's waits assume PERS_X younger VMEM ops or a drain
  int par = 0;    // buffer parity of this tile's K-tile 0 (the stream alternates it for odd nk)
  // nk >= 3: per-tile LayerNorm coefficients / next statistics DMA inside the main loop
  const bool early = nk >= 3;
  while (true) {
    const int m0 = tm * BIG_BM, n0 = tn * BIG_BN;
    f32x4 acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    int ln = lane;
    asm volatile("" : "+v"(ln));  // per-tile lane addresses: not hoisted out of the tile loop
    u32x4 rre[2][4];  // ER: residual row pair 0 loaded before the last K-tile
    const int next = tile + G;
    int ntm = 0, ntn = 0;
    const bool has_next = pers_tile(next, G, p.ntiles, xg, total, ntm, ntn);
    if (!has_next) ntm = ntn = 0;
    // the next tile's prologue rides in the last K-tiles' idle DMA slots (big8_ktile) as K-tiles
    // nk, nk + 1 of one stream: for odd nk the next tile starts at the other buffer parity
    const bool cont = has_next && nk >= 2;
    const int npar = cont ? par ^ (nk & 1) : 0;
    auto last = [&]() {
      if constexpr (ER > 0) pers_resid_early<0, 1>(p, wm, wn, ln, m0, n0, rre);
    };
    auto last3 = [&]() {  // row pair 1 once the n-half-1 fragments are dead (phase 3)
      if constexpr (ER > 1) pers_resid_early<1, 2>(p, wm, wn, ln, m0, n0, rre);
    };
    if (early) {
      // this tile's LayerNorm coefficients by wave group 1 while it waits for group 0's first
      // phase; the next tile's statistics rows / column vectors DMA'd after K-tile 0 (PERS_RAW is
      // free once those coefficients are read: every later phase retires group 1's LDS ops)
      auto pre1 = [&]() { pers_coef<FL, WIDE>(p, smem, tid - 256); };
      auto mid = [&]() {
        if (has_next) pers_coop_dma<FL, WIDE>(p, smem, wave, lane, ntm * BIG_BM, ntn * BIG_BN);
      };
      // WIDE (nk >= PERS_WIDE_MIN_NK): round 0 (mid) has landed in every wave once K-tile 1's
      // waits and K-tile 2's barriers are past; its sums leave PERS_RAW free a K-tile before
      // round 1 overwrites it (the comment at PERS_ACC)
      auto after = [&](int t) {
        if (!has_next) return;
        if (t == 2) pers_wide_reduce(smem, tid);
        if (t == 3) pers_coop_dma<FL, WIDE>(p, smem, wave, lane, ntm * BIG_BM, ntn * BIG_BN, 1);
      };
      if constexpr (WIDE)
        big8_loop<PERS_X, true, decltype(pre1), decltype(mid), (ER > 0 ? 4 : 0), decltype(last),
                  (ER > 1 ? 4 : 0), decltype(last3), P, KT2, U2, decltype(after)>(
            p, smem, acc, wave, ln, wm, wn, m0, n0, nk, cont, ntm * BIG_BM, ntn * BIG_BN, pre1, mid,
            last, last3, par, after);
      else
        big8_loop<PERS_X, true, decltype(pre1), decltype(mid), (ER > 0 ? 4 : 0), decltype(last),
                  (ER > 1 ? 4 : 0), decltype(last3), P, KT2, U2>(
            p, smem, acc, wave, ln, wm, wn, m0, n0, nk, cont, ntm * BIG_BM, ntn * BIG_BN, pre1, mid,
            last, last3, par);
      if (has_next && !cont) big8_prologue(p, smem, wave, lane, ntm * BIG_BM, ntn * BIG_BN, nk);
    } else {
      big8_loop<PERS_X, false, NoOp, NoOp, (ER > 0 ? 4 : 0), decltype(last), (ER > 1 ? 4 : 0),
                decltype(last3), P, KT2, U2>(p, smem, acc, wave, ln, wm, wn, m0, n0, nk, cont, ntm * BIG_BM,
                                    ntn * BIG_BN, {}, {}, last, last3, par);
      pers_coef<FL>(p, smem, tid);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      big8_bar();
      if (has_next) {
        pers_coop_dma<FL>(p, smem, wave, lane, ntm * BIG_BM, ntn * BIG_BN);
        if (!cont) big8_prologue(p, smem, wave, lane, ntm * BIG_BM, ntn * BIG_BN, nk);
      }
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    const bool interior = (m0 + BIG_BM <= p.M) && (n0 + BIG_BN <= p.N);
    pers_epilogue<FL, PADN, ER>(p, smem, acc, wave, wm, wn, m0, n0, tn, lane, interior, rre, npar);
    if (!has_next) break;
    if (!interior) wait_vmcnt0();
    par = npar;
    tile = next;
    tm = ntm;
    tn = ntn;
  }
}

template <int FL, bool PADN = true, bool WIDE = false>
__global__ __launch_bounds__(512, 2) void gemm_pers_kernel(GemmParams p, int total) {
  __shared__ __attribute__((aligned(16))) char smem[WIDE ? PERS_LDS_WIDE : PERS_LDS_ALL];
  const int G = gridDim.x;  // XCD-aware order when a multiple of 8
  const int tile = (G & 7) ? (int)blockIdx.x : (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3);
  {
    int tm, tn;
    if (!pers_tile(tile, G, p.ntiles, p.xgroups, total, tm, tn)) return;
  }
  if constexpr ((FL & EPI_GATHER) != 0) {
    MergeParams q;
    static_cast<GemmParams&>(q) = p;
    pers_run<FL, PADN, MergeParams, WIDE>(q, total, tile, smem);
  } else if constexpr ((FL & EPI_SPLIT) != 0) {
    UnfoldParams q;
    static_cast<GemmParams&>(q) = p;
    pers_run<FL, PADN, UnfoldParams, WIDE>(q, total, tile, smem);
  } else {
    pers_run<FL, PADN, GemmParams, WIDE>(p, total, tile, smem);
  }
}

}  // namespace

}  // namespace evt
