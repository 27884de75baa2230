// Shared pieces of the GEMM kernels (included by gemm.hip): the MFMA wrappers, the XCD-aware tile
// remap and the staged row-major epilogue ("epi_rows") of the 128x128 and 256x256 kernels.
#pragma once
#include <type_traits>

#include "common.h"
#include "evt_internal.h"

namespace evt {

namespace {

constexpr int ROWB = 128;                       // bytes of K per row per stage
constexpr int TILE_BYTES = GEMM_BM * ROWB;      // 16 KiB per operand tile
constexpr int STAGE_BYTES = 2 * TILE_BYTES;     // A + W

template <typename T> struct Mma;
template <> struct Mma<bf16> {
  static __device__ __forceinline__ void run(const u32x4& a, const u32x4& b, f32x4& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};
template <> struct Mma<float> {
  static __device__ __forceinline__ void run(const u32x4& a, const u32x4& b, f32x4& c) {
    const f32x4 af = __builtin_bit_cast(f32x4, a), bf = __builtin_bit_cast(f32x4, b);
#pragma unroll
    for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_16x16x4f32(af[e], bf[e], c, 0, 0, 0);
  }
};

// Bijective XCD-aware remap: blocks b and b+8 share an XCD (round-robin dispatch), so give each
// XCD a contiguous range of logical tiles (tile order: all N tiles of one M block consecutively,
// so an XCD's L2 keeps the A panel while it sweeps N).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int xcd = bid & 7, local = bid >> 3, q8 = nwg >> 3, r8 = nwg & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + local;
}

// Load 4 per-column fp32 values (zero past N).
__device__ __forceinline__ f32x4 col4(const float* v, int n, int N, bool full) {
  if (full) return load4(v + n);
  f32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = (n + j < N) ? v[n + j] : 0.f;
  return r;
}

// LayerNorm coefficients of one row from its per-slab partial statistics
// stats[row][slot][2] = (sum, sumsq), summed over the slots in a fixed order (deterministic).
__device__ __forceinline__ void ln_coef(const float* stats, int nslots, int64_t row, float inv_d,
                                        float eps, float& mu, float& r) {
  const float2* st = (const float2*)(stats + 2 * nslots * row);
  float s1 = 0.f, s2 = 0.f;
  for (int j = 0; j < nslots; ++j) {
    const float2 v = st[j];
    s1 += v.x;
    s2 += v.y;
  }
  mu = s1 * inv_d;
  r = rsqrtf(fmaxf(s2 * inv_d - mu * mu, 0.f) + eps);
}

// Staged-tile addressing: fp32 rows of 512 B (128 columns), 16-B chunk c of row r at
// c ^ (r & 7): conflict-free for the 16-B fragment writes and the row reads.
__device__ __forceinline__ int stg_off(int row, int chunk) { return row * 512 + ((chunk ^ (row & 7)) << 4); }

// Broadcast the value held by lane `l0` (lanes 0-31) or `l0 + 1` (lanes 32-63): per-row
// coefficients of the two rows an iteration covers, with two v_readlane (no LDS traffic).
__device__ __forceinline__ float row_bcast(float v, int l0, int sub) {
  const int a = __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l0);
  const int b = __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l0 + 1);
  return __builtin_bit_cast(float, sub ? b : a);
}

// Row-major epilogue over the 32 staged rows [row_lo, row_lo+32) of one wave (2 rows per
// iteration: lane>>5) of a staged 128-column slab; lane chunk c = lane & 31 holds global columns
// n .. n+3 (n supplied by the caller: the slab need not be contiguous). Per-row LayerNorm
// coefficients are computed once per lane (lane c: row row_lo + c) and broadcast with readlane.
// EPI_STATS: each lane parks its 4-column partial (sum, sumsq) of the stored values in the LDS
// row it has just consumed; at the end every row's 32 partials are summed in a fixed order and
// written to stats slot `slot` of that row (no atomics: bitwise reproducible).
template <typename T, int FL, bool INTERIOR>
__device__ __forceinline__ void epi_rows_t(const GemmParams& p, EVT_LDS char* stg, int m0, int n,
                                           int row_lo, int lane, int slot) {
  typedef typename std::conditional<(FL & EPI_OUT_F32) != 0, float, T>::type TO;
  constexpr bool interior = INTERIOR;  // interior tiles: no per-row / per-column range checks
  const int sub = lane >> 5, c = lane & 31;
  const bool col_ok = interior || n < p.N;
  const bool full = interior || (p.vec_ok && n + 4 <= p.N);
  f32x4 bias4 = f32x4{0.f, 0.f, 0.f, 0.f}, cs4 = bias4, g4 = bias4, b4 = bias4;
  if (col_ok) {
    if (FL & EPI_BIAS) bias4 = col4(p.bias, n, p.N, full);
    if (FL & EPI_LNIN) cs4 = col4(p.colsum, n, p.N, full);
    if (FL & EPI_RESLN) {
      g4 = col4(p.rgamma, n, p.N, full);
      b4 = col4(p.rbeta, n, p.N, full);
    }
  }
  // per-row LayerNorm coefficients: lane c (both halves) owns row row_lo + c
  const int64_t rs_step = p.rs_step > 1 ? p.rs_step : 1;  // rstats / stats_out rows per row m
  float in_mu = 0.f, in_r = 0.f, rs_mu = 0.f, rs_r = 0.f;
  if (FL & (EPI_LNIN | EPI_RESLN)) {
    const int mr = m0 + row_lo + c;
    if (interior || mr < p.M) {
      if (FL & EPI_LNIN)
        ln_coef(p.stats_in, p.nslots, (int64_t)mr * (p.stats_step > 1 ? p.stats_step : 1), p.inv_d,
                p.eps, in_mu, in_r);
      if (FL & EPI_RESLN) ln_coef(p.rstats, p.nslots, (int64_t)mr * rs_step, p.inv_d, p.eps, rs_mu, rs_r);
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    // two groups of 8 iterations: bounds how many loads the scheduler hoists (VGPR pressure)
    if (i == 8) __builtin_amdgcn_sched_barrier(0);
    const int row = row_lo + 2 * i + sub;
    const int m = m0 + row;
    const bool ok = col_ok && (interior || m < p.M);
    f32x4 v = *(const EVT_LDS f32x4*)(stg + stg_off(row, c));
    int64_t orow = m;
    if (FL & EPI_LNIN) {
      const float mu = row_bcast(in_mu, 2 * i, sub), r = row_bcast(in_r, 2 * i, sub);
      // f32: gemm_nt_kernel subtracted mu from the A rows, acc is (x - mu) . W' already
      if constexpr (std::is_same<T, float>::value) v = v * r + bias4;
      else v = v * r - cs4 * (r * mu) + bias4;
    } else if (FL & EPI_BIAS) {
      v += bias4;
    }
    if (FL & (EPI_GELU | EPI_GELU_ERF))
      v = gelu4(v, (FL & EPI_GELU) ? 0 : std::is_same<T, bf16>::value ? 2 : 1);
    if (FL & EPI_POS) {
      const int img = m / p.P, t = m - img * p.P;
      orow = (int64_t)img * (p.P + 1) + 1 + t;
      if (ok) v += col4(p.pos + (int64_t)(t + 1) * p.ldp, n, p.N, full);
    }
    if (FL & EPI_RESID) {
      f32x4 rv = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ok) {
        const T* rp = (const T*)p.resid + (int64_t)m * p.ldr + n;
        if (full) rv = load4(rp);
        else
          for (int j = 0; j < 4; ++j) rv[j] = (n + j < p.N) ? to_f32(rp[j]) : 0.f;
      }
      if (FL & EPI_RESLN) {
        const float mu = row_bcast(rs_mu, 2 * i, sub), r = row_bcast(rs_r, 2 * i, sub);
        rv = (rv - mu) * r * g4 + b4;
      }
      v += rv;
    }
    if (ok) {
      TO* cp = (TO*)p.C + orow * p.ldc + n;
      if (full) store4_nt(cp, v);
      else
        for (int j = 0; j < 4; ++j)
          if (n + j < p.N) cp[j] = from_f32<TO>(v[j]);
    }
    if (FL & EPI_STATS) {
      // partial statistics of the values as stored (what the next LayerNorm reads), parked in
      // the first 512 B of row row_lo + 2i, which both half-waves have already read
      float s1 = 0.f, s2 = 0.f;
      if (ok) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float q = (full || n + j < p.N) ? to_f32(from_f32<TO>(v[j])) : 0.f;
          s1 += q;
          s2 += q * q;
        }
      }
      *(EVT_LDS f32x2*)(stg + (row_lo + 2 * i) * 512 + sub * 256 + c * 8) = f32x2{s1, s2};
    }
  }
  if (FL & EPI_STATS) {
    // lane (q = lane & 31, hf = lane >> 5): row row_lo + q, partials [16 hf, 16 hf + 16)
    const int q = lane & 31, hf = lane >> 5;
    const EVT_LDS char* src = stg + (row_lo + (q & ~1)) * 512 + (q & 1) * 256 + hf * 128;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const f32x4 v = *(const EVT_LDS f32x4*)(src + j * 16);
      s1 += v[0] + v[2];
      s2 += v[1] + v[3];
    }
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    const int m = m0 + row_lo + q;
    if (hf == 0 && (interior || m < p.M)) {
      int64_t orow = m;
      if (FL & EPI_POS) {
        const int img = m / p.P, t = m - img * p.P;
        orow = (int64_t)img * (p.P + 1) + 1 + t;
      }
      *(f32x2*)(p.stats_out + 2 * (p.nslots * orow * rs_step + slot)) = f32x2{s1, s2};
    }
  }
}

// bf16-output form of epi_rows: every lane owns 8 consecutive columns (two staged chunks) of one
// row, 4 rows per iteration, so each output store is 16 B per lane (dwordx4). Measured: the
// 8-B-store epilogue is store-issue bound (writing fp32 with 16-B stores was faster than bf16
// with 8-B stores). Per-row coefficients come from lane (4i + q) via ds_bpermute; statistics
// partials (16 per row) are parked in the row just consumed and summed in a fixed order.
// Requires p.vec_ok >= 2 (ldc, ldr, ldp multiples of 8); n = first of the lane's 8 columns.
template <int FL, bool INTERIOR>
__device__ __forceinline__ void epi_rows8_t(const GemmParams& p, EVT_LDS char* stg, int m0, int n,
                                            int row_lo, int lane, int slot) {
  constexpr bool interior = INTERIOR;
  const int q = lane >> 4, c8 = lane & 15;
  const bool col_ok = interior || n < p.N;
  const bool full = interior || n + 8 <= p.N;
  f32x4 bias4[2], cs4[2], g4[2], b4[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    bias4[h] = cs4[h] = g4[h] = b4[h] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool fh = interior || n + 4 * h + 4 <= p.N;
    if (col_ok) {
      if (FL & EPI_BIAS) bias4[h] = col4(p.bias, n + 4 * h, p.N, fh);
      if (FL & EPI_LNIN) cs4[h] = col4(p.colsum, n + 4 * h, p.N, fh);
      if (FL & EPI_RESLN) {
        g4[h] = col4(p.rgamma, n + 4 * h, p.N, fh);
        b4[h] = col4(p.rbeta, n + 4 * h, p.N, fh);
      }
    }
  }
  const int64_t rs_step = p.rs_step > 1 ? p.rs_step : 1;  // rstats / stats_out rows per row m
  float in_mu = 0.f, in_r = 0.f, rs_mu = 0.f, rs_r = 0.f;  // lane c: row row_lo + (c & 31)
  if (FL & (EPI_LNIN | EPI_RESLN)) {
    const int mr = m0 + row_lo + (lane & 31);
    if (interior || mr < p.M) {
      if (FL & EPI_LNIN)
        ln_coef(p.stats_in, p.nslots, (int64_t)mr * (p.stats_step > 1 ? p.stats_step : 1), p.inv_d,
                p.eps, in_mu, in_r);
      if (FL & EPI_RESLN) ln_coef(p.rstats, p.nslots, (int64_t)mr * rs_step, p.inv_d, p.eps, rs_mu, rs_r);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    // bound how many iterations' loads the scheduler hoists (VGPR pressure: the other half of
    // the accumulators is still live in pass 0)
    if ((FL & EPI_RESID) ? (i & 1) == 0 && i > 0 : i == 4) __builtin_amdgcn_sched_barrier(0);
    const int row = row_lo + 4 * i + q;
    const int m = m0 + row;
    const bool ok = col_ok && (interior || m < p.M);
    const int src = (4 * i + q) * 4;  // ds_bpermute byte index of the lane holding this row
    f32x4 v[2];
    v[0] = *(const EVT_LDS f32x4*)(stg + stg_off(row, 2 * c8));
    v[1] = *(const EVT_LDS f32x4*)(stg + stg_off(row, 2 * c8 + 1));
    int64_t orow = m;
    if (FL & EPI_LNIN) {
      const float mu = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, in_mu)));
      const float r = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, in_r)));
#pragma unroll
      for (int h = 0; h < 2; ++h) v[h] = v[h] * r - cs4[h] * (r * mu) + bias4[h];
    } else if (FL & EPI_BIAS) {
      v[0] += bias4[0];
      v[1] += bias4[1];
    }
    if (FL & (EPI_GELU | EPI_GELU_ERF)) {
#pragma unroll
      for (int h = 0; h < 2; ++h) v[h] = gelu4(v[h], (FL & EPI_GELU) ? 0 : 2);  // bf16 only
    }
    if (FL & EPI_POS) {
      const int img = m / p.P, t = m - img * p.P;
      orow = (int64_t)img * (p.P + 1) + 1 + t;
      if (ok) {
        const float* pr = p.pos + (int64_t)(t + 1) * p.ldp;
        v[0] += col4(pr, n, p.N, interior || n + 4 <= p.N);
        v[1] += col4(pr, n + 4, p.N, full);
      }
    }
    if (FL & EPI_RESID) {
      f32x4 rv[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      if (ok) {
        const bf16* rp = (const bf16*)p.resid + (int64_t)m * p.ldr + n;
        if (full) {
          const bf16x8 r8 = __builtin_bit_cast(bf16x8, *(const u32x4*)rp);
          rv[0] = f32x4{(float)r8[0], (float)r8[1], (float)r8[2], (float)r8[3]};
          rv[1] = f32x4{(float)r8[4], (float)r8[5], (float)r8[6], (float)r8[7]};
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (n + j < p.N) rv[j >> 2][j & 3] = to_f32(rp[j]);
        }
      }
      if (FL & EPI_RESLN) {
        const float mu = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, rs_mu)));
        const float r = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, rs_r)));
#pragma unroll
        for (int h = 0; h < 2; ++h) rv[h] = (rv[h] - mu) * r * g4[h] + b4[h];
      }
      v[0] += rv[0];
      v[1] += rv[1];
    }
    const bf16x8 o = {(bf16)v[0][0], (bf16)v[0][1], (bf16)v[0][2], (bf16)v[0][3],
                      (bf16)v[1][0], (bf16)v[1][1], (bf16)v[1][2], (bf16)v[1][3]};
    if (ok) {
      bf16* cp = (bf16*)p.C + orow * p.ldc + n;
      if (full) store_b128_nt(cp, __builtin_bit_cast(u32x4, o));
      else
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (n + j < p.N) cp[j] = o[j];
    }
    if (FL & EPI_STATS) {
      float s1 = 0.f, s2 = 0.f;
      if (ok) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float x = (full || n + j < p.N) ? (float)o[j] : 0.f;
          s1 += x;
          s2 += x * x;
        }
      }
      // park in row `row` (read above by these same lanes): partial c8 at byte c8 * 8
      *(EVT_LDS f32x2*)(stg + row * 512 + c8 * 8) = f32x2{s1, s2};
    }
  }
  if (FL & EPI_STATS) {
    // lane (r = lane & 31, hf = lane >> 5): row row_lo + r, partials [8 hf, 8 hf + 8)
    const int r = lane & 31, hf = lane >> 5;
    const EVT_LDS char* src = stg + (row_lo + r) * 512 + hf * 64;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 v = *(const EVT_LDS f32x4*)(src + j * 16);
      s1 += v[0] + v[2];
      s2 += v[1] + v[3];
    }
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    const int m = m0 + row_lo + r;
    if (hf == 0 && (interior || m < p.M)) {
      int64_t orow = m;
      if (FL & EPI_POS) {
        const int img = m / p.P, t = m - img * p.P;
        orow = (int64_t)img * (p.P + 1) + 1 + t;
      }
      *(f32x2*)(p.stats_out + 2 * (p.nslots * orow * rs_step + slot)) = f32x2{s1, s2};
    }
  }
}

// n4: first column of the lane in the 4-column layout (lane chunk c = lane & 31);
// n8: first column in the 8-column layout (lane chunks 2 (lane & 15), +1).
// ONLY8: the caller guarantees p.vec_ok >= 2 (the 256x256 kernel), so only the 8-column form is
// compiled in (the dead 4-column form otherwise costs registers: hoisted addresses spill).
template <typename T, int FL, bool ONLY8 = false>
__device__ __forceinline__ void epi_rows(const GemmParams& p, EVT_LDS char* stg, int m0, int n4,
                                         int n8, int row_lo, int lane, int slot, bool interior) {
  constexpr bool out16 = std::is_same<T, bf16>::value && !(FL & EPI_OUT_F32);
  if (out16 && (ONLY8 || p.vec_ok >= 2)) {
    if (interior) epi_rows8_t<FL, true>(p, stg, m0, n8, row_lo, lane, slot);
    else epi_rows8_t<FL, false>(p, stg, m0, n8, row_lo, lane, slot);
    return;
  }
  if constexpr (!(out16 && ONLY8)) {
    if (interior) epi_rows_t<T, FL, true>(p, stg, m0, n4, row_lo, lane, slot);
    else epi_rows_t<T, FL, false>(p, stg, m0, n4, row_lo, lane, slot);
  }
}

}  // namespace

}  // namespace evt
