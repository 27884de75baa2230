// The core of the Swin window-attention kernels, defined once and templated on the window size
// W (7 or 12; head size 32), the sibling of attn_scores.h. Its users:
//
//   swin.hip       window_attn_bf16<W> (window_attn_bf16_kernel, window12_attn_bf16_kernel) and
//                  phase P2 of swin_attn96_kernel: everything below. The fp32 parity kernels and
//                  the swin_attn96 prefetch: WinGeom only.
//   attn_maps.hip  window_probs_bf16_kernel<W>: geometry, traits and key tables. Its score step
//                  stays its own (score_tile gave the same bits but measured 7 to 9 % slower
//                  there at w = 7, profiles/window_core_speed.json), as do its reductions, its
//                  1 / sum and its stores. window_probs_f32_kernel<W>: WinGeom and the traits.
//
//   WinTraits<W>   the compile-time constants: tokens, tiles, t / W as a multiply-shift, the
//                  compact relative-position table's row and its offset forms a(q), b(k)
//   WinGeom<W>     window-local token -> image-local raster row with the cyclic shift; the window
//                  type and the SW-MSA region code of a token
//   key_tables     per-lane table offsets b(k) and byte-packed region codes of a lane's keys
//   score_tile     S^T = K Q^T of one query tile on the MFMA, scale + bias, region mask, key padding
//   softmax_exp    row maximum and sum (permlane butterflies), exp2 in place
//   pv_accumulate  O^T += V^T P^T with transposed LDS reads of V
//
// The file is compiled with -ffp-contract=on: a floating-point expression contracts only within
// itself, so every expression below keeps its boundaries (score * scale + bias is one).
#pragma once
#include <cmath>

#include "common.h"

namespace evt {

template <int W>
struct WinTraits {
  static_assert(W == 7 || W == 12, "window 7 or 12");
  static constexpr int N = W * W;                // tokens of a window
  static constexpr int NKT = (N + 15) / 16;      // 16-token MFMA tiles (the last one padded, w = 7)
  static constexpr int PV_STEPS = (NKT + 1) / 2;  // 32-key k-steps of P . V (w = 12: the fifth half
                                                  // empty)
  static constexpr int VROWS = 32 * PV_STEPS;    // key rows of a V tile in LDS
  static constexpr int TW = 2 * W - 1;           // side of the relative-position table
  static constexpr int CROW = (TW * TW + 63) / 64 * 64;  // floats of a head's compact table: entry
                                                         // r = table[r][h] log2 e, 0 past TW^2
  // t / W for every token of the padded window
  static constexpr int div(int t) { return W == 7 ? (t * 37) >> 8 : (t * 171) >> 11; }
  // bias(q, k) = T[TW (qi - ki + W - 1) + (qj - kj + W - 1)] = T[a(q) - b(k)]
  static constexpr int a(int qi, int q) { return (W - 1) * qi + q + TW * (W - 1) + (W - 1); }
  static constexpr int b(int ki, int k) { return (W - 1) * ki + k; }
  // tokens past N - 1 of the last tile (w = 7) repeat token N - 1 and are masked
  static constexpr int clamp(int t) { return N % 16 ? (t < N - 1 ? t : N - 1) : t; }
};
template <int W>
constexpr bool win_div_exact() {
  for (int t = 0; t < WinTraits<W>::VROWS; ++t)
    if (WinTraits<W>::div(t) != t / W) return false;
  return true;
}
static_assert(win_div_exact<7>(), "(t * 37) >> 8 must equal t / 7 over the padded window");
static_assert(win_div_exact<12>(), "(t * 171) >> 11 must equal t / 12 over the padded window");
static_assert(WinTraits<7>::CROW == 192 && WinTraits<12>::CROW == 576, "compact table rows");

// Window `win` (row-major over the shifted frame's windows) of an R x R token map.
template <int W>
struct WinGeom {
  int R;
  int y0, x0;  // shifted-frame origin of the window (wy W + shift, wx W + shift)
  int wtype;   // 2 (last window row) + 1 (last window column) under a shift, else 0: the windows
               // that see the SW-MSA region split (and the w = 7 dense table's type)
  int cut;     // W - shift: first window-local row / column of the wrapped-around part
  unsigned mask;  // the region-code bits this window sees, in each of four bytes
  __device__ __forceinline__ WinGeom(int R_, int nwx, int shift, int win) : R(R_) {
    const int wy = win / nwx, wx = win - wy * nwx;
    y0 = wy * W + shift;
    x0 = wx * W + shift;
    wtype = shift ? (wy == nwx - 1 ? 2 : 0) + (wx == nwx - 1 ? 1 : 0) : 0;
    cut = W - shift;
    mask = ((wtype & 2) ? 0x01010101u : 0u) | ((wtype & 1) ? 0x02020202u : 0u);
  }
  // image-local raster row of window token t (with the cyclic shift)
  __device__ __forceinline__ int row(int t) const {
    const int i = WinTraits<W>::div(t), j = t - W * i;
    int y = y0 + i, x = x0 + j;
    if (y >= R) y -= R;
    if (x >= R) x -= R;
    return y * R + x;
  }
  // region code of window-local (row i, column j): bit 0: i >= cut in a window of the last window
  // row, bit 1: j >= cut in one of the last window column. Attention stays within one code.
  __device__ __forceinline__ unsigned code(int i, int j) const {
    return ((i >= cut ? 1u : 0u) | (j >= cut ? 2u : 0u)) & mask & 3u;
  }
};

// Per-lane tables of lane group g's keys k = 16 kt + 4 g + j (MFMA result rows): the offset
// b(k) into the compact table and the region codes, one byte per j. Only the final `& mask`
// depends on the window, so a kernel that loops over windows keeps the rest out of its loop.
template <int W>
__device__ __forceinline__ void key_tables(const WinGeom<W>& G, int g,
                                           int (&kofs)[WinTraits<W>::NKT][4],
                                           unsigned (&kc)[WinTraits<W>::NKT]) {
  using T = WinTraits<W>;
#pragma unroll
  for (int kt = 0; kt < T::NKT; ++kt) {
    kc[kt] = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = T::clamp(16 * kt + 4 * g + j), ki = T::div(k);
      kofs[kt][j] = T::b(ki, k);  // in floats: as negated bytes each costs a full 32-bit multiply
      kc[kt] |= ((ki >= G.cut ? 1u : 0u) | (k - W * ki >= G.cut ? 2u : 0u)) << (8 * j);
    }
    kc[kt] &= G.mask;
  }
}

// Scores of one query tile: s[kt][j] = S^T[key 16 kt + 4 g + j][query q] in the log2 domain, q the
// lane's (clamped) window-local query token, kf / qf the K tiles' and the query tile's fragments
// (lane: token 16 i + (lane & 15), d 8 g .. 8 g + 7), Ts the head's compact table in LDS. Keys of
// another SW-MSA region and the keys past N - 1 get -inf (the reference's -100 leaves e^-100
// relative weights, below fp32 resolution against the row maximum's 1).
template <int W>
__device__ __forceinline__ void score_tile(const WinGeom<W>& G, const u32x4 (&kf)[WinTraits<W>::NKT],
                                           u32x4 qf, int q, int g, const EVT_LDS char* Ts,
                                           float scale_log2,
                                           const int (&kofs)[WinTraits<W>::NKT][4],
                                           const unsigned (&kc)[WinTraits<W>::NKT],
                                           f32x4 (&s)[WinTraits<W>::NKT]) {
  using T = WinTraits<W>;
  const int qi = T::div(q);
  const EVT_LDS float* Tq = (const EVT_LDS float*)Ts + T::a(qi, q);
  const unsigned cq = G.code(qi, q - W * qi) * 0x01010101u;
  const float NEG = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < T::NKT; ++kt) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kf[kt]),
                                                    __builtin_bit_cast(bf16x8, qf), acc, 0, 0, 0);
  }
  // scale + bias on packed pairs, then the masks
  const f32x2 sc2 = {scale_log2, scale_log2};
#pragma unroll
  for (int kt = 0; kt < T::NKT; ++kt) {
    f32x4 bv;
#pragma unroll
    for (int j = 0; j < 4; ++j) bv[j] = Tq[-kofs[kt][j]];
    const f32x2 lo = f32x2{s[kt][0], s[kt][1]} * sc2 + f32x2{bv[0], bv[1]};
    const f32x2 hi = f32x2{s[kt][2], s[kt][3]} * sc2 + f32x2{bv[2], bv[3]};
    f32x4 v = {lo[0], lo[1], hi[0], hi[1]};
    if (G.wtype) {  // SW-MSA window on the last row / column: keys of another region
      const unsigned x = kc[kt] ^ cq;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = ((x >> (8 * j)) & 3u) ? NEG : v[j];
    }
    s[kt] = v;
  }
  if constexpr (T::N % 16 != 0) {
    // the padding of the last tile: its first PADK keys are real (w = 7: key 48 of 48 .. 63), so
    // for j >= PADK the mask is a compile-time constant and the compiler drops those scores
    constexpr int PADK = T::N - 16 * (T::NKT - 1);
    f32x4 v = s[T::NKT - 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (j >= PADK || 4 * g + j >= PADK) ? NEG : v[j];
    s[T::NKT - 1] = v;
  }
}

// Butterfly max / sum over lanes l ^ 16 and l ^ 32 on the VALU: v_permlane16_swap / 32_swap of a
// value with itself leave the two halves of each row pair (of the wave) in the two results, so one
// max / add gives every lane the reduction (no LDS round trip as with ds_bpermute).
__device__ __forceinline__ float bfly_max_16_32(float x) {
  unsigned u = __builtin_bit_cast(unsigned, x);
  const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  x = fmaxf(__builtin_bit_cast(float, (unsigned)a[0]), __builtin_bit_cast(float, (unsigned)a[1]));
  u = __builtin_bit_cast(unsigned, x);
  const auto c = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return fmaxf(__builtin_bit_cast(float, (unsigned)c[0]), __builtin_bit_cast(float, (unsigned)c[1]));
}
__device__ __forceinline__ float bfly_sum_16_32(float x) {
  unsigned u = __builtin_bit_cast(unsigned, x);
  const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  x = __builtin_bit_cast(float, (unsigned)a[0]) + __builtin_bit_cast(float, (unsigned)a[1]);
  u = __builtin_bit_cast(unsigned, x);
  const auto c = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __builtin_bit_cast(float, (unsigned)c[0]) + __builtin_bit_cast(float, (unsigned)c[1]);
}

// s -> 2^(s - row maximum) in place; returns the row sum. The order of the additions is each
// kernel's own: four tiles sum as a tree, nine in sequence.
template <int W>
__device__ __forceinline__ float softmax_exp(f32x4 (&s)[WinTraits<W>::NKT]) {
  constexpr int NKT = WinTraits<W>::NKT;
  float m[NKT], l[NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) m[kt] = fmaxf(fmaxf(s[kt][0], s[kt][1]), fmaxf(s[kt][2], s[kt][3]));
  float mx;
  if constexpr (NKT == 4) {
    mx = fmaxf(fmaxf(m[0], m[1]), fmaxf(m[2], m[3]));
  } else {
    mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) mx = fmaxf(mx, m[kt]);
  }
  mx = bfly_max_16_32(mx);
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
    for (int j = 0; j < 4; ++j) s[kt][j] = __builtin_amdgcn_exp2f(s[kt][j] - mx);
    l[kt] = (s[kt][0] + s[kt][1]) + (s[kt][2] + s[kt][3]);
  }
  float sum;
  if constexpr (NKT == 4) {
    sum = (l[0] + l[1]) + (l[2] + l[3]);
  } else {
    sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) sum += l[kt];
  }
  return bfly_sum_16_32(sum);
}

// o[dt][j] = O^T[d = 16 dt + 4 g + j][query] += V^T P^T: P = s rounded to bf16, V^T from
// ds_read_tr16_b64 reads of the LDS V rows (key rows of VROW bytes; V: the head's first column).
// SWZ: the 16-B chunks of a row are swizzled with (row >> 2) & 3, as the LDS-DMA of the V tile
// stores them. An odd tile count leaves the last step's upper 16 keys at P = 0 (their V rows must
// be finite).
template <int W, int VROW, bool SWZ>
__device__ __forceinline__ void pv_accumulate(const f32x4 (&s)[WinTraits<W>::NKT],
                                              const EVT_LDS char* V, int lane, f32x4 (&o)[2]) {
  constexpr int NKT = WinTraits<W>::NKT;
  const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
#pragma unroll
  for (int ks = 0; ks < WinTraits<W>::PV_STEPS; ++ks) {
    bf16x8 pf;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pf[j] = (bf16)s[2 * ks][j];
      pf[4 + j] = 2 * ks + 1 < NKT ? (bf16)s[(2 * ks + 1) % NKT][j] : (bf16)0.f;
    }
    const int key0 = ks * 32 + 4 * g + tq;  // and key0 + 16: same (row >> 2) & 3 swizzle
    const int sw = SWZ ? (key0 >> 2) & 3 : 0;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const int chunk = 2 * dt + (tp >> 1);
      const int off = ((chunk ^ sw) * 16) + (tp & 1) * 8;
      const i16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((EVT_LDS i16x4*)(V + key0 * VROW + off));
      const i16x4 v1 =
          __builtin_amdgcn_ds_read_tr16_b64_v4i16((EVT_LDS i16x4*)(V + (key0 + 16) * VROW + off));
      const i16x8 vv = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vv), pf, o[dt], 0,
                                                      0, 0);
    }
  }
}

}  // namespace evt
