// Attention-map export (include/evt_attention_maps.h): the softmax probabilities the fused
// attention kernels (attention.hip) form in registers and discard, written as fp32 into
// caller-owned memory, either the row of query token 0 (CLS) or every row.
//
//   out[b][h][i][j] = softmax_j(q_i . k_j * h_k^-0.5),  i < nq (1 or N), j < N
//
// of the q and k the QKV GEMM stored (bf16 or fp32): scores accumulated in fp32, the statistics in
// fp32, the result normalised in fp32. This is the probability BEFORE the bf16 rounding the fused
// bf16 kernels apply to P for the P.V product, and it is normalised by 1 / l where they normalise
// O: it is what a user compares against softmax(q k^T scale), not a dump of their registers.
//
// One code path for both modes. A workgroup (4 waves) takes (image, head, 64 queries), a wave one
// 16-query tile, S^T = K Q^T as in attention.hip (one query per lane column, four consecutive keys
// per lane), in two passes over 64-key blocks for every N up to EVT_ATTN_MAX_TOKENS:
//
//   pass 1  the running max m and the running sum l of 2^((s - m) c) (the online softmax of
//           attn_long_*_kernel without the O accumulators)
//   pass 2  the scores again, p = 2^((s - m) c) / l, stored
//
// The scores and pass 1 are AttnScores (attn_scores.h), the one definition this kernel shares
// with the head statistics and the head mean below: what those two call "the export's" m, l and
// scores is the same code. Each kernel here holds only its own pass 2.
//
// Recomputing costs twice the MFMA work and no trip of fp32 scores through memory; ALL mode is
// bound by its B H N^2 4 bytes of stores, CLS mode by the read of K. MFMA columns are independent
// and the CLS row is column 0 of tile 0 of the same kernel, so out_cls == out_all[:, :, 0] bitwise
// (a GEMV for the CLS row would not be); rows >= nq of tile 0 are computed and not stored.
// (s - m) c <= 0 exactly (c > 0, checked by the launcher) and l >= 1 (the maximum's own term), so
// every value is in [0, 1]; keys past N get -inf scores and are not stored.
//
// bf16: v_mfma_f32_16x16x32_bf16, every head size zero-padded to DP = 32 / 64 / 96 / 128, each
// 64-key block of K staged to LDS through registers (the image of attn_gen_bf16_kernel), rows
// past N clamped; the token-major and the head-major layout (AttnParams sb / sh / ko) stage the
// same values, so their results are bitwise equal. fp32: exact v_mfma_f32_16x16x4_f32 with every
// operand straight from the qkv rows (the parity path, attn_long_f32_kernel's addressing).
//
// Stores. The MFMA result has one query per lane column: stored as it stands, a wave instruction
// would write 4-byte pieces of 16 rows. Each wave instead passes its 16 x 64 block of P through a
// private LDS tile and stores whole row segments, non-temporal (nothing on the forward re-reads
// them). A row of N floats starts 16-byte aligned only when its element offset is a multiple of
// 4 (N = 197, 257, 577: one row in four), so two forms exist:
//   dword  a lane per key, 64 consecutive floats (256 B) of one row per instruction
//          (store_tile_rows, attn_scores.h)
//   wide   a lane per aligned group of 4 keys, four rows per instruction: 16-B stores
//          (store4_nt) for the aligned body of the row's segment, 4-B stores for the at most 3
//          floats before it and after it
// The dword form is the one launched: measured on DeiT-base bf16 (197 tokens, ALL mode) it takes
// 75 us at 64 images and 510 us at 512 against 125 and 833 us for the wide form, whose four rows
// per instruction and divergent edges cost more than its wider stores save (256 contiguous
// bytes per wave instruction already store at the full rate). EVT_ATTN_MAPS_STORE=wide selects
// the other form for a measurement (scripts/attention_maps_measure.py; DESIGN.md, attention maps).
// Every row and output offset is 64-bit (B H N^2 passes 2^31 elements at ordinary sizes).
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "attn_scores.h"
#include "common.h"
#include "evt_internal.h"
#include "window_scores.h"

namespace evt {

namespace {

using namespace scores;  // attn_scores.h

// A wave's P tile (and head_mean_kernel's (m, 1 / l) table) is its own: LDS operations of a wave
// complete in order, so a wave-level fence orders the writes before the reads (wave_lds_written)
// and the reads before the next block's writes (wave_lds_read).
__device__ __forceinline__ void wave_lds_written() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void wave_lds_read() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// T: bf16 (DP = h_k padded to 32 / 64 / 96 / 128) or float (DP = 64 / 128: feature groups of 64).
// nqb: 64-query groups per (image, head).
template <typename T, int DP, bool WIDE>
__global__ __launch_bounds__(256) void attn_probs_kernel(AttnParams p, int nq, int nqb,
                                                         float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool BF = sizeof(T) == 2;
  AttnScores<T, DP> sc(p, (EVT_LDS char*)smem + 4 * PTILE * 4);  // bf16: one K block, [64][DP]
  const int lane = sc.lane, wave = sc.tid >> 6, g = sc.g, c16 = sc.c16, N = sc.N, nkb = sc.nkb;
  EVT_LDS float* Ps = (EVT_LDS float*)smem + wave * PTILE;  // this wave's [16 queries][64 keys]
  int bh, qb;
  unswizzle_block(blockIdx.x, p.B * p.H, nqb, bh, qb);
  const int b = bh / p.H, h = bh - b * p.H;
  const int nqt = (nq + 15) >> 4;
  const int qt = qb * 4 + wave;
  const bool active = qt < nqt;  // wave-uniform
  if constexpr (!BF) {
    if (!active) return;  // no barrier in the fp32 kernel
  }
  sc.set_image(b);
  sc.set_tile(qt);
  sc.head(h);
  const float c = p.scale_log2;

  // ---- pass 1; nothing is staged yet, so no barrier ahead of its first block
  float m, l;
  sc.template pass1<false>(active, m, l);
  const float inv = 1.0f / l;

  // ---- pass 2: p = 2^((s - m) c) / l, through the wave's LDS tile, stored by rows
  const int64_t row0 = ((int64_t)bh * nq + (int64_t)qt * 16) * N;  // element offset of the tile's row 0
  for (int kb = 0; kb < nkb; ++kb) {
    if (!sc.template stage_block<true>(kb, active)) continue;
    f32x4 s[NKT];
    sc.scores(kb, s);
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      f32x4 pv;
#pragma unroll
      for (int j = 0; j < 4; ++j) pv[j] = ex2<BF>((s[kt][j] - m) * c) * inv;
      *(EVT_LDS f32x4*)(Ps + c16 * PROW + kt * 16 + 4 * g) = pv;
    }
    wave_lds_written();
    const int nk = min(KB, N - kb * KB);  // keys of this block
    if constexpr (!WIDE) {
      store_tile_rows<true>(Ps, out + row0, qt * 16, nq, kb * KB, nk, N, lane);
    } else {
      const int rr = lane >> 4, ql = lane & 15;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * i + rr;
        if (qt * 16 + r >= nq) continue;
        const int64_t e0 = row0 + (int64_t)r * N + kb * KB;  // key 0 of the block in this row
        const int a = (int)((-e0) & 3);                      // floats before the aligned body
        const EVT_LDS float* pr = Ps + r * PROW;
        float* dst = out + e0;
        const int lk = a + 4 * ql;
        if (lk + 3 < nk) {
          store4_nt(dst + lk, f32x4{pr[lk], pr[lk + 1], pr[lk + 2], pr[lk + 3]});
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (lk + j < nk) store1_nt(dst + lk + j, pr[lk + j]);
        }
        if (ql == 0) {
#pragma unroll
          for (int j = 0; j < 3; ++j)
            if (j < a && j < nk) store1_nt(dst + j, pr[j]);
        }
      }
    }
    wave_lds_read();
  }
}

// the store form (file header): dword unless EVT_ATTN_MAPS_STORE=wide asks for the other one
bool wide_stores() {
  const char* e = std::getenv("EVT_ATTN_MAPS_STORE");
  return e && std::strcmp(e, "wide") == 0;
}

}  // namespace

hipError_t attn_probs_launch(int dtype, const AttnParams& p_in, int nq, float* out, hipStream_t s) {
  if (p_in.B <= 0) return hipSuccess;
  AttnParams p;
  if (!prepare(dtype, p_in, out, p) || (nq != 1 && nq != p.N)) return hipErrorInvalidValue;
  const int nqb = ((nq + 15) / 16 + 3) / 4;
  if ((int64_t)p.B * p.H * nqb > INT32_MAX) return hipErrorInvalidValue;
  const bool wide = wide_stores();
  return dispatch(dtype, p.hd, [&](auto v) {
    using V = decltype(v);
    using T = typename V::type;
    const dim3 grid(p.B * p.H * nqb), block(256);
    const size_t lds = score_lds(sizeof(T), V::DP, true);
    if (wide)
      hipLaunchKernelGGL((attn_probs_kernel<T, V::DP, true>), grid, block, lds, s, p, nq, nqb, out);
    else
      hipLaunchKernelGGL((attn_probs_kernel<T, V::DP, false>), grid, block, lds, s, p, nq, nqb, out);
    return hipGetLastError();
  });
}

// ---- Head statistics (include/evt_head_stats.h) ------------------------------------------------
//
//   stats[b][h] = (confidence, entropy, distance, cls_mass)
//
// four reductions of the probabilities p_ij attn_probs_kernel forms, with no map store:
//   confidence  mean_i max_j p_ij                           = mean_i 1 / l_i (the maximum's term is 2^0)
//   entropy     mean_i -sum_j p_ij ln p_ij                  = mean_i ln l_i - (ln 2 / l_i) sum_j e_ij t_ij
//   distance    mean_{i >= prefix} sum_{j >= prefix} p_ij d(i, j)
//   cls_mass    mean_{i >= prefix} sum_{j < prefix} p_ij
// with t_ij = (s_ij - m_i) c <= 0, e_ij = 2^t_ij, l_i = sum_j e_ij and d the Euclidean distance of
// the patch-grid cells of tokens i and j (token t >= prefix: row (t - prefix) / grid_w, column
// (t - prefix) % grid_w).
//
// TWO PASSES, as attn_probs_kernel: pass 1 is AttnScores::pass1 (m, l), the code the export runs;
// pass 2 forms the scores again, through the same AttnScores::scores, and accumulates the three
// sums sum e t, sum_{j >= prefix} e d and sum_{j < prefix} e against the final m, so nothing is
// rescaled. This kernel's own: the cell geometry, those sums and the fp64 reduction.
//
// Keys past N carry -inf scores: t = -inf, e = 0. They are selected out of the e t sum by index (a
// product would be 0 * -inf = NaN; this file is compiled honouring NaN and inf); in the other two
// sums their e = 0 multiplies a finite d. A finite t whose e underflows contributes exactly 0.
// Key coordinates: one float-reciprocal division per lane per group of four consecutive keys per
// block ((r + 0.5) * (1 / grid_w), exact for r < 2^22 as in the GEMM's gathered loaders), the other
// three by stepping; d = sqrt(dy dy + dx dx) of small integers in fp32 (the sum exact, v_sqrt_f32).
//
// Determinism: one 4-wave workgroup per (image, head) walks the 64-query groups; a lane sums its
// query's values over the groups in fp64 (a mean of T fp32 values then carries one rounding, and
// q = 0 gives confidence = fl(1 / N) exactly), the wave's 16 queries are added by a butterfly, the
// four waves through LDS in wave order. No atomics, no scratch; the four floats leave as one 16-B
// store. Nothing depends on the batch position, and both qkv layouts stage the same values.
namespace {

template <typename T, int DP>
__global__ __launch_bounds__(256) void head_stats_kernel(AttnParams p, int prefix, int gw,
                                                         float inv_gw, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double red[4][4];
  constexpr bool BF = sizeof(T) == 2;
  AttnScores<T, DP> sc(p, (EVT_LDS char*)smem);  // bf16: one K block, [64][DP]
  const int tid = sc.tid, lane = sc.lane, wave = tid >> 6, g = sc.g, c16 = sc.c16;
  const int N = sc.N, nkb = sc.nkb;
  const int bh = blockIdx.x;
  const int b = bh / p.H, h = bh - b * p.H;
  sc.set_image(b);
  const int nqt = (N + 15) >> 4, nqb = (nqt + 3) >> 2;
  const float c = p.scale_log2;

  // grid cell (row, column) of patch r = token - prefix, as floats (a query below prefix or past N
  // gets a finite cell nobody reads)
  auto cell = [&](int r, float& y, float& x) {
    const int yi = (int)(((float)r + 0.5f) * inv_gw);
    y = (float)yi;
    x = (float)(r - yi * gw);
  };

  double a_conf = 0.0, a_ent = 0.0, a_dist = 0.0, a_cls = 0.0;  // this lane's query, over the groups
  for (int qb = 0; qb < nqb; ++qb) {
    const int qt = qb * 4 + wave, qi = qt * 16 + c16;
    const bool active = qt < nqt;  // wave-uniform
    if constexpr (!BF) {
      if (!active) continue;  // no barrier in the fp32 loops
    }
    sc.set_tile(qt);
    sc.head(h);
    // ---- pass 1; an earlier query group has staged a block before, so a barrier ahead of each
    float m, l;
    sc.template pass1<true>(active, m, l);

    // ---- pass 2: sum_j e t, sum_{j >= prefix} e d, sum_{j < prefix} e with e = 2^t, t = (s - m) c
    float qy, qx;
    cell(qi - prefix, qy, qx);
    float et = 0.f, ed = 0.f, ec = 0.f;
    for (int kb = 0; kb < nkb; ++kb) {
      if (!sc.template stage_block<true>(kb, active)) continue;
      f32x4 s[NKT];
      sc.scores(kb, s);
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        const int k0 = kb * KB + kt * 16 + 4 * g;  // this lane's four consecutive keys
        float ky, kx;  // the cell of key max(k0, prefix): it steps once a key is a patch
        cell(max(k0 - prefix, 0), ky, kx);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int key = k0 + j;
          const float t = (s[kt][j] - m) * c;
          const float e = ex2<BF>(t);
          et += key < N ? e * t : 0.f;
          const float dy = qy - ky, dx = qx - kx;
          const float d = __builtin_amdgcn_sqrtf(dy * dy + dx * dx);
          ed += key >= prefix ? e * d : 0.f;
          ec += key < prefix ? e : 0.f;
          if (key >= prefix) {  // the next key's cell
            kx += 1.f;
            if (kx >= (float)gw) {
              kx = 0.f;
              ky += 1.f;
            }
          }
        }
      }
    }
    et += __shfl_xor(et, 16, 64);
    et += __shfl_xor(et, 32, 64);
    ed += __shfl_xor(ed, 16, 64);
    ed += __shfl_xor(ed, 32, 64);
    ec += __shfl_xor(ec, 16, 64);
    ec += __shfl_xor(ec, 32, 64);
    if (active && qi < N) {  // l >= 1, et <= 0: 0 < 1 / l <= 1 and the entropy is >= 0
      const float inv = 1.0f / l;
      a_conf += (double)inv;
      a_ent += (double)(logf(l) - (0.6931471805599453f * inv) * et);
      if (qi >= prefix) {
        a_dist += (double)(ed * inv);
        a_cls += (double)fminf(ec * inv, 1.0f);
      }
    }
  }
  // the wave's 16 queries (the four lanes of a query hold the same values), then the four waves
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    a_conf += __shfl_xor(a_conf, o, 64);
    a_ent += __shfl_xor(a_ent, o, 64);
    a_dist += __shfl_xor(a_dist, o, 64);
    a_cls += __shfl_xor(a_cls, o, 64);
  }
  if (lane == 0) {
    red[wave][0] = a_conf;
    red[wave][1] = a_ent;
    red[wave][2] = a_dist;
    red[wave][3] = a_cls;
  }
  __syncthreads();
  if (tid == 0) {
    double t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    const double nall = (double)N, npatch = (double)(N - prefix);
    store_f32x4(out + (int64_t)bh * 4, f32x4{(float)(t[0] / nall), (float)(t[1] / nall),
                                             (float)(t[2] / npatch), (float)(t[3] / npatch)});
  }
}

}  // namespace

hipError_t head_stats_launch(int dtype, const AttnParams& p_in, int prefix, int grid_w, float* out,
                             hipStream_t s) {
  if (p_in.B <= 0) return hipSuccess;
  AttnParams p;
  if (!prepare(dtype, p_in, out, p) || prefix < 0 || prefix >= p.N || grid_w < 1 ||
      (p.N - prefix) % grid_w)
    return hipErrorInvalidValue;
  if ((int64_t)p.B * p.H > INT32_MAX) return hipErrorInvalidValue;
  return dispatch(dtype, p.hd, [&](auto v) {
    using V = decltype(v);
    using T = typename V::type;
    hipLaunchKernelGGL((head_stats_kernel<T, V::DP>), dim3(p.B * p.H), dim3(256),
                       score_lds(sizeof(T), V::DP, false), s, p, prefix, grid_w,
                       1.0f / (float)grid_w, out);
    return hipGetLastError();
  });
}

// ---- Head mean (include/evt_rollout.h) ---------------------------------------------------------
//
//   out[b][i][j] = (sum_h p[b][h][i][j]) * fl(1 / H)
//
// the mean over the heads of the probabilities attn_probs_kernel forms, fp32 [B][N][N], with no
// per-head map stored: the A operand of an attention-rollout step (rollout.hip). A workgroup (4
// waves) takes (image, 64 queries), a wave one 16-query tile, and loops over the heads inside:
//
//   pass 1  for every head: AttnScores::pass1, the export's (m, l) from the export's code; m and
//           1 / l of the wave's 16 queries go to a per-wave LDS table [H][16][2]
//   pass 2  for every key block: for h = 0 .. H - 1 in that order the scores again
//           (AttnScores::scores), p = 2^((s - m_h) c) / l_h (the export's expression on the
//           export's m, l and s, so the same bits) added to an fp32 accumulator that starts at 0;
//           then one product with fl(1 / H), the block through the wave's LDS tile and out by row
//           segments
//
// A [16 x N] accumulator per wave does not fit anywhere for N up to 4096, hence the key block as
// the outer loop of pass 2 and the table; bf16 stages the same number of K blocks (H nkb per pass)
// as a loop with the head outside would, and reloads the q fragments per (block, head) from L2.
// This kernel's own: the table, the head loop inside each key block and the fl(1 / H) product.
// The head sum has one order, nothing is atomic, nothing depends on the batch position, and
// both qkv layouts stage the same values: results are bitwise reproducible and layout independent.
// Every p is in [0, 1], so the sum is in [0, H] and the mean in [0, 1] up to one rounding; keys
// past N get -inf scores, contribute 2^-inf = 0 and are not stored.
//
// Stores: the dword row-segment form that won for the export (store_tile_rows), plain rather than
// non-temporal: the rollout step reads the buffer next. Every row and output offset is 64-bit.
namespace {

template <typename T, int DP>
__global__ __launch_bounds__(256) void head_mean_kernel(AttnParams p, int nqb, float inv_h,
                                                        float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool BF = sizeof(T) == 2;
  AttnScores<T, DP> sc(p, (EVT_LDS char*)smem + 4 * PTILE * 4);  // bf16: one K block, [64][DP]
  const int lane = sc.lane, wave = sc.tid >> 6, g = sc.g, c16 = sc.c16;
  const int H = p.H, N = sc.N, nkb = sc.nkb;
  EVT_LDS float* Ps = (EVT_LDS float*)smem + wave * PTILE;  // this wave's [16 queries][64 keys]
  // this wave's (m, 1 / l) of head h, query c16 at [(h * 16 + c16) * 2]
  EVT_LDS float* St = (EVT_LDS float*)(smem + 4 * PTILE * 4 + (BF ? KB * DP * 2 : 0)) + wave * 32 * H;
  int b, qb;  // workgroups of one image read the same K
  unswizzle_block(blockIdx.x, p.B, nqb, b, qb);
  const int nqt = (N + 15) >> 4;
  const int qt = qb * 4 + wave;
  const bool active = qt < nqt;  // wave-uniform
  if constexpr (!BF) {
    if (!active) return;  // no barrier in the fp32 kernel
  }
  sc.set_image(b);
  sc.set_tile(qt);
  const float c = p.scale_log2;

  // ---- pass 1, head by head; the head before has staged a block, so a barrier ahead of each
  for (int h = 0; h < H; ++h) {
    sc.head(h);
    float m, l;
    sc.template pass1<true>(active, m, l);
    if (active && g == 0) *(EVT_LDS f32x2*)(St + (h * 16 + c16) * 2) = f32x2{m, 1.0f / l};
  }
  wave_lds_written();  // the table is this wave's alone, as its tile

  // ---- pass 2, key block by key block: sum_h p in head order, times fl(1 / H), stored by rows
  const int64_t row0 = ((int64_t)b * N + (int64_t)qt * 16) * N;  // element offset of the tile's row 0
  for (int kb = 0; kb < nkb; ++kb) {
    f32x4 acc[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) acc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int h = 0; h < H; ++h) {
      sc.head(h);
      if (!sc.template stage_block<true>(kb, active)) continue;
      f32x4 s[NKT];
      sc.scores(kb, s);
      const f32x2 ml = *(const EVT_LDS f32x2*)(St + (h * 16 + c16) * 2);
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float pv = ex2<BF>((s[kt][j] - ml[0]) * c) * ml[1];  // the export's value, rounded
          acc[kt][j] += pv;                                          // on its own, then added
        }
    }
    if (!active) continue;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
      *(EVT_LDS f32x4*)(Ps + c16 * PROW + kt * 16 + 4 * g) = acc[kt] * inv_h;
    wave_lds_written();
    const int nk = min(KB, N - kb * KB);  // keys of this block
    store_tile_rows<false>(Ps, out + row0, qt * 16, N, kb * KB, nk, N, lane);
    wave_lds_read();
  }
}

size_t head_mean_lds(int elem, int DP, int H) {
  return score_lds(elem, DP, true) + (size_t)4 * 32 * H * sizeof(float);  // + the (m, 1 / l) tables
}

}  // namespace

hipError_t head_mean_launch(int dtype, const AttnParams& p_in, float* out, hipStream_t s) {
  if (p_in.B <= 0) return hipSuccess;
  AttnParams p;
  if (!prepare(dtype, p_in, out, p)) return hipErrorInvalidValue;
  if (head_mean_lds(2, 128, p.H) > 160 * 1024) return hipErrorInvalidValue;  // H <= 254
  const int nqb = ((p.N + 15) / 16 + 3) / 4;
  if ((int64_t)p.B * nqb > INT32_MAX) return hipErrorInvalidValue;
  return dispatch(dtype, p.hd, [&](auto v) {
    using V = decltype(v);
    using T = typename V::type;
    const size_t lds = head_mean_lds(sizeof(T), V::DP, p.H);
    if (lds > 64 * 1024) {  // many heads: the table takes the LDS past the default limit
      const hipError_t e = hipFuncSetAttribute((const void*)head_mean_kernel<T, V::DP>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((head_mean_kernel<T, V::DP>), dim3(p.B * nqb), dim3(256), lds, s, p, nqb,
                       1.0f / (float)p.H, out);
    return hipGetLastError();
  });
}

// ---- Swin window attention maps (include/evt_window_attention.h) -------------------------------
//
//   out[b][win][h][q][k] = softmax_k(q_q . k_k 32^-0.5 + rpb[rel(q, k)][h] + mask(win, q, k))
//
// of the q and k rows the block's QKV GEMM stored in raster order: what the window kernels of
// swin.hip form in registers, multiply by V and discard. q, k: window-local tokens of the SHIFTED
// frame, row-major inside the window (window_scores.h WinGeom::row); win: row-major over that frame's
// windows; N = w * w tokens per window, head size 32. A pair in different SW-MSA regions gets a
// -inf score, so exactly 0.0f (the reference's additive -100 leaves at most e^-100 of relative
// weight, below fp32 resolution); a query shares a region with itself, so no row is empty and the
// row maximum's own term keeps the sum >= 1: every value is finite and in [0, 1]. Scores,
// statistics and normalisation in fp32: the probability before the bf16 rounding the forward
// applies for P . V.
//
// The bias comes from the head's compact table (rpb_compact_table: entry r = table[r][h] log2 e),
// bias(q, k) = T[(2w - 1)(qi - ki + w - 1) + (qj - kj + w - 1)], copied to LDS; the regions are
// worked out on the VALU (region bit 0: rows >= w - shift of a window of the last window row,
// bit 1: the same for columns). Geometry, constants and key tables are window_scores.h's, the
// definitions the forward kernels of swin.hip use; the score loop, the reductions, the division
// and the stores below are this kernel's own. There is no V, no LDS V tile and no P . V.
//
// bf16 (window_probs_bf16_kernel<w>): the geometry of window_attn_bf16_kernel (w = 7: four waves
// per block, a wave per (image, window, head), four 16-token tiles of which keys 49 .. 63 never
// contribute and are never stored) and of window12_attn_bf16_kernel (w = 12: three waves per
// (image, window, head), three query tiles each, nine K tiles). Q / K fragments are 16-B loads
// straight from the raster qkv rows through the image's buffer descriptor, S^T = K Q^T is one
// v_mfma_f32_16x16x32_bf16 per tile pair. Every wave keeps its own copy of the bias table, so the
// kernel has no block barrier. fp32 (window_probs_f32_kernel<w>): thread = query on the VALU, K
// and the table in LDS, the scores computed twice (maximum, then exp2) as in
// window12_attn_f32_kernel.
//
// Stores. The [N, N] matrix of one (image, window, head) is one contiguous run of the output
// (9604 B for w = 7, 82944 B for w = 12), and the 16 query rows of a tile are a contiguous piece of
// it. The MFMA result has a query per lane column, so each wave passes its tile through a private
// LDS tile and stores the piece as consecutive non-temporal dwords, a lane per float: 256
// contiguous bytes per wave instruction, the form that won for the ViT export (above). A w = 7
// matrix starts 16-byte aligned one time in four and keeps that form; a w = 12 matrix always does
// (and its rows are 576 B), so the bf16 w = 12 kernel also has a 16-B form, a lane per 4 keys, and
// launches it: measured at Swin-B 384 px stage 1 with 64 images (1.36 GB) 400.8 us against 444.2 us
// for the dword form (scripts/window_attention_maps_measure.py). Unlike the ViT rows it
// has no unaligned edges to peel. EVT_WINDOW_MAPS_STORE=dword selects the other form for a
// measurement; both write the same bits. Output offsets are 64-bit.
namespace {

constexpr int wp_prow(int w) { return w == 7 ? 49 : 148; }  // LDS tile row (148: b128 conflict-free)

template <int W, bool WIDE>
__global__ __launch_bounds__(W == 7 ? 256 : 192) void window_probs_bf16_kernel(
    SwinAttnParams p, const float* __restrict__ table, int trow, float* __restrict__ out) {
  using T = WinTraits<W>;
  constexpr int N = T::N, NKT = T::NKT;
  constexpr int PW = W == 7 ? 1 : 3;  // waves per (image, window, head)
  constexpr int PB = W == 7 ? 4 : 1;  // (image, window, head) per block
  constexpr int QTW = NKT / PW;       // query tiles per wave
  constexpr int PROW = wp_prow(W), PT = 16 * PROW, TL = T::CROW;  // TL: LDS floats of a table copy
  static_assert(NKT % PW == 0 && PT % 4 == 0 && (!WIDE || N % 4 == 0), "geometry");
  __shared__ __attribute__((aligned(16))) float smem[PB * PW * (PT + TL)];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: scalar index math
  const int pair = blockIdx.x * PB + wave / PW, pw = wave % PW;  // (pairs < 2^31: the launcher)
  const int nw = p.nwx * p.nwx;
  if (pair >= p.B * nw * p.H) return;  // wave-uniform; the kernel has no block barrier
  const int h = pair % p.H;
  const int bw = pair / p.H;
  const int win = bw % nw, b = bw / nw;
  const int R = p.R;
  const WinGeom<W> G(R, p.nwx, p.shift, win);
  const int ldq2 = (int)p.ldq * 2, C2 = p.C * 2;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      (char*)const_cast<void*>(p.qkv) + (int64_t)b * R * R * ldq2, 0, R * R * ldq2, 0x00020000);
  EVT_LDS float* Ps = (EVT_LDS float*)smem + wave * (PT + TL);  // this wave's [16 queries][PROW]
  EVT_LDS float* Ts = Ps + PT;                                  // and its copy of the head's table
  for (int e = lane; e < T::TW * T::TW; e += 64) Ts[e] = table[(int64_t)h * trow + e];
  // K fragments of every tile, Q fragments of this wave's: tile i, lane (token 16 i + c16,
  // d 8 g .. 8 g + 7); tokens past N - 1 (w = 7) repeat token N - 1 and are masked below
  const int g = lane >> 4, c16 = lane & 15;
  u32x4 kf[NKT], qf[QTW];
#pragma unroll
  for (int i = 0; i < NKT; ++i) {
    const int vo = G.row(T::clamp(16 * i + c16)) * ldq2 + (h * 32 + 8 * g) * 2;
    kf[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, C2, 0));
  }
#pragma unroll
  for (int n = 0; n < QTW; ++n) {
    const int vo = G.row(T::clamp(16 * (pw * QTW + n) + c16)) * ldq2 + (h * 32 + 8 * g) * 2;
    qf[n] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, 0, 0));
  }
  // per-lane table offsets of its keys k = 16 kt + 4 g + j and their region codes, a byte per j
  int kofs[NKT][4];
  unsigned kc[NKT];
  key_tables<W>(G, g, kofs, kc);
  // the table copy is this wave's alone: LDS operations of a wave complete in order
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  const int64_t obase = (int64_t)pair * N * N;  // element offset of the (image, window, head)
#pragma unroll
  for (int n = 0; n < QTW; ++n) {
    const int qt = pw * QTW + n;
    const int q = T::clamp(16 * qt + c16), qi = T::div(q);
    const EVT_LDS float* Tq = Ts + T::a(qi, q);
    const unsigned cq = G.code(qi, q - W * qi) * 0x01010101u;
    // s[kt][j] = S^T[key 16 kt + 4 g + j][query q], in the log2 domain, + bias, then the masks.
    // Not window_scores.h's score_tile: with it this kernel measured 7 to 9 % slower at w = 7
    // (profiles/window_core_speed.json), so the step keeps the form it was tuned in
    f32x4 s[NKT];
    const float NEG = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      const f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kf[kt]),
                                                      __builtin_bit_cast(bf16x8, qf[n]), acc, 0, 0,
                                                      0);
      const unsigned x = kc[kt] ^ cq;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[kt][j] = s[kt][j] * p.scale_log2 + Tq[-kofs[kt][j]];
        if ((x >> (8 * j)) & 3u) s[kt][j] = NEG;            // a key of another region
        if (N % 16 != 0 && 16 * kt + 4 * g + j >= N) s[kt][j] = NEG;  // w = 7: keys 49 .. 63
      }
    }
    float mx = NEG;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
      mx = fmaxf(mx, fmaxf(fmaxf(s[kt][0], s[kt][1]), fmaxf(s[kt][2], s[kt][3])));
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
      for (int j = 0; j < 4; ++j) s[kt][j] = __builtin_amdgcn_exp2f(s[kt][j] - mx);
      sum += (s[kt][0] + s[kt][1]) + (s[kt][2] + s[kt][3]);
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      const f32x4 pv = s[kt] * inv;
      if constexpr (PROW % 4 == 0) {
        *(EVT_LDS f32x4*)(Ps + c16 * PROW + 16 * kt + 4 * g) = pv;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (16 * kt + 4 * g + j < N) Ps[c16 * PROW + 16 * kt + 4 * g + j] = pv[j];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // rows 16 qt .. of the matrix: one contiguous piece of nr * N floats
    const int nr = min(16, N - 16 * qt);
    float* dst = out + obase + (int64_t)16 * qt * N;
    if constexpr (!WIDE) {
      for (int e = lane; e < nr * N; e += 64) {
        const int r = e / N, k = e - r * N;
        store1_nt(dst + e, Ps[r * PROW + k]);
      }
    } else {
      for (int e = lane; e < nr * (N / 4); e += 64) {
        const int r = e / (N / 4), k = 4 * (e - r * (N / 4));
        store4_nt(dst + r * N + k, *(const EVT_LDS f32x4*)(Ps + r * PROW + k));
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// fp32 (parity path): block = one (image, window, head), thread = query (49 of 64, 144 of 192)
template <int W>
__global__ __launch_bounds__(W == 7 ? 64 : 192) void window_probs_f32_kernel(
    SwinAttnParams p, const float* __restrict__ table, int trow, float* __restrict__ out) {
  using T = WinTraits<W>;
  constexpr int N = T::N, NT = W == 7 ? 64 : 192, TW = T::TW;
  constexpr int PR = N % 2 ? N : N + 1;  // row stride of the P tile: odd, so conflict-free
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Ks = (float*)smem;  // [N][33]
  float* Ts = Ks + N * 33;   // [TW * TW]
  float* Ps = Ts + TW * TW;  // [N][PR]
  const int tid = threadIdx.x;
  const int64_t pair = blockIdx.x;
  const int nw = p.nwx * p.nwx;
  const int h = (int)(pair % p.H);
  const int64_t bw = pair / p.H;
  const int win = (int)(bw % nw), b = (int)(bw / nw);
  const WinGeom<W> G(p.R, p.nwx, p.shift, win);
  const int64_t base = (int64_t)b * p.R * p.R;
  const float* qkv = (const float*)p.qkv;
  for (int e = tid; e < N * 32; e += NT) {
    const int t = e >> 5, d = e & 31;
    Ks[t * 33 + d] = qkv[(base + G.row(t)) * p.ldq + p.C + h * 32 + d];
  }
  for (int e = tid; e < TW * TW; e += NT) Ts[e] = table[(int64_t)h * trow + e];
  __syncthreads();
  if (tid < N) {
    const int t = tid, qi = t / W, qj = t - W * qi;
    const int64_t qrow = base + G.row(t);
    float q[32];
#pragma unroll
    for (int d = 0; d < 32; ++d) q[d] = qkv[qrow * p.ldq + h * 32 + d];
    const unsigned cq = G.code(qi, qj);
    const float* Tq = Ts + T::a(qi, t);
    auto score = [&](int k, int ki, int kj) {
      float a = 0.f;
#pragma unroll
      for (int d = 0; d < 32; ++d) a += q[d] * Ks[k * 33 + d];
      return G.code(ki, kj) != cq ? -INFINITY : a * p.scale_log2 + Tq[-T::b(ki, k)];
    };
    float mx = -INFINITY;
#pragma unroll 1
    for (int ki = 0, k = 0; ki < W; ++ki)
      for (int kj = 0; kj < W; ++kj, ++k) mx = fmaxf(mx, score(k, ki, kj));
    float sum = 0.f;
#pragma unroll 1
    for (int ki = 0, k = 0; ki < W; ++ki)
      for (int kj = 0; kj < W; ++kj, ++k) {
        const float e = exp2f(score(k, ki, kj) - mx);
        Ps[t * PR + k] = e;
        sum += e;
      }
    const float inv = 1.0f / sum;
    for (int k = 0; k < N; ++k) Ps[t * PR + k] *= inv;  // the thread's own row
  }
  __syncthreads();
  float* dst = out + pair * N * N;
  for (int e = tid; e < N * N; e += NT) {
    const int r = e / N, k = e - r * N;
    store1_nt(dst + e, Ps[r * PR + k]);
  }
}

template <int W>
constexpr size_t wp_f32_lds() {
  constexpr int N = WinTraits<W>::N, TW = WinTraits<W>::TW;
  return (size_t)(N * 33 + TW * TW + N * (N % 2 ? N : N + 1)) * sizeof(float);
}

// the store form of the bf16 w = 12 kernel: 16-B unless EVT_WINDOW_MAPS_STORE=dword asks for the
// other one (for the measurement)
bool window_wide_stores() {
  const char* e = std::getenv("EVT_WINDOW_MAPS_STORE");
  return !(e && std::strcmp(e, "dword") == 0);
}

}  // namespace

hipError_t window_probs_launch(int dtype, int w, const SwinAttnParams& p, float* out,
                               hipStream_t s) {
  if (p.B <= 0) return hipSuccess;
  if ((w != 7 && w != 12) || !p.qkv || !p.bias || !out || ((uintptr_t)out & 15) || p.R <= 0 ||
      p.R % w || p.nwx * w != p.R || p.H <= 0 || p.C != p.H * 32 || p.ldq < 3 * (int64_t)p.C ||
      p.shift < 0 || p.shift >= w || (p.shift && p.R == w))
    return hipErrorInvalidValue;
  // the -inf masks and 2^(s - m) <= 1 need a positive finite scale
  if (!(p.scale_log2 > 0.f && p.scale_log2 < INFINITY)) return hipErrorInvalidValue;
  const int64_t pairs = (int64_t)p.B * p.nwx * p.nwx * p.H;
  if (pairs + 4 >= (int64_t)1 << 31) return hipErrorInvalidValue;
  int trow = 0;
  const float* table = rpb_compact_table(p.bias, p.H, w, p.shift, &trow);
  if (dtype == DT_BF16) {
    // 16-B fragment loads and per-image 32-bit buffer offsets
    if (p.ldq % 8 || ((uintptr_t)p.qkv & 15) || (int64_t)p.R * p.R * p.ldq * 2 >= (int64_t)1 << 31)
      return hipErrorInvalidValue;
    if (w == 7)
      hipLaunchKernelGGL((window_probs_bf16_kernel<7, false>), dim3((unsigned)((pairs + 3) / 4)),
                         dim3(256), 0, s, p, table, trow, out);
    else if (window_wide_stores())
      hipLaunchKernelGGL((window_probs_bf16_kernel<12, true>), dim3((unsigned)pairs), dim3(192), 0,
                         s, p, table, trow, out);
    else
      hipLaunchKernelGGL((window_probs_bf16_kernel<12, false>), dim3((unsigned)pairs), dim3(192), 0,
                         s, p, table, trow, out);
    return hipGetLastError();
  }
  if (dtype != DT_F32) return hipErrorInvalidValue;
  if (w == 7) {
    hipLaunchKernelGGL(window_probs_f32_kernel<7>, dim3((unsigned)pairs), dim3(64), wp_f32_lds<7>(),
                       s, p, table, trow, out);
  } else {
    (void)hipFuncSetAttribute((const void*)window_probs_f32_kernel<12>,  // 104644 B of LDS
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)wp_f32_lds<12>());
    hipLaunchKernelGGL(window_probs_f32_kernel<12>, dim3((unsigned)pairs), dim3(192),
                       wp_f32_lds<12>(), s, p, table, trow, out);
  }
  return hipGetLastError();
}

}  // namespace evt
