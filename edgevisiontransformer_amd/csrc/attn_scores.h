// The score core of the ViT attention-map kernels (attn_maps.hip: attn_probs_kernel,
// head_stats_kernel, head_mean_kernel; token_pruning.hip: token_scores_kernel), defined once so
// that they form the same scores and
// the same softmax statistics (m, l), bit for bit, by construction:
//
//   S^T = K Q^T on the MFMA (one query per lane column, four consecutive keys per lane) over
//   64-key blocks; bf16 with every head size zero-padded to DP = 32 / 64 / 96 / 128 and each block
//   of K staged to swizzled LDS through registers, fp32 exact with every operand straight from the
//   qkv rows (DP = 64 / 128: feature groups of 64); rows past N clamped, keys past N at -inf, row
//   offsets 64-bit; pass 1 of the two-pass softmax, the running max m and sum l of 2^((s - m) c).
//
// Also here: the helpers attention.hip's any-head-size kernels share with it (k_swm, chunk8,
// chunk4), the XCD unswizzle of a (group, 64-query block) grid and the row-segment store of a
// wave's P tile; and what the kernels' launchers share (prepare, dispatch, score_lds).
//
// The file is compiled with -ffp-contract=on: a floating-point expression contracts only within
// itself, so every expression below keeps its boundaries (l = l * ex2(..) + sum is one).
#pragma once
#include <cmath>

#include "common.h"
#include "evt_internal.h"

namespace evt {

// swizzle mask of staged K / V rows of DP * 2 bytes: 16-B chunk c of row r at chunk c ^ (r & mask)
template <int DP>
constexpr int k_swm() {
  constexpr int nch = DP / 8;
  return nch == 4 ? 3 : ((nch >= 8 && (nch & (nch - 1)) == 0) ? 7 : 0);
}

// 8 consecutive head features [d0, d0 + 8) of a bf16 row, zero past h_k
__device__ __forceinline__ u32x4 chunk8(const bf16* row, int d0, int hd) {
  if ((hd & 7) == 0) {
    if (d0 < hd) return *(const u32x4*)(row + d0);
    return u32x4{0u, 0u, 0u, 0u};
  }
  bf16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = d0 + e < hd ? row[d0 + e] : (bf16)0.f;
  return __builtin_bit_cast(u32x4, v);
}

// 4 consecutive head features of an fp32 row, zero past h_k
__device__ __forceinline__ f32x4 chunk4(const float* row, int d0, int hd) {
  if ((hd & 3) == 0) return d0 < hd ? *(const f32x4*)(row + d0) : f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = d0 + e < hd ? row[d0 + e] : 0.f;
  return v;
}

// What follows is the map kernels' alone (attn_maps.hip), under names short enough to clash
// elsewhere: a namespace of its own.
namespace scores {

constexpr int KB = 64;         // keys per block
constexpr int NKT = KB / 16;   // 16-key MFMA tiles per block
constexpr int PROW = KB + 4;   // floats per row of a wave's P tile (rows 4 banks apart)
constexpr int PTILE = 16 * PROW;

template <bool FAST>
__device__ __forceinline__ float ex2(float x) {
  return FAST ? __builtin_amdgcn_exp2f(x) : exp2f(x);
}

// Workgroup L of a (G groups) x (nqb 64-query blocks) grid -> (group, block). Workgroups of one
// group read the same K: the index is unswizzled as in attn_long_bf16_kernel so that they run on
// one XCD (speed only).
__device__ __forceinline__ void unswizzle_block(int L, int G, int nqb, int& grp, int& qb) {
  const int full = (G >> 3) * 8 * nqb;
  if (L < full) {
    grp = (L & 7) + 8 * (L / (8 * nqb));
    qb = (L >> 3) % nqb;
  } else {
    grp = (G & ~7) + (L - full) / nqb;
    qb = (L - full) % nqb;
  }
}

// A wave's P tile (queries q0 .. q0 + 15, the nk keys from k0 on) to the rows of dst (row 0 is
// query q0's, rows N floats apart), the queries below nq only: a lane per key, 64 consecutive
// floats (256 B) of one row per instruction. NT: non-temporal stores.
template <bool NT>
__device__ __forceinline__ void store_tile_rows(const EVT_LDS float* Ps, float* dst, int q0, int nq,
                                                int k0, int nk, int N, int lane) {
  for (int r = 0; r < 16 && q0 + r < nq; ++r) {
    const float v = Ps[r * PROW + lane];
    if (lane < nk) {
      if constexpr (NT)
        store1_nt(dst + (int64_t)r * N + k0 + lane, v);
      else
        dst[(int64_t)r * N + k0 + lane] = v;
    }
  }
}

// One wave's view of the scores of a 16-query tile against the keys of an (image, head).
// T: bf16 or float. Ks: the workgroup's LDS K block, [64][DP] bf16 (unused for fp32).
// fp32 has no block barrier: a wave without a query tile leaves before any of this. bf16 waves
// without one keep staging and taking the barriers (stage_block tells them to skip the rest).
template <typename T, int DP>
struct AttnScores {
  static constexpr bool BF = sizeof(T) == 2;
  static constexpr int RB = DP * 2, NCH = DP / 8, SWM = k_swm<DP>(), KS = DP / 32, NG = DP / 64;
  const AttnParams& p;
  EVT_LDS char* const Ks;
  const int tid, lane, g, c16;
  const int hd, N, nkb;  // head size, tokens, key blocks
  const T* image;  // head 0's q of the image
  int64_t qoff;    // this lane's query row (query c16 of the tile) inside a head's slice
  const T* slice;  // q of the (image, head); k at + ko
  const T* qrow;   // slice + qoff
  u32x4 qf[BF ? KS : 1];

  __device__ __forceinline__ AttnScores(const AttnParams& p_, EVT_LDS char* Ks_)
      : p(p_), Ks(Ks_), tid(threadIdx.x), lane(tid & 63), g(lane >> 4), c16(lane & 15),
        hd(p_.hd), N(p_.N), nkb((p_.N + KB - 1) / KB), image(nullptr), qoff(0), slice(nullptr),
        qrow(nullptr) {}

  // The image and the query tile stay while a kernel walks the heads (head_mean_kernel): only
  // head() is per head.
  __device__ __forceinline__ void set_image(int b) { image = (const T*)p.qkv + b * p.sb; }
  __device__ __forceinline__ void set_tile(int qt) {
    qoff = (int64_t)min(qt * 16 + c16, N - 1) * p.ldq;
  }
  // head h's slice, this lane's q row of it and, for bf16, its q fragments
  __device__ __forceinline__ void head(int h) {
    slice = image + h * p.sh;
    qrow = slice + qoff;
    if constexpr (BF) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) qf[ks] = chunk8((const bf16*)qrow, 32 * ks + 8 * g, hd);
    }
  }
  // bf16: key block kb of K into LDS, 16-B chunk ch of row r at chunk ch ^ (r & SWM)
  __device__ __forceinline__ void stage(int kb) {
    for (int i = tid; i < KB * NCH; i += 256) {
      const int row = i / NCH, ch = i - row * NCH;
      const bf16* rp = (const bf16*)slice + (int64_t)min(kb * KB + row, N - 1) * p.ldq + p.ko;
      *(EVT_LDS u32x4*)(Ks + row * RB + ((ch ^ (row & SWM)) << 4)) = chunk8(rp, ch * 8, hd);
    }
  }
  // bf16: stage(kb) between the barrier that ends every wave's use of the block staged before
  // (SYNC_FIRST = false: not ahead of block 0, for a kernel that has staged nothing yet) and the
  // one that publishes it. False for a wave that has no query tile.
  template <bool SYNC_FIRST>
  __device__ __forceinline__ bool stage_block(int kb, bool active) {
    if constexpr (BF) {
      if (SYNC_FIRST || kb) __syncthreads();
      stage(kb);
      __syncthreads();
      return active;
    }
    return true;
  }
  // s[kt][j] = S^T[key = kb*64 + kt*16 + 4g + j][query = qt*16 + c16], -inf for keys past N
  __device__ __forceinline__ void scores(int kb, f32x4 (&s)[NKT]) const {
    if constexpr (BF) {
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        const int row = kt * 16 + c16;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const u32x4 kf = *(const EVT_LDS u32x4*)(Ks + row * RB + (((4 * ks + g) ^ (row & SWM)) << 4));
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kf),
                                                        __builtin_bit_cast(bf16x8, qf[ks]), acc, 0, 0, 0);
        }
        s[kt] = acc;
      }
    } else {
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int kk = 0; kk < 4 * NG; ++kk) {
        const int d0 = 16 * kk + 4 * g;
        const f32x4 qv = chunk4((const float*)qrow, d0, hd);
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
          const float* krow =
              (const float*)slice + (int64_t)min(kb * KB + kt * 16 + c16, N - 1) * p.ldq + p.ko;
          const f32x4 kv = chunk4(krow, d0, hd);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            s[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[e], qv[e], s[kt], 0, 0, 0);
        }
      }
    }
    if ((kb + 1) * KB > N) {  // wave-uniform: only the last block holds keys past N
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (kb * KB + kt * 16 + 4 * g + j >= N) s[kt][j] = -INFINITY;
    }
  }
  // Pass 1 over every key block: m = max_j s, l = sum_j 2^((s - m) c) of this lane's query (the
  // four lanes of a query end with the same m and l). Every block holds a valid key, so its
  // maximum is finite; on the first block m = -inf and 2^(-inf) = 0 drops the empty sum.
  // SYNC_FIRST: as stage_block.
  template <bool SYNC_FIRST>
  __device__ __forceinline__ void pass1(bool active, float& m_out, float& l_out) {
    const float c = p.scale_log2;
    float m = -INFINITY, l = 0.f;
    for (int kb = 0; kb < nkb; ++kb) {
      if (!stage_block<SYNC_FIRST>(kb, active)) continue;
      f32x4 s[NKT];
      scores(kb, s);
      float bm = s[0][0];
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) bm = fmaxf(bm, s[kt][j]);
      bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
      bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
      const float mn = fmaxf(m, bm);
      float sum = 0.f;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) sum += ex2<BF>((s[kt][j] - mn) * c);
      l = l * ex2<BF>((m - mn) * c) + sum;  // the lane's partial sum
      m = mn;
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    m_out = m;
    l_out = l;
  }
};

// ---- the launchers' side (attn_maps.hip, token_pruning.hip) ----

// What the launchers of these kernels ask of their parameters alike; fills the default slice
// layout. c > 0: (s - m) c <= 0 and the -inf masks need it. align: bytes `out` is aligned to.
inline bool prepare(int dtype, const AttnParams& p_in, const float* out, AttnParams& p,
                    int align = 16) {
  if (!p_in.qkv || !out || p_in.N <= 0 || p_in.N > EVT_ATTN_MAX_TOKENS || p_in.H <= 0 ||
      p_in.hd <= 0 || p_in.hd > 128 || ((uintptr_t)out & (uintptr_t)(align - 1)) ||
      (dtype != DT_BF16 && dtype != DT_F32))
    return false;
  if (!(p_in.scale_log2 > 0.f && p_in.scale_log2 < INFINITY)) return false;
  p = p_in;
  if (p.sb || p.sh || p.ko) {  // an explicit slice layout: bf16, h_k = 64, 16-B aligned pieces
    if (dtype != DT_BF16 || p.hd != 64 || p.sb % 8 || p.sh % 8 || p.ldq % 8 || p.ko % 8 ||
        p.ldq < 64 || p.ko < 0 || p.sb < 0 || p.sh < 0)
      return false;
  } else {
    p.sb = (int64_t)p.N * p.ldq;
    p.sh = p.hd;
    p.ko = p.H * p.hd;
  }
  return true;
}

template <typename T, int DP_>
struct Variant {
  using type = T;
  static constexpr int DP = DP_;
};

// f(Variant<T, DP>) of the instantiation for a (prepared) dtype and head size
template <typename F>
hipError_t dispatch(int dtype, int hd, F&& f) {
  if (dtype == DT_BF16) {
    if (hd <= 32) return f(Variant<bf16, 32>{});
    if (hd <= 64) return f(Variant<bf16, 64>{});
    if (hd <= 96) return f(Variant<bf16, 96>{});
    return f(Variant<bf16, 128>{});
  }
  if (hd <= 64) return f(Variant<float, 64>{});
  return f(Variant<float, 128>{});
}

// LDS bytes of the waves' four P tiles (a kernel that stores rows) and, for bf16, one K block
constexpr size_t score_lds(size_t elem, int DP, bool tiles) {
  return (tiles ? 4 * PTILE * 4 : 0) + (elem == 2 ? (size_t)KB * DP * 2 : 0);
}

}  // namespace scores
}  // namespace evt
