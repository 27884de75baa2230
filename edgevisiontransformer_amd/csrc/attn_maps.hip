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

#include "common.h"
#include "evt_internal.h"

namespace evt {

namespace {

constexpr int KB = 64;         // keys per block
constexpr int NKT = KB / 16;   // 16-key MFMA tiles per block
constexpr int PROW = KB + 4;   // floats per row of a wave's P tile (rows 4 banks apart)
constexpr int PTILE = 16 * PROW;

// swizzle mask of the staged K rows (DP * 2 bytes each), as attention.hip gen_swm
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

template <bool FAST>
__device__ __forceinline__ float ex2(float x) {
  return FAST ? __builtin_amdgcn_exp2f(x) : exp2f(x);
}

// T: bf16 (DP = h_k padded to 32 / 64 / 96 / 128) or float (DP = 64 / 128: feature groups of 64).
// nqb: 64-query groups per (image, head). Workgroups of one (image, head) read the same K: the
// block index is unswizzled as in attn_long_bf16_kernel so that they run on one XCD (speed only).
template <typename T, int DP, bool WIDE>
__global__ __launch_bounds__(256) void attn_probs_kernel(AttnParams p, int nq, int nqb,
                                                         float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool BF = sizeof(T) == 2;
  constexpr int RB = DP * 2, NCH = DP / 8, SWM = k_swm<DP>(), KS = DP / 32, NG = DP / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c16 = lane & 15;
  EVT_LDS float* Ps = (EVT_LDS float*)smem + wave * PTILE;  // this wave's [16 queries][64 keys]
  EVT_LDS char* Ks = (EVT_LDS char*)smem + 4 * PTILE * 4;   // bf16: one K block, [64][DP]
  int bh, qb;
  {
    const int BH = p.B * p.H, full = (BH >> 3) * 8 * nqb, L = blockIdx.x;
    if (L < full) {
      bh = (L & 7) + 8 * (L / (8 * nqb));
      qb = (L >> 3) % nqb;
    } else {
      bh = (BH & ~7) + (L - full) / nqb;
      qb = (L - full) % nqb;
    }
  }
  const int b = bh / p.H, h = bh - b * p.H, hd = p.hd, N = p.N;
  const T* slice = (const T*)p.qkv + b * p.sb + h * p.sh;  // q of the (image, head); k at + ko
  const int nqt = (nq + 15) >> 4, nkb = (N + KB - 1) / KB;
  const int qt = qb * 4 + wave;
  const bool active = qt < nqt;  // wave-uniform
  if constexpr (!BF) {
    if (!active) return;  // no barrier in the fp32 kernel
  }
  const T* qrow = slice + (int64_t)min(qt * 16 + c16, N - 1) * p.ldq;
  const float c = p.scale_log2;

  u32x4 qf[BF ? KS : 1];
  if constexpr (BF) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = chunk8((const bf16*)qrow, 32 * ks + 8 * g, hd);
  }
  // bf16: key block kb of K into LDS, 16-B chunk ch of row r at chunk ch ^ (r & SWM)
  auto stage = [&](int kb) {
    for (int i = tid; i < KB * NCH; i += 256) {
      const int row = i / NCH, ch = i - row * NCH;
      const bf16* rp = (const bf16*)slice + (int64_t)min(kb * KB + row, N - 1) * p.ldq + p.ko;
      *(EVT_LDS u32x4*)(Ks + row * RB + ((ch ^ (row & SWM)) << 4)) = chunk8(rp, ch * 8, hd);
    }
  };
  // s[kt][j] = S^T[key = kb*64 + kt*16 + 4g + j][query = qt*16 + c16], -inf for keys past N
  auto scores = [&](int kb, f32x4(&s)[NKT]) {
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
  };

  // ---- pass 1: m = max_j s, l = sum_j 2^((s - m) c). Every block holds a valid key, so its
  // maximum is finite; on the first block m = -inf and 2^(-inf) = 0 drops the empty sum.
  float m = -INFINITY, l = 0.f;
  for (int kb = 0; kb < nkb; ++kb) {
    if constexpr (BF) {
      if (kb) __syncthreads();  // every wave is done with the previous block
      stage(kb);
      __syncthreads();
      if (!active) continue;
    }
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
    l = l * ex2<BF>((m - mn) * c) + sum;  // the lane's partial sum; the four lanes of a query
    m = mn;                               // hold the same m
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const float inv = 1.0f / l;

  // ---- pass 2: p = 2^((s - m) c) / l, through the wave's LDS tile, stored by rows
  const int64_t row0 = ((int64_t)bh * nq + (int64_t)qt * 16) * N;  // element offset of the tile's row 0
  for (int kb = 0; kb < nkb; ++kb) {
    if constexpr (BF) {
      __syncthreads();
      stage(kb);
      __syncthreads();
      if (!active) continue;
    }
    f32x4 s[NKT];
    scores(kb, s);
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      f32x4 pv;
#pragma unroll
      for (int j = 0; j < 4; ++j) pv[j] = ex2<BF>((s[kt][j] - m) * c) * inv;
      *(EVT_LDS f32x4*)(Ps + c16 * PROW + kt * 16 + 4 * g) = pv;
    }
    // the tile is this wave's alone: LDS operations of a wave complete in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int nk = min(KB, N - kb * KB);  // keys of this block
    if constexpr (!WIDE) {
      for (int r = 0; r < 16 && qt * 16 + r < nq; ++r) {
        const float v = Ps[r * PROW + lane];
        if (lane < nk) store1_nt(out + row0 + (int64_t)r * N + kb * KB + lane, v);
      }
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
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

template <typename T, int DP>
hipError_t launch_probs(const AttnParams& p, int nq, int nqb, bool wide, float* out, hipStream_t s) {
  const size_t lds = 4 * PTILE * 4 + (sizeof(T) == 2 ? (size_t)KB * DP * 2 : 0);
  const dim3 grid(p.B * p.H * nqb), block(256);
  if (wide)
    hipLaunchKernelGGL((attn_probs_kernel<T, DP, true>), grid, block, lds, s, p, nq, nqb, out);
  else
    hipLaunchKernelGGL((attn_probs_kernel<T, DP, false>), grid, block, lds, s, p, nq, nqb, out);
  return hipGetLastError();
}

// the store form (file header): dword unless EVT_ATTN_MAPS_STORE=wide asks for the other one
bool wide_stores() {
  const char* e = std::getenv("EVT_ATTN_MAPS_STORE");
  return e && std::strcmp(e, "wide") == 0;
}

}  // namespace

hipError_t attn_probs_launch(int dtype, const AttnParams& p_in, int nq, float* out, hipStream_t s) {
  if (p_in.B <= 0) return hipSuccess;
  if (!p_in.qkv || !out || p_in.N <= 0 || p_in.N > EVT_ATTN_MAX_TOKENS || p_in.H <= 0 ||
      p_in.hd <= 0 || p_in.hd > 128 || (nq != 1 && nq != p_in.N) || ((uintptr_t)out & 15))
    return hipErrorInvalidValue;
  // (s - m) c <= 0 and the -inf masks need c > 0
  if (!(p_in.scale_log2 > 0.f && p_in.scale_log2 < INFINITY)) return hipErrorInvalidValue;
  AttnParams p = p_in;
  if (p.sb || p.sh || p.ko) {  // an explicit slice layout: bf16, h_k = 64, 16-B aligned pieces
    if (dtype != DT_BF16 || p.hd != 64 || p.sb % 8 || p.sh % 8 || p.ldq % 8 || p.ko % 8 ||
        p.ldq < 64 || p.ko < 0 || p.sb < 0 || p.sh < 0)
      return hipErrorInvalidValue;
  } else {
    p.sb = (int64_t)p.N * p.ldq;
    p.sh = p.hd;
    p.ko = p.H * p.hd;
  }
  const int nqb = ((nq + 15) / 16 + 3) / 4;
  if ((int64_t)p.B * p.H * nqb > INT32_MAX) return hipErrorInvalidValue;
  const bool wide = wide_stores();
  if (dtype == DT_BF16) {
    if (p.hd <= 32) return launch_probs<bf16, 32>(p, nq, nqb, wide, out, s);
    if (p.hd <= 64) return launch_probs<bf16, 64>(p, nq, nqb, wide, out, s);
    if (p.hd <= 96) return launch_probs<bf16, 96>(p, nq, nqb, wide, out, s);
    return launch_probs<bf16, 128>(p, nq, nqb, wide, out, s);
  }
  if (dtype != DT_F32) return hipErrorInvalidValue;
  if (p.hd <= 64) return launch_probs<float, 64>(p, nq, nqb, wide, out, s);
  return launch_probs<float, 128>(p, nq, nqb, wide, out, s);
}

}  // namespace evt
