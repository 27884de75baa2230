// Token pruning (include/evt_token_pruning.h): the three launches that follow a scheduled encoder
// block's FC2 (encoder.cpp token_prune) and the op-level entry points of the parity tests.
//
//   scores  score[b][j] = sum_h p[b][h][0][j], the CLS row of the probabilities attn_probs_kernel
//           (attn_maps.hip) exports, heads added in index order in fp32, not divided
//   select  kept[b] = (0, the K patch tokens j >= 1 with the largest score, ascending)
//   gather  rows kept[b][:] of the stream, and their LayerNorm statistics slots, packed
//
// SCORES. A workgroup (4 waves) takes (image, 64-key block kb). Wave 0 owns query tile 0, whose
// column 0 is the CLS query; for bf16 the other waves only help stage K (AttnScores, the map
// kernels' geometry), for fp32 they leave. For h = 0 .. H - 1 in that order: AttnScores::pass1 over
// every key block, the export's (m, l) from the export's code; then block kb's scores again
// (AttnScores::scores) and p = 2^((s - m) c) * (1 / l), the export's expression on the export's m, l
// and s, so the same bits, added to an fp32 accumulator that starts at 0. There is no second
// softmax here: the statistics are attn_scores.h's. Pass 1 is repeated by each of an image's
// ceil(N / 64) workgroups; that buys ceil(N / 64) times the workgroups of a launch that is latency
// bound at ordinary batches (B H N 64 bf16 of K per pass). MFMA columns are independent, so column
// 0 of the tile is bitwise the CLS row of the export (which computes the same tile). The four
// lanes of column 0 (c16 == 0, g = 0 .. 3) hold 16 keys each and store them as dwords: a row of N
// floats is 16-byte aligned one time in four, and a workgroup writes 256 bytes.
//
// SELECT. One workgroup per image, N <= 4096, any K. The order is that of
// np.argsort(-s, kind="stable") over the patch tokens: larger score first, ties (and -0.0 against
// +0.0) to the lower index, NaN last. Each score becomes a 32-bit key whose unsigned order is that
// order (NaN -> 0, +-0 -> the key of +0, else the usual sign flip), in LDS; thread j counts the
// patch tokens that come before token j (rank counting: N / 4 broadcast 16-B LDS reads per token),
// and token j is kept iff rank < K: exactly K tokens, since the ranks are a permutation. The
// output is ascending: a token's position is the number of kept tokens below it, from a ballot
// per wave (the lanes below), the 64 per-(256-token slot, wave) totals scanned by wave 0 with
// shuffles. Nothing is atomic: one result whatever the timing.
//
// GATHER. A thread per 16-byte chunk of a destination row or of its statistics slots: D elements
// (D % 8 == 0, so whole chunks for bf16 and fp32 and any D, a multiple of 64 or not) and `slots`
// (sum, sumsq) pairs (slots is even: 16-byte chunks too). Source and destination are different
// buffers: image b's destination rows overlap image b - 1's source rows, so in place would race.
// An index of kept outside [0, T) is clamped: the kernel cannot read outside its image's rows.
#include <cstdint>

#include "attn_scores.h"
#include "common.h"
#include "evt_internal.h"

namespace evt {

namespace {

using namespace scores;  // attn_scores.h

template <typename T, int DP>
__global__ __launch_bounds__(256) void token_scores_kernel(AttnParams p, int nkb,
                                                           float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool BF = sizeof(T) == 2;
  AttnScores<T, DP> sc(p, (EVT_LDS char*)smem);  // bf16: one K block, [64][DP]
  const int wave = sc.tid >> 6, g = sc.g, c16 = sc.c16, N = sc.N;
  const int b = blockIdx.x / nkb, kb = blockIdx.x - b * nkb;
  const bool active = wave == 0;  // wave-uniform: query tile 0 is wave 0's
  if constexpr (!BF) {
    if (!active) return;  // no barrier in the fp32 kernel
  }
  sc.set_image(b);
  sc.set_tile(0);
  const float c = p.scale_log2;
  f32x4 acc[NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) acc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int h = 0; h < p.H; ++h) {
    sc.head(h);
    // the head before has staged a block, so a barrier ahead of each
    float m, l;
    sc.template pass1<true>(active, m, l);
    const float inv = 1.0f / l;
    if (!sc.template stage_block<true>(kb, active)) continue;
    f32x4 s[NKT];
    sc.scores(kb, s);
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float pv = ex2<BF>((s[kt][j] - m) * c) * inv;  // the export's value, rounded on its
        acc[kt][j] += pv;                                    // own, then added
      }
  }
  if (!active || c16 != 0) return;
  float* row = out + (int64_t)b * N;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = kb * KB + kt * 16 + 4 * g + j;
      if (key < N) row[key] = acc[kt][j];
    }
}

constexpr int SEL_MAX = 4096;  // tokens per image (EVT_ATTN_MAX_TOKENS)
static_assert(SEL_MAX == EVT_ATTN_MAX_TOKENS && SEL_MAX == 16 * 256, "64 (slot, wave) totals");

// unsigned key whose descending order is the selection's: NaN lowest, -0.0 == +0.0
__device__ __forceinline__ uint32_t order_key(float v) {
  uint32_t u = __builtin_bit_cast(uint32_t, v);
  const uint32_t mag = u & 0x7fffffffu;
  if (mag > 0x7f800000u) return 0u;  // NaN: below -inf's key 0x007fffff
  if (mag == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void token_select_kernel(const float* __restrict__ scores, int N,
                                                           int K, int* __restrict__ kept) {
  __shared__ __attribute__((aligned(16))) uint32_t key[SEL_MAX];
  __shared__ uint16_t rank[SEL_MAX];
  __shared__ int wtot[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* s = scores + (int64_t)blockIdx.x * N;
  int* out = kept + (int64_t)blockIdx.x * (K + 1);
  const int n4 = (N + 3) >> 2, nslot = (N + 255) >> 8;
  // token 0 (the CLS token) and the padding past N get key 0 and the highest / lowest indices'
  // tie rule; what token 0 adds to a NaN token's count is taken off below
  for (int i = tid; i < 4 * n4; i += 256) key[i] = (i >= 1 && i < N) ? order_key(s[i]) : 0u;
  if (tid < 64) wtot[tid] = 0;
  __syncthreads();
  for (int sl = 0; sl < nslot; ++sl) {
    const int j = sl * 256 + tid;
    const bool patch = j >= 1 && j < N;
    const uint32_t kj = patch ? key[j] : 0u;
    int cnt = kj == 0u ? -1 : 0;  // token 0: key 0 and a lower index than every patch token
    for (int i4 = 0; i4 < n4; ++i4) {
      const u32x4 kv = *(const EVT_LDS u32x4*)((const EVT_LDS uint32_t*)key + 4 * i4);  // broadcast
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = 4 * i4 + e;
        cnt += (kv[e] > kj || (kv[e] == kj && i < j)) ? 1 : 0;
      }
    }
    const bool keep = patch && cnt < K;
    if (patch) rank[j] = (uint16_t)min(cnt, 65535);
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wtot[sl * 4 + wave] = __popcll(mask);
  }
  __syncthreads();
  if (wave == 0) {  // exclusive scan of the 64 totals, in token order
    const int own = wtot[lane];
    int v = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(v, o, 64);
      if (lane >= o) v += t;
    }
    wtot[lane] = v - own;
  }
  __syncthreads();
  if (tid == 0) out[0] = 0;
  for (int sl = 0; sl < nslot; ++sl) {
    const int j = sl * 256 + tid;
    const bool keep = j >= 1 && j < N && (int)rank[j] < K;
    const unsigned long long mask = __ballot(keep);
    const int below = __popcll(mask & ((1ull << lane) - 1ull));
    const int pos = wtot[sl * 4 + wave] + below;
    if (keep && pos < K) out[1 + pos] = j;  // pos < K always: K tokens have a rank below K
  }
}

__global__ __launch_bounds__(256) void token_gather_kernel(
    const u32x4* __restrict__ src, u32x4* __restrict__ dst, const u32x4* __restrict__ ssrc,
    u32x4* __restrict__ sdst, const int* __restrict__ kept, int T, int K1, int cr, int cs,
    int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int per = cr + cs;
  const int r = idx / per, ch = idx - r * per;  // destination row, its chunk
  const int b = r / K1;
  const int k = min(max(kept[r], 0), T - 1);
  const int64_t srow = (int64_t)b * T + k;
  if (ch < cr)
    store_b128(dst + (int64_t)r * cr + ch, src[srow * cr + ch]);
  else
    store_b128(sdst + (int64_t)r * cs + (ch - cr), ssrc[srow * cs + (ch - cr)]);
}

}  // namespace

hipError_t token_scores_launch(int dtype, const AttnParams& p_in, float* out, hipStream_t s) {
  if (p_in.B <= 0) return hipSuccess;
  AttnParams p;
  if (!prepare(dtype, p_in, out, p, 4)) return hipErrorInvalidValue;
  const int nkb = (p.N + KB - 1) / KB;
  if ((int64_t)p.B * nkb > INT32_MAX) return hipErrorInvalidValue;
  return dispatch(dtype, p.hd, [&](auto v) {
    using V = decltype(v);
    using T = typename V::type;
    hipLaunchKernelGGL((token_scores_kernel<T, V::DP>), dim3(p.B * nkb), dim3(256),
                       score_lds(sizeof(T), V::DP, false), s, p, nkb, out);
    return hipGetLastError();
  });
}

hipError_t token_select_launch(const float* scores, int B, int N, int K, int* kept,
                               hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (!scores || !kept || N < 2 || N > SEL_MAX || K < 1 || K > N - 1 ||
      (((uintptr_t)scores | (uintptr_t)kept) & 3))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(token_select_kernel, dim3(B), dim3(256), 0, s, scores, N, K, kept);
  return hipGetLastError();
}

hipError_t token_gather_launch(int dtype, const void* src, void* dst, const float* ssrc,
                               float* sdst, int slots, const int* kept, int B, int T, int K1,
                               int D, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if ((dtype != DT_BF16 && dtype != DT_F32) || !src || !dst || !kept || T < 1 || K1 < 1 ||
      K1 > T || D < 8 || D % 8 || (!ssrc) != (!sdst) || (ssrc && (slots < 2 || slots % 2)) ||
      (((uintptr_t)src | (uintptr_t)dst | (uintptr_t)ssrc | (uintptr_t)sdst) & 15) ||
      ((uintptr_t)kept & 3))
    return hipErrorInvalidValue;
  const int cr = D * (dtype == DT_BF16 ? 2 : 4) / 16, cs = ssrc ? slots * 8 / 16 : 0;
  const int64_t total = (int64_t)B * K1 * (cr + cs);
  if (total > INT32_MAX - 256) return hipErrorInvalidValue;
  hipLaunchKernelGGL(token_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                     (const u32x4*)src, (u32x4*)dst, (const u32x4*)ssrc, (u32x4*)sdst, kept, T, K1,
                     cr, cs, (int)total);
  return hipGetLastError();
}

}  // namespace evt
