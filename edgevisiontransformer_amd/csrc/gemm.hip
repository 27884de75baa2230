// Token-matrix GEMM for the ViT encoder on gfx950 (MI355X, CDNA4).
//
// Replaces every tf.keras.layers.Dense on the hot path (reference `modeling/layers/attention.py:17-18`
// to_qkv / to_out, `modeling/layers/ffn.py:8-9` FC1+gelu / FC2, `modeling/models/vit.py:23,38-39`
// patch_to_embedding / mlp_head) with fused epilogues, including the two LayerNorms of every
// encoder layer (reference `modeling/layers/norm.py:6,12`), which never run as kernels of their
// own (see "LayerNorm folding" below).
//
// Layout. A (activations) is row-major [M][lda]; weights are packed once at model creation to
// Wp[Npad][Kpad] (K-contiguous, zero padded), so both MFMA operands are 16-byte K-contiguous
// reads. Tiles of A and W are staged into LDS with global_load_lds (async, 16 B/lane); the LDS
// image is row-linear and the bank-conflict swizzle (chunk ^ (row & 7)) is applied to the
// per-lane SOURCE address and to the ds_read address (glds writes lane-linear).
//
// MFMA. The product is computed transposed, C^T = W . A^T (16x16 C layout: col = lane&15 ->
// token row m, row = 4*(lane>>4)+j -> feature n).
//   bf16: v_mfma_f32_16x16x32_bf16, one 16-B chunk (8 k) per MFMA.
//   f32 : v_mfma_f32_16x16x4_f32 (exact fp32, the parity path), one 16-B chunk = 4 MFMAs with a
//         k-permutation shared by both operands.
//
// Kernels.
//   gemm_nt_kernel   128x128 tile, 4 waves (64x64 each), 2 blocks/CU; bf16 and f32.
//   gemm_big_kernel  256x256 tile, 8 waves (128x64 each), 128 KiB LDS, 1 block/CU; bf16, used
//                    when the problem has >= 256 such tiles (every encoder GEMM at bs >= 64).
// Both stage the finished accumulator tile through LDS (fp32, XOR-swizzled 512-B rows) and run
// the epilogue row-major ("epi_rows"): every lane owns 4 consecutive columns of one row and a
// wave streams 2 full 128-column row segments per instruction, so bias / residual / position
// loads, output stores and LayerNorm row statistics are all coalesced.
//
// LayerNorm folding. The reference sublayer is y = LN(x); out = f(y) + y (norm.py:11-12 +
// residual.py:9; the residual is the NORMALISED input). With per-row mean mu, rstd r of x and
// LN(x) = (x - mu) r gamma + beta, the first Dense of the sublayer is
//     y . W = r (x . W') - r mu s + c,   W' = diag(gamma) W,  s = 1^T W',  c = beta . W (+ bias)
// so QKV / FC1 consume the raw stream x and apply (mu, r) per row in the epilogue (EPI_LNIN);
// the residual y is rebuilt element-wise from x in the out-proj / FC2 epilogue (EPI_RESLN), and
// those epilogues accumulate the row sums (sum x, sum x^2) of the new stream for the next
// LayerNorm with one atomic pair per row segment (EPI_STATS). No LayerNorm kernel, no fp32
// stream: the token stream x is kept in the activation dtype.
//
// Grid. 1-D, XCD-aware bijective remap so that consecutive logical tiles (same A rows, all N
// tiles) run on one XCD and share its L2.
#include <type_traits>

#include "common.h"
#include "evt_internal.h"
#include "gemm_epi.h"
#include "gemm_nt.h"
#include "gemm_big8.h"
#include "gemm_big.h"
#include "gemm_pers.h"
#include "gemm_p384.h"
#include "gemm_sk.h"

namespace evt {

namespace {

// evt_set_gemm_variant, per calling thread (launch decisions are made on the launching thread).
// The numbers are the ABI. (Round-4 main-loop experiments measured slower - B-fragment prefetch,
// buffer-descriptor loader, residual in the main loop, residual L2 prefetch, phase-level lgkmcnt
// waits, DMA-first phases, MFMA priority - were removed in round 5, the ablation / timeline / A-B
// variants of the persistent kernel later; DESIGN.md records them and git history holds the code.)
enum : int {
  V_AUTO = 0,
  V_NT = 1,           // force 128x128
  V_BIG_PLAIN = 2,    // non-persistent 256x256, main loop without the explicit issue order
  V_BIG_SCHED = 6,    //   ... with it (sched_group_barrier)
  V_BIG8 = 8,         //   ... 8-phase main loop
  V_PERS = 9,         // tile-persistent
  V_STREAMK = 16,     // stream-K
  V_P384 = 30,        // 128 x 384 persistent wherever it applies
  V_NO_P384 = 31,     // automatic without 128 x 384
  V_NO_BALANCE = 36,  // automatic without grid balancing (launch_pers)
};
thread_local int g_gemm_variant = V_AUTO;

int g_num_cus = 0;
// persistent grid balancing (launch_pers): 1 = for launches of 2-4 tile rounds (default),
// 0 = never, 2 = always; EVT_GRID_BALANCE, read once (A/B switch)
const int g_grid_balance = [] {
  const char* e = std::getenv("EVT_GRID_BALANCE");
  return (e && e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : 1;
}();

int num_cus() {
  if (!g_num_cus) {
    int dev = 0;
    hipGetDevice(&dev);
    hipDeviceGetAttribute(&g_num_cus, hipDeviceAttributeMultiprocessorCount, dev);
  }
  return g_num_cus;
}

// The big kernels address inside a tile with 32-bit offsets: the LDS-DMA lane offsets (glds16s,
// unsigned, up to 384 rows of lda / ldw) and the epilogue's buffer-descriptor ranges (signed, up
// to 256 rows of ldc / ldr). Leading dimensions past that take the 128 x 128 kernel.
constexpr int64_t BIG_MAX_LD = ((int64_t)1 << 31) / (2 * 384) - 64;

constexpr bool pers_fl(int fl) {
  return fl == 0 || fl == EPI_BIAS || fl == (EPI_BIAS | EPI_GELU) || fl == (EPI_LNIN | EPI_BIAS) ||
         fl == (EPI_BIAS | EPI_POS | EPI_STATS) ||
         fl == (EPI_LNIN | EPI_BIAS | EPI_GELU) ||
         fl == (EPI_BIAS | EPI_RESID | EPI_RESLN | EPI_STATS) ||
         fl == (EPI_LNIN | EPI_BIAS | EPI_GELU_ERF) || fl == (EPI_BIAS | EPI_RESID | EPI_STATS) ||
         fl == (EPI_LNIN | EPI_BIAS | EPI_STATS) ||
         fl == (EPI_LNIN | EPI_BIAS | EPI_STATS | EPI_GATHER) ||
         fl == (EPI_LNIN | EPI_BIAS | EPI_SPLIT) || fl == (EPI_BIAS | EPI_POS | EPI_STATS | EPI_SPLIT) ||
         fl == (EPI_LNIN | EPI_BIAS | EPI_HM);
}

// LayerNorm rows of 10 / 12 statistics slots (widths 1025..1536): the WIDE instantiations of the
// persistent kernel (two statistics rounds, the comment at PERS_ACC), for the epilogues that meet
// such rows (Swin-L's 1536-wide stage and evt_dense); not the T2T / head-major ViT ones
constexpr bool pers_wide_fl(int fl) {
  return fl == (EPI_LNIN | EPI_BIAS) || fl == (EPI_LNIN | EPI_BIAS | EPI_GELU) ||
         fl == (EPI_LNIN | EPI_BIAS | EPI_GELU_ERF) || fl == (EPI_LNIN | EPI_BIAS | EPI_STATS) ||
         fl == (EPI_LNIN | EPI_BIAS | EPI_STATS | EPI_GATHER) ||
         fl == (EPI_BIAS | EPI_RESID | EPI_RESLN | EPI_STATS);
}

constexpr bool p384_fl(int fl) {
  return fl == (EPI_BIAS | EPI_RESID | EPI_RESLN | EPI_STATS) ||
         fl == (EPI_BIAS | EPI_RESID | EPI_STATS) || fl == (EPI_LNIN | EPI_BIAS | EPI_GELU) ||
         fl == (EPI_LNIN | EPI_BIAS);
}

bool use_big(const GemmParams& p, int flags) {
  // the CLS tail's launches: rstats / stats_out at a row step (the 128x128 epilogue only), and
  // one kernel whatever the batch is
  if (p.force_nt || p.rs_step > 1) return false;
  if ((p.ntiles * GEMM_BN) % BIG_BN) return false;
  if (std::max(std::max(p.lda, p.ldw), std::max(p.ldc, p.resid ? p.ldr : (int64_t)0)) > BIG_MAX_LD)
    return false;
  if (!(flags & EPI_OUT_F32) && p.vec_ok < 2) return false;  // big epilogue: 16-B bf16 stores only
  const int v = (g_gemm_variant == V_NO_P384 || g_gemm_variant == V_NO_BALANCE) ? V_AUTO
                                                                                : g_gemm_variant;
  if (v == V_NT) return false;
  if (v != V_AUTO) return true;  // every other variant is a 256 x 256 (or 128 x 384) kernel
  // 256x256 tiles unless their rounds cost more: time in 256-tile units, the 128x128 kernel at a
  // quarter of the work per tile and about half the FLOP rate (measured at 64 images: FC2 107 us
  // on 594 128x128 tiles against ~80 us for one round of 150 256x256 tiles); tiny problems (the
  // bs1 forward) keep the small tiles
  const int64_t G = num_cus();
  const int64_t t256 = (int64_t)((p.M + 255) / 256) * (p.ntiles * GEMM_BN / 256);
  const int64_t t128 = (int64_t)((p.M + 127) / 128) * p.ntiles;
  return (t256 + G - 1) / G <= 0.5 * (double)((t128 + G - 1) / G);
}

bool pers_wide(const GemmParams& p, int flags) {
  return (flags & (EPI_LNIN | EPI_RESLN)) && p.nslots > 8;
}

// persistent kernel: supported epilogue, 8-column output groups, LN rows of <= 8 slots (10 / 12:
// pers_wide)
bool use_pers(const GemmParams& p, int flags) {
  const int v = g_gemm_variant;
  if (v != V_AUTO && v != V_PERS && v != V_STREAMK && v != V_NO_P384 && v != V_NO_BALANCE)
    return false;
  if (p.N % 8 || p.vec_ok < 2 || p.force_nt || p.rs_step > 1) return false;
  if ((flags & (EPI_LNIN | EPI_RESLN)) && (p.nslots > 12 || p.nslots % 2 || p.stats_step > 1))
    return false;
  // 10 / 12 slots: two statistics rounds inside the main loop, which needs its K-tiles
  // (not under stream-K)
  if (pers_wide(p, flags) &&
      (!pers_wide_fl(flags) || p.K / 64 < PERS_WIDE_MIN_NK || v == V_STREAMK))
    return false;
  // POS: the bf16 copy of the position table rides in resid / ldr (else the staged-epilogue kernel)
  if ((flags & EPI_POS) && (!p.resid || p.ldr % 8 || p.P <= 0 || p.M >= (1 << 22))) return false;
  return true;
}

// XCD groups of the persistent walk (pers_tile): 2 where the weight panels split evenly over
// two groups of four XCDs and the launch has more than one round (FC1 of the D = 768 models: 12
// panels -> 6 per group; measured round 4: one group 484.5 us, two 479.9, four 479.3 per FC1 launch)
int pers_xgroups(int ntiles, int G, int total) {
  if (G != 256 || total <= G) return 1;  // the walk arithmetic assumes 8 XCDs of 32 blocks
  return (ntiles % 2 == 0 && ntiles / 2 >= 3) ? 2 : 1;
}

// 128 x 384 persistent tiles (gemm_p384_kernel) where the width is a multiple of 384 and their
// tile rounds cost less than the 256 x 256 grid's: rounds x tile work, a 128 x 384 tile = 0.75 of
// a 256 x 256 one (e.g. T2T-ViT-14 out-proj / FC2: 2 x 0.75 against 2 rounds of half-padded
// tiles; DeiT-base out-proj / FC2 at 64 images: 1 x 0.75 against one round on 150 CUs).
// evt_set_gemm_variant 30 forces it wherever it applies, 31 never.
bool use_p384(const GemmParams& p, int flags) {
  const int v = g_gemm_variant;
  if ((v != V_AUTO && v != V_P384) || p.N % 384 || p.vec_ok < 2 || p.K < 64) return false;
  if (p.force_nt || p.rs_step > 1) return false;
  if (std::max(std::max(p.lda, p.ldw), std::max(p.ldc, p.resid ? p.ldr : (int64_t)0)) > BIG_MAX_LD)
    return false;
  if ((flags & (EPI_LNIN | EPI_RESLN)) && (p.nslots > 8 || p.nslots % 2 || p.stats_step > 1))
    return false;
  if ((flags & EPI_STATS) && 3 * (p.N / 384) > p.nslots) return false;
  // automatic selection: never. Measured (round 4, rocprofv3, same box): a 128 x 384 tile takes
  // as long per K-tile as a 256 x 256 one (the main loop is bound by its 8 LDS-DMA instructions
  // per wave per K-tile, the same for both shapes, not by its MFMAs), so 0.75 of the work runs at
  // 0.75 of the FLOP rate: T2T-ViT-14 out-proj / FC2 53.1 vs 52.8 us, Swin-T 65.2 vs 65.1 us,
  // DeiT-base at 64 images 80.8 vs 70.6 us (128x128). Kept as the forced diagnostic variant 30.
  return v == V_P384;
}

constexpr int SK_MAX_G = 256;

int sk_grid() { return min(num_cus(), SK_MAX_G) & ~7; }

// stream-K: scratch bound, auto (0) or forced (16), every range of K-iterations at least one
// tile long (each tile has at most two parts)
bool use_sk(const GemmParams& p) {
  // explicit diagnostic only: an automatic stream-K split breaks bitwise batch-position
  // independence ("Stream-K for the 1.5-round D = 384 GEMMs")
  if (!p.sk_flags || !p.sk_part || g_gemm_variant != V_STREAMK) return false;
  const int G = sk_grid();
  const int total = ((p.M + BIG_BM - 1) / BIG_BM) * ((p.ntiles * GEMM_BN) / BIG_BN);
  return G >= 8 && total >= G;
}

bool headmajor_fits(const GemmParams& p) {
  return p.N % 192 == 0 && p.P > 0 && p.M % p.P == 0 && p.M < (1 << 22) &&
         (int64_t)p.M * p.N * 2 < ((int64_t)1 << 31) && g_gemm_variant != V_STREAMK &&
         g_gemm_variant != V_P384;
}

template <int FL>
hipError_t launch_big(const GemmParams& p, hipStream_t s) {
  const int mtiles = (p.M + BIG_BM - 1) / BIG_BM;
  GemmParams q = p;
  q.ntiles = (p.ntiles * GEMM_BN) / BIG_BN;
  const dim3 grid(mtiles * q.ntiles);
  // (gemm_big_kernel's VAR: 0 plain, 6 explicit issue order, 8 the 8-phase loop)
  if (g_gemm_variant == V_BIG_PLAIN)
    hipLaunchKernelGGL((gemm_big_kernel<FL, 0>), grid, dim3(512), 0, s, q);
  else if (g_gemm_variant == V_BIG8)
    hipLaunchKernelGGL((gemm_big_kernel<FL, 8>), grid, dim3(512), 0, s, q);
  else if constexpr ((FL & EPI_POS) != 0)  // patch embedding: 8-phase loop (153 vs 179 us, bs512)
    hipLaunchKernelGGL((gemm_big_kernel<FL, 8>), grid, dim3(512), 0, s, q);
  else
    hipLaunchKernelGGL((gemm_big_kernel<FL, 6>), grid, dim3(512), 0, s, q);
  return hipGetLastError();
}

template <int FL>
hipError_t launch_pers(const GemmParams& p, hipStream_t s) {
  num_cus();
  GemmParams q = p;
  q.ntiles = (p.ntiles * GEMM_BN) / BIG_BN;
  const int total = ((p.M + BIG_BM - 1) / BIG_BM) * q.ntiles;
  int G = min(total, g_num_cus);
  if (G >= 8 && total > G) G &= ~7;
  // 2-4 tile rounds: as few blocks as keep the round count (multiple of 8), every block the same
  // number of tiles. Measured round 6 (r6f, alternating): DeiT-base at 64 images 22.67k -> 23.30k
  // img/s (FC1 600 tiles: 200 blocks x 3 instead of 256 with 88 taking a third; QKV 450: 232 x 2),
  // the CUs left idle let the busy ones hold a higher clock; at 512 images (>= 5 rounds) -0.3 %,
  // not applied there. evt_set_gemm_variant 36: never (the tile -> block assignment only: bitwise
  // the same outputs); EVT_GRID_BALANCE=0 / 2: never / always (A/B)
  const int rounds = (total + G - 1) / G;
  const int bal = (g_gemm_variant == V_NO_BALANCE || p.no_balance) ? 0 : g_grid_balance;
  if (total > G && G >= 8 && (bal == 2 || (bal == 1 && rounds <= 4)))
    G = min(G, (((total + rounds - 1) / rounds) + 7) & ~7);
  // one round (one block per tile): up to a multiple of 8 blocks (the surplus exits at once) so
  // that the XCD-major start order applies and an m-panel's n-tiles run on one XCD, its A panel
  // fetched once into that L2 (DeiT-base FC2 at 64 images: 150 tiles, 3 per 1.5 MB A panel; in
  // block order the 3 went to 3 XCDs: 292 MB fetched per launch for ~100 MB of operands)
  else if (total <= G && (G & 7) && ((G + 7) & ~7) <= max(g_num_cus, 8)) G = (G + 7) & ~7;
  q.xgroups = pers_xgroups(q.ntiles, G, total);
  if constexpr (pers_wide_fl(FL)) {
    if (pers_wide(p, FL)) {
      if (p.N % BIG_BN == 0)
        hipLaunchKernelGGL((gemm_pers_kernel<FL, false, true>), dim3(G), dim3(512), 0, s, q, total);
      else
        hipLaunchKernelGGL((gemm_pers_kernel<FL, true, true>), dim3(G), dim3(512), 0, s, q, total);
      return hipGetLastError();
    }
  }
  if (p.N % BIG_BN == 0)
    hipLaunchKernelGGL((gemm_pers_kernel<FL, false>), dim3(G), dim3(512), 0, s, q, total);
  else
    hipLaunchKernelGGL((gemm_pers_kernel<FL>), dim3(G), dim3(512), 0, s, q, total);
  return hipGetLastError();
}

template <int FL>
hipError_t launch_p384(const GemmParams& p, hipStream_t s) {
  GemmParams q = p;
  q.ntiles = p.N / 384;
  const int total = ((p.M + 127) / 128) * q.ntiles;
  int G = min(total, num_cus());
  if (G >= 8 && total > G) G &= ~7;
  hipLaunchKernelGGL((gemm_p384_kernel<FL>), dim3(G), dim3(512), 0, s, q, total);
  return hipGetLastError();
}

template <int FL>
hipError_t launch_sk(const GemmParams& p, hipStream_t s) {
  GemmParams q = p;
  q.ntiles = (p.ntiles * GEMM_BN) / BIG_BN;
  const int total = ((p.M + BIG_BM - 1) / BIG_BM) * q.ntiles;
  hipLaunchKernelGGL((gemm_sk_kernel<FL>), dim3(sk_grid()), dim3(512), 0, s, q, total);
  return hipGetLastError();
}

template <typename T, int FL>
hipError_t launch_t(const GemmParams& p, hipStream_t s) {
  if constexpr ((FL & EPI_HM) != 0) {  // head-major store: the persistent kernel or nothing
    if constexpr (std::is_same<T, bf16>::value && pers_fl(FL)) {
      if (headmajor_fits(p) && use_big(p, FL) && use_pers(p, FL)) return launch_pers<FL>(p, s);
    }
    return hipErrorNotSupported;
  } else if constexpr ((FL & (EPI_GATHER | EPI_SPLIT)) != 0) {  // gathering loader: persistent kernel
    if constexpr (std::is_same<T, bf16>::value) {
      constexpr bool MERGE = (FL & EPI_GATHER) != 0;
      const bool merge = MERGE && p.gmode == 1 && p.gR % 2 == 0 && p.gOW == p.gR / 2 &&
                         p.gC % 8 == 0 && p.K == 4 * p.gC;
      const bool unfold = !MERGE && p.gmode == 2 && p.gC == 64 && p.K == 9 * 64 && p.gzero &&
                          p.gOW == (p.gR + 1) / 2;
      // the gathered loaders decode rows with float reciprocals: exact for rows < 2^22
      if ((merge || unfold) && p.gR > 0 && p.M < (1 << 22) && use_big(p, FL) && use_pers(p, FL) &&
          !use_sk(p))
        return launch_pers<FL>(p, s);
    }
    return hipErrorNotSupported;
  } else {
    if constexpr (std::is_same<T, bf16>::value) {
      if constexpr (p384_fl(FL)) {
        if (use_p384(p, FL)) return launch_p384<FL>(p, s);
      }
      if (use_big(p, FL)) {
        if constexpr (pers_fl(FL)) {
          if (use_pers(p, FL)) return use_sk(p) ? launch_sk<FL>(p, s) : launch_pers<FL>(p, s);
        }
        return launch_big<FL>(p, s);
      }
    }
    const int mtiles = (p.M + GEMM_BM - 1) / GEMM_BM;
    hipLaunchKernelGGL((gemm_nt_kernel<T, FL>), dim3(mtiles * p.ntiles), dim3(256), 0, s, p);
    return hipGetLastError();
  }
}

template <typename T>
hipError_t dispatch(int flags, const GemmParams& p, hipStream_t s) {
  switch (flags) {
#define EVT_CASE(F) \
  case (F): return launch_t<T, (F)>(p, s);
    EVT_CASE(0)                                              // plain (op-level)
    EVT_CASE(EPI_BIAS)
    EVT_CASE(EPI_BIAS | EPI_GELU)                            // head1
    EVT_CASE(EPI_BIAS | EPI_OUT_F32)                         // head2 (logits)
    EVT_CASE(EPI_BIAS | EPI_RESID | EPI_OUT_F32)             // op-level residual
    EVT_CASE(EPI_BIAS | EPI_POS | EPI_OUT_F32)               // op-level patch embed
    EVT_CASE(EPI_BIAS | EPI_POS | EPI_STATS)                 // patch embed -> stream + stats
    EVT_CASE(EPI_LNIN | EPI_BIAS)                            // LN1-folded QKV
    EVT_CASE(EPI_LNIN | EPI_BIAS | EPI_GELU)                 // LN2-folded FC1 + GELU
    EVT_CASE(EPI_LNIN | EPI_BIAS | EPI_OUT_F32)              // LN-folded classifier (T2T)
    EVT_CASE(EPI_BIAS | EPI_RESID | EPI_RESLN | EPI_STATS)   // out-proj / FC2 + LN residual
    EVT_CASE(EPI_LNIN | EPI_BIAS | EPI_GELU_ERF)             // Swin LN2-folded FC1 + erf GELU
    EVT_CASE(EPI_LNIN | EPI_BIAS | EPI_STATS | EPI_GATHER)   // Swin PatchMerging (gathered A)
    EVT_CASE(EPI_LNIN | EPI_BIAS | EPI_SPLIT)                // T2T soft_split1 + kqv (gathered A)
    EVT_CASE(EPI_BIAS | EPI_POS | EPI_STATS | EPI_SPLIT)     // T2T soft_split2 + project
    EVT_CASE(EPI_BIAS | EPI_RESID | EPI_STATS)               // Swin proj / FC2 + plain residual
    EVT_CASE(EPI_LNIN | EPI_BIAS | EPI_STATS)                // Swin LN-folded patch-merge reduction
    EVT_CASE(EPI_LNIN | EPI_BIAS | EPI_HM)                   // LN1-folded QKV, head-major output
#undef EVT_CASE
    default: return hipErrorInvalidValue;
  }
}

// out[m][n] = epilogue(sum_z part[z][m][n] + bias[n]), z in order (4 columns per thread)
template <typename T, bool GELU>
__global__ void splitk_reduce_kernel(const float* __restrict__ part, int S, int64_t stride,
                                     int ldp, const float* __restrict__ bias, T* __restrict__ out,
                                     int64_t ldo, int M, int N) {
  const int n4 = (N + 3) >> 2;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)M * n4) return;
  const int m = (int)(i / n4), n = (int)(i - (int64_t)m * n4) * 4;
  f32x4 v = *(const f32x4*)(part + (int64_t)m * ldp + n);
  for (int z = 1; z < S; ++z) v += *(const f32x4*)(part + z * stride + (int64_t)m * ldp + n);
  if (bias) v += *(const f32x4*)(bias + n);  // bias: >= ntiles*128 floats (zero padded)
  if (GELU) v = gelu4(v, 0);
  for (int j = 0; j < 4; ++j)
    if (n + j < N) out[(int64_t)m * ldo + n + j] = (T)v[j];
}

template <typename T>
hipError_t splitk_t(int flags, const GemmParams& p, int S, float* part, hipStream_t s) {
  GemmParams q = p;
  const int ldp = p.ntiles * GEMM_BN;
  q.ks_chunk = p.K / S;
  q.ks_stride = (int64_t)p.M * ldp;
  q.C = part;
  q.ldc = ldp;
  q.N = ldp;
  q.vec_ok = 2;
  q.bias = nullptr;
  const int mtiles = (p.M + GEMM_BM - 1) / GEMM_BM;
  hipLaunchKernelGGL((gemm_nt_kernel<T, EPI_OUT_F32>), dim3(mtiles * p.ntiles, S), dim3(256), 0, s, q);
  const int64_t n = (int64_t)p.M * ((p.N + 3) / 4);
  const dim3 grid((unsigned)((n + 255) / 256));
  const bool gelu = (flags & EPI_GELU) != 0;
  if (flags & EPI_OUT_F32) {
    if (gelu)
      hipLaunchKernelGGL((splitk_reduce_kernel<float, true>), grid, dim3(256), 0, s, part, S,
                         q.ks_stride, ldp, p.bias, (float*)p.C, p.ldc, p.M, p.N);
    else
      hipLaunchKernelGGL((splitk_reduce_kernel<float, false>), grid, dim3(256), 0, s, part, S,
                         q.ks_stride, ldp, p.bias, (float*)p.C, p.ldc, p.M, p.N);
  } else {
    if (gelu)
      hipLaunchKernelGGL((splitk_reduce_kernel<T, true>), grid, dim3(256), 0, s, part, S,
                         q.ks_stride, ldp, p.bias, (T*)p.C, p.ldc, p.M, p.N);
    else
      hipLaunchKernelGGL((splitk_reduce_kernel<T, false>), grid, dim3(256), 0, s, part, S,
                         q.ks_stride, ldp, p.bias, (T*)p.C, p.ldc, p.M, p.N);
  }
  return hipGetLastError();
}


// Wp[n][k] = W[k][n] * (scale ? scale[k] : 1) (fp32 [K][N] in) converted to T, zero outside
// [N) x [K). `scale` folds a LayerNorm gamma into the weight rows.
template <typename T>
__global__ void pack_kernel(const float* __restrict__ W, const float* __restrict__ scale, int K,
                            int N, T* __restrict__ Wp, int Kpad, int Npad) {
  __shared__ float tile[32][33];
  const int k0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: 8 rows per pass
  for (int r = ty; r < 32; r += 8) {
    const int k = k0 + r, n = n0 + tx;
    tile[r][tx] = (k < K && n < N) ? W[(int64_t)k * N + n] * (scale ? scale[k] : 1.f) : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int n = n0 + r, k = k0 + tx;
    if (n < Npad && k < Kpad) Wp[(int64_t)n * Kpad + k] = from_f32<T>(tile[tx][r]);
  }
}

// LayerNorm-fold vectors: colsum[n] = sum_k Wp[n][k] (of the packed, rounded weights, so that
// r (x.W') - r mu colsum == r ((x - mu).W') exactly w.r.t. the weights the GEMM uses) and
// cvec[n] = sum_k beta[k] W[k][n] + bias[n]. One wave per output column n.
template <typename T>
__global__ void fold_kernel(const T* __restrict__ Wp, int Kpad, const float* __restrict__ W,
                            const float* __restrict__ beta, const float* __restrict__ bias, int K,
                            int N, float* __restrict__ colsum, float* __restrict__ cvec, int Npad) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= Npad) return;
  float s = 0.f, c = 0.f;
  if (n < N) {
    for (int k = lane; k < K; k += 64) {
      s += to_f32(Wp[(int64_t)n * Kpad + k]);
      c += beta[k] * W[(int64_t)k * N + n];
    }
  }
  s = wave_sum(s);
  c = wave_sum(c);
  if (lane == 0) {
    colsum[n] = s;
    cvec[n] = (n < N) ? c + (bias ? bias[n] : 0.f) : 0.f;
  }
}

}  // namespace

int device_cus() { return num_cus(); }
void gemm_set_variant(int v) { g_gemm_variant = v; }
bool gemm_variant_supported(int v) {
  return v == V_AUTO || v == V_NT || v == V_BIG_PLAIN || v == V_BIG_SCHED || v == V_BIG8 ||
         v == V_PERS || v == V_STREAMK || v == V_P384 || v == V_NO_P384 || v == V_NO_BALANCE;
}
int gemm_variant() { return g_gemm_variant; }

size_t gemm_sk_bytes() { return 4096 + (size_t)SK_MAX_G * SK_SLOT_FLOATS * sizeof(float); }

void gemm_sk_bind(void* ws, GemmParams& p) {
  p.sk_flags = ws ? (int*)ws : nullptr;
  p.sk_part = ws ? (float*)((char*)ws + 4096) : nullptr;
}

bool gemm_headmajor_ok(int dtype, int flags, const GemmParams& p) {
  constexpr int F = EPI_LNIN | EPI_BIAS | EPI_HM;
  return dtype == DT_BF16 && (flags | EPI_HM) == F && p.K % PAD_K == 0 && p.K > 0 &&
         p.ntiles * GEMM_BN >= p.N && headmajor_fits(p) && use_big(p, F) && use_pers(p, F);
}

hipError_t gemm_launch(int dtype, int flags, const GemmParams& p, hipStream_t s) {
  if (p.M <= 0 || p.N <= 0) return hipSuccess;
  if (p.K % PAD_K != 0 || p.K <= 0) return hipErrorInvalidValue;
  if (p.ntiles * GEMM_BN < p.N) return hipErrorInvalidValue;
  return dtype == DT_BF16 ? dispatch<bf16>(flags, p, s) : dispatch<float>(flags, p, s);
}

hipError_t gemm_splitk_launch(int dtype, int flags, const GemmParams& p, int S, float* part,
                              hipStream_t s) {
  if (p.M <= 0 || p.N <= 0) return hipSuccess;
  if (S < 1 || p.K % (S * PAD_K) || (flags & ~(EPI_BIAS | EPI_GELU | EPI_OUT_F32)) || !part)
    return hipErrorInvalidValue;
  return dtype == DT_BF16 ? splitk_t<bf16>(flags, p, S, part, s) : splitk_t<float>(flags, p, S, part, s);
}

namespace {
__global__ void to_bf16_kernel(const float* __restrict__ x, bf16* __restrict__ y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = (bf16)x[i];
}
}  // namespace

hipError_t to_bf16_launch(const float* x, void* y, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(to_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, (bf16*)y, n);
  return hipGetLastError();
}

hipError_t pack_weight(int dtype, const float* W, const float* row_scale, int K, int N, void* Wp,
                       int Kpad, int Npad, hipStream_t s) {
  dim3 grid((Kpad + 31) / 32, (Npad + 31) / 32);
  if (dtype == DT_BF16)
    hipLaunchKernelGGL(pack_kernel<bf16>, grid, dim3(256), 0, s, W, row_scale, K, N, (bf16*)Wp,
                       Kpad, Npad);
  else
    hipLaunchKernelGGL(pack_kernel<float>, grid, dim3(256), 0, s, W, row_scale, K, N, (float*)Wp,
                       Kpad, Npad);
  return hipGetLastError();
}

hipError_t ln_fold(int dtype, const void* Wp, int Kpad, const float* W, const float* beta,
                   const float* bias, int K, int N, float* colsum, float* cvec, int Npad,
                   hipStream_t s) {
  dim3 grid((Npad + 3) / 4);
  if (dtype == DT_BF16)
    hipLaunchKernelGGL(fold_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)Wp, Kpad, W, beta,
                       bias, K, N, colsum, cvec, Npad);
  else
    hipLaunchKernelGGL(fold_kernel<float>, grid, dim3(256), 0, s, (const float*)Wp, Kpad, W, beta,
                       bias, K, N, colsum, cvec, Npad);
  return hipGetLastError();
}

}  // namespace evt
