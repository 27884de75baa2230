// Activation Grams (include/evt_gram.h): second moments of a row-major matrix a[r][j] of R rows and
// F columns (row pitch ld elements, model dtype), in fp32:
//
//   gram[i][j] = sum_r a[r][i] a[r][j]     [F][F], both triangles, bitwise symmetric
//   sums[j]    = sum_r a[r][j]             [F]
//
// gram_kernel. A workgroup (4 waves) owns one 128 x 128 tile (ti <= tj) of the upper triangle and
// one chunk of rows; a wave a 64 x 64 quadrant as 4 x 4 MFMA tiles (64 accumulator registers). Both
// MFMA operands are columns of `a`, so both are read along the non-contiguous axis:
//
//   bf16  v_mfma_f32_16x16x32_bf16. A 64-row piece of the two 128-column panels (columns of tile
//         ti, columns of tile tj; one panel on the diagonal) goes through registers into an LDS
//         image of plain 256-byte rows whose 16-byte chunks are swizzled,
//             off(row, ch) = 256 row + 16 (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))),
//         and every fragment is two ds_read_tr16_b64 of it: lane 4 q + p of a 16-lane group
//         gives the address of row r0 + q, columns 4 p .. 4 p + 3 of a 4-row x 16-column block and
//         receives column (lane & 15) of the four rows. Within a 32-row step lane group g reads the
//         blocks at rows 8 (g & 1) + 4 (g >> 1) and 16 more, for both operands alike (the k order
//         of an MFMA is free as long as both operands share it). The two groups of a 32-lane half
//         are then 8 rows apart in the same columns: their chunk swizzles differ in bit 1, the 32
//         lanes cover the 32 8-byte slots of the 64 banks once, no conflict. Addresses are
//         multiples of 8 and the kernel has no divergent branch around a read (EXEC all ones).
//   fp32  the exact v_mfma_f32_16x16x4_f32 (one k per lane: no transpose). 32-row pieces, LDS rows
//         of 128 + 4 floats: the lane groups of a ds_read_b32 (rows 4 g + e) land 16 banks apart.
//
// The loads of piece i + 1 are issued before the MFMAs of piece i. A row >= the chunk's end or a
// 16-byte vector whose first column is >= F is never loaded: its LDS image is literal zeros, which add
// +0. ld is a multiple of the vector and >= F, so every vector that is loaded lies inside its row's
// pitch. When F is no multiple of the vector (a pruned block's 230 neurons under a pitch of 256) the
// vector that straddles F brings up to V - 1 padding columns, whatever they hold, into column c >= F
// of a panel: an MFMA keeps them in output row / column c, which no store touches (only i, j < F
// are written).
//
// sums: the diagonal tiles stream every row of their 128 columns. A staging thread owns one
// 16-byte vector of columns for all its rows, adds them in fp32 in row order, and the threads of a
// column meet in LDS in thread order.
//
// Row chunks. Few tiles (F = 768: 21) leave most of the device idle, so gram_plan (evt_internal.h)
// also splits the rows, by (R, F) alone: each (tile, chunk) workgroup then writes its fp32 tile into
// the caller's scratch and gram_reduce_kernel adds the chunks in chunk order and stores. With one
// chunk the tile kernel stores itself and no scratch is read. Either way an element of the upper
// triangle is computed once and stored twice, at [i][j] and [j][i] (on a diagonal tile only i <= j
// is stored from), so the result is bitwise symmetric; the order of every sum depends on (R, F)
// alone, so it is bitwise reproducible. No atomics, no scratch memory (private segment 0 bytes),
// 64-bit row offsets. The wave that owns the strictly lower quadrant of a diagonal tile computes
// what is never stored: skipping its MFMAs under a wave-uniform branch was tried and made the
// compiler keep the accumulators live in both files (166 VGPRs + 96 AGPRs instead of 120 + 64, one
// wave per SIMD instead of two), so the quadrant stays.
#include "common.h"
#include "evt_internal.h"

namespace evt {

namespace {

constexpr int TILE = GRAM_TILE, THREADS = 256;
static_assert(TILE == 128, "the wave quadrants and the staging maps are written for 128");

template <typename T> struct GramCfg;
template <> struct GramCfg<bf16> {
  static constexpr int V = 8, KC = 64;
  typedef bf16x8 vec_t;
  static constexpr int PANEL = KC * TILE * 2;  // bytes
  // byte offset of 16-byte chunk ch (0 .. 15) of row `row` of the panel image
  static __device__ __forceinline__ int off(int row, int ch) {
    return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
  }
};
template <> struct GramCfg<float> {
  static constexpr int V = 4, KC = 32, PITCH = TILE + 4;
  typedef f32x4 vec_t;
  static constexpr int PANEL = KC * PITCH * 4;  // bytes
  static __device__ __forceinline__ int off(int row, int ch) { return (row * PITCH + 4 * ch) * 4; }
};
static_assert(GramCfg<bf16>::KC == GRAM_ROW_QUANTUM && GRAM_ROW_QUANTUM % GramCfg<float>::KC == 0,
              "a row chunk is whole pieces of both kernels");

// One staged piece: acc[mt][nt] += (columns 64 wr + 16 mt .. of panel A)^T (columns 64 wc + 16 nt ..
// of panel B). acc[mt][nt][j] belongs to tile row 64 wr + 16 mt + 4 g + j, column 64 wc + 16 nt + c16.
__device__ __forceinline__ void gram_mma(const char* As, const char* Bs, f32x4 (&acc)[4][4], int wr,
                                         int wc, int lane, bf16) {
  typedef GramCfg<bf16> C;
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int rg = 8 * (g & 1) + 4 * (g >> 1) + q;
#pragma unroll
  for (int ks = 0; ks < C::KC / 32; ++ks) {
    const int r0 = 32 * ks + rg, r1 = r0 + 16;
    bf16x8 af[4], bfr[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int ca = 8 * wr + 2 * t + (p >> 1), cb = 8 * wc + 2 * t + (p >> 1), h = 8 * (p & 1);
      const i16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((EVT_LDS i16x4*)(As + C::off(r0, ca) + h));
      const i16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((EVT_LDS i16x4*)(As + C::off(r1, ca) + h));
      const i16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((EVT_LDS i16x4*)(Bs + C::off(r0, cb) + h));
      const i16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((EVT_LDS i16x4*)(Bs + C::off(r1, cb) + h));
      af[t] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7));
      bfr[t] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7));
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[mt], bfr[nt], acc[mt][nt], 0, 0, 0);
  }
}

__device__ __forceinline__ void gram_mma(const char* As, const char* Bs, f32x4 (&acc)[4][4], int wr,
                                         int wc, int lane, float) {
  typedef GramCfg<float> C;
  const int g = lane >> 4, c16 = lane & 15;
  const float* A = (const float*)As + 64 * wr + c16;
  const float* B = (const float*)Bs + 64 * wc + c16;
#pragma unroll
  for (int kg = 0; kg < C::KC / 16; ++kg) {
    float a[4][4], b[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a[t][e] = A[(16 * kg + 4 * g + e) * C::PITCH + 16 * t];
        b[t][e] = B[(16 * kg + 4 * g + e) * C::PITCH + 16 * t];
      }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][e], b[nt][e], acc[mt][nt], 0, 0, 0);
  }
}

// part == nullptr: one row chunk, the tile and its mirror go to gram, the diagonal tiles' column
// sums to sums. Otherwise chunk s of tile t writes its 128 x 128 fp32 tile to part[s * tiles + t] and a
// diagonal tile its 128 column sums behind the tiles, at [s * nt + ti] (gram_reduce_kernel).
template <typename T>
__global__ __launch_bounds__(THREADS) void gram_kernel(const T* __restrict__ a, int64_t ld, int R,
                                                       int F, int nt, int tiles, int rows_per_chunk,
                                                       int chunks, float* __restrict__ gram,
                                                       float* __restrict__ sums,
                                                       float* __restrict__ part) {
  typedef GramCfg<T> C;
  typedef typename C::vec_t vec_t;
  constexpr int V = C::V, KC = C::KC, CH = TILE / V, RSTEP = THREADS / CH, NLD = KC / RSTEP;
  static_assert(2 * C::PANEL >= RSTEP * TILE * 4, "the column sums meet in the panels' space");
  __shared__ __attribute__((aligned(16))) char smem[2 * C::PANEL];
  char* As = smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int s = blockIdx.x / tiles, t = blockIdx.x - s * tiles;
  int ti = 0, rem = t;
  while (rem >= nt - ti) {  // tile t of the upper triangle, row by row
    rem -= nt - ti;
    ++ti;
  }
  const int tj = ti + rem, i0 = ti * TILE, j0 = tj * TILE;
  const bool diag = ti == tj;
  char* Bs = diag ? As : smem + C::PANEL;
  const int r_begin = s * rows_per_chunk;
  const int r_end = min(R, r_begin + rows_per_chunk);

  // this thread's NLD + NLD vectors of a piece: rows rrow + RSTEP i, chunk ch of both panels
  const int ch = tid % CH, rrow = tid / CH;
  const int ca = i0 + V * ch, cb = j0 + V * ch;
  vec_t ra[NLD], rb[NLD];
  auto load = [&](int r0) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int row = r0 + rrow + RSTEP * i;
      vec_t z;
#pragma unroll
      for (int e = 0; e < V; ++e) z[e] = (T)0.f;
      ra[i] = rb[i] = z;
      if (row < r_end) {
        const T* src = a + (int64_t)row * ld;
        if (ca < F) ra[i] = *(const vec_t*)(src + ca);
        if (!diag && cb < F) rb[i] = *(const vec_t*)(src + cb);
      }
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[mt][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float csum[V];
#pragma unroll
  for (int e = 0; e < V; ++e) csum[e] = 0.f;

  load(r_begin);
  for (int r0 = r_begin; r0 < r_end; r0 += KC) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int o = C::off(rrow + RSTEP * i, ch);
      *(EVT_LDS vec_t*)(As + o) = ra[i];
      if (!diag) *(EVT_LDS vec_t*)(Bs + o) = rb[i];
    }
    if (diag) {
#pragma unroll
      for (int i = 0; i < NLD; ++i)
#pragma unroll
        for (int e = 0; e < V; ++e) csum[e] += (float)ra[i][e];
    }
    __syncthreads();
    if (r0 + KC < r_end) load(r0 + KC);  // in flight under the MFMAs below
    gram_mma(As, Bs, acc, wr, wc, lane, T());
    __syncthreads();  // every wave is done with the piece before the next one lands
  }

  const int g = lane >> 4, c16 = lane & 15;
  const bool vec_rows = F % 4 == 0;  // every output row starts 16-byte aligned
  if (part) {
    float* dst = part + ((int64_t)s * tiles + t) * (TILE * TILE);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          dst[(64 * wr + 16 * mt + 4 * g + j) * TILE + 64 * wc + 16 * n + c16] = acc[mt][n][j];
  } else {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int m4 = i0 + 64 * wr + 16 * mt + 4 * g, col = j0 + 64 * wc + 16 * n + c16;
        if (col >= F || m4 >= F) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (m4 + j < F && (!diag || m4 + j <= col)) gram[(int64_t)(m4 + j) * F + col] = acc[mt][n][j];
        if (!diag && vec_rows) {  // rows m4 .. m4 + 3 are all below F and 16-byte aligned
          store_f32x4(gram + (int64_t)col * F + m4, acc[mt][n]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (m4 + j < F && (!diag || m4 + j < col)) gram[(int64_t)col * F + m4 + j] = acc[mt][n][j];
        }
      }
  }

  if (diag) {  // block-uniform
    float* cs = (float*)smem;  // [RSTEP][TILE]; the loop's last barrier freed the panels
#pragma unroll
    for (int e = 0; e < V; ++e) cs[rrow * TILE + V * ch + e] = csum[e];
    __syncthreads();
    if (tid < TILE) {
      float v = cs[tid];
#pragma unroll
      for (int r = 1; r < RSTEP; ++r) v += cs[r * TILE + tid];
      if (part) part[(int64_t)chunks * tiles * (TILE * TILE) + ((int64_t)s * nt + ti) * TILE + tid] = v;
      else if (i0 + tid < F) sums[i0 + tid] = v;
    }
  }
}

// The chunks of a tile added in chunk order, then stored as gram_kernel stores. Block b < 16 tiles:
// rows 8 (b % 16) .. + 7 of tile b / 16, a thread four consecutive columns; the nt blocks after them:
// the column sums of one diagonal tile.
__global__ __launch_bounds__(THREADS) void gram_reduce_kernel(const float* __restrict__ part,
                                                              int chunks, int tiles, int nt, int F,
                                                              float* __restrict__ gram,
                                                              float* __restrict__ sums) {
  const int tid = threadIdx.x;
  const int64_t tile_sz = TILE * TILE;
  if ((int)blockIdx.x >= 16 * tiles) {
    const int ti = blockIdx.x - 16 * tiles;
    if (tid >= TILE) return;
    const float* src = part + (int64_t)chunks * tiles * tile_sz + ti * TILE + tid;
    float v = src[0];
    for (int s = 1; s < chunks; ++s) v += src[(int64_t)s * nt * TILE];
    if (ti * TILE + tid < F) sums[ti * TILE + tid] = v;
    return;
  }
  const int t = blockIdx.x >> 4, strip = blockIdx.x & 15;
  int ti = 0, rem = t;
  while (rem >= nt - ti) {
    rem -= nt - ti;
    ++ti;
  }
  const int tj = ti + rem;
  const int row = 8 * strip + (tid >> 5), c4 = 4 * (tid & 31);
  const float* src = part + (int64_t)t * tile_sz + row * TILE + c4;
  f32x4 v = *(const f32x4*)src;
  for (int s = 1; s < chunks; ++s) v += *(const f32x4*)(src + (int64_t)s * tiles * tile_sz);
  const int m = ti * TILE + row, n4 = tj * TILE + c4;
  if (m >= F || n4 >= F) return;
  if (ti != tj && F % 4 == 0) {  // columns n4 .. n4 + 3 are all below F and 16-byte aligned
    store_f32x4(gram + (int64_t)m * F + n4, v);
#pragma unroll
    for (int c = 0; c < 4; ++c) gram[(int64_t)(n4 + c) * F + m] = v[c];
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (n4 + c >= F) continue;
      if (ti != tj || m <= n4 + c) gram[(int64_t)m * F + n4 + c] = v[c];
      if (ti != tj || m < n4 + c) gram[(int64_t)(n4 + c) * F + m] = v[c];
    }
  }
}

}  // namespace

hipError_t gram_launch(int dtype, const void* a, int64_t ld, int rows, int F, float* gram,
                       float* sums, void* scratch, size_t scratch_bytes, hipStream_t s) {
  const int V = dtype == DT_BF16 ? 8 : 4;
  if ((dtype != DT_BF16 && dtype != DT_F32) || !a || !gram || !sums || rows < 1 || F < 1 ||
      F > GRAM_MAX_WIDTH || ld < F || ld % V ||
      (((uintptr_t)a | (uintptr_t)gram | (uintptr_t)sums) & 15))
    return hipErrorInvalidValue;
  const GramPlan p = gram_plan(rows, F);
  if (p.scratch_bytes && (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < p.scratch_bytes))
    return hipErrorInvalidValue;
  float* part = p.scratch_bytes ? (float*)scratch : nullptr;
  const dim3 grid((unsigned)(p.chunks * p.tiles)), block(THREADS);
  if (dtype == DT_BF16)
    hipLaunchKernelGGL(gram_kernel<bf16>, grid, block, 0, s, (const bf16*)a, ld, rows, F, p.nt,
                       p.tiles, p.rows_per_chunk, p.chunks, gram, sums, part);
  else
    hipLaunchKernelGGL(gram_kernel<float>, grid, block, 0, s, (const float*)a, ld, rows, F, p.nt,
                       p.tiles, p.rows_per_chunk, p.chunks, gram, sums, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !part) return e;
  hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)(16 * p.tiles + p.nt)), block, 0, s, part,
                     p.chunks, p.tiles, p.nt, F, gram, sums);
  return hipGetLastError();
}

}  // namespace evt
