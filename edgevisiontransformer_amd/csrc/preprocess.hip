// uint8 resize + centre crop (include/evt_preprocess.h): Pillow's 8-bit resampling, integer work
// only. The 22-bit fixed-point tables come from the host (capi.cpp); the output is a pure function
// of the tables and the bytes.
//
// One workgroup = one image and a band of tr output rows (ResizeDesc). It
//   1. runs the horizontal pass over exactly the input rows the band's vertical taps read
//      (bounds_v[y0].ymin .. bounds_v[y1-1].ymin + n) and the S crop columns, and leaves the uint8
//      intermediate [rows][S*C] in LDS (row pitch rounded up to 16 B, so a 16-B chunk of a row is
//      one aligned ds_read_b128);
//   2. runs the vertical pass out of LDS and stores the band, which is one contiguous byte range
//      of the dense output, in 16-B-aligned chunks through store_b128; where S*C is no multiple of
//      16 the range's head and tail go out as dwords and a chunk may straddle two rows.
// The source is read through L1 with byte loads: no alignment is asked of a source pointer or
// pitch, and no byte outside an image row is touched. Neighbouring lanes read neighbouring pixels
// and a row's taps overlap, so the lines stay in L1 for the whole row; the tables (a few KB per
// plan) are read the same way. Products are 8-bit x 24-bit (|kk| < 2^23 is checked at plan
// creation): v_mad_i32_i24, full rate.
#include "common.h"

namespace evt {

// clamp(acc >> 22, 0, 255), written as a clamp to [0, 2^30) before the shift. The direct form is
// matched by hipcc 7.2 into v_ashr_pk_u8_i32 for two neighbouring bytes; that instruction writes
// 16 bits and leaves the upper half of its destination as it was, while the code around it ORs
// bytes 2 and 3 in as if the upper half were zero (seen on gfx950: byte 2 of dwords 1-3 of every
// 16-byte chunk came out ORed with the previous dword's). This form compiles to v_med3 + v_lshr.
__device__ __forceinline__ unsigned clamp_u8(int acc) {
  return (unsigned)min(max(acc, 0), 0x3fffffff) >> 22;
}

// 4 output bytes at byte offset `off` of the band (off % 4 == 0; a dword never straddles a row
// since S*C % 4 == 0)
__device__ __forceinline__ unsigned vertical_dword(const uint8_t* lds, int off, int rowb, int lp,
                                                   int y0, int ymin0, const int32_t* bv,
                                                   const int32_t* kv, int ksv) {
  const int dy = off / rowb, j = off - dy * rowb, y = y0 + dy;
  const int ymin = bv[2 * y], n = bv[2 * y + 1];
  const int32_t* k = kv + y * ksv;
  const uint8_t* p = lds + (ymin - ymin0) * lp + j;
  int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
  for (int t = 0; t < n; ++t) {
    const unsigned w = *(const unsigned*)(p + t * lp);
    const int c = k[t];
    a0 += __mul24((int)(w & 255u), c);
    a1 += __mul24((int)((w >> 8) & 255u), c);
    a2 += __mul24((int)((w >> 16) & 255u), c);
    a3 += __mul24((int)(w >> 24), c);
  }
  return clamp_u8(a0) | (clamp_u8(a1) << 8) | (clamp_u8(a2) << 16) | (clamp_u8(a3) << 24);
}

template <int C>
__global__ __launch_bounds__(256) void resize_crop_kernel(ResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x, blk = blockIdx.x;
  int img = 0;
  while (img + 1 < a.n && blk >= a.d[img + 1].blk0) ++img;  // wave-uniform, at most 63 steps
  const ResizeDesc d = a.d[img];
  const int S = a.S, rowb = S * C, lp = (rowb + 15) & ~15;
  const int32_t* bh = d.tab;
  const int32_t* kh = bh + 2 * S;
  const int32_t* bv = kh + S * d.ksh;
  const int32_t* kv = bv + 2 * S;
  const int y0 = (blk - d.blk0) * d.tr, y1 = min(y0 + d.tr, S);
  const int ymin0 = bv[2 * y0];
  const int rows = bv[2 * (y1 - 1)] + bv[2 * (y1 - 1) + 1] - ymin0;

  // ---- horizontal: input rows ymin0 .. ymin0+rows-1, crop columns, into LDS ----
  for (int it = tid; it < rows * S; it += 256) {
    const int r = it / S, x = it - r * S;
    const int xmin = bh[2 * x], n = bh[2 * x + 1];
    const int32_t* k = kh + x * d.ksh;
    const uint8_t* p = d.src + (int64_t)(ymin0 + r) * d.pitch + xmin * C;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << 21;
    for (int t = 0; t < n; ++t) {
      const int w = k[t];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += __mul24((int)p[t * C + c], w);
    }
    uint8_t* q = lds + r * lp + x * C;
    if (C == 4) {
      *(unsigned*)q = clamp_u8(acc[0]) | (clamp_u8(acc[C > 1 ? 1 : 0]) << 8) |
                      (clamp_u8(acc[C > 2 ? 2 : 0]) << 16) | (clamp_u8(acc[C > 3 ? 3 : 0]) << 24);
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) q[c] = (uint8_t)clamp_u8(acc[c]);
    }
  }
  __syncthreads();

  // ---- vertical: the band's bytes [0, total) of the output, from LDS ----
  const int total = (y1 - y0) * rowb;  // % 4 == 0
  uint8_t* o = a.out + ((int64_t)img * S + y0) * rowb;
  if ((rowb & 15) == 0) {
    // rows are whole 16-B chunks and o is 16-B aligned: a chunk is one row's, at j % 16 == 0
    const int per = rowb >> 4;
    for (int ch = tid; ch < (total >> 4); ch += 256) {
      const int dy = ch / per, j = (ch - dy * per) << 4, y = y0 + dy;
      const int ymin = bv[2 * y], n = bv[2 * y + 1];
      const int32_t* k = kv + y * d.ksv;
      const uint8_t* p = lds + (ymin - ymin0) * lp + j;
      int acc[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 1 << 21;
      for (int t = 0; t < n; ++t) {
        const u32x4 w = *(const u32x4*)(p + t * lp);
        const int c = k[t];
#pragma unroll
        for (int i = 0; i < 16; ++i)
          acc[i] += __mul24((int)((w[i >> 2] >> (8 * (i & 3))) & 255u), c);
      }
      u32x4 v;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        v[i] = clamp_u8(acc[4 * i]) | (clamp_u8(acc[4 * i + 1]) << 8) |
               (clamp_u8(acc[4 * i + 2]) << 16) | (clamp_u8(acc[4 * i + 3]) << 24);
      store_b128(o + (ch << 4), v);
    }
  } else {
    // o is 4-B aligned: dwords up to the first 16-B boundary, aligned chunks, dwords after
    const int head = min(total, (int)((16u - (unsigned)((uintptr_t)o & 15u)) & 15u));
    const int nch = (total - head) >> 4;
    const int tail0 = head + (nch << 4);
    for (int ch = tid; ch < nch; ch += 256) {
      const int off = head + (ch << 4);
      u32x4 v;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        v[i] = vertical_dword(lds, off + 4 * i, rowb, lp, y0, ymin0, bv, kv, d.ksv);
      store_b128(o + off, v);
    }
    const int nhead = head >> 2, nedge = nhead + ((total - tail0) >> 2);
    for (int e = tid; e < nedge; e += 256) {
      const int off = e < nhead ? 4 * e : tail0 + 4 * (e - nhead);
      *(unsigned*)(o + off) = vertical_dword(lds, off, rowb, lp, y0, ymin0, bv, kv, d.ksv);
    }
  }
}

hipError_t resize_crop_launch(const ResizeArgs& a, int C, int blocks, size_t lds, hipStream_t s) {
  if (blocks <= 0 || lds > 65536 || a.n < 1 || a.n > RESIZE_CHUNK) return hipErrorInvalidValue;
  switch (C) {
    case 1: hipLaunchKernelGGL(resize_crop_kernel<1>, dim3(blocks), dim3(256), lds, s, a); break;
    case 2: hipLaunchKernelGGL(resize_crop_kernel<2>, dim3(blocks), dim3(256), lds, s, a); break;
    case 3: hipLaunchKernelGGL(resize_crop_kernel<3>, dim3(blocks), dim3(256), lds, s, a); break;
    case 4: hipLaunchKernelGGL(resize_crop_kernel<4>, dim3(blocks), dim3(256), lds, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace evt
