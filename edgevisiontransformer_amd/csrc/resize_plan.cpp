// Host side of include/evt_preprocess.h: the filter tables, the geometry, the plans and
// evt_resize_crop_u8 (the kernel is preprocess.hip).
#include "model.h"

using namespace evt;

extern "C" {

// ---- uint8 resize + centre crop (include/evt_preprocess.h) -----------------------------------
// The tables are Pillow's (libImaging Resample.c precompute_coeffs / normalize_coeffs_8bpc),
// restated. fp64, every operation rounded on its own: no contraction in this part of the file.
#pragma clang fp contract(off)

static double resize_filter(int filter, double x) {
  if (x < 0.0) x = -x;
  if (filter == EVT_RESIZE_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
  const double a = -0.5;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

static bool resize_filter_ok(int filter) {
  return filter == EVT_RESIZE_BILINEAR || filter == EVT_RESIZE_BICUBIC;
}

static int resize_ksize(int in, int out, int filter) {
  double fs = (double)in / (double)out;
  if (fs < 1.0) fs = 1.0;
  const double support = (filter == EVT_RESIZE_BILINEAR ? 1.0 : 2.0) * fs;
  return (int)std::ceil(support) * 2 + 1;
}

// bounds [count][2] and kk [count][ksize] of output indices first .. first+count-1; false if a
// coefficient leaves the 24-bit range the kernel multiplies in (it cannot for these filters)
static bool resize_tables(int in, int out, int first, int count, int filter, int32_t* bounds,
                          int32_t* kk) {
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = (filter == EVT_RESIZE_BILINEAR ? 1.0 : 2.0) * fs;
  const double ss = 1.0 / fs;
  const int ksize = (int)std::ceil(support) * 2 + 1;
  std::vector<double> w((size_t)ksize);
  bool ok = true;
  for (int i = 0; i < count; ++i) {
    const double center = (first + i + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    const int n = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      w[x] = resize_filter(filter, (x + xmin - center + 0.5) * ss);
      ww += w[x];
    }
    int32_t* k = kk + (size_t)i * ksize;
    for (int x = 0; x < ksize; ++x) k[x] = 0;
    for (int x = 0; x < n; ++x) {
      const double v = ww != 0.0 ? w[x] / ww : w[x];
      const double f = v < 0 ? -0.5 + v * (double)(1 << 22) : 0.5 + v * (double)(1 << 22);
      if (!(std::fabs(f) < (double)(1 << 23))) ok = false;
      k[x] = (int32_t)f;
    }
    bounds[2 * i] = xmin;
    bounds[2 * i + 1] = n;
  }
  return ok;
}

struct ResizeGeom {
  int oh, ow, top, left, ksh, ksv;
};

static int round_half_even_half(int d) {  // round(d / 2.0), d >= 0, ties to even
  const int q = d / 2;
  return (d & 1) ? q + (q & 1) : q;
}

static int resize_geom(int in_h, int in_w, int R, int S, int filter, ResizeGeom* g) {
  if (in_h < 1 || in_w < 1 || in_h > EVT_RESIZE_MAX_SIDE || in_w > EVT_RESIZE_MAX_SIDE)
    return fail(EVT_EINVAL, "resize: image sides must be in [1, " +
                                std::to_string(EVT_RESIZE_MAX_SIDE) + "]");
  if (S < 1 || S > EVT_RESIZE_MAX_SIDE)
    return fail(EVT_EINVAL, "resize: crop must be in [1, " + std::to_string(EVT_RESIZE_MAX_SIDE) + "]");
  if (R < 0 || R > EVT_RESIZE_MAX_SIDE)
    return fail(EVT_EINVAL, "resize: resize_short must be in [0, " +
                                std::to_string(EVT_RESIZE_MAX_SIDE) + "] (0: int(256/224 * crop))");
  if (!resize_filter_ok(filter))
    return fail(EVT_EINVAL, "resize: filter must be EVT_RESIZE_BILINEAR (2) or EVT_RESIZE_BICUBIC (3)");
  if (R == 0) R = (int)((256.0 / 224.0) * (double)S);
  if (R < 1) return fail(EVT_EINVAL, "resize: resize_short must be at least 1");
  double other;
  if (in_w <= in_h) {
    other = (double)((int64_t)R * in_h) / (double)in_w;
    g->ow = R;
  } else {
    other = (double)((int64_t)R * in_w) / (double)in_h;
    g->oh = R;
  }
  if (other > 16.0 * EVT_RESIZE_MAX_SIDE)
    return fail(EVT_EINVAL, "resize: the resized long side is beyond any supported size");
  (in_w <= in_h ? g->oh : g->ow) = (int)other;
  if (g->oh < S || g->ow < S)
    return fail(EVT_EINVAL, "resize: the resized image " + std::to_string(g->oh) + " x " +
                                std::to_string(g->ow) + " is smaller than the crop " +
                                std::to_string(S) + " (padding is not done)");
  g->top = round_half_even_half(g->oh - S);
  g->left = round_half_even_half(g->ow - S);
  g->ksh = resize_ksize(in_w, g->ow, filter);
  g->ksv = resize_ksize(in_h, g->oh, filter);
  return EVT_OK;
}

#pragma clang fp contract(on)

struct evt_resize_plan {
  uint32_t magic;
  int in_h, in_w, C, S, tr, nbands;
  size_t lds;  // bytes of the largest band
  ResizeGeom g;
  int32_t* tab;  // device: ResizeDesc::tab
};
static constexpr uint32_t RESIZE_MAGIC = 0x52535a50u;  // "RSZP"
static constexpr int RESIZE_MAX_TR = 16;
static_assert(RESIZE_CHUNK == EVT_RESIZE_CHUNK, "evt_preprocess.h and evt_internal.h disagree");

int evt_resize_geometry(int in_h, int in_w, int resize_short, int crop, int filter, int* oh,
                        int* ow, int* top, int* left, int* ksize_h, int* ksize_v) {
  ResizeGeom g{};
  EVT_RC(resize_geom(in_h, in_w, resize_short, crop, filter, &g));
  if (oh) *oh = g.oh;
  if (ow) *ow = g.ow;
  if (top) *top = g.top;
  if (left) *left = g.left;
  if (ksize_h) *ksize_h = g.ksh;
  if (ksize_v) *ksize_v = g.ksv;
  return EVT_OK;
}

int evt_resize_coefficients(int in_size, int out_size, int first, int count, int filter,
                            int32_t* bounds, int32_t* kk) {
  if (!bounds || !kk) return fail(EVT_EINVAL, "resize_coefficients: bounds and kk must be non-null");
  if (in_size < 1 || out_size < 1 || in_size > EVT_RESIZE_MAX_SIDE ||
      out_size > 16 * EVT_RESIZE_MAX_SIDE)
    return fail(EVT_EINVAL, "resize_coefficients: sizes out of range");
  if (first < 0 || count < 0 || first > out_size - count)
    return fail(EVT_EINVAL, "resize_coefficients: the window must lie inside [0, out_size]");
  if (!resize_filter_ok(filter))
    return fail(EVT_EINVAL, "resize_coefficients: filter must be EVT_RESIZE_BILINEAR (2) or "
                            "EVT_RESIZE_BICUBIC (3)");
  if (!resize_tables(in_size, out_size, first, count, filter, bounds, kk))
    return fail(EVT_EINVAL, "resize_coefficients: a coefficient is outside the 24-bit range");
  return EVT_OK;
}

int evt_resize_plan_create(int in_h, int in_w, int channels, int resize_short, int crop,
                           int filter, evt_resize_plan** out) {
  if (!out) return fail(EVT_EINVAL, "resize_plan_create: out is NULL");
  *out = nullptr;
  if (channels < 1 || channels > 4)
    return fail(EVT_EINVAL, "resize_plan_create: uint8 images have 1 to 4 channels");
  ResizeGeom g{};
  EVT_RC(resize_geom(in_h, in_w, resize_short, crop, filter, &g));
  const int S = crop, C = channels;
  if (((int64_t)S * C) % 4)
    return fail(EVT_EINVAL, "resize_plan_create: crop*channels must be a multiple of 4");
  const int64_t lp = ((int64_t)S * C + 15) & ~(int64_t)15;
  const size_t ntab = (size_t)S * (4 + g.ksh + g.ksv);
  std::vector<int32_t> tab(ntab);
  int32_t* bh = tab.data();
  int32_t* kh = bh + 2 * S;
  int32_t* bv = kh + (size_t)S * g.ksh;
  int32_t* kv = bv + 2 * S;
  if (!resize_tables(in_w, g.ow, g.left, S, filter, bh, kh) ||
      !resize_tables(in_h, g.oh, g.top, S, filter, bv, kv))
    return fail(EVT_EINVAL, "resize_plan_create: a coefficient is outside the 24-bit range");
  // the kernel's band is rows bv[y0].ymin .. bv[y1-1].ymin + n: both ends must not decrease with y
  for (int y = 0; y < S; ++y) {
    const bool in_range = bv[2 * y] >= 0 && bv[2 * y + 1] >= 1 && bv[2 * y] + bv[2 * y + 1] <= in_h &&
                          bh[2 * y] >= 0 && bh[2 * y + 1] >= 1 && bh[2 * y] + bh[2 * y + 1] <= in_w &&
                          bv[2 * y + 1] <= g.ksv && bh[2 * y + 1] <= g.ksh;
    const bool monotonic = y == 0 || (bv[2 * y] >= bv[2 * y - 2] &&
                                      bv[2 * y] + bv[2 * y + 1] >= bv[2 * y - 2] + bv[2 * y - 1]);
    if (!in_range || !monotonic)
      return fail(EVT_EINVAL, "resize_plan_create: internal error, tap bounds out of order");
  }
  auto band_bytes = [&](int tr) {
    int64_t worst = 0;
    for (int y0 = 0; y0 < S; y0 += tr) {
      const int y1 = std::min(y0 + tr, S) - 1;
      worst = std::max<int64_t>(worst, (int64_t)(bv[2 * y1] + bv[2 * y1 + 1] - bv[2 * y0]) * lp);
    }
    return worst;
  };
  int tr = std::min(RESIZE_MAX_TR, S);
  while (tr > 1 && band_bytes(tr) > EVT_RESIZE_LDS_BYTES) --tr;
  const int64_t lds = band_bytes(tr);
  if (lds > EVT_RESIZE_LDS_BYTES)
    return fail(EVT_EINVAL, "resize_plan_create: one output row's " + std::to_string(g.ksv) +
                                " vertical taps of " + std::to_string(lp) + " bytes exceed the " +
                                std::to_string(EVT_RESIZE_LDS_BYTES) + "-byte LDS band (reduce "
                                "the image first)");
  evt_resize_plan* p = new (std::nothrow) evt_resize_plan{};
  if (!p) return fail(EVT_ENOMEM, "resize_plan_create: host allocation failed");
  p->in_h = in_h; p->in_w = in_w; p->C = C; p->S = S; p->tr = tr;
  p->nbands = (S + tr - 1) / tr; p->lds = (size_t)lds; p->g = g;
  hipError_t e = hipMalloc((void**)&p->tab, ntab * sizeof(int32_t));
  if (e == hipSuccess) {
    e = hipMemcpy(p->tab, tab.data(), ntab * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) (void)hipFree(p->tab);
  }
  if (e != hipSuccess) {
    delete p;
    return hip_fail(e, "resize_plan_create");
  }
  p->magic = RESIZE_MAGIC;
  *out = p;
  return EVT_OK;
}

int evt_resize_plan_destroy(evt_resize_plan* p) {
  if (!p) return EVT_OK;
  if (p->magic != RESIZE_MAGIC) return fail(EVT_EINVAL, "resize_plan_destroy: not a live plan");
  p->magic = 0;
  const hipError_t e = hipFree(p->tab);
  delete p;
  if (e != hipSuccess) return hip_fail(e, "resize_plan_destroy");
  return EVT_OK;
}

int evt_resize_crop_u8(const evt_resize_item* items, int batch, int channels, int crop,
                       uint8_t* out, void* stream) {
  if (!items || !out) return fail(EVT_EINVAL, "resize_crop_u8: items and out must be non-null");
  if (batch < 0) return fail(EVT_EINVAL, "resize_crop_u8: batch must not be negative");
  if (channels < 1 || channels > 4)
    return fail(EVT_EINVAL, "resize_crop_u8: uint8 images have 1 to 4 channels");
  if (crop < 1 || ((int64_t)crop * channels) % 4)
    return fail(EVT_EINVAL, "resize_crop_u8: crop*channels must be a positive multiple of 4");
  if ((uintptr_t)out & 15) return fail(EVT_EINVAL, "resize_crop_u8: out must be 16-byte aligned");
  for (int b = 0; b < batch; ++b) {
    const evt_resize_item& it = items[b];
    const std::string at = "resize_crop_u8: item " + std::to_string(b);
    if (!it.src || !it.plan) return fail(EVT_EINVAL, at + ": src and plan must be non-null");
    if (it.plan->magic != RESIZE_MAGIC) return fail(EVT_EINVAL, at + ": not a live plan");
    if (it.plan->C != channels)
      return fail(EVT_EINVAL, at + ": the plan has " + std::to_string(it.plan->C) +
                                  " channels, the call " + std::to_string(channels));
    if (it.plan->S != crop)
      return fail(EVT_EINVAL, at + ": the plan's crop is " + std::to_string(it.plan->S) +
                                  ", the call's " + std::to_string(crop));
    if (it.pitch < (int64_t)it.plan->in_w * channels)
      return fail(EVT_EINVAL, at + ": pitch " + std::to_string(it.pitch) + " is less than " +
                                  std::to_string((int64_t)it.plan->in_w * channels) +
                                  " bytes (width*channels)");
  }
  const int64_t per_image = (int64_t)crop * crop * channels;
  for (int b0 = 0; b0 < batch; b0 += RESIZE_CHUNK) {
    ResizeArgs a{};
    a.out = out + (int64_t)b0 * per_image;
    a.S = crop;
    a.n = std::min(RESIZE_CHUNK, batch - b0);
    int blocks = 0;
    size_t lds = 0;
    for (int i = 0; i < a.n; ++i) {
      const evt_resize_item& it = items[b0 + i];
      a.d[i] = ResizeDesc{it.src, it.pitch, it.plan->tab, it.plan->g.ksh, it.plan->g.ksv,
                          it.plan->tr, blocks};
      blocks += it.plan->nbands;
      lds = std::max(lds, it.plan->lds);
    }
    EVT_HIP(resize_crop_launch(a, channels, blocks, lds, (hipStream_t)stream), "resize_crop_u8");
  }
  return EVT_OK;
}

}  // extern "C"
