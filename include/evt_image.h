/* Companion of evt.h (which includes it): uint8 image input. Same conventions as evt.h: C ABI of
 * libevt_hip.so, EVT_* return codes, evt_last_error() for the text.
 *
 * evt_*_forward take normalised fp32 images. A decoder, PIL / OpenCV or a data loader deliver
 * uint8, interleaved HWC; with EVT_IMG_U8_NHWC the first kernel of every family reads those bytes
 * itself and normalises them on the way in:
 *
 *   layout  uint8, dense [batch, S, S, in_chans], in_chans <= 4, for every family (ViT and Swin
 *           too, whose fp32 input is NCHW); planar uint8 and strided views are not taken
 *   value   v = fmaf((float)u, scale[c], shift[c]) in fp32, one rounding; then the conversion the
 *           fp32 path applies (bf16 round-to-nearest-even for bf16 and MX8 handles)
 *   host    scale[c] = 1 / (255 std[c]), shift[c] = -mean[c] / std[c], computed in fp64 and
 *           rounded once to fp32, gives the usual Normalize(mean, std) of u / 255
 *   padding T2T soft-split padding, K-padding columns and row tails are 0 after normalisation,
 *           as on the fp32 path (not shift[c])
 *
 * The kernels deposit the same fp32 values the fp32 loaders would read, and everything after is
 * the same code: a uint8 forward is bitwise the fp32 forward of the image
 * float(double(u) * scale[c] + shift[c]) in the family's native layout (for constants of ordinary
 * magnitude that double expression is exact, so its rounding is the fmaf's). scale and shift
 * travel by value in the kernel arguments: no allocation, no copy, no synchronisation, and the
 * call can be captured in a HIP graph. */
#ifndef EVT_IMAGE_H_
#define EVT_IMAGE_H_
#include <stdint.h>

#include "evt_features.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EVT_IMG_F32     0   /* the family's native fp32 layout, as evt_*_forward */
#define EVT_IMG_U8_NHWC 1

typedef struct evt_image_args {
  const void* data;                  /* device pointer; EVT_IMG_U8_NHWC: 4-byte aligned (the fused
                                      * Swin stem, embed_dim 96 / patch 4 in bf16: 16-byte) */
  int32_t format;                    /* EVT_IMG_* */
  float scale[4], shift[4];          /* EVT_IMG_U8_NHWC: per channel, finite */
} evt_image_args;

/* One forward of any family. `out` is as evt_forward_features (logits alone is allowed, and then
 * the batch runs over the handle's lanes like evt_*_forward; with pooled, tokens or taps it runs
 * as one lane). EVT_IMG_F32 routes to evt_*_forward / evt_forward_features. The logits are bitwise
 * those of evt_*_forward on the normalised fp32 image. With evt_model_profile on, the uint8
 * readers report under the roles of their fp32 counterparts (1 byte per input element).
 * EVT_EINVAL before any launch: a NULL in, out, data or model; an unknown format; a model with
 * in_chans > 4; a non-finite scale or shift among the first in_chans; patch_size*S*in_chans % 4
 * != 0 (ViT, Swin); a ViT whose patch vectors are not channel-major (patch_size % 8 != 0 with
 * patch_size^2*in_chans % 64 == 0); misaligned data; batch outside [1, max_batch]; everything
 * evt_forward_features rejects. */
int evt_forward_image(evt_model* m, const evt_image_args* in, int batch,
                      const evt_features_args* out, void* stream);
/* evt_graph_capture with an image descriptor; replay with evt_graph_launch after refilling the
 * bytes at in->data in place. */
int evt_graph_capture_image(evt_model* m, const evt_image_args* in, int batch, float* logits,
                            void* stream);

/* Op level (the parity tests). evt_patchify_ld (evt_patchify.h) from uint8 NHWC img [B, HW, HW, C]:
 * the same out, CLS rows and stats bytes as evt_patchify_ld on the normalised NCHW image (and as
 * evt_patchify_cm when ldo == ps*ps*C). scale / shift: C floats each in host memory, finite.
 * EVT_EINVAL: what evt_patchify_ld rejects, C > 4, ps*HW*C % 4 != 0, img not 4-byte aligned. */
int evt_patchify_u8(int dtype, const uint8_t* img, int B, int C, int HW, int ps, void* out,
                    int64_t ldo, void* x, const float* cls, const float* pos, int D, float* stats,
                    const float* scale, const float* shift, void* stream);
/* evt_unfold(dtype, in_f32 = 1, ...) from a uint8 NHWC image [B, H, W, C], C <= 4: the same rows
 * and statistics bytes as evt_unfold on the normalised fp32 image, padding 0. */
int evt_unfold_u8(int dtype, const uint8_t* in, int B, int H, int W, int C, int k, int stride,
                  int pad, void* out, int ldo, float* stats, int nslots, const float* scale,
                  const float* shift, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVT_IMAGE_H_ */
