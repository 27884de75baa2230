/* Companion of evt.h (which includes it): the uint8 eval transform on the device. Same conventions
 * as evt.h: C ABI of libevt_hip.so, EVT_* return codes, evt_last_error() for the text.
 *
 * The reference's accuracy path (utils.py:593-607, build_eval_transform) is
 * Resize(int(256/224*S), interpolation=3), CenterCrop(S), ToTensor, Normalize. evt_image.h does the
 * last two inside the forward's first kernel; this header does the first two, on decoded uint8
 * images of any size, and writes the dense uint8 NHWC batch evt_forward_image takes. The result is
 * bitwise what Pillow's Image.resize followed by the crop produces (Pillow resamples 8-bit images
 * in integer arithmetic, so the contract below is exact and not an approximation of it).
 *
 *   input     B uint8 interleaved HWC images, each with its own device pointer, height, width and
 *             row pitch in bytes (pitch >= W*C); C channels, 1 to 4, one value per call. No
 *             alignment is asked of a pointer or pitch (a sub-tensor view of a decoder's buffer
 *             works): the kernel loads single bytes and touches no byte outside the image rows.
 *             Each channel is resampled on its own (no alpha premultiplication).
 *   geometry  torchvision's Resize(R) + CenterCrop(S): the short side becomes R,
 *               w <= h:  ow = R, oh = (int)(R*h / w)      else  oh = R, ow = (int)(R*w / h)
 *             (the quotient in fp64, truncated), then the S x S window at
 *               top = round_half_even((oh - S) / 2), left = round_half_even((ow - S) / 2).
 *             oh >= S and ow >= S are required (torchvision would pad): EVT_EINVAL otherwise.
 *             resize_short == 0 asks for the reference's default R = (int)((256.0 / 224.0) * S).
 *   resample  for each axis whose output size differs from its input size, horizontal first, then
 *             vertical on the horizontal pass's uint8 result. With in / out the axis sizes:
 *               scale = in / out, fs = max(scale, 1), support = fsup * fs
 *               center = (xx + 0.5) * scale
 *               xmin = max((int)(center - support + 0.5), 0)
 *               xmax = min((int)(center + support + 0.5), in),  n = xmax - xmin
 *               w[x] = f((x + xmin - center + 0.5) * (1 / fs)),  x = 0 .. n-1
 *             the weights are summed in index order from 0.0 and, if the sum is non-zero, each is
 *             divided by it; kk[x] = (int)(w * 2^22 + 0.5) for w >= 0, (int)(w * 2^22 - 0.5) for
 *             w < 0 ((int) truncates towards zero). All of that in fp64 without fused multiply-add.
 *               byte = clamp((2^21 + sum_x pixel[xmin + x] * kk[x]) >> 22, 0, 255)
 *             with an int32 accumulator and an arithmetic shift.
 *             EVT_RESIZE_BICUBIC (fsup 2, a = -0.5): ((a+2)x - (a+3))x^2 + 1 for |x| < 1,
 *             (((x-5)x + 8)x - 4)a for 1 <= |x| < 2, else 0. EVT_RESIZE_BILINEAR (fsup 1): 1 - |x|
 *             for |x| < 1, else 0. An axis whose size does not change gets no pass (its tables are
 *             an exact identity, which is what the kernel applies).
 *   output    dense uint8 NHWC [B, S, S, C], 16-byte aligned, S*C % 4 == 0 (the uint8 readers' own
 *             rule): exactly the `data` of an evt_image_args. Not normalised.
 *
 * The tables (tap bounds and kk of both axes, for the S columns and S rows of the crop window only)
 * are computed on the host at plan creation and uploaded once; the kernel does integer work only,
 * so its output is a pure function of the tables and the bytes. |kk| < 2^23 is asserted at plan
 * creation (24-bit multiplies).
 *
 * Limits (EVT_EINVAL, never a wrong answer): input sides and R at most EVT_RESIZE_MAX_SIDE; the
 * uint8 rows one output row's vertical taps read must fit the kernel's LDS band,
 *   ksize_v * round_up(S*C, 16) <= EVT_RESIZE_LDS_BYTES
 * (ksize_v = 2*ceil(support_v) + 1 as evt_resize_geometry reports it: 224 x 3 takes a vertical
 * reduction of 24x in bicubic). */
#ifndef EVT_PREPROCESS_H_
#define EVT_PREPROCESS_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EVT_RESIZE_BILINEAR 2      /* Pillow's / the reference's interpolation codes */
#define EVT_RESIZE_BICUBIC  3
#define EVT_RESIZE_MAX_SIDE  32768
#define EVT_RESIZE_LDS_BYTES 65536
#define EVT_RESIZE_CHUNK     64    /* images per kernel launch of evt_resize_crop_u8 */

typedef struct evt_resize_plan evt_resize_plan;

typedef struct evt_resize_item {
  const uint8_t* src;            /* device pointer to pixel (0, 0) */
  int64_t pitch;                 /* bytes between rows, >= in_w * channels */
  const evt_resize_plan* plan;   /* of this image's (in_h, in_w) */
} evt_resize_item;

/* The geometry of one image size; host only, no device needed. Any output pointer may be NULL.
 * ksize_h / ksize_v: the table width of each axis, 2*ceil(support) + 1 (an upper bound of n).
 * EVT_EINVAL: a size < 1 or > EVT_RESIZE_MAX_SIDE, resize_short < 0, an unknown filter,
 * oh < crop or ow < crop. */
int evt_resize_geometry(int in_h, int in_w, int resize_short, int crop, int filter, int* oh,
                        int* ow, int* top, int* left, int* ksize_h, int* ksize_v);
/* The tables of one axis for output indices first .. first+count-1; host only. bounds[2*i] = xmin,
 * bounds[2*i + 1] = n; kk[i*ksize + x], zero past n; ksize = 2*ceil(support) + 1.
 * EVT_EINVAL: NULLs, sizes < 1 or > EVT_RESIZE_MAX_SIDE, a window outside [0, out_size], an
 * unknown filter. */
int evt_resize_coefficients(int in_size, int out_size, int first, int count, int filter,
                            int32_t* bounds, int32_t* kk);

/* A plan holds the tables of one (in_h, in_w, channels, resize_short, crop, filter) in one device
 * allocation on the current device. It is immutable: share it between calls and streams; destroy
 * it once no launch that uses it is still running. EVT_EINVAL: what evt_resize_geometry rejects,
 * channels outside 1..4, crop*channels % 4 != 0, the LDS limit above, out == NULL. */
int evt_resize_plan_create(int in_h, int in_w, int channels, int resize_short, int crop,
                           int filter, evt_resize_plan** out);
int evt_resize_plan_destroy(evt_resize_plan* plan);

/* out[b] = crop(resize(items[b])), b < batch. `items` is a HOST array, read before the call
 * returns; images of different sizes mix freely. No allocation, copy or synchronisation: the
 * per-image descriptors travel by value in the kernel arguments, EVT_RESIZE_CHUNK images per
 * launch, so the call can be captured in a HIP graph. A workgroup takes one image and a band of
 * output rows; the band height is the plan's (at most 16 rows, fewer at large vertical reductions).
 * EVT_EINVAL before any launch: items or out NULL; batch < 0; channels outside 1..4; an item with a
 * NULL src or plan, a plan of other channels or another crop, pitch < in_w*channels; out not
 * 16-byte aligned. */
int evt_resize_crop_u8(const evt_resize_item* items, int batch, int channels, int crop,
                       uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVT_PREPROCESS_H_ */
