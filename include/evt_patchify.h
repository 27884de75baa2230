/* Companion of evt.h (which includes it): entry points added after evt.h's own list was fixed.
 * Same conventions: C ABI of libevt_hip.so, EVT_* return codes, evt_last_error() for the text. */
#ifndef EVT_PATCHIFY_H_
#define EVT_PATCHIFY_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* evt_patchify_cm for any patch size, at a row stride: out [B*P, ldo] (dtype) with
 *   out[patch][k] = img[b][c][h*ps + p1][w*ps + p2],  k = (c*ps + p1)*ps + p2 < ps*ps*C
 * (channel-major (c p1 p2), the K order of evt_patchify_cm: element (p1 p2 c) of the reference
 * vector is at k = c*ps*ps + p1*ps + p2) and out[patch][k] = 0 for ps*ps*C <= k < ldo, written
 * on every call (the model's patch matrix shares a buffer with the FFN activations, and its GEMM
 * reads whole 64-column K-tiles: patch 14 has 588 columns at ldo = 640). CLS row and statistics
 * as evt_patchify. ldo >= ps*ps*C, ldo % 8 == 0, HW % ps == 0, ps*HW % 4 == 0,
 * C*ps*HW*4 <= 160 KiB, out 16-byte aligned; anything else is EVT_EINVAL before any launch. */
int evt_patchify_ld(int dtype, const float* img, int B, int C, int HW, int ps, void* out,
                    int64_t ldo, void* x, const float* cls, const float* pos, int D, float* stats,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVT_PATCHIFY_H_ */
