/* Companion of evt.h (which includes it): diagnostic entry points of the tokens-to-token stage.
 * Same conventions: C ABI of libevt_hip.so, EVT_* return codes, evt_last_error() for the text.
 * They reach, at op level, the two things of the T2T-ViT model's bf16 path that evt_performer does
 * not: the permuted kqv columns with the per-token statistics, and the gather of those statistics
 * into the LayerNorm statistics of the next soft split (tests/test_gpu_performer_probes.py). */
#ifndef EVT_PERFORMER_H_
#define EVT_PERFORMER_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* evt_performer with the model's two extras, handed to the same launcher unchanged:
 *   kqv_perm  non-zero: within each of the k, q and v blocks, feature f sits at column
 *             16 * ((f >> 2) & 3) + 4 * (f >> 4) + (f & 3), the order the model's kqv Dense
 *             writes (every lane's 16 features as two 16-byte pieces). Needs ldq % 8 == 0 and a
 *             16-byte aligned kqv.
 *   tstats    [B*T][2] fp32 or NULL: (sum, sum of squares) of every token's 64 stored outputs.
 * Both are bf16 only: EVT_EINVAL with EVT_DTYPE_F32. `out` is bitwise the same with and without
 * either (the permutation applied to the input). Everything else as evt_performer. */
int evt_performer_ex(int dtype, const void* kqv, int64_t ldq, int B, int T, const float* w,
                     const float* out_w, const float* out_b, const float* ln2_g,
                     const float* ln2_b, const float* fc1_w, const float* fc1_b,
                     const float* fc2_w, const float* fc2_b, float* part, void* out, int64_t ldo,
                     int kqv_perm, float* tstats, void* stream);

/* Row statistics of the soft split (k 3, stride 2, pad 1) of an R x R token map from per-token
 * statistics: tstats [B*R*R][2] -> dst [B*OW*OW][nslots][2], OW = (R + 1) / 2. Slot 0 of row
 * (b, y, x) is the sum of the (sum, sumsq) of its <= 9 source tokens (2y - 1 + kh, 2x - 1 + kw)
 * inside the map, the other slots are zeroed. */
int evt_unfold_stats(const float* tstats, int B, int R, float* dst, int nslots, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVT_PERFORMER_H_ */
