/* Companion of evt.h (which includes it): per-head attention statistics of a model handle. Same
 * conventions as evt.h: C ABI of libevt_hip.so, EVT_* return codes, evt_last_error() for the text.
 *
 * The attention maps (evt_attention_maps.h) are [batch, H, T, T] floats per block. What a pruning
 * or analysis pass wants of them is four numbers per head; evt_forward_head_stats forms them on the
 * device from the same probabilities, without storing a map.
 *
 * For a block with H heads and T tokens per image let p[b,h,i,j] be the value evt_attention_maps.h
 * defines: softmax_j(q_i . k_j * h_k^-0.5) of the stored q and k, scores, statistics and
 * normalisation in fp32. With `prefix` leading non-patch tokens and a patch grid of `grid_w`
 * columns, patch token t >= prefix sits at row (t - prefix) / grid_w, column (t - prefix) % grid_w.
 * The output of a block is stats[b][h][0..3], fp32, contiguous [batch, H, EVT_HEAD_STATS]:
 *
 *   EVT_HEAD_CONFIDENCE  mean over all T queries of max_j p_ij
 *   EVT_HEAD_ENTROPY     mean over all T queries of -sum_j p_ij ln p_ij (nats, 0 ln 0 = 0)
 *   EVT_HEAD_DISTANCE    mean over patch queries i >= prefix of sum_{j >= prefix} p_ij d(i, j), d the
 *                        Euclidean distance in patch units; the probabilities are not renormalised
 *   EVT_HEAD_CLS_MASS    mean over patch queries of sum_{j < prefix} p_ij (0 when prefix == 0)
 *
 * Every value is finite; confidence is in (0, 1], entropy >= 0 (at most ln T up to rounding),
 * distance >= 0, cls_mass in [0, 1]. A (b, h) result is bitwise reproducible, does not depend on
 * the image's position in the batch, and is bitwise equal for the token-major and the head-major
 * QKV layout (evt_model_qkv_layout): one workgroup reduces an (image, head) in a fixed order, with
 * no atomics and no scratch memory.
 *
 * Families: those of evt_forward_attention (ViT, pruned or not, and T2T-ViT). Swin and an
 * EVT_DTYPE_MX8 handle are EVT_EINVAL.
 *
 * The forward is evt_forward_attention's: logits, pooled, tokens and taps (through `feat`) are
 * bitwise those of evt_forward_features; the statistics of block i are one more launch right after
 * the block's attention kernel (the last block included: its QKV GEMM stores every row's q and k
 * while its attention runs on the CLS rows). A handle with lanes runs the call as one lane. The
 * call only enqueues kernels on `stream`: no allocation, no synchronisation. With
 * evt_model_profile on, the launches count under EVT_PROF_HEAD. evt_graph_capture stays
 * logits-only. */
#ifndef EVT_HEAD_STATS_H_
#define EVT_HEAD_STATS_H_
#include <stdint.h>

#include "evt_image.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EVT_HEAD_STATS 4
#define EVT_HEAD_CONFIDENCE 0
#define EVT_HEAD_ENTROPY 1
#define EVT_HEAD_DISTANCE 2
#define EVT_HEAD_CLS_MASS 3

typedef struct evt_head_stats_args {
  int32_t n_blocks;          /* 0..64 */
  const int32_t* blocks;     /* [n_blocks] block indices, strictly increasing (host memory) */
  float* const* stats;       /* [n_blocks] device pointers (host array), 16-byte aligned */
} evt_head_stats_args;

/* Heads of block `block` (0 <= block < depth), tokens per image, and the geometry the distances
 * use: prefix = 1 (the CLS token), grid_w = image_size / patch_size (ViT) or image_size / 16
 * (T2T-ViT). EVT_EINVAL: a NULL argument, a block out of range, a Swin or EVT_DTYPE_MX8 handle. */
int evt_head_stats_shape(const evt_model* m, int block, int* heads, int* tokens, int* prefix,
                         int* grid_w);

/* One forward of the images `in` that writes the statistics of `hs` and, when `feat` is non-NULL,
 * the outputs of `feat` as evt_forward_features does. With feat == NULL no classifier head runs.
 * EVT_EINVAL before any launch (nothing written): a NULL model, in or hs; a Swin or EVT_DTYPE_MX8
 * handle; n_blocks outside [0, 64]; n_blocks == 0 with feat == NULL; n_blocks > 0 with a NULL
 * array or a NULL stats pointer; a block out of range or blocks not strictly increasing; a stats
 * pointer that is not 16-byte aligned; everything evt_forward_image rejects of (in, batch, feat). */
int evt_forward_head_stats(evt_model* m, const evt_image_args* in, int batch,
                           const evt_features_args* feat, const evt_head_stats_args* hs,
                           void* stream);

/* Op level (the parity tests): out[b][h][0..3] of the q and k in qkv, with the arguments and layout
 * rules of evt_attention_probs (both layouts of the same values give bitwise equal results;
 * N <= 4096, head_dim in [1, 128], scale positive and finite, out 16-byte aligned), and
 * 0 <= prefix < N, grid_w >= 1, (N - prefix) % grid_w == 0 (a rectangular grid is fine). */
int evt_attention_head_stats(int dtype, const void* qkv, int64_t ldq, int64_t sb, int64_t sh,
                             int ko, int B, int N, int H, int head_dim, float scale, int prefix,
                             int grid_w, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVT_HEAD_STATS_H_ */
