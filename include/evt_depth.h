/* Companion of evt.h (which includes it): the depth axis of a ViT handle. How much each attention
 * and FFN sublayer changes the token stream, measured on the device, and a runtime switch that
 * leaves chosen sublayers out of the forward. Same conventions as evt.h: C ABI of libevt_hip.so,
 * EVT_* return codes, evt_last_error() for the text.
 *
 * Statistics. For a sublayer with input rows a[b,t,:] and output rows b[b,t,:] (the token stream as
 * stored in the model dtype, T tokens per image, D wide), everything in fp32:
 *
 *   EVT_DEPTH_COSINE      mean_t  a_t . b_t / max(|a_t| |b_t|, FLT_MIN)
 *   EVT_DEPTH_REL_UPDATE  mean_t  |b_t - a_t| / max(|a_t|, FLT_MIN)   (the difference element by
 *                         element, never from the dot products: that cancels for a small update)
 *   EVT_DEPTH_NORM_RATIO  mean_t  |b_t| / max(|a_t|, FLT_MIN)
 *   EVT_DEPTH_CLS_COSINE  the cosine of token 0 alone
 *
 * b = a gives exactly (1, 0, 1, 1) and b = -a exactly (-1, 2, 1, -1). A zero row of a is held
 * finite by the FLT_MIN clamp as long as |b_t| / FLT_MIN is (|b_t| < 4); above that the two ratios
 * of the image are +inf. A result is bitwise reproducible and does not depend on the image's
 * position in the batch or on the batch size: the order of every sum is fixed by (T, D), with no
 * floating-point atomics (depth_stats.hip).
 *
 * evt_forward_block_stats writes, per requested block, stats[b][s][0..3], fp32 contiguous
 * [batch, 2, EVT_DEPTH_STATS], s = EVT_DEPTH_ATTN: the attention sublayer (the block's input
 * against the out-projection's output), s = EVT_DEPTH_FFN: the FFN sublayer (that against FC2's
 * output). Both operands are resident when the launch runs, so nothing is stashed and the workspace
 * does not grow; the per-chunk partials of the reduction live in the FFN hidden buffer, idle at both
 * points. The forward is evt_forward_features': logits, pooled, tokens and taps (through `feat`)
 * are bitwise those of evt_forward_features. Asking for the last block runs its full-row launches
 * beside the CLS tail (evt_tail.h), exactly as evt_forward_ffn_stats does; the statistics are those
 * of the full-row launches, the CLS rows the head reads stay the tail's. A handle with lanes runs
 * the call as one lane. The launches count under EVT_PROF_HEAD. evt_graph_capture stays
 * logits-only. A skipped sublayer (below) reports (1, 0, 1, 1) without a kernel launch. Refused
 * (EVT_EINVAL) while a token schedule is set, and on T2T-ViT, Swin and EVT_DTYPE_MX8 handles.
 *
 * Skips. evt_model_set_skips takes one byte per block: EVT_SKIP_ATTN leaves the block's attention
 * sublayer out, EVT_SKIP_FFN its FFN sublayer, both the whole block. A skipped sublayer is absent:
 * the stream passes through unchanged, its LayerNorm goes with it (for EVT_VIT_REFERENCE, whose
 * residual is LN(x), that is not what zero gates give), and none of its kernels is launched (QKV,
 * attention and out-projection; FC1 and FC2; the last block's tail launches included). A model with
 * blocks S skipped whole is bitwise a fresh model created from the parameters without the layers
 * S: the CLS tail moves to the last block that still runs. Head and FFN gates of a skipped
 * sublayer are kept and act again once the skip is cleared. evt_model_profile_work counts what
 * runs.
 *
 * A set is refused (EVT_EINVAL, nothing changed) on T2T-ViT, Swin and EVT_DTYPE_MX8 handles, on a
 * lane child, for a mask that skips every block, while `stream` is capturing, and on a handle
 * with a captured graph: as for a token schedule, the graph would be stale, so set the skips
 * before evt_graph_capture. It is refused too
 * when the handle's token schedule names a block whose attention would be skipped or that would
 * be the last block that runs (or a later one). While skips are set, evt_forward_attention,
 * evt_forward_head_stats and evt_forward_rollout refuse a block whose attention is skipped,
 * evt_forward_ffn_stats a block whose FFN is skipped, and evt_model_set_token_schedule an entry
 * as above. Taps and tokens work: a skipped block's tap is its input. Lanes carry the mask. */
#ifndef EVT_DEPTH_H_
#define EVT_DEPTH_H_
#include <stdint.h>

#include "evt_image.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EVT_DEPTH_STATS 4
#define EVT_DEPTH_COSINE 0
#define EVT_DEPTH_REL_UPDATE 1
#define EVT_DEPTH_NORM_RATIO 2
#define EVT_DEPTH_CLS_COSINE 3
#define EVT_DEPTH_ATTN 0
#define EVT_DEPTH_FFN 1
#define EVT_DEPTH_MAX_TOKENS 4096 /* tokens per image of the op-level entry point */
#define EVT_SKIP_ATTN 1
#define EVT_SKIP_FFN 2

typedef struct evt_block_stats_args {
  int32_t n_blocks;          /* 0..64 */
  const int32_t* blocks;     /* [n_blocks] block indices, strictly increasing (host memory) */
  float* const* stats;       /* [n_blocks] device pointers (host array), 16-byte aligned */
} evt_block_stats_args;

/* Sublayers per block (2), statistics per sublayer (4) and tokens per image of block `block`
 * (0 <= block < depth). EVT_EINVAL: a NULL argument, a block out of range, a T2T-ViT, Swin or
 * EVT_DTYPE_MX8 handle. */
int evt_block_stats_shape(const evt_model* m, int block, int* sublayers, int* stats, int* tokens);

/* One forward of the images `in` that writes the statistics of `bs` and, when `feat` is non-NULL,
 * the outputs of `feat` as evt_forward_features does. With feat == NULL no classifier head runs.
 * EVT_EINVAL before any launch (nothing written): a NULL model, in or bs; a family or dtype without
 * the statistics; a token schedule set; n_blocks outside [0, 64]; n_blocks == 0 with feat == NULL;
 * n_blocks > 0 with a NULL array or a NULL stats pointer; a block out of range or blocks not
 * strictly increasing; a stats pointer that is not 16-byte aligned; everything evt_forward_image
 * rejects of (in, batch, feat). */
int evt_forward_block_stats(evt_model* m, const evt_image_args* in, int batch,
                            const evt_features_args* feat, const evt_block_stats_args* bs,
                            void* stream);

/* Op level (the parity tests): out[b][0..3] of the row-major matrices a and b of B * T rows of D
 * elements with pitches of lda / ldb elements. dtype EVT_DTYPE_BF16 or EVT_DTYPE_F32. EVT_EINVAL
 * with a message: B < 1; T < 1 or > EVT_DEPTH_MAX_TOKENS; D < 8 or not a multiple of 8; a pitch
 * below D or not a multiple of 16 bytes; a, b or out NULL or not 16-byte aligned. For T > 16 the
 * call takes B * ceil(T / 16) * 16 bytes from the stream's memory pool for the partial sums and
 * gives them back, stream-ordered. */
int evt_stream_delta_stats(int dtype, const void* a, int64_t lda, const void* b, int64_t ldb,
                           int B, int T, int D, float* out, void* stream);

/* Skip mask of the handle: mask[i] (bits EVT_SKIP_ATTN | EVT_SKIP_FFN) for block i, depth = the
 * model's block count; mask == NULL (depth ignored) clears. Forwards enqueued later see it. See the
 * head of this file for what is refused. */
int evt_model_set_skips(evt_model* m, const uint8_t* mask, int depth, void* stream);

/* *depth = the model's block count; mask[i] for i < min(depth, cap) when mask is non-NULL (all 0
 * with no skips set). */
int evt_model_get_skips(const evt_model* m, uint8_t* mask, int cap, int* depth);

#ifdef __cplusplus
}
#endif
#endif /* EVT_DEPTH_H_ */
