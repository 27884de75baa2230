/* Companion of evt.h (which includes it): token pruning of a ViT handle. Same conventions as
 * evt.h: C ABI of libevt_hip.so, EVT_* return codes, evt_last_error() for the text.
 *
 * The third axis along which a ViT shrinks, after heads and FFN neurons, and the only one that
 * needs no new checkpoint: between encoder blocks the stream drops the patch tokens the CLS token
 * attends to least (the CLS-attention score of EViT, Liang et al. 2022, and of its baselines), and
 * every later block, the CLS tail and the head run on fewer rows. It is opt-in: a handle without a
 * schedule runs exactly what it ran before.
 *
 * A TOKEN SCHEDULE is a list of (block l, K_l), the blocks strictly ascending with
 * 0 <= l < depth - 1. After block l the stream keeps the CLS token and K_l of its T_l - 1 patch
 * tokens: T_{l+1} = 1 + K_l, 1 <= K_l <= T_l - 1 (T_0 = the model's tokens per image). For each
 * scheduled block, after its FC2:
 *
 *   1. Score.   score[b, j] = sum_h p_l[b, h, 0, j], with p_l the probability
 *               evt_attention_maps.h defines (scores, statistics and normalisation in fp32, of the
 *               q and k the block stored). The heads are added in index order in fp32 and the sum
 *               is not divided (only the order matters): bitwise the head-ordered fp32 sum of the
 *               CLS rows evt_forward_attention exports. fp32 [B, T_l]; entry 0 is the CLS token's
 *               attention to itself and takes no part in the selection.
 *   2. Select.  The K_l patch tokens (j >= 1) with the largest score are kept. Ties, and -0.0
 *               against +0.0, go to the lower index; NaN comes last: the order of
 *               np.argsort(-s, kind="stable"), which evt_classify.h documents too.
 *               kept[b, 0] = 0, then the chosen positions ASCENDING (raster order is preserved).
 *               int32 [B, 1 + K_l] in the block's own numbering 0 .. T_l - 1.
 *   3. Gather.  Rows kept[b, :] of the block's output stream are packed to [B (1 + K_l), D],
 *               image b at row b (1 + K_l), and their LayerNorm row statistics move with them: a
 *               bitwise copy into the stream buffer that is idle at block end, whose role the two
 *               then swap (an in-place gather would race between images).
 *
 * The FFN acts per token, so selecting after FC2 gives the kept tokens exactly the values EViT's
 * placement (after the attention, before the FFN) gives them; the cost is block l's FFN on the
 * rows that are dropped. EViT's fused "inattentive" token is not formed (a follow-up: it needs row
 * statistics of a synthesised row).
 *
 * Three launches per scheduled block (scores, select, gather), counted under EVT_PROF_HEAD. The
 * workspace does not grow: scores and kept live in the FFN hidden buffer, idle at block end. The
 * forward allocates nothing and does not synchronise. Results are bitwise reproducible, do not
 * depend on the image's position in the batch, and are equal between the head-major and the
 * token-major QKV layout and over lanes.
 *
 * With a schedule set, the plain forward (evt_vit_forward), evt_forward_image,
 * evt_forward_classify, graph capture / replay and profiling run the scheduled forward, and
 * evt_forward_features still gives logits and pooled. What reads all T tokens of a block returns
 * EVT_EINVAL with a message that names the schedule: evt_forward_attention,
 * evt_forward_head_stats, evt_forward_rollout, evt_forward_ffn_stats, and the tokens / taps of a
 * features forward. Clear the schedule (n = 0) to use them.
 *
 * Families: ViT (reference and standard, pruned or not) in f32 and bf16. Swin, T2T-ViT (its shared
 * encoder is a follow-up) and EVT_DTYPE_MX8 handles are EVT_EINVAL. */
#ifndef EVT_TOKEN_PRUNING_H_
#define EVT_TOKEN_PRUNING_H_
#include <stddef.h>
#include <stdint.h>

#include "evt_image.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EVT_TOKEN_SCHEDULE_MAX 64 /* most entries of a schedule */

/* Outputs of evt_forward_token_pruning, one entry per scheduled block in schedule order. Either
 * array may be NULL, and so may any entry: that output is then not exported. */
typedef struct evt_token_pruning_args {
  int32_t n_blocks;        /* entries of the arrays: the schedule's length */
  float* const* scores;    /* [n_blocks] device, 4-byte aligned: fp32 [batch, T_l] */
  int32_t* const* kept;    /* [n_blocks] device, 4-byte aligned: int32 [batch, 1 + K_l] */
} evt_token_pruning_args;

/* Set (n > 0) or clear (n == 0) the handle's schedule: keep[i] patch tokens after block blocks[i].
 * It may synchronise the device, like evt_model_set_lanes; it reaches the handle's lanes, and lanes
 * set later inherit it. `stream` is reserved (nothing is enqueued today). EVT_EINVAL: a NULL
 * model; a captured graph ("set the schedule before capture"); a Swin, T2T-ViT or EVT_DTYPE_MX8
 * handle; n outside [0, EVT_TOKEN_SCHEDULE_MAX]; NULL arrays with n > 0; blocks not strictly
 * ascending; a block outside [0, depth - 1); a keep outside [1, T_l - 1]. On an error the
 * schedule is unchanged. */
int evt_model_set_token_schedule(evt_model* m, int n, const int32_t* blocks, const int32_t* keep,
                                 void* stream);

/* The schedule: *n entries; blocks / keep (each may be NULL) receive up to `cap` of them. Host
 * only. EVT_EINVAL: a NULL model or n, cap < 0. */
int evt_model_token_schedule(const evt_model* m, int* n, int32_t* blocks, int32_t* keep, int cap);

/* Tokens per image T_l that block `block` runs on under the schedule (the model's own count
 * without one). Host only. EVT_EINVAL: a NULL argument, a Swin or T2T-ViT handle, block outside
 * [0, depth). */
int evt_model_tokens_at(const evt_model* m, int block, int* tokens);

/* The scheduled forward of the images `in` that also exports, per scheduled block, its scores and
 * kept table (tp; NULL: none), and the outputs of `feat` as evt_forward_features does: logits and
 * pooled only. A handle with lanes runs the call as one lane. EVT_EINVAL before any launch: a NULL
 * model, in or feat; no schedule set; tp->n_blocks != the schedule's length; a misaligned export
 * pointer; feat->tokens or taps; everything evt_forward_image rejects of (in, batch, feat). */
int evt_forward_token_pruning(evt_model* m, const evt_image_args* in, int batch,
                              const evt_features_args* feat, const evt_token_pruning_args* tp,
                              void* stream);

/* Op level (the parity tests). evt_token_scores: step 1 for one block; the arguments and layout
 * rules are those of evt_attention_probs (both layouts of the same values give bitwise equal
 * results; N <= 4096, head_dim in [1, 128], scale positive and finite); scores: fp32 [B, N],
 * 4-byte aligned. */
int evt_token_scores(int dtype, const void* qkv, int64_t ldq, int64_t sb, int64_t sh, int ko,
                     int B, int N, int H, int head_dim, float scale, float* scores, void* stream);

/* Step 2: kept [B, 1 + K] int32 from scores [B, N] fp32 (rows N floats apart), 2 <= N <= 4096,
 * 1 <= K <= N - 1. Both 4-byte aligned. */
int evt_token_select(const float* scores, int B, int N, int K, int32_t* kept, void* stream);

/* Step 3: dst row b K1 + t = src row b T + kept[b, t] for t < K1, rows of D elements of `dtype`
 * (EVT_DTYPE_F32 / EVT_DTYPE_BF16), contiguous, 16-byte aligned, D a multiple of 8; with stats_src
 * and stats_dst (both or neither) the rows' `slots` x 2 floats move the same way (slots even).
 * 1 <= K1 <= T; an entry of kept outside [0, T) is clamped into it. EVT_EINVAL also when a
 * destination overlaps its source (a gather cannot run in place). */
int evt_token_gather(int dtype, const void* src, void* dst, const float* stats_src,
                     float* stats_dst, int slots, const int32_t* kept, int B, int T, int K1, int D,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVT_TOKEN_PRUNING_H_ */
