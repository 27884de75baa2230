/* Companion of evt.h (which includes it): per-neuron statistics of the FFN hidden activations of a
 * model handle. Same conventions as evt.h: C ABI of libevt_hip.so, EVT_* return codes,
 * evt_last_error() for the text.
 *
 * Every encoder block's FC1 stores the GELU output of all batch * T token rows, and FC2 reads it
 * back: at DeiT-base and 512 images that matrix is 620 MB per block. What a pruning or dead-neuron
 * analysis wants of it is a few numbers per neuron; evt_forward_ffn_stats forms them on the device
 * between FC1 and FC2, without exporting the matrix.
 *
 * For a block with F FFN neurons (its un-padded width; a pruned ViT's differ per block) and T
 * tokens per image let a[b,t,j] be the value FC1's epilogue stored in the hidden buffer: the GELU
 * output as rounded to the model dtype, which is what FC2 multiplies. The output of a block is
 * stats[b][j][0..3], fp32, contiguous [batch, F, EVT_FFN_STATS]:
 *
 *   EVT_FFN_MEAN      (sum_t a) / T
 *   EVT_FFN_MEAN_ABS  (sum_t |a|) / T
 *   EVT_FFN_MEAN_SQ   (sum_t a^2) / T
 *   EVT_FFN_MAX_ABS   max_t |a|   (exact: it is one of the stored values)
 *
 * The sums are fp32 and run over all T tokens, the CLS token included. All four are continuous in
 * the activations; an "active fraction" (a > 0) is deliberately not among them: it flips on
 * rounding near 0. mean and mean_sq give the variance (and the mean to replace a pruned neuron by);
 * mean_sq times the squared norm of the neuron's FC2 row is the usual output-energy importance.
 * A (b, j) result is bitwise reproducible and does not depend on the image's position in the batch
 * or on the batch size: the order of every sum is fixed, with no atomics and no scratch memory.
 * The hidden buffer's padding columns (F up to the stored row width) never reach the output.
 *
 * Families: the users of the shared encoder, ViT (reference and STANDARD semantics, pruned or not)
 * and T2T-ViT (the blocks of its backbone). Swin and an EVT_DTYPE_MX8 handle are EVT_EINVAL: Swin's
 * stage-1 fused MLP never stores its hidden rows, and the MX8 encoder keeps them block-scaled 8-bit
 * (its FC1 epilogue quantises them), so neither has the matrix this contract is about.
 *
 * The forward is evt_forward_features': logits, pooled, tokens and taps (through `feat`) are bitwise
 * those of evt_forward_features; the statistics of block i are one more launch after the block's
 * full-row FC1 and before its FC2. The last block: a logits forward runs its FC1 on the B CLS rows
 * only (evt_tail.h); when the last block's statistics are asked for, the full-row block runs as
 * well, exactly as for `tokens` or a tap on it, and the statistics are those of the full-row FC1
 * launch. The CLS rows the head and `pooled` read stay the tail's, so logits stay bitwise; the CLS
 * row that enters the statistics is the full-row kernel's, not the tail kernel's (the same value up
 * to the two kernels' summation orders). A handle with lanes runs the call as one lane. The call
 * only enqueues kernels on `stream`: no allocation, no synchronisation. With evt_model_profile on,
 * the launches count under EVT_PROF_HEAD, as every export does. evt_graph_capture stays
 * logits-only. */
#ifndef EVT_FFN_STATS_H_
#define EVT_FFN_STATS_H_
#include <stdint.h>

#include "evt_image.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EVT_FFN_STATS 4
#define EVT_FFN_MEAN 0
#define EVT_FFN_MEAN_ABS 1
#define EVT_FFN_MEAN_SQ 2
#define EVT_FFN_MAX_ABS 3
#define EVT_FFN_STATS_MAX_TOKENS 4096 /* tokens per image of the op-level entry point */

typedef struct evt_ffn_stats_args {
  int32_t n_blocks;          /* 0..64 */
  const int32_t* blocks;     /* [n_blocks] block indices, strictly increasing (host memory) */
  float* const* stats;       /* [n_blocks] device pointers (host array), 16-byte aligned */
} evt_ffn_stats_args;

/* FFN neurons of block `block` (0 <= block < depth) and tokens per image. EVT_EINVAL: a NULL
 * argument, a block out of range, a Swin or EVT_DTYPE_MX8 handle. */
int evt_ffn_stats_shape(const evt_model* m, int block, int* neurons, int* tokens);

/* One forward of the images `in` that writes the statistics of `fs` and, when `feat` is non-NULL,
 * the outputs of `feat` as evt_forward_features does. With feat == NULL no classifier head runs.
 * EVT_EINVAL before any launch (nothing written): a NULL model, in or fs; a Swin or EVT_DTYPE_MX8
 * handle; n_blocks outside [0, 64]; n_blocks == 0 with feat == NULL; n_blocks > 0 with a NULL
 * array or a NULL stats pointer; a block out of range or blocks not strictly increasing; a stats
 * pointer that is not 16-byte aligned; everything evt_forward_image rejects of (in, batch, feat). */
int evt_forward_ffn_stats(evt_model* m, const evt_image_args* in, int batch,
                          const evt_features_args* feat, const evt_ffn_stats_args* fs,
                          void* stream);

/* Op level (the parity tests): out[b][j][0..3], j < F, of the row-major matrix h of B * T rows with
 * a pitch of ld elements (row b T + t is token t of image b; columns F .. ld - 1 are never stored
 * into out). dtype EVT_DTYPE_BF16 or EVT_DTYPE_F32; h and out 16-byte aligned; ld >= F and the row
 * pitch a multiple of 16 bytes (ld % 8 == 0 for bf16, ld % 4 == 0 for f32); 1 <= T <=
 * EVT_FFN_STATS_MAX_TOKENS, F >= 1, B >= 1. */
int evt_ffn_neuron_stats(int dtype, const void* h, int64_t ld, int B, int T, int F, float* out,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVT_FFN_STATS_H_ */
