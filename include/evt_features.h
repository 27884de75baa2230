/* Companion of evt.h (which includes it): feature outputs of a model handle. Same conventions as
 * evt.h: C ABI of libevt_hip.so, EVT_* return codes, evt_last_error() for the text.
 *
 * evt_*_forward end in logits. evt_forward_features runs the same forward and also writes, as
 * fp32 into contiguous caller-owned device memory (16-byte aligned; logits: as evt_*_forward),
 * any of
 *
 *   pooled [batch, F]     the vector the classifier reads
 *   tokens [batch, T, F]  the final token map
 *   taps   [batch, tokens_i, width_i]  the residual stream after chosen blocks
 *
 *   family                  pooled                        tokens                 tap blocks
 *   ViT, EVT_VIT_REFERENCE  token 0 of the last block's   the last block's       depth encoder
 *                           output (the reference has no  output, T = P + 1      blocks, [T, D]
 *                           final LayerNorm, vit.py:54)
 *   ViT, EVT_VIT_STANDARD   LN(x)[:, 0]                   LN(x) of every token   as above
 *   T2T-ViT                 LN(x)[:, 0] (the reference's  LN(x)                  as above
 *                           forward_features,
 *                           t2t_vit.py:129-130)
 *   Swin                    mean over tokens of LN(x),    LN(x), T = R^2 and     blocks numbered
 *                           in the activation dtype (the  F = width of the last  consecutively over
 *                           head GEMM's operand)          stage                  the stages, tap i
 *                                                                                is its stage's
 *                                                                                [R^2, C]
 *
 * LN is the model's final LayerNorm, computed in fp32 from the stream as stored (bf16 or fp32).
 * A tap is the stream after block i (after its FC2 and residual), un-normalised; tap_norm = 1
 * passes every tap through the final LayerNorm (the get_intermediate_layers(norm=True)
 * convention) and is EVT_EINVAL for EVT_VIT_REFERENCE (no final LayerNorm) and for Swin (stage
 * widths differ). EVT_DTYPE_MX8 handles give logits, pooled and tokens; taps there are EVT_EINVAL.
 *
 * The kernels that produce `logits` are the ones evt_*_forward launches, in the same order on the
 * same operands: the logits are bitwise those of the plain forward. A handle with lanes
 * (evt_model_set_lanes) runs a features forward as one lane on its own workspace. The call only
 * enqueues kernels on `stream`: no allocation, no synchronisation. With evt_model_profile on,
 * the export launches count under EVT_PROF_HEAD. evt_graph_capture stays logits-only. */
#ifndef EVT_FEATURES_H_
#define EVT_FEATURES_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct evt_model evt_model;  /* evt.h */

typedef struct evt_features_args {
  float* logits;              /* [batch, num_classes] or NULL */
  float* pooled;              /* [batch, F] or NULL: the vector the classifier reads */
  float* tokens;              /* [batch, T, F] or NULL: the final token map */
  int32_t n_taps;             /* 0..64 */
  const int32_t* tap_blocks;  /* [n_taps] block indices, strictly increasing (host memory) */
  float* const* taps;         /* [n_taps] device pointers (host array), tap i is
                               * [batch, tokens_i, width_i] (evt_tap_shape) */
  int32_t tap_norm;           /* 1: taps pass through the final LayerNorm; else 0 */
} evt_features_args;

/* F, T and the number of blocks a tap can name (any of the three may be NULL). */
int evt_features_shape(const evt_model* m, int* F, int* T, int* n_blocks);
/* Tokens per image and width of the tap after block `block` (0 <= block < n_blocks). */
int evt_tap_shape(const evt_model* m, int block, int* tokens, int* width);
/* EVT_EINVAL before any launch (nothing written): a NULL model, img or args; every output NULL
 * with n_taps == 0; batch outside [1, max_batch]; n_taps outside [0, 64]; n_taps > 0 with a NULL
 * array or a NULL tap pointer; a tap index out of range or not strictly increasing; tap_norm
 * other than 0 / 1, or 1 where the table above rules it out; taps on an MX8 handle; a pooled,
 * tokens or tap pointer that is not 16-byte aligned. */
int evt_forward_features(evt_model* m, const float* img, int batch,
                         const evt_features_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVT_FEATURES_H_ */
