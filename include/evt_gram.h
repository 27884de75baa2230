/* Companion of evt.h (which includes it): second moments ("Grams") of the activations a pruned
 * layer's consumer reads, formed on the device during a forward. Same conventions as evt.h: C ABI
 * of libevt_hip.so, EVT_* return codes, evt_last_error() for the text.
 *
 * A closed-form least-squares repair of the layer behind a cut (FC2 after an FFN cut, the
 * out-projection after a head cut; pruning.py reconstruct_linear) needs, of the matrix H the layer
 * multiplies, G = H^T H and the column sums. H is resident in every forward and too large to
 * export (620 MB per block at DeiT-base and 512 images):
 *
 *   EVT_GRAM_FFN   the FC1 output (GELU, rounded to the model dtype) FC2 reads, [batch T, F],
 *                  F = the block's FFN neurons
 *   EVT_GRAM_ATTN  the attention context the out-projection reads, [batch T, heads * head_dim]
 *
 * For a row-major matrix a of R rows and F columns the outputs are fp32 whatever the dtype,
 * written, not accumulated:
 *
 *   gram[i][j] = sum_r a[r][i] a[r][j]     contiguous [F][F], both triangles, bitwise symmetric
 *   sums[j]    = sum_r a[r][j]             [F]
 *
 * Products are exact for bf16 and rounded once for fp32 (the MFMA's fused multiply-add); sums are
 * fp32. The order of every sum is a function of (R, F) alone: a result is bitwise reproducible.
 * No atomics. Few output tiles (F = 768: 21) would leave most of the device idle, so the rows are
 * also split into chunks whose fp32 partial tiles go through a caller-owned scratch and are added
 * in chunk order by a second launch; evt_gram_scratch_bytes sizes it from (rows, width) alone.
 *
 * Families: the users of the shared encoder, ViT (reference and STANDARD semantics, pruned or not)
 * and T2T-ViT (the blocks of its backbone). Swin and an EVT_DTYPE_MX8 handle are EVT_EINVAL, as
 * for the FFN statistics (evt_ffn_stats.h), and so is a handle with a token schedule (its later
 * blocks see a subset of the tokens) and a request for a sublayer that is skipped (evt_depth.h).
 *
 * The forward is evt_forward_features': logits, pooled, tokens and taps (through `feat`) are bitwise
 * those of evt_forward_features. An EVT_GRAM_FFN Gram of block i is launched after the block's
 * full-row FC1 and before its FC2, an EVT_GRAM_ATTN Gram after its attention kernel and before its
 * out-projection. The last block runs its full-row form when its Gram is asked for, exactly as for
 * evt_forward_ffn_stats; the CLS rows the head and `pooled` read stay the CLS tail's (evt_tail.h),
 * so logits stay bitwise. The Gram of block i does not depend on block i's own gates (evt_gates.h):
 * it reads what FC1 or the attention kernel stored. A handle with lanes runs the call as one lane.
 * The call only enqueues kernels on `stream`: no allocation, no synchronisation. With
 * evt_model_profile on, the launches count under EVT_PROF_HEAD with 2 R F^2 FLOPs. */
#ifndef EVT_GRAM_H_
#define EVT_GRAM_H_
#include <stddef.h>
#include <stdint.h>

#include "evt_image.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EVT_GRAM_FFN 0
#define EVT_GRAM_ATTN 1
#define EVT_GRAM_MAX_WIDTH 6144

typedef struct evt_gram_args {
  int32_t n_blocks;          /* 0..64 */
  const int32_t* blocks;     /* [n_blocks] block indices, strictly increasing (host memory) */
  int32_t which;             /* EVT_GRAM_FFN or EVT_GRAM_ATTN */
  float* const* grams;       /* [n_blocks] device pointers (host array) to [F_i][F_i], 16-B aligned */
  float* const* sums;        /* [n_blocks] device pointers (host array) to [F_i], 16-B aligned */
  void* scratch;             /* device, 16-byte aligned (NULL when no block needs any) */
  size_t scratch_bytes;      /* >= evt_gram_scratch_bytes(batch * tokens, F_i) of every block */
} evt_gram_args;

/* Bytes of scratch evt_gram wants for a matrix of `rows` rows and `width` columns (0: one launch,
 * no scratch). Host only; a function of (rows, width) alone, never of the device. EVT_EINVAL: a
 * NULL bytes, rows outside [1, 2^31 - 1], width outside [1, EVT_GRAM_MAX_WIDTH]. */
int evt_gram_scratch_bytes(int64_t rows, int width, size_t* bytes);

/* Op level: gram [width][width] and sums [width] of the row-major matrix a (`rows` rows, a pitch of
 * ld elements; columns width .. ld - 1 may be loaded and never reach a stored element, rows past
 * `rows` are not read). dtype EVT_DTYPE_BF16 or EVT_DTYPE_F32. EVT_EINVAL with a message naming
 * `gram`, nothing written: a NULL a, gram or sums; a, gram, sums or scratch not 16-byte aligned;
 * width not a positive multiple of the 16-byte vector (8 bf16, 4 f32) or above EVT_GRAM_MAX_WIDTH;
 * ld < width or not a multiple of the vector; rows < 1 or above 2^31 - 1; scratch_bytes below
 * evt_gram_scratch_bytes(rows, width), or a NULL scratch when that is not 0. */
int evt_gram(int dtype, const void* a, int64_t ld, int64_t rows, int width, float* gram,
             float* sums, void* scratch, size_t scratch_bytes, void* stream);

/* Width of block `block`'s Gram (EVT_GRAM_FFN: its FFN neurons, EVT_GRAM_ATTN: heads * head_dim;
 * a pruned ViT's differ per block) and tokens per image: a batch of B images is a matrix of
 * B * tokens rows. EVT_EINVAL: a NULL argument, a block out of range, an unknown `which`, a Swin
 * or EVT_DTYPE_MX8 handle. */
int evt_gram_shape(const evt_model* m, int block, int which, int* width, int* tokens);

/* One forward of the images `in` that writes the Grams of `ga` and, when `feat` is non-NULL, the
 * outputs of `feat` as evt_forward_features does. With feat == NULL no classifier head runs.
 * EVT_EINVAL before any launch (nothing written): a NULL model, in or ga; a Swin or EVT_DTYPE_MX8
 * handle; a handle with a token schedule; n_blocks outside [0, 64]; n_blocks == 0 with feat ==
 * NULL; an unknown `which`; n_blocks > 0 with a NULL array or a NULL gram or sums pointer; a block
 * out of range or blocks not strictly increasing; a block whose sublayer (`which`) is skipped; a
 * gram, sums or scratch pointer that is not 16-byte aligned; a scratch smaller than a block needs;
 * everything evt_forward_image rejects of (in, batch, feat). */
int evt_forward_grams(evt_model* m, const evt_image_args* in, int batch,
                      const evt_features_args* feat, const evt_gram_args* ga, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVT_GRAM_H_ */
