/* Companion of evt.h (which includes it): the window attention maps of a Swin handle. Same
 * conventions as evt.h: C ABI of libevt_hip.so, EVT_* return codes, evt_last_error() for the text.
 *
 * Swin's attention is windowed and biased, a different object from the [T, T] maps of
 * evt_attention_maps.h (whose entry points keep refusing a Swin handle): its window kernels form
 * the probabilities of one 7 x 7 or 12 x 12 window in registers, multiply them by V and discard
 * them, and the fused stage-1 sublayer never writes q and k to memory at all.
 * evt_forward_window_attention runs the same forward and also writes, for chosen blocks, those
 * probabilities as fp32 into contiguous caller-owned device memory:
 *
 *   map_i[b, win, h, q, k] = softmax_k(q_q . k_k * 32^-0.5 + rpb[rel(q, k), h] + mask(win, q, k))
 *   shape [batch, nW, H_i, N, N]
 *
 * with w the effective window of block i's stage (7 or 12; evt_window_attn_map_shape), N = w * w,
 * nW = (R / w)^2 the windows of its R x R token map, H_i the stage's heads (head size 32). Blocks
 * are numbered consecutively over the stages, as for taps (evt_features.h).
 *   q, k   window-local token numbers in the SHIFTED frame (the token map rolled by -shift along
 *          both axes in a shifted block), row-major inside the window
 *   win    row-major over the windows of the shifted frame
 *   rel    the relative position index into the block's [(2w - 1)^2, H] bias table
 *   mask   the SW-MSA region mask of a shifted block: a (query, key) pair in different regions is
 *          written as EXACTLY 0.0f, in both dtypes (the reference's additive -100 leaves a
 *          relative weight of at most e^-100, below fp32 resolution; the bf16 forward kernels use
 *          -inf there as well)
 * Window-local token (i, j) of window (wy, wx) is the token at row (wy w + i + shift) mod R,
 * column (wx w + j + shift) mod R of the block's raster token map.
 *
 * Value: of the q and k the block's LN1-folded QKV GEMM stores (bf16 or fp32), with the scores,
 * the statistics and the normalisation in fp32. This is the probability BEFORE the bf16 rounding a
 * bf16 model's kernel applies to it for the product with V. Every query shares a region with
 * itself, so no row is empty; every written value is finite and in [0, 1].
 *
 * Fused blocks. A bf16 model's 96-channel, 3-head, window-7 stage runs its attention sublayer as
 * one kernel that keeps q, k and v on chip. For a REQUESTED block of such a stage the call also
 * runs the block's QKV GEMM of the general path into the workspace and exports the map of those q
 * and k; the fused sublayer itself runs unchanged. The map of such a block is therefore of the
 * q / k the general path computes: the fused kernel's own differ from them only by bf16 rounding
 * order (its bias is seeded into the accumulators, its LayerNorm runs in registers). A block that
 * is not requested costs nothing.
 *
 * The kernels that produce the logits (and pooled / tokens / taps through `feat`) are the ones
 * evt_swin_forward / evt_forward_features launch, in the same order on the same operands: those
 * outputs are bitwise the same. The export of block i is one more launch right after the block's
 * window-attention kernel (fused blocks: two, before the sublayer). A handle with lanes
 * (evt_model_set_lanes) runs the call as one lane on its own workspace. The call only enqueues
 * kernels on `stream`: no allocation, no synchronisation. With evt_model_profile on, the export
 * launches count under EVT_PROF_HEAD. evt_graph_capture stays logits-only. One map is
 * batch * nW * H_i * N * N * 4 bytes (Swin-B at 384 px, stage 1, 64 images: 1.36 GB); every
 * output offset is 64-bit. */
#ifndef EVT_WINDOW_ATTENTION_H_
#define EVT_WINDOW_ATTENTION_H_
#include <stdint.h>

#include "evt_attention_maps.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Windows per image, heads and tokens per window (N) of block `block` of a Swin handle.
 * EVT_EINVAL: a NULL argument, a handle that is not Swin, a block out of range. */
int evt_window_attn_map_shape(const evt_model* m, int block, int* windows, int* heads,
                              int* tokens);

/* One forward of the images `in` (evt_image.h) that writes the window maps of `attn`
 * (evt_attention_maps.h: evt_attn_args, with queries = EVT_ATTN_ALL) and, when `feat` is non-NULL,
 * the outputs of `feat` as evt_forward_features does. With feat == NULL no classifier head runs.
 * EVT_EINVAL before any launch (nothing written): a NULL model, in or attn; a handle that is not
 * Swin (its maps are evt_forward_attention's); n_maps outside [0, 64]; n_maps == 0 with
 * feat == NULL; n_maps > 0 with a NULL array or a NULL map pointer; a block out of range or blocks
 * not strictly increasing; queries other than EVT_ATTN_ALL; a map pointer that is not 16-byte
 * aligned; everything evt_forward_image rejects of (in, batch, feat). */
int evt_forward_window_attention(evt_model* m, const evt_image_args* in, int batch,
                                 const evt_features_args* feat, const evt_attn_args* attn,
                                 void* stream);

/* Op level (the parity tests): out [B, (R / window)^2, H, N, N] as above from qkv, the raster
 * token rows [B * R * R, ldq >= 3 * C] with columns (qkv h d), head size 32 (C = 32 * H), and rpb,
 * the raw [(2 * window - 1)^2, H] fp32 bias table, which the call expands with the model's table
 * kernels into stream-ordered scratch. EVT_EINVAL: a dtype other than EVT_DTYPE_F32 /
 * EVT_DTYPE_BF16, a NULL pointer, window not 7 or 12, R not a positive multiple of window,
 * C != 32 * H, shift outside [0, window), a non-zero shift with R == window, ldq < 3 * C, B < 0,
 * out not 16-byte aligned, and for EVT_DTYPE_BF16 qkv not 16-byte aligned or ldq % 8 != 0. */
int evt_window_attention_probs(int dtype, const void* qkv, int64_t ldq, const float* rpb, int B,
                               int R, int window, int C, int H, int shift, float* out,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVT_WINDOW_ATTENTION_H_ */
