/* Companion of evt.h (which includes it): attention-map outputs of a model handle. Same
 * conventions as evt.h: C ABI of libevt_hip.so, EVT_* return codes, evt_last_error() for the text.
 *
 * The fused attention kernels form softmax(q k^T h_k^-0.5) in registers, multiply by V and discard
 * it, and the next layer overwrites q and k: a block tap cannot recover the probabilities.
 * evt_forward_attention runs the same forward and also writes, for chosen encoder blocks, the
 * attention probabilities as fp32 into contiguous caller-owned device memory:
 *
 *   EVT_ATTN_CLS  [batch, H_i, T]     the row of query token 0 (the CLS token)
 *   EVT_ATTN_ALL  [batch, H_i, T, T]  indexed [.., query, key]
 *
 * H_i is the number of heads of block i (a pruned model's differ per block) and T the tokens per
 * image (evt_attn_map_shape).
 *
 * Value: softmax_j(q_i . k_j * h_k^-0.5) of the q and k the block's QKV GEMM stored (bf16 or
 * fp32), with the scores accumulated in fp32, the statistics in fp32 and the result normalised in
 * fp32. This is the probability BEFORE the bf16 rounding a bf16 model's fused kernel applies to
 * it for the product with V, so it is slightly more precise than what the model multiplied by.
 * Keys >= T never contribute; every written value is finite and in [0, 1]. The CLS output is
 * bitwise the ALL output's [:, :, 0, :] (one kernel, one code path), and the head-major and the
 * token-major QKV layout (evt_model_qkv_layout) give bitwise equal maps.
 *
 * Families: ViT (EVT_VIT_REFERENCE and EVT_VIT_STANDARD, pruned or not) and T2T-ViT (its encoder
 * blocks). Swin is EVT_EINVAL: its windowed, biased attention is a different object, with its own
 * entry points (evt_window_attention.h). An EVT_DTYPE_MX8 handle is EVT_EINVAL, as for taps.
 *
 * The kernels that produce the logits (and pooled / tokens / taps through `feat`) are the ones
 * evt_*_forward / evt_forward_features launch, in the same order on the same operands: those
 * outputs are bitwise the same. The export of block i is one more launch right after the block's
 * attention kernel. A handle with lanes (evt_model_set_lanes) runs the call as one lane on its own
 * workspace. The call only enqueues kernels on `stream`: no allocation, no synchronisation. With
 * evt_model_profile on, the export launches count under EVT_PROF_HEAD. evt_graph_capture stays
 * logits-only. */
#ifndef EVT_ATTENTION_MAPS_H_
#define EVT_ATTENTION_MAPS_H_
#include <stdint.h>

#include "evt_image.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EVT_ATTN_CLS 0
#define EVT_ATTN_ALL 1

typedef struct evt_attn_args {
  int32_t n_maps;            /* 0..64 */
  const int32_t* blocks;     /* [n_maps] block indices, strictly increasing (host memory) */
  float* const* maps;        /* [n_maps] device pointers (host array), 16-byte aligned */
  int32_t queries;           /* EVT_ATTN_CLS | EVT_ATTN_ALL */
} evt_attn_args;

/* Heads of block `block` (0 <= block < depth) and tokens per image. EVT_EINVAL: a NULL argument,
 * a block out of range, a Swin or EVT_DTYPE_MX8 handle. */
int evt_attn_map_shape(const evt_model* m, int block, int* heads, int* tokens);

/* One forward of the images `in` (evt_image.h: fp32 in the family's layout or uint8 NHWC) that
 * writes the maps of `attn` and, when `feat` is non-NULL, the outputs of `feat` as
 * evt_forward_features does. With feat == NULL no classifier head runs.
 * EVT_EINVAL before any launch (nothing written): a NULL model, in or attn; a Swin or
 * EVT_DTYPE_MX8 handle; n_maps outside [0, 64]; n_maps == 0 with feat == NULL; n_maps > 0 with a
 * NULL array or a NULL map pointer; a block out of range or blocks not strictly increasing;
 * queries other than EVT_ATTN_CLS / EVT_ATTN_ALL; a map pointer that is not 16-byte aligned;
 * everything evt_forward_image rejects of (in, batch, feat) (a non-NULL feat must name an
 * output). */
int evt_forward_attention(evt_model* m, const evt_image_args* in, int batch,
                          const evt_features_args* feat, const evt_attn_args* attn, void* stream);

/* Op level (the parity tests): out[b][h][i][j] = softmax_j(q_i . k_j * scale), fp32, contiguous
 * [B, H, nq, N] with nq = 1 (the row of query 0) or nq = N. qkv as evt_attention_hd: [B*N, ldq >=
 * 3*H*head_dim] columns (qkv h d) when sb, sh and ko are all 0; otherwise the slice of (image b,
 * head h) starts at qkv + b*sb + h*sh (elements), its rows are ldq apart and k is at column ko of
 * a row (EVT_DTYPE_BF16, head_dim 64, all multiples of 8: the head-major layout of the model's
 * QKV GEMM is sb = 3*H*N*64, sh = 3*N*64, ldq = 64, ko = N*64). Both layouts of the same values
 * give bitwise equal results. N <= 4096, head_dim in [1, 128], scale positive and finite, out
 * 16-byte aligned, qkv rows 16-byte aligned when head_dim is a multiple of 16 bytes. */
int evt_attention_probs(int dtype, const void* qkv, int64_t ldq, int64_t sb, int64_t sh, int ko,
                        int B, int N, int H, int head_dim, float scale, int nq, float* out,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVT_ATTENTION_MAPS_H_ */
