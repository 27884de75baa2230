/* Companion of evt.h (which includes it): attention rollout of a model handle. Same conventions
 * as evt.h: C ABI of libevt_hip.so, EVT_* return codes, evt_last_error() for the text.
 *
 * The attention maps (evt_attention_maps.h) are [batch, H, T, T] floats per block. What users do
 * with them is compose them into one attribution per image, attention rollout (Abnar & Zuidema,
 * 2020): which tokens the CLS token, or any other token, draws on through the whole encoder.
 * evt_forward_rollout forms it on the device from the same probabilities, without storing a
 * per-head map.
 *
 * For encoder block l with H_l heads and T tokens per image let p_l[b,h,i,j] be the value
 * evt_attention_maps.h defines: softmax_j(q_i . k_j * h_k^-0.5) of the stored q and k, scores,
 * statistics and normalisation in fp32. Then
 *
 *   Abar_l[b] = (1 / H_l) * sum_h p_l[b,h]                 [T, T], rows sum to 1
 *   Ahat_l[b] = 0.5 * (Abar_l[b] + I)
 *   R_l[b]    = Ahat_l[b] @ R_{l-1}[b],   R_{start-1} = I   ([query, source token])
 *   rollout   = R_{depth-1}
 *
 * mean head fusion with residual weight 0.5 over blocks start .. depth-1. Every Ahat_l is
 * row-stochastic, so there is no renormalisation step. Everything is fp32 whatever the model's
 * dtype: the head sum (heads added in index order, then one product with the fp32 nearest to
 * 1 / H_l), the + I, and both operands and the accumulator of the matrix product (the exact fp32
 * MFMA; no bf16 or split product). Outputs are fp32, contiguous and caller-owned:
 *
 *   EVT_ROLLOUT_CLS  [batch, T]     row 0 of the rollout: how much the CLS token draws on each
 *                                   token; [:, 1:] reshaped to the patch grid is the usual saliency map
 *   EVT_ROLLOUT_ALL  [batch, T, T]  indexed [.., query, source]
 *
 * Every value is finite and in [0, 1] up to rounding, and every row sums to 1 up to rounding (the
 * relative error of an element after L steps is at most the sum over the steps of
 * 2 eps_l + (H_l + T + 2) 2^-24, eps_l the probabilities' error; DESIGN.md, attention rollout).
 * The CLS output is bitwise the ALL output's [:, 0, :]. The head-major and the token-major QKV
 * layout (evt_model_qkv_layout) give bitwise equal results. A result does not depend on the
 * image's position in the batch and is bitwise reproducible: no atomics, one reduction order.
 *
 * Families: those of evt_forward_attention (ViT, reference and standard, pruned or not, and
 * T2T-ViT's encoder blocks). Swin and an EVT_DTYPE_MX8 handle are EVT_EINVAL (windows do not
 * compose this way: see evt_window_attention.h for Swin's per-window maps).
 *
 * Scratch. The handle's workspace does not grow for this: the caller owns the scratch (up to three
 * [batch, T, T] fp32 buffers: the head mean and two rollout buffers that alternate, because a step
 * cannot run in place), sized by evt_rollout_scratch_bytes and passed with every call. Its contents
 * are undefined afterwards.
 *
 * The forward is evt_forward_attention's: the same kernels in the same order, so logits, pooled,
 * tokens and taps (through `feat`) are bitwise those of evt_forward_features. The rollout launches
 * (a head mean and a matrix step per block) come right after each block's attention kernel from
 * block `start` on, the last block included (its QKV GEMM stores every row's q and k while its
 * attention runs on the CLS rows). A handle with lanes runs the call as one lane. The call only
 * enqueues kernels on `stream`: no allocation, no synchronisation. With evt_model_profile on, the
 * launches count under EVT_PROF_HEAD. evt_graph_capture stays logits-only. */
#ifndef EVT_ROLLOUT_H_
#define EVT_ROLLOUT_H_
#include <stddef.h>
#include <stdint.h>

#include "evt_image.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EVT_ROLLOUT_CLS 0
#define EVT_ROLLOUT_ALL 1

typedef struct evt_rollout_args {
  int32_t start;         /* first block of the product, 0 <= start < depth */
  int32_t mode;          /* EVT_ROLLOUT_CLS | EVT_ROLLOUT_ALL */
  float* out;            /* device, 16-byte aligned: [batch, T] or [batch, T, T] */
  void* scratch;         /* device, 16-byte aligned, scratch_bytes long */
  size_t scratch_bytes;  /* >= evt_rollout_scratch_bytes(m, batch, mode) */
} evt_rollout_args;

/* Tokens per image T and the number of encoder blocks (depth). Host only. EVT_EINVAL: a NULL
 * argument, a Swin or EVT_DTYPE_MX8 handle. */
int evt_rollout_shape(const evt_model* m, int* tokens, int* blocks);

/* Bytes of scratch a rollout forward of `batch` images needs in `mode`, for any `start`. Host
 * only. EVT_EINVAL: a NULL argument, a Swin or EVT_DTYPE_MX8 handle, a bad mode, batch outside
 * [1, max_batch]. */
int evt_rollout_scratch_bytes(const evt_model* m, int batch, int mode, size_t* bytes);

/* One forward of the images `in` that writes the rollout of `ro` and, when `feat` is non-NULL, the
 * outputs of `feat` as evt_forward_features does. With feat == NULL no classifier head runs.
 * EVT_EINVAL before any launch (nothing written): a NULL model, in or ro; a Swin or EVT_DTYPE_MX8
 * handle; start outside [0, depth); a mode other than EVT_ROLLOUT_CLS / EVT_ROLLOUT_ALL; a NULL or
 * not 16-byte aligned out or scratch; scratch_bytes too small; everything evt_forward_image rejects
 * of (in, batch, feat). */
int evt_forward_rollout(evt_model* m, const evt_image_args* in, int batch,
                        const evt_features_args* feat, const evt_rollout_args* ro, void* stream);

/* Op level (the parity tests): one block's step, r_out[b] = 0.5 (r_in[b] + Abar[b] @ r_in[b]) with
 * Abar the head mean of the q and k in qkv; r_in, r_out: [B, N, N] fp32, 16-byte aligned. The
 * arguments and layout rules are those of evt_attention_probs (both layouts of the same values give
 * bitwise equal results; N <= 4096, head_dim in [1, 128], H <= 254, scale positive and finite).
 * r_in == NULL means the identity: r_out = 0.5 (Abar + I). r_in must not overlap r_out
 * (EVT_EINVAL). scratch: device, 16-byte aligned, scratch_bytes >= B * N * N * 4 (it holds Abar
 * afterwards; nothing past B * N * N * 4 bytes is touched). */
int evt_attention_rollout_step(int dtype, const void* qkv, int64_t ldq, int64_t sb, int64_t sh,
                               int ko, int B, int N, int H, int head_dim, float scale,
                               const float* r_in, float* r_out, void* scratch, size_t scratch_bytes,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVT_ROLLOUT_H_ */
