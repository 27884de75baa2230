/* Companion of evt.h (which includes it): structured gates of a ViT handle. Same conventions as
 * evt.h: C ABI of libevt_hip.so, EVT_* return codes, evt_last_error() for the text.
 *
 * A gate silences or scales one attention head or one FFN neuron of the model that is already on
 * the device, without a rebuild: the head-ablation sweep of are_16_heads (mask one head, read the
 * accuracy), cumulative masking, and the real-valued head gates xi_h of Michel et al. 2019.
 *
 *   head gate g of head h of block l    multiplies the head's head_dim columns of the attention
 *                                       output before the out-projection
 *   FFN gate g of neuron j of block l   multiplies column j of the hidden activation before FC2
 *
 * Both are linear into a GEMM, so they are applied to the packed weights, once, when the gates
 * change: W'[n][k] = round_dtype(g[k] * W0[n][k]) over the out-projection / FC2 weight of the
 * block, with W0 the pristine weight. The forward itself is unchanged and costs nothing more.
 *
 * CONTRACT. A gated handle is bitwise a fresh handle created from gated parameters: the out_w
 * of block l with row h * head_dim + d multiplied by its head's gate, the fc2_w of block l with
 * row j multiplied by neuron j's gate (Keras [in, out] layout, evt_vit_num_weights order), the
 * product taken in fp32 of the value the loader stores (the fp32 weight of an EVT_DTYPE_F32
 * handle, the bf16-rounded weight of an EVT_DTYPE_BF16 one). That holds for every output: logits,
 * pooled, tokens, taps, maps, statistics, rollout, token-pruning exports. All-ones gates and
 * evt_model_clear_gates restore the packed weights bitwise. Any finite float is a gate (negative,
 * above 1); 0 times a negative weight is -0.0, as in the fresh handle. Padding stays zero.
 *
 * WHAT A BLOCK'S OWN GATES DO NOT CHANGE. The attention maps, head statistics and rollout
 * matrix of block l are statistics of the probabilities block l computed: they do not depend on
 * block l's head gates. The FFN statistics of block l are statistics of what FC1 stored: they do
 * not depend on block l's FFN gates. Later blocks see the gated stream.
 *
 * PRISTINE COPIES. The first non-identity gate of a (block, role) allocates a device copy of that
 * packed weight in the model dtype and a [kpad] fp32 gate vector (hipMalloc: it may synchronise
 * the device, once per role); the handle owns them until evt_model_destroy. Every set reads the
 * pristine copy, so successive sets do not compound rounding. The forward allocates nothing.
 *
 * STREAMS AND GRAPHS. A set enqueues on `stream` a copy of the expanded gates and one kernel
 * (gates.hip); forwards enqueued later on that stream (its lanes included) see the new gates,
 * earlier ones the old. The host array is read before the call returns. A captured graph reads the
 * same weight allocations: it needs no recapture, its next replay is gated. The calls that enqueue
 * are refused while `stream` is capturing (EVT_EINVAL, "capturing").
 *
 * Families: ViT handles (reference and standard, pruned or not) in f32 and bf16, the parent handle
 * only. EVT_EINVAL with the reason: T2T-ViT, Swin, EVT_DTYPE_MX8 (block-scaled weights would need
 * requantising), a lane child. */
#ifndef EVT_GATES_H_
#define EVT_GATES_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* gates[h] for the n heads of block `block` (n = evt_head_stats_shape's heads; block < 0 counts
 * from the last, as in the analysis block lists). EVT_EINVAL: a NULL model or array; an unsupported
 * handle; block outside [-depth, depth); n != the block's heads; a NaN or infinite gate; a
 * capturing stream. On an error nothing changes. */
int evt_model_set_head_gates(evt_model* m, int block, const float* gates, int n, void* stream);

/* gates[j] for the n FFN neurons of block `block` (n = evt_ffn_stats_shape's neurons). Errors as
 * evt_model_set_head_gates. */
int evt_model_set_ffn_gates(evt_model* m, int block, const float* gates, int n, void* stream);

/* Every gate back to 1: the packed weights of every gated role are restored from their pristine
 * copies (device-to-device, on `stream`). EVT_EINVAL: a NULL model, an unsupported handle, a
 * capturing stream. */
int evt_model_clear_gates(evt_model* m, void* stream);

/* The host-side record of block `block`: *n = its heads / neurons, gates (may be NULL) receives up
 * to `cap` of them (1 where none was set). Host only. EVT_EINVAL: a NULL model or n, an unsupported
 * handle, block out of range, cap < 0. */
int evt_model_get_head_gates(const evt_model* m, int block, float* gates, int cap, int* n);
int evt_model_get_ffn_gates(const evt_model* m, int block, float* gates, int cap, int* n);

/* Op level (the parity tests): w[r][k] = round_dtype(gates[k] * w0[r][k]) for r < npad, k < kpad
 * of a packed weight [npad][kpad] of `dtype` (EVT_DTYPE_F32 / EVT_DTYPE_BF16), gates fp32 [kpad];
 * the product in fp32, the rounding evt_pack_weight's. npad >= 1, kpad a positive multiple of 64;
 * w0, w and gates 16-byte aligned; w must not overlap w0 or gates (EVT_EINVAL otherwise). */
int evt_gate_weights(int dtype, const void* w0, void* w, const float* gates, int npad, int kpad,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVT_GATES_H_ */
