/* Companion of evt.h (which includes it): classification outputs. Same conventions as evt.h: C ABI
 * of libevt_hip.so, EVT_* return codes, evt_last_error() for the text.
 *
 * A forward ends in [batch, num_classes] fp32 logits. What an evaluation does next (the
 * reference's evaluate_* routines, utils.py: argmax against the target, correct / total over the
 * dataset; trt_benchmark's topk) is one more kernel here: the ordered top-k classes, their
 * probabilities or logits, the log-sum-exp, each label's rank, and hit counters that stay on the
 * device, so a loop over a dataset only enqueues work and reads three integers at its end.
 *
 * Order. For a row of C logits l[0..C) one total order on the classes:
 *   i comes before j  iff  l_i > l_j, or l_i == l_j and i < j
 *   -0.0 == +0.0 (the index decides); a NaN comes after every non-NaN, NaNs among themselves by
 *   index.
 * This is numpy's argsort(-l, kind="stable"); its first element is argmax(l).
 *
 * Outputs per row b, each optional (NULL: not written):
 *   indices[b, j]  int32, j < k: the j-th class in that order
 *   vals[b, j]     fp32: EVT_CLASSIFY_LOGIT the logit itself, a bitwise copy;
 *                  EVT_CLASSIFY_PROB exp(l_i - m) / sum_c exp(l_c - m), m = max_c l_c, in fp32
 *   lse[b]         fp32: m + log sum_c exp(l_c - m)
 *   rank[b]        int32, with labels[b] = y (int32, device): the position of y in the order,
 *                  #{c : l_c > l_y} + #{c < y : l_c == l_y}; 0 is top-1. y outside [0, C) (-1: "no
 *                  label") gives -1 and is not counted
 *   counters       int64[3], with labels: += (rows with a valid label, rows with rank < 1, rows
 *                  with rank < k). Added to with integer atomics, never zeroed: exact and
 *                  independent of the order of the calls
 *
 * A row's outputs are a function of its C values alone: a permuted batch gives permuted,
 * bitwise-equal outputs, and evt_classify on a forward's logits gives the bits of
 * evt_forward_classify. Rows with non-finite logits: indices and rank still follow the order; vals
 * (PROB) and lse are what IEEE arithmetic gives. A row of finite and -inf entries with at least
 * one finite one has finite probabilities, exactly 0 at the -inf entries.
 *
 * Limits: 1 <= k <= min(C, EVT_CLASSIFY_MAX_K), 1 <= C <= 2^20, ldl >= C, batch >= 1. Rows need
 * 4-byte alignment only (C = 10: rows 40 bytes apart). */
#ifndef EVT_CLASSIFY_H_
#define EVT_CLASSIFY_H_
#include <stdint.h>

#include "evt_image.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EVT_CLASSIFY_PROB 0
#define EVT_CLASSIFY_LOGIT 1
#define EVT_CLASSIFY_MAX_K 32

typedef struct evt_classify_args {
  int32_t k;                /* 1..min(C, EVT_CLASSIFY_MAX_K) */
  int32_t values;           /* EVT_CLASSIFY_PROB | EVT_CLASSIFY_LOGIT: what vals holds */
  int32_t* indices;         /* [batch, k] or NULL */
  float* vals;              /* [batch, k] or NULL */
  float* lse;               /* [batch] or NULL */
  const int32_t* labels;    /* [batch] or NULL */
  int32_t* rank;            /* [batch] or NULL (needs labels) */
  int64_t* counters;        /* [3] or NULL (needs labels): valid, top-1 hits, top-k hits */
} evt_classify_args;        /* 56 bytes */

/* Op level: the kernel alone on device logits [batch, num_classes], rows ldl elements apart (for
 * example after evt_graph_launch, on the same stream). One launch, no allocation, no
 * synchronisation.
 * EVT_EINVAL before the launch (nothing written): NULL logits or a; batch < 1; num_classes outside
 * [1, 2^20]; ldl < num_classes; k out of range; values neither PROB nor LOGIT; indices, vals, lse,
 * rank and counters all NULL; rank or counters without labels; a pointer that is not 4-byte
 * (counters: 8-byte) aligned. */
int evt_classify(const float* logits, int64_t ldl, int batch, int num_classes,
                 const evt_classify_args* a, void* stream);

/* The forward evt_forward_image runs for (in, batch, feat) (over the handle's lanes when feat names
 * logits only, as one lane otherwise), then, after the lanes have joined, the classify launch on
 * `stream` over feat->logits (ldl = num_classes). feat and feat->logits are required: the caller
 * owns the logits buffer; the workspace does not change. Logits, pooled, tokens and taps are
 * bitwise those of evt_forward_image. Every family and dtype (Swin and EVT_DTYPE_MX8 too: it reads
 * logits only). No allocation, no synchronisation; with evt_model_profile on, the launch counts
 * under EVT_PROF_HEAD. evt_graph_capture stays logits-only.
 * EVT_EINVAL before any launch (nothing written): a NULL model, in, feat, feat->logits or cls;
 * everything evt_classify rejects of cls; everything evt_forward_image rejects. */
int evt_forward_classify(evt_model* m, const evt_image_args* in, int batch,
                         const evt_features_args* feat, const evt_classify_args* cls, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVT_CLASSIFY_H_ */
