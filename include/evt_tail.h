/* Companion of evt.h (which includes it): the CLS tail of the ViT / T2T-ViT encoder and its query.
 * Same conventions: C ABI of libevt_hip.so, EVT_* return codes, evt_last_error() for the text. */
#ifndef EVT_TAIL_H_
#define EVT_TAIL_H_
#ifdef __cplusplus
extern "C" {
#endif

struct evt_model;

/* The classifier of a ViT (head on token 0, vit.py:54-55; STANDARD: final LayerNorm of the CLS
 * rows folded in) and of a T2T-ViT (t2t_vit.py:129-134) reads token 0 of the last encoder block's
 * output and nothing else, and so does `pooled`. After the last block's QKV Dense that row needs
 * the image's K and V of every token, its own attention row, and its own row of the block input.
 * So the last block of a forward runs its out-proj, FC1 and FC2 on the B CLS rows only (M = B
 * instead of B T, always the 128 x 128 GEMM kernel: one image alone gives the bits it gives in a
 * batch) and, in bf16 with head size 64 up to 256 tokens, its attention on query tile 0 only (K
 * and V staged as ever, the same tile code: row 0 is bitwise the full launch's row 0). The rows
 * stay where they were: rows b T of the token stream and of its LayerNorm statistics.
 *
 * A call that exports the last block's token map (evt_forward_features / evt_forward_image /
 * evt_forward_attention with `tokens`, or a tap on the last block) runs the full-row block too,
 * each full-row launch before the CLS launch of its role; the CLS rows of that map, `pooled` and
 * the logits are the CLS tail's, so they equal a plain forward's bit for bit.
 *
 * Not affected: EVT_DTYPE_MX8 models, depth 0, Swin (it pools over all tokens): mode 0.
 *
 * mode: bit 0 set when the handle's last forward ran the CLS tail, bit 1 when it ran the
 * full-row last block (1: logits-only, pooled-only and attention-map calls; 3: tokens or a
 * last-block tap). Lets the tests assert which path ran. */
int evt_model_tail_mode(const struct evt_model* m, int* mode);

#ifdef __cplusplus
}
#endif
#endif /* EVT_TAIL_H_ */
