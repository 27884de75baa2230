// The transformer encoder ViT and T2T-ViT share: its weights, workspace buffers and layers.
//
// The model handle owns the packed weights (kernel operand layout, zero padded, LayerNorm gamma
// folded in) and one workspace sized for max_batch; evt_vit_forward enqueues the whole ViT
// forward of reference `modeling/models/vit.py:41-55` on the caller's stream with no host
// synchronisation. Per encoder layer (transformer_encoder.py:13-18):
//
//   QKV GEMM   A = x (raw stream), epilogue applies LN1 per row        (attention.py:24 + norm.py:12)
//   attention  fused softmax(q k^T * 64^-0.5) v                        (attention.py:20-34)
//   out GEMM   + bias + LN1(x) residual -> xm, row stats of xm         (attention.py:35, residual.py:9)
//   FC1 GEMM   A = xm, epilogue applies LN2 per row, + bias, GELU      (ffn.py:8)
//   FC2 GEMM   + bias + LN2(xm) residual -> x, row stats of x          (ffn.py:9, residual.py:9)
//
// Row statistics (sum, sum of squares) are written by the producing GEMM's epilogue as one partial
// per 128-column slab (stats slot) with plain stores; consumers sum the slots in a fixed order, so
// the forward is bitwise reproducible and needs no memsets.
#include "model.h"

using namespace evt;

namespace evt {

// Encoder weights (11 tensors per layer, 12 with the STANDARD qkv bias; evt_vit_num_weights
// order) for m->heads / m->ffn.
int build_encoder(evt_model* m, const float* const* w, hipStream_t s) {
  const int D = m->D;
  const int depth = (int)m->heads.size();
  const int qb = m->standard ? 1 : 0;  // qkv bias present
  m->layers.resize(depth);
  int k = 0;
  for (int i = 0; i < depth; ++i) {
    Layer& L = m->layers[i];
    L.heads = m->heads[i];
    L.hd = m->head_dim[i];
    L.inner = L.heads * L.hd;
    L.ffn = m->ffn[i];
    L.ffn_st = (int)round_up(L.ffn, PAD_N);
    EVT_RC(copy_vec(m, &L.ln1_g, w[k + 0], D, s));
    EVT_RC(copy_vec(m, &L.ln1_b, w[k + 1], D, s));
    if (m->mx8) {  // reference semantics only (validate): no qkv bias
      EVT_RC(copy_vec(m, &L.ln2_g, w[k + 5], D, s));
      EVT_RC(copy_vec(m, &L.ln2_b, w[k + 6], D, s));
      EVT_RC(make_mx8(m, &L.mqkv, w[k + 2], nullptr, D, 3 * L.inner, s));
      EVT_RC(make_mx8(m, &L.mout, w[k + 3], w[k + 4], L.inner, D, s));
      EVT_RC(make_mx8(m, &L.mfc1, w[k + 7], w[k + 8], D, L.ffn, s));
      EVT_RC(make_mx8(m, &L.mfc2, w[k + 9], w[k + 10], L.ffn, D, s));
      k += 11;
      continue;
    }
    EVT_RC(make_dense(m, &L.qkv, w[k + 2], qb ? w[k + 3] : nullptr, D, 3 * L.inner, s, w[k + 0],
                      w[k + 1]));
    k += qb;
    EVT_RC(make_dense(m, &L.out, w[k + 3], w[k + 4], L.inner, D, s));
    EVT_RC(copy_vec(m, &L.ln2_g, w[k + 5], D, s));
    EVT_RC(copy_vec(m, &L.ln2_b, w[k + 6], D, s));
    EVT_RC(make_dense(m, &L.fc1, w[k + 7], w[k + 8], D, L.ffn, s, w[k + 5], w[k + 6]));
    EVT_RC(make_dense(m, &L.fc2, w[k + 9], w[k + 10], L.ffn, D, s));
    k += 11;
  }
  return EVT_OK;
}

// Token-stream workspace of the encoder for B images (hbuf_bytes: the FFN hidden buffer), and the
// stream-K scratch of the model's GEMMs (its flag block zeroed once; kernels leave it zeroed).
void encoder_ws(const Shape& sh, int dtype, bool mx8, int B, size_t hbuf_bytes, WsLayout* l) {
  const size_t es = elem_size(dtype);
  if (dtype == DT_BF16)
    l->bufs.push_back({EVT_WS(sk), gemm_sk_bytes(), 4096, "memset stream-K flags"});
  const size_t rows = (size_t)B * sh.T;
  // x, xm (width D) and o (width heads * h_k) are GEMM A operands read in 64-column K-tiles: with
  // a width that is not a multiple of 64 a row's last K-tile runs into the next row (cancelled by
  // the zero-padded weight rows) and the last row into PAD_K zeroed slack elements; every byte is
  // zeroed once here (finite everywhere)
  const size_t xb = (rows * sh.D + PAD_K) * es, ob = (rows * sh.max_inner + PAD_K) * es;
  const size_t stats_bytes = rows * stats_slots(sh.D) * 2 * sizeof(float);
  l->bufs.push_back({EVT_WS(x), xb, xb, "memset x"});
  l->bufs.push_back({EVT_WS(xm), xb, xb, "memset xm"});
  l->bufs.push_back({EVT_WS(sx), stats_bytes});
  l->bufs.push_back({EVT_WS(sm), stats_bytes});
  l->bufs.push_back({EVT_WS(qkv), rows * 3 * sh.max_inner * es});
  l->bufs.push_back({EVT_WS(o), ob, ob, "memset o"});
  l->bufs.push_back({EVT_WS(hbuf), hbuf_bytes});
  l->hbuf_bytes = hbuf_bytes;
  // the CLS tail's FFN hidden rows (FC1 writes all ffn_st columns of a row before FC2 reads them)
  if (!mx8) l->bufs.push_back({EVT_WS(hc), (size_t)B * sh.max_ffn_st * es});
}

// Small-M, long-K Dense layers (the classifier head: M = batch) as K splits in one launch when the
// plain tile grid would leave most CUs idle; fp32 partials in the (then idle) hidden buffer.
int dense_head(const evt_model* m, const DenseW& w, const DenseCall& c, hipStream_t s) {
  const int tiles = ((c.M + GEMM_BM - 1) / GEMM_BM) * (w.npad / GEMM_BN);
  int S = 1;
  while (S < 8 && tiles * S * 2 <= device_cus() && w.kpad % (S * 2 * PAD_K) == 0) S *= 2;
  // sized for the handle's max_batch, not this call's M: whether the partials fit the hidden buffer
  // (they always do from about 20 tokens per image; 5-token models are where it matters) must not
  // depend on the batch, or one image alone and the same image in a batch take different sums
  const size_t part = (size_t)S * std::max(c.M, m->max_batch) * w.npad * sizeof(float);
  if (S < 2 || !m->ws.hbuf || part > m->ws.hbuf_bytes ||
      (c.flags & ~(EPI_BIAS | EPI_GELU | EPI_OUT_F32)))
    return dense(m, w, c, s);
  dense_work(m, w, c);
  const GemmParams p = gemm_operands(c.A, c.lda, w.w, w.kpad, w.npad, c.C, c.ldc, c.M, c.N, w.b,
                                     nullptr, 0, nullptr, 0, 0);
  EVT_HIP(gemm_splitk_launch(m->dtype, c.flags, p, S, (float*)m->ws.hbuf, s), "dense (split-K)");
  return EVT_OK;
}

// After a scheduled block's FC2 (include/evt_token_pruning.h): the CLS-attention scores of the q and
// k the block left in ws.qkv (`ap`), the K kept patch tokens, and the stream rows and statistics
// of the kept tokens packed from x / sx into xm / sm, idle at block end, whose roles then swap
// (vit_run puts the handle's pointers back when the call has been enqueued). Scores and the kept
// table live in the FFN hidden buffer, idle too, or where the call exports them. Three launches,
// counted under EVT_PROF_HEAD.
static int token_prune(evt_model* m, ForwardCall& call, const AttnParams& ap, int K, int entry) {
  const int B = call.B, T = ap.N, D = m->D, slots = stats_slots(D);
  hipStream_t s = call.s;
  const size_t sbytes = (size_t)round_up((int64_t)B * T * sizeof(float), 16);
  if (sbytes + (size_t)B * (K + 1) * sizeof(int32_t) > m->ws.hbuf_bytes)
    return fail(EVT_EINVAL, "token pruning: the FFN hidden buffer is too small for the scores");
  float* sc = (float*)m->ws.hbuf;
  int32_t* kept = (int32_t*)((char*)m->ws.hbuf + sbytes);
  if (const evt_token_pruning_args* a = call.tprune) {
    if (a->scores && a->scores[entry]) sc = a->scores[entry];
    if (a->kept && a->kept[entry]) kept = a->kept[entry];
  }
  const double es = (double)elem_size(m->dtype);
  {
    ProfScope ps(m, EVT_PROF_HEAD, s);
    const double nkb = (T + 63) / 64;  // pass 1 once per key block of an image, then the block
    prof_work(m, 2.0 * B * ap.H * 16.0 * (double)T * ap.hd * (nkb + 1),
              (double)B * ap.H * T * ap.hd * es * (nkb + 1) + 4.0 * B * T);
    EVT_HIP(token_scores_launch(m->dtype, ap, sc, s), "token scores");
  }
  {
    ProfScope ps(m, EVT_PROF_HEAD, s);
    prof_work(m, 0.0, 4.0 * B * (T + K + 1));
    EVT_HIP(token_select_launch(sc, B, T, K, kept, s), "token select");
  }
  {
    ProfScope ps(m, EVT_PROF_HEAD, s);
    prof_work(m, 0.0, 2.0 * B * (K + 1) * (D * es + slots * 8.0) + 4.0 * B * (K + 1));
    EVT_HIP(token_gather_launch(m->dtype, m->ws.x, m->ws.xm, m->ws.sx, m->ws.sm, slots, kept, B, T,
                                K + 1, D, s),
            "token gather");
  }
  std::swap(m->ws.x, m->ws.xm);
  std::swap(m->ws.sx, m->ws.sm);
  return EVT_OK;
}

// Encoder layers (transformer_encoder.py:13-18 / :26-34) on the token stream m->ws.x (+ stats sx).
// T tokens per image: sh.T until a block of the handle's token schedule, 1 + K_l after it.
//
// A skipped sublayer (evt_model_set_skips, include/evt_depth.h) launches nothing: the stream and
// its row statistics stay where they are and the x / xm and sx / sm roles swap for the rest of the
// call, as token_prune swaps them (vit_run puts the handle's pointers back), so the next consumer
// finds them under the name it reads. Whatever is skipped, a block leaves the stream in ws.x.
int run_encoder(evt_model* m, ForwardCall& call) {
  const int B = call.B, D = m->D;
  int T = m->sh.T, rows = B * T;
  hipStream_t s = call.s;
  const float log2e = 1.4426950408889634f;
  m->hm_layers = 0;
  m->tail_mode = 0;
  call.tprune_next = 0;
  // the block of the CLS tail: the last one that runs a sublayer (the last block, without skips)
  const int last_block = m->last_running();
  int block = 0;
  for (const Layer& L : m->layers) {
    const uint8_t skip = m->skip_of(block);
    const bool run_attn = !(skip & EVT_SKIP_ATTN), run_ffn = !(skip & EVT_SKIP_FFN);
    // The classifier and `pooled` read token 0 of the last block and nothing else, so its
    // out-proj, FC1 and FC2 run on the B CLS rows (the CLS tail, below) and its attention on query
    // tile 0. A call that exports the last block's token map (tokens, or a tap on it or on a
    // skipped block after it) runs the full-row block as well; the CLS rows it exports, and the
    // head reads, are still the tail's. The last block's FFN and stream statistics and its Grams are
    // those of the full-row launches (evt_ffn_stats.h, evt_depth.h, evt_gram.h).
    const bool last = block == last_block;
    // the call asks for this block's stream statistics (read here: the cursor moves on at the
    // block's FFN sublayer)
    const bool bs = call.bstats.wants(block);
    const bool full = !last || (call.feat && call.feat->tokens) || call.taps.reaches(block) ||
                      call.fstats.last_is(block) || call.grams.last_is(block) || bs;
    if (last) m->tail_mode = full ? 3 : 1;
    // The CLS tail's form of a launch: row b is row b T of the stream and statistics buffers, in
    // place (the head, and `pooled`, read them where they always did), the FFN hidden rows compact
    // in ws.hc, and the 128x128 kernel whatever B is (one image alone = the image in a batch). It
    // counts the layer's model work, or nothing where the full-row launch of the role did.
    auto tail = [&](DenseCall c) {
      c.M = B;
      if (c.A == m->ws.hbuf) c.A = m->ws.hc;
      else c.lda *= T;
      if (c.C == m->ws.hbuf) c.C = m->ws.hc;
      else c.ldc *= T;
      c.ldr *= T;
      c.stats_step = c.rs_step = T;
      c.force_nt = true;
      c.work_M = full ? -1 : rows;
      return c;
    };
    // out-proj / FC2 epilogue: + bias + LN(x) residual (+ stats); STANDARD: + x
    const int resid_flags = m->standard ? (EPI_BIAS | EPI_RESID | EPI_STATS)
                                        : (EPI_BIAS | EPI_RESID | EPI_RESLN | EPI_STATS);
    AttnParams ap{};
    if (run_attn) {
      const float scale_log2 = log2e / std::sqrt((float)L.hd);  // h_k^-0.5 (attention.py:13)
      // qkv head-major ([B][heads][q | k | v][T][64], EPI_HM) where the QKV GEMM takes the
      // persistent kernel (h_k = 64, bf16): an (image, head)'s q, k and v are three contiguous 25 KB
      // runs instead of T 128-B pieces at a 3 D-element stride each; token-major otherwise
      bool hm = false;
      {  // LN1-folded QKV (attention.py:24)
        ProfScope ps(m, EVT_PROF_QKV, s);
        DenseCall c;
        c.flags = EPI_LNIN | EPI_BIAS;
        c.A = m->ws.x; c.lda = D; c.C = m->ws.qkv; c.ldc = 3 * L.inner; c.M = rows; c.N = 3 * L.inner;
        c.stats_in = m->ws.sx;
        if (L.hd == 64 && m->headmajor) {
          DenseCall h = c;
          h.flags |= EPI_HM;
          h.ldc = 64;
          h.P = T;
          if (gemm_headmajor_ok(m->dtype, h.flags, dense_params(m, L.qkv, h))) {
            c = h;
            hm = true;
            ++m->hm_layers;
          }
        }
        EVT_RC(dense(m, L.qkv, c, s));
      }
      ap = AttnParams{m->ws.qkv, 3 * L.inner, m->ws.o, L.inner, T, L.heads, B, scale_log2};
      ap.hd = L.hd;
      if (hm) {
        ap.ldq = 64;
        ap.sb = (int64_t)L.heads * 3 * T * 64;
        ap.sh = (int64_t)3 * T * 64;
        ap.ko = T * 64;
        ap.vo = 2 * T * 64;
      }
      {
        ProfScope ps(m, EVT_PROF_ATTENTION, s);
        prof_work(m, 4.0 * B * L.heads * (double)T * T * L.hd,
                  (double)rows * 4 * L.inner * elem_size(m->dtype));  // qkv read + O written
        // (the model's work also where only query tile 0 runs: evt_model_profile_work)
        AttnParams aq = ap;
        aq.cls_only = !full && attention_cls_ok(m->dtype, ap);
        EVT_HIP(attention_launch(m->dtype, aq, s), "attention");
      }
      EVT_RC(attn_map(m, call, block, ap));
      EVT_RC(head_stats(m, call, block, ap));
      EVT_RC(rollout_step(m, call, block, ap));
      if (full) EVT_RC(gram_hook(m, call, block, EVT_GRAM_ATTN, m->ws.o, L.inner, rows, L.inner));
      // out-proj + bias + LN1(x) residual -> xm (+ stats); STANDARD: + x
      DenseCall co;
      co.flags = resid_flags;
      co.A = m->ws.o; co.lda = L.inner; co.C = m->ws.xm; co.ldc = D; co.M = rows; co.N = D;
      co.resid = m->ws.x; co.ldr = D; co.rstats = m->ws.sx; co.rgamma = L.ln1_g; co.rbeta = L.ln1_b;
      co.stats_out = m->ws.sm;
      // Each full-row launch comes before its role's tail launch: the tail's out-proj still finds
      // the block's input rows in x / sx, and what it, FC1 and FC2 leave in rows b T of xm / sm,
      // hc and x / sx is what the next tail launch, the exports and the head read.
      // The stream statistics of a block the call asks for (then `full`) read the full-row
      // launch's rows, so they run between the two.
      {
        ProfScope ps(m, EVT_PROF_OUT_PROJ, s);
        if (full) EVT_RC(dense(m, L.out, co, s));
        if (last && !bs) EVT_RC(dense(m, L.out, tail(co), s));
      }
      if (bs) {
        EVT_RC(block_stats(m, call, block, 0, m->ws.x, m->ws.xm, T));
        if (last) {
          ProfScope ps(m, EVT_PROF_OUT_PROJ, s);
          EVT_RC(dense(m, L.out, tail(co), s));
        }
      }
    } else {
      std::swap(m->ws.x, m->ws.xm);
      std::swap(m->ws.sx, m->ws.sm);
      EVT_RC(block_stats(m, call, block, 0, nullptr, nullptr, T));
    }
    if (run_ffn) {
      // LN2-folded FC1 + GELU (ffn.py:8; STANDARD: exact erf GELU)
      DenseCall c1;
      c1.flags = EPI_LNIN | EPI_BIAS | (m->standard ? EPI_GELU_ERF : EPI_GELU);
      c1.A = m->ws.xm; c1.lda = D; c1.C = m->ws.hbuf; c1.ldc = L.ffn_st; c1.M = rows; c1.N = L.ffn_st;
      c1.stats_in = m->ws.sm;
      // FC2 + bias + LN2(xm) residual -> x (+ stats); STANDARD: + xm
      DenseCall c2;
      c2.flags = resid_flags;
      c2.A = m->ws.hbuf; c2.lda = L.ffn_st; c2.C = m->ws.x; c2.ldc = D; c2.M = rows; c2.N = D;
      c2.resid = m->ws.xm; c2.ldr = D; c2.rstats = m->ws.sm; c2.rgamma = L.ln2_g; c2.rbeta = L.ln2_b;
      c2.stats_out = m->ws.sx;
      {
        ProfScope ps(m, EVT_PROF_FC1, s);
        if (full) EVT_RC(dense(m, L.fc1, c1, s));
        if (last) EVT_RC(dense(m, L.fc1, tail(c1), s));
      }
      if (full) EVT_RC(ffn_stats(m, call, block, L, rows));
      if (full) EVT_RC(gram_hook(m, call, block, EVT_GRAM_FFN, m->ws.hbuf, L.ffn_st, rows, L.ffn));
      {
        ProfScope ps(m, EVT_PROF_FC2, s);
        if (full) EVT_RC(dense(m, L.fc2, c2, s));
        if (last && !bs) EVT_RC(dense(m, L.fc2, tail(c2), s));
      }
      if (bs) {
        EVT_RC(block_stats(m, call, block, 1, m->ws.xm, m->ws.x, T));
        if (last) {
          ProfScope ps(m, EVT_PROF_FC2, s);
          EVT_RC(dense(m, L.fc2, tail(c2), s));
        }
      }
    } else {
      std::swap(m->ws.x, m->ws.xm);
      std::swap(m->ws.sx, m->ws.sm);
      EVT_RC(block_stats(m, call, block, 1, nullptr, nullptr, T));
    }
    EVT_RC(feat_tap(m, call, block, D, rows, D));
    if (call.tprune_next < (int)m->tp_blocks.size() && m->tp_blocks[call.tprune_next] == block) {
      const int K = m->tp_keep[call.tprune_next];
      EVT_RC(token_prune(m, call, ap, K, call.tprune_next++));
      T = K + 1;
      rows = B * T;
    }
    ++block;
  }
  call.T = T;
  return EVT_OK;
}

// MX8 encoder (reference semantics, transformer_encoder.py:13-18): per sublayer the LayerNorm
// runs in the quantizer (which keeps each row's (mu, rstd)), the Dense layers on the block-scaled
// MFMA, the residual LN(x) (norm.py:11-12 + residual.py:9) re-formed in the out-proj / FC2
// epilogues from x and those statistics; the attention and FC1 (GELU) outputs are quantized in
// their producing kernels' epilogues.
int run_encoder_mx8(evt_model* m, ForwardCall& call) {
  const int B = call.B, D = m->D, T = m->sh.T, rows = B * T;
  hipStream_t s = call.s;
  const float log2e = 1.4426950408889634f;
  const int dpad = (int)round_up(D, 128);
  for (const Layer& L : m->layers) {
    EVT_HIP(ln_mx8_launch(m->ws.x, rows, D, dpad, L.ln1_g, L.ln1_b, m->eps, m->ws.lnst, m->ws.qa,
                          m->ws.sa, s),
            "ln1 mx8");
    EVT_RC(dense_mx8(L.mqkv, EPI_BIAS, m->ws.qa, dpad, m->ws.sa, m->ws.qkv, 3 * L.inner, nullptr,
                     rows, nullptr, 0, s));
    // attention writes O straight as the MX8 operand of the out-proj (columns [inner, ipad) of
    // qa keep finite stale values, cancelled by the zero rows of the packed weights)
    const int ipad = L.mout.kpad;
    AttnParams ap{m->ws.qkv, 3 * L.inner, m->ws.o, L.inner, T, L.heads, B, 0.125f * log2e};
    ap.q8 = (uint8_t*)m->ws.qa;
    ap.s8 = m->ws.sa;
    ap.ldq8 = ipad;
    ap.rows8 = rows;
    EVT_HIP(attention_launch(DT_BF16, ap, s), "attention");
    EVT_RC(dense_mx8(L.mout, EPI_BIAS | EPI_RESID | EPI_RESLN, m->ws.qa, ipad, m->ws.sa, m->ws.xm,
                     D, nullptr, rows, m->ws.x, D, s, m->ws.lnst, L.ln1_g, L.ln1_b));
    EVT_HIP(ln_mx8_launch(m->ws.xm, rows, D, dpad, L.ln2_g, L.ln2_b, m->eps, m->ws.lnst, m->ws.qa,
                          m->ws.sa, s),
            "ln2 mx8");
    EVT_RC(dense_mx8(L.mfc1, EPI_BIAS | EPI_GELU | EPI_OUT_MX8, m->ws.qa, dpad, m->ws.sa, m->ws.qh,
                     m->ws.qh_ld, m->ws.shd, rows, nullptr, 0, s));
    EVT_RC(dense_mx8(L.mfc2, EPI_BIAS | EPI_RESID | EPI_RESLN, m->ws.qh, m->ws.qh_ld, m->ws.shd,
                     m->ws.x, D, nullptr, rows, m->ws.xm, D, s, m->ws.lnst, L.ln2_g, L.ln2_b));
  }
  return EVT_OK;
}

// The final token map and the pooled (CLS) vector of a ViT / T2T-ViT features forward, from the
// stream the last encoder block left in ws.x
int encoder_features(evt_model* m, const ForwardCall& call) {
  const evt_features_args* a = call.feat;
  const int B = call.B, D = m->D, T = call.T ? call.T : m->sh.T;
  hipStream_t s = call.s;
  const bool norm = m->norm_g != nullptr;  // REFERENCE ViT: no final LayerNorm (vit.py:54)
  if (a->tokens) EVT_RC(feat_export(m, m->ws.x, D, 1, a->tokens, norm, B * T, D, s));
  if (a->pooled) EVT_RC(feat_export(m, m->ws.x, D, T, a->pooled, norm, B, D, s));
  return EVT_OK;
}

}  // namespace evt
