// The model handle of libevt_hip.so (include/evt.h): what the three families share, lanes, graph
// capture, profiling and the features / image / attention-map / classification forwards.
#include "model.h"

using namespace evt;

namespace evt {

static thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  return fail(EVT_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

// EVT_QKV_LAYOUT=token (read when a model is created): keep the token-major qkv layout
bool qkv_headmajor_default() {
  const char* e = std::getenv("EVT_QKV_LAYOUT");
  return !(e && std::strcmp(e, "token") == 0);
}

void prof_reset(evt_model* m) {
  if (!m->prof) return;
  m->prof_role.clear();
  m->prof_gflop.clear();
  m->prof_gbytes.clear();
}
// add algorithmic work (flops, bytes) to the innermost open ProfScope of a profiled forward
void prof_work(const evt_model* m, double flops, double bytes) {
  if (!m->prof || m->prof_gflop.empty()) return;
  m->prof_gflop.back() += flops * 1e-9;
  m->prof_gbytes.back() += bytes * 1e-9;
}

int dev_alloc(evt_model* m, void** p, size_t bytes) {
  if (bytes == 0) bytes = 16;
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess)
    return fail(EVT_ENOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e));
  m->allocs.push_back(*p);
  return EVT_OK;
}

const FamilyOps& family_ops(const ModelCore& m) {
  static const FamilyOps* const table[] = {&vit_ops(), &t2t_ops(), &swin_ops()};  // by Family
  return *table[m.family];
}

int encoder_blocks(const ModelCore& m) { return (int)m.layers.size(); }

void encoder_shape(const ModelCore& m, int, int* tokens, int* width) {
  *tokens = m.sh.T;
  *width = m.D;
}

int alloc_ws(evt_model* m, int B, hipStream_t s) {
  const WsLayout l = family_ops(*m).workspace(*m, B);
  for (const WsBuf& b : l.bufs) {
    void** p = (void**)((char*)&m->ws + b.member);
    EVT_RC(dev_alloc(m, p, b.bytes));
    m->ws_bytes += b.bytes;
    if (b.zeroed) EVT_HIP(hipMemsetAsync(*p, 0, b.zeroed, s), b.what);
  }
  m->ws.hbuf_bytes = l.hbuf_bytes;
  m->ws.qa_ld = l.qa_ld;
  m->ws.qh_ld = l.qh_ld;
  if (l.patch_in_hbuf) m->ws.apatch = m->ws.hbuf;
  return EVT_OK;
}

// Pack a Keras [K, N] Dense kernel. With ln_g/ln_b (the LayerNorm in front of it), gamma is folded
// into the weight rows and b becomes c = beta . W + bias, with the column sums of the packed
// weights alongside (gemm.hip, "LayerNorm folding").
int make_dense(evt_model* m, DenseW* dw, const float* W, const float* bias, int K, int N,
               hipStream_t s, const float* ln_g, const float* ln_b) {
  const int dt = m->dtype;
  dw->K = K;
  dw->N = N;
  dw->kpad = (int)round_up(K, PAD_K);
  dw->npad = (int)round_up(N, PACK_N);
  EVT_RC(dev_alloc(m, &dw->w, (size_t)dw->kpad * dw->npad * elem_size(dt)));
  EVT_HIP(pack_weight(dt, W, ln_g, K, N, dw->w, dw->kpad, dw->npad, s), "pack_weight");
  if (ln_g) {
    EVT_RC(dev_alloc(m, (void**)&dw->b, (size_t)dw->npad * sizeof(float)));
    EVT_RC(dev_alloc(m, (void**)&dw->colsum, (size_t)dw->npad * sizeof(float)));
    EVT_HIP(ln_fold(dt, dw->w, dw->kpad, W, ln_b, bias, K, N, dw->colsum, dw->b, dw->npad, s),
            "ln_fold");
  } else if (bias) {
    EVT_RC(dev_alloc(m, (void**)&dw->b, (size_t)dw->npad * sizeof(float)));
    EVT_HIP(hipMemsetAsync(dw->b, 0, (size_t)dw->npad * sizeof(float), s), "memset bias");
    EVT_HIP(hipMemcpyAsync(dw->b, bias, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, s),
            "copy bias");
  }
  return EVT_OK;
}

int copy_vec(evt_model* m, float** dst, const float* src, size_t n, hipStream_t s) {
  EVT_RC(dev_alloc(m, (void**)dst, n * sizeof(float)));
  EVT_HIP(hipMemcpyAsync(*dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s), "copy vec");
  return EVT_OK;
}

// Pack a Keras [K, N] Dense kernel to MXFP8 (no LayerNorm folding: the MX8 model normalises in
// the quantizer). N is padded to 32 columns of zeros so an MX8 output covers whole blocks.
int make_mx8(evt_model* m, Mx8W* dw, const float* W, const float* bias, int K, int N,
             hipStream_t s) {
  dw->K = K;
  dw->N = (int)round_up(N, 32);
  dw->kpad = (int)round_up(K, 128);
  dw->npad = (int)round_up(N, 128);
  EVT_RC(dev_alloc(m, &dw->w, (size_t)dw->kpad * dw->npad));
  EVT_RC(dev_alloc(m, (void**)&dw->s, (size_t)dw->kpad / 128 * dw->npad * 4));
  EVT_HIP(mx8_pack_launch(W, nullptr, K, N, dw->w, dw->kpad, dw->npad, dw->s, s), "mx8_pack");
  EVT_RC(dev_alloc(m, (void**)&dw->b, (size_t)dw->npad * sizeof(float)));
  EVT_HIP(hipMemsetAsync(dw->b, 0, (size_t)dw->npad * sizeof(float), s), "memset bias");
  if (bias)
    EVT_HIP(hipMemcpyAsync(dw->b, bias, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, s),
            "copy bias");
  return EVT_OK;
}

int dense_mx8(const Mx8W& w, int flags, const void* A, int64_t lda, const uint32_t* as, void* C,
              int64_t ldc, uint32_t* cs, int M, const void* resid, int64_t ldr, hipStream_t s,
              const float* rstats, const float* rgamma, const float* rbeta) {
  Mx8GemmParams p{};
  p.A = (const uint8_t*)A; p.lda = lda; p.As = as; p.ldas = M;
  p.W = (const uint8_t*)w.w; p.ldw = w.kpad; p.Ws = w.s; p.ldws = w.npad;
  p.C = C; p.ldc = ldc; p.Cs = cs; p.ldcs = M;
  p.M = M; p.N = w.N; p.K = w.kpad;
  p.bias = w.b; p.resid = resid; p.ldr = ldr;
  p.rstats = rstats; p.rgamma = rgamma; p.rbeta = rbeta;
  EVT_HIP(gemm_mx8_launch(flags, p, s), "dense_mx8");
  return EVT_OK;
}

// Algorithmic work of one Dense launch: 2 M K N with the layer's real K and N; bytes = A and W
// read once, C written once, plus the residual, the row statistics read / written and the small
// bias / position vectors (what the kernel cannot avoid moving). A CLS-tail launch (work_M) counts
// the layer's model work, all B T rows, once per role: the reference's count, whatever rows ran.
void dense_work(const evt_model* m, const DenseW& w, const DenseCall& c) {
  if (!m->prof || c.work_M < 0) return;
  const double es = (double)elem_size(m->dtype);
  const double M = c.work_M ? c.work_M : c.M, K = w.K, N = std::min(c.N, w.N);
  const int width = c.ln_width ? c.ln_width : m->D;
  const double slot_row = (double)stats_slots(c.slot_width ? c.slot_width : width) * 8.0;
  double bytes = M * K * es + K * N * es + M * N * ((c.flags & EPI_OUT_F32) ? 4.0 : es) + 8.0 * N;
  if (c.flags & EPI_RESID) bytes += M * N * es;
  if (c.flags & EPI_LNIN) bytes += M * slot_row;
  if (c.flags & EPI_RESLN) bytes += M * slot_row + 8.0 * N;
  if (c.flags & EPI_STATS) bytes += M * slot_row;
  if (c.flags & EPI_POS) bytes += (double)(c.P + 1) * N * 4.0;
  prof_work(m, 2.0 * M * K * N, bytes);
}

GemmParams gemm_operands(const void* A, int64_t lda, const void* W, int Kpad, int Npad, void* C,
                         int64_t ldc, int M, int N, const float* bias, const void* resid,
                         int64_t ldr, const float* pos, int64_t ldp, int P) {
  GemmParams p{};
  p.A = A; p.lda = lda; p.W = W; p.ldw = Kpad; p.C = C; p.ldc = ldc;
  p.M = M; p.N = N; p.K = Kpad; p.ntiles = Npad / GEMM_BN;
  p.bias = bias; p.resid = resid; p.ldr = ldr; p.pos = pos; p.ldp = ldp; p.P = P;
  p.vec_ok = (ldc % 4 == 0) && (ldr % 4 == 0) && (ldp % 4 == 0);
  if (p.vec_ok && ldc % 8 == 0 && ldr % 8 == 0 && ldp % 8 == 0 &&
      (((uintptr_t)C | (uintptr_t)resid) & 15) == 0)
    p.vec_ok = 2;
  return p;
}

GemmParams dense_params(const evt_model* m, const DenseW& w, const DenseCall& c) {
  GemmParams p = gemm_operands(c.A, c.lda, w.w, w.kpad, w.npad, c.C, c.ldc, c.M, c.N, w.b,
                               c.resid, c.ldr, c.pos, c.ldp, c.P);
  p.colsum = w.colsum;
  p.no_balance = m->no_balance;
  p.stats_in = c.stats_in;
  p.rstats = c.rstats;
  p.rgamma = c.rgamma;
  p.rbeta = c.rbeta;
  p.stats_out = c.stats_out;
  const int width = c.ln_width ? c.ln_width : m->D;
  p.inv_d = 1.0f / (float)width;
  p.eps = m->eps;  // Keras LayerNormalization(epsilon=1e-5), reference norm.py:6
  p.nslots = stats_slots(c.slot_width ? c.slot_width : width);
  p.stats_step = c.stats_step;
  p.rs_step = c.rs_step;
  p.force_nt = c.force_nt;
  gemm_sk_bind(m->ws.sk, p);
  return p;
}

int dense(const evt_model* m, const DenseW& w, const DenseCall& c, hipStream_t s) {
  dense_work(m, w, c);
  const GemmParams p = dense_params(m, w, c);
  EVT_HIP(gemm_launch(m->dtype, c.flags, p, s), "dense");
  return EVT_OK;
}

// evt_forward_features: one stream-export launch (features.hip) of `rows` rows of width D, through
// the final LayerNorm when `norm`; counted under EVT_PROF_HEAD
int feat_export(evt_model* m, const void* x, int64_t ldx, int64_t row_step, float* out, bool norm,
                int rows, int D, hipStream_t s) {
  ProfScope ps(m, EVT_PROF_HEAD, s);
  prof_work(m, 0.0, (double)rows * D * (elem_size(m->dtype) + 4.0));
  EVT_HIP(export_rows_launch(m->dtype, x, ldx, row_step, out, norm ? m->norm_g : nullptr,
                             norm ? m->norm_b : nullptr, rows, D, m->eps, s),
          "feature export");
  return EVT_OK;
}

// After block `block` of a features forward, its output in ws.x: the tap, if one was asked for
int feat_tap(evt_model* m, ForwardCall& call, int block, int64_t ldx, int rows, int D) {
  float* out = call.taps.take(block);
  if (!out) return EVT_OK;
  return feat_export(m, m->ws.x, ldx, 1, out, call.feat->tap_norm != 0, rows, D, call.s);
}

// Right after block `block`'s attention kernel of an evt_forward_attention call, while ws.qkv still
// holds the block's q and k in the layout `ap` describes: the block's map, if one was asked for
// (attn_maps.hip; counted under EVT_PROF_HEAD like the feature exports)
int attn_map(evt_model* m, ForwardCall& call, int block, const AttnParams& ap) {
  float* out = call.maps.take(block);
  if (!out) return EVT_OK;
  const int nq = call.map_queries == EVT_ATTN_ALL ? ap.N : 1;
  ProfScope ps(m, EVT_PROF_HEAD, call.s);
  const double bh = (double)ap.B * ap.H;
  prof_work(m, 4.0 * bh * nq * (double)ap.N * ap.hd,  // the scores, twice
            bh * ((double)(nq + ap.N) * ap.hd * elem_size(m->dtype) + (double)nq * ap.N * 4.0));
  EVT_HIP(attn_probs_launch(m->dtype, ap, nq, out, call.s), "attention map");
  return EVT_OK;
}

// Columns of the patch grid behind an encoder's tokens 1 .. T - 1 (token 0 is the CLS token):
// image_size / patch_size for a ViT, image_size / 16 after T2T-ViT's three soft splits
static int patch_grid_w(const ModelCore& m) {
  return m.family == FAM_T2T ? m.image_size / 16 : m.image_size / m.patch_size;
}

// At the same point of an evt_forward_head_stats call: the block's four statistics per head, if they
// were asked for (attn_maps.hip; counted under EVT_PROF_HEAD)
int head_stats(evt_model* m, ForwardCall& call, int block, const AttnParams& ap) {
  float* out = call.hstats.take(block);
  if (!out) return EVT_OK;
  ProfScope ps(m, EVT_PROF_HEAD, call.s);
  const double bh = (double)ap.B * ap.H;
  prof_work(m, 4.0 * bh * ap.N * (double)ap.N * ap.hd,  // the scores, twice
            bh * (2.0 * ap.N * ap.hd * elem_size(m->dtype) + 4.0 * EVT_HEAD_STATS));
  EVT_HIP(head_stats_launch(m->dtype, ap, 1, patch_grid_w(*m), out, call.s), "head statistics");
  return EVT_OK;
}

// Between the full-row FC1 and FC2 of an evt_forward_ffn_stats call, while ws.hbuf holds block
// `block`'s hidden rows: the block's four statistics per neuron, if they were asked for
// (ffn_stats.hip; counted under EVT_PROF_HEAD)
int ffn_stats(evt_model* m, ForwardCall& call, int block, const Layer& L, int rows) {
  float* out = call.fstats.take(block);
  if (!out) return EVT_OK;
  ProfScope ps(m, EVT_PROF_HEAD, call.s);
  prof_work(m, 5.0 * rows * (double)L.ffn,  // |a|, three adds (one fused with a^2) and a max
            (double)rows * L.ffn * elem_size(m->dtype) + 4.0 * call.B * L.ffn * EVT_FFN_STATS);
  EVT_HIP(ffn_stats_launch(m->dtype, m->ws.hbuf, L.ffn_st, call.B, rows / call.B, L.ffn, out,
                           call.s),
          "ffn statistics");
  return EVT_OK;
}

// At the same point of an evt_forward_grams call for EVT_GRAM_FFN, and right after the attention
// kernel (ws.o) for EVT_GRAM_ATTN: the block's Gram and column sums, if they were asked for
// (gram.hip: one launch, or two through the call's scratch; counted under EVT_PROF_HEAD)
int gram_hook(evt_model* m, ForwardCall& call, int block, int which, const void* a, int64_t ld,
              int rows, int width) {
  if (!call.gram || call.gram->which != which || !call.grams.wants(block)) return EVT_OK;
  float* sums = call.gram->sums[call.grams.next];
  float* out = call.grams.take(block);
  ProfScope ps(m, EVT_PROF_HEAD, call.s);
  prof_work(m, 2.0 * rows * (double)width * width,
            (double)rows * width * elem_size(m->dtype) + 4.0 * width * (width + 1.0));
  EVT_HIP(gram_launch(m->dtype, a, ld, rows, width, out, sums, call.gram->scratch,
                      call.gram->scratch_bytes, call.s),
          "activation gram");
  return EVT_OK;
}

// At both sublayer ends of an evt_forward_block_stats call, while the sublayer's input rows `a`
// and output rows `b` are both resident (run_encoder): its four stream statistics, if the block
// is the next one asked for (depth_stats.hip; counted under EVT_PROF_HEAD). The per-chunk partials
// live in the FFN hidden buffer, idle at both points. A skipped sublayer (a == nullptr) gets the
// identity values by a strided copy from the handle's constant rows: no kernel.
int block_stats(evt_model* m, ForwardCall& call, int block, int sub, const void* a, const void* b,
                int T) {
  if (!call.bstats.wants(block)) return EVT_OK;
  float* out = call.bstats.out[call.bstats.next] + sub * EVT_DEPTH_STATS;
  if (sub == 1) ++call.bstats.next;
  const size_t row = EVT_DEPTH_STATS * sizeof(float);
  if (!a) {
    // the rows are the parent handle's (evt_model_set_skips): an analysis forward runs as one lane
    // on the handle's own workspace, never on a lane child, which has none
    if (!m->skip_ident)
      return fail(EVT_EINVAL, "block statistics: a lane child has no identity rows");
    EVT_HIP(hipMemcpy2DAsync(out, 2 * row, m->skip_ident, row, row, call.B,
                             hipMemcpyDeviceToDevice, call.s),
            "block statistics of a skipped sublayer");
    return EVT_OK;
  }
  if (stream_delta_part_bytes(call.B, T) > m->ws.hbuf_bytes)
    return fail(EVT_EINVAL, "block statistics: the FFN hidden buffer is too small for the partials");
  ProfScope ps(m, EVT_PROF_HEAD, call.s);
  const double rows = (double)call.B * T;
  prof_work(m, 8.0 * rows * m->D,  // four fused multiply-adds per element pair
            2.0 * rows * m->D * elem_size(m->dtype) + 4.0 * call.B * EVT_DEPTH_STATS);
  EVT_HIP(stream_delta_launch(m->dtype, a, m->D, b, m->D, call.B, T, m->D, out,
                              2 * EVT_DEPTH_STATS, (float*)m->ws.hbuf, call.s),
          "block statistics");
  return EVT_OK;
}

// Scratch layout of a rollout call (include/evt_rollout.h): the head mean, then up to two rollout
// buffers that alternate (a step cannot run in place); the last step writes the caller's output
static int rollout_bufs(int depth) { return 1 + std::min(depth - 1, 2); }

// At the same point of an evt_forward_rollout call, from block `start` on: the block's head mean
// into the scratch and one rollout step on it (attn_maps.hip, rollout.hip; two launches, counted
// under EVT_PROF_HEAD). Step 0 reads no rollout (R = I); the last block writes a->out, in
// EVT_ROLLOUT_CLS mode its row 0 alone.
int rollout_step(evt_model* m, ForwardCall& call, int block, const AttnParams& ap) {
  const evt_rollout_args* a = call.rollout;
  if (!a || block < a->start) return EVT_OK;
  const int step = block - a->start, N = ap.N;
  const bool last = block + 1 == (int)m->layers.size();
  const size_t buf = rollout_buf_bytes(ap.B, N);
  float* abar = (float*)a->scratch;
  auto r = [&](int i) { return (float*)((char*)a->scratch + (size_t)(1 + (i & 1)) * buf); };
  const int nq = last && a->mode == EVT_ROLLOUT_CLS ? 1 : N;
  ProfScope ps(m, EVT_PROF_HEAD, call.s);
  const double bh = (double)ap.B * ap.H, bnn = (double)ap.B * N * N;
  prof_work(m, 4.0 * bh * N * (double)N * ap.hd + (step ? 2.0 * ap.B * nq * (double)N * N : 0.0),
            bh * 2.0 * N * ap.hd * elem_size(m->dtype) + 4.0 * (2.0 * bnn + (step ? bnn : 0.0)) +
                4.0 * ap.B * nq * (double)N * (step ? 2.0 : 1.0));
  EVT_HIP(head_mean_launch(m->dtype, ap, abar, call.s), "rollout head mean");
  EVT_HIP(rollout_step_launch(abar, step ? r(step - 1) : nullptr, last ? a->out : r(step), ap.B, N,
                              nq, call.s),
          "rollout step");
  return EVT_OK;
}

// The Swin counterpart (evt_forward_window_attention): while ws.qkv holds block `block`'s LN1-folded
// QKV rows that `ap` describes, the block's window map, if it is the next one asked for
int window_attn_map(evt_model* m, ForwardCall& call, int block, int w, const SwinAttnParams& ap) {
  float* out = call.maps.take(block);
  if (!out) return EVT_OK;
  ProfScope ps(m, EVT_PROF_HEAD, call.s);
  const double n = (double)w * w, wh = (double)ap.B * ap.nwx * ap.nwx * ap.H;
  prof_work(m, 2.0 * wh * n * n * 32,  // the scores
            wh * (2.0 * n * 32 * elem_size(m->dtype) + n * n * 4.0));
  EVT_HIP(window_probs_launch(m->dtype, w, ap, out, call.s), "window attention map");
  return EVT_OK;
}

// T_l of block `block` under m's token schedule: the tokens per image the block runs on
int tokens_at(const ModelCore& m, int block) {
  int T = m.sh.T;
  for (size_t i = 0; i < m.tp_blocks.size() && m.tp_blocks[i] < block; ++i) T = m.tp_keep[i] + 1;
  return T;
}

int no_token_schedule(const evt_model* m, const char* what) {
  if (m->tp_blocks.empty()) return EVT_OK;
  return fail(EVT_EINVAL, std::string(what) + " is not available while a token schedule is set: "
                          "the stream drops tokens between blocks (clear it with "
                          "evt_model_set_token_schedule(m, 0, ...))");
}

int finish_create(evt_model* m, int rc, evt_model** out) {
  if (rc) {
    std::string keep = g_err;
    evt_model_destroy(m);
    g_err = keep;
    return rc;
  }
  *out = m;
  return EVT_OK;
}

static int lanes_forward(evt_model* m, const ForwardCall& call) {
  // the joins go onto s after every lane's work: a lane stream that shares s's hardware queue
  // would otherwise queue its kernels behind s's wait for the previous lane (measured: lanes
  // serialised in part)
  const int k = (int)m->lanes.size(), B = call.B;
  hipStream_t s = call.s;
  EVT_HIP(hipEventRecord(m->lane_ev[0], s), "lanes fork");
  for (int i = 0; i < k; ++i)
    EVT_HIP(hipStreamWaitEvent(m->lane_s[i], m->lane_ev[0], 0), "lane fork wait");
  for (int i = 0; i < k; ++i) {
    const int b0 = (int)((int64_t)B * i / k), b1 = (int)((int64_t)B * (i + 1) / k);
    if (b1 > b0) {
      ForwardCall lane = call.slice(b0, b1, m->img_elems, m->num_classes, m->lane_s[i]);
      EVT_RC(family_ops(*m).run(m->lanes[i], lane));
    }
    EVT_HIP(hipEventRecord(m->lane_ev[1 + i], m->lane_s[i]), "lane done");
  }
  for (int i = 0; i < k; ++i)
    EVT_HIP(hipStreamWaitEvent(s, m->lane_ev[1 + i], 0), "lanes join");
  m->hm_layers = m->lanes[0]->hm_layers;
  m->tail_mode = m->lanes[0]->tail_mode;
  return EVT_OK;
}

int check_batch(const evt_model* m, int B) {
  if (B <= 0 || B > m->max_batch)
    return fail(EVT_EINVAL, "batch must be in [1, max_batch=" + std::to_string(m->max_batch) + "]");
  return EVT_OK;
}

// Every forward, eager or captured: over the lanes when the caller asked for them (logits-only
// forwards do), the handle has lanes, is not profiling (profiling: one lane) and every lane gets
// an image; on this handle's own workspace otherwise.
int forward(evt_model* m, ForwardCall& call, bool use_lanes) {
  EVT_RC(check_batch(m, call.B));
  if (use_lanes && !m->lanes.empty() && !m->prof && call.B >= (int)m->lanes.size())
    return lanes_forward(m, call);
  return family_ops(*m).run(m, call);
}

// What evt_{vit,t2t,swin}_forward are: the argument checks, then the forward of an fp32 batch
int family_forward(evt_model* m, int family, const char* wrong_family, const float* img, int B,
                   float* logits, void* stream) {
  if (!m || !img || !logits) return fail(EVT_EINVAL, "model, img and logits must be non-null");
  if (m->family != family) return fail(EVT_EINVAL, wrong_family);
  ForwardCall call;
  call.img = img; call.B = B; call.logits = logits; call.s = (hipStream_t)stream;
  return forward(m, call, true);
}

int affine_from(const float* scale, const float* shift, int C, ImgAffine* aff,
                const char* what) {
  if (C < 1 || C > 4) return fail(EVT_EINVAL, std::string(what) + ": uint8 images have 1 to 4 channels");
  if (!scale || !shift) return fail(EVT_EINVAL, std::string(what) + ": scale and shift must be non-null");
  *aff = ImgAffine{};
  for (int c = 0; c < C; ++c) {
    if (!std::isfinite(scale[c]) || !std::isfinite(shift[c]))
      return fail(EVT_EINVAL, std::string(what) + ": scale and shift must be finite");
    aff->scale[c] = scale[c];
    aff->shift[c] = shift[c];
  }
  return EVT_OK;
}

}  // namespace evt

extern "C" {

int evt_init(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return fail(EVT_ENODEV, "no HIP device visible");
  if (device < 0 || device >= n) return fail(EVT_ENODEV, "device index out of range");
  hipDeviceProp_t prop;
  EVT_HIP(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(EVT_ENODEV, std::string("device is ") + prop.gcnArchName + ", this build is gfx950");
  EVT_HIP(hipSetDevice(device), "hipSetDevice");
  return EVT_OK;
}

const char* evt_last_error(void) { return g_err.c_str(); }

// evt_model_set_lanes: the children (their workspaces), streams and events of a model
static void release_lanes(evt_model* m) {
  for (evt_model* c : m->lanes) evt_model_destroy(c);
  for (size_t i = 0; i < m->lane_s.size(); ++i)
    if (m->lane_own[i]) (void)hipStreamDestroy(m->lane_s[i]);
  for (hipEvent_t e : m->lane_ev) (void)hipEventDestroy(e);
  m->lanes.clear();
  m->lane_s.clear();
  m->lane_own.clear();
  m->lane_ev.clear();
}

int evt_model_destroy(evt_model* m) {
  if (!m) return EVT_OK;
  // forwards enqueued on any stream may still read the workspace / weights: wait for the device
  // before freeing (hipFree would also synchronise, but only implicitly)
  (void)hipDeviceSynchronize();
  release_lanes(m);
  if (m->graph_exec) (void)hipGraphExecDestroy(m->graph_exec);
  if (m->graph) (void)hipGraphDestroy(m->graph);
  for (hipEvent_t e : m->prof_ev) (void)hipEventDestroy(e);
  for (void* p : m->allocs) (void)hipFree(p);
  delete m;
  return EVT_OK;
}

int evt_model_profile(evt_model* m, int enable) {
  if (!m) return fail(EVT_EINVAL, "model is NULL");
  if (m->graph && enable) return fail(EVT_EINVAL, "profiling a model with a captured graph");
  m->prof = enable != 0;
  m->prof_role.clear();
  m->prof_gflop.clear();
  m->prof_gbytes.clear();
  return EVT_OK;
}

int evt_model_profile_read(evt_model* m, float* us, int* launches) {
  if (!m || !us || !launches) return fail(EVT_EINVAL, "null argument");
  for (int r = 0; r < EVT_PROF_ROLES; ++r) {
    us[r] = 0.f;
    launches[r] = 0;
  }
  for (size_t i = 0; i < m->prof_role.size(); ++i) {
    EVT_HIP(hipEventSynchronize(m->prof_ev[2 * i + 1]), "profile sync");
    float ms = 0.f;
    EVT_HIP(hipEventElapsedTime(&ms, m->prof_ev[2 * i], m->prof_ev[2 * i + 1]), "profile read");
    us[m->prof_role[i]] += 1000.f * ms;
    launches[m->prof_role[i]] += 1;
  }
  return EVT_OK;
}

int evt_model_qkv_layout(const evt_model* m, int* headmajor_layers) {
  if (!m || !headmajor_layers) return fail(EVT_EINVAL, "null argument");
  *headmajor_layers = m->hm_layers;
  return EVT_OK;
}

int evt_model_tail_mode(const evt_model* m, int* mode) {
  if (!m || !mode) return fail(EVT_EINVAL, "null argument");
  *mode = m->tail_mode;
  return EVT_OK;
}

int evt_model_set_lanes(evt_model* m, int lanes, void* stream) {
  if (!m) return fail(EVT_EINVAL, "model is NULL");
  if (m->is_lane) return fail(EVT_EINVAL, "the model is a lane of another model");
  if (lanes < 1 || lanes > 4) return fail(EVT_EINVAL, "lanes must be in [1, 4]");
  if (m->graph) return fail(EVT_EINVAL, "set the lanes before evt_graph_capture");
  (void)hipDeviceSynchronize();  // forwards of the current lanes may still be running
  release_lanes(m);
  if (lanes == 1) return EVT_OK;
  hipStream_t s = (hipStream_t)stream;
  const int per = (m->max_batch + lanes - 1) / lanes;
  auto run = [&]() -> int {
    for (int i = 0; i < lanes; ++i) {
      // a fresh handle with a copy of the parent's core: it shares the weights (whose allocations
      // stay the parent's) and nothing else, and allocates its own workspace for `per` images
      evt_model* c = new evt_model();
      static_cast<ModelCore&>(*c) = *m;
      c->bind_desc();
      c->is_lane = true;
      c->max_batch = per;
      c->no_balance = m->family == FAM_T2T ? 1 : 0;
      m->lanes.push_back(c);
      EVT_RC(alloc_ws(c, per, s));
      hipStream_t st = nullptr;
      EVT_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "lane stream");
      m->lane_s.push_back(st);
      m->lane_own.push_back(1);
    }
    for (int i = 0; i <= lanes; ++i) {
      hipEvent_t e = nullptr;
      EVT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming), "lane event");
      m->lane_ev.push_back(e);
    }
    EVT_HIP(hipStreamSynchronize(s), "lanes sync");
    return EVT_OK;
  };
  const int rc = run();
  if (rc) {
    const std::string keep = g_err;
    (void)hipDeviceSynchronize();
    release_lanes(m);
    g_err = keep;
  }
  return rc;
}

int evt_model_set_lane_streams(evt_model* m, int n, void* const* streams) {
  if (!m || !streams) return fail(EVT_EINVAL, "null argument");
  if (m->lanes.empty() || n != (int)m->lanes.size())
    return fail(EVT_EINVAL, "n must equal the lane count (evt_model_set_lanes first)");
  for (int i = 0; i < n; ++i)
    if (!streams[i]) return fail(EVT_EINVAL, "lane streams must be non-NULL");
  if (m->graph) return fail(EVT_EINVAL, "set the lane streams before evt_graph_capture");
  (void)hipDeviceSynchronize();
  for (int i = 0; i < n; ++i) {
    if (m->lane_own[i]) (void)hipStreamDestroy(m->lane_s[i]);
    m->lane_s[i] = (hipStream_t)streams[i];
    m->lane_own[i] = 0;
  }
  return EVT_OK;
}

int evt_model_lanes(const evt_model* m, int* lanes) {
  if (!m || !lanes) return fail(EVT_EINVAL, "null argument");
  *lanes = m->lanes.empty() ? 1 : (int)m->lanes.size();
  return EVT_OK;
}

int evt_model_workspace_bytes(const evt_model* m, size_t* bytes) {
  if (!m || !bytes) return fail(EVT_EINVAL, "null argument");
  *bytes = m->ws_bytes;
  for (const evt_model* c : m->lanes) *bytes += c->ws_bytes;
  return EVT_OK;
}

int evt_model_profile_work(evt_model* m, double* gflop, double* gbytes) {
  if (!m || !gflop || !gbytes) return fail(EVT_EINVAL, "null argument");
  for (int r = 0; r < EVT_PROF_ROLES; ++r) gflop[r] = gbytes[r] = 0.0;
  for (size_t i = 0; i < m->prof_role.size(); ++i) {
    gflop[m->prof_role[i]] += m->prof_gflop[i];
    gbytes[m->prof_role[i]] += m->prof_gbytes[i];
  }
  return EVT_OK;
}

// Capture what `enqueue` puts on `stream` as the model's graph (evt_graph_capture[_image])
static int graph_capture(evt_model* m, void* stream, const std::function<int()>& enqueue) {
  if (!m || !stream) return fail(EVT_EINVAL, "graph capture needs a model and a non-NULL stream");
  if (m->prof)  // the events would be captured into the graph, never recorded on the stream
    return fail(EVT_EINVAL, "graph capture while profiling is enabled (evt_model_profile(m, 0) first)");
  hipStream_t s = (hipStream_t)stream;
  if (m->graph_exec) {
    (void)hipGraphExecDestroy(m->graph_exec);
    m->graph_exec = nullptr;
  }
  if (m->graph) {
    (void)hipGraphDestroy(m->graph);
    m->graph = nullptr;
  }
  EVT_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal), "begin capture");
  const int rc = enqueue();
  hipGraph_t g = nullptr;
  const hipError_t e = hipStreamEndCapture(s, &g);
  if (rc) {
    if (g) (void)hipGraphDestroy(g);
    return rc;
  }
  if (e != hipSuccess) return hip_fail(e, "end capture");
  hipGraphExec_t ge = nullptr;
  const hipError_t ei = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  if (ei != hipSuccess) {
    (void)hipGraphDestroy(g);
    return hip_fail(ei, "graph instantiate");
  }
  m->graph = g;
  m->graph_exec = ge;
  return EVT_OK;
}

int evt_graph_capture(evt_model* m, const float* img, int batch, float* logits, void* stream) {
  return graph_capture(m, stream, [&]() {  // any family: the handle's own
    return family_forward(m, m->family, "", img, batch, logits, stream);
  });
}

int evt_graph_launch(evt_model* m, void* stream) {
  if (!m || !m->graph_exec) return fail(EVT_EINVAL, "no captured graph (call evt_graph_capture)");
  EVT_HIP(hipGraphLaunch(m->graph_exec, (hipStream_t)stream), "graph launch");
  return EVT_OK;
}

// ---- feature outputs (include/evt_features.h) ---------------------------------------------

static int model_blocks(const evt_model* m) { return family_ops(*m).blocks(*m); }

int evt_features_shape(const evt_model* m, int* F, int* T, int* n_blocks) {
  if (!m) return fail(EVT_EINVAL, "model is NULL");
  int tokens = 0, width = 0;
  family_ops(*m).shape(*m, -1, &tokens, &width);
  if (F) *F = width;
  if (T) *T = tokens;
  if (n_blocks) *n_blocks = model_blocks(m);
  return EVT_OK;
}

int evt_tap_shape(const evt_model* m, int block, int* tokens, int* width) {
  if (!m || !tokens || !width) return fail(EVT_EINVAL, "null argument");
  if (block < 0 || block >= model_blocks(m))
    return fail(EVT_EINVAL, "block must be in [0, " + std::to_string(model_blocks(m)) + ")");
  family_ops(*m).shape(*m, block, tokens, width);
  return EVT_OK;
}

// One per-block output list of a public args struct with the nouns of its messages: the count
// field, the two arrays, a block, the block list, a pointer, and what must be aligned
struct BlockList {
  int n;
  const int32_t* blocks;
  float* const* out;
  const char *count, *arrays, *block, *list, *pointer, *aligned;
  BlockCursor cursor() const { return BlockCursor{blocks, out, n}; }
};

static int check_count(const BlockList& l) {
  if (l.n < 0 || l.n > 64) return fail(EVT_EINVAL, std::string(l.count) + " must be in [0, 64]");
  return EVT_OK;
}

// The entries of a list whose count is in range, on a model of nb blocks: the arrays, `refused`
// (why this model takes no such list, or null), then entry by entry the block in [0, nb) and above
// the one before, the pointer non-null and 16-byte aligned. With `bits` the pointers are or-ed
// into it instead, for the caller's one alignment check after the list (the feature outputs).
static int check_blocks(const BlockList& l, int nb, const char* refused, uintptr_t* bits) {
  if (l.n == 0) return EVT_OK;
  if (!l.blocks || !l.out)
    return fail(EVT_EINVAL, std::string(l.count) + " > 0 needs the " + l.arrays + " arrays");
  if (refused) return fail(EVT_EINVAL, refused);
  for (int i = 0; i < l.n; ++i) {
    if (l.blocks[i] < 0 || l.blocks[i] >= nb)
      return fail(EVT_EINVAL, std::string(l.block) + " " + std::to_string(l.blocks[i]) +
                                  " is outside [0, " + std::to_string(nb) + ")");
    if (i > 0 && l.blocks[i] <= l.blocks[i - 1])
      return fail(EVT_EINVAL, std::string(l.list) + " must be strictly increasing");
    if (!l.out[i])
      return fail(EVT_EINVAL, std::string(l.pointer) + " " + std::to_string(i) + " is NULL");
    if (bits) *bits |= (uintptr_t)l.out[i];
    else if ((uintptr_t)l.out[i] & 15)
      return fail(EVT_EINVAL, std::string(l.aligned) + " must be 16-byte aligned");
  }
  return EVT_OK;
}

// The entries of a validated list on a handle with skips (include/evt_depth.h): EVT_EINVAL naming
// the skip if one of them is a block whose sublayer `bit` (EVT_SKIP_ATTN / _FFN) is skipped
static int no_skipped(const evt_model* m, const BlockList& l, int bit) {
  for (int i = 0; i < l.n; ++i)
    if (m->skip_of(l.blocks[i]) & bit)
      return fail(EVT_EINVAL, std::string(l.block) + " " + std::to_string(l.blocks[i]) + ": the " +
                                  "block's " + (bit == EVT_SKIP_ATTN ? "attention" : "FFN") +
                                  " sublayer is skipped (evt_model_set_skips), it computes nothing");
  return EVT_OK;
}

static BlockList tap_list(const evt_features_args* a) {
  return {a->n_taps, a->tap_blocks, a->taps, "n_taps", "tap_blocks and taps", "tap block",
          "tap_blocks", "tap pointer", "feature outputs"};
}

// What evt_forward_features checks of (model, outputs, batch); evt_forward_image shares it
static int validate_features(const evt_model* m, const evt_features_args* a, int B) {
  const BlockList taps = tap_list(a);
  EVT_RC(check_count(taps));
  if (!a->logits && !a->pooled && !a->tokens && a->n_taps == 0)
    return fail(EVT_EINVAL, "no output requested: logits, pooled and tokens are NULL, n_taps is 0");
  EVT_RC(check_batch(m, B));  // (here, ahead of forward's own: the order the checks fire in)
  if (a->tokens) EVT_RC(no_token_schedule(m, "the final token map (tokens)"));
  if (a->n_taps > 0) EVT_RC(no_token_schedule(m, "a block tap"));
  if (a->tap_norm != 0 && a->tap_norm != 1) return fail(EVT_EINVAL, "tap_norm must be 0 or 1");
  if (a->tap_norm && (m->family == FAM_SWIN || !m->norm_g))
    return fail(EVT_EINVAL, m->family == FAM_SWIN
                                ? "tap_norm: Swin stage widths differ from the final LayerNorm's"
                                : "tap_norm: a REFERENCE ViT has no final LayerNorm");
  // one alignment check of every output, after the tap list (16-B stores, features.hip)
  uintptr_t align = (uintptr_t)a->pooled | (uintptr_t)a->tokens;
  EVT_RC(check_blocks(taps, model_blocks(m),
                      m->mx8 ? "taps are not available on an EVT_DTYPE_MX8 model" : nullptr, &align));
  if (align & 15) return fail(EVT_EINVAL, std::string(taps.aligned) + " must be 16-byte aligned");
  return EVT_OK;
}

int evt_forward_features(evt_model* m, const float* img, int B, const evt_features_args* a,
                         void* stream) {
  if (!m || !img || !a) return fail(EVT_EINVAL, "model, img and args must be non-null");
  EVT_RC(validate_features(m, a, B));
  ForwardCall call;
  call.img = img; call.B = B; call.logits = a->logits; call.s = (hipStream_t)stream;
  call.set_feat(a);
  // one lane, on this handle's own workspace, whatever its lane count (as a profiled forward)
  return forward(m, call, false);
}

// ---- uint8 image input (include/evt_image.h) ------------------------------------------------

// The descriptor alone (no model needed), then what the model adds for EVT_IMG_U8_NHWC
static int validate_image(const evt_model* m, const evt_image_args* in, ImgAffine* aff) {
  if (!in) return fail(EVT_EINVAL, "image descriptor is NULL");
  if (!in->data) return fail(EVT_EINVAL, "image data is NULL");
  if (in->format != EVT_IMG_F32 && in->format != EVT_IMG_U8_NHWC)
    return fail(EVT_EINVAL, "unknown image format " + std::to_string(in->format));
  if (!m) return fail(EVT_EINVAL, "model is NULL");
  if (in->format == EVT_IMG_F32) return EVT_OK;
  const int C = m->in_chans, S = m->image_size;
  if (C > 4) return fail(EVT_EINVAL, "uint8 input: in_chans must be <= 4");
  EVT_RC(affine_from(in->scale, in->shift, C, aff, "uint8 input"));
  const uintptr_t a = (uintptr_t)in->data;
  if (m->family == FAM_T2T) return (C == 4 && (a & 3)) ? fail(EVT_EINVAL, "uint8 input: data must be 4-byte aligned") : EVT_OK;
  const int ps = m->patch_size;
  if (((int64_t)ps * S * C) % 4)
    return fail(EVT_EINVAL, "uint8 input: patch_size*image_size*in_chans must be a multiple of 4");
  if (m->family == FAM_VIT && !m->patch_cm && !m->patch_ld)
    return fail(EVT_EINVAL, "uint8 input: this ViT's patch vectors are not channel-major "
                            "(patch_size % 8 != 0 with patch_size^2*in_chans % 64 == 0)");
  // lanes start at multiples of S*S*C bytes: a multiple of 4 (and of 16 for the fused stem)
  const bool stem96 = m->family == FAM_SWIN && m->dtype == DT_BF16 && C == 3 && ps == 4 &&
                      m->stages[0].C == 96 && S % 16 == 0 && S <= 256 && m->stages[0].w == 7;
  if (a & (stem96 ? 15 : 3))
    return fail(EVT_EINVAL, stem96 ? "uint8 input: data must be 16-byte aligned (fused Swin stem)"
                                   : "uint8 input: data must be 4-byte aligned");
  return EVT_OK;
}

// A call of B images from a validated image descriptor (aff: validate_image's; uint8 only reads it)
static ForwardCall image_call(const evt_image_args* in, const ImgAffine& aff, int B, float* logits,
                              void* stream) {
  ForwardCall call;
  if (in->format == EVT_IMG_F32) call.img = (const float*)in->data;
  else call.img8 = (const uint8_t*)in->data;
  call.aff = aff; call.B = B; call.logits = logits; call.s = (hipStream_t)stream;
  return call;
}

// The forward of evt_forward_image and evt_forward_classify from validated arguments. Logits alone:
// over the handle's lanes, like evt_*_forward; anything more: a features forward, as one lane
static int image_forward(evt_model* m, const evt_image_args* in, const ImgAffine& aff, int B,
                         const evt_features_args* a, void* stream) {
  const bool logits_only = a->logits && !a->pooled && !a->tokens && a->n_taps == 0;
  ForwardCall call = image_call(in, aff, B, a->logits, stream);
  if (!logits_only) call.set_feat(a);
  return forward(m, call, logits_only);
}

int evt_forward_image(evt_model* m, const evt_image_args* in, int B, const evt_features_args* a,
                      void* stream) {
  ImgAffine aff{};
  if (!a) return fail(EVT_EINVAL, "image descriptor, outputs and model must be non-null");
  EVT_RC(validate_image(m, in, &aff));
  EVT_RC(validate_features(m, a, B));
  return image_forward(m, in, aff, B, a, stream);
}

// What the analysis forwards below open with, after their own null check: the image descriptor,
// the family (`family` fails with the reason it is refused), the token schedule (refused under the
// name `no_schedule` unless that is null), `list`'s count and "no output" (list: the call's own
// block list, or null), then feat's outputs or, without feat, the batch. On EVT_OK *call is the
// call, feat set; it runs as one lane on the handle's own workspace, whatever its lane count (as
// a features forward).
static int analysis_call(evt_model* m, const evt_image_args* in, int B,
                         const evt_features_args* feat, void* stream,
                         int (*family)(const evt_model*), const char* no_schedule,
                         const BlockList* list, ForwardCall* call) {
  ImgAffine aff{};
  EVT_RC(validate_image(m, in, &aff));
  EVT_RC(family(m));
  if (no_schedule) EVT_RC(no_token_schedule(m, no_schedule));
  if (list) {
    EVT_RC(check_count(*list));
    if (list->n == 0 && !feat)
      return fail(EVT_EINVAL, std::string("no output requested: ") + list->count +
                                  " is 0 and feat is NULL");
  }
  if (feat) EVT_RC(validate_features(m, feat, B));
  else EVT_RC(check_batch(m, B));
  *call = image_call(in, aff, B, feat ? feat->logits : nullptr, stream);
  call->set_feat(feat);
  return EVT_OK;
}

int evt_graph_capture_image(evt_model* m, const evt_image_args* in, int B, float* logits,
                            void* stream) {
  ImgAffine aff{};
  EVT_RC(validate_image(m, in, &aff));
  if (in->format == EVT_IMG_F32)
    return evt_graph_capture(m, (const float*)in->data, B, logits, stream);
  if (!logits || !stream)
    return fail(EVT_EINVAL, "graph capture needs logits and a non-NULL stream");
  EVT_RC(check_batch(m, B));  // ahead of the capture's own checks, and of the previous graph's end
  ForwardCall call = image_call(in, aff, B, logits, stream);
  return graph_capture(m, stream, [&]() { return forward(m, call, true); });
}

// ---- attention-map outputs (include/evt_attention_maps.h) -----------------------------------

static int attn_family(const evt_model* m) {
  if (const char* why = family_ops(*m).no_attn_maps) return fail(EVT_EINVAL, why);
  if (m->mx8) return fail(EVT_EINVAL, "attention maps are not available on an EVT_DTYPE_MX8 model");
  return EVT_OK;
}

int evt_attn_map_shape(const evt_model* m, int block, int* heads, int* tokens) {
  if (!m || !heads || !tokens) return fail(EVT_EINVAL, "null argument");
  EVT_RC(attn_family(m));
  if (block < 0 || block >= (int)m->layers.size())
    return fail(EVT_EINVAL, "block must be in [0, " + std::to_string(m->layers.size()) + ")");
  *heads = m->layers[block].heads;
  *tokens = m->sh.T;
  return EVT_OK;
}

// An attention call (evt_forward_attention, or the window maps) on a model of nb blocks, from the
// null check on. cls_ok: EVT_ATTN_CLS is a mode of the call (evt_forward_attention) or not.
static int attention_forward(evt_model* m, const evt_image_args* in, int B,
                             const evt_features_args* feat, const evt_attn_args* a, void* stream,
                             int (*family)(const evt_model*), const char* no_schedule, bool cls_ok) {
  const BlockList maps = {a->n_maps, a->blocks, a->maps, "n_maps", "blocks and maps", "map block",
                          "map blocks", "map pointer", "attention maps"};
  ForwardCall call;
  EVT_RC(analysis_call(m, in, B, feat, stream, family, no_schedule, &maps, &call));
  if (!cls_ok && a->queries != EVT_ATTN_ALL)
    return fail(EVT_EINVAL, "window attention maps: queries must be EVT_ATTN_ALL");
  if (a->queries != EVT_ATTN_CLS && a->queries != EVT_ATTN_ALL)
    return fail(EVT_EINVAL, "queries must be EVT_ATTN_CLS or EVT_ATTN_ALL");
  EVT_RC(check_blocks(maps, model_blocks(m), nullptr, nullptr));
  EVT_RC(no_skipped(m, maps, EVT_SKIP_ATTN));
  call.maps = maps.cursor();
  call.map_queries = a->queries;
  return forward(m, call, false);
}

int evt_forward_attention(evt_model* m, const evt_image_args* in, int B,
                          const evt_features_args* feat, const evt_attn_args* a, void* stream) {
  if (!m || !in || !a) return fail(EVT_EINVAL, "model, image descriptor and attn must be non-null");
  return attention_forward(m, in, B, feat, a, stream, attn_family, "evt_forward_attention", true);
}

// ---- head statistics (include/evt_head_stats.h) ---------------------------------------------

// Why m has no head statistics (its patch tokens are not rows of patch_grid_w columns), or null
static const char* no_patch_grid(const evt_model* m) {
  const int gw = patch_grid_w(*m);
  if (gw >= 1 && (m->sh.T - 1) % gw == 0) return nullptr;
  return "head statistics: the tokens after the CLS token are not a grid of image_size / patch rows";
}

int evt_head_stats_shape(const evt_model* m, int block, int* heads, int* tokens, int* prefix,
                         int* grid_w) {
  if (!m || !heads || !tokens || !prefix || !grid_w) return fail(EVT_EINVAL, "null argument");
  EVT_RC(attn_family(m));
  if (block < 0 || block >= (int)m->layers.size())
    return fail(EVT_EINVAL, "block must be in [0, " + std::to_string(m->layers.size()) + ")");
  if (const char* why = no_patch_grid(m)) return fail(EVT_EINVAL, why);
  const int gw = patch_grid_w(*m);
  *heads = m->layers[block].heads;
  *tokens = m->sh.T;
  *prefix = 1;
  *grid_w = gw;
  return EVT_OK;
}

int evt_forward_head_stats(evt_model* m, const evt_image_args* in, int B,
                           const evt_features_args* feat, const evt_head_stats_args* a,
                           void* stream) {
  if (!m || !in || !a) return fail(EVT_EINVAL, "model, image descriptor and hs must be non-null");
  const BlockList stats = {a->n_blocks, a->blocks, a->stats, "n_blocks", "blocks and stats",
                           "head statistics block", "head statistics blocks", "stats pointer",
                           "head statistics"};
  ForwardCall call;
  EVT_RC(analysis_call(m, in, B, feat, stream, attn_family, "evt_forward_head_stats", &stats,
                       &call));
  EVT_RC(check_blocks(stats, model_blocks(m), no_patch_grid(m), nullptr));
  EVT_RC(no_skipped(m, stats, EVT_SKIP_ATTN));
  call.hstats = stats.cursor();
  return forward(m, call, false);
}

// ---- FFN neuron statistics (include/evt_ffn_stats.h) ----------------------------------------

// the users of run_encoder: Swin's fused MLP never stores its hidden rows, the MX8 encoder keeps
// them quantised
static int ffn_stats_family(const evt_model* m) {
  if (m->family == FAM_SWIN)
    return fail(EVT_EINVAL, "FFN statistics: Swin's fused MLP does not store its hidden rows");
  if (m->mx8)
    return fail(EVT_EINVAL, "FFN statistics are not available on an EVT_DTYPE_MX8 model (its "
                            "hidden rows are kept quantised)");
  return EVT_OK;
}

int evt_ffn_stats_shape(const evt_model* m, int block, int* neurons, int* tokens) {
  if (!m || !neurons || !tokens) return fail(EVT_EINVAL, "null argument");
  EVT_RC(ffn_stats_family(m));
  if (block < 0 || block >= (int)m->layers.size())
    return fail(EVT_EINVAL, "block must be in [0, " + std::to_string(m->layers.size()) + ")");
  *neurons = m->layers[block].ffn;
  *tokens = m->sh.T;
  return EVT_OK;
}

int evt_forward_ffn_stats(evt_model* m, const evt_image_args* in, int B,
                          const evt_features_args* feat, const evt_ffn_stats_args* a,
                          void* stream) {
  if (!m || !in || !a) return fail(EVT_EINVAL, "model, image descriptor and fs must be non-null");
  const BlockList stats = {a->n_blocks, a->blocks, a->stats, "n_blocks", "blocks and stats",
                           "FFN statistics block", "FFN statistics blocks", "stats pointer",
                           "FFN statistics"};
  ForwardCall call;
  EVT_RC(analysis_call(m, in, B, feat, stream, ffn_stats_family, "evt_forward_ffn_stats", &stats,
                       &call));
  EVT_RC(check_blocks(stats, model_blocks(m), nullptr, nullptr));
  EVT_RC(no_skipped(m, stats, EVT_SKIP_FFN));
  call.fstats = stats.cursor();
  return forward(m, call, false);
}

// ---- activation Grams (include/evt_gram.h) --------------------------------------------------

// the users of run_encoder, for the reasons of ffn_stats_family
static int gram_family(const evt_model* m) {
  if (m->family == FAM_SWIN)
    return fail(EVT_EINVAL, "activation gram: Swin's fused MLP and window attention do not store "
                            "the rows a Gram is formed of");
  if (m->mx8)
    return fail(EVT_EINVAL, "activation gram: not available on an EVT_DTYPE_MX8 model (its hidden "
                            "and attention rows are kept quantised)");
  return EVT_OK;
}

static int gram_which(int which) {
  if (which != EVT_GRAM_FFN && which != EVT_GRAM_ATTN)
    return fail(EVT_EINVAL, "activation gram: which must be EVT_GRAM_FFN or EVT_GRAM_ATTN");
  return EVT_OK;
}

static int gram_width(const Layer& L, int which) { return which == EVT_GRAM_FFN ? L.ffn : L.inner; }

int evt_gram_shape(const evt_model* m, int block, int which, int* width, int* tokens) {
  if (!m || !width || !tokens) return fail(EVT_EINVAL, "activation gram: null argument");
  EVT_RC(gram_family(m));
  EVT_RC(gram_which(which));
  if (block < 0 || block >= (int)m->layers.size())
    return fail(EVT_EINVAL, "block must be in [0, " + std::to_string(m->layers.size()) + ")");
  *width = gram_width(m->layers[block], which);
  *tokens = m->sh.T;
  return EVT_OK;
}

int evt_forward_grams(evt_model* m, const evt_image_args* in, int B,
                      const evt_features_args* feat, const evt_gram_args* a, void* stream) {
  if (!m || !in || !a) return fail(EVT_EINVAL, "model, image descriptor and ga must be non-null");
  const BlockList grams = {a->n_blocks, a->blocks, a->grams, "n_blocks", "blocks, grams and sums",
                           "gram block", "gram blocks", "gram pointer", "activation gram outputs"};
  ForwardCall call;
  EVT_RC(analysis_call(m, in, B, feat, stream, gram_family, "evt_forward_grams", &grams, &call));
  EVT_RC(gram_which(a->which));
  if (a->n_blocks > 0 && !a->sums)
    return fail(EVT_EINVAL, "n_blocks > 0 needs the blocks, grams and sums arrays");
  EVT_RC(check_blocks(grams, model_blocks(m), nullptr, nullptr));
  EVT_RC(no_skipped(m, grams, a->which == EVT_GRAM_FFN ? EVT_SKIP_FFN : EVT_SKIP_ATTN));
  if ((uintptr_t)a->scratch & 15)
    return fail(EVT_EINVAL, "activation gram outputs: scratch must be 16-byte aligned");
  for (int i = 0; i < a->n_blocks; ++i) {
    if (!a->sums[i]) return fail(EVT_EINVAL, "gram sums pointer " + std::to_string(i) + " is NULL");
    if ((uintptr_t)a->sums[i] & 15)
      return fail(EVT_EINVAL, "activation gram outputs must be 16-byte aligned");
    const int width = gram_width(m->layers[a->blocks[i]], a->which);
    if (width > EVT_GRAM_MAX_WIDTH)
      return fail(EVT_EINVAL, "gram block " + std::to_string(a->blocks[i]) + ": its width " +
                                  std::to_string(width) + " is above " +
                                  std::to_string(EVT_GRAM_MAX_WIDTH));
    const size_t need = gram_plan(B * m->sh.T, width).scratch_bytes;
    if (need && (!a->scratch || a->scratch_bytes < need))
      return fail(EVT_EINVAL, "activation gram: scratch_bytes is " +
                                  std::to_string(a->scratch ? a->scratch_bytes : 0) + ", block " +
                                  std::to_string(a->blocks[i]) + " needs " + std::to_string(need) +
                                  " (evt_gram_scratch_bytes)");
  }
  call.grams = grams.cursor();
  call.gram = a;
  return forward(m, call, false);
}

// ---- attention rollout (include/evt_rollout.h) ----------------------------------------------

static int rollout_family(const evt_model* m) {
  if (m->family == FAM_SWIN)
    return fail(EVT_EINVAL, "attention rollout: Swin's windowed attention does not compose this way "
                            "(per-window maps: evt_forward_window_attention)");
  EVT_RC(attn_family(m));
  return EVT_OK;
}

int evt_rollout_shape(const evt_model* m, int* tokens, int* blocks) {
  if (!m || !tokens || !blocks) return fail(EVT_EINVAL, "null argument");
  EVT_RC(rollout_family(m));
  *tokens = m->sh.T;
  *blocks = (int)m->layers.size();
  return EVT_OK;
}

int evt_rollout_scratch_bytes(const evt_model* m, int B, int mode, size_t* bytes) {
  if (!m || !bytes) return fail(EVT_EINVAL, "null argument");
  EVT_RC(rollout_family(m));
  if (mode != EVT_ROLLOUT_CLS && mode != EVT_ROLLOUT_ALL)
    return fail(EVT_EINVAL, "rollout mode must be EVT_ROLLOUT_CLS or EVT_ROLLOUT_ALL");
  EVT_RC(check_batch(m, B));
  *bytes = (size_t)rollout_bufs((int)m->layers.size()) * rollout_buf_bytes(B, m->sh.T);
  return EVT_OK;
}

int evt_forward_rollout(evt_model* m, const evt_image_args* in, int B,
                        const evt_features_args* feat, const evt_rollout_args* a, void* stream) {
  if (!m || !in || !a) return fail(EVT_EINVAL, "model, image descriptor and ro must be non-null");
  ForwardCall call;
  EVT_RC(analysis_call(m, in, B, feat, stream, rollout_family, "evt_forward_rollout", nullptr,
                       &call));
  const int depth = (int)m->layers.size();
  if (a->start < 0 || a->start >= depth)
    return fail(EVT_EINVAL, "rollout start must be in [0, " + std::to_string(depth) + ")");
  if (a->mode != EVT_ROLLOUT_CLS && a->mode != EVT_ROLLOUT_ALL)
    return fail(EVT_EINVAL, "rollout mode must be EVT_ROLLOUT_CLS or EVT_ROLLOUT_ALL");
  if (!a->out || !a->scratch) return fail(EVT_EINVAL, "rollout out and scratch must be non-null");
  if (((uintptr_t)a->out | (uintptr_t)a->scratch) & 15)
    return fail(EVT_EINVAL, "rollout out and scratch must be 16-byte aligned");
  const size_t need = (size_t)rollout_bufs(depth) * rollout_buf_bytes(B, m->sh.T);
  if (a->scratch_bytes < need)
    return fail(EVT_EINVAL, "rollout scratch_bytes is " + std::to_string(a->scratch_bytes) +
                                ", this call needs " + std::to_string(need));
  for (int i = a->start; i < depth; ++i)
    if (m->skip_of(i) & EVT_SKIP_ATTN)
      return fail(EVT_EINVAL, "rollout: the attention sublayer of block " + std::to_string(i) +
                                  " is skipped (evt_model_set_skips), it has no attention map");
  call.rollout = a;
  return forward(m, call, false);
}

// ---- token pruning (include/evt_token_pruning.h) ---------------------------------------------

static int token_pruning_family(const evt_model* m) {
  if (m->family == FAM_SWIN)
    return fail(EVT_EINVAL, "token pruning: Swin's windows need the whole token grid");
  if (m->family == FAM_T2T)
    return fail(EVT_EINVAL, "token pruning: T2T-ViT is not supported yet (ViT handles only)");
  if (m->mx8)
    return fail(EVT_EINVAL, "token pruning is not available on an EVT_DTYPE_MX8 model");
  return EVT_OK;
}

// A skip mask and a token schedule on one handle (include/evt_depth.h): a scheduled block scores
// its tokens by the attention it ran, and has a block that runs after it
static int skips_fit_schedule(const evt_model* m, const std::vector<uint8_t>& mask,
                              const int32_t* blocks, int n) {
  if (mask.empty()) return EVT_OK;
  int last = (int)mask.size() - 1;
  while (last >= 0 && mask[last] == (EVT_SKIP_ATTN | EVT_SKIP_FFN)) --last;
  for (int i = 0; i < n; ++i) {
    if (mask[blocks[i]] & EVT_SKIP_ATTN)
      return fail(EVT_EINVAL, "token schedule: the attention sublayer of block " +
                                  std::to_string(blocks[i]) + " is skipped (evt_model_set_skips): "
                                  "it has no CLS attention to score tokens by");
    if (blocks[i] >= last)
      return fail(EVT_EINVAL, "token schedule: block " + std::to_string(blocks[i]) + " is the last "
                                  "block that runs under the skip mask (evt_model_set_skips), or "
                                  "comes after it: its output is the CLS token's alone");
  }
  return EVT_OK;
}

int evt_model_set_token_schedule(evt_model* m, int n, const int32_t* blocks, const int32_t* keep,
                                 void*) {
  if (!m) return fail(EVT_EINVAL, "model is NULL");
  if (m->is_lane) return fail(EVT_EINVAL, "the model is a lane of another model");
  EVT_RC(token_pruning_family(m));
  if (m->graph) return fail(EVT_EINVAL, "set the schedule before evt_graph_capture");
  if (n < 0 || n > EVT_TOKEN_SCHEDULE_MAX)
    return fail(EVT_EINVAL, "token schedule: n must be in [0, " +
                                std::to_string(EVT_TOKEN_SCHEDULE_MAX) + "]");
  if (n > 0 && (!blocks || !keep))
    return fail(EVT_EINVAL, "token schedule: n > 0 needs the blocks and keep arrays");
  const int depth = (int)m->layers.size();
  int T = m->sh.T;
  for (int i = 0; i < n; ++i) {
    if (i > 0 && blocks[i] <= blocks[i - 1])
      return fail(EVT_EINVAL, "token schedule: blocks must be strictly ascending");
    if (blocks[i] < 0 || blocks[i] >= depth - 1)
      return fail(EVT_EINVAL, "token schedule: block " + std::to_string(blocks[i]) +
                                  " is outside [0, depth - 1 = " + std::to_string(depth - 1) +
                                  "): the last block's output is the CLS token's alone");
    if (keep[i] < 1 || keep[i] > T - 1)
      return fail(EVT_EINVAL, "token schedule: keep " + std::to_string(keep[i]) + " after block " +
                                  std::to_string(blocks[i]) + " is outside [1, " +
                                  std::to_string(T - 1) + "], the block's patch tokens");
    T = keep[i] + 1;
  }
  EVT_RC(skips_fit_schedule(m, m->skips, blocks, n));
  m->tp_blocks.assign(blocks, blocks + n);
  m->tp_keep.assign(keep, keep + n);
  for (evt_model* c : m->lanes) {  // lanes set later copy the core, the schedule with it
    c->tp_blocks = m->tp_blocks;
    c->tp_keep = m->tp_keep;
  }
  return EVT_OK;
}

int evt_model_token_schedule(const evt_model* m, int* n, int32_t* blocks, int32_t* keep, int cap) {
  if (!m || !n || cap < 0) return fail(EVT_EINVAL, "token schedule: a NULL model or n, or cap < 0");
  *n = (int)m->tp_blocks.size();
  for (int i = 0; i < *n && i < cap; ++i) {
    if (blocks) blocks[i] = m->tp_blocks[i];
    if (keep) keep[i] = m->tp_keep[i];
  }
  return EVT_OK;
}

int evt_model_tokens_at(const evt_model* m, int block, int* tokens) {
  if (!m || !tokens) return fail(EVT_EINVAL, "null argument");
  if (m->family != FAM_VIT)
    return fail(EVT_EINVAL, "tokens_at: token schedules are a ViT handle's");
  if (block < 0 || block >= (int)m->layers.size())
    return fail(EVT_EINVAL, "block must be in [0, " + std::to_string(m->layers.size()) + ")");
  *tokens = tokens_at(*m, block);
  return EVT_OK;
}

// evt_forward_token_pruning: a family that has token schedules, and a schedule set
static int scheduled_family(const evt_model* m) {
  EVT_RC(token_pruning_family(m));
  if (m->tp_blocks.empty())
    return fail(EVT_EINVAL, "forward_token_pruning: the model has no token schedule "
                            "(evt_model_set_token_schedule first)");
  return EVT_OK;
}

int evt_forward_token_pruning(evt_model* m, const evt_image_args* in, int B,
                              const evt_features_args* feat, const evt_token_pruning_args* tp,
                              void* stream) {
  if (!m || !in || !feat)
    return fail(EVT_EINVAL, "model, image descriptor and feat must be non-null");
  ForwardCall call;
  // (feat's tokens and taps are refused under a schedule: validate_features)
  EVT_RC(analysis_call(m, in, B, feat, stream, scheduled_family, nullptr, nullptr, &call));
  if (tp) {
    const int n = (int)m->tp_blocks.size();
    if (tp->n_blocks != n)
      return fail(EVT_EINVAL, "forward_token_pruning: n_blocks must be the schedule's length " +
                                  std::to_string(n));
    for (int i = 0; i < n; ++i)
      if (((tp->scores ? (uintptr_t)tp->scores[i] : 0) | (tp->kept ? (uintptr_t)tp->kept[i] : 0)) & 3)
        return fail(EVT_EINVAL, "forward_token_pruning: scores and kept must be 4-byte aligned");
  }
  call.tprune = tp;
  return forward(m, call, false);
}

// ---- structured gates (include/evt_gates.h) --------------------------------------------------

static int gates_family(const evt_model* m) {
  if (m->is_lane) return fail(EVT_EINVAL, "structured gates: the model is a lane of another model");
  if (m->family == FAM_SWIN)
    return fail(EVT_EINVAL, "structured gates: Swin is not supported (ViT handles only)");
  if (m->family == FAM_T2T)
    return fail(EVT_EINVAL, "structured gates: T2T-ViT is not supported (ViT handles only)");
  if (m->mx8)
    return fail(EVT_EINVAL, "structured gates are not available on an EVT_DTYPE_MX8 model: its "
                            "block-scaled weights would need requantising");
  return EVT_OK;
}

// block (negative: from the last) -> its index, or EVT_EINVAL
static int gate_block(const evt_model* m, int block, int* index) {
  const int depth = (int)m->layers.size();
  const int i = block < 0 ? block + depth : block;
  if (i < 0 || i >= depth)
    return fail(EVT_EINVAL, "structured gates: block " + std::to_string(block) +
                                " is outside the model's " + std::to_string(depth) + " blocks");
  *index = i;
  return EVT_OK;
}

// The calls that enqueue on s refuse a capturing stream: they allocate at a role's first gate, and
// a graph has no use for a gate set inside it (its replays read the weights the set wrote)
static int not_capturing(hipStream_t s, const char* what) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  EVT_HIP(hipStreamIsCapturing(s, &st), "stream capture status");
  if (st != hipStreamCaptureStatusNone)
    return fail(EVT_EINVAL, std::string(what) + ": the stream is capturing (set the gates outside "
                            "the capture; a captured graph needs no recapture)");
  return EVT_OK;
}

// The n gates of one role of block `block`: out-projection (per head, each over its hd K columns)
// or FC2 (per neuron). Everything is checked before anything is allocated, enqueued or recorded.
static int set_gates(evt_model* m, int block, bool ffn, const float* gates, int n, void* stream) {
  const char* what = ffn ? "set_ffn_gates" : "set_head_gates";
  if (!m || !gates) return fail(EVT_EINVAL, std::string(what) + ": model and gates must be non-null");
  EVT_RC(gates_family(m));
  int i = 0;
  EVT_RC(gate_block(m, block, &i));
  const Layer& L = m->layers[i];
  const DenseW& dw = ffn ? L.fc2 : L.out;
  const int count = ffn ? L.ffn : L.heads, per = ffn ? 1 : L.hd;
  if (n != count)
    return fail(EVT_EINVAL, std::string(what) + ": n is " + std::to_string(n) + ", block " +
                                std::to_string(i) + " has " + std::to_string(count) +
                                (ffn ? " FFN neurons" : " heads"));
  bool identity = true;
  for (int j = 0; j < n; ++j) {
    if (!std::isfinite(gates[j]))
      return fail(EVT_EINVAL, std::string(what) + ": gate " + std::to_string(j) +
                                  " is not finite (NaN or infinite)");
    identity = identity && gates[j] == 1.0f;
  }
  hipStream_t s = (hipStream_t)stream;
  EVT_RC(not_capturing(s, what));
  if (m->gates.empty()) m->gates.resize(m->layers.size());
  GateRole& r = ffn ? m->gates[i].ffn : m->gates[i].head;
  if (identity && !r.w0) {  // the packed weight is still the pristine one
    r.rec.assign(gates, gates + n);
    return EVT_OK;
  }
  if (!r.w0) {
    const size_t bytes = (size_t)dw.npad * dw.kpad * elem_size(m->dtype);
    void* w0 = nullptr;
    float* g = nullptr;
    EVT_RC(dev_alloc(m, &w0, bytes));
    EVT_RC(dev_alloc(m, (void**)&g, (size_t)dw.kpad * sizeof(float)));
    EVT_HIP(hipMemcpyAsync(w0, dw.w, bytes, hipMemcpyDeviceToDevice, s), "pristine weight copy");
    r.w0 = w0;
    r.g = g;
  }
  std::vector<float> k((size_t)dw.kpad, 1.0f);  // 1 in the K padding: its zero columns stay +0
  for (int j = 0; j < n; ++j) std::fill_n(k.begin() + (size_t)j * per, per, gates[j]);
  // pageable source: staged before the call returns, so k (and the caller's array) may go
  EVT_HIP(hipMemcpyAsync(r.g, k.data(), k.size() * sizeof(float), hipMemcpyHostToDevice, s),
          "gate upload");
  // the layer's N rows: the padding rows [N, npad) keep the +0 make_dense gave them
  EVT_HIP(gate_weights_launch(m->dtype, r.w0, dw.w, r.g, dw.N, dw.kpad, s), "gate_weights");
  r.rec.assign(gates, gates + n);
  return EVT_OK;
}

static int get_gates(const evt_model* m, int block, bool ffn, float* gates, int cap, int* n) {
  if (!m || !n || cap < 0)
    return fail(EVT_EINVAL, "get gates: a NULL model or n, or cap < 0");
  EVT_RC(gates_family(m));
  int i = 0;
  EVT_RC(gate_block(m, block, &i));
  *n = ffn ? m->layers[i].ffn : m->layers[i].heads;
  const GateRole* r = m->gates.empty() ? nullptr : ffn ? &m->gates[i].ffn : &m->gates[i].head;
  for (int j = 0; gates && j < *n && j < cap; ++j)
    gates[j] = r && !r->rec.empty() ? r->rec[j] : 1.0f;
  return EVT_OK;
}

int evt_model_set_head_gates(evt_model* m, int block, const float* gates, int n, void* stream) {
  return set_gates(m, block, false, gates, n, stream);
}

int evt_model_set_ffn_gates(evt_model* m, int block, const float* gates, int n, void* stream) {
  return set_gates(m, block, true, gates, n, stream);
}

int evt_model_clear_gates(evt_model* m, void* stream) {
  if (!m) return fail(EVT_EINVAL, "clear_gates: model is NULL");
  EVT_RC(gates_family(m));
  hipStream_t s = (hipStream_t)stream;
  EVT_RC(not_capturing(s, "clear_gates"));
  for (size_t i = 0; i < m->gates.size(); ++i) {
    const Layer& L = m->layers[i];
    for (int ffn = 0; ffn < 2; ++ffn) {
      GateRole& r = ffn ? m->gates[i].ffn : m->gates[i].head;
      const DenseW& dw = ffn ? L.fc2 : L.out;
      // a role without a pristine copy was never written; all-ones gates wrote the pristine bits
      if (r.w0 && std::any_of(r.rec.begin(), r.rec.end(), [](float g) { return g != 1.0f; }))
        EVT_HIP(hipMemcpyAsync(dw.w, r.w0, (size_t)dw.npad * dw.kpad * elem_size(m->dtype),
                               hipMemcpyDeviceToDevice, s),
                "restore pristine weight");
      r.rec.clear();
    }
  }
  return EVT_OK;
}

int evt_model_get_head_gates(const evt_model* m, int block, float* gates, int cap, int* n) {
  return get_gates(m, block, false, gates, cap, n);
}

int evt_model_get_ffn_gates(const evt_model* m, int block, float* gates, int cap, int* n) {
  return get_gates(m, block, true, gates, cap, n);
}

// ---- depth: stream statistics and sublayer skips (include/evt_depth.h) ------------------------

static int depth_family(const evt_model* m, const char* what) {
  if (m->family == FAM_SWIN)
    return fail(EVT_EINVAL, std::string(what) + ": Swin is not supported (ViT handles only)");
  if (m->family == FAM_T2T)
    return fail(EVT_EINVAL, std::string(what) + ": T2T-ViT is not supported yet (ViT handles only)");
  if (m->mx8)
    return fail(EVT_EINVAL, std::string(what) + " is not available on an EVT_DTYPE_MX8 model");
  return EVT_OK;
}
static int block_stats_family(const evt_model* m) { return depth_family(m, "block statistics"); }

int evt_block_stats_shape(const evt_model* m, int block, int* sublayers, int* stats, int* tokens) {
  if (!m || !sublayers || !stats || !tokens) return fail(EVT_EINVAL, "null argument");
  EVT_RC(block_stats_family(m));
  if (block < 0 || block >= (int)m->layers.size())
    return fail(EVT_EINVAL, "block must be in [0, " + std::to_string(m->layers.size()) + ")");
  *sublayers = 2;
  *stats = EVT_DEPTH_STATS;
  *tokens = m->sh.T;
  return EVT_OK;
}

int evt_forward_block_stats(evt_model* m, const evt_image_args* in, int B,
                            const evt_features_args* feat, const evt_block_stats_args* a,
                            void* stream) {
  if (!m || !in || !a) return fail(EVT_EINVAL, "model, image descriptor and bs must be non-null");
  const BlockList stats = {a->n_blocks, a->blocks, a->stats, "n_blocks", "blocks and stats",
                           "block statistics block", "block statistics blocks", "stats pointer",
                           "block statistics"};
  ForwardCall call;
  EVT_RC(analysis_call(m, in, B, feat, stream, block_stats_family, "evt_forward_block_stats",
                       &stats, &call));
  EVT_RC(check_blocks(stats, model_blocks(m), nullptr, nullptr));
  call.bstats = stats.cursor();
  return forward(m, call, false);
}

int evt_model_set_skips(evt_model* m, const uint8_t* mask, int depth, void* stream) {
  if (!m) return fail(EVT_EINVAL, "set_skips: model is NULL");
  if (m->is_lane) return fail(EVT_EINVAL, "set_skips: the model is a lane of another model");
  EVT_RC(depth_family(m, "sublayer skipping"));
  if (m->graph) return fail(EVT_EINVAL, "set the skips before evt_graph_capture");
  hipStream_t s = (hipStream_t)stream;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  EVT_HIP(hipStreamIsCapturing(s, &st), "stream capture status");
  if (st != hipStreamCaptureStatusNone)
    return fail(EVT_EINVAL, "set_skips: the stream is capturing (a graph records the launches of "
                            "the mask it was captured under: set the skips before the capture)");
  std::vector<uint8_t> skips;
  if (mask) {
    const int nb = (int)m->layers.size();
    if (depth != nb)
      return fail(EVT_EINVAL, "set_skips: depth is " + std::to_string(depth) + ", the model has " +
                                  std::to_string(nb) + " blocks");
    bool any = false;
    for (int i = 0; i < nb; ++i) {
      if (mask[i] & ~(EVT_SKIP_ATTN | EVT_SKIP_FFN))
        return fail(EVT_EINVAL, "set_skips: mask of block " + std::to_string(i) + " has bits "
                                    "beyond EVT_SKIP_ATTN | EVT_SKIP_FFN");
      any = any || mask[i];
    }
    if (any) skips.assign(mask, mask + nb);
    if (any && std::all_of(skips.begin(), skips.end(),
                           [](uint8_t v) { return v == (EVT_SKIP_ATTN | EVT_SKIP_FFN); }))
      return fail(EVT_EINVAL, "set_skips: the mask skips every block, no sublayer of the encoder "
                              "would run (create the model with depth 0 instead)");
  }
  EVT_RC(skips_fit_schedule(m, skips, m->tp_blocks.data(), (int)m->tp_blocks.size()));
  if (!skips.empty() && !m->skip_ident) {
    std::vector<float> rows((size_t)m->max_batch * EVT_DEPTH_STATS);
    for (size_t i = 0; i < rows.size(); i += EVT_DEPTH_STATS) {
      rows[i + EVT_DEPTH_COSINE] = rows[i + EVT_DEPTH_NORM_RATIO] = rows[i + EVT_DEPTH_CLS_COSINE] = 1.f;
      rows[i + EVT_DEPTH_REL_UPDATE] = 0.f;
    }
    float* d = nullptr;
    EVT_RC(dev_alloc(m, (void**)&d, rows.size() * sizeof(float)));
    // once per handle, 16 bytes per image: a synchronous copy, so the rows are on the device
    // before any forward, on whatever stream, can be enqueued behind this call
    EVT_HIP(hipMemcpy(d, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice),
            "skip identity rows");
    m->skip_ident = d;
  }
  m->skips = skips;
  for (evt_model* c : m->lanes) c->skips = skips;  // lanes set later copy the core, the mask with it
  return EVT_OK;
}

int evt_model_get_skips(const evt_model* m, uint8_t* mask, int cap, int* depth) {
  if (!m || !depth || cap < 0) return fail(EVT_EINVAL, "get_skips: a NULL model or depth, or cap < 0");
  EVT_RC(depth_family(m, "sublayer skipping"));
  *depth = (int)m->layers.size();
  for (int i = 0; mask && i < *depth && i < cap; ++i) mask[i] = m->skip_of(i);
  return EVT_OK;
}

// ---- Swin window attention maps (include/evt_window_attention.h) ----------------------------

static int window_attn_family(const evt_model* m) {
  if (m->family != FAM_SWIN)
    return fail(EVT_EINVAL, "window attention maps are Swin's: this model's maps are "
                            "evt_forward_attention's");
  return EVT_OK;
}

int evt_window_attn_map_shape(const evt_model* m, int block, int* windows, int* heads,
                              int* tokens) {
  if (!m || !windows || !heads || !tokens) return fail(EVT_EINVAL, "null argument");
  EVT_RC(window_attn_family(m));
  int i = block;
  for (const SwinStage& st : m->stages) {
    if (i >= 0 && i < (int)st.blocks.size()) {
      *windows = (st.R / st.w) * (st.R / st.w);
      *heads = st.H;
      *tokens = st.w * st.w;
      return EVT_OK;
    }
    i -= (int)st.blocks.size();
  }
  return fail(EVT_EINVAL, "block must be in [0, " + std::to_string(model_blocks(m)) + ")");
}

int evt_forward_window_attention(evt_model* m, const evt_image_args* in, int B,
                                 const evt_features_args* feat, const evt_attn_args* a,
                                 void* stream) {
  if (!m || !in || !a) return fail(EVT_EINVAL, "model, image descriptor and attn must be non-null");
  return attention_forward(m, in, B, feat, a, stream, window_attn_family, nullptr, false);
}

int evt_forward_classify(evt_model* m, const evt_image_args* in, int B,
                         const evt_features_args* feat, const evt_classify_args* cls,
                         void* stream) {
  ImgAffine aff{};
  if (!feat || !cls)
    return fail(EVT_EINVAL, "forward_classify: feat and cls must be non-null");
  EVT_RC(validate_image(m, in, &aff));
  if (!feat->logits)
    return fail(EVT_EINVAL, "forward_classify: feat->logits is required (the caller owns the "
                            "logits the classification reads)");
  if ((uintptr_t)feat->logits & 3)
    return fail(EVT_EINVAL, "forward_classify: logits must be 4-byte aligned");
  EVT_RC(validate_features(m, feat, B));
  ClassifyParams p;
  EVT_RC(validate_classify(cls, B, m->num_classes, m->num_classes, &p));
  EVT_RC(image_forward(m, in, aff, B, feat, stream));
  // the lanes have joined `stream` (lanes_forward): the logits of every image are ordered before
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(m, EVT_PROF_HEAD, s);
  prof_work(m, 0.0, (double)B * m->num_classes * 4.0 * (p.k + 1 + (p.labels ? 1 : 0)));
  EVT_HIP(classify_launch(feat->logits, m->num_classes, B, m->num_classes, p, s), "classify");
  return EVT_OK;
}

}  // extern "C"
