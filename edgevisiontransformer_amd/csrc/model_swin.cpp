// Swin Transformer: descriptor checks, geometry, workspace, create and forward.
#include "model.h"

using namespace evt;

namespace {

int validate_swin(const evt_swin_desc* d, SwinGeo* g) {
  if (!d) return fail(EVT_EINVAL, "desc is NULL");
  if (d->dtype != EVT_DTYPE_F32 && d->dtype != EVT_DTYPE_BF16)
    return fail(EVT_EINVAL, "dtype must be EVT_DTYPE_F32 or EVT_DTYPE_BF16");
  if (d->num_stages < 1 || d->num_stages > EVT_SWIN_MAX_STAGES)
    return fail(EVT_EINVAL, "num_stages must be in [1, 8]");
  if (d->patch_size <= 0 || d->image_size <= 0 || d->image_size % d->patch_size)
    return fail(EVT_EINVAL, "image_size must be a multiple of patch_size");
  if (d->in_chans <= 0 || d->num_classes <= 0 || d->max_batch <= 0 || !(d->mlp_ratio > 0.f))
    return fail(EVT_EINVAL, "in_chans, num_classes, max_batch, mlp_ratio must be positive");
  if (d->window_size != 7 && d->window_size != 12)
    return fail(EVT_EINVAL, "window_size must be 7 or 12 in this build");
  if (d->embed_dim <= 0 || d->embed_dim % 32)
    return fail(EVT_EINVAL, "embed_dim must be a positive multiple of 32");
  g->ns = d->num_stages;
  g->pd = d->in_chans * d->patch_size * d->patch_size;
  g->pdst = (int)round_up(g->pd, PAD_K);
  int R = d->image_size / d->patch_size;
  for (int i = 0; i < g->ns; ++i) {
    if (i > 0) {
      if (R % 2) return fail(EVT_EINVAL, "patch merging needs an even resolution");
      R /= 2;
    }
    // the reference rule: a stage no larger than the window is one window of its own size
    const int win = std::min(d->window_size, R);
    if ((win != 7 && win != 12) || R % win)
      return fail(EVT_EINVAL, "stage " + std::to_string(i) + ": resolution " + std::to_string(R) +
                                  " with window " + std::to_string(win) +
                                  "; every stage resolution must be a multiple of the window (" +
                                  std::to_string(d->window_size) + ") and its window 7 or 12");
    g->w[i] = win;
    const int C = d->embed_dim << i;
    if (C > 1536) return fail(EVT_EINVAL, "stage width must be <= 1536");
    if (d->depths[i] < 0) return fail(EVT_EINVAL, "depths must be >= 0");
    if (d->num_heads[i] <= 0 || C % d->num_heads[i] || C / d->num_heads[i] != 32)
      return fail(EVT_EINVAL, "head size (stage width / num_heads) must be 32 in this build");
    g->C[i] = C;
    // Row stride = C (a multiple of 32): no stream padding. The GEMMs that consume these rows
    // read K rounded up to 64 columns; the columns past C belong to the next row (finite values,
    // multiplied by the zero-padded weight rows) and the last row's overrun lands in the zeroed
    // slack SWIN_SLACK at the end of each such buffer.
    g->Cst[i] = C;
    g->R[i] = R;
    g->mlp[i] = (int)(C * d->mlp_ratio);
    if (g->mlp[i] <= 0) return fail(EVT_EINVAL, "mlp width must be positive");
    g->mst[i] = (int)round_up(g->mlp[i], PAD_N);
  }
  if (g->R[0] * g->R[0] > 3136 || g->C[g->ns - 1] > 1024) {
    // As validate() past 256 tokens: several kernels form byte offsets into an activation buffer
    // in 32 bits. Up to 56 x 56 tokens (224 px) and stage widths of 1024 the supported batches are
    // as they were; past either a max_batch whose largest buffer (image batch, patch matrix, qkv,
    // MLP hidden, merge gather, row statistics) would reach 2^31 bytes is refused. A model with a
    // stage wider than 1024 has wider rows at every resolution: Swin-L at 224 px holds
    // 3136 x 768 elements per image in its MLP hidden, 2^31 bytes at 446 bf16 / 223 f32 images.
    const size_t es = d->dtype == EVT_DTYPE_F32 ? 4 : 2, B = (size_t)d->max_batch;
    size_t big = B * d->in_chans * d->image_size * d->image_size * sizeof(float);
    big = std::max(big, B * g->R[0] * g->R[0] * g->pdst * es);
    for (int i = 0; i < g->ns; ++i) {
      const size_t rows = B * g->R[i] * g->R[i];
      const size_t widest = std::max<size_t>({(size_t)3 * g->C[i], (size_t)g->mst[i],
                                              i > 0 ? (size_t)4 * g->C[i - 1] : 0});
      big = std::max({big, rows * widest * es, rows * stats_slots(g->C[i]) * 2 * sizeof(float)});
    }
    if (big >= (size_t)1 << 31)
      return fail(EVT_EINVAL, "max_batch too large for more than 3136 tokens per image or a stage "
                              "wider than 1024: every activation buffer must stay below 2^31 bytes");
  }
  return EVT_OK;
}

constexpr size_t SWIN_SLACK = 64;  // zeroed elements after x / xm / o (K-padding overrun)

struct SwinWs {  // element / float counts of the Swin workspace for B images
  size_t stream = 0, stats = 0, qkv = 0, o = 0, hbuf = 0, pooled = 0;
};

SwinWs swin_ws(const SwinGeo& g, int B) {
  SwinWs w;
  for (int i = 0; i < g.ns; ++i) {
    const size_t rows = (size_t)B * g.R[i] * g.R[i];
    w.stream = std::max(w.stream, rows * g.Cst[i]);
    w.stats = std::max(w.stats, rows * stats_slots(g.C[i]) * 2);
    w.qkv = std::max(w.qkv, rows * 3 * g.C[i]);
    w.o = std::max(w.o, rows * g.Cst[i]);
    w.hbuf = std::max(w.hbuf, rows * g.mst[i]);
    if (i > 0) w.hbuf = std::max(w.hbuf, rows * 4 * g.C[i - 1]);
  }
  w.hbuf = std::max(w.hbuf, (size_t)B * g.R[0] * g.R[0] * g.pdst);
  w.pooled = (size_t)B * g.Cst[g.ns - 1];
  return w;
}

// The Swin workspace for B images (activation buffers only; lanes allocate their own)
WsLayout swin_ws_layout(const SwinGeo& g, int dtype, int B) {
  WsLayout l;
  const SwinWs ws = swin_ws(g, B);
  const size_t es = elem_size(dtype);
  const size_t xb = (ws.stream + SWIN_SLACK) * es, ob = (ws.o + SWIN_SLACK) * es;
  l.bufs.push_back({EVT_WS(x), xb, xb, "memset x"});
  l.bufs.push_back({EVT_WS(xm), xb, xb, "memset xm"});
  l.bufs.push_back({EVT_WS(sx), ws.stats * sizeof(float)});
  l.bufs.push_back({EVT_WS(sm), ws.stats * sizeof(float)});
  l.bufs.push_back({EVT_WS(qkv), ws.qkv * es});
  l.bufs.push_back({EVT_WS(o), ob, ob, "memset o"});
  l.bufs.push_back({EVT_WS(hbuf), ws.hbuf * es});
  l.bufs.push_back({EVT_WS(pooled), ws.pooled * es});
  if (dtype == DT_BF16)
    l.bufs.push_back({EVT_WS(sk), gemm_sk_bytes(), 4096, "memset stream-K flags"});
  return l;
}

int swin_blocks(const ModelCore& m) {
  int n = 0;
  for (const SwinStage& st : m.stages) n += (int)st.blocks.size();
  return n;
}

// block's stage (blocks are numbered consecutively over the stages); block < 0: the last stage
void swin_shape(const ModelCore& m, int block, int* tokens, int* width) {
  const SwinStage* at = &m.stages.back();
  for (const SwinStage& st : m.stages) {
    if (block >= 0 && block < (int)st.blocks.size()) {
      at = &st;
      break;
    }
    block -= (int)st.blocks.size();
  }
  *tokens = at->R * at->R;
  *width = at->C;
}
// The Swin forward on this handle's own workspace (features forwards: as vit_run)
int swin_run(evt_model* m, ForwardCall& call) {
  prof_reset(m);
  const evt_swin_desc& d = m->sdesc;
  const int B = call.B, dt = d.dtype;
  float* logits = call.logits;
  hipStream_t s = call.s;
  const SwinStage& s0 = m->stages[0];
  const int pdst = m->swin.pdst;
  const float scale_log2 = 0.17677669529663687f * 1.4426950408889634f;  // 32^-0.5 * log2(e)
  // patch embed: Conv2d(k = s = patch) as im2col + Dense, then its LayerNorm -> stream x + stats
  int rows = B * s0.R * s0.R;
  const double es = (double)elem_size(dt);
  const bool stem96 = dt == DT_BF16 && d.in_chans == 3 && d.patch_size == 4 && s0.C == 96 &&
                      s0.Cst == 96 && m->patch.kpad == 64 && d.image_size % 16 == 0 &&
                      d.image_size <= 256 && s0.w == 7;
  if (stem96) {  // Conv2d + embedding LayerNorm in one kernel (swin.hip, swin_embed96_kernel)
    ProfScope ps(m, EVT_PROF_PATCH_EMBED, s);
    prof_work(m, 2.0 * rows * 96 * 48,
              (double)B * 3 * d.image_size * d.image_size * (call.img8 ? 1 : 4) +
                  (double)rows * 96 * es + (double)rows * stats_slots(96) * 8);
    SwinEmbedParams ep;
    ep.img = call.img; ep.img8 = call.img8; ep.aff = call.aff;
    ep.w = m->patch.w; ep.ldw = m->patch.kpad; ep.bias = m->patch.b;
    ep.gamma = m->pnorm_g; ep.beta = m->pnorm_b; ep.x = m->ws.x; ep.stats = m->ws.sx;
    ep.B = B; ep.S = d.image_size; ep.nslots = stats_slots(96); ep.eps = 1e-5f;
    EVT_HIP(swin_embed96_launch(ep, s), "fused patch embedding");
  } else {
  {
    ProfScope ps(m, EVT_PROF_PATCHIFY, s);
    prof_work(m, 0.0, (double)B * d.in_chans * d.image_size * d.image_size * (call.img8 ? 1 : 4) +
                          (double)rows * d.in_chans * d.patch_size * d.patch_size * es);
    if (call.img8)
      EVT_HIP(swin_patch_u8_launch(dt, call.img8, B, d.in_chans, d.image_size, d.patch_size,
                                   m->ws.hbuf, pdst, call.aff, s),
              "patch im2col (uint8)");
    else
      EVT_HIP(swin_patch_launch(dt, call.img, B, d.in_chans, d.image_size, d.patch_size,
                                m->ws.hbuf, pdst, s),
              "patch im2col");
  }
  {
    ProfScope ps(m, EVT_PROF_PATCH_EMBED, s);
    DenseCall c;
    c.flags = EPI_BIAS;
    c.A = m->ws.hbuf; c.lda = pdst; c.C = m->ws.xm; c.ldc = s0.Cst; c.M = rows; c.N = s0.Cst;
    EVT_RC(dense(m, m->patch, c, s));
    prof_work(m, 0.0, 2.0 * rows * s0.C * es + (double)rows * stats_slots(s0.C) * 8);
    EVT_HIP(ln_rows_launch(dt, m->ws.xm, s0.Cst, m->ws.x, m->pnorm_g, m->pnorm_b, rows, s0.C, 1e-5f,
                           m->ws.sx, stats_slots(s0.C), s),
            "patch norm");
  }
  }
  int nblock = 0;
  for (size_t i = 0; i < m->stages.size(); ++i) {
    const SwinStage& st = m->stages[i];
    const int C = st.C, Cst = st.Cst;
    rows = B * st.R * st.R;
    if (i > 0) {  // PatchMerging: gather -> LN(4C)-folded reduction -> stream x (+ stats)
      const SwinStage& pv = m->stages[i - 1];
      ProfScope ps(m, EVT_PROF_MERGE, s);
      DenseCall c;
      c.flags = EPI_LNIN | EPI_BIAS | EPI_STATS;
      c.C = m->ws.x; c.ldc = Cst; c.M = rows; c.N = Cst;
      c.stats_in = m->ws.sm; c.stats_out = m->ws.sx; c.ln_width = 4 * pv.C; c.slot_width = C;
      bool fused = false;
      if (dt == DT_BF16 && pv.Cst == pv.C && pv.R % 2 == 0) {
        // the gather inside the reduction GEMM's A loader (gemm.hip, EPI_GATHER): A = the old
        // stream, read in place, so the new stream goes to xm and the two buffers swap roles
        DenseCall g = c;
        g.flags |= EPI_GATHER;
        g.A = m->ws.x; g.lda = pv.Cst; g.C = m->ws.xm;
        GemmParams p = dense_params(m, st.merge, g);
        const int R2 = pv.R / 2;
        p.gmode = 1; p.gR = pv.R; p.gC = pv.C; p.gOW = R2;
        p.g_inv_rr = 1.0f / (float)(R2 * R2); p.g_inv_r = 1.0f / (float)R2;
        EVT_HIP(merge_stats_launch(m->ws.sx, stats_slots(pv.C), B, pv.R, m->ws.sm, stats_slots(C),
                                   s),
                "merge statistics");
        const hipError_t e = gemm_launch(dt, g.flags, p, s);
        if (e == hipSuccess) {
          c.A = m->ws.x; c.lda = 4 * pv.C;  // (work accounting: the same A bytes, gathered)
          dense_work(m, st.merge, c);
          std::swap(m->ws.x, m->ws.xm);
          fused = true;
        } else if (e != hipErrorNotSupported) {
          EVT_HIP(e, "patch merge (gathered)");
        }
      }
      if (!fused) {
        prof_work(m, 0.0, 2.0 * rows * 4 * pv.C * es + (double)rows * stats_slots(C) * 8);
        EVT_HIP(merge_launch(dt, m->ws.x, pv.Cst, B, pv.R, pv.C, m->ws.hbuf, m->ws.sm,
                             stats_slots(C), s),
                "patch merge");
        c.A = m->ws.hbuf; c.lda = 4 * pv.C;
        EVT_RC(dense(m, st.merge, c, s));
      }
    }
    for (const SwinBlock& bl : st.blocks) {
      const int block = nblock++;  // numbered consecutively over the stages (feature taps)
      // the fused C = 96 sublayers are window-7 kernels; a window-12 stage takes the GEMM path
      const bool fuse96 = dt == DT_BF16 && C == 96 && st.H == 3 && st.w == 7 && gemm_auto();
      const double slot_rows = (double)rows * stats_slots(C) * 8;
      DenseCall qc;  // LN1-folded QKV (+ bias): ws.x -> ws.qkv
      qc.flags = EPI_LNIN | EPI_BIAS;
      qc.A = m->ws.x; qc.lda = Cst; qc.C = m->ws.qkv; qc.ldc = 3 * C; qc.M = rows; qc.N = 3 * C;
      qc.stats_in = m->ws.sx; qc.ln_width = C;
      const SwinAttnParams ap{m->ws.qkv, 3 * C, m->ws.o, Cst, bl.bias, B, st.R, st.R / st.w, C, st.H,
                              bl.shift, scale_log2};
      if (fuse96 && call.maps.wants(block)) {
        // The fused sublayer keeps q and k on chip: for a requested block only, the general
        // path's QKV GEMM into ws.qkv (ws.x / ws.sx stay as the sublayer reads them) and the map
        // of its q / k; the sublayer below runs unchanged (evt_window_attention.h)
        {
          ProfScope ps(m, EVT_PROF_HEAD, s);
          EVT_RC(dense(m, bl.qkv, qc, s));
        }
        EVT_RC(window_attn_map(m, call, block, st.w, ap));
      }
      if (fuse96) {  // stage-1 attention sublayer fused (swin.hip, swin_attn96_kernel)
        ProfScope ps(m, EVT_PROF_ATTN_SUBLAYER, s);
        prof_work(m, 2.0 * rows * C * 4 * C + 4.0 * rows * 49 * C,
                  2.0 * rows * C * es + 2 * slot_rows + 4.0 * C * C * es);
        SwinAttnBlockParams ab{m->ws.x, m->ws.xm, m->ws.sx, m->ws.sm, bl.qkv.w, bl.qkv.b, bl.proj.w,
                               bl.proj.b, bl.bias, bl.qkv.kpad, bl.proj.kpad, B, st.R, bl.shift,
                               stats_slots(C), m->eps};
        EVT_HIP(swin_attn96_launch(ab, s), "fused window attention sublayer");
      }
      if (!fuse96) {  // LN1-folded QKV (+ bias)
        {
          ProfScope ps(m, EVT_PROF_QKV, s);
          EVT_RC(dense(m, bl.qkv, qc, s));
        }
        {
          ProfScope ps(m, EVT_PROF_ATTENTION, s);
          prof_work(m, 4.0 * rows * st.w * st.w * C, 4.0 * rows * C * es);  // w^2 keys per query
          EVT_HIP(window_attn_launch(dt, st.w, ap, s),
                  "window attention");
        }
        EVT_RC(window_attn_map(m, call, block, st.w, ap));  // ws.qkv still holds the block
        ProfScope ps(m, EVT_PROF_OUT_PROJ, s);
        DenseCall pc;  // proj + bias + residual x -> xm (+ stats)
        pc.flags = EPI_BIAS | EPI_RESID | EPI_STATS;
        pc.A = m->ws.o; pc.lda = Cst; pc.C = m->ws.xm; pc.ldc = Cst; pc.M = rows; pc.N = Cst;
        pc.resid = m->ws.x; pc.ldr = Cst; pc.stats_out = m->ws.sm; pc.ln_width = C;
        EVT_RC(dense(m, bl.proj, pc, s));
      }
      if (dt == DT_BF16 && C == 96 && st.mlp == 384 && st.w == 7 && gemm_auto()) {
        // stage-1 MLP (C = 96) fused: hidden kept on chip (swin.hip, swin_mlp96_kernel)
        ProfScope ps(m, EVT_PROF_MLP, s);
        prof_work(m, 4.0 * rows * C * st.mlp, 2.0 * rows * C * es + 2 * slot_rows +
                                                   2.0 * C * st.mlp * es);
        SwinMlpParams mp{m->ws.xm, m->ws.x, m->ws.sm, m->ws.sx, bl.fc1.w, bl.fc1.colsum, bl.fc1.b,
                         bl.fc2.w, bl.fc2.b, bl.fc1.kpad, bl.fc2.kpad, rows, stats_slots(C),
                         m->eps};
        EVT_HIP(swin_mlp96_launch(mp, s), "fused MLP");
      } else {
      {  // LN2-folded FC1 + erf GELU
        ProfScope ps(m, EVT_PROF_FC1, s);
        DenseCall c;
        c.flags = EPI_LNIN | EPI_BIAS | EPI_GELU_ERF;
        c.A = m->ws.xm; c.lda = Cst; c.C = m->ws.hbuf; c.ldc = st.mst; c.M = rows; c.N = st.mst;
        c.stats_in = m->ws.sm; c.ln_width = C;
        EVT_RC(dense(m, bl.fc1, c, s));
      }
      {  // FC2 + bias + residual xm -> x (+ stats)
        ProfScope ps(m, EVT_PROF_FC2, s);
        DenseCall c;
        c.flags = EPI_BIAS | EPI_RESID | EPI_STATS;
        c.A = m->ws.hbuf; c.lda = st.mst; c.C = m->ws.x; c.ldc = Cst; c.M = rows; c.N = Cst;
        c.resid = m->ws.xm; c.ldr = Cst; c.stats_out = m->ws.sx; c.ln_width = C;
        EVT_RC(dense(m, bl.fc2, c, s));
      }
      }
      EVT_RC(feat_tap(m, call, block, Cst, rows, C));  // either way the block's output is in ws.x
    }
  }
  const SwinStage& sl = m->stages.back();
  const evt_features_args* fa = call.feat;
  if (fa && fa->tokens)  // LN(x) of the last stage, its padding columns [C, Cst) dropped
    EVT_RC(feat_export(m, m->ws.x, sl.Cst, 1, fa->tokens, true, B * sl.R * sl.R, sl.C, s));
  if (!logits && !(fa && fa->pooled)) return EVT_OK;
  // final LayerNorm + mean over tokens -> head Dense (fp32 logits)
  {
    ProfScope ps_head(m, EVT_PROF_HEAD, s);
    prof_work(m, 0.0, (double)B * sl.R * sl.R * sl.C * es + (double)B * sl.R * sl.R * stats_slots(sl.C) * 8 +
                          (double)B * sl.C * es);
    EVT_HIP(ln_pool_launch(dt, m->ws.x, sl.Cst, B, sl.R * sl.R, sl.C, m->ws.sx, stats_slots(sl.C),
                           m->norm_g, m->norm_b, m->ws.pooled, sl.Cst, s),
            "norm + avgpool");
    if (logits) {
      DenseCall c;
      c.flags = EPI_BIAS | EPI_OUT_F32;
      c.A = m->ws.pooled; c.lda = sl.Cst; c.C = logits; c.ldc = d.num_classes; c.M = B;
      c.N = d.num_classes;
      EVT_RC(dense(m, m->head, c, s));
    }
  }
  if (fa && fa->pooled)  // the head's operand as it stands (activation dtype) -> fp32
    EVT_RC(feat_export(m, m->ws.pooled, sl.Cst, 1, fa->pooled, false, B, sl.C, s));
  return EVT_OK;
}

}  // namespace

const FamilyOps& evt::swin_ops() {
  static const FamilyOps ops = {
      [](const ModelCore& c, int B) { return swin_ws_layout(c.swin, c.dtype, B); }, swin_run,
      swin_blocks, swin_shape,
      "attention maps: Swin's windowed, biased attention is not exported"};
  return ops;
}

extern "C" {

int evt_swin_num_weights(const evt_swin_desc* desc) {
  if (!desc || desc->num_stages < 1 || desc->num_stages > EVT_SWIN_MAX_STAGES)
    return fail(EVT_EINVAL, "bad desc");
  int n = 4 + 4;
  for (int i = 0; i < desc->num_stages; ++i) n += (i > 0 ? 3 : 0) + 13 * desc->depths[i];
  return n;
}

int evt_swin_query_workspace(const evt_swin_desc* desc, int batch, size_t* bytes) {
  SwinGeo g;
  EVT_RC(validate_swin(desc, &g));
  if (!bytes || batch <= 0) return fail(EVT_EINVAL, "bytes must be non-null and batch positive");
  *bytes = swin_ws_layout(g, desc->dtype, batch).bytes();
  return EVT_OK;
}

int evt_swin_create(const evt_swin_desc* desc, const float* const* w, int n_weights, void* stream,
                    evt_model** out) {
  SwinGeo g;
  EVT_RC(create_prologue(desc, validate_swin, &g, evt_swin_num_weights, w, n_weights, out));
  hipStream_t s = (hipStream_t)stream;
  evt_model* m = new evt_model();
  m->family = FAM_SWIN;
  m->dtype = desc->dtype;
  m->D = desc->embed_dim;
  m->max_batch = desc->max_batch;
  m->num_classes = desc->num_classes;
  m->sdesc = *desc;
  m->swin = g;
  m->in_chans = desc->in_chans;
  m->image_size = desc->image_size;
  m->patch_size = desc->patch_size;
  m->img_elems = (size_t)desc->in_chans * desc->image_size * desc->image_size;
  auto run = [&]() -> int {
    const int E = desc->embed_dim;
    int k = 0;
    EVT_RC(make_dense(m, &m->patch, w[0], w[1], g.pd, E, s));  // Conv2d(k = s = patch)
    EVT_RC(copy_vec(m, &m->pnorm_g, w[2], E, s));
    EVT_RC(copy_vec(m, &m->pnorm_b, w[3], E, s));
    k = 4;
    m->stages.resize(g.ns);
    for (int i = 0; i < g.ns; ++i) {
      SwinStage& st = m->stages[i];
      st.C = g.C[i];
      st.Cst = g.Cst[i];
      st.H = desc->num_heads[i];
      st.R = g.R[i];
      st.mlp = g.mlp[i];
      st.mst = g.mst[i];
      st.w = g.w[i];
      if (i > 0) {  // PatchMerging: LayerNorm(4C) folded into reduction Linear(4C, 2C, bias=False)
        EVT_RC(make_dense(m, &st.merge, w[k + 2], nullptr, 4 * g.C[i - 1], st.C, s, w[k], w[k + 1]));
        k += 3;
      }
      st.blocks.resize(desc->depths[i]);
      for (int j = 0; j < desc->depths[i]; ++j) {
        SwinBlock& bl = st.blocks[j];
        // SW-MSA on odd blocks; none where the stage is one window (R <= window_size)
        bl.shift = (j % 2 == 1 && st.R > desc->window_size) ? desc->window_size / 2 : 0;
        const int C = st.C;
        EVT_RC(make_dense(m, &bl.qkv, w[k + 2], w[k + 3], C, 3 * C, s, w[k + 0], w[k + 1]));
        EVT_RC(dev_alloc(m, (void**)&bl.bias, rpb_table_floats(st.H, st.w, bl.shift) * sizeof(float)));
        EVT_HIP(rpb_dense_launch(w[k + 4], st.H, st.w, bl.shift, bl.bias, s), "relative position bias");
        EVT_RC(make_dense(m, &bl.proj, w[k + 5], w[k + 6], C, C, s));
        EVT_RC(make_dense(m, &bl.fc1, w[k + 9], w[k + 10], C, st.mlp, s, w[k + 7], w[k + 8]));
        EVT_RC(make_dense(m, &bl.fc2, w[k + 11], w[k + 12], st.mlp, C, s));
        k += 13;
      }
    }
    const int nf = g.C[g.ns - 1];
    EVT_RC(copy_vec(m, &m->norm_g, w[k + 0], nf, s));
    EVT_RC(copy_vec(m, &m->norm_b, w[k + 1], nf, s));
    EVT_RC(make_dense(m, &m->head, w[k + 2], w[k + 3], nf, desc->num_classes, s));
    EVT_RC(alloc_ws(m, desc->max_batch, s));
    EVT_HIP(hipStreamSynchronize(s), "create sync");
    return EVT_OK;
  };
  return finish_create(m, run(), out);
}

int evt_swin_forward(evt_model* m, const float* img, int B, float* logits, void* stream) {
  return family_forward(m, FAM_SWIN, "model is not a Swin Transformer", img, B, logits, stream);
}

}  // extern "C"
