// T2T-ViT: descriptor checks, geometry, workspace, create and forward.
#include "model.h"

using namespace evt;

namespace {

int validate_t2t(const evt_t2t_desc* d, T2TShape* ts) {
  if (!d) return fail(EVT_EINVAL, "desc is NULL");
  if (d->dtype != EVT_DTYPE_F32 && d->dtype != EVT_DTYPE_BF16)
    return fail(EVT_EINVAL, "dtype must be EVT_DTYPE_F32 or EVT_DTYPE_BF16");
  if (d->image_size <= 0 || d->image_size % 16)
    return fail(EVT_EINVAL, "image_size must be a positive multiple of 16");
  if (d->in_chans <= 0 || d->num_classes <= 0 || d->depth < 0 || d->mlp_dim <= 0)
    return fail(EVT_EINVAL, "in_chans, num_classes, mlp_dim must be positive, depth >= 0");
  if (d->dim <= 0 || d->dim % 8 != 0 || d->dim > 1024)
    return fail(EVT_EINVAL, "dim must be a positive multiple of 8 and <= 1024");
  if (d->heads <= 0 || d->dim % d->heads != 0)  // Attention raises ValueError (attention.py:8-9)
    return fail(EVT_EINVAL, "hidden_size must be a multiple of num_heads");
  if (d->dim / d->heads > 128) return fail(EVT_EINVAL, "head size (dim / heads) must be <= 128");
  if (d->token_size != 64) return fail(EVT_EINVAL, "token_size must be 64 in this build");
  if (d->max_batch <= 0) return fail(EVT_EINVAL, "max_batch must be positive");
  const int S = d->image_size;
  ts->grid[0] = S / 4;
  ts->grid[1] = S / 8;
  ts->grid[2] = S / 16;
  ts->din[0] = 49 * d->in_chans;
  ts->din[1] = 9 * 64;
  Shape& sh = ts->enc;
  sh.P = ts->grid[2] * ts->grid[2];
  sh.T = sh.P + 1;
  if (sh.T > EVT_ATTN_MAX_TOKENS)
    return fail(EVT_EINVAL, "at most 4095 patches per image are supported");
  sh.D = d->dim;
  sh.pd = 9 * 64;
  sh.max_inner = d->dim;  // heads * (dim / heads)
  sh.max_ffn_st = (int)round_up(d->mlp_dim, PAD_N);
  sh.head_st = 0;
  if (sh.T > 256) {  // as validate(): no buffer of 2^31 bytes or more past 256 tokens
    const size_t es = d->dtype == EVT_DTYPE_F32 ? 4 : 2, B = (size_t)d->max_batch;
    const size_t t1 = (size_t)ts->grid[0] * ts->grid[0], t2 = (size_t)ts->grid[1] * ts->grid[1];
    const size_t big = std::max({B * t1 * round_up(ts->din[0], PAD_K) * es, B * t2 * ts->din[1] * es,
                                 B * t1 * 4 * 64 * es, B * sh.T * 4 * sh.max_inner * es,
                                 B * sh.T * sh.max_ffn_st * es,
                                 B * d->in_chans * S * S * sizeof(float)});
    if (big >= (size_t)1 << 31)
      return fail(EVT_EINVAL, "max_batch too large for more than 256 tokens per image: every "
                              "activation buffer must stay below 2^31 bytes");
  }
  return EVT_OK;
}

size_t t2t_unfold_elems(const T2TShape& ts, int B) {
  const size_t t1 = (size_t)ts.grid[0] * ts.grid[0], t2 = (size_t)ts.grid[1] * ts.grid[1];
  const size_t t3 = (size_t)ts.grid[2] * ts.grid[2];
  return (size_t)B * std::max({t1 * round_up(ts.din[0], PAD_K), t2 * ts.din[1], t3 * ts.din[1]});
}

size_t t2t_unfold_stat_floats(const T2TShape& ts, int B) {
  const size_t t1 = (size_t)ts.grid[0] * ts.grid[0], t2 = (size_t)ts.grid[1] * ts.grid[1];
  return (size_t)B * std::max(t1 * stats_slots(ts.din[0]), t2 * stats_slots(ts.din[1])) * 2;
}

// The T2T-ViT workspace for B images (activation buffers only; lanes allocate their own)
WsLayout t2t_ws(const T2TShape& ts, int dtype, int B) {
  WsLayout l;
  const size_t es = elem_size(dtype);
  const size_t t1 = (size_t)B * ts.grid[0] * ts.grid[0];
  l.bufs.push_back({EVT_WS(u), t2t_unfold_elems(ts, B) * es});
  l.bufs.push_back({EVT_WS(su), t2t_unfold_stat_floats(ts, B) * sizeof(float)});
  l.bufs.push_back({EVT_WS(kqvb), t1 * 3 * 64 * es});
  l.bufs.push_back({EVT_WS(pout), t1 * 64 * es});
  l.bufs.push_back({EVT_WS(tstats), t1 * 2 * sizeof(float)});
  l.bufs.push_back({EVT_WS(zrow), 256, 256, "memset zero row"});
  l.bufs.push_back({EVT_WS(part), performer_part_floats(B, ts.grid[0] * ts.grid[0]) *
                                      sizeof(float)});
  encoder_ws(ts.enc, dtype, false, B, (size_t)B * ts.enc.T * ts.enc.max_ffn_st * es, &l);
  return l;
}
// The T2T-ViT forward on this handle's own workspace (features forwards: as vit_run)
int t2t_run(evt_model* m, ForwardCall& call) {
  prof_reset(m);
  const evt_t2t_desc& d = m->tdesc;
  const int B = call.B, dt = d.dtype, D = d.dim, T = m->sh.T, P = m->sh.P, S = d.image_size;
  float* logits = call.logits;
  hipStream_t s = call.s;
  const int g1 = m->t2t.grid[0], g2 = m->t2t.grid[1];
  const int t1 = g1 * g1, t2 = g2 * g2;
  // iteration 1: soft_split0 (k7 s4 p2) of the NHWC image -> TokenPerformer    (t2t_vit.py:66-68)
  const double es = (double)elem_size(dt);
  // performer core per token (transformer_encoder.py:67-99): prm_exp of k and q (2 x 64x32),
  // D (32), kptv (32x64), y (32x64), attn_output Dense (64x64), FFN (2 x 64x64)
  const double perf_flops = 2.0 * (2 * 64 * 32 + 32 + 32 * 64 + 32 * 64 + 3 * 64 * 64);
  const Performer& P1 = m->perf[0];
  {
    ProfScope ps(m, EVT_PROF_T2T_UNFOLD, s);
    prof_work(m, 0.0, (double)B * S * S * d.in_chans * (call.img8 ? 1 : 4) +
                          (double)B * t1 * P1.din * es + (double)B * t1 * stats_slots(P1.din) * 8);
    if (call.img8)
      EVT_HIP(unfold_u8_launch(dt, call.img8, B, S, S, d.in_chans, 7, 4, 2, m->ws.u, P1.dpad,
                               m->ws.su, stats_slots(P1.din), call.aff, s),
              "soft_split0 (uint8)");
    else
      EVT_HIP(unfold_launch(dt, 1, call.img, B, S, S, d.in_chans, 7, 4, 2, m->ws.u, P1.dpad,
                            m->ws.su, stats_slots(P1.din), s),
              "soft_split0");
  }
  {
    ProfScope ps(m, EVT_PROF_T2T_KQV, s);
    DenseCall c;
    c.flags = EPI_LNIN | EPI_BIAS;
    c.A = m->ws.u; c.lda = P1.dpad; c.C = m->ws.kqvb; c.ldc = 3 * 64; c.M = B * t1; c.N = 3 * 64;
    c.stats_in = m->ws.su; c.ln_width = P1.din;
    EVT_RC(dense(m, P1.kqv, c, s));
  }
  // soft_split1 gathered inside the kqv GEMM's A loader where it can (bf16, persistent GEMM): the
  // performer then also writes per-token statistics, from which the split rows' are summed
  const Performer& P2 = m->perf[1];
  const bool gather1 = dt == DT_BF16 && P2.dpad == 9 * 64 && g2 == (g1 + 1) / 2 && m->ws.zrow;
  {
    ProfScope ps(m, EVT_PROF_T2T_PERFORMER, s);
    prof_work(m, perf_flops * B * t1, (double)B * t1 * (3 * 64 + 64) * es);
    EVT_HIP(performer_launch(dt, m->ws.kqvb, 3 * 64, B, t1, P1.w, m->ws.part, m->ws.pout, 64, s,
                             gather1 ? m->ws.tstats : nullptr, dt == DT_BF16),
            "performer1");
  }
  // iteration 2: soft_split1 (k3 s2 p1) of the [B, S/4, S/4, 64] map -> TokenPerformer (:72-77)
  bool fused1 = false;
  if (gather1) {
    ProfScope ps(m, EVT_PROF_T2T_KQV, s);
    DenseCall c;
    c.flags = EPI_LNIN | EPI_BIAS | EPI_SPLIT;
    c.A = m->ws.pout; c.lda = 64; c.C = m->ws.kqvb; c.ldc = 3 * 64; c.M = B * t2; c.N = 3 * 64;
    c.stats_in = m->ws.su; c.ln_width = P2.din;
    GemmParams p = dense_params(m, P2.kqv, c);
    p.gmode = 2; p.gR = g1; p.gC = 64; p.gOW = g2; p.gzero = m->ws.zrow;
    p.g_inv_rr = 1.0f / (float)(g2 * g2); p.g_inv_r = 1.0f / (float)g2;
    EVT_HIP(unfold_stats_launch(m->ws.tstats, B, g1, m->ws.su, stats_slots(P2.din), s),
            "soft_split1 statistics");
    const hipError_t e = gemm_launch(dt, c.flags, p, s);
    if (e == hipSuccess) {
      c.flags &= ~EPI_SPLIT;
      dense_work(m, P2.kqv, c);
      fused1 = true;
    } else if (e != hipErrorNotSupported) {
      EVT_HIP(e, "soft_split1 + kqv (gathered)");
    }
  }
  if (!fused1) {
    {
      ProfScope ps(m, EVT_PROF_T2T_UNFOLD, s);
      prof_work(m, 0.0, (double)B * t1 * 64 * es + (double)B * t2 * P2.din * es +
                            (double)B * t2 * stats_slots(P2.din) * 8);
      EVT_HIP(unfold_launch(dt, 0, m->ws.pout, B, g1, g1, 64, 3, 2, 1, m->ws.u, P2.dpad, m->ws.su,
                            stats_slots(P2.din), s),
              "soft_split1");
    }
    ProfScope ps(m, EVT_PROF_T2T_KQV, s);
    DenseCall c;
    c.flags = EPI_LNIN | EPI_BIAS;
    c.A = m->ws.u; c.lda = P2.dpad; c.C = m->ws.kqvb; c.ldc = 3 * 64; c.M = B * t2; c.N = 3 * 64;
    c.stats_in = m->ws.su; c.ln_width = P2.din;
    EVT_RC(dense(m, P2.kqv, c, s));
  }
  {
    ProfScope ps(m, EVT_PROF_T2T_PERFORMER, s);
    prof_work(m, perf_flops * B * t2, (double)B * t2 * (3 * 64 + 64) * es);
    EVT_HIP(performer_launch(dt, m->ws.kqvb, 3 * 64, B, t2, P2.w, m->ws.part, m->ws.pout, 64, s,
                             nullptr, dt == DT_BF16),
            "performer2");
  }
  // soft_split2 -> project Dense(D) into token rows 1..P, + CLS row, + sinusoid pos (:81-86,121-125)
  // (the split gathered inside the project GEMM's A loader where it can, as soft_split1)
  const int g3 = m->t2t.grid[2];
  bool fused2 = false;
  if (dt == DT_BF16 && g3 == (g2 + 1) / 2 && m->ws.zrow && m->pos_h) {
    ProfScope ps(m, EVT_PROF_PATCH_EMBED, s);
    prof_work(m, 0.0, (double)B * D * es + (double)B * stats_slots(D) * 8);
    EVT_HIP(cls_rows_launch(dt, m->ws.x, B, T, D, m->cls, m->pos, m->ws.sx, s), "cls rows");
    DenseCall c;
    c.flags = EPI_BIAS | EPI_POS | EPI_STATS | EPI_SPLIT;
    c.A = m->ws.pout; c.lda = 64; c.C = m->ws.x; c.ldc = D; c.M = B * P; c.N = D;
    c.pos = m->pos; c.ldp = D; c.P = P; c.stats_out = m->ws.sx;
    c.resid = m->pos_h; c.ldr = D;
    GemmParams p = dense_params(m, m->project, c);
    p.gmode = 2; p.gR = g2; p.gC = 64; p.gOW = g3; p.gzero = m->ws.zrow;
    p.g_inv_rr = 1.0f / (float)(g3 * g3); p.g_inv_r = 1.0f / (float)g3;
    const hipError_t e = gemm_launch(dt, c.flags, p, s);
    if (e == hipSuccess) {
      c.flags &= ~EPI_SPLIT;
      dense_work(m, m->project, c);
      fused2 = true;
    } else if (e != hipErrorNotSupported) {
      EVT_HIP(e, "soft_split2 + project (gathered)");
    }
  }
  if (!fused2) {
    {
      ProfScope ps(m, EVT_PROF_T2T_UNFOLD, s);
      prof_work(m, 0.0, (double)B * t2 * 64 * es + (double)B * P * 9 * 64 * es);
      EVT_HIP(unfold_launch(dt, 0, m->ws.pout, B, g2, g2, 64, 3, 2, 1, m->ws.u, 9 * 64, nullptr, 0,
                            s),
              "soft_split2");
    }
    ProfScope ps(m, EVT_PROF_PATCH_EMBED, s);
    prof_work(m, 0.0, (double)B * D * es + (double)B * stats_slots(D) * 8);
    EVT_HIP(cls_rows_launch(dt, m->ws.x, B, T, D, m->cls, m->pos, m->ws.sx, s), "cls rows");
    DenseCall c;
    c.flags = EPI_BIAS | EPI_POS | EPI_STATS;
    c.A = m->ws.u; c.lda = 9 * 64; c.C = m->ws.x; c.ldc = D; c.M = B * P; c.N = D;
    c.pos = m->pos; c.ldp = D; c.P = P; c.stats_out = m->ws.sx;
    EVT_RC(dense(m, m->project, c, s));
  }
  EVT_RC(run_encoder(m, call));  // :127
  if (call.feat) EVT_RC(encoder_features(m, call));
  if (!logits) return EVT_OK;
  {  // LayerNorm of the CLS rows folded into the classifier (:129-134)
    ProfScope ps(m, EVT_PROF_HEAD, s);
    DenseCall c;
    c.flags = EPI_LNIN | EPI_BIAS | EPI_OUT_F32;
    c.A = m->ws.x; c.lda = (int64_t)T * D; c.C = logits; c.ldc = d.num_classes; c.M = B;
    c.N = d.num_classes; c.stats_in = m->ws.sx; c.stats_step = T;
    EVT_RC(dense(m, m->head, c, s));
  }
  return EVT_OK;
}

}  // namespace

const FamilyOps& evt::t2t_ops() {
  static const FamilyOps ops = {[](const ModelCore& c, int B) { return t2t_ws(c.t2t, c.dtype, B); },
                                t2t_run, encoder_blocks, encoder_shape, nullptr};
  return ops;
}

extern "C" {

int evt_t2t_num_weights(const evt_t2t_desc* desc) {
  if (!desc || desc->depth < 0) return fail(EVT_EINVAL, "bad desc");
  return 2 * 13 + 4 + 11 * desc->depth + 4;
}

int evt_t2t_query_workspace(const evt_t2t_desc* desc, int batch, size_t* bytes) {
  T2TShape ts;
  EVT_RC(validate_t2t(desc, &ts));
  if (!bytes || batch <= 0) return fail(EVT_EINVAL, "bytes must be non-null and batch positive");
  *bytes = t2t_ws(ts, desc->dtype, batch).bytes();
  return EVT_OK;
}

int evt_t2t_create(const evt_t2t_desc* desc, const float* const* w, int n_weights, void* stream,
                   evt_model** out) {
  T2TShape ts;
  EVT_RC(create_prologue(desc, validate_t2t, &ts, evt_t2t_num_weights, w, n_weights, out));
  hipStream_t s = (hipStream_t)stream;
  evt_model* m = new evt_model();
  m->family = FAM_T2T;
  m->dtype = desc->dtype;
  m->D = desc->dim;
  m->max_batch = desc->max_batch;
  m->num_classes = desc->num_classes;
  m->tdesc = *desc;
  m->heads.assign(desc->depth, desc->heads);
  m->head_dim.assign(desc->depth, desc->dim / desc->heads);  // h_k = dim // heads
  m->ffn.assign(desc->depth, desc->mlp_dim);
  m->sh = ts.enc;
  m->t2t = ts;
  m->in_chans = desc->in_chans;
  m->image_size = desc->image_size;
  m->img_elems = (size_t)desc->image_size * desc->image_size * desc->in_chans;
  const int D = desc->dim;
  auto run = [&]() -> int {
    int k = 0;
    for (int pi = 0; pi < 2; ++pi) {  // transformer_encoder.py:43-65
      Performer& P = m->perf[pi];
      P.din = ts.din[pi];
      P.dpad = (int)round_up(P.din, PAD_K);
      if (m->dtype == DT_BF16) {  // output columns permuted for the performers' 16-B loads
        float *wp = nullptr, *bp = nullptr;
        EVT_RC(dev_alloc(m, (void**)&wp, (size_t)P.din * 3 * 64 * sizeof(float)));
        EVT_RC(dev_alloc(m, (void**)&bp, 3 * 64 * sizeof(float)));
        EVT_HIP(kqv_permute_launch(w[k + 2], w[k + 3], P.din, wp, bp, s), "kqv permute");
        EVT_RC(make_dense(m, &P.kqv, wp, bp, P.din, 3 * 64, s, w[k + 0], w[k + 1]));
      } else {
        EVT_RC(make_dense(m, &P.kqv, w[k + 2], w[k + 3], P.din, 3 * 64, s, w[k + 0], w[k + 1]));
      }
      const float* src[9] = {w[k + 4], w[k + 5], w[k + 6], w[k + 7], w[k + 8],
                             w[k + 9], w[k + 10], w[k + 11], w[k + 12]};
      const size_t len[9] = {32 * 64, 64 * 64, 64, 64, 64, 64 * 64, 64, 64 * 64, 64};
      float* dst[9];
      for (int j = 0; j < 9; ++j) EVT_RC(copy_vec(m, &dst[j], src[j], len[j], s));
      P.w = PerformerWeights{dst[0], dst[1], dst[2], dst[3], dst[4], dst[5], dst[6], dst[7], dst[8]};
      k += 13;
    }
    EVT_RC(make_dense(m, &m->project, w[k + 0], w[k + 1], 9 * 64, D, s));  // t2t_vit.py:56,86
    EVT_RC(copy_vec(m, &m->cls, w[k + 2], D, s));
    EVT_RC(copy_vec(m, &m->pos, w[k + 3], (size_t)ts.enc.T * D, s));
    if (desc->dtype == DT_BF16) {  // bf16 table for the persistent project GEMM (EPI_POS)
      EVT_RC(dev_alloc(m, &m->pos_h, (size_t)ts.enc.T * D * 2));
      EVT_HIP(to_bf16_launch(m->pos, m->pos_h, (int64_t)ts.enc.T * D, s), "pos -> bf16");
    }
    k += 4;
    EVT_RC(build_encoder(m, w + k, s));
    k += 11 * desc->depth;
    // final LayerNorm (t2t_vit.py:111,129) folded into the classifier (:114,134)
    EVT_RC(make_dense(m, &m->head, w[k + 2], w[k + 3], D, desc->num_classes, s, w[k + 0], w[k + 1]));
    EVT_RC(copy_vec(m, &m->norm_g, w[k + 0], D, s));  // unfolded, for the feature outputs
    EVT_RC(copy_vec(m, &m->norm_b, w[k + 1], D, s));
    EVT_RC(alloc_ws(m, desc->max_batch, s));
    EVT_HIP(hipStreamSynchronize(s), "create sync");
    return EVT_OK;
  };
  return finish_create(m, run(), out);
}

int evt_t2t_forward(evt_model* m, const float* img, int B, float* logits, void* stream) {
  return family_forward(m, FAM_T2T, "model is not a T2T-ViT (use evt_vit_forward)", img, B, logits,
                        stream);
}

}  // extern "C"
