// ViT / ViT_Pruned / STANDARD ViT: descriptor checks, geometry, workspace, create and forward.
#include "model.h"

using namespace evt;

namespace {

int validate(const evt_vit_desc* d, Shape* sh) {
  if (!d) return fail(EVT_EINVAL, "desc is NULL");
  if (d->dtype != EVT_DTYPE_F32 && d->dtype != EVT_DTYPE_BF16 && d->dtype != EVT_DTYPE_MX8)
    return fail(EVT_EINVAL, "dtype must be EVT_DTYPE_F32, EVT_DTYPE_BF16 or EVT_DTYPE_MX8");
  if (d->dtype == EVT_DTYPE_MX8 && d->semantics != EVT_VIT_REFERENCE)
    return fail(EVT_EINVAL, "EVT_DTYPE_MX8 supports EVT_VIT_REFERENCE semantics only");
  if (d->patch_size <= 0 || d->image_size <= 0 || d->image_size % d->patch_size != 0)
    return fail(EVT_EINVAL, "image dimensions must be divisible by the patch size");
  if (d->in_chans <= 0 || d->num_classes <= 0 || d->depth < 0 || d->mlp_dim <= 0)
    return fail(EVT_EINVAL, "in_chans, num_classes, mlp_dim must be positive, depth >= 0");
  if (d->dim <= 0 || d->dim % 8 != 0 || d->dim > 1536)
    return fail(EVT_EINVAL, "dim must be a positive multiple of 8 and <= 1536");
  if (d->dtype == EVT_DTYPE_MX8 && d->dim > 1024)
    return fail(EVT_EINVAL, "EVT_DTYPE_MX8 supports dim <= 1024 (the MX8 LayerNorm quantizer holds "
                            "rows of at most 1024 columns); wider models run in bf16 or f32");
  if (d->dtype == EVT_DTYPE_MX8 && d->dim % 64 != 0)
    return fail(EVT_EINVAL, "EVT_DTYPE_MX8 needs dim % 64 == 0");
  if (d->max_batch <= 0) return fail(EVT_EINVAL, "max_batch must be positive");
  if (d->semantics != EVT_VIT_REFERENCE && d->semantics != EVT_VIT_STANDARD)
    return fail(EVT_EINVAL, "semantics must be EVT_VIT_REFERENCE or EVT_VIT_STANDARD");
  if (d->layer_norm_eps < 0.f) return fail(EVT_EINVAL, "layer_norm_eps must be >= 0");
  if (d->depth > 0 && (!d->heads || !d->head_dim || !d->ffn))
    return fail(EVT_EINVAL, "heads/head_dim/ffn arrays are required");
  const int np = d->image_size / d->patch_size;
  sh->P = np * np;
  sh->T = sh->P + 1;
  if (sh->T > EVT_ATTN_MAX_TOKENS)
    return fail(EVT_EINVAL, "at most 4095 patches per image are supported");
  if (d->dtype == EVT_DTYPE_MX8 && sh->T > 256)
    return fail(EVT_EINVAL, "EVT_DTYPE_MX8 supports at most 255 patches per image (its attention "
                            "kernel writes MX8 output for up to 256 tokens only)");
  sh->pd = d->patch_size * d->patch_size * d->in_chans;
  // pd % 64 != 0 (patch 14: 588): rows at the next multiple of 64, the tail zeroed by the kernel
  sh->pdst = (int)round_up(sh->pd, PAD_K);
  if (d->patch_size * d->image_size % 4)
    return fail(EVT_EINVAL, "patch_size * image_size must be a multiple of 4");
  if ((size_t)d->in_chans * d->patch_size * d->image_size * 4 > 160 * 1024)
    return fail(EVT_EINVAL, "image strip exceeds LDS");
  sh->D = d->dim;
  sh->max_inner = 0;
  sh->max_ffn_st = 0;
  for (int i = 0; i < d->depth; ++i) {
    if (d->heads[i] <= 0) return fail(EVT_EINVAL, "heads per layer must be positive");
    // any h_k (attention.py:6-12) up to 128; 64 runs the tuned kernels, others the generic ones
    if (d->head_dim[i] <= 0 || d->head_dim[i] > 128)
      return fail(EVT_EINVAL, "head size must be in [1, 128]");
    if (d->heads[i] * d->head_dim[i] % 8)
      return fail(EVT_EINVAL, "heads * head size must be a multiple of 8 (16-B token rows)");
    if (d->dtype == EVT_DTYPE_MX8 && d->head_dim[i] != 64)
      return fail(EVT_EINVAL, "EVT_DTYPE_MX8 supports head size 64 only");
    if (d->ffn[i] <= 0) return fail(EVT_EINVAL, "ffn width per layer must be positive");
    sh->max_inner = std::max(sh->max_inner, d->heads[i] * d->head_dim[i]);
    sh->max_ffn_st = std::max<int>(sh->max_ffn_st, (int)round_up(d->ffn[i], PAD_N));
  }
  sh->head_st = (int)round_up(d->mlp_dim, PAD_N);
  if (sh->T > 256) {
    // Several kernels form byte offsets into an activation buffer in 32 bits. Up to 256 tokens the
    // supported batches were measured as they are; past them the create call refuses a max_batch
    // whose largest buffer (image batch, patch matrix, qkv, FFN hidden) would reach 2^31 bytes.
    const size_t es = d->dtype == EVT_DTYPE_F32 ? 4 : 2, B = (size_t)d->max_batch;
    const size_t widest = std::max<size_t>({(size_t)3 * sh->max_inner, (size_t)sh->max_ffn_st,
                                            (size_t)sh->D});
    const size_t big = std::max({B * sh->T * widest * es, B * sh->P * sh->pdst * es,
                                 B * d->in_chans * d->image_size * d->image_size * sizeof(float)});
    if (big >= (size_t)1 << 31)
      return fail(EVT_EINVAL, "max_batch too large for more than 256 tokens per image: every "
                              "activation buffer must stay below 2^31 bytes");
  }
  return EVT_OK;
}

// The ViT workspace for B images (activation buffers only; lanes allocate their own). dtype: the
// activation dtype (bf16 for an MX8 model).
WsLayout vit_ws(const Shape& sh, int dtype, bool mx8, int B) {
  WsLayout l;
  const size_t es = elem_size(dtype);
  encoder_ws(sh, dtype, mx8, B, std::max((size_t)B * sh.T * sh.max_ffn_st,
                                         (size_t)B * sh.P * sh.pdst) * es, &l);
  l.patch_in_hbuf = true;
  l.bufs.push_back({EVT_WS(hh), (size_t)B * sh.head_st * es});
  if (mx8) {
    const size_t rows = (size_t)B * sh.T;
    l.qa_ld = (int)std::max(round_up(sh.D, 128), round_up(sh.max_inner, 128));
    // the widest ffn rounded up to 128 (max_ffn_st is it rounded up to PAD_N = 64 already)
    l.qh_ld = (int)round_up(sh.max_ffn_st, 128);
    const size_t qa = rows * l.qa_ld, sa = rows * (l.qa_ld / 128) * 4;
    const size_t qh = rows * l.qh_ld, shd = rows * (l.qh_ld / 128) * 4;
    // every byte of the MX8 operands is written finite before it is read (NaN-free padding); FC1
    // writes columns < roundup(ffn, 32) only: the rest of the FC2 operand stays zero
    l.bufs.push_back({EVT_WS(qa), qa, qa, "memset qa"});
    l.bufs.push_back({EVT_WS(sa), sa, sa, "memset qa scales"});
    l.bufs.push_back({EVT_WS(qh), qh, qh, "memset qh"});
    l.bufs.push_back({EVT_WS(shd), shd, shd, "memset qh scales"});
    l.bufs.push_back({EVT_WS(lnst), rows * 2 * sizeof(float)});
  }
  return l;
}
// The ViT forward of call.B images on this handle's own workspace. In a features forward
// (call.feat) the taps, tokens and pooled are exported along the way and logits may be NULL (no
// head then).
int vit_run(evt_model* m, ForwardCall& call) {
  const evt_vit_desc& d = m->desc;
  const Shape& sh = m->sh;
  const int B = call.B, D = d.dim, dt = m->dtype;
  const float* img = call.img;
  float* logits = call.logits;
  hipStream_t s = call.s;
  prof_reset(m);
  // a token schedule swaps the roles of x / xm and sx / sm at every scheduled block (encoder.cpp
  // token_prune): the handle gets its own pointers back once the call is enqueued, however it ends
  struct StreamRoles {
    Workspace& ws;
    void *x, *xm;
    float *sx, *sm;
    ~StreamRoles() { ws.x = x; ws.xm = xm; ws.sx = sx; ws.sm = sm; }
  } roles{m->ws, m->ws.x, m->ws.xm, m->ws.sx, m->ws.sm};
  // patch embedding (vit.py:45-51): rearrange -> Dense(D) + pos, CLS row = cls + pos[0]
  {
    ProfScope ps(m, EVT_PROF_PATCHIFY, s);
    prof_work(m, 0.0, (double)B * d.in_chans * d.image_size * d.image_size * (call.img8 ? 1 : 4) +
                          (double)B * (sh.P * sh.pdst + D) * elem_size(dt) +
                          (double)B * stats_slots(D) * 8);  // image read, patch rows + CLS rows
    if (call.img8)  // uint8 NHWC (evt_forward_image): channel-major rows at stride pdst
      EVT_HIP(patchify_u8_launch(dt, call.img8, B, d.in_chans, d.image_size, d.patch_size,
                                 m->ws.apatch, sh.pdst, m->ws.x, m->cls, m->pos, D, m->ws.sx,
                                 call.aff, s),
              "patchify (uint8)");
    else if (m->patch_ld)
      EVT_HIP(patchify_ld_launch(dt, img, B, d.in_chans, d.image_size, d.patch_size, m->ws.apatch,
                                 sh.pdst, m->ws.x, m->cls, m->pos, D, m->ws.sx, s),
              "patchify");
    else
      EVT_HIP(patchify_launch(dt, img, B, d.in_chans, d.image_size, d.patch_size, m->ws.apatch,
                              m->ws.x, m->cls, m->pos, D, m->ws.sx, s, m->patch_cm),
              "patchify");
  }
  {
    ProfScope ps(m, EVT_PROF_PATCH_EMBED, s);
    DenseCall c;
    c.flags = EPI_BIAS | EPI_POS | EPI_STATS;
    c.A = m->ws.apatch; c.lda = sh.pdst; c.C = m->ws.x; c.ldc = D; c.M = B * sh.P; c.N = D;
    c.pos = m->pos; c.ldp = D; c.P = sh.P; c.stats_out = m->ws.sx;
    c.resid = m->pos_h; c.ldr = m->pos_h ? D : 0;  // bf16 table for the persistent kernel
    EVT_RC(dense(m, m->patch, c, s));
  }
  call.T = sh.T;
  EVT_RC(m->mx8 ? run_encoder_mx8(m, call) : run_encoder(m, call));
  const int T = call.T;  // tokens per image of the stream the last block left (token schedule)
  if (call.feat) EVT_RC(encoder_features(m, call));
  if (!logits) return EVT_OK;
  ProfScope ps_head(m, EVT_PROF_HEAD, s);
  if (m->standard) {  // final LayerNorm of the CLS rows folded into the Linear head
    DenseCall c;
    c.flags = EPI_LNIN | EPI_BIAS | EPI_OUT_F32;
    c.A = m->ws.x; c.lda = (int64_t)T * D; c.C = logits; c.ldc = d.num_classes; c.M = B;
    c.N = d.num_classes; c.stats_in = m->ws.sx; c.stats_step = T;
    EVT_RC(dense(m, m->head, c, s));
    return EVT_OK;
  }
  // head on token 0 (vit.py:54-55; no final LayerNorm): rows b*T of the stream, stride T*D
  {
    DenseCall c;
    c.flags = EPI_BIAS | EPI_GELU;
    c.A = m->ws.x; c.lda = (int64_t)T * D; c.C = m->ws.hh; c.ldc = sh.head_st; c.M = B;
    c.N = sh.head_st;
    EVT_RC(dense_head(m, m->head1, c, s));
  }
  {
    DenseCall c;
    c.flags = EPI_BIAS | EPI_OUT_F32;
    c.A = m->ws.hh; c.lda = sh.head_st; c.C = logits; c.ldc = d.num_classes; c.M = B;
    c.N = d.num_classes;
    EVT_RC(dense_head(m, m->head2, c, s));
  }
  return EVT_OK;
}

}  // namespace

const FamilyOps& evt::vit_ops() {
  static const FamilyOps ops = {
      [](const ModelCore& c, int B) { return vit_ws(c.sh, c.dtype, c.mx8, B); }, vit_run,
      encoder_blocks, encoder_shape, nullptr};
  return ops;
}

extern "C" {

int evt_vit_num_weights(const evt_vit_desc* desc) {
  if (!desc || desc->depth < 0) return fail(EVT_EINVAL, "bad desc");
  return 4 + (desc->semantics == EVT_VIT_STANDARD ? 12 : 11) * desc->depth + 4;
}

int evt_query_workspace(const evt_vit_desc* desc, int batch, size_t* bytes) {
  Shape sh;
  EVT_RC(validate(desc, &sh));
  if (!bytes || batch <= 0) return fail(EVT_EINVAL, "bytes must be non-null and batch positive");
  const bool mx8 = desc->dtype == EVT_DTYPE_MX8;
  *bytes = vit_ws(sh, mx8 ? DT_BF16 : desc->dtype, mx8, batch).bytes();
  return EVT_OK;
}

int evt_vit_create(const evt_vit_desc* desc, const float* const* w, int n_weights, void* stream,
                   evt_model** out) {
  Shape sh;
  EVT_RC(create_prologue(desc, validate, &sh, evt_vit_num_weights, w, n_weights, out));
  hipStream_t s = (hipStream_t)stream;
  evt_model* m = new evt_model();
  m->family = FAM_VIT;
  m->mx8 = desc->dtype == EVT_DTYPE_MX8;
  m->dtype = m->mx8 ? DT_BF16 : desc->dtype;  // MX8 models keep bf16 for everything else
  m->D = desc->dim;
  m->max_batch = desc->max_batch;
  m->num_classes = desc->num_classes;
  m->desc = *desc;
  m->standard = desc->semantics == EVT_VIT_STANDARD;
  if (desc->layer_norm_eps > 0.f) m->eps = desc->layer_norm_eps;
  m->heads.assign(desc->heads, desc->heads + desc->depth);
  m->head_dim.assign(desc->head_dim, desc->head_dim + desc->depth);
  m->ffn.assign(desc->ffn, desc->ffn + desc->depth);
  m->bind_desc();
  m->sh = sh;
  m->in_chans = desc->in_chans;
  m->image_size = desc->image_size;
  m->patch_size = desc->patch_size;
  m->img_elems = (size_t)desc->in_chans * desc->image_size * desc->image_size;
  const int D = desc->dim;
  auto run = [&]() -> int {
    m->patch_ld = sh.pd % PAD_K != 0;
    if (desc->patch_size % 8 == 0 || m->patch_ld) {
      // channel-major patch vectors (patchify_cm_kernel; patchify_ld_kernel with its rows padded
      // to sh.pdst columns: make_dense packs K = pd rows and zero rows up to kpad = pdst)
      float* wcm = nullptr;
      EVT_RC(dev_alloc(m, (void**)&wcm, (size_t)sh.pd * D * sizeof(float)));
      EVT_HIP(patch_weight_cm(w[0], wcm, desc->in_chans, desc->patch_size, D, s), "patch weight");
      EVT_RC(make_dense(m, &m->patch, wcm, w[1], sh.pd, D, s));
      m->patch_cm = !m->patch_ld;
    } else {
      EVT_RC(make_dense(m, &m->patch, w[0], w[1], sh.pd, D, s));
    }
    EVT_RC(copy_vec(m, &m->cls, w[2], D, s));
    EVT_RC(copy_vec(m, &m->pos, w[3], (size_t)sh.T * D, s));
    if (m->dtype == DT_BF16) {
      EVT_RC(dev_alloc(m, &m->pos_h, (size_t)sh.T * D * 2));
      EVT_HIP(to_bf16_launch(m->pos, m->pos_h, (int64_t)sh.T * D, s), "pos -> bf16");
    }
    EVT_RC(build_encoder(m, w + 4, s));
    const int k = 4 + (m->standard ? 12 : 11) * desc->depth;
    if (m->standard) {  // final LayerNorm folded into the classifier (CLS rows)
      EVT_RC(make_dense(m, &m->head, w[k + 2], w[k + 3], D, desc->num_classes, s, w[k + 0],
                        w[k + 1]));
      EVT_RC(copy_vec(m, &m->norm_g, w[k + 0], D, s));  // unfolded, for the feature outputs
      EVT_RC(copy_vec(m, &m->norm_b, w[k + 1], D, s));
    } else {
      EVT_RC(make_dense(m, &m->head1, w[k + 0], w[k + 1], D, desc->mlp_dim, s));
      EVT_RC(make_dense(m, &m->head2, w[k + 2], w[k + 3], desc->mlp_dim, desc->num_classes, s));
    }
    EVT_RC(alloc_ws(m, desc->max_batch, s));
    EVT_HIP(hipStreamSynchronize(s), "create sync");
    return EVT_OK;
  };
  return finish_create(m, run(), out);
}

int evt_vit_forward(evt_model* m, const float* img, int B, float* logits, void* stream) {
  return family_forward(m, FAM_VIT, "model is not a ViT (use evt_t2t_forward)", img, B, logits, stream);
}

}  // extern "C"
