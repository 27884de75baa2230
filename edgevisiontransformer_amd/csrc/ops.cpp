// Op-level entry points of include/evt.h and its companion headers: the calls that take no
// evt_model (the kernels one at a time, for the parity tests and for callers with their own model).
#include "model.h"

using namespace evt;

// What evt_classify checks of its arguments (the logits pointer aside); evt_forward_classify
// shares it. Fills the launch parameters.
int evt::validate_classify(const evt_classify_args* a, int B, int C, int64_t ldl,
                           ClassifyParams* p) {
  if (!a) return fail(EVT_EINVAL, "classify: the classify arguments are NULL");
  if (B < 1) return fail(EVT_EINVAL, "classify: batch must be at least 1");
  if (C < 1 || C > (1 << 20)) return fail(EVT_EINVAL, "classify: num_classes must be in [1, 2^20]");
  if (ldl < C) return fail(EVT_EINVAL, "classify: ldl must be at least num_classes");
  const int kmax = std::min(C, EVT_CLASSIFY_MAX_K);
  if (a->k < 1 || a->k > kmax)
    return fail(EVT_EINVAL, "classify: k must be in [1, min(num_classes, EVT_CLASSIFY_MAX_K) = " +
                                std::to_string(kmax) + "]");
  if (a->values != EVT_CLASSIFY_PROB && a->values != EVT_CLASSIFY_LOGIT)
    return fail(EVT_EINVAL, "classify: values must be EVT_CLASSIFY_PROB or EVT_CLASSIFY_LOGIT");
  if (!a->indices && !a->vals && !a->lse && !a->rank && !a->counters)
    return fail(EVT_EINVAL, "classify: no output requested: indices, vals, lse, rank and counters "
                            "are NULL");
  if ((a->rank || a->counters) && !a->labels)
    return fail(EVT_EINVAL, "classify: rank and counters need labels");
  if (((uintptr_t)a->indices | (uintptr_t)a->vals | (uintptr_t)a->lse | (uintptr_t)a->labels |
       (uintptr_t)a->rank) & 3)
    return fail(EVT_EINVAL, "classify: indices, vals, lse, labels and rank must be 4-byte aligned");
  if ((uintptr_t)a->counters & 7)
    return fail(EVT_EINVAL, "classify: counters must be 8-byte aligned");
  p->k = a->k;
  p->values = a->values == EVT_CLASSIFY_LOGIT ? CLS_LOGIT : CLS_PROB;
  p->indices = a->indices; p->vals = a->vals; p->lse = a->lse;
  p->labels = a->labels; p->rank = a->rank; p->counters = (long long*)a->counters;
  return EVT_OK;
}

extern "C" {

int evt_set_gemm_variant(int variant) {
  if (!gemm_variant_supported(variant))
    return fail(EVT_EINVAL, "variant must be 0, 1, 2, 6, 8, 9, 16, 30, 31 or 36");
  gemm_set_variant(variant);
  return EVT_OK;
}

int evt_pack_weight(int dtype, const float* W, const float* row_scale, int K, int N, void* Wp,
                    int Kpad, int Npad, void* stream) {
  if (!W || !Wp || K <= 0 || N <= 0 || Kpad < K || Npad < N || Kpad % PAD_K || Npad % GEMM_BN)
    return fail(EVT_EINVAL, "pack: bad shape (Npad % 128, Kpad % 64, Kpad >= K, Npad >= N)");
  EVT_HIP(pack_weight(dtype, W, row_scale, K, N, Wp, Kpad, Npad, (hipStream_t)stream),
          "pack_weight");
  return EVT_OK;
}

int evt_mx8_quantize(int in_dtype, const void* x, int64_t ldx, int rows, int K, int Kpad, void* q,
                     int64_t ldq, uint32_t* scales, int64_t ld_s, void* stream) {
  if (!x || !q || !scales || rows < 0 || K <= 0 || K % 8 || Kpad < K || Kpad % 128 ||
      ldx < K || ldq < Kpad || ld_s < rows || ldq % 8 ||
      (in_dtype != EVT_DTYPE_F32 && in_dtype != EVT_DTYPE_BF16) ||
      ldx % (in_dtype == EVT_DTYPE_F32 ? 4 : 8))
    return fail(EVT_EINVAL, "mx8_quantize: bad shape (K % 8, Kpad % 128, aligned rows)");
  EVT_HIP(mx8_quantize_launch(in_dtype, x, ldx, rows, K, Kpad, q, ldq, scales, ld_s,
                              (hipStream_t)stream),
          "mx8_quantize");
  return EVT_OK;
}

int evt_mx8_pack_weight(const float* W, const float* row_scale, int K, int N, void* Wq, int Kpad,
                        int Npad, uint32_t* scales, void* stream) {
  if (!W || !Wq || !scales || K <= 0 || N <= 0 || Kpad < K || Npad < N || Kpad % 128 ||
      Npad % 128)
    return fail(EVT_EINVAL, "mx8_pack: bad shape (Kpad % 128, Npad % 128)");
  EVT_HIP(mx8_pack_launch(W, row_scale, K, N, Wq, Kpad, Npad, scales, (hipStream_t)stream),
          "mx8_pack");
  return EVT_OK;
}

int evt_dense_mx8(const evt_dense_mx8_args* a, void* stream) {
  if (!a || !a->A || !a->a_scales || !a->Wq || !a->w_scales || !a->C || a->M < 0 || a->N <= 0 ||
      a->N % 8 || a->N > a->Npad || a->Kpad <= 0 || a->Kpad % 128 || a->Npad % 128 ||
      a->lda < a->Kpad || a->lda % 16 || a->ld_as < a->M || a->ldc < a->N || a->ldc % 8)
    return fail(EVT_EINVAL, "dense_mx8: bad shape (N % 8, Kpad % 128, Npad % 128, lda % 16)");
  const int f = a->flags;
  if ((f & EPI_BIAS) && !a->bias) return fail(EVT_EINVAL, "dense_mx8: bias flag without bias");
  if ((f & EPI_RESID) && (!a->resid || a->ldr < a->N || a->ldr % 8))
    return fail(EVT_EINVAL, "dense_mx8: bad resid");
  if ((f & EPI_RESLN) && (!(f & EPI_RESID) || !a->rstats || !a->rgamma || !a->rbeta))
    return fail(EVT_EINVAL, "dense_mx8: LN residual needs resid, rstats, rgamma, rbeta");
  if (f & (EPI_LNIN | EPI_STATS | EPI_POS))
    return fail(EVT_EINVAL, "dense_mx8: unsupported flags");
  if ((f & EPI_OUT_MX8) && (!a->c_scales || a->N % 32 || a->ld_cs < a->M))
    return fail(EVT_EINVAL, "dense_mx8: MX8 output needs c_scales, N % 32, ld_cs >= M");
  Mx8GemmParams p{};
  p.A = (const uint8_t*)a->A; p.lda = a->lda; p.As = a->a_scales; p.ldas = a->ld_as;
  p.W = (const uint8_t*)a->Wq; p.ldw = a->Kpad; p.Ws = a->w_scales; p.ldws = a->Npad;
  p.C = a->C; p.ldc = a->ldc; p.Cs = a->c_scales; p.ldcs = a->ld_cs;
  p.M = a->M; p.N = a->N; p.K = a->Kpad;
  p.bias = a->bias; p.resid = a->resid; p.ldr = a->ldr;
  p.rstats = a->rstats; p.rgamma = a->rgamma; p.rbeta = a->rbeta;
  hipError_t e = gemm_mx8_launch(f, p, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(EVT_EINVAL, "dense_mx8: unsupported flags");
  EVT_HIP(e, "dense_mx8");
  return EVT_OK;
}

int evt_mx8_layernorm(const void* x, int rows, int D, int Kpad, const float* gamma,
                      const float* beta, float eps, float* stats, void* q, uint32_t* scales,
                      void* stream) {
  if (!x || !gamma || !beta || !q || !scales || rows < 0 || D <= 0 || D % 8 || D > Kpad ||
      Kpad % 128 || Kpad > 1024 || !(eps > 0.f))
    return fail(EVT_EINVAL, "mx8_layernorm: bad shape (D % 8, D <= Kpad <= 1024, Kpad % 128)");
  if ((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)q) & 15) ||
      (((uintptr_t)scales | (uintptr_t)stats) & 7))
    return fail(EVT_EINVAL, "mx8_layernorm: misaligned pointer");
  EVT_HIP(ln_mx8_launch(x, rows, D, Kpad, gamma, beta, eps, stats, q, scales,
                        (hipStream_t)stream),
          "mx8_layernorm");
  return EVT_OK;
}

int evt_attention_mx8(const void* qkv, int64_t ldq, void* q8, int64_t ldq8, uint32_t* s8,
                      int64_t ld_s8, int B, int N, int H, float scale, void* stream) {
  if (!qkv || !q8 || !s8 || B < 0 || N <= 0 || N > 256 || H <= 0 || ldq < 3 * H * 64 ||
      ldq % 8 || ldq8 < H * 64 || ldq8 % 128 || ld_s8 < (int64_t)B * N || ld_s8 > INT32_MAX)
    return fail(EVT_EINVAL, "attention_mx8: bad shape (N <= 256, head size 64, ldq8 % 128)");
  AttnParams p{qkv, ldq, nullptr, 0, N, H, B, scale * 1.4426950408889634f};
  p.q8 = (uint8_t*)q8;
  p.s8 = s8;
  p.ldq8 = ldq8;
  p.rows8 = (int)ld_s8;
  EVT_HIP(attention_launch(DT_BF16, p, (hipStream_t)stream), "attention_mx8");
  return EVT_OK;
}

int evt_ln_fold(int dtype, const void* Wp, int Kpad, int Npad, const float* W, const float* beta,
                const float* bias, int K, int N, float* colsum, float* cvec, void* stream) {
  if (!Wp || !W || !beta || !colsum || !cvec || K <= 0 || N <= 0 || Kpad < K || Npad < N)
    return fail(EVT_EINVAL, "ln_fold: bad shape");
  EVT_HIP(ln_fold(dtype, Wp, Kpad, W, beta, bias, K, N, colsum, cvec, Npad, (hipStream_t)stream),
          "ln_fold");
  return EVT_OK;
}

int evt_dense(int dtype, const evt_dense_args* a, void* stream) {
  if (!a || !a->A || !a->Wp || !a->C || a->M < 0 || a->N <= 0 || a->N > a->Npad ||
      a->Kpad % PAD_K || a->Npad % GEMM_BN || a->lda < a->Kpad || a->ldc < a->N)
    return fail(EVT_EINVAL, "dense: bad shape");
  const int f = a->flags;
  if ((f & EPI_BIAS) && !a->bias) return fail(EVT_EINVAL, "dense: bias flag without bias");
  if ((f & EPI_RESID) && (!a->resid || a->ldr < a->N)) return fail(EVT_EINVAL, "dense: bad resid");
  if ((f & EPI_POS) && (!a->pos || a->P <= 0 || a->ldp < a->N || (a->resid && a->ldr < a->N)))
    return fail(EVT_EINVAL, "dense: bad pos");
  if ((f & EPI_LNIN) && (!a->colsum || !a->stats_in || a->ln_width <= 0))
    return fail(EVT_EINVAL, "dense: LN-in needs colsum, stats_in, ln_width");
  if ((f & EPI_RESLN) && (!a->rstats || !a->rgamma || !a->rbeta || a->ln_width <= 0))
    return fail(EVT_EINVAL, "dense: LN residual needs rstats, rgamma, rbeta, ln_width");
  if ((f & EPI_STATS) && !a->stats_out)
    return fail(EVT_EINVAL, "dense: stats flag without stats_out");
  GemmParams p = gemm_operands(a->A, a->lda, a->Wp, a->Kpad, a->Npad, a->C, a->ldc, a->M, a->N,
                               a->bias, a->resid, a->ldr, a->pos, a->ldp, a->P);
  p.colsum = a->colsum; p.stats_in = a->stats_in; p.rstats = a->rstats;
  p.rgamma = a->rgamma; p.rbeta = a->rbeta; p.stats_out = a->stats_out;
  p.inv_d = a->ln_width > 0 ? 1.0f / (float)a->ln_width : 0.f;
  p.eps = a->ln_eps;
  p.nslots = a->ln_width > 0 ? stats_slots(a->ln_width) : 1;
  p.stats_step = a->stats_step;
  if (dtype == EVT_DTYPE_BF16) {  // op-level calls share one stream-K scratch (one stream at a time)
    static void* sk = nullptr;
    if (!sk) {
      EVT_HIP(hipMalloc(&sk, gemm_sk_bytes()), "hipMalloc stream-K scratch");
      EVT_HIP(hipMemset(sk, 0, 4096), "memset stream-K flags");
    }
    gemm_sk_bind(sk, p);
  }
  hipError_t e = gemm_launch(dtype, f, p, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(EVT_EINVAL, "dense: unsupported flags/shape");
  EVT_HIP(e, "dense");
  return EVT_OK;
}

int evt_dense_splitk(int dtype, const evt_dense_args* a, int splits, float* partials,
                     void* stream) {
  if (!a || !a->A || !a->Wp || !a->C || !partials || a->M < 0 || a->N <= 0 || a->N > a->Npad ||
      a->Kpad % PAD_K || a->Npad % GEMM_BN || a->lda < a->Kpad || a->ldc < a->N)
    return fail(EVT_EINVAL, "dense_splitk: bad shape");
  if (a->flags & ~(EPI_BIAS | EPI_GELU | EPI_OUT_F32))
    return fail(EVT_EINVAL, "dense_splitk: flags must be a subset of BIAS | GELU | OUT_F32");
  if ((a->flags & EPI_BIAS) && !a->bias) return fail(EVT_EINVAL, "dense_splitk: bias flag without bias");
  if (splits < 1 || splits > 64 || a->Kpad % (splits * PAD_K))
    return fail(EVT_EINVAL, "dense_splitk: Kpad must be a multiple of splits * 64");
  const GemmParams p = gemm_operands(a->A, a->lda, a->Wp, a->Kpad, a->Npad, a->C, a->ldc, a->M,
                                     a->N, a->bias, nullptr, 0, nullptr, 0, 0);
  hipError_t e = gemm_splitk_launch(dtype, a->flags, p, splits, partials, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(EVT_EINVAL, "dense_splitk: unsupported flags/shape");
  EVT_HIP(e, "dense_splitk");
  return EVT_OK;
}

int evt_attention_hd(int dtype, const void* qkv, int64_t ldq, void* out, int64_t ldo, int B,
                     int N, int H, int head_dim, float scale, void* stream) {
  if (!qkv || !out || B < 0 || N <= 0 || N > EVT_ATTN_MAX_TOKENS || H <= 0 || head_dim <= 0 ||
      head_dim > 128 || ldq < 3 * (int64_t)H * head_dim || ldo < (int64_t)H * head_dim)
    return fail(EVT_EINVAL, "attention: bad shape (N <= 4096, head size in [1, 128])");
  if (N > 256 && !(scale > 0.f && scale < INFINITY))
    return fail(EVT_EINVAL, "attention: more than 256 tokens need a positive finite scale");
  // vector accesses: 16-B loads of q / k / v rows when h_k is a multiple of 16 B, 4-element stores
  // of O when h_k % 4 == 0 (head size 64: the tuned kernels' 16-B loads and stores)
  const int64_t vec = dtype == DT_BF16 ? 8 : 4;
  const bool vload = head_dim % vec == 0, vstore = head_dim % 4 == 0;
  if (vload && (ldq % vec || ((uintptr_t)qkv & 15)))
    return fail(EVT_EINVAL, "attention: qkv rows must be 16-B aligned for this head size");
  if ((vstore || head_dim == 64) && (ldo % (head_dim == 64 ? vec : 4) || ((uintptr_t)out & 15)))
    return fail(EVT_EINVAL, "attention: out rows must be 16-B aligned for this head size");
  AttnParams p{qkv, ldq, out, ldo, N, H, B, scale * 1.4426950408889634f};
  p.hd = head_dim;
  EVT_HIP(attention_launch(dtype, p, (hipStream_t)stream), "attention");
  return EVT_OK;
}

int evt_attention(int dtype, const void* qkv, int64_t ldq, void* out, int64_t ldo, int B, int N,
                  int H, float scale, void* stream) {
  // 16-B Q / O accesses: row pitches of 16 bytes multiple, 16-B aligned bases
  const int64_t vec = dtype == DT_BF16 ? 8 : 4;
  if (!qkv || !out || B < 0 || N <= 0 || N > EVT_ATTN_MAX_TOKENS || H <= 0 || ldq < 3 * H * 64 ||
      ldo < H * 64 || ldq % vec || ldo % vec || (((uintptr_t)qkv | (uintptr_t)out) & 15))
    return fail(EVT_EINVAL, "attention: bad shape (N <= 4096, head size 64, 16-B aligned rows)");
  if (N > 256 && !(scale > 0.f && scale < INFINITY))
    return fail(EVT_EINVAL, "attention: more than 256 tokens need a positive finite scale");
  AttnParams p{qkv, ldq, out, ldo, N, H, B, scale * 1.4426950408889634f};
  EVT_HIP(attention_launch(dtype, p, (hipStream_t)stream), "attention");
  return EVT_OK;
}

int evt_layernorm(int dtype, const float* x, int64_t ldx, void* y, int64_t ldy,
                  const float* gamma, const float* beta, int rows, int D, float eps,
                  void* stream) {
  if (!x || !y || !gamma || !beta || rows < 0 || D <= 0 || D > 1024 || D % 4 || ldx < D || ldy < D)
    return fail(EVT_EINVAL, "layernorm: bad shape (D % 4 == 0, D <= 1024)");
  EVT_HIP(layernorm_launch(dtype, x, ldx, y, ldy, gamma, beta, rows, D, eps, (hipStream_t)stream),
          "layernorm");
  return EVT_OK;
}

int evt_patchify(int dtype, const float* img, int B, int C, int HW, int ps, void* out, void* x,
                 const float* cls, const float* pos, int D, float* stats, void* stream) {
  if (!img || !out || !x || !cls || !pos || B < 0 || C <= 0 || ps <= 0 || HW % ps)
    return fail(EVT_EINVAL, "patchify: bad shape");
  EVT_HIP(patchify_launch(dtype, img, B, C, HW, ps, out, x, cls, pos, D, stats,
                          (hipStream_t)stream),
          "patchify");
  return EVT_OK;
}

int evt_patchify_cm(int dtype, const float* img, int B, int C, int HW, int ps, void* out, void* x,
                    const float* cls, const float* pos, int D, float* stats, void* stream) {
  if (!img || !out || !x || !cls || !pos || B < 0 || C <= 0 || ps <= 0 || HW % ps || ps % 8)
    return fail(EVT_EINVAL, "patchify_cm: bad shape (ps % 8 == 0)");
  EVT_HIP(patchify_launch(dtype, img, B, C, HW, ps, out, x, cls, pos, D, stats,
                          (hipStream_t)stream, true),
          "patchify_cm");
  return EVT_OK;
}

int evt_patchify_ld(int dtype, const float* img, int B, int C, int HW, int ps, void* out,
                    int64_t ldo, void* x, const float* cls, const float* pos, int D, float* stats,
                    void* stream) {
  if (dtype != EVT_DTYPE_F32 && dtype != EVT_DTYPE_BF16)
    return fail(EVT_EINVAL, "patchify_ld: dtype must be EVT_DTYPE_F32 or EVT_DTYPE_BF16");
  if (B < 0 || D <= 0 || !patchify_ld_ok(C, HW, ps, ldo))
    return fail(EVT_EINVAL, "patchify_ld: bad shape (HW % ps == 0, ps*HW % 4 == 0, ldo >= ps*ps*C, "
                            "ldo % 8 == 0, C*ps*HW*4 <= 160 KiB)");
  if (!img || !out || !x || !cls || !pos || ((uintptr_t)out & 15))
    return fail(EVT_EINVAL, "patchify_ld: img, out, x, cls, pos must be non-null, out 16-B aligned");
  EVT_HIP(patchify_ld_launch(dtype, img, B, C, HW, ps, out, ldo, x, cls, pos, D, stats,
                             (hipStream_t)stream),
          "patchify_ld");
  return EVT_OK;
}

int evt_unfold(int dtype, int in_f32, const void* in, int B, int H, int W, int C, int k,
               int stride, int pad, void* out, int ldo, float* stats, int nslots, void* stream) {
  if (!in || !out || B < 0 || H <= 0 || W <= 0 || C <= 0 || k <= 0 || stride <= 0 || pad < 0 ||
      H + 2 * pad < k || W + 2 * pad < k || ldo < k * k * C || (stats && nslots <= 0) ||
      ldo > ((C % 4 == 0 && ldo % 4 == 0) ? 1024 : (ldo % 2 == 0 ? 512 : 256)))
    return fail(EVT_EINVAL, "unfold: bad shape (ldo <= 256; <= 512 if even; <= 1024 if C % 4 == 0)");
  if (dtype == EVT_DTYPE_F32 && !in_f32) return fail(EVT_EINVAL, "unfold: f32 path needs f32 input");
  EVT_HIP(unfold_launch(dtype, in_f32, in, B, H, W, C, k, stride, pad, out, ldo, stats, nslots,
                        (hipStream_t)stream),
          "unfold");
  return EVT_OK;
}

int64_t evt_performer_scratch(int B, int T) {
  if (B <= 0 || T <= 0) return 0;
  return (int64_t)performer_part_floats(B, T);
}

int evt_performer(int dtype, const void* kqv, int64_t ldq, int B, int T, const float* w,
                  const float* out_w, const float* out_b, const float* ln2_g, const float* ln2_b,
                  const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b,
                  float* part, void* out, int64_t ldo, void* stream) {
  if (!kqv || !w || !out_w || !out_b || !ln2_g || !ln2_b || !fc1_w || !fc1_b || !fc2_w ||
      !fc2_b || !part || !out || B < 0 || T <= 0 || ldq < 192 || ldo < 64 || ldq % 4 || ldo % 4)
    return fail(EVT_EINVAL, "performer: bad arguments (ldq >= 192, ldo >= 64, multiples of 4)");
  PerformerWeights pw{w, out_w, out_b, ln2_g, ln2_b, fc1_w, fc1_b, fc2_w, fc2_b};
  EVT_HIP(performer_launch(dtype, kqv, ldq, B, T, pw, part, out, ldo, (hipStream_t)stream),
          "performer");
  return EVT_OK;
}

// include/evt_performer.h: evt_performer's checks, then the launcher with the model's two extras
int evt_performer_ex(int dtype, const void* kqv, int64_t ldq, int B, int T, const float* w,
                     const float* out_w, const float* out_b, const float* ln2_g,
                     const float* ln2_b, const float* fc1_w, const float* fc1_b,
                     const float* fc2_w, const float* fc2_b, float* part, void* out, int64_t ldo,
                     int kqv_perm, float* tstats, void* stream) {
  if (!kqv || !w || !out_w || !out_b || !ln2_g || !ln2_b || !fc1_w || !fc1_b || !fc2_w ||
      !fc2_b || !part || !out || B < 0 || T <= 0 || ldq < 192 || ldo < 64 || ldq % 4 || ldo % 4)
    return fail(EVT_EINVAL, "performer_ex: bad arguments (ldq >= 192, ldo >= 64, multiples of 4)");
  if ((kqv_perm || tstats) && dtype != EVT_DTYPE_BF16)
    return fail(EVT_EINVAL, "performer_ex: kqv_perm and tstats are bf16 only");
  if (kqv_perm && (ldq % 8 || ((uintptr_t)kqv & 15)))
    return fail(EVT_EINVAL, "performer_ex: kqv_perm needs ldq % 8 == 0 and a 16-B aligned kqv");
  PerformerWeights pw{w, out_w, out_b, ln2_g, ln2_b, fc1_w, fc1_b, fc2_w, fc2_b};
  EVT_HIP(performer_launch(dtype, kqv, ldq, B, T, pw, part, out, ldo, (hipStream_t)stream, tstats,
                           kqv_perm != 0),
          "performer_ex");
  return EVT_OK;
}

int evt_unfold_stats(const float* tstats, int B, int R, float* dst, int nslots, void* stream) {
  if (!tstats || !dst || B < 0 || R <= 0 || nslots <= 0)
    return fail(EVT_EINVAL, "unfold_stats: bad arguments (tstats, dst non-null, R > 0, nslots > 0)");
  EVT_HIP(unfold_stats_launch(tstats, B, R, dst, nslots, (hipStream_t)stream), "unfold_stats");
  return EVT_OK;
}

int evt_window_attention(int dtype, const void* qkv, int64_t ldq, void* out, int64_t ldo,
                         const float* rpb, int B, int R, int C, int H, int shift, void* stream) {
  if (!qkv || !out || !rpb) return fail(EVT_EINVAL, "null pointer");
  if (dtype != EVT_DTYPE_F32 && dtype != EVT_DTYPE_BF16) return fail(EVT_EINVAL, "bad dtype");
  if (B < 0 || R <= 0 || R % 7 || H <= 0 || C != 32 * H || ldo < C || ldq < 3 * C || shift < 0 ||
      shift >= 7 || ldq % 8 || ldo % 4)
    return fail(EVT_EINVAL, "bad window-attention shape (R % 7 == 0, head size 32, 0 <= shift < 7)");
  hipStream_t s = (hipStream_t)stream;
  float* dense_bias = nullptr;
  EVT_HIP(hipMallocAsync((void**)&dense_bias, rpb_table_floats(H, 7, shift) * sizeof(float), s),
          "malloc bias");
  EVT_HIP(rpb_dense_launch(rpb, H, 7, shift, dense_bias, s), "relative position bias");
  SwinAttnParams ap{qkv, ldq, out, ldo, dense_bias, B, R, R / 7, C, H, shift,
                    0.17677669529663687f * 1.4426950408889634f};
  const hipError_t e = window_attn_launch(dtype, 7, ap, s);
  (void)hipFreeAsync(dense_bias, s);
  EVT_HIP(e, "window attention");
  return EVT_OK;
}

int evt_patch_merge(int dtype, const void* x, int64_t ldx, int B, int R, int C, void* out,
                    float* stats, int nslots, void* stream) {
  if (!x || !out || !stats) return fail(EVT_EINVAL, "null pointer");
  if (dtype != EVT_DTYPE_F32 && dtype != EVT_DTYPE_BF16) return fail(EVT_EINVAL, "bad dtype");
  if (B < 0 || R <= 0 || R % 2 || C <= 0 || ldx < C || nslots <= 0 || nslots > 64)
    return fail(EVT_EINVAL, "bad patch-merge shape");
  EVT_HIP(merge_launch(dtype, x, ldx, B, R, C, out, stats, nslots, (hipStream_t)stream), "merge");
  return EVT_OK;
}

int evt_attention_probs(int dtype, const void* qkv, int64_t ldq, int64_t sb, int64_t sh, int ko,
                        int B, int N, int H, int head_dim, float scale, int nq, float* out,
                        void* stream) {
  if (dtype != EVT_DTYPE_F32 && dtype != EVT_DTYPE_BF16)
    return fail(EVT_EINVAL, "attention_probs: dtype must be EVT_DTYPE_F32 or EVT_DTYPE_BF16");
  if (!qkv || !out || B < 0 || N <= 0 || N > EVT_ATTN_MAX_TOKENS || H <= 0 || head_dim <= 0 ||
      head_dim > 128)
    return fail(EVT_EINVAL, "attention_probs: bad shape (N <= 4096, head size in [1, 128])");
  if (nq != 1 && nq != N) return fail(EVT_EINVAL, "attention_probs: nq must be 1 or N");
  if (!(scale > 0.f && scale < INFINITY))
    return fail(EVT_EINVAL, "attention_probs: the scale must be positive and finite");
  if ((uintptr_t)out & 15) return fail(EVT_EINVAL, "attention_probs: out must be 16-byte aligned");
  const int64_t vec = dtype == DT_BF16 ? 8 : 4;
  if (sb || sh || ko) {
    if (dtype != DT_BF16 || head_dim != 64 || sb < 0 || sh < 0 || ko < 0 || sb % 8 || sh % 8 ||
        ko % 8 || ldq % 8 || ldq < 64 || ((uintptr_t)qkv & 15))
      return fail(EVT_EINVAL, "attention_probs: a slice layout needs bf16, head size 64 and "
                              "non-negative strides that are multiples of 8");
  } else {
    if (ldq < 3 * (int64_t)H * head_dim)
      return fail(EVT_EINVAL, "attention_probs: ldq must be at least 3*H*head_dim");
    if (head_dim % vec == 0 && (ldq % vec || ((uintptr_t)qkv & 15)))
      return fail(EVT_EINVAL, "attention_probs: qkv rows must be 16-B aligned for this head size");
  }
  AttnParams p{qkv, ldq, nullptr, 0, N, H, B, scale * 1.4426950408889634f};
  p.hd = head_dim;
  p.sb = sb; p.sh = sh; p.ko = ko;
  EVT_HIP(attn_probs_launch(dtype, p, nq, out, (hipStream_t)stream), "attention_probs");
  return EVT_OK;
}

// include/evt_head_stats.h: evt_attention_probs' checks of (qkv, layout, shape, scale, out), then
// the patch geometry
int evt_attention_head_stats(int dtype, const void* qkv, int64_t ldq, int64_t sb, int64_t sh,
                             int ko, int B, int N, int H, int head_dim, float scale, int prefix,
                             int grid_w, float* out, void* stream) {
  if (dtype != EVT_DTYPE_F32 && dtype != EVT_DTYPE_BF16)
    return fail(EVT_EINVAL, "attention_head_stats: dtype must be EVT_DTYPE_F32 or EVT_DTYPE_BF16");
  if (!qkv || !out || B < 0 || N <= 0 || N > EVT_ATTN_MAX_TOKENS || H <= 0 || head_dim <= 0 ||
      head_dim > 128)
    return fail(EVT_EINVAL, "attention_head_stats: bad shape (N <= 4096, head size in [1, 128])");
  if (!(scale > 0.f && scale < INFINITY))
    return fail(EVT_EINVAL, "attention_head_stats: the scale must be positive and finite");
  if (prefix < 0 || prefix >= N || grid_w < 1 || (N - prefix) % grid_w)
    return fail(EVT_EINVAL, "attention_head_stats: needs 0 <= prefix < N, grid_w >= 1 and "
                            "(N - prefix) % grid_w == 0");
  if ((uintptr_t)out & 15)
    return fail(EVT_EINVAL, "attention_head_stats: out must be 16-byte aligned");
  const int64_t vec = dtype == DT_BF16 ? 8 : 4;
  if (sb || sh || ko) {
    if (dtype != DT_BF16 || head_dim != 64 || sb < 0 || sh < 0 || ko < 0 || sb % 8 || sh % 8 ||
        ko % 8 || ldq % 8 || ldq < 64 || ((uintptr_t)qkv & 15))
      return fail(EVT_EINVAL, "attention_head_stats: a slice layout needs bf16, head size 64 and "
                              "non-negative strides that are multiples of 8");
  } else {
    if (ldq < 3 * (int64_t)H * head_dim)
      return fail(EVT_EINVAL, "attention_head_stats: ldq must be at least 3*H*head_dim");
    if (head_dim % vec == 0 && (ldq % vec || ((uintptr_t)qkv & 15)))
      return fail(EVT_EINVAL,
                  "attention_head_stats: qkv rows must be 16-B aligned for this head size");
  }
  AttnParams p{qkv, ldq, nullptr, 0, N, H, B, scale * 1.4426950408889634f};
  p.hd = head_dim;
  p.sb = sb; p.sh = sh; p.ko = ko;
  EVT_HIP(head_stats_launch(dtype, p, prefix, grid_w, out, (hipStream_t)stream),
          "attention_head_stats");
  return EVT_OK;
}

// include/evt_ffn_stats.h
int evt_ffn_neuron_stats(int dtype, const void* h, int64_t ld, int B, int T, int F, float* out,
                         void* stream) {
  if (dtype != EVT_DTYPE_F32 && dtype != EVT_DTYPE_BF16)
    return fail(EVT_EINVAL, "ffn_neuron_stats: dtype must be EVT_DTYPE_F32 or EVT_DTYPE_BF16");
  if (!h || !out || B < 1 || T < 1 || T > EVT_FFN_STATS_MAX_TOKENS || F < 1)
    return fail(EVT_EINVAL, "ffn_neuron_stats: bad shape (B >= 1, 1 <= T <= 4096, F >= 1)");
  static_assert(EVT_FFN_STATS_MAX_TOKENS == FFN_STATS_MAX_TOKENS, "header and kernel agree");
  const int64_t vec = dtype == DT_BF16 ? 8 : 4;
  if (ld < F || ld % vec)
    return fail(EVT_EINVAL, "ffn_neuron_stats: ld must be at least F and the row pitch a multiple "
                            "of 16 bytes");
  if (((uintptr_t)h | (uintptr_t)out) & 15)
    return fail(EVT_EINVAL, "ffn_neuron_stats: h and out must be 16-byte aligned");
  EVT_HIP(ffn_stats_launch(dtype, h, ld, B, T, F, out, (hipStream_t)stream), "ffn_neuron_stats");
  return EVT_OK;
}

// include/evt_gram.h
int evt_gram_scratch_bytes(int64_t rows, int width, size_t* bytes) {
  static_assert(EVT_GRAM_MAX_WIDTH == GRAM_MAX_WIDTH, "header and kernel agree");
  if (!bytes) return fail(EVT_EINVAL, "gram scratch: bytes is NULL");
  if (rows < 1 || rows > INT32_MAX)
    return fail(EVT_EINVAL, "gram scratch: rows must be in [1, 2^31 - 1]");
  if (width < 1 || width > EVT_GRAM_MAX_WIDTH)
    return fail(EVT_EINVAL, "gram scratch: width must be in [1, " +
                                std::to_string(EVT_GRAM_MAX_WIDTH) + "]");
  *bytes = gram_plan((int)rows, width).scratch_bytes;
  return EVT_OK;
}

int evt_gram(int dtype, const void* a, int64_t ld, int64_t rows, int width, float* gram,
             float* sums, void* scratch, size_t scratch_bytes, void* stream) {
  if (dtype != EVT_DTYPE_F32 && dtype != EVT_DTYPE_BF16)
    return fail(EVT_EINVAL, "gram: dtype must be EVT_DTYPE_F32 or EVT_DTYPE_BF16");
  if (!a || !gram || !sums) return fail(EVT_EINVAL, "gram: a, gram and sums must be non-null");
  const int vec = dtype == DT_BF16 ? 8 : 4;
  if (width < vec || width % vec || width > EVT_GRAM_MAX_WIDTH)
    return fail(EVT_EINVAL, "gram: width must be a multiple of " + std::to_string(vec) +
                                " in [" + std::to_string(vec) + ", " +
                                std::to_string(EVT_GRAM_MAX_WIDTH) + "]");
  if (ld < width || ld % vec)
    return fail(EVT_EINVAL, "gram: ld must be at least width and the row pitch a multiple of 16 "
                            "bytes");
  if (rows < 1 || rows > INT32_MAX) return fail(EVT_EINVAL, "gram: rows must be in [1, 2^31 - 1]");
  if (((uintptr_t)a | (uintptr_t)gram | (uintptr_t)sums | (uintptr_t)scratch) & 15)
    return fail(EVT_EINVAL, "gram: a, gram, sums and scratch must be 16-byte aligned");
  const size_t need = gram_plan((int)rows, width).scratch_bytes;
  if (need && (!scratch || scratch_bytes < need))
    return fail(EVT_EINVAL, "gram: scratch_bytes is " + std::to_string(scratch ? scratch_bytes : 0) +
                                ", this call needs " + std::to_string(need) +
                                " (evt_gram_scratch_bytes)");
  EVT_HIP(gram_launch(dtype, a, ld, (int)rows, width, gram, sums, scratch, scratch_bytes,
                      (hipStream_t)stream),
          "gram");
  return EVT_OK;
}

// include/evt_depth.h: the stream-delta kernel on caller buffers; the per-chunk partials of an
// image of more than 16 tokens come from, and go back to, the stream's memory pool
int evt_stream_delta_stats(int dtype, const void* a, int64_t lda, const void* b, int64_t ldb,
                           int B, int T, int D, float* out, void* stream) {
  if (dtype != EVT_DTYPE_F32 && dtype != EVT_DTYPE_BF16)
    return fail(EVT_EINVAL, "stream_delta_stats: dtype must be EVT_DTYPE_F32 or EVT_DTYPE_BF16");
  static_assert(EVT_DEPTH_MAX_TOKENS == STREAM_DELTA_MAX_TOKENS, "header and kernel agree");
  if (B < 1) return fail(EVT_EINVAL, "stream_delta_stats: B must be at least 1");
  if (T < 1 || T > EVT_DEPTH_MAX_TOKENS)
    return fail(EVT_EINVAL, "stream_delta_stats: T must be in [1, 4096]");
  if (D < 8 || D % 8)
    return fail(EVT_EINVAL, "stream_delta_stats: D must be a positive multiple of 8");
  const int64_t vec = dtype == DT_BF16 ? 8 : 4;
  if (lda < D || ldb < D || lda % vec || ldb % vec)
    return fail(EVT_EINVAL, "stream_delta_stats: lda and ldb must be at least D and the row "
                            "pitches a multiple of 16 bytes");
  if (!a || !b || !out) return fail(EVT_EINVAL, "stream_delta_stats: a, b and out must be non-null");
  if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15)
    return fail(EVT_EINVAL, "stream_delta_stats: a, b and out must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  float* part = nullptr;
  const size_t bytes = stream_delta_part_bytes(B, T);
  if (bytes) EVT_HIP(hipMallocAsync((void**)&part, bytes, s), "malloc partials");
  const hipError_t e = stream_delta_launch(dtype, a, lda, b, ldb, B, T, D, out, 4, part, s);
  if (part) (void)hipFreeAsync(part, s);
  EVT_HIP(e, "stream_delta_stats");
  return EVT_OK;
}

// include/evt_rollout.h: evt_attention_probs' checks of (qkv, layout, shape, scale), then the
// rollout buffers and the scratch; two launches (the head mean into the scratch, then the step)
int evt_attention_rollout_step(int dtype, const void* qkv, int64_t ldq, int64_t sb, int64_t sh,
                               int ko, int B, int N, int H, int head_dim, float scale,
                               const float* r_in, float* r_out, void* scratch, size_t scratch_bytes,
                               void* stream) {
  if (dtype != EVT_DTYPE_F32 && dtype != EVT_DTYPE_BF16)
    return fail(EVT_EINVAL, "attention_rollout_step: dtype must be EVT_DTYPE_F32 or EVT_DTYPE_BF16");
  if (!qkv || !r_out || !scratch || B < 0 || N <= 0 || N > EVT_ATTN_MAX_TOKENS || H <= 0 ||
      H > 254 || head_dim <= 0 || head_dim > 128)
    return fail(EVT_EINVAL, "attention_rollout_step: bad shape (N <= 4096, H <= 254, head size in "
                            "[1, 128]) or a NULL qkv, r_out or scratch");
  if (!(scale > 0.f && scale < INFINITY))
    return fail(EVT_EINVAL, "attention_rollout_step: the scale must be positive and finite");
  if (((uintptr_t)r_in | (uintptr_t)r_out | (uintptr_t)scratch) & 15)
    return fail(EVT_EINVAL, "attention_rollout_step: r_in, r_out and scratch must be 16-byte aligned");
  const size_t bytes = (size_t)B * N * N * sizeof(float);
  if (scratch_bytes < bytes)
    return fail(EVT_EINVAL, "attention_rollout_step: scratch_bytes must be at least B*N*N*4");
  const uintptr_t ri = (uintptr_t)r_in, ro = (uintptr_t)r_out;
  if (r_in && (ri == ro || (ri < ro + bytes && ro < ri + bytes)))
    return fail(EVT_EINVAL, "attention_rollout_step: r_in must not overlap r_out (a step cannot run "
                            "in place)");
  const int64_t vec = dtype == DT_BF16 ? 8 : 4;
  if (sb || sh || ko) {
    if (dtype != DT_BF16 || head_dim != 64 || sb < 0 || sh < 0 || ko < 0 || sb % 8 || sh % 8 ||
        ko % 8 || ldq % 8 || ldq < 64 || ((uintptr_t)qkv & 15))
      return fail(EVT_EINVAL, "attention_rollout_step: a slice layout needs bf16, head size 64 and "
                              "non-negative strides that are multiples of 8");
  } else {
    if (ldq < 3 * (int64_t)H * head_dim)
      return fail(EVT_EINVAL, "attention_rollout_step: ldq must be at least 3*H*head_dim");
    if (head_dim % vec == 0 && (ldq % vec || ((uintptr_t)qkv & 15)))
      return fail(EVT_EINVAL,
                  "attention_rollout_step: qkv rows must be 16-B aligned for this head size");
  }
  AttnParams p{qkv, ldq, nullptr, 0, N, H, B, scale * 1.4426950408889634f};
  p.hd = head_dim;
  p.sb = sb; p.sh = sh; p.ko = ko;
  EVT_HIP(head_mean_launch(dtype, p, (float*)scratch, (hipStream_t)stream),
          "attention_rollout_step (head mean)");
  EVT_HIP(rollout_step_launch((const float*)scratch, r_in, r_out, B, N, N, (hipStream_t)stream),
          "attention_rollout_step");
  return EVT_OK;
}

// include/evt_token_pruning.h: evt_attention_probs' checks of (qkv, layout, shape, scale)
int evt_token_scores(int dtype, const void* qkv, int64_t ldq, int64_t sb, int64_t sh, int ko,
                     int B, int N, int H, int head_dim, float scale, float* scores, void* stream) {
  if (dtype != EVT_DTYPE_F32 && dtype != EVT_DTYPE_BF16)
    return fail(EVT_EINVAL, "token_scores: dtype must be EVT_DTYPE_F32 or EVT_DTYPE_BF16");
  if (!qkv || !scores || B < 0 || N <= 0 || N > EVT_ATTN_MAX_TOKENS || H <= 0 || head_dim <= 0 ||
      head_dim > 128)
    return fail(EVT_EINVAL, "token_scores: bad shape (N <= 4096, head size in [1, 128])");
  if (!(scale > 0.f && scale < INFINITY))
    return fail(EVT_EINVAL, "token_scores: the scale must be positive and finite");
  if ((uintptr_t)scores & 3) return fail(EVT_EINVAL, "token_scores: scores must be 4-byte aligned");
  const int64_t vec = dtype == DT_BF16 ? 8 : 4;
  if (sb || sh || ko) {
    if (dtype != DT_BF16 || head_dim != 64 || sb < 0 || sh < 0 || ko < 0 || sb % 8 || sh % 8 ||
        ko % 8 || ldq % 8 || ldq < 64 || ((uintptr_t)qkv & 15))
      return fail(EVT_EINVAL, "token_scores: a slice layout needs bf16, head size 64 and "
                              "non-negative strides that are multiples of 8");
  } else {
    if (ldq < 3 * (int64_t)H * head_dim)
      return fail(EVT_EINVAL, "token_scores: ldq must be at least 3*H*head_dim");
    if (head_dim % vec == 0 && (ldq % vec || ((uintptr_t)qkv & 15)))
      return fail(EVT_EINVAL, "token_scores: qkv rows must be 16-B aligned for this head size");
  }
  AttnParams p{qkv, ldq, nullptr, 0, N, H, B, scale * 1.4426950408889634f};
  p.hd = head_dim;
  p.sb = sb; p.sh = sh; p.ko = ko;
  EVT_HIP(token_scores_launch(dtype, p, scores, (hipStream_t)stream), "token_scores");
  return EVT_OK;
}

int evt_token_select(const float* scores, int B, int N, int K, int32_t* kept, void* stream) {
  if (!scores || !kept || B < 0)
    return fail(EVT_EINVAL, "token_select: scores and kept must be non-null, B >= 0");
  if (N < 2 || N > EVT_ATTN_MAX_TOKENS || K < 1 || K > N - 1)
    return fail(EVT_EINVAL, "token_select: needs 2 <= N <= 4096 and 1 <= K <= N - 1");
  if (((uintptr_t)scores | (uintptr_t)kept) & 3)
    return fail(EVT_EINVAL, "token_select: scores and kept must be 4-byte aligned");
  EVT_HIP(token_select_launch(scores, B, N, K, kept, (hipStream_t)stream), "token_select");
  return EVT_OK;
}

int evt_token_gather(int dtype, const void* src, void* dst, const float* stats_src,
                     float* stats_dst, int slots, const int32_t* kept, int B, int T, int K1, int D,
                     void* stream) {
  if (dtype != EVT_DTYPE_F32 && dtype != EVT_DTYPE_BF16)
    return fail(EVT_EINVAL, "token_gather: dtype must be EVT_DTYPE_F32 or EVT_DTYPE_BF16");
  if (!src || !dst || !kept || B < 0 || T < 1 || K1 < 1 || K1 > T || D < 8 || D % 8)
    return fail(EVT_EINVAL, "token_gather: needs src, dst, kept, 1 <= K1 <= T and D a positive "
                            "multiple of 8");
  if ((!stats_src) != (!stats_dst) || (stats_src && (slots < 2 || slots % 2)))
    return fail(EVT_EINVAL, "token_gather: stats_src and stats_dst go together, slots even");
  if ((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)stats_src | (uintptr_t)stats_dst) & 15) ||
      ((uintptr_t)kept & 3))
    return fail(EVT_EINVAL, "token_gather: rows and statistics must be 16-byte aligned, kept "
                            "4-byte aligned");
  auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
  };
  const size_t es = dtype == DT_BF16 ? 2 : 4;
  if (overlap(src, (size_t)B * T * D * es, dst, (size_t)B * K1 * D * es) ||
      (stats_src && overlap(stats_src, (size_t)B * T * slots * 8, stats_dst,
                            (size_t)B * K1 * slots * 8)))
    return fail(EVT_EINVAL, "token_gather: dst must not overlap src (a gather cannot run in place)");
  EVT_HIP(token_gather_launch(dtype, src, dst, stats_src, stats_dst, slots, kept, B, T, K1, D,
                              (hipStream_t)stream),
          "token_gather");
  return EVT_OK;
}

// include/evt_gates.h: the gate kernel on caller buffers
int evt_gate_weights(int dtype, const void* w0, void* w, const float* gates, int npad, int kpad,
                     void* stream) {
  if (dtype != EVT_DTYPE_F32 && dtype != EVT_DTYPE_BF16)
    return fail(EVT_EINVAL, "gate_weights: dtype must be EVT_DTYPE_F32 or EVT_DTYPE_BF16");
  if (!w0 || !w || !gates) return fail(EVT_EINVAL, "gate_weights: w0, w and gates must be non-null");
  if (npad < 1 || kpad < PAD_K || kpad % PAD_K)
    return fail(EVT_EINVAL, "gate_weights: needs npad >= 1 and kpad a positive multiple of 64");
  if (((uintptr_t)w0 | (uintptr_t)w | (uintptr_t)gates) & 15)
    return fail(EVT_EINVAL, "gate_weights: w0, w and gates must be 16-byte aligned");
  auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
  };
  const size_t bytes = (size_t)npad * kpad * (dtype == DT_BF16 ? 2 : 4);
  if (overlap(w, bytes, w0, bytes) || overlap(w, bytes, gates, (size_t)kpad * sizeof(float)))
    return fail(EVT_EINVAL, "gate_weights: w must not overlap w0 or gates (the kernel always "
                            "reads the pristine copy)");
  EVT_HIP(gate_weights_launch(dtype, w0, w, gates, npad, kpad, (hipStream_t)stream),
          "gate_weights");
  return EVT_OK;
}

int evt_window_attention_probs(int dtype, const void* qkv, int64_t ldq, const float* rpb, int B,
                               int R, int window, int C, int H, int shift, float* out,
                               void* stream) {
  if (dtype != EVT_DTYPE_F32 && dtype != EVT_DTYPE_BF16)
    return fail(EVT_EINVAL, "window_attention_probs: dtype must be EVT_DTYPE_F32 or EVT_DTYPE_BF16");
  if (!qkv || !rpb || !out) return fail(EVT_EINVAL, "window_attention_probs: null pointer");
  if (window != 7 && window != 12)
    return fail(EVT_EINVAL, "window_attention_probs: window must be 7 or 12");
  if (B < 0 || R <= 0 || R % window || H <= 0 || C != 32 * H || shift < 0 || shift >= window ||
      (shift && R == window) || ldq < 3 * (int64_t)C)
    return fail(EVT_EINVAL, "window_attention_probs: bad shape (R % window == 0, C == 32*H, "
                            "0 <= shift < window, no shift with a single window, ldq >= 3*C)");
  if ((uintptr_t)out & 15)
    return fail(EVT_EINVAL, "window_attention_probs: out must be 16-byte aligned");
  if (dtype == EVT_DTYPE_BF16 && (ldq % 8 || ((uintptr_t)qkv & 15)))
    return fail(EVT_EINVAL, "window_attention_probs: bf16 qkv rows must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  float* tables = nullptr;
  EVT_HIP(hipMallocAsync((void**)&tables, rpb_table_floats(H, window, shift) * sizeof(float), s),
          "malloc bias");
  hipError_t e = rpb_dense_launch(rpb, H, window, shift, tables, s);
  if (e == hipSuccess) {
    SwinAttnParams ap{qkv, ldq, nullptr, 0, tables, B, R, R / window, C, H, shift,
                      0.17677669529663687f * 1.4426950408889634f};
    e = window_probs_launch(dtype, window, ap, out, s);
  }
  (void)hipFreeAsync(tables, s);
  EVT_HIP(e, "window_attention_probs");
  return EVT_OK;
}

int evt_classify(const float* logits, int64_t ldl, int B, int C, const evt_classify_args* a,
                 void* stream) {
  if (!logits) return fail(EVT_EINVAL, "classify: logits are NULL");
  if ((uintptr_t)logits & 3) return fail(EVT_EINVAL, "classify: logits must be 4-byte aligned");
  ClassifyParams p;
  EVT_RC(validate_classify(a, B, C, ldl, &p));
  EVT_HIP(classify_launch(logits, ldl, B, C, p, (hipStream_t)stream), "classify");
  return EVT_OK;
}

int evt_patchify_u8(int dtype, const uint8_t* img, int B, int C, int HW, int ps, void* out,
                    int64_t ldo, void* x, const float* cls, const float* pos, int D, float* stats,
                    const float* scale, const float* shift, void* stream) {
  if (dtype != EVT_DTYPE_F32 && dtype != EVT_DTYPE_BF16)
    return fail(EVT_EINVAL, "patchify_u8: dtype must be EVT_DTYPE_F32 or EVT_DTYPE_BF16");
  ImgAffine aff;
  EVT_RC(affine_from(scale, shift, C, &aff, "patchify_u8"));
  if (B < 0 || D <= 0 || !patchify_u8_ok(C, HW, ps, ldo))
    return fail(EVT_EINVAL, "patchify_u8: bad shape (C <= 4, HW % ps == 0, ps*HW % 4 == 0, "
                            "ps*HW*C % 4 == 0, ldo >= ps*ps*C, ldo % 8 == 0, C*ps*HW*4 <= 160 KiB)");
  if (!img || !out || !x || !cls || !pos || ((uintptr_t)out & 15) || ((uintptr_t)img & 3))
    return fail(EVT_EINVAL, "patchify_u8: img, out, x, cls, pos must be non-null, out 16-B and img "
                            "4-B aligned");
  EVT_HIP(patchify_u8_launch(dtype, img, B, C, HW, ps, out, ldo, x, cls, pos, D, stats, aff,
                             (hipStream_t)stream),
          "patchify_u8");
  return EVT_OK;
}

int evt_unfold_u8(int dtype, const uint8_t* in, int B, int H, int W, int C, int k, int stride,
                  int pad, void* out, int ldo, float* stats, int nslots, const float* scale,
                  const float* shift, void* stream) {
  if (dtype != EVT_DTYPE_F32 && dtype != EVT_DTYPE_BF16)
    return fail(EVT_EINVAL, "unfold_u8: dtype must be EVT_DTYPE_F32 or EVT_DTYPE_BF16");
  ImgAffine aff;
  EVT_RC(affine_from(scale, shift, C, &aff, "unfold_u8"));
  if (!in || !out || B < 0 || H <= 0 || W <= 0 || k <= 0 || stride <= 0 || pad < 0 ||
      H + 2 * pad < k || W + 2 * pad < k || ldo < k * k * C || (stats && nslots <= 0) ||
      ldo > ((C % 4 == 0 && ldo % 4 == 0) ? 1024 : (ldo % 2 == 0 ? 512 : 256)) ||
      (C == 4 && ((uintptr_t)in & 3)))
    return fail(EVT_EINVAL, "unfold_u8: bad shape (as evt_unfold; C <= 4, C == 4: in 4-B aligned)");
  EVT_HIP(unfold_u8_launch(dtype, in, B, H, W, C, k, stride, pad, out, ldo, stats, nslots, aff,
                           (hipStream_t)stream),
          "unfold_u8");
  return EVT_OK;
}

}  // extern "C"
