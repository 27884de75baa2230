// C ABI of libevt_hip.so (declared in include/evt.h): model plumbing around the HIP kernels.
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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/evt.h"
#include "evt_internal.h"

using namespace evt;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  return fail(EVT_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define EVT_HIP(call, what)                            \
  do {                                                 \
    hipError_t e__ = (call);                           \
    if (e__ != hipSuccess) return hip_fail(e__, what); \
  } while (0)

#define EVT_RC(x)          \
  do {                     \
    int rc__ = (x);        \
    if (rc__) return rc__; \
  } while (0)

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
inline size_t elem_size(int dtype) { return dtype == DT_BF16 ? 2 : 4; }

struct DenseW {  // packed Dense layer
  void* w = nullptr;        // [npad][kpad] activation dtype
  float* b = nullptr;       // [npad] fp32, zero padded (bias, or the LN-fold vector c)
  float* colsum = nullptr;  // [npad] LN fold: column sums of the packed weights (or null)
  int K = 0, N = 0, kpad = 0, npad = 0;
};

struct Mx8W {  // MXFP8-packed Dense layer (mx8.hip): Wq [npad][kpad] e4m3, scales [kpad/128][npad]
  void* w = nullptr;
  uint32_t* s = nullptr;
  float* b = nullptr;       // [npad] fp32 bias, zero padded (zeros for the bias-less QKV)
  int K = 0, N = 0, kpad = 0, npad = 0;
};

struct Layer {
  int heads = 0, hd = 64, inner = 0, ffn = 0, ffn_st = 0;
  float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
  DenseW qkv, out, fc1, fc2;
  Mx8W mqkv, mout, mfc1, mfc2;  // EVT_DTYPE_MX8 models
};

struct Shape {
  int P = 0, T = 0, pd = 0, D = 0, max_inner = 0, max_ffn_st = 0, head_st = 0;
  int pdst = 0;  // ViT: row stride of the patch matrix, pd rounded up to PAD_K (patch 14: 640)
};

}  // namespace

struct Performer {  // one TokenPerformer (transformer_encoder.py:39-101)
  int din = 0, dpad = 0;     // unfolded input width, padded to PAD_K
  DenseW kqv;                // LN1-folded Dense(3*64) + bias
  PerformerWeights w{};      // fp32 device copies (Keras layouts)
};

struct SwinBlock {  // one Swin block (microsoft SwinTransformerBlock)
  int shift = 0;
  float* bias = nullptr;     // [H][49][64] dense relative position bias (* log2 e)
  DenseW qkv, proj, fc1, fc2;
};

struct SwinStage {
  int C = 0, Cst = 0, H = 0, R = 0, mlp = 0, mst = 0;
  int w = 7;                 // window of the stage: min(window_size, R), 7 or 12
  DenseW merge;              // LN(4C)-folded reduction Linear(4C, 2C, bias=False) (stage > 0)
  std::vector<SwinBlock> blocks;
};

// EVT_QKV_LAYOUT=token (read when a model is created): keep the token-major qkv layout
static bool qkv_headmajor_default() {
  const char* e = std::getenv("EVT_QKV_LAYOUT");
  return !(e && std::strcmp(e, "token") == 0);
}

// What is fixed once evt_*_create returns: configuration, geometry and the packed weights. Lane
// children (evt_model_set_lanes) copy it, so they share the parent's weight allocations.
struct ModelCore {
  int family = 0;            // 0: ViT / ViT_Pruned, 1: T2T-ViT, 2: Swin
  bool standard = false;     // ViT with EVT_VIT_STANDARD semantics
  bool mx8 = false;          // EVT_DTYPE_MX8: MXFP8 encoder Dense layers (dtype is then bf16)
  // QKV output head-major where the GEMM supports it (run_encoder); EVT_QKV_LAYOUT=token at model
  // creation keeps the token-major layout (the A/B and bitwise-equality tests)
  bool headmajor = qkv_headmajor_default();
  bool patch_cm = false;     // ViT: channel-major patch vectors / patch weight rows
  bool patch_ld = false;     // ViT: pd % 64 != 0 (patch 14): channel-major rows at the padded
                             // stride sh.pdst with a zeroed tail (patchify_ld_kernel)
  float eps = 1e-5f;         // LayerNorm epsilon of every folded LayerNorm
  int dtype = 0, D = 0, num_classes = 0;
  size_t img_elems = 0;      // fp32 elements of one input image
  evt_vit_desc desc{};       // ViT only
  evt_t2t_desc tdesc{};      // T2T only
  evt_swin_desc sdesc{};     // Swin only
  std::vector<int32_t> heads, head_dim, ffn;
  Shape sh;
  DenseW patch, head1, head2;
  float *cls = nullptr, *pos = nullptr;
  void* pos_h = nullptr;     // bf16 copy of pos (the persistent patch-embedding GEMM's EPI_POS)
  std::vector<Layer> layers;
  // T2T stage
  Performer perf[2];
  DenseW project, head;      // head: LN-folded classifier (final LayerNorm, t2t_vit.py:129,134)
  int grid[3] = {0, 0, 0};   // token grids S/4, S/8, S/16
  // Swin (family 2)
  std::vector<SwinStage> stages;
  // norm_g / norm_b: the final LayerNorm; STANDARD ViT and T2T-ViT keep it too (their heads have
  // it folded into the weights) for the feature outputs; null for a REFERENCE ViT (it has none)
  float *pnorm_g = nullptr, *pnorm_b = nullptr, *norm_g = nullptr, *norm_b = nullptr;
  // desc's per-layer arrays live in this core's own vectors (after every copy of a core)
  void bind_desc() {
    desc.heads = heads.data();
    desc.head_dim = head_dim.data();
    desc.ffn = ffn.data();
  }
};

// The buffers a forward writes, filled in by the *_alloc_ws functions for one handle's max_batch
// and never shared: every lane child has its own. The allocations are owned by evt_model::allocs.
struct Workspace {
  // T2T stage
  void* u = nullptr;         // unfold output (GEMM A operand)
  float* su = nullptr;       // unfold row statistics
  void* kqvb = nullptr;      // [B*T1, 192]
  void* pout = nullptr;      // [B*T1, 64] performer output (NHWC for the next unfold)
  float* tstats = nullptr;   // [B*T1, 2] per-token (sum, sumsq) of pout (gathered soft split)
  void* zrow = nullptr;      // 256 zero bytes: the soft split's padding rows (gathered loader)
  float* part = nullptr;     // performer partial sums
  // token stream (activation dtype unless noted)
  void* apatch = nullptr;    // [B*P, pdst] patch matrix (aliases hbuf)
  void* x = nullptr;         // [B*T, D] token stream at layer input / output
  void* xm = nullptr;        // [B*T, D] token stream between the two sublayers
  float* sx = nullptr;       // [B*T, nslots, 2] fp32 per-slab (sum, sumsq) of x rows
  float* sm = nullptr;       // [B*T, nslots, 2] fp32 per-slab (sum, sumsq) of xm rows
  void* qkv = nullptr;       // [B*T, 3*inner]
  void* o = nullptr;         // [B*T, inner]
  void* hbuf = nullptr;      // [B*T, ffn_st]
  size_t hbuf_bytes = 0;
  void* hc = nullptr;        // [B, max ffn_st] FFN hidden rows of the CLS tail (run_encoder)
  void* hh = nullptr;        // [B, head_st]
  void* sk = nullptr;        // stream-K scratch of the model's GEMMs (gemm_sk_bytes)
  void* pooled = nullptr;    // Swin: [B, Cst_last] LayerNorm + token mean (head A operand)
  void* qa = nullptr;        // MX8: [rows][max(Dpad, innerpad)] e4m3 A operand (LN out / attn out)
  uint32_t* sa = nullptr;    // MX8: its scales [pad/128][rows]
  void* qh = nullptr;        // MX8: [rows][ffnpad] FC1 output (e4m3, zero-initialised)
  uint32_t* shd = nullptr;   // MX8: its scales
  float* lnst = nullptr;     // MX8: [rows][2] (mu, rstd) of the last LayerNorm'd rows
  int qa_ld = 0, qh_ld = 0;
};
static_assert(std::is_trivially_copyable<Workspace>::value, "raw pointers and integers only");

struct evt_model : ModelCore {  // a handle: the core, its own workspace, its own runtime state
  Workspace ws;
  int max_batch = 0;
  std::vector<void*> allocs;         // every device allocation this handle owns (weights, ws)
  int hm_layers = 0;         // encoder layers whose QKV stored head-major in the last forward
  int tail_mode = 0;         // last forward's last encoder block: bit 0 CLS tail, bit 1 full rows
  hipGraph_t graph = nullptr;        // evt_graph_capture
  hipGraphExec_t graph_exec = nullptr;
  // evt_model_profile: HIP events around every launch of the last forward, by role
  bool prof = false;
  std::vector<hipEvent_t> prof_ev;   // pool (pairs)
  std::vector<int> prof_role;        // role of pair i of the last forward
  // algorithmic work of pair i (evt_model_profile_work): GFLOP and GB its kernels must do / move
  mutable std::vector<double> prof_gflop, prof_gbytes;
  // evt_model_set_lanes: the batch split over k lanes, each a child model with its own workspace
  // (the weights are this model's) on its own HIP stream, forked from / joined to the caller's
  // stream by events; the kernels of the lanes then fill each other's idle CUs
  std::vector<evt_model*> lanes;
  std::vector<hipStream_t> lane_s;
  std::vector<char> lane_own;        // lane_s[i] created (and destroyed) by the library
  std::vector<hipEvent_t> lane_ev;   // [0]: fork, [1 + i]: lane i done
  bool is_lane = false;              // a child: weights and lanes belong to the parent
  // T2T-ViT lanes: their persistent GEMMs keep one block per CU at 2-4 tile rounds (the other
  // lane fills the CUs a balanced grid leaves idle; measured +2.9 % on T2T-ViT-14 bs256, while
  // Swin lanes measured -1.3 % without the balancing: DESIGN.md, batch lanes)
  int no_balance = 0;
};

namespace {

// The arguments of one forward. The entry points build one and the run functions read it; nothing
// of a call is kept on the handle (hm_layers and tail_mode, which evt_model_qkv_layout and
// evt_model_tail_mode read later, aside).
struct ForwardCall {
  const float* img = nullptr;     // the fp32 batch, or null with
  const uint8_t* img8 = nullptr;  // a uint8 NHWC batch (evt_forward_image) and
  ImgAffine aff{};                // its per-channel affine
  int B = 0;
  float* logits = nullptr;        // may be null in a features forward (no head then)
  const evt_features_args* feat = nullptr;  // evt_forward_features outputs (null: plain forward)
  int feat_next = 0;              // the next entry of feat's tap list
  const evt_attn_args* attn = nullptr;  // evt_forward_attention maps (null: none)
  int attn_next = 0;              // the next entry of attn's block list
  hipStream_t s = nullptr;
  // images [b0, b1) of a logits-only call, on stream `lane`: the input advances by whole images
  // (4 bytes per element of an fp32 batch, 1 of a uint8 one), the logits by rows
  ForwardCall slice(int b0, int b1, size_t img_elems, int num_classes, hipStream_t lane) const {
    ForwardCall c = *this;
    if (img) c.img += (size_t)b0 * img_elems;
    if (img8) c.img8 += (size_t)b0 * img_elems;
    c.B = b1 - b0;
    c.logits += (size_t)b0 * num_classes;
    c.s = lane;
    return c;
  }
};

// evt_model_profile: a pair of events around each launch of a forward (profiling forwards only)
struct ProfScope {
  evt_model* m;
  hipStream_t s;
  int pair = -1;
  ProfScope(evt_model* m_, int role, hipStream_t s_) : m(m_), s(s_) {
    if (!m->prof) return;
    pair = (int)m->prof_role.size();
    while ((int)m->prof_ev.size() < 2 * (pair + 1)) {
      hipEvent_t e = nullptr;
      if (hipEventCreate(&e) != hipSuccess) {
        pair = -1;
        return;
      }
      m->prof_ev.push_back(e);
    }
    m->prof_role.push_back(role);
    m->prof_gflop.push_back(0.0);
    m->prof_gbytes.push_back(0.0);
    (void)hipEventRecord(m->prof_ev[2 * pair], s);
  }
  ~ProfScope() {
    if (pair >= 0) (void)hipEventRecord(m->prof_ev[2 * pair + 1], s);
  }
};
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

// Pack a Keras [K, N] Dense kernel. With ln_g/ln_b (the LayerNorm in front of it), gamma is folded
// into the weight rows and b becomes c = beta . W + bias, with the column sums of the packed
// weights alongside (gemm.hip, "LayerNorm folding").
int make_dense(evt_model* m, DenseW* dw, const float* W, const float* bias, int K, int N,
               hipStream_t s, const float* ln_g = nullptr, const float* ln_b = nullptr) {
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
              const float* rstats = nullptr, const float* rgamma = nullptr,
              const float* rbeta = nullptr) {
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

size_t workspace_bytes(const evt_vit_desc* d, const Shape& sh, int B) {
  const bool mx8 = d->dtype == EVT_DTYPE_MX8;
  const size_t es = elem_size(mx8 ? DT_BF16 : d->dtype);
  const size_t rows = (size_t)B * sh.T;
  const size_t hb = std::max(rows * sh.max_ffn_st, (size_t)B * sh.P * sh.pdst) * es;
  size_t extra = 0;
  if (mx8) {  // qa + sa, qh + its scales, LayerNorm row statistics (run_encoder_mx8)
    const size_t qa = std::max(round_up(sh.D, 128), round_up(sh.max_inner, 128));
    int maxffn = 0;
    for (int i = 0; i < d->depth; ++i) maxffn = std::max(maxffn, (int)d->ffn[i]);
    const size_t qh = round_up(maxffn, 128);
    extra = rows * (qa + qa / 32 + qh + qh / 32 + 2 * sizeof(float)) + 5 * 256;
  }
  return 2 * rows * sh.D * es + 2 * rows * stats_slots(sh.D) * 2 * sizeof(float) +
         rows * 3 * sh.max_inner * es +
         rows * sh.max_inner * es + hb + (size_t)B * sh.max_ffn_st * es +  // hc (the CLS tail)
         (size_t)B * sh.head_st * es + 10 * 256 + extra;
}

struct DenseCall {
  int flags = 0;
  const void* A = nullptr;
  int64_t lda = 0;
  void* C = nullptr;
  int64_t ldc = 0;
  int M = 0, N = 0;
  const void* resid = nullptr;
  int64_t ldr = 0;
  const float* pos = nullptr;
  int64_t ldp = 0;
  int P = 0;
  const float* stats_in = nullptr;
  const float* rstats = nullptr;
  const float* rgamma = nullptr;
  const float* rbeta = nullptr;
  float* stats_out = nullptr;
  int ln_width = 0;    // LayerNorm width of stats_in / rstats / stats_out (0: the model width D)
  int stats_step = 1;  // EPI_LNIN: A row m reads stats_in row m * stats_step
  int slot_width = 0;  // width whose stats_slots() numbers the slots (0: ln_width)
  // the encoder's CLS tail (run_encoder): its M = B launches
  int rs_step = 1;     // EPI_RESLN / EPI_STATS: row m's rstats / stats_out rows are m * rs_step
  bool force_nt = false;  // the 128x128 kernel whatever M is (the same bits at every batch)
  int work_M = 0;      // rows evt_model_profile_work counts (0: M, < 0: none), dense_work
};

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

GemmParams dense_params(const evt_model* m, const DenseW& w, const DenseCall& c) {
  GemmParams p{};
  p.A = c.A;
  p.lda = c.lda;
  p.W = w.w;
  p.ldw = w.kpad;
  p.C = c.C;
  p.ldc = c.ldc;
  p.M = c.M;
  p.N = c.N;
  p.K = w.kpad;
  p.ntiles = w.npad / GEMM_BN;
  p.bias = w.b;
  p.resid = c.resid;
  p.ldr = c.ldr;
  p.pos = c.pos;
  p.ldp = c.ldp;
  p.P = c.P;
  p.vec_ok = (c.ldc % 4 == 0) && (c.ldr % 4 == 0) && (c.ldp % 4 == 0);
  if (p.vec_ok && c.ldc % 8 == 0 && c.ldr % 8 == 0 && c.ldp % 8 == 0 &&
      (((uintptr_t)c.C | (uintptr_t)c.resid) & 15) == 0)
    p.vec_ok = 2;
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
  const evt_features_args* a = call.feat;
  if (!a || call.feat_next >= a->n_taps || a->tap_blocks[call.feat_next] != block) return EVT_OK;
  return feat_export(m, m->ws.x, ldx, 1, a->taps[call.feat_next++], a->tap_norm != 0, rows, D,
                     call.s);
}

// Right after block `block`'s attention kernel of an evt_forward_attention call, while ws.qkv still
// holds the block's q and k in the layout `ap` describes: the block's map, if one was asked for
// (attn_maps.hip; counted under EVT_PROF_HEAD like the feature exports)
int attn_map(evt_model* m, ForwardCall& call, int block, const AttnParams& ap) {
  const evt_attn_args* a = call.attn;
  if (!a || call.attn_next >= a->n_maps || a->blocks[call.attn_next] != block) return EVT_OK;
  const int nq = a->queries == EVT_ATTN_ALL ? ap.N : 1;
  ProfScope ps(m, EVT_PROF_HEAD, call.s);
  const double bh = (double)ap.B * ap.H;
  prof_work(m, 4.0 * bh * nq * (double)ap.N * ap.hd,  // the scores, twice
            bh * ((double)(nq + ap.N) * ap.hd * elem_size(m->dtype) + (double)nq * ap.N * 4.0));
  EVT_HIP(attn_probs_launch(m->dtype, ap, nq, a->maps[call.attn_next++], call.s), "attention map");
  return EVT_OK;
}

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
int alloc_encoder_ws(evt_model* m, int B, size_t hbuf_bytes, hipStream_t s) {
  const size_t es = elem_size(m->dtype);
  if (m->dtype == DT_BF16) {
    EVT_RC(dev_alloc(m, &m->ws.sk, gemm_sk_bytes()));
    EVT_HIP(hipMemsetAsync(m->ws.sk, 0, 4096, s), "memset stream-K flags");
  }
  const size_t rows = (size_t)B * m->sh.T;
  // x, xm (width D) and o (width heads * h_k) are GEMM A operands read in 64-column K-tiles: with
  // a width that is not a multiple of 64 a row's last K-tile runs into the next row (cancelled by
  // the zero-padded weight rows) and the last row into PAD_K zeroed slack elements; every byte is
  // zeroed once here (finite everywhere)
  const size_t xb = (rows * m->D + PAD_K) * es, ob = (rows * m->sh.max_inner + PAD_K) * es;
  EVT_RC(dev_alloc(m, &m->ws.x, xb));
  EVT_RC(dev_alloc(m, &m->ws.xm, xb));
  const size_t stats_bytes = rows * stats_slots(m->D) * 2 * sizeof(float);
  EVT_RC(dev_alloc(m, (void**)&m->ws.sx, stats_bytes));
  EVT_RC(dev_alloc(m, (void**)&m->ws.sm, stats_bytes));
  EVT_RC(dev_alloc(m, &m->ws.qkv, rows * 3 * m->sh.max_inner * es));
  EVT_RC(dev_alloc(m, &m->ws.o, ob));
  EVT_HIP(hipMemsetAsync(m->ws.x, 0, xb, s), "memset x");
  EVT_HIP(hipMemsetAsync(m->ws.xm, 0, xb, s), "memset xm");
  EVT_HIP(hipMemsetAsync(m->ws.o, 0, ob, s), "memset o");
  EVT_RC(dev_alloc(m, &m->ws.hbuf, hbuf_bytes));
  m->ws.hbuf_bytes = hbuf_bytes;
  // the CLS tail's FFN hidden rows (FC1 writes all ffn_st columns of a row before FC2 reads them)
  if (!m->mx8) EVT_RC(dev_alloc(m, &m->ws.hc, (size_t)B * m->sh.max_ffn_st * es));
  return EVT_OK;
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
  GemmParams p{};
  p.A = c.A; p.lda = c.lda; p.W = w.w; p.ldw = w.kpad; p.C = c.C; p.ldc = c.ldc;
  p.M = c.M; p.N = c.N; p.K = w.kpad; p.ntiles = w.npad / GEMM_BN; p.bias = w.b;
  EVT_HIP(gemm_splitk_launch(m->dtype, c.flags, p, S, (float*)m->ws.hbuf, s), "dense (split-K)");
  return EVT_OK;
}

// Encoder layers (transformer_encoder.py:13-18 / :26-34) on the token stream m->ws.x (+ stats sx).
int run_encoder(evt_model* m, ForwardCall& call) {
  const int B = call.B, D = m->D, T = m->sh.T, rows = B * T;
  hipStream_t s = call.s;
  const float log2e = 1.4426950408889634f;
  m->hm_layers = 0;
  m->tail_mode = 0;
  int block = 0;
  for (const Layer& L : m->layers) {
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
    AttnParams ap{m->ws.qkv, 3 * L.inner, m->ws.o, L.inner, T, L.heads, B, scale_log2};
    ap.hd = L.hd;
    if (hm) {
      ap.ldq = 64;
      ap.sb = (int64_t)L.heads * 3 * T * 64;
      ap.sh = (int64_t)3 * T * 64;
      ap.ko = T * 64;
      ap.vo = 2 * T * 64;
    }
    // The classifier and `pooled` read token 0 of the last block and nothing else, so its
    // out-proj, FC1 and FC2 run on the B CLS rows (the CLS tail, below) and its attention on query
    // tile 0. A call that exports the last block's token map (tokens, or a tap on it) runs the
    // full-row block as well; the CLS rows it exports, and the head reads, are still the tail's.
    const bool last = block + 1 == (int)m->layers.size();
    bool full = !last;
    if (last && call.feat) {
      const evt_features_args* a = call.feat;
      full = a->tokens || (a->n_taps > 0 && a->tap_blocks[a->n_taps - 1] == block);
    }
    if (last) m->tail_mode = full ? 3 : 1;
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
    // out-proj + bias + LN1(x) residual -> xm (+ stats); STANDARD: + x
    DenseCall co;
    co.flags = m->standard ? (EPI_BIAS | EPI_RESID | EPI_STATS)
                           : (EPI_BIAS | EPI_RESID | EPI_RESLN | EPI_STATS);
    co.A = m->ws.o; co.lda = L.inner; co.C = m->ws.xm; co.ldc = D; co.M = rows; co.N = D;
    co.resid = m->ws.x; co.ldr = D; co.rstats = m->ws.sx; co.rgamma = L.ln1_g; co.rbeta = L.ln1_b;
    co.stats_out = m->ws.sm;
    // LN2-folded FC1 + GELU (ffn.py:8; STANDARD: exact erf GELU)
    DenseCall c1;
    c1.flags = EPI_LNIN | EPI_BIAS | (m->standard ? EPI_GELU_ERF : EPI_GELU);
    c1.A = m->ws.xm; c1.lda = D; c1.C = m->ws.hbuf; c1.ldc = L.ffn_st; c1.M = rows; c1.N = L.ffn_st;
    c1.stats_in = m->ws.sm;
    // FC2 + bias + LN2(xm) residual -> x (+ stats); STANDARD: + xm
    DenseCall c2;
    c2.flags = co.flags;
    c2.A = m->ws.hbuf; c2.lda = L.ffn_st; c2.C = m->ws.x; c2.ldc = D; c2.M = rows; c2.N = D;
    c2.resid = m->ws.xm; c2.ldr = D; c2.rstats = m->ws.sm; c2.rgamma = L.ln2_g; c2.rbeta = L.ln2_b;
    c2.stats_out = m->ws.sx;
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
    // Each full-row launch comes before its role's tail launch: the tail's out-proj still finds
    // the block's input rows in x / sx, and what it, FC1 and FC2 leave in rows b T of xm / sm,
    // hc and x / sx is what the next tail launch, the exports and the head read.
    {
      ProfScope ps(m, EVT_PROF_OUT_PROJ, s);
      if (full) EVT_RC(dense(m, L.out, co, s));
      if (last) EVT_RC(dense(m, L.out, tail(co), s));
    }
    {
      ProfScope ps(m, EVT_PROF_FC1, s);
      if (full) EVT_RC(dense(m, L.fc1, c1, s));
      if (last) EVT_RC(dense(m, L.fc1, tail(c1), s));
    }
    {
      ProfScope ps(m, EVT_PROF_FC2, s);
      if (full) EVT_RC(dense(m, L.fc2, c2, s));
      if (last) EVT_RC(dense(m, L.fc2, tail(c2), s));
    }
    EVT_RC(feat_tap(m, call, block++, D, rows, D));
  }
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

struct T2TShape {
  Shape enc;             // encoder geometry (P = (S/16)^2 patches, T = P + 1)
  int grid[3] = {0, 0, 0};
  int din[2] = {0, 0};   // unfolded widths feeding performer 1 / 2
};

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

size_t t2t_workspace_bytes(const evt_t2t_desc* d, const T2TShape& ts, int B) {
  const size_t es = elem_size(d->dtype);
  const size_t rows = (size_t)B * ts.enc.T, t1 = (size_t)B * ts.grid[0] * ts.grid[0];
  return t2t_unfold_elems(ts, B) * es + t2t_unfold_stat_floats(ts, B) * 4 + t1 * 4 * 64 * es +
         performer_part_floats(B, ts.grid[0] * ts.grid[0]) * 4 + 2 * rows * d->dim * es +
         2 * rows * stats_slots(d->dim) * 2 * 4 + rows * 4 * ts.enc.max_inner * es +
         rows * ts.enc.max_ffn_st * es + (size_t)B * ts.enc.max_ffn_st * es +  // hbuf, hc
         t1 * 2 * 4 + 2 * 256;
}

// ---- Swin geometry ------------------------------------------------------------------------
struct SwinGeo {
  int ns = 0;
  int C[EVT_SWIN_MAX_STAGES], Cst[EVT_SWIN_MAX_STAGES], R[EVT_SWIN_MAX_STAGES];
  int mlp[EVT_SWIN_MAX_STAGES], mst[EVT_SWIN_MAX_STAGES];
  int w[EVT_SWIN_MAX_STAGES];  // window of the stage: min(window_size, R)
  int pd = 0, pdst = 0;  // patch vector width (c, kh, kw) and its K padding
};

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

size_t swin_workspace_bytes(const evt_swin_desc* d, const SwinGeo& g, int B) {
  const SwinWs w = swin_ws(g, B);
  const size_t es = elem_size(d->dtype);
  return (2 * w.stream + w.qkv + w.o + w.hbuf + w.pooled + 3 * SWIN_SLACK) * es +
         2 * w.stats * sizeof(float);
}

// What the three creates open with: the checks of out, the descriptor (-> *geo) and the weights.
template <class Desc, class Geo>
int create_prologue(const Desc* desc, int (*validate_fn)(const Desc*, Geo*), Geo* geo,
                    int (*num_weights)(const Desc*), const float* const* w, int n_weights,
                    evt_model** out) {
  if (!out) return fail(EVT_EINVAL, "out is NULL");
  *out = nullptr;
  EVT_RC(validate_fn(desc, geo));
  if (n_weights != num_weights(desc) || !w)
    return fail(EVT_EINVAL, "expected " + std::to_string(num_weights(desc)) + " weights");
  for (int i = 0; i < n_weights; ++i)
    if (!w[i]) return fail(EVT_EINVAL, "weight pointer " + std::to_string(i) + " is NULL");
  return EVT_OK;
}

}  // namespace

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

int evt_vit_num_weights(const evt_vit_desc* desc) {
  if (!desc || desc->depth < 0) return fail(EVT_EINVAL, "bad desc");
  return 4 + (desc->semantics == EVT_VIT_STANDARD ? 12 : 11) * desc->depth + 4;
}

int evt_query_workspace(const evt_vit_desc* desc, int batch, size_t* bytes) {
  Shape sh;
  EVT_RC(validate(desc, &sh));
  if (!bytes || batch <= 0) return fail(EVT_EINVAL, "bytes must be non-null and batch positive");
  *bytes = workspace_bytes(desc, sh, batch);
  return EVT_OK;
}

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

static int swin_alloc_ws(evt_model* m, int B, hipStream_t s);  // (the Swin section)

// A forward of B images over the model's lanes (evt_model_set_lanes): lane i takes images
// [B i / k, B (i + 1) / k) on its own stream, forked from and joined to s by events (a HIP graph
// capture on s records the lanes as parallel branches)
static int run_family(evt_model* m, ForwardCall& call);
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
      EVT_RC(run_family(m->lanes[i], lane));
    }
    EVT_HIP(hipEventRecord(m->lane_ev[1 + i], m->lane_s[i]), "lane done");
  }
  for (int i = 0; i < k; ++i)
    EVT_HIP(hipStreamWaitEvent(s, m->lane_ev[1 + i], 0), "lanes join");
  m->hm_layers = m->lanes[0]->hm_layers;
  m->tail_mode = m->lanes[0]->tail_mode;
  return EVT_OK;
}

static int check_batch(const evt_model* m, int B) {
  if (B <= 0 || B > m->max_batch)
    return fail(EVT_EINVAL, "batch must be in [1, max_batch=" + std::to_string(m->max_batch) + "]");
  return EVT_OK;
}

// Every forward, eager or captured: over the lanes when the caller asked for them (logits-only
// forwards do), the handle has lanes, is not profiling (profiling: one lane) and every lane gets
// an image; on this handle's own workspace otherwise.
static int forward(evt_model* m, ForwardCall& call, bool use_lanes) {
  EVT_RC(check_batch(m, call.B));
  if (use_lanes && !m->lanes.empty() && !m->prof && call.B >= (int)m->lanes.size())
    return lanes_forward(m, call);
  return run_family(m, call);
}

// What evt_{vit,t2t,swin}_forward are: the argument checks, then the forward of an fp32 batch
static int family_forward(evt_model* m, int family, const char* wrong_family, const float* img,
                          int B, float* logits, void* stream) {
  if (!m || !img || !logits) return fail(EVT_EINVAL, "model, img and logits must be non-null");
  if (m->family != family) return fail(EVT_EINVAL, wrong_family);
  ForwardCall call;
  call.img = img; call.B = B; call.logits = logits; call.s = (hipStream_t)stream;
  return forward(m, call, true);
}

// The ViT workspace for B images (activation buffers only; lanes allocate their own)
static int vit_alloc_ws(evt_model* m, int B, hipStream_t s) {
  const Shape& sh = m->sh;
  const int D = m->D;
  const size_t es = elem_size(m->dtype);
  EVT_RC(alloc_encoder_ws(m, B, std::max((size_t)B * sh.T * sh.max_ffn_st,
                                         (size_t)B * sh.P * sh.pdst) * es, s));
  m->ws.apatch = m->ws.hbuf;
  EVT_RC(dev_alloc(m, &m->ws.hh, (size_t)B * sh.head_st * es));
  if (m->mx8) {
    const size_t rows = (size_t)B * sh.T;
    m->ws.qa_ld = (int)std::max(round_up(D, 128), round_up(sh.max_inner, 128));
    int maxffn = 0;
    for (int f : m->ffn) maxffn = std::max(maxffn, f);
    m->ws.qh_ld = (int)round_up(maxffn, 128);
    EVT_RC(dev_alloc(m, &m->ws.qa, rows * m->ws.qa_ld));
    EVT_RC(dev_alloc(m, (void**)&m->ws.sa, rows * (m->ws.qa_ld / 128) * 4));
    EVT_RC(dev_alloc(m, &m->ws.qh, rows * m->ws.qh_ld));
    EVT_RC(dev_alloc(m, (void**)&m->ws.shd, rows * (m->ws.qh_ld / 128) * 4));
    EVT_RC(dev_alloc(m, (void**)&m->ws.lnst, rows * 2 * sizeof(float)));
    // every byte of the MX8 operands is written finite before it is read (NaN-free padding)
    EVT_HIP(hipMemsetAsync(m->ws.qa, 0, rows * m->ws.qa_ld, s), "memset qa");
    EVT_HIP(hipMemsetAsync(m->ws.sa, 0, rows * (m->ws.qa_ld / 128) * 4, s), "memset qa scales");
    // FC1 writes columns < roundup(ffn, 32) only: the rest of the FC2 operand stays zero
    EVT_HIP(hipMemsetAsync(m->ws.qh, 0, rows * m->ws.qh_ld, s), "memset qh");
    EVT_HIP(hipMemsetAsync(m->ws.shd, 0, rows * (m->ws.qh_ld / 128) * 4, s), "memset qh scales");
  }
  return EVT_OK;
}

int evt_vit_create(const evt_vit_desc* desc, const float* const* w, int n_weights, void* stream,
                   evt_model** out) {
  Shape sh;
  EVT_RC(create_prologue(desc, validate, &sh, evt_vit_num_weights, w, n_weights, out));
  hipStream_t s = (hipStream_t)stream;
  evt_model* m = new evt_model();
  m->family = 0;
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
    EVT_RC(vit_alloc_ws(m, desc->max_batch, s));
    EVT_HIP(hipStreamSynchronize(s), "create sync");
    return EVT_OK;
  };
  return finish_create(m, run(), out);
}

// The final token map and the pooled (CLS) vector of a ViT / T2T-ViT features forward, from the
// stream the last encoder block left in ws.x
static int encoder_features(evt_model* m, const ForwardCall& call) {
  const evt_features_args* a = call.feat;
  const int B = call.B, D = m->D, T = m->sh.T;
  hipStream_t s = call.s;
  const bool norm = m->norm_g != nullptr;  // REFERENCE ViT: no final LayerNorm (vit.py:54)
  if (a->tokens) EVT_RC(feat_export(m, m->ws.x, D, 1, a->tokens, norm, B * T, D, s));
  if (a->pooled) EVT_RC(feat_export(m, m->ws.x, D, T, a->pooled, norm, B, D, s));
  return EVT_OK;
}

// The ViT forward of call.B images on this handle's own workspace. In a features forward
// (call.feat) the taps, tokens and pooled are exported along the way and logits may be NULL (no
// head then).
static int vit_run(evt_model* m, ForwardCall& call) {
  const evt_vit_desc& d = m->desc;
  const Shape& sh = m->sh;
  const int B = call.B, D = d.dim, T = sh.T, dt = m->dtype;
  const float* img = call.img;
  float* logits = call.logits;
  hipStream_t s = call.s;
  prof_reset(m);
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
  EVT_RC(m->mx8 ? run_encoder_mx8(m, call) : run_encoder(m, call));
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

int evt_vit_forward(evt_model* m, const float* img, int B, float* logits, void* stream) {
  return family_forward(m, 0, "model is not a ViT (use evt_t2t_forward)", img, B, logits, stream);
}

// ---- T2T-ViT ----------------------------------------------------------------------------

int evt_t2t_num_weights(const evt_t2t_desc* desc) {
  if (!desc || desc->depth < 0) return fail(EVT_EINVAL, "bad desc");
  return 2 * 13 + 4 + 11 * desc->depth + 4;
}

int evt_t2t_query_workspace(const evt_t2t_desc* desc, int batch, size_t* bytes) {
  T2TShape ts;
  EVT_RC(validate_t2t(desc, &ts));
  if (!bytes || batch <= 0) return fail(EVT_EINVAL, "bytes must be non-null and batch positive");
  *bytes = t2t_workspace_bytes(desc, ts, batch);
  return EVT_OK;
}

// The T2T-ViT workspace for B images (activation buffers only; lanes allocate their own)
static int t2t_alloc_ws(evt_model* m, int B, hipStream_t s) {
  T2TShape ts;
  EVT_RC(validate_t2t(&m->tdesc, &ts));
  const size_t es = elem_size(m->dtype);
  const size_t t1 = (size_t)B * ts.grid[0] * ts.grid[0];
  EVT_RC(dev_alloc(m, &m->ws.u, t2t_unfold_elems(ts, B) * es));
  EVT_RC(dev_alloc(m, (void**)&m->ws.su, t2t_unfold_stat_floats(ts, B) * sizeof(float)));
  EVT_RC(dev_alloc(m, &m->ws.kqvb, t1 * 3 * 64 * es));
  EVT_RC(dev_alloc(m, &m->ws.pout, t1 * 64 * es));
  EVT_RC(dev_alloc(m, (void**)&m->ws.tstats, t1 * 2 * sizeof(float)));
  EVT_RC(dev_alloc(m, &m->ws.zrow, 256));
  EVT_HIP(hipMemsetAsync(m->ws.zrow, 0, 256, s), "memset zero row");
  EVT_RC(dev_alloc(m, (void**)&m->ws.part, performer_part_floats(B, ts.grid[0] * ts.grid[0]) *
                                            sizeof(float)));
  EVT_RC(alloc_encoder_ws(m, B, (size_t)B * ts.enc.T * ts.enc.max_ffn_st * es, s));
  return EVT_OK;
}

int evt_t2t_create(const evt_t2t_desc* desc, const float* const* w, int n_weights, void* stream,
                   evt_model** out) {
  T2TShape ts;
  EVT_RC(create_prologue(desc, validate_t2t, &ts, evt_t2t_num_weights, w, n_weights, out));
  hipStream_t s = (hipStream_t)stream;
  evt_model* m = new evt_model();
  m->family = 1;
  m->dtype = desc->dtype;
  m->D = desc->dim;
  m->max_batch = desc->max_batch;
  m->num_classes = desc->num_classes;
  m->tdesc = *desc;
  m->heads.assign(desc->depth, desc->heads);
  m->head_dim.assign(desc->depth, desc->dim / desc->heads);  // h_k = dim // heads
  m->ffn.assign(desc->depth, desc->mlp_dim);
  m->sh = ts.enc;
  m->img_elems = (size_t)desc->image_size * desc->image_size * desc->in_chans;
  for (int i = 0; i < 3; ++i) m->grid[i] = ts.grid[i];
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
    EVT_RC(t2t_alloc_ws(m, desc->max_batch, s));
    EVT_HIP(hipStreamSynchronize(s), "create sync");
    return EVT_OK;
  };
  return finish_create(m, run(), out);
}

// The T2T-ViT forward on this handle's own workspace (features forwards: as vit_run)
static int t2t_run(evt_model* m, ForwardCall& call) {
  prof_reset(m);
  const evt_t2t_desc& d = m->tdesc;
  const int B = call.B, dt = d.dtype, D = d.dim, T = m->sh.T, P = m->sh.P, S = d.image_size;
  float* logits = call.logits;
  hipStream_t s = call.s;
  const int g1 = m->grid[0], g2 = m->grid[1];
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
  const int g3 = m->grid[2];
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

int evt_t2t_forward(evt_model* m, const float* img, int B, float* logits, void* stream) {
  return family_forward(m, 1, "model is not a T2T-ViT (use evt_vit_forward)", img, B, logits,
                        stream);
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
      c->no_balance = m->family == 1 ? 1 : 0;
      m->lanes.push_back(c);
      EVT_RC(m->family == 0   ? vit_alloc_ws(c, per, s)
             : m->family == 1 ? t2t_alloc_ws(c, per, s)
                              : swin_alloc_ws(c, per, s));
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

// ---- Swin Transformer -------------------------------------------------------------------

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
  *bytes = swin_workspace_bytes(desc, g, batch);
  return EVT_OK;
}

// The Swin workspace for B images (activation buffers only; lanes allocate their own)
static int swin_alloc_ws(evt_model* m, int B, hipStream_t s) {
  SwinGeo g;
  EVT_RC(validate_swin(&m->sdesc, &g));
  const SwinWs ws = swin_ws(g, B);
  const size_t es = elem_size(m->dtype);
  EVT_RC(dev_alloc(m, &m->ws.x, (ws.stream + SWIN_SLACK) * es));
  EVT_RC(dev_alloc(m, &m->ws.xm, (ws.stream + SWIN_SLACK) * es));
  EVT_HIP(hipMemsetAsync(m->ws.x, 0, (ws.stream + SWIN_SLACK) * es, s), "memset x");
  EVT_HIP(hipMemsetAsync(m->ws.xm, 0, (ws.stream + SWIN_SLACK) * es, s), "memset xm");
  EVT_RC(dev_alloc(m, (void**)&m->ws.sx, ws.stats * sizeof(float)));
  EVT_RC(dev_alloc(m, (void**)&m->ws.sm, ws.stats * sizeof(float)));
  EVT_RC(dev_alloc(m, &m->ws.qkv, ws.qkv * es));
  EVT_RC(dev_alloc(m, &m->ws.o, (ws.o + SWIN_SLACK) * es));
  EVT_HIP(hipMemsetAsync(m->ws.o, 0, (ws.o + SWIN_SLACK) * es, s), "memset o");
  EVT_RC(dev_alloc(m, &m->ws.hbuf, ws.hbuf * es));
  EVT_RC(dev_alloc(m, &m->ws.pooled, ws.pooled * es));
  if (m->dtype == DT_BF16) {
    EVT_RC(dev_alloc(m, &m->ws.sk, gemm_sk_bytes()));
    EVT_HIP(hipMemsetAsync(m->ws.sk, 0, 4096, s), "memset stream-K flags");
  }
  return EVT_OK;
}

int evt_swin_create(const evt_swin_desc* desc, const float* const* w, int n_weights, void* stream,
                    evt_model** out) {
  SwinGeo g;
  EVT_RC(create_prologue(desc, validate_swin, &g, evt_swin_num_weights, w, n_weights, out));
  hipStream_t s = (hipStream_t)stream;
  evt_model* m = new evt_model();
  m->family = 2;
  m->dtype = desc->dtype;
  m->D = desc->embed_dim;
  m->max_batch = desc->max_batch;
  m->num_classes = desc->num_classes;
  m->sdesc = *desc;
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
    EVT_RC(swin_alloc_ws(m, desc->max_batch, s));
    EVT_HIP(hipStreamSynchronize(s), "create sync");
    return EVT_OK;
  };
  return finish_create(m, run(), out);
}

// The Swin forward on this handle's own workspace (features forwards: as vit_run)
static int swin_run(evt_model* m, ForwardCall& call) {
  prof_reset(m);
  const evt_swin_desc& d = m->sdesc;
  const int B = call.B, dt = d.dtype;
  float* logits = call.logits;
  hipStream_t s = call.s;
  const SwinStage& s0 = m->stages[0];
  const int pdst = (int)round_up(d.in_chans * d.patch_size * d.patch_size, PAD_K);
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
          DenseCall c;
          c.flags = EPI_LNIN | EPI_BIAS;
          c.A = m->ws.x; c.lda = Cst; c.C = m->ws.qkv; c.ldc = 3 * C; c.M = rows; c.N = 3 * C;
          c.stats_in = m->ws.sx; c.ln_width = C;
          EVT_RC(dense(m, bl.qkv, c, s));
        }
        {
          ProfScope ps(m, EVT_PROF_ATTENTION, s);
          prof_work(m, 4.0 * rows * st.w * st.w * C, 4.0 * rows * C * es);  // w^2 keys per query
          SwinAttnParams ap{m->ws.qkv, 3 * C, m->ws.o, Cst, bl.bias, B, st.R, st.R / st.w, C, st.H,
                            bl.shift, scale_log2};
          EVT_HIP(st.w == 12 ? window12_attn_launch(dt, ap, s) : window_attn_launch(dt, ap, s),
                  "window attention");
        }
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

int evt_swin_forward(evt_model* m, const float* img, int B, float* logits, void* stream) {
  return family_forward(m, 2, "model is not a Swin Transformer", img, B, logits, stream);
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
  const hipError_t e = window_attn_launch(dtype, ap, s);
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

// ---- op-level entry points --------------------------------------------------------------

int evt_set_gemm_variant(int variant) {
  if (!gemm_variant_supported(variant))
    return fail(EVT_EINVAL, "variant must be 0, 1, 2, 6, 8, 9, 16, 30, 31 or 36 (lab builds: also "
                            "10, 11, 13, 15, 17-25, 106, 108)");
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
  GemmParams p{};
  p.A = a->A; p.lda = a->lda; p.W = a->Wp; p.ldw = a->Kpad; p.C = a->C; p.ldc = a->ldc;
  p.M = a->M; p.N = a->N; p.K = a->Kpad; p.ntiles = a->Npad / GEMM_BN;
  p.bias = a->bias; p.resid = a->resid; p.ldr = a->ldr; p.pos = a->pos; p.ldp = a->ldp; p.P = a->P;
  p.vec_ok = (a->ldc % 4 == 0) && (a->ldr % 4 == 0) && (a->ldp % 4 == 0);
  if (p.vec_ok && a->ldc % 8 == 0 && a->ldr % 8 == 0 && a->ldp % 8 == 0 &&
      (((uintptr_t)a->C | (uintptr_t)a->resid) & 15) == 0)
    p.vec_ok = 2;
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
  GemmParams p{};
  p.A = a->A; p.lda = a->lda; p.W = a->Wp; p.ldw = a->Kpad; p.C = a->C; p.ldc = a->ldc;
  p.M = a->M; p.N = a->N; p.K = a->Kpad; p.ntiles = a->Npad / GEMM_BN; p.bias = a->bias;
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

// ---- feature outputs (include/evt_features.h) ---------------------------------------------

static int model_blocks(const evt_model* m) {
  if (m->family != 2) return (int)m->layers.size();
  int n = 0;
  for (const SwinStage& st : m->stages) n += (int)st.blocks.size();
  return n;
}

int evt_features_shape(const evt_model* m, int* F, int* T, int* n_blocks) {
  if (!m) return fail(EVT_EINVAL, "model is NULL");
  const bool swin = m->family == 2;
  if (F) *F = swin ? m->stages.back().C : m->D;
  if (T) *T = swin ? m->stages.back().R * m->stages.back().R : m->sh.T;
  if (n_blocks) *n_blocks = model_blocks(m);
  return EVT_OK;
}

int evt_tap_shape(const evt_model* m, int block, int* tokens, int* width) {
  if (!m || !tokens || !width) return fail(EVT_EINVAL, "null argument");
  if (block < 0 || block >= model_blocks(m))
    return fail(EVT_EINVAL, "block must be in [0, " + std::to_string(model_blocks(m)) + ")");
  *tokens = m->sh.T;
  *width = m->D;
  if (m->family == 2) {
    for (const SwinStage& st : m->stages) {
      if (block < (int)st.blocks.size()) {
        *tokens = st.R * st.R;
        *width = st.C;
        break;
      }
      block -= (int)st.blocks.size();
    }
  }
  return EVT_OK;
}

// What evt_forward_features checks of (model, outputs, batch); evt_forward_image shares it
static int validate_features(const evt_model* m, const evt_features_args* a, int B) {
  if (a->n_taps < 0 || a->n_taps > 64) return fail(EVT_EINVAL, "n_taps must be in [0, 64]");
  if (!a->logits && !a->pooled && !a->tokens && a->n_taps == 0)
    return fail(EVT_EINVAL, "no output requested: logits, pooled and tokens are NULL, n_taps is 0");
  EVT_RC(check_batch(m, B));  // (here, ahead of forward's own: the order the checks fire in)
  if (a->tap_norm != 0 && a->tap_norm != 1) return fail(EVT_EINVAL, "tap_norm must be 0 or 1");
  if (a->tap_norm && (m->family == 2 || !m->norm_g))
    return fail(EVT_EINVAL, m->family == 2
                                ? "tap_norm: Swin stage widths differ from the final LayerNorm's"
                                : "tap_norm: a REFERENCE ViT has no final LayerNorm");
  uintptr_t align = (uintptr_t)a->pooled | (uintptr_t)a->tokens;  // 16-B stores (features.hip)
  if (a->n_taps > 0) {
    if (!a->tap_blocks || !a->taps)
      return fail(EVT_EINVAL, "n_taps > 0 needs the tap_blocks and taps arrays");
    if (m->mx8) return fail(EVT_EINVAL, "taps are not available on an EVT_DTYPE_MX8 model");
    const int nb = model_blocks(m);
    for (int i = 0; i < a->n_taps; ++i) {
      if (a->tap_blocks[i] < 0 || a->tap_blocks[i] >= nb)
        return fail(EVT_EINVAL, "tap block " + std::to_string(a->tap_blocks[i]) +
                                    " is outside [0, " + std::to_string(nb) + ")");
      if (i > 0 && a->tap_blocks[i] <= a->tap_blocks[i - 1])
        return fail(EVT_EINVAL, "tap_blocks must be strictly increasing");
      if (!a->taps[i]) return fail(EVT_EINVAL, "tap pointer " + std::to_string(i) + " is NULL");
      align |= (uintptr_t)a->taps[i];
    }
  }
  if (align & 15) return fail(EVT_EINVAL, "feature outputs must be 16-byte aligned");
  return EVT_OK;
}

static int run_family(evt_model* m, ForwardCall& call) {
  return m->family == 0 ? vit_run(m, call) : m->family == 1 ? t2t_run(m, call) : swin_run(m, call);
}

int evt_forward_features(evt_model* m, const float* img, int B, const evt_features_args* a,
                         void* stream) {
  if (!m || !img || !a) return fail(EVT_EINVAL, "model, img and args must be non-null");
  EVT_RC(validate_features(m, a, B));
  ForwardCall call;
  call.img = img; call.B = B; call.logits = a->logits; call.feat = a; call.s = (hipStream_t)stream;
  // one lane, on this handle's own workspace, whatever its lane count (as a profiled forward)
  return forward(m, call, false);
}

// ---- uint8 image input (include/evt_image.h) ------------------------------------------------

static int affine_from(const float* scale, const float* shift, int C, ImgAffine* aff,
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

// The descriptor alone (no model needed), then what the model adds for EVT_IMG_U8_NHWC
static int validate_image(const evt_model* m, const evt_image_args* in, ImgAffine* aff) {
  if (!in) return fail(EVT_EINVAL, "image descriptor is NULL");
  if (!in->data) return fail(EVT_EINVAL, "image data is NULL");
  if (in->format != EVT_IMG_F32 && in->format != EVT_IMG_U8_NHWC)
    return fail(EVT_EINVAL, "unknown image format " + std::to_string(in->format));
  if (!m) return fail(EVT_EINVAL, "model is NULL");
  if (in->format == EVT_IMG_F32) return EVT_OK;
  const int C = m->family == 0 ? m->desc.in_chans : m->family == 1 ? m->tdesc.in_chans
                                                                   : m->sdesc.in_chans;
  const int S = m->family == 0 ? m->desc.image_size : m->family == 1 ? m->tdesc.image_size
                                                                     : m->sdesc.image_size;
  if (C > 4) return fail(EVT_EINVAL, "uint8 input: in_chans must be <= 4");
  EVT_RC(affine_from(in->scale, in->shift, C, aff, "uint8 input"));
  const uintptr_t a = (uintptr_t)in->data;
  if (m->family == 1) return (C == 4 && (a & 3)) ? fail(EVT_EINVAL, "uint8 input: data must be 4-byte aligned") : EVT_OK;
  const int ps = m->family == 0 ? m->desc.patch_size : m->sdesc.patch_size;
  if (((int64_t)ps * S * C) % 4)
    return fail(EVT_EINVAL, "uint8 input: patch_size*image_size*in_chans must be a multiple of 4");
  if (m->family == 0 && !m->patch_cm && !m->patch_ld)
    return fail(EVT_EINVAL, "uint8 input: this ViT's patch vectors are not channel-major "
                            "(patch_size % 8 != 0 with patch_size^2*in_chans % 64 == 0)");
  // lanes start at multiples of S*S*C bytes: a multiple of 4 (and of 16 for the fused stem)
  const bool stem96 = m->family == 2 && m->dtype == DT_BF16 && C == 3 && ps == 4 &&
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

int evt_forward_image(evt_model* m, const evt_image_args* in, int B, const evt_features_args* a,
                      void* stream) {
  ImgAffine aff{};
  if (!a) return fail(EVT_EINVAL, "image descriptor, outputs and model must be non-null");
  EVT_RC(validate_image(m, in, &aff));
  EVT_RC(validate_features(m, a, B));
  // logits alone: over the handle's lanes, like evt_*_forward; anything more: a features forward
  const bool logits_only = a->logits && !a->pooled && !a->tokens && a->n_taps == 0;
  ForwardCall call = image_call(in, aff, B, a->logits, stream);
  if (!logits_only) call.feat = a;
  return forward(m, call, logits_only);
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
  if (m->family == 2)
    return fail(EVT_EINVAL, "attention maps: Swin's windowed, biased attention is not exported");
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

int evt_forward_attention(evt_model* m, const evt_image_args* in, int B,
                          const evt_features_args* feat, const evt_attn_args* a, void* stream) {
  ImgAffine aff{};
  if (!m || !in || !a) return fail(EVT_EINVAL, "model, image descriptor and attn must be non-null");
  EVT_RC(validate_image(m, in, &aff));
  EVT_RC(attn_family(m));
  if (a->n_maps < 0 || a->n_maps > 64) return fail(EVT_EINVAL, "n_maps must be in [0, 64]");
  if (a->n_maps == 0 && !feat)
    return fail(EVT_EINVAL, "no output requested: n_maps is 0 and feat is NULL");
  if (feat) EVT_RC(validate_features(m, feat, B));
  else EVT_RC(check_batch(m, B));
  if (a->queries != EVT_ATTN_CLS && a->queries != EVT_ATTN_ALL)
    return fail(EVT_EINVAL, "queries must be EVT_ATTN_CLS or EVT_ATTN_ALL");
  if (a->n_maps > 0) {
    if (!a->blocks || !a->maps) return fail(EVT_EINVAL, "n_maps > 0 needs the blocks and maps arrays");
    const int nb = (int)m->layers.size();
    for (int i = 0; i < a->n_maps; ++i) {
      if (a->blocks[i] < 0 || a->blocks[i] >= nb)
        return fail(EVT_EINVAL, "map block " + std::to_string(a->blocks[i]) + " is outside [0, " +
                                    std::to_string(nb) + ")");
      if (i > 0 && a->blocks[i] <= a->blocks[i - 1])
        return fail(EVT_EINVAL, "map blocks must be strictly increasing");
      if (!a->maps[i]) return fail(EVT_EINVAL, "map pointer " + std::to_string(i) + " is NULL");
      if ((uintptr_t)a->maps[i] & 15) return fail(EVT_EINVAL, "attention maps must be 16-byte aligned");
    }
  }
  ForwardCall call = image_call(in, aff, B, feat ? feat->logits : nullptr, stream);
  call.feat = feat;
  call.attn = a;
  // one lane, on this handle's own workspace, whatever its lane count (as a features forward)
  return forward(m, call, false);
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

// ---- classification outputs (include/evt_classify.h) ----------------------------------------

// What evt_classify checks of its arguments (the logits pointer aside); evt_forward_classify
// shares it. Fills the launch parameters.
static int validate_classify(const evt_classify_args* a, int B, int C, int64_t ldl,
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

int evt_classify(const float* logits, int64_t ldl, int B, int C, const evt_classify_args* a,
                 void* stream) {
  if (!logits) return fail(EVT_EINVAL, "classify: logits are NULL");
  if ((uintptr_t)logits & 3) return fail(EVT_EINVAL, "classify: logits must be 4-byte aligned");
  ClassifyParams p;
  EVT_RC(validate_classify(a, B, C, ldl, &p));
  EVT_HIP(classify_launch(logits, ldl, B, C, p, (hipStream_t)stream), "classify");
  return EVT_OK;
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
  // the forward of evt_forward_image: logits alone over the lanes, anything more as one lane
  const bool logits_only = !feat->pooled && !feat->tokens && feat->n_taps == 0;
  ForwardCall call = image_call(in, aff, B, feat->logits, stream);
  if (!logits_only) call.feat = feat;
  EVT_RC(forward(m, call, logits_only));
  // the lanes have joined `stream` (lanes_forward): the logits of every image are ordered before
  ProfScope ps(m, EVT_PROF_HEAD, call.s);
  prof_work(m, 0.0, (double)B * m->num_classes * 4.0 * (p.k + 1 + (p.labels ? 1 : 0)));
  EVT_HIP(classify_launch(feat->logits, m->num_classes, B, m->num_classes, p, call.s), "classify");
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

// ---- uint8 resize + centre crop (include/evt_preprocess.h) -----------------------------------
// The tables are Pillow's (libImaging Resample.c precompute_coeffs / normalize_coeffs_8bpc),
// restated. fp64, every operation rounded on its own: no contraction in this part of the file.
#pragma clang fp contract(off)

static double resize_filter(int filter, double x) {
  if (x < 0.0) x = -x;
  if (filter == EVT_RESIZE_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
  const double a = -0.5;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

static bool resize_filter_ok(int filter) {
  return filter == EVT_RESIZE_BILINEAR || filter == EVT_RESIZE_BICUBIC;
}

static int resize_ksize(int in, int out, int filter) {
  double fs = (double)in / (double)out;
  if (fs < 1.0) fs = 1.0;
  const double support = (filter == EVT_RESIZE_BILINEAR ? 1.0 : 2.0) * fs;
  return (int)std::ceil(support) * 2 + 1;
}

// bounds [count][2] and kk [count][ksize] of output indices first .. first+count-1; false if a
// coefficient leaves the 24-bit range the kernel multiplies in (it cannot for these filters)
static bool resize_tables(int in, int out, int first, int count, int filter, int32_t* bounds,
                          int32_t* kk) {
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = (filter == EVT_RESIZE_BILINEAR ? 1.0 : 2.0) * fs;
  const double ss = 1.0 / fs;
  const int ksize = (int)std::ceil(support) * 2 + 1;
  std::vector<double> w((size_t)ksize);
  bool ok = true;
  for (int i = 0; i < count; ++i) {
    const double center = (first + i + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    const int n = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      w[x] = resize_filter(filter, (x + xmin - center + 0.5) * ss);
      ww += w[x];
    }
    int32_t* k = kk + (size_t)i * ksize;
    for (int x = 0; x < ksize; ++x) k[x] = 0;
    for (int x = 0; x < n; ++x) {
      const double v = ww != 0.0 ? w[x] / ww : w[x];
      const double f = v < 0 ? -0.5 + v * (double)(1 << 22) : 0.5 + v * (double)(1 << 22);
      if (!(std::fabs(f) < (double)(1 << 23))) ok = false;
      k[x] = (int32_t)f;
    }
    bounds[2 * i] = xmin;
    bounds[2 * i + 1] = n;
  }
  return ok;
}

struct ResizeGeom {
  int oh, ow, top, left, ksh, ksv;
};

static int round_half_even_half(int d) {  // round(d / 2.0), d >= 0, ties to even
  const int q = d / 2;
  return (d & 1) ? q + (q & 1) : q;
}

static int resize_geom(int in_h, int in_w, int R, int S, int filter, ResizeGeom* g) {
  if (in_h < 1 || in_w < 1 || in_h > EVT_RESIZE_MAX_SIDE || in_w > EVT_RESIZE_MAX_SIDE)
    return fail(EVT_EINVAL, "resize: image sides must be in [1, " +
                                std::to_string(EVT_RESIZE_MAX_SIDE) + "]");
  if (S < 1 || S > EVT_RESIZE_MAX_SIDE)
    return fail(EVT_EINVAL, "resize: crop must be in [1, " + std::to_string(EVT_RESIZE_MAX_SIDE) + "]");
  if (R < 0 || R > EVT_RESIZE_MAX_SIDE)
    return fail(EVT_EINVAL, "resize: resize_short must be in [0, " +
                                std::to_string(EVT_RESIZE_MAX_SIDE) + "] (0: int(256/224 * crop))");
  if (!resize_filter_ok(filter))
    return fail(EVT_EINVAL, "resize: filter must be EVT_RESIZE_BILINEAR (2) or EVT_RESIZE_BICUBIC (3)");
  if (R == 0) R = (int)((256.0 / 224.0) * (double)S);
  if (R < 1) return fail(EVT_EINVAL, "resize: resize_short must be at least 1");
  double other;
  if (in_w <= in_h) {
    other = (double)((int64_t)R * in_h) / (double)in_w;
    g->ow = R;
  } else {
    other = (double)((int64_t)R * in_w) / (double)in_h;
    g->oh = R;
  }
  if (other > 16.0 * EVT_RESIZE_MAX_SIDE)
    return fail(EVT_EINVAL, "resize: the resized long side is beyond any supported size");
  (in_w <= in_h ? g->oh : g->ow) = (int)other;
  if (g->oh < S || g->ow < S)
    return fail(EVT_EINVAL, "resize: the resized image " + std::to_string(g->oh) + " x " +
                                std::to_string(g->ow) + " is smaller than the crop " +
                                std::to_string(S) + " (padding is not done)");
  g->top = round_half_even_half(g->oh - S);
  g->left = round_half_even_half(g->ow - S);
  g->ksh = resize_ksize(in_w, g->ow, filter);
  g->ksv = resize_ksize(in_h, g->oh, filter);
  return EVT_OK;
}

#pragma clang fp contract(on)

struct evt_resize_plan {
  uint32_t magic;
  int in_h, in_w, C, S, tr, nbands;
  size_t lds;  // bytes of the largest band
  ResizeGeom g;
  int32_t* tab;  // device: ResizeDesc::tab
};
static constexpr uint32_t RESIZE_MAGIC = 0x52535a50u;  // "RSZP"
static constexpr int RESIZE_MAX_TR = 16;
static_assert(RESIZE_CHUNK == EVT_RESIZE_CHUNK, "evt_preprocess.h and evt_internal.h disagree");

int evt_resize_geometry(int in_h, int in_w, int resize_short, int crop, int filter, int* oh,
                        int* ow, int* top, int* left, int* ksize_h, int* ksize_v) {
  ResizeGeom g{};
  EVT_RC(resize_geom(in_h, in_w, resize_short, crop, filter, &g));
  if (oh) *oh = g.oh;
  if (ow) *ow = g.ow;
  if (top) *top = g.top;
  if (left) *left = g.left;
  if (ksize_h) *ksize_h = g.ksh;
  if (ksize_v) *ksize_v = g.ksv;
  return EVT_OK;
}

int evt_resize_coefficients(int in_size, int out_size, int first, int count, int filter,
                            int32_t* bounds, int32_t* kk) {
  if (!bounds || !kk) return fail(EVT_EINVAL, "resize_coefficients: bounds and kk must be non-null");
  if (in_size < 1 || out_size < 1 || in_size > EVT_RESIZE_MAX_SIDE ||
      out_size > 16 * EVT_RESIZE_MAX_SIDE)
    return fail(EVT_EINVAL, "resize_coefficients: sizes out of range");
  if (first < 0 || count < 0 || first > out_size - count)
    return fail(EVT_EINVAL, "resize_coefficients: the window must lie inside [0, out_size]");
  if (!resize_filter_ok(filter))
    return fail(EVT_EINVAL, "resize_coefficients: filter must be EVT_RESIZE_BILINEAR (2) or "
                            "EVT_RESIZE_BICUBIC (3)");
  if (!resize_tables(in_size, out_size, first, count, filter, bounds, kk))
    return fail(EVT_EINVAL, "resize_coefficients: a coefficient is outside the 24-bit range");
  return EVT_OK;
}

int evt_resize_plan_create(int in_h, int in_w, int channels, int resize_short, int crop,
                           int filter, evt_resize_plan** out) {
  if (!out) return fail(EVT_EINVAL, "resize_plan_create: out is NULL");
  *out = nullptr;
  if (channels < 1 || channels > 4)
    return fail(EVT_EINVAL, "resize_plan_create: uint8 images have 1 to 4 channels");
  ResizeGeom g{};
  EVT_RC(resize_geom(in_h, in_w, resize_short, crop, filter, &g));
  const int S = crop, C = channels;
  if (((int64_t)S * C) % 4)
    return fail(EVT_EINVAL, "resize_plan_create: crop*channels must be a multiple of 4");
  const int64_t lp = ((int64_t)S * C + 15) & ~(int64_t)15;
  const size_t ntab = (size_t)S * (4 + g.ksh + g.ksv);
  std::vector<int32_t> tab(ntab);
  int32_t* bh = tab.data();
  int32_t* kh = bh + 2 * S;
  int32_t* bv = kh + (size_t)S * g.ksh;
  int32_t* kv = bv + 2 * S;
  if (!resize_tables(in_w, g.ow, g.left, S, filter, bh, kh) ||
      !resize_tables(in_h, g.oh, g.top, S, filter, bv, kv))
    return fail(EVT_EINVAL, "resize_plan_create: a coefficient is outside the 24-bit range");
  // the kernel's band is rows bv[y0].ymin .. bv[y1-1].ymin + n: both ends must not decrease with y
  for (int y = 0; y < S; ++y) {
    const bool in_range = bv[2 * y] >= 0 && bv[2 * y + 1] >= 1 && bv[2 * y] + bv[2 * y + 1] <= in_h &&
                          bh[2 * y] >= 0 && bh[2 * y + 1] >= 1 && bh[2 * y] + bh[2 * y + 1] <= in_w &&
                          bv[2 * y + 1] <= g.ksv && bh[2 * y + 1] <= g.ksh;
    const bool monotonic = y == 0 || (bv[2 * y] >= bv[2 * y - 2] &&
                                      bv[2 * y] + bv[2 * y + 1] >= bv[2 * y - 2] + bv[2 * y - 1]);
    if (!in_range || !monotonic)
      return fail(EVT_EINVAL, "resize_plan_create: internal error, tap bounds out of order");
  }
  auto band_bytes = [&](int tr) {
    int64_t worst = 0;
    for (int y0 = 0; y0 < S; y0 += tr) {
      const int y1 = std::min(y0 + tr, S) - 1;
      worst = std::max<int64_t>(worst, (int64_t)(bv[2 * y1] + bv[2 * y1 + 1] - bv[2 * y0]) * lp);
    }
    return worst;
  };
  int tr = std::min(RESIZE_MAX_TR, S);
  while (tr > 1 && band_bytes(tr) > EVT_RESIZE_LDS_BYTES) --tr;
  const int64_t lds = band_bytes(tr);
  if (lds > EVT_RESIZE_LDS_BYTES)
    return fail(EVT_EINVAL, "resize_plan_create: one output row's " + std::to_string(g.ksv) +
                                " vertical taps of " + std::to_string(lp) + " bytes exceed the " +
                                std::to_string(EVT_RESIZE_LDS_BYTES) + "-byte LDS band (reduce "
                                "the image first)");
  evt_resize_plan* p = new (std::nothrow) evt_resize_plan{};
  if (!p) return fail(EVT_ENOMEM, "resize_plan_create: host allocation failed");
  p->in_h = in_h; p->in_w = in_w; p->C = C; p->S = S; p->tr = tr;
  p->nbands = (S + tr - 1) / tr; p->lds = (size_t)lds; p->g = g;
  hipError_t e = hipMalloc((void**)&p->tab, ntab * sizeof(int32_t));
  if (e == hipSuccess) {
    e = hipMemcpy(p->tab, tab.data(), ntab * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) (void)hipFree(p->tab);
  }
  if (e != hipSuccess) {
    delete p;
    return hip_fail(e, "resize_plan_create");
  }
  p->magic = RESIZE_MAGIC;
  *out = p;
  return EVT_OK;
}

int evt_resize_plan_destroy(evt_resize_plan* p) {
  if (!p) return EVT_OK;
  if (p->magic != RESIZE_MAGIC) return fail(EVT_EINVAL, "resize_plan_destroy: not a live plan");
  p->magic = 0;
  const hipError_t e = hipFree(p->tab);
  delete p;
  if (e != hipSuccess) return hip_fail(e, "resize_plan_destroy");
  return EVT_OK;
}

int evt_resize_crop_u8(const evt_resize_item* items, int batch, int channels, int crop,
                       uint8_t* out, void* stream) {
  if (!items || !out) return fail(EVT_EINVAL, "resize_crop_u8: items and out must be non-null");
  if (batch < 0) return fail(EVT_EINVAL, "resize_crop_u8: batch must not be negative");
  if (channels < 1 || channels > 4)
    return fail(EVT_EINVAL, "resize_crop_u8: uint8 images have 1 to 4 channels");
  if (crop < 1 || ((int64_t)crop * channels) % 4)
    return fail(EVT_EINVAL, "resize_crop_u8: crop*channels must be a positive multiple of 4");
  if ((uintptr_t)out & 15) return fail(EVT_EINVAL, "resize_crop_u8: out must be 16-byte aligned");
  for (int b = 0; b < batch; ++b) {
    const evt_resize_item& it = items[b];
    const std::string at = "resize_crop_u8: item " + std::to_string(b);
    if (!it.src || !it.plan) return fail(EVT_EINVAL, at + ": src and plan must be non-null");
    if (it.plan->magic != RESIZE_MAGIC) return fail(EVT_EINVAL, at + ": not a live plan");
    if (it.plan->C != channels)
      return fail(EVT_EINVAL, at + ": the plan has " + std::to_string(it.plan->C) +
                                  " channels, the call " + std::to_string(channels));
    if (it.plan->S != crop)
      return fail(EVT_EINVAL, at + ": the plan's crop is " + std::to_string(it.plan->S) +
                                  ", the call's " + std::to_string(crop));
    if (it.pitch < (int64_t)it.plan->in_w * channels)
      return fail(EVT_EINVAL, at + ": pitch " + std::to_string(it.pitch) + " is less than " +
                                  std::to_string((int64_t)it.plan->in_w * channels) +
                                  " bytes (width*channels)");
  }
  const int64_t per_image = (int64_t)crop * crop * channels;
  for (int b0 = 0; b0 < batch; b0 += RESIZE_CHUNK) {
    ResizeArgs a{};
    a.out = out + (int64_t)b0 * per_image;
    a.S = crop;
    a.n = std::min(RESIZE_CHUNK, batch - b0);
    int blocks = 0;
    size_t lds = 0;
    for (int i = 0; i < a.n; ++i) {
      const evt_resize_item& it = items[b0 + i];
      a.d[i] = ResizeDesc{it.src, it.pitch, it.plan->tab, it.plan->g.ksh, it.plan->g.ksv,
                          it.plan->tr, blocks};
      blocks += it.plan->nbands;
      lds = std::max(lds, it.plan->lds);
    }
    EVT_HIP(resize_crop_launch(a, channels, blocks, lds, (hipStream_t)stream), "resize_crop_u8");
  }
  return EVT_OK;
}

}  // extern "C"
