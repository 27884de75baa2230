// Internal header of the host layer (model.cpp, model_{vit,t2t,swin}.cpp, ops.cpp,
// resize_plan.cpp): the error helpers, the model handle and what the families share.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/evt.h"
#include "evt_internal.h"

#pragma GCC visibility push(hidden)  // the host layer's own: not exported from libevt_hip.so

namespace evt {

int fail(int code, const std::string& msg);  // sets the thread's evt_last_error text
int hip_fail(hipError_t e, const char* what);

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

struct T2TShape {  // what validate_t2t derives from an evt_t2t_desc
  Shape enc;             // encoder geometry (P = (S/16)^2 patches, T = P + 1)
  int grid[3] = {0, 0, 0};
  int din[2] = {0, 0};   // unfolded widths feeding performer 1 / 2
};

struct SwinGeo {  // what validate_swin derives from an evt_swin_desc
  int ns = 0;
  int C[EVT_SWIN_MAX_STAGES] = {}, Cst[EVT_SWIN_MAX_STAGES] = {}, R[EVT_SWIN_MAX_STAGES] = {};
  int mlp[EVT_SWIN_MAX_STAGES] = {}, mst[EVT_SWIN_MAX_STAGES] = {};
  int w[EVT_SWIN_MAX_STAGES] = {};  // window of the stage: min(window_size, R)
  int pd = 0, pdst = 0;  // patch vector width (c, kh, kw) and its K padding
};

bool qkv_headmajor_default();  // EVT_QKV_LAYOUT=token (read when a model is created): false

enum Family : int { FAM_VIT = 0, FAM_T2T = 1, FAM_SWIN = 2 };

// What is fixed once evt_*_create returns: configuration, geometry and the packed weights. Lane
// children (evt_model_set_lanes) copy it, so they share the parent's weight allocations.
struct ModelCore {
  int family = FAM_VIT;      // ViT / ViT_Pruned, T2T-ViT or Swin: the index of family_ops()
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
  int in_chans = 0, image_size = 0;
  int patch_size = 0;        // ViT and Swin
  size_t img_elems = 0;      // fp32 elements of one input image
  evt_vit_desc desc{};       // ViT only
  evt_t2t_desc tdesc{};      // T2T only
  evt_swin_desc sdesc{};     // Swin only
  std::vector<int32_t> heads, head_dim, ffn;
  Shape sh;                  // ViT and T2T: the encoder's geometry
  T2TShape t2t;              // T2T: the token grids S/4, S/8, S/16 and the unfolded widths
  SwinGeo swin;              // Swin: the stages' geometry
  DenseW patch, head1, head2;
  float *cls = nullptr, *pos = nullptr;
  void* pos_h = nullptr;     // bf16 copy of pos (the persistent patch-embedding GEMM's EPI_POS)
  std::vector<Layer> layers;
  // T2T stage
  Performer perf[2];
  DenseW project, head;      // head: LN-folded classifier (final LayerNorm, t2t_vit.py:129,134)
  // Swin
  std::vector<SwinStage> stages;
  // norm_g / norm_b: the final LayerNorm; STANDARD ViT and T2T-ViT keep it too (their heads have
  // it folded into the weights) for the feature outputs; null for a REFERENCE ViT (it has none)
  float *pnorm_g = nullptr, *pnorm_b = nullptr, *norm_g = nullptr, *norm_b = nullptr;
  // evt_model_set_token_schedule (ViT): after block tp_blocks[i] the stream keeps the CLS token and
  // tp_keep[i] patch tokens. The one part of a core that changes after create; lane children get
  // the parent's copy (set_lanes copies the core, set_token_schedule writes every lane)
  std::vector<int32_t> tp_blocks, tp_keep;
  // evt_model_set_skips (ViT; include/evt_depth.h): per block bit 0 = the attention sublayer, bit 1
  // = the FFN sublayer is left out of the forward; empty: none. Changes after create like the
  // schedule, and reaches the lanes the same way
  std::vector<uint8_t> skips;
  uint8_t skip_of(int block) const { return skips.empty() ? 0 : skips[block]; }
  // the last block that runs a sublayer: the CLS tail's block (evt_model_set_skips refuses a mask
  // that skips every block; -1 only for a model of depth 0)
  int last_running() const {
    int i = (int)layers.size() - 1;
    while (i >= 0 && skip_of(i) == 3) --i;
    return i;
  }
  // desc's per-layer arrays live in this core's own vectors (after every copy of a core)
  void bind_desc() {
    desc.heads = heads.data();
    desc.head_dim = head_dim.data();
    desc.ffn = ffn.data();
  }
};

// The buffers a forward writes, filled in by alloc_ws from the family's WsLayout for one handle's
// max_batch and never shared: every lane child has its own. The allocations are owned by
// evt_model::allocs.
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

// Structured gates (include/evt_gates.h) of one packed weight, a block's out-projection (head
// gates) or FC2 (FFN gates): the host-side record and, from the first non-identity gate on, the
// pristine copy of the weight and the device gate vector (both owned through evt_model::allocs)
struct GateRole {
  std::vector<float> rec;  // one gate per head / neuron; empty: never set, all 1
  void* w0 = nullptr;      // [npad][kpad] model dtype: DenseW::w as make_dense packed it
  float* g = nullptr;      // [kpad] fp32: rec expanded over the K columns, 1 in the padding
};
struct LayerGates {
  GateRole head, ffn;
};

}  // namespace evt

struct evt_model : evt::ModelCore {  // a handle: the core, its own workspace, its own runtime state
  evt::Workspace ws;
  size_t ws_bytes = 0;       // what alloc_ws asked for (evt_model_workspace_bytes)
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
  // evt_model_set_head_gates / _ffn_gates: per encoder block, sized at the first set. The parent
  // handle's alone: the lanes read the parent's weight allocations, which the gate kernel rewrites
  std::vector<evt::LayerGates> gates;
  // [max_batch][4] fp32 (1, 0, 1, 1): what evt_forward_block_stats copies out for a skipped
  // sublayer; allocated by the first evt_model_set_skips that skips something
  float* skip_ident = nullptr;
};

namespace evt {

// One per-block output list of a call (taps, maps, head or FFN statistics: validated, strictly
// increasing) and where the forward stands in it. The run functions visit the blocks in order, so
// the block a hook is called for either is the list's next entry or is not in the list.
struct BlockCursor {
  const int32_t* blocks = nullptr;
  float* const* out = nullptr;
  int n = 0, next = 0;
  bool wants(int block) const { return next < n && blocks[next] == block; }
  // block's output pointer, moving on to the next entry, if block is the next entry; else null
  float* take(int block) { return wants(block) ? out[next++] : nullptr; }
  bool last_is(int block) const { return n > 0 && blocks[n - 1] == block; }
  bool reaches(int block) const { return n > 0 && blocks[n - 1] >= block; }  // an entry >= block
};

// The arguments of one forward. The entry points build one and the run functions read it; nothing
// of a call is kept on the handle (hm_layers and tail_mode, which evt_model_qkv_layout and
// evt_model_tail_mode read later, aside).
struct ForwardCall {
  const float* img = nullptr;     // the fp32 batch, or null with
  const uint8_t* img8 = nullptr;  // a uint8 NHWC batch (evt_forward_image) and
  ImgAffine aff{};                // its per-channel affine
  int B = 0;
  float* logits = nullptr;        // may be null in a features forward (no head then)
  // evt_forward_features outputs (null: plain forward): tokens, pooled and tap_norm are read here,
  // the tap list through `taps` (set_feat)
  const evt_features_args* feat = nullptr;
  BlockCursor taps;               // feat's block taps
  BlockCursor maps;               // evt_forward_attention / _window_attention maps, of
  int map_queries = 0;            // EVT_ATTN_CLS or EVT_ATTN_ALL rows
  BlockCursor hstats;             // evt_forward_head_stats blocks
  BlockCursor fstats;             // evt_forward_ffn_stats blocks
  BlockCursor bstats;             // evt_forward_block_stats blocks
  BlockCursor grams;              // evt_forward_grams blocks (out: the Grams), with
  const evt_gram_args* gram = nullptr;  // their `which`, column-sum pointers and scratch
  void set_feat(const evt_features_args* a) {
    feat = a;
    if (a) taps = BlockCursor{a->tap_blocks, a->taps, a->n_taps};
  }
  const evt_rollout_args* rollout = nullptr;  // evt_forward_rollout (null: none)
  const evt_token_pruning_args* tprune = nullptr;  // evt_forward_token_pruning exports (null: none)
  int tprune_next = 0;            // the next entry of the handle's token schedule
  int T = 0;                      // tokens per image of the stream run_encoder left (0: sh.T)
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

// One buffer of a handle's workspace. A family's layout function lists them in allocation order;
// alloc_ws makes one dev_alloc per entry and the *_query_workspace calls sum the same list.
struct WsBuf {
  size_t member;               // offsetof(Workspace, the pointer it fills)
  size_t bytes;
  size_t zeroed = 0;           // leading bytes zeroed once at allocation
  const char* what = nullptr;  // the memset's name in an error
};
struct WsLayout {
  std::vector<WsBuf> bufs;
  size_t hbuf_bytes = 0;       // Workspace::hbuf_bytes
  int qa_ld = 0, qh_ld = 0;    // Workspace::qa_ld / qh_ld (MX8)
  bool patch_in_hbuf = false;  // ws.apatch = ws.hbuf (ViT)
  size_t bytes() const {
    size_t n = 0;
    for (const WsBuf& b : bufs) n += b.bytes;
    return n;
  }
};
#define EVT_WS(member) offsetof(Workspace, member)
// The encoder's token-stream buffers for B images (ViT and T2T-ViT), appended to *l
void encoder_ws(const Shape& sh, int dtype, bool mx8, int B, size_t hbuf_bytes, WsLayout* l);

// What differs between the model families; family_ops() looks a handle's up by ModelCore::family
struct FamilyOps {
  WsLayout (*workspace)(const ModelCore&, int B);  // the buffers of a handle for B images
  int (*run)(evt_model*, ForwardCall&);  // the forward of call.B images on m's own workspace
  int (*blocks)(const ModelCore&);       // blocks a feature tap can name
  // tokens and width of block's output (block < 0: of the final token map)
  void (*shape)(const ModelCore&, int block, int* tokens, int* width);
  const char* no_attn_maps;              // why evt_forward_attention refuses the family, or null
};
const FamilyOps& vit_ops();   // model_vit.cpp
const FamilyOps& t2t_ops();   // model_t2t.cpp
const FamilyOps& swin_ops();  // model_swin.cpp
const FamilyOps& family_ops(const ModelCore& m);
int encoder_blocks(const ModelCore& m);  // FamilyOps::blocks / shape of the encoder families
void encoder_shape(const ModelCore& m, int block, int* tokens, int* width);

// ---- model.cpp ----
void prof_reset(evt_model* m);
// add algorithmic work (flops, bytes) to the innermost open ProfScope of a profiled forward
void prof_work(const evt_model* m, double flops, double bytes);
int dev_alloc(evt_model* m, void** p, size_t bytes);
// m's workspace for B images: the family's layout, buffer by buffer (lanes allocate their own)
int alloc_ws(evt_model* m, int B, hipStream_t s);
int make_dense(evt_model* m, DenseW* dw, const float* W, const float* bias, int K, int N,
               hipStream_t s, const float* ln_g = nullptr, const float* ln_b = nullptr);
int copy_vec(evt_model* m, float** dst, const float* src, size_t n, hipStream_t s);
int make_mx8(evt_model* m, Mx8W* dw, const float* W, const float* bias, int K, int N,
             hipStream_t s);
// The operand, shape, bias / residual / position fields of a Dense launch and the vector-epilogue
// rule (vec_ok) that follows from them; everything else is the caller's
GemmParams gemm_operands(const void* A, int64_t lda, const void* W, int Kpad, int Npad, void* C,
                         int64_t ldc, int M, int N, const float* bias, const void* resid,
                         int64_t ldr, const float* pos, int64_t ldp, int P);
void dense_work(const evt_model* m, const DenseW& w, const DenseCall& c);
GemmParams dense_params(const evt_model* m, const DenseW& w, const DenseCall& c);
int dense(const evt_model* m, const DenseW& w, const DenseCall& c, hipStream_t s);
int dense_mx8(const Mx8W& w, int flags, const void* A, int64_t lda, const uint32_t* as, void* C,
              int64_t ldc, uint32_t* cs, int M, const void* resid, int64_t ldr, hipStream_t s,
              const float* rstats = nullptr, const float* rgamma = nullptr,
              const float* rbeta = nullptr);
int feat_export(evt_model* m, const void* x, int64_t ldx, int64_t row_step, float* out, bool norm,
                int rows, int D, hipStream_t s);
int feat_tap(evt_model* m, ForwardCall& call, int block, int64_t ldx, int rows, int D);
int attn_map(evt_model* m, ForwardCall& call, int block, const AttnParams& ap);
// evt_forward_head_stats: block's statistics, if the call asks for them next (beside attn_map)
int head_stats(evt_model* m, ForwardCall& call, int block, const AttnParams& ap);
// evt_forward_ffn_stats: block's neuron statistics of the `rows` hidden rows the full-row FC1 left in
// ws.hbuf, if the call asks for them next (between FC1 and FC2)
int ffn_stats(evt_model* m, ForwardCall& call, int block, const Layer& L, int rows);
// evt_forward_grams: the Gram and column sums of the `rows` rows of `a` (pitch ld, `width` columns:
// ws.hbuf after the full-row FC1 for `which` EVT_GRAM_FFN, ws.o after the attention kernel for
// EVT_GRAM_ATTN), if the call asks for Grams of that kind and for the block next
int gram_hook(evt_model* m, ForwardCall& call, int block, int which, const void* a, int64_t ld,
              int rows, int width);
// evt_forward_block_stats: sublayer `sub` (0 attention, 1 FFN) of block `block`, if the call asks
// for the block next: the statistics of the stream rows b against a (T tokens per image), or with
// a == nullptr the identity values of a skipped sublayer. sub == 1 moves the cursor on.
int block_stats(evt_model* m, ForwardCall& call, int block, int sub, const void* a, const void* b,
                int T);
// evt_forward_rollout: block's head mean and rollout step, from the call's start block on
int rollout_step(evt_model* m, ForwardCall& call, int block, const AttnParams& ap);
// Token pruning (include/evt_token_pruning.h). tokens_at: T_l of block `block` under m's schedule.
// no_token_schedule: EVT_EINVAL naming the schedule if m has one (`what` reads all T tokens).
int tokens_at(const ModelCore& m, int block);
int no_token_schedule(const evt_model* m, const char* what);
// evt_forward_window_attention (Swin): block's window map, if the call asks for it next
int window_attn_map(evt_model* m, ForwardCall& call, int block, int w, const SwinAttnParams& ap);
int finish_create(evt_model* m, int rc, evt_model** out);
int check_batch(const evt_model* m, int B);
int forward(evt_model* m, ForwardCall& call, bool use_lanes);
int family_forward(evt_model* m, int family, const char* wrong_family, const float* img, int B,
                   float* logits, void* stream);
// the per-channel affine of a uint8 image input (evt_forward_image, evt_patchify_u8, evt_unfold_u8)
int affine_from(const float* scale, const float* shift, int C, ImgAffine* aff, const char* what);

// ---- encoder.cpp (ViT and T2T-ViT) ----
int build_encoder(evt_model* m, const float* const* w, hipStream_t s);
int dense_head(const evt_model* m, const DenseW& w, const DenseCall& c, hipStream_t s);
int run_encoder(evt_model* m, ForwardCall& call);
int run_encoder_mx8(evt_model* m, ForwardCall& call);
int encoder_features(evt_model* m, const ForwardCall& call);

// ---- ops.cpp ----
// What evt_classify checks of its arguments (the logits pointer aside); evt_forward_classify
// shares it. Fills the launch parameters.
int validate_classify(const evt_classify_args* a, int B, int C, int64_t ldl, ClassifyParams* p);

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

}  // namespace evt

#pragma GCC visibility pop
