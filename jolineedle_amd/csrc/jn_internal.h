// Internal structures of libjnroll.so (host side).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../include/jnroll.h"
#include "jn_kernels.h"

namespace jnr {

void set_error(const char* fmt, ...);

#define JN_HIP(call)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) {                                                               \
      jnr::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      return JN_EHIP;                                                                     \
    }                                                                                     \
  } while (0)

#define JN_CHECK(cond, code, ...)   \
  do {                              \
    if (!(cond)) {                  \
      jnr::set_error(__VA_ARGS__);   \
      return (code);                \
    }                               \
  } while (0)

// ---- activation buffers: NHWC fp32, per-image size known at plan time --------------
struct Buf {
  int H = 0, W = 0, C = 0;          // C = channel stride of a pixel (ld)
  size_t per_image() const { return (size_t)H * W * C; }
};

// A channel slice of a buffer.
struct View {
  int buf = -1;
  int H = 0, W = 0;
  int C = 0;      // channels in the view
  int coff = 0;   // first channel inside the buffer
};

enum OpKind {
  OP_STEM = 0,      // Focus + dense 3x3 (== 6x6 stride-2 on the image) + bias + SiLU
  OP_PW,            // 1x1 conv  (GEMM)   + bias + act (+ residual)
  OP_DW,            // depthwise 3x3 s1/s2 + bias + SiLU
  OP_CONV3,         // dense 3x3 s1/s2    + bias + SiLU       (non-depthwise models)
  OP_SPP,           // maxpool 5/9/13 of slice 0 into slices 1..3
  OP_UPSAMPLE,      // nearest x2 (raw values) into a slice
  OP_ADDACT,        // bottleneck shortcut: out = act(in) + act(res), materialised
  OP_PRED,          // YOLOXHead predictors of one level + decode (in = reg_feat, res = cls_feat)
};

struct Op {
  OpKind kind;
  View in, out;
  View res;                 // OP_ADDACT: the shortcut input (buf = -1: none)
  View alias;               // conv: second view that receives this layer's (scale, shift) (upsampled copy)
  int stride = 1;
  int act = ACT_SILU;
  int wslot = -1;           // index into Net::convs (packed weights)
  int level = 0, anchor0 = 0;   // OP_PRED
  bool acc_in = false;      // backward: add into g[in] (another consumer, later in forward order, wrote it first)
  bool acc_res = false;     // backward: same for g[res]
  std::string name;         // module prefix, e.g. "backbone.dark2.0.dconv"
};

// Packed (device) weights of one conv layer.
struct ConvW {
  std::string prefix;       // "<...>.conv" / "<...>.bn" live under this module prefix
  // Two 1x1 BaseConvs that read the same input (CSPLayer.conv2 and .conv1) run as ONE conv of cout channels:
  // rows [0, cout_first) belong to `prefix`, the rest to `prefix2`; their tensors are stored back to back.
  std::string prefix2;
  int cout_first = 0;
  int cin = 0, cout = 0, k = 1, groups = 1;
  bool has_bn = true;       // BaseConv; false = plain Conv2d with optional bias
  bool has_bias = false;    // plain Conv2d bias
  float* w_dev = nullptr;   // raw conv weight, layout depends on the op (see pack_conv)
  void* w_bf16 = nullptr;   // dense 3x3 in bf16 inference mode: the same [tap][N][K] layout pre-rounded to bf16
  float* b_dev = nullptr;   // [cout] bias of a BN-free Conv2d (else null)
  float *gamma_dev = nullptr, *beta_dev = nullptr;     // BN affine
  float *rmean_dev = nullptr, *rvar_dev = nullptr;     // BN running statistics (updated in train mode)
  int stat_off = 0;         // first channel of this layer in the per-slot stats / save arrays
};

struct Net {
  std::string prefix;       // "gpt_backbone." or "yolox.backbone."
  bool depthwise = false;
  float depth = 0, width = 0;
  int P = 0;
  std::vector<Buf> bufs;
  std::vector<Op> ops;
  std::vector<ConvW> convs;
  View fpn[3];              // pan_out2, pan_out1, pan_out0
  int n_backbone_ops = -1;  // ops before the detection head (-1: no head, all ops)
  size_t x3_lo = 0, x3_hi = 0;   // arena range of the 1x1 weights (multiples of 8 floats; hi == 0: not computed yet)
  bool x3_dirty = true;           // the bf16 planes of that range are older than the parameters (see mark_params_written)
  X3FragConv* x3_frag = nullptr;  // device table of the 1x1 convs whose planes are kept in fragment order (pw_x3_fragment_order)
  int x3_frag_n = 0, x3_frag_max = 0;   // its rows, the largest cout * cin among them
  int n_anchors = 0, head_hid = 0;
  float* pred_w[3] = {nullptr, nullptr, nullptr};   // [6][hid] reg(4), obj, cls predictor rows
  float* pred_b[3] = {nullptr, nullptr, nullptr};   // [6]
  size_t per_image_floats = 0;
  std::vector<size_t> buf_off;    // per-image offset of each buffer (floats)
  std::vector<int> tab_off;       // first table channel of each buffer
  int tab_channels = 0;           // sum of buffer channels (table length)
  int stat_channels = 0;          // sum of BN channels
  // workspace slots: slot 0 = eval / single-step; slots 1..n = one per glimpse step when training.  The small per-step
  // state (tab / save / stats) has n_slots slots, the activations a_slots: the two counts are equal, and a step's
  // activation slot is its table slot, unless a train-mode rollout runs under jn_set_activation_slots, which keeps a
  // ring of activation slots and replays a step's forward before its backward (run_net's replay mode)
  int n_slots = 0;
  int a_slots = 0;
  int act_dtype = 0;              // JN_F32 / JN_BF16 storage of the activation buffers
  char* act = nullptr;            // [a_slots][per_image_floats * max_batch] elements of act_dtype
  float* tab = nullptr;           // [n_slots][3][tab_channels]
  float* save = nullptr;          // [n_slots][2 * stat_channels]  (mean, invstd)
  double* stats = nullptr;        // [n_slots][2 * stat_channels]  (sum, sumsq)
  double* stats_sink = nullptr;   // one slot of sums nobody reads: where the producers of a replayed pass add theirs
  int g_slots = 0;                // slots of the three gradient-side buffers below (backward is step-batched)
  float* gact = nullptr;          // [g_slots] gradient buffers: mirror of one `act` slot each
  double* bred = nullptr;         // [g_slots][JN_NREP][2 * stat_channels] backward reductions (sum g_y, sum g_y * zhat)
  float* bconsts = nullptr;       // [g_slots][3 * stat_channels] per-channel backward constants
  bool eval_tab_dirty = true;     // slot-0 table must be rebuilt from the running statistics
  // deferred BatchNorm tables (ChanTab in jn_kernels.h): per table channel / per BatchNorm channel descriptors
  bool defer_ok = false, defer_built = false;
  int *td_src = nullptr, *td_goff = nullptr, *td_boff = nullptr; float* td_hw = nullptr;      // [tab_channels]
  float* fd_hw = nullptr; int *fd_goff = nullptr, *fd_boff = nullptr, *fd_t0 = nullptr, *fd_t1 = nullptr;   // [stat_channels]
  float **fd_rm = nullptr, **fd_rv = nullptr;
  std::vector<float> h_td_hw;     // host copies of the per-table-channel descriptors (td_hw: 0 where td_src < 0)
  std::vector<int> h_td_src, h_td_goff, h_td_boff;
};

// ---- backward plan (plan.cpp: plan_backward): the route of every op of the conv-stack backward --------------
enum BwdRoute {
  BR_NONE = 0,
  BR_PW_FUSED, BR_PW_FUSED_HALVES,        // pw_bwd_fused_kernel over the whole 1x1 conv / the two halves of a merged pair
  BR_DW_FUSED, BR_STEM_FUSED,             // dw_bwd_fused_kernel, the stem's weight gradient with bn_bwd_gz inside
  BR_PW, BR_DW, BR_CONV3_S1, BR_CONV3_S2,   // bn_bwd_gz, then separate data / weight gradients
  BR_ADDACT_COPY, BR_ADDACT_FOLD,         // shortcut add: g[res] (+)= g[sum] by a copy / inside the fold conv's kernel
  BR_SPP, BR_UPSAMPLE,
};
struct BwdStep {           // op indices only: the launcher turns them into pointers
  BwdRoute route = BR_NONE;
  View g;                  // conv: the gradient view it reads (a shortcut sum's, in place, when the conv feeds the add)
  int red_by = 0;          // BN conv: bit h = a consumer forms the sums of half h of a merged pair (bit 0: of the conv)
  // fused consumer: its epilogue forms the BN sums of input channels [0, red_split or cin) for op red_in and of the
  // rest for op red_in2 (-1: none); half -1 = the whole conv, 0 / 1 = a half of a merged pair.  red2: the run of red_in
  // is a shortcut sum and red_in the conv behind it (whose z and table replace the input's)
  int red_in = -1, red_half = -1, red_in2 = -1, red_half2 = -1, red_split = 0;
  bool red2 = false;
  int fold = -1;           // 1x1 conv: the shortcut add whose copy of g[sum] into g[in] its kernel absorbs
};
int plan_backward(const Net& net, bool with_head, int fpn_zero, std::vector<BwdStep>& plan);

// ---- forward plan (plan.cpp: plan_forward): the route of every op of one conv-stack forward pass ---------------------
enum FwdRoute {
  FR_NONE = 0,
  FR_STEM, FR_CONV,              // launch_stem; launch_pw / launch_dw / launch_conv3 by the op's kind
  FR_DWPW, FR_DWPW_ADD,          // eval DWConv (depthwise + pointwise) in one kernel; with the bottleneck's shortcut add
  FR_ABSORBED,                   // nothing to launch: the kernel of op `link` covers this op
  FR_SPP, FR_UPSAMPLE, FR_ADDACT, FR_PRED,
};
struct FwdStep {           // op indices and flags only: the launcher turns them into pointers
  FwdRoute route = FR_NONE;
  // FR_ABSORBED: the op whose kernel covers this one.  FR_DWPW / FR_DWPW_ADD: the pointwise op.  FR_CONV of an fp32 1x1
  // conv: the upsample whose copy its kernel MAY write (the launcher asks pw_fuses_upsample of its route).  -1: none
  int link = -1;
  int add = -1;            // FR_DWPW_ADD: the shortcut add
  bool deferred = false;   // BatchNorm conv: no finalize launch of its own, its consumers read the batch sums
};
bool defer_eligible(const Net& net);   // the net's train-mode passes without the head may defer BatchNorm tables
// plan[i] belongs to op first_op + i; defer: this pass defers (train && !with_head && defer_eligible && its tables exist)
int plan_forward(const Net& net, int N, bool train, bool with_head, int first_op, bool defer, std::vector<FwdStep>& plan);

struct ParamEntry {
  jn_param_info info;
};
// one row of the state-dict table (plan.cpp)
void add_param(std::vector<ParamEntry>& params, const std::string& name, std::initializer_list<int64_t> shape, int dtype,
               bool buffer, bool used);

// One trainable tensor inside the flat parameter arena.
struct ParamSeg {
  std::string name;          // the reference's state-dict name
  int kind = 0, d0 = 0, d1 = 0, d2 = 0;   // packing (api_ctx.hip: PackKind) and its dimensions
  size_t off = 0, numel = 0;
};

struct GptW {   // device, packed
  float *wte = nullptr, *wpe = nullptr, *embed_class = nullptr;
  float *proj_wt = nullptr, *proj_b = nullptr;          // project_concat: Wt [n_in][C]
  float *pos1d = nullptr;                                // [T+1][C] 1-D sinusoid table
  float *pos2d_col = nullptr, *pos2d_row = nullptr;      // [256][ch2] tables (column / row halves)
  float *efpn_w = nullptr;                               // embed_fpn.0 weight [C][cin]
  float *efpn_lin_wt = nullptr, *efpn_lin_b = nullptr;   // embed_fpn.3: Wt [(h*w)*C + c][C]
  float *head_wt = nullptr;                              // [C][nA]
  float *lnf_w = nullptr, *lnf_b = nullptr;
  struct Layer {
    float *ln1_w, *ln1_b, *qkv_wt, *qkv_b, *proj_wt, *proj_b, *ln2_w, *ln2_b, *fc_wt, *fc_b, *fc2_wt, *fc2_b;
  };
  std::vector<Layer> layers;
};

struct EnvState {
  bool ready = false;
  const void* images = nullptr;   // [B,3,H,W] fp32, or uint8 when images_u8 (byte b = b / 255): not copied
  int images_u8 = 0;
  int B = 0, H = 0, W = 0, nb = 0, Gh = 0, Gw = 0, T = 0, stop = 0;
  int64_t* positions = nullptr;   // [B,2]
  uint8_t* bbox_masks = nullptr;  // [B,Gh,Gw]
  uint8_t* visited = nullptr;     // [B,Gh,Gw]
  int32_t* steps = nullptr;       // [B]
  uint8_t* has_stopped = nullptr; // [B]
  int32_t* n_bbox_tiles = nullptr;// [B] sum(bbox_masks)
  // view mode (jn_env_init_views): `images` is null and H x W is the logical canvas; the patches of a glimpse step are
  // gathered through the views into column `col` of the staging stack, which the encoders then read as plain patches
  bool view_mode = false;
  jn_image_view* views = nullptr; // [B] device copy of the table (capacity max_batch)
  void* stage = nullptr;          // [stage_cols][B][3][P][P] in the sources' element type (images_u8); hipMalloc / hipFree
  size_t stage_bytes = 0;
  int stage_cols = 0;             // columns in use: T + 1 when a later pass reads them again, else 1
  int64_t* stage_pos = nullptr;   // [block_size + 1][B][2] = (3 B t, 0): "position" of column t's first patch in units of P rows
  int stage_pos_B = 0;            // the B that table was written for
  // ragged mode (jn_env_init_ragged): view mode plus a per-agent grid extent; the table is allocated by the first
  // ragged init, so that an env that never uses it allocates what it always did
  bool ragged = false;
  int32_t* extent = nullptr;      // [max_batch][2] = (gh, gw)
};

// A per-agent host table behind a rollout switch (jn_set_rollout_keys, jn_set_rollout_classes): the context's own copy
// of the caller's [rows][Width] values, armed while it is not empty, and its device twin, which the next rollout
// uploads on its own stream when the copy has changed.  The one ordering rule: `ev` sits behind the most recent upload,
// and set() waits for it before it rewrites the copy, which that asynchronous upload may still be reading (no event
// exists before the first armed rollout).
template <typename T, int Width = 1>
struct AgentTable {
  std::vector<T> host; T* dev = nullptr; size_t dev_rows = 0; bool dirty = false;
  hipEvent_t ev = nullptr;

  bool armed() const { return !host.empty(); }
  int rows() const { return (int)(host.size() / Width); }
  void clear() { host.clear(); }
  int set(const T* values, size_t n_rows) {
    if (ev) JN_HIP(hipEventSynchronize(ev));
    host.assign(values, values + n_rows * Width);
    dirty = true;
    return JN_OK;
  }
  // *dev_out = the device table holding the armed rows (at least min_rows of capacity), or null when not armed
  int upload(jn_ctx* ctx, int min_rows, hipStream_t s, const T** dev_out);
  AgentTable() = default;
  AgentTable(const AgentTable&) = delete;      // owns `ev`
  ~AgentTable() { if (ev) (void)hipEventDestroy(ev); }
};

}  // namespace jnr

struct jn_ctx {
  jn_config cfg;
  std::vector<jnr::ParamEntry> params_tab;
  const std::vector<jnr::ParamEntry>& params_table() const { return params_tab; }
  // flat trainable-parameter arena + gradient / AdamW mirrors
  float* params = nullptr; float* grads = nullptr; float* adam_m = nullptr; float* adam_v = nullptr;
  uint16_t* params_x3 = nullptr;   // 3 bf16 per arena float: the 1x1 weights split for pw_x3_kernel (refreshed at the start of every fp32 pass)
  uint16_t* params_x3t = nullptr;  // the TRANSPOSED 1x1 weights of the wide layers as three bf16 planes (data gradient, split per backward)
  size_t arena_size = 0, arena_used = 0, gpt_arena_end = 0;   // [0, gpt_arena_end) = optim_gpt parameters
  int adam_step = 0, adam_step_yolox = 0;
  bool freeze_det_backbone = false;   // --freeze-image-processor: yolox.backbone.* keep their values (src/models/gpt.py:264-268)
  size_t det_head_begin = 0;          // arena offset of the first yolox.head.* tensor
  jnr::GptLayerPtrs* g_layers_dev = nullptr;
  float* efpn_train = nullptr;    // [T][B][h*w*C] embed_fpn.0 activations of every glimpse step
  float* tok_emb_train = nullptr; // [B][T][C] patch embeddings of every glimpse step
  float* d_tok_emb = nullptr;     // [B][T][C] their gradients
  float* dlogits = nullptr;       // [B][T][nA]
  float* de_ws = nullptr;         // [B][h*w*C] gradient of embed_fpn.0 activations (one step)
  float* sup_final_emb = nullptr; float* sup_logits = nullptr;   // supervised step: [B][T+1][C], [B][T][nA]
  float* gpt_bwd_scratch = nullptr; size_t gpt_bwd_scratch_floats = 0;
  std::vector<jnr::ParamSeg> segs;
  std::map<std::string, int> seg_index;
  jnr::Net nets[2];                // [JN_NET_GPT_BACKBONE], [JN_NET_DETECTOR]
  bool has_net[2] = {false, false};
  int enc_net = 0;                // which net encodes patches for the GPT
  jnr::GptW gpt;
  int efpn_cin = 0, efpn_h = 0, efpn_w = 0;
  bool weights_loaded = false;
  std::vector<void*> owned;       // device allocations to free
  jnr::GptLayerPtrs* layers_dev = nullptr;
  std::vector<jnr::GptLayerPtrs> layers_host;   // the same table on the host (the wide route launches per layer)
  int decision_route = 0;         // 0: gpt_step_kernel, one workgroup per agent; 1: the wide route (kernels_gptwide.hip)
  float* wide_scratch = nullptr;  // gpt_wide_scratch_floats(n_embd, n_parts, max_batch) floats of a wide context
  float* emb_part = nullptr;      // [B][KS][C] split-K partials of embed_fpn.3
  int KS = 8;
  int32_t* found = nullptr;       // [B] visited bbox tiles
  float* ident = nullptr;         // identity table (scale 1, shift 0, flag 0) for gradient operands
  float* wpart = nullptr;         // [JN_NREP][JN_WPART_MAX] replicated weight-gradient partials (kept zero)
  // second stream of the conv-stack backward: the wide 1x1 weight-gradient GEMMs run beside the data-gradient GEMMs
  hipStream_t aux_stream = nullptr; hipEvent_t aux_fork = nullptr, aux_join = nullptr;
  bool stats_prezeroed = false;   // run_net(train): the caller already zeroed the BN sums of the slots it walks
  int64_t* det_pos = nullptr; size_t det_pos_cap = 0;   // [T+1][B][2] per-step position snapshots for the detector stream
  float* det_raw = nullptr;       // [B][A][6] decoded head output
  float* det_logits = nullptr;    // [B][A][6] raw predictor outputs of the training pass (consumed by the loss kernel)
  // one entry per resident detector training pass (jn_detector_forward ... jn_detector_backward, api_det.hip)
  struct DetPass {
    float* dlogits = nullptr;     // [B][A][6] d loss / d raw (before the 1 / num_fg factor)
    float* acc = nullptr;         // [8] scale (scale[0] = loss_scale / max(num_fg, 1)), then [max_batch][8] per-patch loss sums
    const float* patches = nullptr; int N = 0;   // caller-owned input of the pass (the stem's weight gradient reads it)
    bool valid = false;           // cleared by every pass over the same workspace slot and by the backward
  };
  std::vector<DetPass> det_pass;
  float* det_bwd_scale = nullptr; // [1] scale of the backward in flight: forward scale x upstream d loss x chunk weight
  float* det_labels = nullptr;    // [B][nb][5] cxcywh labels of the training pass
  size_t det_labels_rows = 0;
  float* det_tmp_boxes = nullptr; int32_t* det_tmp_counts = nullptr;   // one step's detections before the scatter
  float* tok_emb = nullptr;       // [B][T][C] patch embeddings of jn_gpt_forward / jn_supervised_eval
  float* eval_logits = nullptr;   // [B][T][nA] logits of jn_supervised_eval when the caller wants none
  float* det_eval_dlogits = nullptr; float* det_eval_acc = nullptr;   // jn_detector_eval_loss: the loss kernel's d_raw / sums (unused)
  jnr::EnvState env;
  // rollout workspaces
  float* patch_emb = nullptr;     // [B, C]
  float* efpn_act = nullptr;      // [B, h*w, C]
  float* kcache = nullptr;        // [L][B][T+1][C]
  float* vcache = nullptr;
  float* logits_ws = nullptr;     // [B, nA]
  int32_t* n_done = nullptr;      // [T+1] number of finished envs after step t (index t+1)
  int32_t* n_done_host = nullptr; // pinned copy of n_done (rollout_steps_begin / _end); n_done_host_n ints
  int n_done_host_n = 0;
  hipEvent_t steps_ev = nullptr;  // behind that copy
  int64_t* prev_action = nullptr; // [B]
  int32_t* cache_len = nullptr;   // [B]
  int last_T = 0;
  bool last_stop_early = true;
  bool pos_by_token = false;      // jn_set_rollout_positions: the token of step t gets 1-D position t (eval rollouts only)
  bool det_all = false;           // jn_set_det_candidates: every passing anchor reaches the NMS (launch_postprocess_all)
  bool det_loss_all = false;      // jn_set_det_loss_boxes: targets wider than 8 rows go to launch_yolox_loss_wide
  // jn_set_rollout_teacher: armed while teacher_sets is set; caller-owned [B,T] bytes and [B,Gh,Gw] grid (null = bbox_masks)
  uint8_t* teacher_sets = nullptr; const uint8_t* teacher_targets = nullptr;
  // jn_set_rollout_keys: the [n][2] = (stream seed, stream index) table; jn_set_rollout_classes: the class id behind
  // every agent's class token.  A train-mode rollout leaves the ids it ran with in classes_used (its own device copy,
  // like drop_seed_used: the backward runs after the caller has cleared or rewritten the table); classes_used_n = 0: it
  // ran without a table (class 0)
  jnr::AgentTable<uint64_t, 2> keys; jnr::AgentTable<int64_t> classes;
  int64_t* classes_used = nullptr; size_t classes_used_cap = 0; int classes_used_n = 0;
  // jn_set_rollout_action_mask: the armed policy and the caller's [B,T] buffer (or null); mask_sets: the context's own
  // uint16 [max_batch][block_size] sets of the most recent masked rollout (allocated by the first one); train_mask_policy:
  // the policy the most recent train-mode rollout ran under (0: its loss and backward are the unmasked ones)
  int mask_policy = 0, train_mask_policy = 0; uint16_t* mask_sets_out = nullptr; uint16_t* mask_sets = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool profiling = false;
  bool bwd_timed = false;         // ev[2] / ev[3] bracket a conv-stack backward
  float pdrop = 0.0f;             // --dropout (embd / attn / resid), train-mode passes only (jn_set_dropout)
  uint64_t drop_seed = 0, drop_ctr = 0, drop_seed_used = 0;   // seed of the NEXT / the most recent train-mode forward
  jn_rollout_out train_out{};     // output buffers of the most recent train-mode rollout (jn_reinforce_backward reads them)
  bool train_out_valid = false;   // cleared by every entry point that overwrites what jn_reinforce_backward reads
  // jn_set_activation_slots: act_ring = the setting (0: one activation slot per glimpse step); train_ring = the ring the
  // most recent train-mode rollout ran under (0: all its steps resident); replayed_steps: of the most recent backward
  int act_ring = 0, train_ring = 0, replayed_steps = 0;
  // supervised autograd bridge: inputs of the most recent supervised forward (caller-owned, alive until the backward)
  struct SupState { const float* patches; const int64_t* actions; const int64_t* positions; const int64_t* classes; int B, T; } sup{};
  bool sup_valid = false;         // cleared by every pass over workspace slot 0 of the patch encoder
  jnr::ArenaSeg* segs_dev = nullptr; int segs_dev_n = 0;   // device copy of `segs` for the layout-conversion kernel
  std::vector<hipEvent_t> conv_ev;   // pairs per step when profiling
  int conv_ev_used = 0;
};

// ---- host helpers that cross the api_*.hip units (each defined in the unit its heading names) ----------------------
namespace jnr {

// where a stem reads its patches: plain patches (positions = null) or windows of whole images at `positions`
struct StemSrc {
  const void* src; const int64_t* positions; long long sample_stride, chan_stride; int row_stride;
  int pos_stride = 2;
  int src_u8 = 0;     // src holds uint8 (the env's byte images): StemArgs::src_u8
};

template <typename T>
int dev_alloc(jn_ctx* ctx, T** out, size_t count) {
  void* p = nullptr;
  if (count == 0) count = 1;
  hipError_t e = hipMalloc(&p, count * sizeof(T));
  if (e != hipSuccess) {
    set_error("hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
    return JN_ENOMEM;
  }
  ctx->owned.push_back(p);
  *out = (T*)p;
  return JN_OK;
}

template <typename T, int Width>
int AgentTable<T, Width>::upload(jn_ctx* ctx, int min_rows, hipStream_t s, const T** dev_out) {
  *dev_out = nullptr;
  if (!armed()) return JN_OK;
  const size_t n = (size_t)rows();
  if (dev_rows < n) {
    const size_t want = std::max((size_t)min_rows, n);
    int rc = dev_alloc(ctx, &dev, want * Width);
    if (rc) return rc;
    dev_rows = want;
    dirty = true;
  }
  if (dirty) {
    if (!ev) JN_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    JN_HIP(hipMemcpyAsync(dev, host.data(), n * Width * sizeof(T), hipMemcpyHostToDevice, s));
    JN_HIP(hipEventRecord(ev, s));
    dirty = false;
  }
  *dev_out = dev;
  return JN_OK;
}

// workspace slots.  Activation buffers are stored as net.act_dtype (JN_F32: 4-byte, JN_BF16: 2-byte elements).
// view_ptr takes an ACTIVATION slot (< net.a_slots); view_tab, slot_save and slot_stats take a TABLE slot (< net.n_slots).
inline size_t act_esz(const Net& net) { return net.act_dtype == JN_BF16 ? 2 : 4; }
inline void* view_ptr(const Net& net, int slot, int max_batch, const View& v) {
  const size_t elem = (size_t)slot * net.per_image_floats * max_batch + net.buf_off[v.buf] * (size_t)max_batch + v.coff;
  return reinterpret_cast<char*>(net.act) + elem * act_esz(net);
}
inline ChanTab view_tab(const Net& net, int slot, const View& v) {
  float* t = net.tab + (size_t)slot * 3 * net.tab_channels + net.tab_off[v.buf] + v.coff;
  return ChanTab{t, t + net.tab_channels, t + 2 * net.tab_channels};
}
inline double* slot_stats(const Net& net, int slot) { return net.stats + (size_t)slot * JN_NREP * 2 * net.stat_channels; }
inline float* slot_save(const Net& net, int slot) { return net.save + (size_t)slot * 2 * net.stat_channels; }
inline float* grad_of(const jn_ctx* ctx, const float* param) { return ctx->grads + (param - ctx->params); }

// api_ctx.hip
int dev_upload(jn_ctx* ctx, float** out, const std::vector<float>& host);
int n_parts(const jn_config& c);
// api_net.hip
StemSrc patch_src(const void* ptr, int P, long long sample_stride = 0);
int ensure_slots(jn_ctx* ctx, Net& net, int n_slots, int a_slots = -1);   // a_slots < 0: as many as n_slots
int refresh_eval_table(jn_ctx* ctx, Net& net, hipStream_t s);
void mark_params_written(jn_ctx* ctx);
// tab_slot < 0: the pass's table slot is its activation slot `slot`
enum RunMode { RUN_PASS = 0, RUN_REPLAY = 1 };
int run_net(jn_ctx* ctx, int ni, int N, const StemSrc& ss, int slot, int train, const int* skip_flag, int skip_when,
            hipStream_t s, bool with_head = false, int first_op = 0, int tab_slot = -1, RunMode mode = RUN_PASS);
int ensure_train_state(jn_ctx* ctx, int g_slots = 1);
int ensure_aux_stream(jn_ctx* ctx);
int run_net_backward(jn_ctx* ctx, int ni, int N, const StemSrc& ss, int slot, hipStream_t s, int nsl = 1,
                     long long pos_slot_stride = 0, bool with_head = false, int fpn_zero = 0, int tab_slot = -1);
int run_embed_fpn(jn_ctx* ctx, int N, int slot, float* e_buf, const int* skip_flag, int skip_when, hipStream_t s, int tab_slot = -1);
int replay_slot_diff(jn_ctx* ctx, Net& net, int slot_a, int slot_b, int N, long long* n_diff, hipStream_t s);
int embed_tokens(jn_ctx* ctx, const StemSrc& ss, int N, int train, float* e_buf, float* out, long long out_stride,
                 hipStream_t s);
// api_det.hip
int det_slot_base(const jn_ctx* ctx);
int detect_impl(jn_ctx* ctx, const StemSrc& ss, int N, float* boxes_dev, int32_t* counts_dev, float* raw_dev,
                const int* skip_flag, int skip_when, hipStream_t s);
// api_env.hip
EnvPtrs env_ptrs(jn_ctx* ctx);
void env_gather(const EnvState& e, float* out, long long out_sample_stride, int P, const int* skip_flag, int skip_when,
                hipStream_t s);
StemSrc env_stem_src(const EnvState& e, const int64_t* positions);
int ensure_stage(jn_ctx* ctx, int cols);
void stage_fill(const EnvState& e, int P, int t, const int* skip_flag, int skip_when, hipStream_t s);
StemSrc stage_stem_src(const EnvState& e, int P, int t);
// api_rollout.hip
int rollout_impl(jn_ctx* ctx, int mode, const int64_t* forced_actions_dev, const int64_t* start_positions_dev, uint64_t seed,
                 int do_detection, int stop_early, const jn_rollout_out* out, int train, void* stream);
// api_train.hip
void fill_gpt_weights(const jn_ctx* ctx, GptStepArgs& a);
// jn_rollout_steps in two halves: _begin enqueues the copy of n_done to pinned memory and an event behind it, _end waits
// for that event alone — whatever the caller enqueues between the two runs while the host waits and reads
int rollout_steps_begin(jn_ctx* ctx, hipStream_t s);
int rollout_steps_end(jn_ctx* ctx, int* n_steps);
int ensure_token_train_buffers(jn_ctx* ctx);

}  // namespace jnr
