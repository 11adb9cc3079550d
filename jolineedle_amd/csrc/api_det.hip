// C ABI of libjnroll.so, detector unit: inference, the resident training passes and the validation loss of the YOLOX detector.
// Host code only (compiled by hipcc as C++); kernels live in kernels_*.hip.
#include <algorithm>

#include "jn_internal.h"

using namespace jnr;

// xyxy (class, x1, y1, x2, y2) -> (class, cx, cy, w, h), src/models/yolox.py:59-60
extern "C"
__global__ void labels_to_cxcywh_kernel(const float* __restrict__ in, float* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* s = in + 5 * i;
  float* d = out + 5 * i;
  d[0] = s[0]; d[1] = 0.5f * (s[1] + s[3]); d[2] = 0.5f * (s[2] + s[4]); d[3] = s[3] - s[1]; d[4] = s[4] - s[2];
}

extern "C"
__global__ void det_scale_kernel(const float* __restrict__ fwd_scale, const float* __restrict__ dloss, float host_scale,
                                 float* __restrict__ out) {
  out[0] = fwd_scale[0] * (dloss ? dloss[0] : 1.0f) * host_scale;
}

namespace jnr {

// ---- detector training: NeedleYOLOX.forward(patches, targets) (src/models/yolox.py:24-91) in two halves ------------
// A "pass" is one train-mode run of PAFPN + head over up to max_batch patches whose activations stay resident in a
// workspace slot of their own until the backward: slot det_slot_base + pass.  With a separate patch encoder the
// detector net's slot 0 is the eval workspace and the passes start at 1; when the detector's own PAFPN encodes the
// patches (no gpt_backbone) a train-mode rollout owns slots 1 .. T <= block_size of the SAME net, so the passes start
// behind them — the rollout's backward may then run after the detector pass, the reference's statement order
// (src/reinforce.py:326-341).
int det_slot_base(const jn_ctx* ctx) { return ctx->enc_net == JN_NET_DETECTOR ? ctx->cfg.block_size + 1 : 1; }

// threshold / sort / NMS of the N patches in det_raw under the context's candidate policy (jn_set_det_candidates)
static void det_postprocess(jn_ctx* ctx, int N, float* boxes_dev, int32_t* counts_dev, hipStream_t s) {
  const jn_config& c = ctx->cfg;
  (ctx->det_all ? launch_postprocess_all : launch_postprocess)(ctx->det_raw, ctx->nets[JN_NET_DETECTOR].n_anchors, N,
                                                               c.det_conf_threshold, c.det_nms_threshold,
                                                               (float)(c.patch_size - 1), boxes_dev, counts_dev,
                                                               c.max_det_per_patch, nullptr, s);
}

// rows of `targets` the default loss kernel can never cut (its DL_MAXG)
constexpr int DET_LOSS_CAP = 8;

// the SimOTA loss of N patches under the context's box policy (jn_set_det_loss_boxes): the wide kernel only where a
// patch could hold more boxes than the default kernel keeps, so every nb <= 8 result is the default kernel's
static int det_loss(jn_ctx* ctx, int N, int nb, const DetGeom& geo, float* d_raw, float* acc, float loss_scale,
                    float* metrics_dev, float* scale_dev, hipStream_t s) {
  const bool wide = ctx->det_loss_all && nb > DET_LOSS_CAP;
  return (wide ? launch_yolox_loss_wide : launch_yolox_loss)(ctx->det_logits, ctx->det_labels, N, nb, geo, d_raw, acc, 1,
                                                             loss_scale, metrics_dev, scale_dev, s);
}

int detect_impl(jn_ctx* ctx, const StemSrc& ss, int N, float* boxes_dev, int32_t* counts_dev, float* raw_dev,
                const int* skip_flag, int skip_when, hipStream_t s) {
  Net& net = ctx->nets[JN_NET_DETECTOR];
  int rc;
  if (!ctx->det_raw)
    if ((rc = dev_alloc(ctx, &ctx->det_raw, (size_t)ctx->cfg.max_batch * net.n_anchors * 6))) return rc;
  if ((rc = run_net(ctx, JN_NET_DETECTOR, N, ss, 0, 0, skip_flag, skip_when, s, true))) return rc;
  if (raw_dev)
    JN_HIP(hipMemcpyAsync(raw_dev, ctx->det_raw, (size_t)N * net.n_anchors * 6 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (boxes_dev && counts_dev)
    det_postprocess(ctx, N, boxes_dev, counts_dev, s);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

static int detector_forward_impl(jn_ctx* ctx, const float* patches_dev, int N, const float* targets_dev, int nb, int pass,
                                 int n_pass, float loss_scale, float* metrics_dev, hipStream_t s) {
  JN_CHECK(ctx && patches_dev && targets_dev && metrics_dev, JN_EINVAL, "detector training pass: null argument");
  JN_CHECK(ctx->has_net[JN_NET_DETECTOR], JN_ESTATE, "context was created without a detector");
  JN_CHECK(ctx->weights_loaded, JN_ESTATE, "jn_load_weights has not been called");
  JN_CHECK(N >= 1 && N <= ctx->cfg.max_batch, JN_EINVAL, "N=%d exceeds max_batch=%d", N, ctx->cfg.max_batch);
  JN_CHECK(nb >= 1, JN_EINVAL, "targets need at least one (padding) row per patch");
  JN_CHECK(!ctx->det_loss_all || nb <= JN_DETLOSS_MAX_BOXES, JN_EINVAL,
           "targets have nb=%d rows per patch, the detector loss takes at most JN_DETLOSS_MAX_BOXES=%d", nb, JN_DETLOSS_MAX_BOXES);
  JN_CHECK(n_pass >= 1 && n_pass <= 64 && pass >= 0 && pass < n_pass, JN_EINVAL, "detector pass %d of %d", pass, n_pass);
  JN_CHECK(ctx->cfg.act_dtype == JN_F32, JN_ESTATE, "training needs act_dtype = fp32 (bf16 is the inference mode)");
  JN_HIP(hipSetDevice(ctx->cfg.device));
  Net& net = ctx->nets[JN_NET_DETECTOR];
  const int MB = ctx->cfg.max_batch, A = net.n_anchors, P = ctx->cfg.patch_size;
  const int slot = det_slot_base(ctx) + pass;
  int rc;
  if ((rc = ensure_slots(ctx, net, det_slot_base(ctx) + n_pass))) return rc;
  if ((rc = ensure_train_state(ctx, ctx->enc_net == JN_NET_DETECTOR ? std::max(1, ctx->nets[ctx->enc_net].g_slots) : 1))) return rc;
  if (!ctx->det_logits) {
    if ((rc = dev_alloc(ctx, &ctx->det_logits, (size_t)MB * A * 6))) return rc;
    if ((rc = dev_alloc(ctx, &ctx->det_bwd_scale, (size_t)4))) return rc;
  }
  if ((int)ctx->det_pass.size() < n_pass) ctx->det_pass.resize(n_pass);
  jn_ctx::DetPass& dp = ctx->det_pass[pass];
  dp.valid = false;
  if (!dp.dlogits) {
    if ((rc = dev_alloc(ctx, &dp.dlogits, (size_t)MB * A * 6))) return rc;
    if ((rc = dev_alloc(ctx, &dp.acc, (size_t)8 + (size_t)8 * MB))) return rc;
  }
  if (!ctx->det_labels || ctx->det_labels_rows < (size_t)N * nb) {
    if ((rc = dev_alloc(ctx, &ctx->det_labels, (size_t)MB * nb * 5))) return rc;
    ctx->det_labels_rows = (size_t)MB * nb;
  }
  hipLaunchKernelGGL(labels_to_cxcywh_kernel, dim3((N * nb + 255) / 256), dim3(256), 0, s, targets_dev, ctx->det_labels, N * nb);
  if ((rc = run_net(ctx, JN_NET_DETECTOR, N, patch_src(patches_dev, P), slot, 1, nullptr, 0, s, true))) return rc;
  DetGeom geo{};
  geo.A = A;
  for (const Op& op : net.ops) {
    if (op.kind != OP_PRED) continue;
    geo.a0[op.level] = op.anchor0; geo.H[op.level] = op.in.H; geo.W[op.level] = op.in.W; geo.stride[op.level] = op.stride;
  }
  rc = det_loss(ctx, N, nb, geo, dp.dlogits, dp.acc + 8, loss_scale, metrics_dev, dp.acc, s);
  JN_CHECK(rc == 0, JN_EINVAL, "detector loss: nb=%d or A=%d is beyond the wide kernel's capacity", nb, A);
  JN_HIP(hipGetLastError());
  dp.patches = patches_dev; dp.N = N; dp.valid = true;
  return JN_OK;
}

// backward of pass `pass`: d loss / d raw (left by the forward, scaled by scale_dev[0]) through the predictors, the head
// and the PAFPN; parameter gradients ACCUMULATE in the arena
static int detector_backward_impl(jn_ctx* ctx, int pass, const float* scale_dev, hipStream_t s) {
  JN_CHECK(pass >= 0 && pass < (int)ctx->det_pass.size() && ctx->det_pass[pass].valid, JN_ESTATE,
           "detector backward: pass %d has no forward to differentiate (none ran, or a later pass overwrote its activations)", pass);
  Net& net = ctx->nets[JN_NET_DETECTOR];
  const jn_ctx::DetPass& dp = ctx->det_pass[pass];
  const int MB = ctx->cfg.max_batch, A = net.n_anchors, P = ctx->cfg.patch_size, N = dp.N;
  const int slot = det_slot_base(ctx) + pass;
  int rc;
  for (const Op& op : net.ops) {
    if (op.kind != OP_PRED) continue;
    float* g_reg = net.gact + net.buf_off[op.in.buf] * (size_t)MB + op.in.coff;
    float* g_cls = net.gact + net.buf_off[op.res.buf] * (size_t)MB + op.res.coff;
    rc = launch_head_pred_bwd(dp.dlogits, scale_dev, view_ptr(net, slot, MB, op.in), net.bufs[op.in.buf].C,
                              view_tab(net, slot, op.in), view_ptr(net, slot, MB, op.res), net.bufs[op.res.buf].C, view_tab(net, slot, op.res),
                              net.act_dtype, net.pred_w[op.level], g_reg, g_cls, grad_of(ctx, net.pred_w[op.level]),
                              grad_of(ctx, net.pred_b[op.level]), net.head_hid, op.in.H * op.in.W, A, op.anchor0, N, s);
    JN_CHECK(rc == 0, JN_ESTATE, "predictor backward: unsupported buffer type");
  }
  if ((rc = run_net_backward(ctx, JN_NET_DETECTOR, N, patch_src(dp.patches, P), slot, s, 1, 0, true))) return rc;
  JN_HIP(hipGetLastError());
  return JN_OK;
}

// The eval-mode head on the TRAIN-mode FPN maps of a pass (src/models/yolox.py:74-91: `self.eval(); outputs =
// self.head(fpn_outs)` after the loss branch — fpn_outs were computed in the module's current mode, the head now uses
// its running statistics as the train pass has just updated them): the three FPN views (raw z + their batch-statistics
// table entries) are copied into the eval workspace (slot 0) and the head ops run there, so the pass's own head
// activations stay intact for the backward.
static int detector_eval_head(jn_ctx* ctx, int pass, float* boxes_dev, int32_t* counts_dev, hipStream_t s) {
  Net& net = ctx->nets[JN_NET_DETECTOR];
  const jn_ctx::DetPass& dp = ctx->det_pass[pass];
  const int MB = ctx->cfg.max_batch, N = dp.N, slot = det_slot_base(ctx) + pass;
  JN_CHECK(net.n_backbone_ops >= 0, JN_ESTATE, "detector without a head");
  int rc;
  if (!ctx->det_raw)
    if ((rc = dev_alloc(ctx, &ctx->det_raw, (size_t)MB * net.n_anchors * 6))) return rc;
  if ((rc = refresh_eval_table(ctx, net, s))) return rc;          // head tables from the running statistics (just updated)
  for (int i = 0; i < 3; ++i) {
    const View& f = net.fpn[i];
    const int ld = net.bufs[f.buf].C;
    launch_grad_copy((const float*)view_ptr(net, slot, MB, f), ld, (float*)view_ptr(net, 0, MB, f), ld, f.C, (long long)N * f.H * f.W, 0, s);
    const ChanTab src = view_tab(net, slot, f), dst = view_tab(net, 0, f);
    JN_HIP(hipMemcpyAsync(dst.sc, src.sc, f.C * sizeof(float), hipMemcpyDeviceToDevice, s));
    JN_HIP(hipMemcpyAsync(dst.sh, src.sh, f.C * sizeof(float), hipMemcpyDeviceToDevice, s));
    JN_HIP(hipMemcpyAsync(dst.fl, src.fl, f.C * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  StemSrc none{nullptr, nullptr, 0, 0, 0};
  rc = run_net(ctx, JN_NET_DETECTOR, N, none, 0, 0, nullptr, 0, s, true, net.n_backbone_ops);
  net.eval_tab_dirty = true;               // slot 0's FPN entries hold batch statistics now: rebuilt before the next eval pass
  if (rc) return rc;
  det_postprocess(ctx, N, boxes_dev, counts_dev, s);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

}  // namespace jnr

extern "C" {

int jn_detect(jn_ctx* ctx, const float* patches_dev, int N, float* boxes_dev, int32_t* counts_dev, float* raw_dev,
              void* stream) {
  JN_CHECK(ctx && patches_dev, JN_EINVAL, "jn_detect: null argument");
  JN_CHECK(ctx->has_net[JN_NET_DETECTOR], JN_ESTATE, "context was created without a detector");
  JN_CHECK(ctx->weights_loaded, JN_ESTATE, "jn_load_weights has not been called");
  JN_CHECK(N >= 1 && N <= ctx->cfg.max_batch, JN_EINVAL, "N=%d exceeds max_batch=%d", N, ctx->cfg.max_batch);
  JN_HIP(hipSetDevice(ctx->cfg.device));
  return detect_impl(ctx, patch_src(patches_dev, ctx->cfg.patch_size), N, boxes_dev, counts_dev, raw_dev, nullptr, 0, (hipStream_t)stream);
}

int jn_set_det_candidates(jn_ctx* ctx, int all) {
  JN_CHECK(ctx, JN_EINVAL, "jn_set_det_candidates: null ctx");
  JN_CHECK(ctx->has_net[JN_NET_DETECTOR], JN_ESTATE, "context was created without a detector");
  const int A = ctx->nets[JN_NET_DETECTOR].n_anchors;
  JN_CHECK(!all || A <= POST_ALL_MAX_A, JN_EINVAL,
           "jn_set_det_candidates: the detector has A=%d anchors at patch size %d, the kernel holds at most %d in LDS", A,
           ctx->cfg.patch_size, POST_ALL_MAX_A);
  ctx->det_all = all != 0;
  return JN_OK;
}

int jn_set_det_loss_boxes(jn_ctx* ctx, int all) {
  JN_CHECK(ctx, JN_EINVAL, "jn_set_det_loss_boxes: null ctx");
  JN_CHECK(ctx->has_net[JN_NET_DETECTOR], JN_ESTATE, "context was created without a detector");
  const int A = ctx->nets[JN_NET_DETECTOR].n_anchors;
  JN_CHECK(!all || A <= DETLOSS_WIDE_MAX_A, JN_EINVAL,
           "jn_set_det_loss_boxes: the detector has A=%d anchors at patch size %d, the kernel holds at most %d in LDS", A,
           ctx->cfg.patch_size, DETLOSS_WIDE_MAX_A);
  ctx->det_loss_all = all != 0;
  return JN_OK;
}

int jn_detector_step(jn_ctx* ctx, const float* patches_dev, int N, const float* targets_dev, int nb, float loss_scale,
                     float* metrics_dev, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = detector_forward_impl(ctx, patches_dev, N, targets_dev, nb, 0, 1, loss_scale, metrics_dev, s);
  if (rc) return rc;
  rc = detector_backward_impl(ctx, 0, ctx->det_pass[0].acc, s);
  ctx->det_pass[0].valid = false;          // the gradient buffers of the head were consumed
  return rc;
}

int jn_detector_forward(jn_ctx* ctx, const float* patches_dev, int N, const float* targets_dev, int nb, int pass, int n_pass,
                        float* metrics_dev, float* boxes_dev, int32_t* counts_dev, float* fpn0_dev, float* fpn1_dev,
                        float* fpn2_dev, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = detector_forward_impl(ctx, patches_dev, N, targets_dev, nb, pass, n_pass, 1.0f, metrics_dev, s);
  if (rc) return rc;
  Net& net = ctx->nets[JN_NET_DETECTOR];
  const int MB = ctx->cfg.max_batch, slot = det_slot_base(ctx) + pass;
  float* outs[3] = {fpn0_dev, fpn1_dev, fpn2_dev};
  for (int i = 0; i < 3; ++i) {
    if (!outs[i]) continue;
    const View& f = net.fpn[i];
    launch_nhwc_to_nchw(view_ptr(net, slot, MB, f), net.act_dtype, net.bufs[f.buf].C, view_tab(net, slot, f), outs[i], f.C, f.H * f.W, N, s);
  }
  if (boxes_dev && counts_dev && (rc = detector_eval_head(ctx, pass, boxes_dev, counts_dev, s))) return rc;
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_detector_backward(jn_ctx* ctx, int pass, const float* dloss_dev, float scale, void* stream) {
  JN_CHECK(ctx, JN_EINVAL, "jn_detector_backward: null ctx");
  JN_CHECK(ctx->has_net[JN_NET_DETECTOR], JN_ESTATE, "context was created without a detector");
  JN_CHECK(pass >= 0 && pass < (int)ctx->det_pass.size() && ctx->det_pass[pass].valid, JN_ESTATE,
           "jn_detector_backward: pass %d has no forward to differentiate (none ran, or a later pass overwrote its activations)", pass);
  JN_HIP(hipSetDevice(ctx->cfg.device));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(det_scale_kernel, dim3(1), dim3(1), 0, s, ctx->det_pass[pass].acc, dloss_dev, scale, ctx->det_bwd_scale);
  int rc = detector_backward_impl(ctx, pass, ctx->det_bwd_scale, s);
  ctx->det_pass[pass].valid = false;       // one backward per forward (retain_graph is not offered)
  return rc;
}

// NeedleYOLOX.forward(patches, targets) as validation calls it (src/supervised.py:465 under model.eval() and no_grad):
// the PAFPN runs in the module's mode, eval, and only the head goes to train mode for the loss (src/models/yolox.py:54-73).
// Everything happens in the eval workspace (slot 0): backbone ops with the running-statistics table, then the head ops
// from n_backbone_ops on as a train-mode pass over those maps (batch statistics over the N patches; the head's running
// statistics move), the SimOTA loss, and on request the eval head with the statistics as just updated.  The resident
// training passes live in slots of their own and nothing they keep for their backward is written here.
int jn_detector_eval_loss(jn_ctx* ctx, const float* patches_dev, int N, const float* targets_dev, int nb, float* metrics_dev,
                          float* boxes_dev, int32_t* counts_dev, float* fpn0_dev, float* fpn1_dev, float* fpn2_dev, void* stream) {
  JN_CHECK(ctx && patches_dev && targets_dev && metrics_dev, JN_EINVAL, "jn_detector_eval_loss: null argument");
  JN_CHECK(ctx->has_net[JN_NET_DETECTOR], JN_ESTATE, "context was created without a detector");
  JN_CHECK(ctx->weights_loaded, JN_ESTATE, "jn_load_weights has not been called");
  JN_CHECK(N >= 1 && N <= ctx->cfg.max_batch, JN_EINVAL, "N=%d exceeds max_batch=%d", N, ctx->cfg.max_batch);
  JN_CHECK(nb >= 1, JN_EINVAL, "targets need at least one (padding) row per patch");
  JN_CHECK(!ctx->det_loss_all || nb <= JN_DETLOSS_MAX_BOXES, JN_EINVAL,
           "targets have nb=%d rows per patch, the detector loss takes at most JN_DETLOSS_MAX_BOXES=%d", nb, JN_DETLOSS_MAX_BOXES);
  JN_CHECK(ctx->cfg.act_dtype == JN_F32, JN_ESTATE, "the detector loss needs act_dtype = fp32 (bf16 is the inference mode)");
  Net& net = ctx->nets[JN_NET_DETECTOR];
  JN_CHECK(net.n_backbone_ops >= 0, JN_ESTATE, "detector without a head");
  JN_HIP(hipSetDevice(ctx->cfg.device));
  hipStream_t s = (hipStream_t)stream;
  const int MB = ctx->cfg.max_batch, A = net.n_anchors, P = ctx->cfg.patch_size;
  int rc;
  if (!ctx->det_logits) {
    if ((rc = dev_alloc(ctx, &ctx->det_logits, (size_t)MB * A * 6))) return rc;
    if ((rc = dev_alloc(ctx, &ctx->det_bwd_scale, (size_t)4))) return rc;
  }
  if (!ctx->det_eval_dlogits) {
    if ((rc = dev_alloc(ctx, &ctx->det_eval_dlogits, (size_t)MB * A * 6))) return rc;
    if ((rc = dev_alloc(ctx, &ctx->det_eval_acc, (size_t)8 + (size_t)8 * MB))) return rc;
  }
  if (!ctx->det_labels || ctx->det_labels_rows < (size_t)N * nb) {
    if ((rc = dev_alloc(ctx, &ctx->det_labels, (size_t)MB * nb * 5))) return rc;
    ctx->det_labels_rows = (size_t)MB * nb;
  }
  if (boxes_dev && counts_dev && !ctx->det_raw)
    if ((rc = dev_alloc(ctx, &ctx->det_raw, (size_t)MB * A * 6))) return rc;
  hipLaunchKernelGGL(labels_to_cxcywh_kernel, dim3((N * nb + 255) / 256), dim3(256), 0, s, targets_dev, ctx->det_labels, N * nb);
  if ((rc = run_net(ctx, JN_NET_DETECTOR, N, patch_src(patches_dev, P), 0, 0, nullptr, 0, s))) return rc;             // PAFPN, eval
  float* outs[3] = {fpn0_dev, fpn1_dev, fpn2_dev};
  for (int i = 0; i < 3; ++i) {
    if (!outs[i]) continue;
    const View& f = net.fpn[i];
    launch_nhwc_to_nchw(view_ptr(net, 0, MB, f), net.act_dtype, net.bufs[f.buf].C, view_tab(net, 0, f), outs[i], f.C, f.H * f.W, N, s);
  }
  StemSrc none{nullptr, nullptr, 0, 0, 0};
  // head, train: writes batch-statistics entries into slot 0's table for the head layers and sets eval_tab_dirty
  if ((rc = run_net(ctx, JN_NET_DETECTOR, N, none, 0, 1, nullptr, 0, s, true, net.n_backbone_ops))) return rc;
  DetGeom geo{};
  geo.A = A;
  for (const Op& op : net.ops) {
    if (op.kind != OP_PRED) continue;
    geo.a0[op.level] = op.anchor0; geo.H[op.level] = op.in.H; geo.W[op.level] = op.in.W; geo.stride[op.level] = op.stride;
  }
  rc = det_loss(ctx, N, nb, geo, ctx->det_eval_dlogits, ctx->det_eval_acc + 8, 1.0f, metrics_dev, ctx->det_eval_acc, s);
  JN_CHECK(rc == 0, JN_EINVAL, "detector loss: nb=%d or A=%d is beyond the wide kernel's capacity", nb, A);
  if (boxes_dev && counts_dev) {
    // head, eval, on the same maps: run_net rebuilds the whole table from the running statistics first (the backbone's
    // entries come out as they were, the head's from the statistics the pass above has just moved)
    if ((rc = run_net(ctx, JN_NET_DETECTOR, N, none, 0, 0, nullptr, 0, s, true, net.n_backbone_ops))) return rc;
    det_postprocess(ctx, N, boxes_dev, counts_dev, s);
  }
  JN_HIP(hipGetLastError());
  return JN_OK;
}

// jn_yolox_loss / jn_yolox_loss_wide: the loss of given predictor outputs with the default or the wide kernel
static int yolox_loss_entry(const char* who, bool wide, const float* raw_dev, const float* targets_dev, int N, int nb, int P,
                            int stride0, int stride1, int stride2, int use_l1, float loss_scale, float* d_raw_dev,
                            float* metrics_dev, float* scale_dev, void* stream) {
  JN_CHECK(raw_dev && targets_dev && d_raw_dev && metrics_dev && scale_dev, JN_EINVAL, "%s: null argument", who);
  JN_CHECK(N >= 1, JN_EINVAL, "%s: N=%d", who, N);
  JN_CHECK(nb >= 1, JN_EINVAL, "%s: targets need at least one (padding) row per patch", who);
  JN_CHECK(P >= 32 && P % 32 == 0, JN_EINVAL, "%s: patch size %d is not a multiple of 32", who, P);
  const int strides[3] = {stride0, stride1, stride2};
  // the geometry detector_forward_impl reads off the three predictor ops: level l is (P / stride)^2 anchors behind level l - 1
  DetGeom geo{};
  for (int l = 0; l < 3; ++l) {
    JN_CHECK(strides[l] >= 1 && P % strides[l] == 0 && (l == 0 || strides[l] > strides[l - 1]), JN_EINVAL,
             "%s: strides %d, %d, %d do not ascend or do not divide patch size %d", who, stride0, stride1, stride2, P);
    geo.a0[l] = geo.A; geo.H[l] = geo.W[l] = P / strides[l]; geo.stride[l] = strides[l];
    geo.A += geo.H[l] * geo.W[l];
  }
  if (wide) {
    JN_CHECK(nb <= JN_DETLOSS_MAX_BOXES, JN_EINVAL, "%s: targets have nb=%d rows per patch, at most JN_DETLOSS_MAX_BOXES=%d", who,
             nb, JN_DETLOSS_MAX_BOXES);
    JN_CHECK(geo.A <= DETLOSS_WIDE_MAX_A, JN_EINVAL, "%s: A=%d anchors at patch size %d, the kernel holds at most %d in LDS", who,
             geo.A, P, DETLOSS_WIDE_MAX_A);
  }
  hipStream_t s = (hipStream_t)stream;
  float* work = nullptr;                                         // cxcywh labels, then the per-patch sums
  const size_t n_lab = (size_t)N * nb * 5;
  JN_HIP(hipMalloc((void**)&work, (n_lab + (size_t)8 * N) * sizeof(float)));
  hipLaunchKernelGGL(labels_to_cxcywh_kernel, dim3((N * nb + 255) / 256), dim3(256), 0, s, targets_dev, work, N * nb);
  (wide ? launch_yolox_loss_wide : launch_yolox_loss)(raw_dev, work, N, nb, geo, d_raw_dev, work + n_lab, use_l1, loss_scale,
                                                      metrics_dev, scale_dev, s);
  const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(s);
  (void)hipFree(work);
  JN_HIP(e1);
  JN_HIP(e2);
  return JN_OK;
}

int jn_yolox_loss(const float* raw_dev, const float* targets_dev, int N, int nb, int P, int stride0, int stride1,
                  int stride2, int use_l1, float loss_scale, float* d_raw_dev, float* metrics_dev, float* scale_dev,
                  void* stream) {
  return yolox_loss_entry("jn_yolox_loss", false, raw_dev, targets_dev, N, nb, P, stride0, stride1, stride2, use_l1, loss_scale,
                          d_raw_dev, metrics_dev, scale_dev, stream);
}

int jn_yolox_loss_wide(const float* raw_dev, const float* targets_dev, int N, int nb, int P, int stride0, int stride1,
                       int stride2, int use_l1, float loss_scale, float* d_raw_dev, float* metrics_dev, float* scale_dev,
                       void* stream) {
  return yolox_loss_entry("jn_yolox_loss_wide", true, raw_dev, targets_dev, N, nb, P, stride0, stride1, stride2, use_l1,
                          loss_scale, d_raw_dev, metrics_dev, scale_dev, stream);
}

}  // extern "C"
