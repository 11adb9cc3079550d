// C ABI of libjnroll.so, context unit: creation, the state-dict table, weight packing and the tensor read-backs.
// Host code only (compiled by hipcc as C++); kernels live in kernels_*.hip.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstring>
#include <memory>

#include "jn_internal.h"

namespace jnr {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int build_pafpn(Net& net, std::vector<ParamEntry>& params, const std::string& prefix, float depth, float width,
                bool depthwise, int P);
int build_head(Net& net, std::vector<ParamEntry>& params, const std::string& prefix, float width, bool depthwise,
               int num_classes);

int dev_upload(jn_ctx* ctx, float** out, const std::vector<float>& host) {
  if (!*out) {                                   // re-uploads (weights changed) reuse the allocation
    int rc = dev_alloc(ctx, out, host.size());
    if (rc) return rc;
  }
  JN_HIP(hipMemcpy(*out, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  return JN_OK;
}

int n_parts(const jn_config& c) { return 2 + (c.no_patch_emb ? 0 : 1) + (c.use_pos_emb ? 1 : 0); }

namespace {

// ---- flat parameter store ---------------------------------------------------------------
// Every trainable tensor lives in one contiguous fp32 arena (packed layouts), mirrored by a
// gradient arena and the AdamW moments: the optimiser and the RCCL all-reduce see ONE buffer.
enum PackKind { PK_RAW = 0, PK_T, PK_STEM, PK_DW, PK_CONV3, PK_EFPN_LIN };

int store_param(jn_ctx* ctx, const std::string& name, const std::vector<float>& packed, int kind, int d0, int d1,
                int d2, float** out) {
  auto it = ctx->seg_index.find(name);
  if (it == ctx->seg_index.end()) {
    const size_t padded = (packed.size() + 3) / 4 * 4;
    // tensors of 64 values and more start on a multiple of 8 floats (pw_x3_kernel's split weights come in groups of 8; the
    // small ones — predictor rows and biases — stay back to back, the head kernels read them as one matrix)
    if (packed.size() >= 64) ctx->arena_used = (ctx->arena_used + 7) / 8 * 8;
    JN_CHECK(ctx->params && ctx->arena_used + padded <= ctx->arena_size, JN_ENOMEM, "parameter arena exhausted at '%s'",
             name.c_str());
    ParamSeg sg;
    sg.name = name; sg.kind = kind; sg.d0 = d0; sg.d1 = d1; sg.d2 = d2; sg.off = ctx->arena_used; sg.numel = packed.size();
    ctx->arena_used += padded;
    ctx->seg_index[name] = (int)ctx->segs.size();
    ctx->segs.push_back(sg);
    it = ctx->seg_index.find(name);
  }
  const ParamSeg& sg = ctx->segs[it->second];
  JN_CHECK(sg.numel == packed.size(), JN_EINVAL, "'%s' changed size between loads", name.c_str());
  JN_HIP(hipMemcpy(ctx->params + sg.off, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
  *out = ctx->params + sg.off;
  return JN_OK;
}

// inverse of the packing: arena layout -> the reference's (PyTorch) layout
std::vector<float> unpack_param(const ParamSeg& sg, const std::vector<float>& p) {
  std::vector<float> t(p.size());
  switch (sg.kind) {
    case PK_T:        // stored [in][out] -> [out][in]; d0 = out, d1 = in
      for (int o = 0; o < sg.d0; ++o)
        for (int i = 0; i < sg.d1; ++i) t[(size_t)o * sg.d1 + i] = p[(size_t)i * sg.d0 + o];
      break;
    case PK_STEM:     // [(c*6+dy)*6+dx][oc] -> [oc][q*3+c][ky][kx]; d0 = cout
      for (int oc = 0; oc < sg.d0; ++oc)
        for (int c = 0; c < 3; ++c)
          for (int dy = 0; dy < 6; ++dy)
            for (int dx = 0; dx < 6; ++dx) {
              const int ky = dy >> 1, py = dy & 1, kx = dx >> 1, px = dx & 1, q = py + 2 * px;
              t[(((size_t)oc * 12 + q * 3 + c) * 3 + ky) * 3 + kx] = p[(size_t)((c * 6 + dy) * 6 + dx) * sg.d0 + oc];
            }
      break;
    case PK_DW:       // [tap][c] -> [c][tap]; d0 = C
      for (int c = 0; c < sg.d0; ++c)
        for (int k = 0; k < 9; ++k) t[(size_t)c * 9 + k] = p[(size_t)k * sg.d0 + c];
      break;
    case PK_CONV3:    // [tap][o][k] -> [o][k][tap]; d0 = cout, d1 = cin
      for (int o = 0; o < sg.d0; ++o)
        for (int k = 0; k < sg.d1; ++k)
          for (int tp = 0; tp < 9; ++tp) t[((size_t)o * sg.d1 + k) * 9 + tp] = p[((size_t)tp * sg.d0 + o) * sg.d1 + k];
      break;
    case PK_EFPN_LIN: // [(p*C + ch)][o] -> [o][ch*HW + p]; d0 = C(out), d1 = HW, d2 = C(in)
      for (int o = 0; o < sg.d0; ++o)
        for (int ch = 0; ch < sg.d2; ++ch)
          for (int q = 0; q < sg.d1; ++q)
            t[(size_t)o * sg.d1 * sg.d2 + (size_t)ch * sg.d1 + q] = p[((size_t)q * sg.d2 + ch) * sg.d0 + o];
      break;
    default: t = p;
  }
  return t;
}

struct TensorMap {
  std::map<std::string, const jn_tensor*> m;
  const float* f32(const std::string& name, size_t numel) const {
    auto it = m.find(name);
    if (it == m.end()) { set_error("state-dict entry '%s' is missing", name.c_str()); return nullptr; }
    const jn_tensor* t = it->second;
    size_t n = 1;
    for (int i = 0; i < t->ndim; ++i) n *= (size_t)t->shape[i];
    if (t->dtype != 0 || n != numel) {
      set_error("state-dict entry '%s' has %zu elements / dtype %d, expected %zu float32", name.c_str(), n, t->dtype, numel);
      return nullptr;
    }
    return (const float*)t->data;
  }
};

// Linear weight [out][in] -> transposed [in][out]
std::vector<float> transpose(const float* w, int out, int in) {
  std::vector<float> t((size_t)out * in);
  for (int o = 0; o < out; ++o)
    for (int i = 0; i < in; ++i) t[(size_t)i * out + o] = w[(size_t)o * in + i];
  return t;
}

int upload_raw(jn_ctx* ctx, const TensorMap& tm, const std::string& name, size_t n, float** out) {
  const float* p = tm.f32(name, n);
  if (!p) return JN_ENOTFOUND;
  return store_param(ctx, name, std::vector<float>(p, p + n), PK_RAW, (int)n, 0, 0, out);
}
int upload_buf(jn_ctx* ctx, const TensorMap& tm, const std::string& name, size_t n, float** out) {
  const float* p = tm.f32(name, n);
  if (!p) return JN_ENOTFOUND;
  return dev_upload(ctx, out, std::vector<float>(p, p + n));
}
int upload_t(jn_ctx* ctx, const TensorMap& tm, const std::string& name, int out_f, int in_f, float** out) {
  const float* p = tm.f32(name, (size_t)out_f * in_f);
  if (!p) return JN_ENOTFOUND;
  return store_param(ctx, name, transpose(p, out_f, in_f), PK_T, out_f, in_f, 0, out);
}

// The two halves of a merged pair (ConvW::prefix2): every tensor kind is stored first-half then second-half, back to
// back, so the kernels see one conv of cout channels.
int pack_conv_pair(jn_ctx* ctx, const TensorMap& tm, ConvW& cw) {
  const int h = cw.cout_first, h2 = cw.cout - h;
  int rc;
  auto pair_raw = [&](const std::string& leaf, size_t n1, size_t n2, float** out) -> int {
    float *a = nullptr, *b = nullptr;
    if ((rc = upload_raw(ctx, tm, cw.prefix + leaf, n1, &a))) return rc;
    if ((rc = upload_raw(ctx, tm, cw.prefix2 + leaf, n2, &b))) return rc;
    JN_CHECK(b == a + n1, JN_ESTATE, "merged conv pair '%s': halves of %s are not contiguous in the arena", cw.prefix.c_str(), leaf.c_str());
    *out = a;
    return JN_OK;
  };
  auto pair_buf = [&](const std::string& leaf, float** out) -> int {
    const float* a = tm.f32(cw.prefix + leaf, h);
    const float* b = tm.f32(cw.prefix2 + leaf, h2);
    if (!a || !b) return JN_ENOTFOUND;
    std::vector<float> both(a, a + h);
    both.insert(both.end(), b, b + h2);
    return dev_upload(ctx, out, both);
  };
  if ((rc = pair_raw(".bn.weight", h, h2, &cw.gamma_dev))) return rc;
  if ((rc = pair_raw(".bn.bias", h, h2, &cw.beta_dev))) return rc;
  if ((rc = pair_buf(".bn.running_mean", &cw.rmean_dev))) return rc;
  if ((rc = pair_buf(".bn.running_var", &cw.rvar_dev))) return rc;
  return pair_raw(".conv.weight", (size_t)h * cw.cin, (size_t)h2 * cw.cin, &cw.w_dev);
}

int pack_conv(jn_ctx* ctx, const TensorMap& tm, ConvW& cw, OpKind kind) {
  if (!cw.prefix2.empty()) return pack_conv_pair(ctx, tm, cw);
  const int cig = cw.cin / cw.groups;
  const std::string wname = cw.prefix + (cw.has_bn ? ".conv.weight" : ".weight");
  const float* w = tm.f32(wname, (size_t)cw.cout * cig * cw.k * cw.k);
  if (!w) return JN_ENOTFOUND;
  int rc;
  if (cw.has_bn) {
    const int co = cw.cout;
    if ((rc = upload_raw(ctx, tm, cw.prefix + ".bn.weight", co, &cw.gamma_dev))) return rc;
    if ((rc = upload_raw(ctx, tm, cw.prefix + ".bn.bias", co, &cw.beta_dev))) return rc;
    if ((rc = upload_buf(ctx, tm, cw.prefix + ".bn.running_mean", co, &cw.rmean_dev))) return rc;
    if ((rc = upload_buf(ctx, tm, cw.prefix + ".bn.running_var", co, &cw.rvar_dev))) return rc;
  } else if (cw.has_bias) {
    if ((rc = upload_raw(ctx, tm, cw.prefix + ".bias", cw.cout, &cw.b_dev))) return rc;
  }
  std::vector<float> packed;
  int pk = PK_RAW;
  if (kind == OP_STEM) {
    pk = PK_STEM;
    // [oc][q*3 + c][ky][kx] (Focus order TL, BL, TR, BR: q = py + 2*px)  ->  [(c*6+dy)*6+dx][oc]
    packed.assign((size_t)108 * cw.cout, 0.0f);
    for (int oc = 0; oc < cw.cout; ++oc)
      for (int c = 0; c < 3; ++c)
        for (int dy = 0; dy < 6; ++dy)
          for (int dx = 0; dx < 6; ++dx) {
            const int ky = dy >> 1, py = dy & 1, kx = dx >> 1, px = dx & 1, q = py + 2 * px;
            packed[(size_t)((c * 6 + dy) * 6 + dx) * cw.cout + oc] = w[(((size_t)oc * 12 + q * 3 + c) * 3 + ky) * 3 + kx];
          }
  } else if (kind == OP_DW) {
    pk = PK_DW;
    packed.resize((size_t)9 * cw.cout);
    for (int c = 0; c < cw.cout; ++c)
      for (int t = 0; t < 9; ++t) packed[(size_t)t * cw.cout + c] = w[(size_t)c * 9 + t];
  } else if (kind == OP_PW) {
    packed.assign(w, w + (size_t)cw.cout * cw.cin);
  } else if (kind == OP_CONV3) {
    // [tap][oc][cin]: every tap is a 1x1 GEMM weight
    pk = PK_CONV3;
    packed.resize((size_t)9 * cw.cout * cw.cin);
    for (int o = 0; o < cw.cout; ++o)
      for (int k = 0; k < cw.cin; ++k)
        for (int t = 0; t < 9; ++t) packed[((size_t)t * cw.cout + o) * cw.cin + k] = w[((size_t)o * cw.cin + k) * 9 + t];
  } else {
    return JN_OK;
  }
  int rcs = store_param(ctx, wname, packed, pk, cw.cout, cw.cin, 0, &cw.w_dev);
  if (rcs == JN_OK && kind == OP_CONV3 && ctx->cfg.act_dtype == JN_BF16) {
    // bf16 inference mode: the MFMA operands are bf16 anyway — round the weights once here (round to nearest even)
    // instead of in every workgroup's staging loop
    std::vector<uint16_t> hb(packed.size());
    for (size_t i = 0; i < packed.size(); ++i) {
      uint32_t u;
      std::memcpy(&u, &packed[i], 4);
      u += 0x7FFFu + ((u >> 16) & 1u);
      hb[i] = (uint16_t)(u >> 16);
    }
    if (!cw.w_bf16) {
      uint16_t* d = nullptr;
      if ((rcs = dev_alloc(ctx, &d, hb.size()))) return rcs;
      cw.w_bf16 = d;
    }
    JN_HIP(hipMemcpy(cw.w_bf16, hb.data(), hb.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  }
  return rcs;
}

// get_emb(pos * inv_freq) of positional_encodings >= 6 (interleaved sin, cos), SURVEY.md §2.2
std::vector<float> sinusoid_row(int pos, int channels) {
  std::vector<float> r(channels);
  for (int i = 0; i < channels; i += 2) {
    const float inv_freq = 1.0f / std::pow(10000.0f, (float)i / (float)channels);
    const float ang = (float)pos * inv_freq;
    r[i] = std::sin(ang);
    if (i + 1 < channels) r[i + 1] = std::cos(ang);
  }
  return r;
}

// Device-side workspaces; allocated on the first jn_load_weights (needs a GPU).
static int alloc_workspaces(jn_ctx* ctx) {
  jn_ctx& x = *ctx;
  const jn_config& c = ctx->cfg;
  const int B = c.max_batch, C = c.n_embd;
  int rc;
  for (int n = 0; n < 2; ++n) {
    if (!ctx->has_net[n]) continue;
    if ((rc = ensure_slots(ctx, ctx->nets[n], 1))) return rc;
  }
  const int Tmax = c.block_size + 1;
  if ((rc = dev_alloc(ctx, &ctx->kcache, (size_t)c.n_layer * B * Tmax * C))) return rc;
  if ((rc = dev_alloc(ctx, &ctx->vcache, (size_t)c.n_layer * B * Tmax * C))) return rc;
  if ((rc = dev_alloc(ctx, &ctx->n_done, (size_t)Tmax + 1))) return rc;
  if ((rc = dev_alloc(ctx, &ctx->prev_action, (size_t)B))) return rc;
  if ((rc = dev_alloc(ctx, &ctx->cache_len, (size_t)B))) return rc;
  if ((rc = dev_alloc(ctx, &x.emb_part, (size_t)B * x.KS * C))) return rc;
  if (!c.no_patch_emb)
    if ((rc = dev_alloc(ctx, &ctx->efpn_act, (size_t)B * ctx->efpn_h * ctx->efpn_w * C))) return rc;
  if ((rc = dev_alloc(ctx, &ctx->patch_emb, (size_t)B * C))) return rc;
  if (ctx->decision_route == 1 && (rc = dev_alloc(ctx, &ctx->wide_scratch, gpt_wide_scratch_floats(C, n_parts(c), B)))) return rc;
  JN_HIP(hipMemset(ctx->n_done, 0, ((size_t)Tmax + 1) * sizeof(int32_t)));
  for (auto& e : ctx->ev) JN_HIP(hipEventCreate(&e));
  return JN_OK;
}

}  // namespace

}  // namespace jnr

using namespace jnr;

extern "C" {

int jn_abi_version(void) { return JN_ABI_VERSION; }
const char* jn_last_error(void) { return jnr::g_err; }

int jn_create(const jn_config* cfg, jn_ctx** out) {
  JN_CHECK(cfg && out, JN_EINVAL, "jn_create: null argument");
  JN_CHECK(cfg->struct_size == (int)sizeof(jn_config), JN_EINVAL, "jn_config.struct_size %d != %zu", cfg->struct_size,
           sizeof(jn_config));
  JN_CHECK(cfg->n_embd > 0 && cfg->n_embd % 4 == 0 &&
               (cfg->n_embd <= GPT_PER_AGENT_MAX_C || (cfg->n_embd <= GPT_WIDE_MAX_C && cfg->n_embd % 64 == 0)),
           JN_EINVAL, "n_embd %d unsupported (a multiple of 4 up to %d, or a multiple of 64 up to %d)", cfg->n_embd,
           GPT_PER_AGENT_MAX_C, GPT_WIDE_MAX_C);
  JN_CHECK(cfg->n_head > 0 && cfg->n_embd % cfg->n_head == 0, JN_EINVAL, "n_embd %% n_head != 0");
  JN_CHECK(cfg->n_actions == 8 || cfg->n_actions == 9, JN_EINVAL, "n_actions must be 8 or 9");
  JN_CHECK(cfg->block_size >= 1 && cfg->block_size <= 255, JN_EINVAL, "block_size out of range");
  JN_CHECK(cfg->max_batch >= 1, JN_EINVAL, "max_batch must be >= 1");
  JN_CHECK(cfg->gpt_bb_width > 0 || cfg->with_detector || cfg->no_patch_emb, JN_EINVAL,
           "no patch encoder: set gpt_bb_width or with_detector (or no_patch_emb)");
  std::unique_ptr<jn_ctx> ctx(new jn_ctx());
  ctx->cfg = *cfg;
  {
    // the decision route: past gpt_step_kernel's envelope the wide one; cfg->gpt_wide (JN_GPT_WIDE=1 of the Python layer)
    // takes it for every narrower model it admits as well — a test and A/B switch, ignored for the shapes it refuses
    const bool want = cfg->n_embd > GPT_PER_AGENT_MAX_C || cfg->gpt_wide == 1;
    ctx->decision_route = want && gpt_wide_admits(cfg->n_embd, cfg->n_head, cfg->block_size) ? 1 : 0;
    JN_CHECK(cfg->n_embd <= GPT_PER_AGENT_MAX_C || ctx->decision_route == 1, JN_EINVAL,
             "n_embd %d (above %d, up to %d) needs the wide decision route, which refuses this shape", cfg->n_embd,
             GPT_PER_AGENT_MAX_C, GPT_WIDE_MAX_C);
  }
  JN_CHECK(cfg->act_dtype == JN_F32 || cfg->act_dtype == JN_BF16, JN_EINVAL, "act_dtype must be 0 (fp32) or 1 (bf16)");
  ctx->nets[0].act_dtype = ctx->nets[1].act_dtype = cfg->act_dtype;
  if (ctx->cfg.det_nms_threshold <= 0) ctx->cfg.det_nms_threshold = 0.45f;
  if (ctx->cfg.max_det_per_patch <= 0) ctx->cfg.max_det_per_patch = 64;
  const int C = cfg->n_embd, nA = cfg->n_actions;
  auto& P = ctx->params_tab;
  // ---- state-dict table in the reference's construction order (src/models/gpt.py:221-318) ----
  add_param(P, "action_head.lm_heads.0.weight", {nA, C}, 0, false, true);
  {
    const int ch2 = (int)std::ceil(C / 4.0) * 2;
    add_param(P, "positional_encoding.inv_freq", {(ch2 + 1) / 2}, 0, true, false);
    if (cfg->decoder_pos_encoding) {
      const int ch1 = (int)std::ceil(C / 2.0) * 2;
      add_param(P, "decoder_token_pos_enc.inv_freq", {ch1 / 2}, 0, true, false);
    }
  }
  add_param(P, "embed_class.weight", {100, C}, 0, false, true);
  if (cfg->concat_emb) {
    add_param(P, "project_concat.weight", {C, (int64_t)n_parts(*cfg) * C}, 0, false, true);
    add_param(P, "project_concat.bias", {C}, 0, false, true);
  }
  int rc;
  if (cfg->with_detector) {
    rc = build_pafpn(ctx->nets[JN_NET_DETECTOR], P, "yolox.backbone.", cfg->det_depth, cfg->det_width,
                     cfg->det_depthwise != 0, cfg->patch_size);
    if (rc) return rc;
    ctx->has_net[JN_NET_DETECTOR] = true;
    rc = build_head(ctx->nets[JN_NET_DETECTOR], P, "yolox.head.", cfg->det_width, cfg->det_depthwise != 0, 1);
    if (rc) return rc;
  }
  if (cfg->gpt_bb_width > 0) {
    rc = build_pafpn(ctx->nets[JN_NET_GPT_BACKBONE], P, "gpt_backbone.", cfg->gpt_bb_depth, cfg->gpt_bb_width,
                     cfg->gpt_bb_depthwise != 0, cfg->patch_size);
    if (rc) return rc;
    ctx->has_net[JN_NET_GPT_BACKBONE] = true;
    ctx->enc_net = JN_NET_GPT_BACKBONE;
  } else {
    ctx->enc_net = JN_NET_DETECTOR;
  }
  // the plans of the training backwards, checked here so that a broken one fails now (each backward plans again): the
  // patch encoder fed through fpn[2] alone, unless it is the detached detector, and the detector with its head.  A bf16
  // context never trains (plan_backward refuses it): nothing to check
  std::vector<BwdStep> plan;
  const bool trains = cfg->act_dtype == JN_F32;
  if (trains && ctx->enc_net != JN_NET_DETECTOR && (rc = plan_backward(ctx->nets[ctx->enc_net], false, 0x3, plan))) return rc;
  if (trains && cfg->with_detector && (rc = plan_backward(ctx->nets[JN_NET_DETECTOR], true, 0, plan))) return rc;
  // ... and the forward passes each net will run (run_net plans again per call), at both ends of the batch range: the
  // PAFPN in eval and train mode, with a head also the whole detector and the head-only range of its training step
  std::vector<FwdStep> fplan;
  for (int ni = 0; ni < 2; ++ni) {
    const Net& net = ctx->nets[ni];
    const bool head = net.n_backbone_ops >= 0;
    if (!ctx->has_net[ni]) continue;
    for (int N : {1, cfg->max_batch})
      for (int train = 0; train < 2; ++train) {
        if ((rc = plan_forward(net, N, train, false, 0, train && defer_eligible(net), fplan))) return rc;
        if (head && (rc = plan_forward(net, N, train, true, 0, false, fplan))) return rc;
        if (head && !train && (rc = plan_forward(net, N, false, true, net.n_backbone_ops, false, fplan))) return rc;
      }
  }
  if (!cfg->no_patch_emb) {
    const Net& enc = ctx->nets[ctx->enc_net];
    ctx->efpn_cin = enc.fpn[2].C; ctx->efpn_h = enc.fpn[2].H; ctx->efpn_w = enc.fpn[2].W;
    // split-K slices of embed_fpn.3: ~192 inputs each, 8..64 slices (their partials are summed by the consumer)
    ctx->KS = std::max(8, std::min(64, (ctx->efpn_h * ctx->efpn_w * C + 191) / 192));
    add_param(P, "embed_fpn.0.weight", {C, ctx->efpn_cin, 1, 1}, 0, false, true);
    add_param(P, "embed_fpn.3.weight", {C, (int64_t)ctx->efpn_h * ctx->efpn_w * C}, 0, false, true);
    add_param(P, "embed_fpn.3.bias", {C}, 0, false, true);
  }
  add_param(P, "transformer.wte.weight", {nA, C}, 0, false, true);
  add_param(P, "transformer.wpe.weight", {cfg->pos_emb_size > 0 ? cfg->pos_emb_size : 1, C}, 0, false,
            !cfg->decoder_pos_encoding);
  const int bs1 = cfg->block_size + 1;
  for (int l = 0; l < cfg->n_layer; ++l) {
    const std::string p = "transformer.h." + std::to_string(l) + ".";
    add_param(P, p + "ln_1.weight", {C}, 0, false, true);
    add_param(P, p + "ln_1.bias", {C}, 0, false, true);
    add_param(P, p + "attn.c_attn.weight", {3 * C, C}, 0, false, true);
    add_param(P, p + "attn.c_attn.bias", {3 * C}, 0, false, true);
    add_param(P, p + "attn.c_proj.weight", {C, C}, 0, false, true);
    add_param(P, p + "attn.c_proj.bias", {C}, 0, false, true);
    add_param(P, p + "attn.bias", {1, 1, bs1, bs1}, 0, true, false);
    add_param(P, p + "ln_2.weight", {C}, 0, false, true);
    add_param(P, p + "ln_2.bias", {C}, 0, false, true);
    add_param(P, p + "mlp.c_fc.weight", {4 * C, C}, 0, false, true);
    add_param(P, p + "mlp.c_fc.bias", {4 * C}, 0, false, true);
    add_param(P, p + "mlp.c_proj.weight", {C, 4 * C}, 0, false, true);
    add_param(P, p + "mlp.c_proj.bias", {C}, 0, false, true);
  }
  add_param(P, "transformer.ln_f.weight", {C}, 0, false, true);
  add_param(P, "transformer.ln_f.bias", {C}, 0, false, true);
  *out = ctx.release();
  return JN_OK;
}

int jn_destroy(jn_ctx* ctx) {
  if (!ctx) return JN_OK;
  (void)hipSetDevice(ctx->cfg.device);
  (void)hipDeviceSynchronize();
  for (void* p : ctx->owned) (void)hipFree(p);
  if (ctx->env.stage) (void)hipFree(ctx->env.stage);
  for (auto& e : ctx->ev) if (e) (void)hipEventDestroy(e);
  for (auto& e : ctx->conv_ev) (void)hipEventDestroy(e);
  if (ctx->aux_fork) (void)hipEventDestroy(ctx->aux_fork);
  if (ctx->aux_join) (void)hipEventDestroy(ctx->aux_join);
  if (ctx->steps_ev) (void)hipEventDestroy(ctx->steps_ev);
  if (ctx->n_done_host) (void)hipHostFree(ctx->n_done_host);
  if (ctx->aux_stream) (void)hipStreamDestroy(ctx->aux_stream);
  delete ctx;
  return JN_OK;
}

int jn_debug_decision_route(const jn_ctx* ctx) { return ctx ? ctx->decision_route : JN_EINVAL; }

int jn_param_count(const jn_ctx* ctx) { return ctx ? (int)ctx->params_tab.size() : JN_EINVAL; }

int jn_param_info_at(const jn_ctx* ctx, int index, jn_param_info* out) {
  JN_CHECK(ctx && out && index >= 0 && index < (int)ctx->params_tab.size(), JN_EINVAL, "jn_param_info_at: bad index %d", index);
  *out = ctx->params_tab[index].info;
  return JN_OK;
}

int jn_load_weights(jn_ctx* ctx, const jn_tensor* tensors, size_t n) {
  JN_CHECK(ctx && tensors, JN_EINVAL, "jn_load_weights: null argument");
  JN_HIP(hipSetDevice(ctx->cfg.device));
  TensorMap tm;
  for (size_t i = 0; i < n; ++i) tm.m[tensors[i].name] = &tensors[i];
  int rc;
  if (!ctx->kcache) {
    if ((rc = alloc_workspaces(ctx))) return rc;
  }
  if (!ctx->params) {
    size_t total = 0;
    for (const ParamEntry& e : ctx->params_table()) {
      if (e.info.dtype != 0 || e.info.is_buffer || !e.info.used) continue;
      size_t n = 1;
      for (int i = 0; i < e.info.ndim; ++i) n *= (size_t)e.info.shape[i];
      total += (n + 3) / 4 * 4 + (n >= 64 ? 4 : 0);
    }
    ctx->arena_size = total;
    if ((rc = dev_alloc(ctx, &ctx->params, total))) return rc;
    JN_HIP(hipMemset(ctx->params, 0, total * sizeof(float)));
    if ((rc = dev_alloc(ctx, &ctx->params_x3, 3 * total))) return rc;
    if ((rc = dev_alloc(ctx, &ctx->params_x3t, 3 * total))) return rc;
  }
  const jn_config& c = ctx->cfg;
  const int C = c.n_embd, nA = c.n_actions;
  auto pack_net = [&](int ni) -> int {
    if (!ctx->has_net[ni]) return JN_OK;
    Net& net = ctx->nets[ni];
    for (const Op& op : net.ops) {
      if (op.wslot < 0) continue;
      int r = pack_conv(ctx, tm, net.convs[op.wslot], op.kind);
      if (r) return r;
    }
    for (const Op& op : net.ops) {
      if (op.kind != OP_PRED) continue;
      const std::string k = std::to_string(op.level), hp = "yolox.head.";
      const int hid = net.head_hid;
      // arena-resident (trainable): reg (4 x hid) | obj (hid) | cls (hid) rows back to back = one [6][hid] matrix;
      // biases reg (4) | obj (1, padded to 4) | cls (1, padded to 4): entries 0..3, 4 and 8 of `pred_b`
      int r;
      float *w_reg = nullptr, *w_obj = nullptr, *w_cls = nullptr, *b_reg = nullptr, *b_obj = nullptr, *b_cls = nullptr;
      if ((r = upload_raw(ctx, tm, hp + "reg_preds." + k + ".weight", (size_t)4 * hid, &w_reg))) return r;
      if ((r = upload_raw(ctx, tm, hp + "obj_preds." + k + ".weight", hid, &w_obj))) return r;
      if ((r = upload_raw(ctx, tm, hp + "cls_preds." + k + ".weight", hid, &w_cls))) return r;
      if ((r = upload_raw(ctx, tm, hp + "reg_preds." + k + ".bias", 4, &b_reg))) return r;
      if ((r = upload_raw(ctx, tm, hp + "obj_preds." + k + ".bias", 1, &b_obj))) return r;
      if ((r = upload_raw(ctx, tm, hp + "cls_preds." + k + ".bias", 1, &b_cls))) return r;
      JN_CHECK(w_obj == w_reg + 4 * hid && w_cls == w_obj + hid && b_obj == b_reg + 4 && b_cls == b_reg + 8, JN_ESTATE,
               "predictor tensors of level %d are not contiguous in the arena", op.level);
      net.pred_w[op.level] = w_reg;
      net.pred_b[op.level] = b_reg;
    }
    return JN_OK;
  };
  mark_params_written(ctx);
  // arena order: [gpt_backbone | decision model] = what optim_gpt updates (gpt.py:552-557), then yolox.*
  if ((rc = pack_net(JN_NET_GPT_BACKBONE))) return rc;
  GptW& g = ctx->gpt;
  if ((rc = upload_raw(ctx, tm, "transformer.wte.weight", (size_t)nA * C, &g.wte))) return rc;
  if (!c.decoder_pos_encoding) {
    if ((rc = upload_raw(ctx, tm, "transformer.wpe.weight", (size_t)std::max(c.pos_emb_size, 1) * C, &g.wpe))) return rc;
  }
  if ((rc = upload_raw(ctx, tm, "embed_class.weight", (size_t)100 * C, &g.embed_class))) return rc;
  if (c.concat_emb) {
    if ((rc = upload_t(ctx, tm, "project_concat.weight", C, n_parts(c) * C, &g.proj_wt))) return rc;
    if ((rc = upload_raw(ctx, tm, "project_concat.bias", C, &g.proj_b))) return rc;
  }
  {
    const int ch1 = (int)std::ceil(C / 2.0) * 2;
    const int Tmax = c.block_size + 1;
    std::vector<float> p1((size_t)Tmax * C);
    for (int t = 0; t < Tmax; ++t) {
      std::vector<float> r = sinusoid_row(t, ch1);
      std::copy(r.begin(), r.begin() + C, p1.begin() + (size_t)t * C);
    }
    if ((rc = dev_upload(ctx, &g.pos1d, p1))) return rc;
    const int ch2 = (int)std::ceil(C / 4.0) * 2;
    std::vector<float> tab((size_t)256 * ch2);
    for (int p = 0; p < 256; ++p) {
      std::vector<float> r = sinusoid_row(p, ch2);
      std::copy(r.begin(), r.end(), tab.begin() + (size_t)p * ch2);
    }
    if ((rc = dev_upload(ctx, &g.pos2d_col, tab))) return rc;
  }
  if (!c.no_patch_emb) {
    if ((rc = upload_raw(ctx, tm, "embed_fpn.0.weight", (size_t)C * ctx->efpn_cin, &g.efpn_w))) return rc;
    const int HW = ctx->efpn_h * ctx->efpn_w;
    const float* lw = tm.f32("embed_fpn.3.weight", (size_t)C * HW * C);
    if (!lw) return JN_ENOTFOUND;
    // Flatten order of the reference is (c, h, w) (nn.Flatten on NCHW, gpt.py:304); ours is (h, w, c).
    std::vector<float> wt((size_t)HW * C * C);
    for (int o = 0; o < C; ++o)
      for (int ch = 0; ch < C; ++ch)
        for (int p = 0; p < HW; ++p) wt[((size_t)p * C + ch) * C + o] = lw[(size_t)o * HW * C + (size_t)ch * HW + p];
    if ((rc = store_param(ctx, "embed_fpn.3.weight", wt, PK_EFPN_LIN, C, HW, C, &g.efpn_lin_wt))) return rc;
    if ((rc = upload_raw(ctx, tm, "embed_fpn.3.bias", C, &g.efpn_lin_b))) return rc;
  }
  if ((rc = upload_t(ctx, tm, "action_head.lm_heads.0.weight", nA, C, &g.head_wt))) return rc;
  if ((rc = upload_raw(ctx, tm, "transformer.ln_f.weight", C, &g.lnf_w))) return rc;
  if ((rc = upload_raw(ctx, tm, "transformer.ln_f.bias", C, &g.lnf_b))) return rc;
  g.layers.resize(c.n_layer);
  std::vector<GptLayerPtrs> lp(c.n_layer);
  for (int l = 0; l < c.n_layer; ++l) {
    const std::string p = "transformer.h." + std::to_string(l) + ".";
    GptW::Layer& L = g.layers[l];
    if ((rc = upload_raw(ctx, tm, p + "ln_1.weight", C, &L.ln1_w))) return rc;
    if ((rc = upload_raw(ctx, tm, p + "ln_1.bias", C, &L.ln1_b))) return rc;
    if ((rc = upload_t(ctx, tm, p + "attn.c_attn.weight", 3 * C, C, &L.qkv_wt))) return rc;
    if ((rc = upload_raw(ctx, tm, p + "attn.c_attn.bias", 3 * C, &L.qkv_b))) return rc;
    if ((rc = upload_t(ctx, tm, p + "attn.c_proj.weight", C, C, &L.proj_wt))) return rc;
    if ((rc = upload_raw(ctx, tm, p + "attn.c_proj.bias", C, &L.proj_b))) return rc;
    if ((rc = upload_raw(ctx, tm, p + "ln_2.weight", C, &L.ln2_w))) return rc;
    if ((rc = upload_raw(ctx, tm, p + "ln_2.bias", C, &L.ln2_b))) return rc;
    if ((rc = upload_t(ctx, tm, p + "mlp.c_fc.weight", 4 * C, C, &L.fc_wt))) return rc;
    if ((rc = upload_raw(ctx, tm, p + "mlp.c_fc.bias", 4 * C, &L.fc_b))) return rc;
    if ((rc = upload_t(ctx, tm, p + "mlp.c_proj.weight", C, 4 * C, &L.fc2_wt))) return rc;
    if ((rc = upload_raw(ctx, tm, p + "mlp.c_proj.bias", C, &L.fc2_b))) return rc;
    lp[l] = GptLayerPtrs{L.ln1_w, L.ln1_b, L.qkv_wt, L.qkv_b, L.proj_wt, L.proj_b,
                         L.ln2_w, L.ln2_b, L.fc_wt, L.fc_b, L.fc2_wt, L.fc2_b};
  }
  {
    GptLayerPtrs* d = nullptr;
    if ((rc = dev_alloc(ctx, &d, (size_t)c.n_layer))) return rc;
    JN_HIP(hipMemcpy(d, lp.data(), lp.size() * sizeof(GptLayerPtrs), hipMemcpyHostToDevice));
    ctx->layers_dev = d;
    ctx->layers_host = lp;
  }
  if (!ctx->gpt_arena_end) ctx->gpt_arena_end = ctx->arena_used;
  if ((rc = pack_net(JN_NET_DETECTOR))) return rc;
  ctx->det_head_begin = ctx->arena_used;
  for (const ParamSeg& sg : ctx->segs)
    if (sg.name.compare(0, 11, "yolox.head.") == 0) { ctx->det_head_begin = std::min(ctx->det_head_begin, sg.off); }
  JN_HIP(hipDeviceSynchronize());
  ctx->weights_loaded = true;
  return JN_OK;
}

int jn_read_tensor(jn_ctx* ctx, const char* name, float* host_out, size_t numel) {
  JN_CHECK(ctx && name && host_out, JN_EINVAL, "jn_read_tensor: null argument");
  JN_CHECK(ctx->weights_loaded, JN_ESTATE, "jn_load_weights has not been called");
  JN_HIP(hipSetDevice(ctx->cfg.device));
  const std::string nm(name);
  for (int ni = 0; ni < 2; ++ni) {
    if (!ctx->has_net[ni]) continue;
    for (const ConvW& cw : ctx->nets[ni].convs) {
      if (!cw.has_bn) continue;
      // a merged pair answers for both of its modules: [0, cout_first) and [cout_first, cout)
      const bool first = nm.compare(0, cw.prefix.size(), cw.prefix) == 0 && nm.size() > cw.prefix.size() && nm[cw.prefix.size()] == '.';
      const bool second = !cw.prefix2.empty() && nm.compare(0, cw.prefix2.size(), cw.prefix2) == 0 &&
                          nm.size() > cw.prefix2.size() && nm[cw.prefix2.size()] == '.';
      if (!first && !second) continue;
      const std::string leaf = nm.substr(first ? cw.prefix.size() : cw.prefix2.size());
      const float* src = leaf == ".bn.running_mean" ? cw.rmean_dev : leaf == ".bn.running_var" ? cw.rvar_dev : nullptr;
      if (!src) continue;
      int n_here = cw.cout;
      if (!cw.prefix2.empty()) { n_here = first ? cw.cout_first : cw.cout - cw.cout_first; if (second) src += cw.cout_first; }
      JN_CHECK(numel == (size_t)n_here, JN_EINVAL, "'%s' has %d elements, not %zu", name, n_here, numel);
      JN_HIP(hipDeviceSynchronize());
      JN_HIP(hipMemcpy(host_out, src, numel * sizeof(float), hipMemcpyDeviceToHost));
      return JN_OK;
    }
  }
  set_error("jn_read_tensor: '%s' is not a tensor the engine updates", name);
  return JN_ENOTFOUND;
}

int jn_read_grad(jn_ctx* ctx, const char* name, float* host_out, size_t numel) {
  JN_CHECK(ctx && name && host_out, JN_EINVAL, "jn_read_grad: null argument");
  JN_CHECK(ctx->grads, JN_ESTATE, "no gradient has been computed yet");
  JN_HIP(hipSetDevice(ctx->cfg.device));
  auto it = ctx->seg_index.find(name);
  JN_CHECK(it != ctx->seg_index.end(), JN_ENOTFOUND, "jn_read_grad: '%s' is not a trainable tensor", name);
  const ParamSeg& sg = ctx->segs[it->second];
  JN_CHECK(sg.numel == numel, JN_EINVAL, "'%s' has %zu elements, not %zu", name, sg.numel, numel);
  std::vector<float> packed(numel);
  JN_HIP(hipDeviceSynchronize());
  JN_HIP(hipMemcpy(packed.data(), ctx->grads + sg.off, numel * sizeof(float), hipMemcpyDeviceToHost));
  const std::vector<float> t = unpack_param(sg, packed);
  std::memcpy(host_out, t.data(), numel * sizeof(float));
  return JN_OK;
}

int jn_read_param(jn_ctx* ctx, const char* name, float* host_out, size_t numel) {
  JN_CHECK(ctx && name && host_out && ctx->params, JN_EINVAL, "jn_read_param: bad argument");
  JN_HIP(hipSetDevice(ctx->cfg.device));
  auto it = ctx->seg_index.find(name);
  JN_CHECK(it != ctx->seg_index.end(), JN_ENOTFOUND, "jn_read_param: '%s' is not a trainable tensor", name);
  const ParamSeg& sg = ctx->segs[it->second];
  JN_CHECK(sg.numel == numel, JN_EINVAL, "'%s' has %zu elements, not %zu", name, sg.numel, numel);
  std::vector<float> packed(numel);
  JN_HIP(hipDeviceSynchronize());
  JN_HIP(hipMemcpy(packed.data(), ctx->params + sg.off, numel * sizeof(float), hipMemcpyDeviceToHost));
  const std::vector<float> t = unpack_param(sg, packed);
  std::memcpy(host_out, t.data(), numel * sizeof(float));
  return JN_OK;
}

}  // extern "C"
