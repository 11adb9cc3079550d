// C ABI of libjnroll.so, training unit: the teacher-forced GPT forward, REINFORCE, the supervised bridge and the optimiser.
// Host code only (compiled by hipcc as C++); kernels live in kernels_*.hip.
#include <algorithm>
#include <cmath>
#include <mutex>

#include "jn_internal.h"

namespace jnr {

void fill_gpt_weights(const jn_ctx* ctx, GptStepArgs& a) {
  const jn_config& c = ctx->cfg;
  const GptW& g = ctx->gpt;
  a.C = c.n_embd; a.n_head = c.n_head; a.n_layer = c.n_layer; a.nA = c.n_actions; a.Tmax = c.block_size + 1;
  a.use_pos_emb = c.use_pos_emb; a.no_patch_emb = c.no_patch_emb; a.concat_emb = c.concat_emb;
  a.dec_pos_enc = c.decoder_pos_encoding; a.n_parts = n_parts(c);
  a.pe2_ch = (int)std::ceil(c.n_embd / 4.0) * 2;
  a.wte = g.wte; a.wpe = g.wpe; a.embed_class = g.embed_class; a.proj_wt = g.proj_wt; a.proj_b = g.proj_b;
  a.pos1d = g.pos1d; a.pe2 = g.pos2d_col; a.head_wt = g.head_wt; a.lnf_w = g.lnf_w; a.lnf_b = g.lnf_b;
  a.layers = ctx->layers_dev; a.emb_part = ctx->emb_part; a.KS = ctx->KS; a.efpn_lin_b = g.efpn_lin_b;
  a.kcache = ctx->kcache; a.vcache = ctx->vcache; a.prev_action = ctx->prev_action; a.cache_len = ctx->cache_len;
  a.n_done = ctx->n_done;
  a.wide = ctx->decision_route; a.layers_host = ctx->layers_host.data(); a.wide_scratch = ctx->wide_scratch;
  // head_wt, ln_f and the layers are packed one after the other (load_weights' order): the step kernel warms L2 with that
  // run.  Should the order ever change, the run is no longer one piece and the kernel is told nothing.
  a.pf_base = nullptr; a.pf_floats = 0;
  if (!g.layers.empty()) {
    const GptW::Layer& last = g.layers.back();
    const size_t C = c.n_embd, per_layer = 12 * C * C + 13 * C;
    const long long run = (last.fc2_b + C) - g.head_wt;
    if (run > 0 && (size_t)run <= (size_t)c.n_actions * C + 2 * C + g.layers.size() * (per_layer + 12 * 16) + 64) {
      a.pf_base = g.head_wt; a.pf_floats = run;
    }
  }
}

// the per-token buffers of a training forward (a train-mode rollout or the supervised forward) and its backward
int ensure_token_train_buffers(jn_ctx* ctx) {
  if (ctx->efpn_train) return JN_OK;
  const jn_config& c = ctx->cfg;
  const size_t MBt = (size_t)c.max_batch * c.block_size, K = (size_t)ctx->efpn_h * ctx->efpn_w * c.n_embd;
  int rc;
  if ((rc = dev_alloc(ctx, &ctx->efpn_train, MBt * K))) return rc;
  if ((rc = dev_alloc(ctx, &ctx->tok_emb_train, MBt * c.n_embd))) return rc;
  if ((rc = dev_alloc(ctx, &ctx->d_tok_emb, MBt * c.n_embd))) return rc;
  if ((rc = dev_alloc(ctx, &ctx->dlogits, MBt * c.n_actions))) return rc;
  return dev_alloc(ctx, &ctx->de_ws, MBt * K);
}

// The teacher-forced decode of GPT.forward (src/models/gpt.py:481-534) over B sequences: the class token, then tokens
// 1 .. T from (patch embedding, action, position) of the teacher's arrays [B][T]; token tok's logits go to row tok - 1 of
// logits [B][L - 1][nA] (null: none), every token's final embedding to final_emb [B][L][C] (null: none).  With prev_emb
// [B][Tp][C] (gpt.py:431-449, the recurrent form) those Tp embeddings are the prefix and only the LAST of the T tokens is
// new.  tok_emb [B][tok_emb_stride][C]: the patch embeddings of the new tokens.  pdrop / drop_seed: train-mode dropout.
static int teacher_forced_decode(jn_ctx* ctx, const int64_t* actions_dev, const int64_t* classes_dev, const int64_t* positions_dev,
                                 const float* prev_emb_dev, int B, int T, int Tp, const float* tok_emb, int tok_emb_stride,
                                 float* logits_dev, float* final_emb_dev, float pdrop, uint64_t drop_seed, hipStream_t s) {
  const int nA = ctx->cfg.n_actions, i0 = prev_emb_dev ? T - 1 : 0;
  const int L = prev_emb_dev ? Tp + 1 : T + 1;
  JN_HIP(hipMemsetAsync(ctx->cache_len, 0, (size_t)B * sizeof(int32_t), s));
  GptStepArgs a{};
  fill_gpt_weights(ctx, a);
  a.pdrop = pdrop; a.drop_seed = drop_seed;
  a.classes = classes_dev;
  a.B = B; a.T = L; a.emb_stride = L; a.out.final_emb = final_emb_dev; a.logits_stride = (L - 1) * nA;
  for (int tok = 0; tok < L; ++tok) {
    a.step = tok;
    a.logits_rows = (tok >= 1 && logits_dev) ? logits_dev + (size_t)(tok - 1) * nA : nullptr;
    if (prev_emb_dev && tok < Tp) {
      a.src_mode = GPT_SRC_GIVEN; a.given_emb = prev_emb_dev; a.given_stride = Tp; a.given_index = tok;
    } else if (!prev_emb_dev && tok == 0) {
      a.src_mode = GPT_SRC_CLASS;
    } else {
      const int i = prev_emb_dev ? 0 : tok - 1;           // index among the new tokens
      a.src_mode = GPT_SRC_TEACH;
      a.t_actions = actions_dev; a.t_positions = positions_dev; a.t_stride = T; a.t_index = i0 + i;
      a.pos_index = prev_emb_dev ? 0 : i;                 // recurrent tokens always get position 0 (gpt.py:431-449)
      a.tok_emb = tok_emb; a.tok_emb_stride = tok_emb_stride; a.tok_emb_index = i;
    }
    JN_CHECK(launch_gpt_step_routed(a, s) == 0, JN_ESTATE, "the decision step could not be launched (n_embd %d, block_size %d)", a.C, a.Tmax - 1);
  }
  return JN_OK;
}

static int build_grad_layer_table(jn_ctx* ctx) {
  if (ctx->g_layers_dev) return JN_OK;
  const int nL = ctx->cfg.n_layer;
  std::vector<GptLayerPtrs> gl(nL);
  for (int l = 0; l < nL; ++l) {
    const GptW::Layer& L = ctx->gpt.layers[l];
    gl[l] = GptLayerPtrs{grad_of(ctx, L.ln1_w), grad_of(ctx, L.ln1_b), grad_of(ctx, L.qkv_wt), grad_of(ctx, L.qkv_b),
                         grad_of(ctx, L.proj_wt), grad_of(ctx, L.proj_b), grad_of(ctx, L.ln2_w), grad_of(ctx, L.ln2_b),
                         grad_of(ctx, L.fc_wt), grad_of(ctx, L.fc_b), grad_of(ctx, L.fc2_wt), grad_of(ctx, L.fc2_b)};
  }
  GptLayerPtrs* d = nullptr;
  int rc = dev_alloc(ctx, &d, (size_t)nL);
  if (rc) return rc;
  JN_HIP(hipMemcpy(d, gl.data(), gl.size() * sizeof(GptLayerPtrs), hipMemcpyHostToDevice));
  ctx->g_layers_dev = d;
  return JN_OK;
}

// GPT backward over a trajectory: scratch + launch, a switch over gpt_backward_route (jn_kernels.h).  The scratch counts the
// per-agent kernel's term only where that kernel can run (T <= GPT_PER_AGENT_MAX_T on the per-agent route: the term grows
// with max_batch * T^2 and would dwarf the rest at long T), and the tiled form's DS buffer where that form runs.
static int launch_gpt_bwd(jn_ctx* ctx, GptBwdArgs& ba, hipStream_t s) {
  const jn_config& c = ctx->cfg;
  const int L = ba.T + 1, nL = c.n_layer, nh = c.n_head, C = c.n_embd;
  const GptBwdRoute route = gpt_backward_route(C, nh, ba.T, ctx->decision_route);
  JN_CHECK(route != GPT_BWD_NONE, JN_EINVAL, "no GPT backward takes n_embd %d, head size %d, T %d%s", C, C / nh, ba.T,
           ctx->decision_route ? " (a wide model has the LDS form alone)" : "");
  const long long per_agent = (long long)(nL + 1) * L * C + (long long)nL * (11LL * L * C + (long long)nh * L * L) +
                              12LL * L * C + (long long)nh * L * L + 4LL * C + 64;
  const bool per_agent_possible = ctx->decision_route == 0 && ba.T <= GPT_PER_AGENT_MAX_T && C <= GPT_PER_AGENT_MAX_C;
  const size_t need = std::max(per_agent_possible ? (size_t)per_agent * c.max_batch : (size_t)0,
                               gpt_backward_batched_scratch(C, nh, nL, c.n_actions, c.max_batch, ba.T, route == GPT_BWD_TILED));
  if (!ctx->gpt_bwd_scratch || ctx->gpt_bwd_scratch_floats < need) {
    int rc = dev_alloc(ctx, &ctx->gpt_bwd_scratch, need);
    if (rc) return rc;
    ctx->gpt_bwd_scratch_floats = need;
  }
  ba.scratch = ctx->gpt_bwd_scratch; ba.scratch_per_agent = per_agent;
  std::vector<GptLayerPtrs> W(nL), G(nL);
  for (int l = 0; l < nL; ++l) {
    const GptW::Layer& y = ctx->gpt.layers[l];
    W[l] = GptLayerPtrs{y.ln1_w, y.ln1_b, y.qkv_wt, y.qkv_b, y.proj_wt, y.proj_b, y.ln2_w, y.ln2_b, y.fc_wt, y.fc_b, y.fc2_wt, y.fc2_b};
    G[l] = GptLayerPtrs{grad_of(ctx, y.ln1_w), grad_of(ctx, y.ln1_b), grad_of(ctx, y.qkv_wt), grad_of(ctx, y.qkv_b),
                        grad_of(ctx, y.proj_wt), grad_of(ctx, y.proj_b), grad_of(ctx, y.ln2_w), grad_of(ctx, y.ln2_b),
                        grad_of(ctx, y.fc_wt), grad_of(ctx, y.fc_b), grad_of(ctx, y.fc2_wt), grad_of(ctx, y.fc2_b)};
  }
  switch (route) {
    case GPT_BWD_LDS:
    case GPT_BWD_TILED:
      JN_CHECK(launch_gpt_backward_batched(ba, W.data(), G.data(), s, route == GPT_BWD_TILED) == 0, JN_ESTATE,
               "the batched GPT backward refused the shape its route admitted (n_embd %d, T %d)", C, ba.T);
      return JN_OK;
    case GPT_BWD_PER_AGENT:
      launch_gpt_backward(ba, s);
      return JN_OK;
    default:
      return JN_EINVAL;
  }
}

// The GptBwdArgs fields that the REINFORCE and the supervised backward share: shapes, flags, weights and their
// gradients, the dropout of the forward, the patch embeddings of the training pass and their gradient buffer.
static void fill_gpt_bwd_common(jn_ctx* ctx, GptBwdArgs& ba) {
  const jn_config& c = ctx->cfg;
  const GptW& g = ctx->gpt;
  ba.C = c.n_embd; ba.n_head = c.n_head; ba.n_layer = c.n_layer; ba.nA = c.n_actions;
  ba.use_pos_emb = c.use_pos_emb; ba.no_patch_emb = c.no_patch_emb; ba.concat_emb = c.concat_emb;
  ba.dec_pos_enc = c.decoder_pos_encoding; ba.pe2_ch = (int)std::ceil(c.n_embd / 4.0) * 2;
  ba.n_done = ctx->n_done; ba.dlogits = ctx->dlogits; ba.tok_emb = ctx->tok_emb_train; ba.d_tok_emb = ctx->d_tok_emb;
  ba.wte = g.wte; ba.wpe = g.wpe; ba.proj_wt = g.proj_wt; ba.pos1d = g.pos1d; ba.pe2 = g.pos2d_col; ba.head_wt = g.head_wt;
  ba.lnf_w = g.lnf_w; ba.lnf_b = g.lnf_b; ba.layers = ctx->layers_dev; ba.g_layers = ctx->g_layers_dev;
  ba.g_wte = grad_of(ctx, g.wte); ba.g_wpe = g.wpe ? grad_of(ctx, g.wpe) : nullptr;
  ba.g_embed_class = grad_of(ctx, g.embed_class);
  ba.g_proj_wt = g.proj_wt ? grad_of(ctx, g.proj_wt) : nullptr; ba.g_proj_b = g.proj_b ? grad_of(ctx, g.proj_b) : nullptr;
  ba.g_head_wt = grad_of(ctx, g.head_wt); ba.g_lnf_w = grad_of(ctx, g.lnf_w); ba.g_lnf_b = grad_of(ctx, g.lnf_b);
  ba.pdrop = ctx->pdrop; ba.drop_seed = ctx->drop_seed_used; ba.Tmax = c.block_size + 1;
}

// The patch-encoder side of a training backward over g_n workspace slots of `rows` patches from slot `slot` (gradient
// slots 0 .. g_n - 1), given e (embed_fpn.0 activations) and dpe (d loss / d patch embedding) of those g_n * rows
// patches: embed_fpn's backward, then the conv stack's.  In training only fpn[2] gets a gradient from outside the
// encoder (embed_fpn): fpn[0] and fpn[1] are zeroed and the conv stack takes the routes of fpn_zero = 0x3.
// `slot` counts activation slots; the tables and saved statistics start at table slot tab_slot (< 0: the same slot).
static int encoder_backward(jn_ctx* ctx, int g_n, int rows, int slot, const float* e, const float* dpe, const StemSrc& ss,
                            long long pos_slot_stride, hipStream_t s, int tab_slot = -1) {
  if (tab_slot < 0) tab_slot = slot;
  const int C = ctx->cfg.n_embd, MB = ctx->cfg.max_batch, HW = ctx->efpn_h * ctx->efpn_w, K = HW * C;
  const GptW& g = ctx->gpt;
  Net& net = ctx->nets[ctx->enc_net];
  const View& f2 = net.fpn[2];
  const ChanTab ident{ctx->ident, ctx->ident + 2048, ctx->ident + 4096};
  const long long g_slot = (long long)net.per_image_floats * MB, Mr = (long long)g_n * rows;
  // Linear backward as two GEMMs on the 1x1-conv kernels: de = dpe . W^T (then the ReLU mask), dW = e^T . dpe
  ConvArgs la2{};
  la2.in = dpe; la2.in_ld = C; la2.in_dtype = JN_F32; la2.itab = ident; la2.w = g.efpn_lin_wt; la2.bias = nullptr;
  la2.out = ctx->de_ws; la2.out_ld = K; la2.out_dtype = JN_F32; la2.bf16_mfma = 0;
  la2.N = (int)Mr; la2.H = 1; la2.W = 1; la2.OH = 1; la2.OW = 1; la2.cin = C; la2.cout = K; la2.stride = 1; la2.act = ACT_NONE;
  JN_CHECK(launch_pw(la2, s) == 0, JN_ESTATE, "backward of embed_fpn.3: no kernel for this shape, or its LDS was refused");
  launch_relu_mask(ctx->de_ws, e, Mr * K, s);
  launch_pw_bwd_weight(e, K, dpe, C, ident, grad_of(ctx, g.efpn_lin_wt), nullptr, Mr, K, C, s);
  launch_colsum_add(dpe, Mr, C, grad_of(ctx, g.efpn_lin_b), s);
  // embed_fpn.0 (1x1 conv) backward into the f2 gradient view of every slot (fp32 operands: the training entry points
  // refuse bf16 activations)
  SlotBatch sb;
  sb.n = g_n; sb.act = g_slot; sb.grad = g_slot; sb.tab = 3LL * net.tab_channels;
  ConvArgs a{};
  a.in = ctx->de_ws; a.in_ld = C; a.in_dtype = JN_F32; a.itab = ident; a.w = g.efpn_w; a.bias = nullptr;
  a.out = net.gact + net.buf_off[f2.buf] * (size_t)MB + f2.coff; a.out_ld = net.bufs[f2.buf].C; a.out_dtype = JN_F32; a.bf16_mfma = 0;
  a.N = rows; a.H = f2.H; a.W = f2.W; a.OH = f2.H; a.OW = f2.W; a.cin = C; a.cout = f2.C; a.stride = 1; a.act = ACT_NONE;
  a.accumulate = 0; a.w_transposed = 1; a.in_identity = 1;
  a.n_slots = g_n; a.in_slot_stride = (long long)rows * K; a.out_slot_stride = g_slot; a.tab_slot_stride = 0;
  // the detector's PAFPN as patch encoder is detached (src/models/gpt.py:376-380 "Do not backpropagate through
  // yolox"): the policy gradient stops at embed_fpn.0's weight
  const bool detached = ctx->enc_net == JN_NET_DETECTOR;
  JN_CHECK(detached || launch_pw(a, s) == 0, JN_ESTATE, "backward of embed_fpn.0: no kernel for this shape, or its LDS was refused");
  launch_pw_bwd_weight(ctx->de_ws, C, (const float*)view_ptr(net, slot, MB, f2), net.bufs[f2.buf].C, view_tab(net, tab_slot, f2),
                       grad_of(ctx, g.efpn_w), ctx->wpart, (long long)rows * HW, C, f2.C, s, sb, (long long)rows * K);
  if (detached) return JN_OK;
  for (int i = 0; i < 2; ++i) {
    const View& f = net.fpn[i];
    for (int j = 0; j < g_n; ++j)
      JN_HIP(hipMemsetAsync(net.gact + (size_t)j * g_slot + net.buf_off[f.buf] * (size_t)MB + f.coff, 0,
                            (size_t)rows * f.H * f.W * f.C * sizeof(float), s));
  }
  return run_net_backward(ctx, ctx->enc_net, rows, ss, slot, s, g_n, pos_slot_stride, false, 0x3, tab_slot);
}

static int check_train_outputs(const jn_rollout_out* out) {
  JN_CHECK(out->logits_dev && out->actions_dev && out->returns_dev && out->logit_masks_dev && out->positions_dev &&
               out->final_emb_dev && out->rewards_dev && out->masks_dev,
           JN_EINVAL, "training needs logits/actions/returns/logit_masks/positions/final_emb/rewards/masks outputs");
  return JN_OK;
}

// what every training entry point needs of the context
// (T: the sequence length about to be trained on, 0 when not known yet)
static int check_can_train(const jn_ctx* ctx, int T) {
  const jn_config& c = ctx->cfg;
  JN_CHECK(!c.no_patch_emb, JN_ESTATE, "training without a patch encoder is not supported");
  // a wide context has no backward but the batched one in its LDS form (gpt_backward_kernel's envelope ends at n_embd 256,
  // and the tiled form is not offered to wide models yet)
  JN_CHECK(ctx->decision_route == 0 || T < 1 || gpt_backward_batched_admits(c.n_embd, c.n_head, T), JN_EINVAL,
           "training a wide model (n_embd %d, head size %d) at T = %d: the batched backward needs n_embd <= %d and "
           "4 (T + 1) head_size + 2 (T + 1)^2 <= 16384", c.n_embd, c.n_embd / c.n_head, T, GPT_WIDE_MAX_C);
  // the length at hand must have a backward (gpt_backward_route: LDS, per agent up to T = 62, tiled up to T = 255)
  JN_CHECK(T < 1 || gpt_backward_route(c.n_embd, c.n_head, T, ctx->decision_route) != GPT_BWD_NONE, JN_EINVAL,
           "no GPT backward takes n_embd %d, head size %d, T = %d", c.n_embd, c.n_embd / c.n_head, T);
  // batch-statistics BatchNorm on bf16-rounded pre-activations is ill-conditioned (the measurement behind
  // that statement: profiles/r03_bf16_train_probe.txt)
  JN_CHECK(ctx->cfg.act_dtype == JN_F32, JN_ESTATE, "training needs act_dtype = fp32 (bf16 is the inference mode)");
  // every BatchNorm layer the conv-stack backward reduces must be one launch_bn_bwd_reduce takes: refused here, by name, not in the
  // middle of a backward (a detached encoder, enc_net == the detector, has no conv-stack backward)
  if (ctx->enc_net != JN_NET_DETECTOR)
    for (const ConvW& cw : ctx->nets[ctx->enc_net].convs)
      JN_CHECK(!cw.has_bn || (bn_bwd_reduce_admits(cw.cout) && (cw.prefix2.empty() || bn_bwd_reduce_admits(cw.cout / 2))), JN_EINVAL,
               "training: BatchNorm layer %s has %d channels; the backward takes whole quads, at most %d, and above 1024 a multiple of 8",
               cw.prefix.c_str(), cw.cout, JN_BN_BWD_MAX_C);
  return JN_OK;
}

// loss.backward() of a train-mode rollout given d loss / d logits in ctx->dlogits, in two halves.  The first, the causal
// GPT over the trajectory (teacher-forced recompute), finds the number of executed steps on the device (n_done), so the
// callers enqueue it BEFORE the host asks for that number: the host's one sync of the iteration then overlaps with the
// queued launches instead of being followed by 77 short launches against an idle GPU.
static int reinforce_backward_gpt(jn_ctx* ctx, const jn_rollout_out* out, int stop_early, hipStream_t s) {
  int rc;
  if ((rc = build_grad_layer_table(ctx))) return rc;
  const EnvState& e = ctx->env;
  const int B = e.B, T = e.T;
  GptBwdArgs ba{};
  fill_gpt_bwd_common(ctx, ba);
  ba.B = B; ba.T = T; ba.stop_early = stop_early ? 1 : 0;
  ba.final_emb = out->final_emb_dev; ba.actions = out->actions_dev;
  ba.positions = out->positions_dev; ba.pos_tokens = T + 1; ba.pos1d_by_token = 0; ba.tok_actions = nullptr;
  ba.classes = ctx->classes_used_n ? ctx->classes_used : nullptr;    // the ids the rollout ran with, not the setter's
  ba.dte_stride_b = 1; ba.dte_stride_t = B;          // [T][B][C]: the rows of one glimpse step are contiguous
  return launch_gpt_bwd(ctx, ba, s);
}

// Where the forward of glimpse step t of the rollout behind `out` read its B patches: the walk's own positions (column t
// of positions [B][T + 1][2]) over the env's images, or, in view mode, staged column t.
static StemSrc rollout_step_src(const jn_ctx* ctx, const jn_rollout_out* out, int t) {
  const EnvState& e = ctx->env;
  if (e.view_mode) return stage_stem_src(e, ctx->cfg.patch_size, t);
  StemSrc ss = env_stem_src(e, out->positions_dev + 2 * t);
  ss.pos_stride = 2 * (e.T + 1);
  return ss;
}

// The second half needs S on the host: embed_fpn, then the patch encoder of all S executed glimpse steps, step-batched.
static int reinforce_backward_encoder(jn_ctx* ctx, const jn_rollout_out* out, int S, hipStream_t s) {
  int rc;
  const jn_config& c = ctx->cfg;
  const EnvState& e = ctx->env;
  const int B = e.B, T = e.T, C = c.n_embd, K = ctx->efpn_h * ctx->efpn_w * C;
  // patch-encoder side: all executed glimpse steps in ONE set of launches (chunks of net.g_slots steps
  // when the gradient buffers of a whole trajectory do not fit): embed_fpn backward, then the PAFPN.
  if (ctx->profiling && ctx->ev[2]) JN_HIP(hipEventRecord(ctx->ev[2], s));     // conv-stack backward section (bench.py)
  // (a detached encoder needs no gradient slots: all steps in one chunk)
  const bool detached = ctx->enc_net == JN_NET_DETECTOR;
  const int ring = detached ? 0 : ctx->train_ring;
  std::vector<int> c_t0(std::max(S, 1)), c_n(std::max(S, 1));
  const int n_chunks = jn_replay_chunks(S, ring, detached ? std::max(S, 1) : ctx->nets[ctx->enc_net].g_slots, c_t0.data(), c_n.data(), (int)c_t0.size());
  if (n_chunks < 0) return n_chunks;
  ctx->replayed_steps = 0;
  JN_CHECK(!ring || !e.view_mode || (e.stage && e.stage_cols == T + 1), JN_ESTATE, "the staged patches of the rollout are gone");
  for (int ci = 0; ci < n_chunks; ++ci) {
    const int t0 = c_t0[ci], k = c_n[ci];
    // under a ring the chunk's steps are run again, from what their table slots kept, into activation slots 1 .. k
    for (int j = 0; ring && j < k; ++j) {
      if ((rc = run_net(ctx, ctx->enc_net, B, rollout_step_src(ctx, out, t0 + j), 1 + j, 1, nullptr, 0, s, false, 0, t0 + j + 1, RUN_REPLAY))) return rc;
      ++ctx->replayed_steps;
    }
    StemSrc ss = env_stem_src(e, out->positions_dev + 2 * t0);
    ss.pos_stride = 2 * (T + 1);
    long long pos_slot = 2;
    if (e.view_mode) {
      // the staged columns t0 ... are one contiguous run of plain patches [step][agent]; the stem's weight gradient
      // steps from pass to pass through its position operand, so the table stage_pos names column t as "P-row 3 B t"
      JN_CHECK(e.stage && e.stage_cols == T + 1, JN_ESTATE, "the staged patches of the rollout are gone");
      ss = stage_stem_src(e, c.patch_size, 0);
      ss.positions = e.stage_pos + (size_t)t0 * B * 2;
      pos_slot = 2LL * B;
    }
    if ((rc = encoder_backward(ctx, k, B, ring ? 1 : t0 + 1, ctx->efpn_train + (size_t)t0 * B * K, ctx->d_tok_emb + (size_t)t0 * B * C, ss,
                               pos_slot, s, t0 + 1)))
      return rc;
  }
  if (ctx->profiling && ctx->ev[3]) { JN_HIP(hipEventRecord(ctx->ev[3], s)); ctx->bwd_timed = true; }
  JN_HIP(hipGetLastError());
  return JN_OK;
}

// Teacher-forced (supervised) step, src/supervised.py:863-902 with the detector term off, in two halves so that the
// reference's own loop can sit between them (GPT.forward -> its CE loss -> loss.backward(), the supervised autograd
// bridge): the forward runs GPT.forward on the full sequence (B*T patches through the encoder in ONE train-mode pass,
// 1-D positions 0..T-1) and leaves the logits in ctx->sup_logits; the backward takes d loss / d logits in ctx->dlogits.
static int supervised_forward_impl(jn_ctx* ctx, const float* patches_dev, const int64_t* current_actions_dev,
                                   const int64_t* classes_dev, const int64_t* positions_dev, int B, int T, float* logits_out_dev,
                                   float* final_emb_out_dev, hipStream_t s) {
  JN_CHECK(ctx->weights_loaded, JN_ESTATE, "jn_load_weights has not been called");
  const jn_config& c = ctx->cfg;
  int rc;
  if ((rc = check_can_train(ctx, T))) return rc;
  JN_CHECK(T >= 1 && T <= c.block_size, JN_EINVAL, "sequence length %d out of range", T);
  JN_CHECK(B >= 1 && B * T <= c.max_batch, JN_EINVAL, "B*T = %d patches exceed max_batch = %d", B * T, c.max_batch);
  JN_CHECK(!c.use_pos_emb || positions_dev, JN_EINVAL, "positions are required when use_pos_emb is set");
  JN_HIP(hipSetDevice(c.device));
  ctx->train_out_valid = false;     // the per-token training buffers (efpn_train, tok_emb_train, dropout seed) are reused
  if ((rc = ensure_train_state(ctx))) return rc;
  if ((rc = build_grad_layer_table(ctx))) return rc;
  const int C = c.n_embd, nA = c.n_actions, N = B * T, L = T + 1;
  if ((rc = ensure_token_train_buffers(ctx))) return rc;
  if (!ctx->sup_final_emb) {
    if ((rc = dev_alloc(ctx, &ctx->sup_final_emb, (size_t)c.max_batch * (c.block_size + 1) * C))) return rc;
    if ((rc = dev_alloc(ctx, &ctx->sup_logits, (size_t)c.max_batch * c.block_size * nA))) return rc;
  }
  // ---- forward: encoder over all B*T patches at once (BN statistics over B*T) ----
  if ((rc = embed_tokens(ctx, patch_src(patches_dev, c.patch_size), N, 1, ctx->efpn_train, ctx->tok_emb_train, C, s))) return rc;
  ctx->drop_seed_used = ctx->drop_seed + ctx->drop_ctr++;
  if ((rc = teacher_forced_decode(ctx, current_actions_dev, classes_dev, positions_dev, nullptr, B, T, 0, ctx->tok_emb_train, T,
                                  ctx->sup_logits, ctx->sup_final_emb, ctx->pdrop, ctx->drop_seed_used, s)))
    return rc;
  if (logits_out_dev)
    JN_HIP(hipMemcpyAsync(logits_out_dev, ctx->sup_logits, (size_t)N * nA * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (final_emb_out_dev)
    JN_HIP(hipMemcpyAsync(final_emb_out_dev, ctx->sup_final_emb, (size_t)B * L * C * sizeof(float), hipMemcpyDeviceToDevice, s));
  ctx->sup = {patches_dev, current_actions_dev, positions_dev, classes_dev, B, T};
  ctx->sup_valid = true;      // (the encoder pass over slot 0 inside embed_tokens cleared it: set last)
  JN_HIP(hipGetLastError());
  return JN_OK;
}

// backward of the forward above for d loss / d logits [B][T][nA] in ctx->dlogits
static int supervised_backward_impl(jn_ctx* ctx, hipStream_t s) {
  JN_CHECK(ctx->sup_valid, JN_ESTATE,
           "the activations of the supervised forward were overwritten (another pass used the encoder's workspace) or no forward ran");
  const int B = ctx->sup.B, T = ctx->sup.T, P = ctx->cfg.patch_size;
  int rc;
  GptBwdArgs ba{};
  fill_gpt_bwd_common(ctx, ba);
  ba.B = B; ba.T = T; ba.stop_early = 0;
  ba.final_emb = ctx->sup_final_emb; ba.actions = ctx->sup.actions;
  ba.tok_actions = ctx->sup.actions; ba.positions = ctx->sup.positions; ba.pos_tokens = T; ba.pos1d_by_token = 1;
  ba.classes = ctx->sup.classes;
  ba.dte_stride_b = T; ba.dte_stride_t = 1;
  if ((rc = launch_gpt_bwd(ctx, ba, s))) return rc;
  // the encoder's B*T patches as one slot
  if ((rc = encoder_backward(ctx, 1, B * T, 0, ctx->efpn_train, ctx->d_tok_emb, patch_src(ctx->sup.patches, P), 0, s))) return rc;
  JN_HIP(hipGetLastError());
  return JN_OK;
}

// ---- arena <-> reference layout on the device (autograd bridge: param.data / param.grad of the Python module are
// views of ONE reference-layout buffer whose segment offsets equal the arena's) ---------------------------------------
static int ensure_segs_dev(jn_ctx* ctx) {
  if (ctx->segs_dev && ctx->segs_dev_n == (int)ctx->segs.size()) return JN_OK;
  std::vector<ArenaSeg> h(ctx->segs.size());
  for (size_t i = 0; i < h.size(); ++i) {
    const ParamSeg& g = ctx->segs[i];
    h[i] = ArenaSeg{(long long)g.off, (long long)g.numel, g.kind, g.d0, g.d1, g.d2};
  }
  ArenaSeg* d = nullptr;
  int rc = dev_alloc(ctx, &d, h.size());
  if (rc) return rc;
  JN_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(ArenaSeg), hipMemcpyHostToDevice));
  ctx->segs_dev = d; ctx->segs_dev_n = (int)h.size();
  return JN_OK;
}

static int arena_copy(jn_ctx* ctx, int what, float* ref_dev, size_t numel, int to_ref, int accumulate, void* stream) {
  JN_CHECK(ctx && ref_dev && ctx->weights_loaded, JN_ESTATE, "jn_load_weights has not been called");
  JN_CHECK(what >= 0 && what <= 3, JN_EINVAL, "what: 0 = parameters, 1 = gradients, 2 / 3 = AdamW first / second moments");
  JN_CHECK(numel >= ctx->arena_used, JN_EINVAL, "reference-layout buffer needs %zu floats, got %zu", ctx->arena_used, numel);
  JN_HIP(hipSetDevice(ctx->cfg.device));
  int rc;
  if (what >= 1 && (rc = ensure_train_state(ctx))) return rc;
  if ((rc = ensure_segs_dev(ctx))) return rc;
  float* arena = what == 0 ? ctx->params : what == 1 ? ctx->grads : what == 2 ? ctx->adam_m : ctx->adam_v;
  launch_arena_copy(ctx->segs_dev, ctx->segs_dev_n, arena, ref_dev, (long long)ctx->arena_used, to_ref, accumulate,
                    (hipStream_t)stream);
  JN_HIP(hipGetLastError());
  if (!to_ref && what == 0) mark_params_written(ctx);
  return JN_OK;
}

}  // namespace jnr

using namespace jnr;

extern "C" {

int jn_gpt_forward(jn_ctx* ctx, const float* patches_dev, const int64_t* actions_dev, const int64_t* classes_dev,
                   const int64_t* positions_dev, const float* prev_emb_dev, int B, int T, int Tp, float* logits_dev,
                   float* final_emb_dev, void* stream) {
  JN_CHECK(ctx && actions_dev, JN_EINVAL, "jn_gpt_forward: null argument");
  JN_CHECK(ctx->weights_loaded, JN_ESTATE, "jn_load_weights has not been called");
  const jn_config& c = ctx->cfg;
  JN_CHECK(B >= 1 && B <= c.max_batch, JN_EINVAL, "B=%d exceeds max_batch=%d", B, c.max_batch);
  // gpt.py:514-518
  JN_CHECK(T >= 1 && T <= c.block_size, JN_EINVAL, "Cannot forward sequence of length %d, block size is only %d", T,
           c.block_size);
  JN_CHECK(!c.use_pos_emb || positions_dev, JN_EINVAL, "positions are required when use_pos_emb is set");
  JN_CHECK(c.no_patch_emb || patches_dev, JN_EINVAL, "patches are required unless no_patch_emb is set");
  JN_CHECK(!prev_emb_dev || (Tp >= 1 && Tp + 1 <= c.block_size + 1), JN_EINVAL, "prev_embeddings length %d out of range", Tp);
  JN_HIP(hipSetDevice(c.device));
  hipStream_t s = (hipStream_t)stream;
  const int C = c.n_embd, P = c.patch_size;
  const int n_new = prev_emb_dev ? 1 : T, i0 = prev_emb_dev ? T - 1 : 0;
  int rc;
  if (!c.no_patch_emb) {
    if (!ctx->tok_emb) {
      if ((rc = dev_alloc(ctx, &ctx->tok_emb, (size_t)c.max_batch * (c.block_size + 1) * C))) return rc;
    }
    for (int i = 0; i < n_new; ++i) {
      // token i0 + i of every sequence: B patches T apart, their embeddings n_new rows apart
      const StemSrc ss = patch_src(patches_dev + (size_t)(i0 + i) * 3 * P * P, P, (long long)T * 3 * P * P);
      if ((rc = embed_tokens(ctx, ss, B, 0, nullptr, ctx->tok_emb + (size_t)i * C, (long long)n_new * C, s))) return rc;
    }
  }
  if ((rc = teacher_forced_decode(ctx, actions_dev, classes_dev, positions_dev, prev_emb_dev, B, T, Tp, ctx->tok_emb, n_new,
                                  logits_dev, final_emb_dev, 0.0f, 0, s)))
    return rc;
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_zero_grad(jn_ctx* ctx, void* stream) {
  JN_CHECK(ctx && ctx->weights_loaded, JN_ESTATE, "jn_load_weights has not been called");
  JN_HIP(hipSetDevice(ctx->cfg.device));
  int rc = ensure_train_state(ctx);
  if (rc) return rc;
  JN_HIP(hipMemsetAsync(ctx->grads, 0, ctx->arena_size * sizeof(float), (hipStream_t)stream));
  return JN_OK;
}

// ---- REINFORCE iteration ------------------------------------------------------------------
int jn_arena_info(jn_ctx* ctx, size_t* total_numel, size_t* optim_gpt_numel) {
  JN_CHECK(ctx && ctx->weights_loaded, JN_ESTATE, "jn_load_weights has not been called");
  if (total_numel) *total_numel = ctx->arena_size;
  if (optim_gpt_numel) *optim_gpt_numel = ctx->gpt_arena_end;
  return JN_OK;
}

int jn_set_grad_arena(jn_ctx* ctx, float* grads_dev, size_t numel) {
  JN_CHECK(ctx && grads_dev && ctx->weights_loaded, JN_ESTATE, "jn_load_weights has not been called");
  JN_CHECK(numel >= ctx->arena_size, JN_EINVAL, "gradient arena needs %zu floats, got %zu", ctx->arena_size, numel);
  JN_HIP(hipSetDevice(ctx->cfg.device));
  int rc = ensure_train_state(ctx);
  if (rc) return rc;
  ctx->grads = grads_dev;         // caller-owned (e.g. a torch tensor handed to RCCL all-reduce)
  ctx->g_layers_dev = nullptr;    // gradient pointer table must be rebuilt
  return JN_OK;
}

// Autograd bridge (SURVEY.md §8b "jn_rollout_backward"): the train-mode rollout alone ...
int jn_reinforce_forward(jn_ctx* ctx, int mode, const int64_t* forced_actions_dev, const int64_t* start_positions_dev,
                         uint64_t seed, int stop_early, const jn_rollout_out* out, void* stream) {
  JN_CHECK(ctx && out, JN_EINVAL, "jn_reinforce_forward: null argument");
  int rc;
  if ((rc = check_train_outputs(out)) || (rc = check_can_train(ctx, ctx->env.ready ? ctx->env.T : 0))) return rc;
  if ((rc = rollout_impl(ctx, mode, forced_actions_dev, start_positions_dev, seed, 0, stop_early, out, 1, stream))) return rc;
  ctx->train_out = *out; ctx->train_out_valid = true;
  return JN_OK;
}

// ... and its backward for GIVEN upstream gradients of the rollout's logprobs / entropies [B, T] (what torch autograd
// hands to the rollout node when the caller differentiates any loss built from them, src/reinforce.py:217-265, 341).
int jn_reinforce_backward(jn_ctx* ctx, const float* dlogprobs_dev, const float* dentropies_dev, void* stream) {
  JN_CHECK(ctx && (dlogprobs_dev || dentropies_dev), JN_EINVAL, "jn_reinforce_backward: null argument");
  JN_CHECK(ctx->train_out_valid, JN_ESTATE, "jn_reinforce_backward needs a preceding jn_reinforce_forward / jn_reinforce_step");
  JN_HIP(hipSetDevice(ctx->cfg.device));
  hipStream_t s = (hipStream_t)stream;
  const jn_rollout_out* out = &ctx->train_out;
  const EnvState& e = ctx->env;
  int S = 0, rc;
  launch_logits_grad(out->logits_dev, out->actions_dev, dlogprobs_dev, dentropies_dev, ctx->n_done, ctx->dlogits, e.B, e.T,
                     ctx->cfg.n_actions, ctx->last_stop_early ? 1 : 0, s, ctx->train_mask_policy ? ctx->mask_sets : nullptr);
  if ((rc = rollout_steps_begin(ctx, s))) return rc;
  if ((rc = reinforce_backward_gpt(ctx, out, ctx->last_stop_early ? 1 : 0, s))) return rc;
  if ((rc = rollout_steps_end(ctx, &S))) return rc;
  return reinforce_backward_encoder(ctx, out, S, s);
}

int jn_reinforce_step(jn_ctx* ctx, int mode, const int64_t* forced_actions_dev, const int64_t* start_positions_dev,
                      uint64_t seed, int stop_early, const jn_train_opts* opts, const jn_rollout_out* out,
                      float* metrics_dev, void* stream) {
  JN_CHECK(ctx && opts && out && metrics_dev, JN_EINVAL, "jn_reinforce_step: null argument");
  JN_CHECK(opts->struct_size == (int)sizeof(jn_train_opts), JN_EINVAL, "jn_train_opts.struct_size mismatch");
  int rc;
  if ((rc = check_train_outputs(out)) || (rc = check_can_train(ctx, ctx->env.ready ? ctx->env.T : 0))) return rc;
  hipStream_t s = (hipStream_t)stream;
  rc = rollout_impl(ctx, mode, forced_actions_dev, start_positions_dev, seed, 0, stop_early, out, 1, stream);
  if (rc) return rc;
  ctx->train_out = *out; ctx->train_out_valid = true;
  const EnvState& e = ctx->env;
  const int B = e.B, T = e.T, nA = ctx->cfg.n_actions;
  LossArgs la{};
  la.logits = out->logits_dev; la.actions = out->actions_dev; la.returns = out->returns_dev; la.rewards = out->rewards_dev;
  la.logit_masks = out->logit_masks_dev; la.n_done = ctx->n_done; la.dlogits = ctx->dlogits; la.metrics = metrics_dev;
  la.B = B; la.T = T; la.nA = nA; la.stop_early = stop_early ? 1 : 0; la.reward_norm = opts->reward_norm;
  la.ret_mean = opts->ret_mean; la.ret_std = opts->ret_std; la.entropy_weight = opts->entropy_weight;
  la.scale = opts->loss_scale;
  la.sets = ctx->train_mask_policy ? ctx->mask_sets : nullptr;      // the sets this rollout decided under
  if ((rc = rollout_steps_begin(ctx, s))) return rc;           // n_done on its way to the host ...
  launch_reinforce_loss(la, s);
  if ((rc = reinforce_backward_gpt(ctx, out, stop_early, s))) return rc;
  int S = 0;
  if ((rc = rollout_steps_end(ctx, &S))) return rc;             // ... the one host wait of the iteration: the GPU runs the queued GPT backward meanwhile
  return reinforce_backward_encoder(ctx, out, S, s);
}

// One supervised (teacher-forced) training step minus the optimiser: forward, CrossEntropy(weight[STOP] = stop_weight)
// over non-padding tokens, backward.
int jn_supervised_step(jn_ctx* ctx, const float* patches_dev, const int64_t* current_actions_dev,
                       const int64_t* next_actions_dev, const int64_t* classes_dev, const int64_t* positions_dev,
                       const uint8_t* masks_dev, int B, int T, float stop_weight, float* logits_out_dev, float* metrics_dev,
                       void* stream) {
  JN_CHECK(ctx && patches_dev && current_actions_dev && next_actions_dev && masks_dev && metrics_dev, JN_EINVAL,
           "jn_supervised_step: null argument");
  hipStream_t s = (hipStream_t)stream;
  int rc = supervised_forward_impl(ctx, patches_dev, current_actions_dev, classes_dev, positions_dev, B, T, logits_out_dev, nullptr, s);
  if (rc) return rc;
  launch_ce_loss(ctx->sup_logits, next_actions_dev, masks_dev, stop_weight, ctx->dlogits, metrics_dev, B * T, ctx->cfg.n_actions, T, s);
  return supervised_backward_impl(ctx, s);
}

// Supervised autograd bridge: GPT.forward(patches [B,T,3,P,P], actions [B,T], classes = 0, positions [B,T,2]) in train
// mode (src/models/gpt.py:481-534 as called by src/supervised.py:863-868) -> logits [B,T,nA], final_emb [B,T+1,C].  The
// input buffers must stay alive until jn_supervised_backward.
int jn_supervised_forward(jn_ctx* ctx, const float* patches_dev, const int64_t* current_actions_dev, const int64_t* classes_dev,
                          const int64_t* positions_dev, int B, int T, float* logits_out_dev, float* final_emb_out_dev, void* stream) {
  JN_CHECK(ctx && patches_dev && current_actions_dev && logits_out_dev, JN_EINVAL, "jn_supervised_forward: null argument");
  return supervised_forward_impl(ctx, patches_dev, current_actions_dev, classes_dev, positions_dev, B, T, logits_out_dev,
                                 final_emb_out_dev, (hipStream_t)stream);
}

// ... and its backward for GIVEN d loss / d logits [B,T,nA] (what torch hands to the logits node when the caller's
// loss.backward() runs, src/supervised.py:897): parameter gradients accumulate in the gradient arena.
int jn_supervised_backward(jn_ctx* ctx, const float* dlogits_dev, void* stream) {
  JN_CHECK(ctx && dlogits_dev, JN_EINVAL, "jn_supervised_backward: null argument");
  JN_CHECK(ctx->sup_valid, JN_ESTATE,
           "jn_supervised_backward: no supervised forward to differentiate (none ran, or a later pass overwrote its activations)");
  JN_HIP(hipSetDevice(ctx->cfg.device));
  hipStream_t s = (hipStream_t)stream;
  JN_HIP(hipMemcpyAsync(ctx->dlogits, dlogits_dev, (size_t)ctx->sup.B * ctx->sup.T * ctx->cfg.n_actions * sizeof(float),
                        hipMemcpyDeviceToDevice, s));
  return supervised_backward_impl(ctx, s);
}

// The validation twin of jn_supervised_step (eval_supervised, src/supervised.py:442-472): GPT.forward in eval mode on the
// teacher's sequences, then the loss / accuracy of compute_metrics.  In eval mode a patch's embedding does not depend
// on its batch, so the encoder walks the B*T patches in flattened (b t) order in chunks of max_batch and every chunk's
// embeddings land at their place in the [B][T][C] token buffer the decode reads.
int jn_supervised_eval(jn_ctx* ctx, const float* patches_dev, const int64_t* current_actions_dev, const int64_t* next_actions_dev,
                       const int64_t* classes_dev, const int64_t* positions_dev, const uint8_t* masks_dev, int B, int T,
                       float stop_weight, int on_self_trajectory, float* logits_out_dev, float* token_loss_out_dev,
                       uint8_t* predicted_out_dev, float* metrics_dev, void* stream) {
  JN_CHECK(ctx && current_actions_dev && next_actions_dev && masks_dev && metrics_dev, JN_EINVAL, "jn_supervised_eval: null argument");
  JN_CHECK(ctx->weights_loaded, JN_ESTATE, "jn_load_weights has not been called");
  const jn_config& c = ctx->cfg;
  JN_CHECK(B >= 1 && B <= c.max_batch, JN_EINVAL, "B=%d exceeds max_batch=%d", B, c.max_batch);
  JN_CHECK(T >= 1 && T <= c.block_size, JN_EINVAL, "Cannot forward sequence of length %d, block size is only %d", T, c.block_size);
  JN_CHECK(!c.use_pos_emb || positions_dev, JN_EINVAL, "positions are required when use_pos_emb is set");
  JN_CHECK(c.no_patch_emb || patches_dev, JN_EINVAL, "patches are required unless no_patch_emb is set");
  JN_HIP(hipSetDevice(c.device));
  hipStream_t s = (hipStream_t)stream;
  const int C = c.n_embd, P = c.patch_size, nA = c.n_actions, N = B * T;
  int rc;
  if (!ctx->eval_logits && !logits_out_dev)
    if ((rc = dev_alloc(ctx, &ctx->eval_logits, (size_t)c.max_batch * c.block_size * nA))) return rc;
  float* logits = logits_out_dev ? logits_out_dev : ctx->eval_logits;
  if (!c.no_patch_emb) {
    if (!ctx->tok_emb)
      if ((rc = dev_alloc(ctx, &ctx->tok_emb, (size_t)c.max_batch * (c.block_size + 1) * C))) return rc;
    for (int n0 = 0; n0 < N; n0 += c.max_batch) {
      const int n = std::min(c.max_batch, N - n0);
      if ((rc = embed_tokens(ctx, patch_src(patches_dev + (size_t)n0 * 3 * P * P, P), n, 0, nullptr, ctx->tok_emb + (size_t)n0 * C, C, s)))
        return rc;
    }
  }
  if ((rc = teacher_forced_decode(ctx, current_actions_dev, classes_dev, positions_dev, nullptr, B, T, 0, ctx->tok_emb, T, logits, nullptr,
                                  0.0f, 0, s)))
    return rc;
  launch_supervised_metrics(logits, current_actions_dev, next_actions_dev, masks_dev, B, T, nA, stop_weight,
                            on_self_trajectory ? 1 : 0, token_loss_out_dev, predicted_out_dev, metrics_dev, s);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

// ---- the chunks of the encoder's backward (host rule, no device) and the replay check -------------------------------------
int jn_replay_chunks(int S, int act_slots, int g_slots, int* t0, int* n, int cap) {
  JN_CHECK(S >= 0 && act_slots >= 0 && g_slots >= 1 && cap >= 0 && ((t0 && n) || cap == 0), JN_EINVAL,
           "jn_replay_chunks: S=%d act_slots=%d g_slots=%d cap=%d", S, act_slots, g_slots, cap);
  const int chunk = act_slots ? std::min(act_slots, g_slots) : g_slots;
  int count = 0;
  for (int at = 0; at < S; at += chunk, ++count)
    if (count < cap) { t0[count] = at; n[count] = std::min(chunk, S - at); }
  return count;
}

int jn_debug_replay_diff(jn_ctx* ctx, int step, long long* n_diff, void* stream) {
  JN_CHECK(ctx && n_diff, JN_EINVAL, "jn_debug_replay_diff: null argument");
  JN_CHECK(ctx->train_out_valid, JN_ESTATE, "jn_debug_replay_diff needs a preceding train-mode rollout (jn_reinforce_forward / jn_reinforce_step)");
  JN_CHECK(ctx->enc_net != JN_NET_DETECTOR && ctx->train_ring == 0, JN_ESTATE,
           "jn_debug_replay_diff compares against resident steps: a patch encoder of its own and jn_set_activation_slots 0");
  JN_HIP(hipSetDevice(ctx->cfg.device));
  hipStream_t s = (hipStream_t)stream;
  int S = 0, rc;
  if ((rc = rollout_steps_begin(ctx, s)) || (rc = rollout_steps_end(ctx, &S))) return rc;
  JN_CHECK(step >= 0 && step < S, JN_EINVAL, "jn_debug_replay_diff: step %d of %d executed steps", step, S);
  const EnvState& e = ctx->env;
  JN_CHECK(!e.view_mode || (e.stage && e.stage_cols == e.T + 1), JN_ESTATE, "the staged patches of the rollout are gone");
  Net& net = ctx->nets[ctx->enc_net];
  // (activation slot 0 is the eval workspace: run_net's replay mode marks what it held as gone)
  if ((rc = run_net(ctx, ctx->enc_net, e.B, rollout_step_src(ctx, &ctx->train_out, step), 0, 1, nullptr, 0, s, false, 0, step + 1, RUN_REPLAY)))
    return rc;
  return replay_slot_diff(ctx, net, 0, step + 1, e.B, n_diff, s);
}

// ---- the GPT backward's route and its attention kernels alone (context-free) -------------------------------------------
int jn_gpt_backward_route(int C, int n_head, int T, int decision_route) {
  JN_CHECK(decision_route == 0 || decision_route == 1, JN_EINVAL, "jn_gpt_backward_route: decision_route=%d", decision_route);
  return (int)gpt_backward_route(C, n_head, T, decision_route);
}

int jn_gpt_attention_backward(int form, const float* QKV_dev, const float* dY_dev, int B, int n_head, int C, int Lm, int L, float pdrop,
                              uint64_t seed, int layer, int Tmax, float* ATT_dev, float* Y_dev, float* dQKV_dev, void* stream) {
  JN_CHECK(QKV_dev && dY_dev && ATT_dev && Y_dev && dQKV_dev, JN_EINVAL, "jn_gpt_attention_backward: null argument");
  JN_CHECK((form == 0 || form == 1) && B >= 1 && B <= 65535 && n_head >= 1 && C >= 1 && C % n_head == 0 && Lm >= 1 && Lm <= 4096 &&
               L >= 1 && L <= Lm && Tmax >= Lm && layer >= 0 && pdrop >= 0.0f && pdrop < 1.0f &&
               (long long)B * n_head <= 0x7fffffffLL / ((long long)3 * C * Lm),
           JN_EINVAL, "jn_gpt_attention_backward: form %d, B %d, n_head %d, C %d, Lm %d, L %d, Tmax %d, layer %d, pdrop %g", form, B,
           n_head, C, Lm, L, Tmax, layer, (double)pdrop);
  hipStream_t s = (hipStream_t)stream;
  // Workspace: the device copy of L, then (tiled form) DS, one buffer of ATT's shape.  It is kept from call to call, one per
  // device, and grows when a call needs more (which waits for the device), so that a timed call is launches alone; calls
  // on one device are therefore for one stream at a time.
  static std::mutex mu;
  static float* ws_of[64];
  static size_t ws_floats_of[64];
  int dev = 0;
  JN_HIP(hipGetDevice(&dev));
  JN_CHECK(dev >= 0 && dev < 64, JN_EINVAL, "jn_gpt_attention_backward: device %d", dev);
  const size_t ws_floats = 16 + (form == 1 ? (size_t)B * n_head * Lm * Lm : 0);
  std::lock_guard<std::mutex> lock(mu);
  if (ws_floats_of[dev] < ws_floats) {
    if (ws_of[dev]) JN_HIP(hipFree(ws_of[dev]));
    ws_of[dev] = nullptr; ws_floats_of[dev] = 0;
    JN_HIP(hipMalloc((void**)&ws_of[dev], ws_floats * sizeof(float)));
    ws_floats_of[dev] = ws_floats;
  }
  float* ws = ws_of[dev];
  JN_HIP(hipMemsetD32Async((hipDeviceptr_t)ws, L, 1, s));
  JN_CHECK(launch_gpt_attention(form, QKV_dev, dY_dev, B, n_head, C, Lm, reinterpret_cast<const int*>(ws), pdrop, seed, layer, Tmax,
                                ATT_dev, Y_dev, ws + 16, dQKV_dev, s) == 0,
           JN_EINVAL, "jn_gpt_attention_backward: the %s form does not take head size %d at Lm = %d", form ? "tiled" : "LDS",
           C / n_head, Lm);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_optimizer_step(jn_ctx* ctx, float lr, float weight_decay, float clip_value, float grad_scale, void* stream) {
  return jn_optimizer_step_group(ctx, 0, lr, weight_decay, clip_value, grad_scale, stream);
}

int jn_optimizer_step_group(jn_ctx* ctx, int group, float lr, float weight_decay, float clip_value, float grad_scale,
                            void* stream) {
  JN_CHECK(ctx && ctx->grads, JN_ESTATE, "no gradients: run jn_reinforce_step / jn_detector_step first");
  JN_CHECK(group == 0 || group == 1, JN_EINVAL, "parameter group %d: 0 = optim_gpt, 1 = optim_yolox", group);
  JN_HIP(hipSetDevice(ctx->cfg.device));
  // a frozen detector backbone (requires_grad = False in the reference: torch's AdamW skips it) keeps its values; its
  // BatchNorm running statistics still move in train-mode passes, as torch's do
  const size_t lo = group == 0 ? 0 : (ctx->freeze_det_backbone ? std::max(ctx->gpt_arena_end, ctx->det_head_begin) : ctx->gpt_arena_end);
  const size_t hi = group == 0 ? ctx->gpt_arena_end : ctx->arena_used;
  JN_CHECK(hi > lo, JN_ESTATE, "parameter group %d is empty", group);
  int& step = group == 0 ? ctx->adam_step : ctx->adam_step_yolox;
  step += 1;
  launch_adamw(ctx->params + lo, ctx->grads + lo, ctx->adam_m + lo, ctx->adam_v + lo, (long long)(hi - lo), lr, 0.9, 0.999, 1e-8f,
               weight_decay, step, clip_value, grad_scale, (hipStream_t)stream);
  mark_params_written(ctx);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_arena_segment(jn_ctx* ctx, const char* name, size_t* off, size_t* numel) {
  JN_CHECK(ctx && name && ctx->weights_loaded, JN_ESTATE, "jn_load_weights has not been called");
  auto it = ctx->seg_index.find(name);
  JN_CHECK(it != ctx->seg_index.end(), JN_ENOTFOUND, "jn_arena_segment: '%s' is not a trainable tensor", name);
  if (off) *off = ctx->segs[it->second].off;
  if (numel) *numel = ctx->segs[it->second].numel;
  return JN_OK;
}

int jn_export_arena(jn_ctx* ctx, int what, float* dst_dev, size_t numel, int accumulate, void* stream) {
  return arena_copy(ctx, what, dst_dev, numel, 1, accumulate, stream);
}

int jn_import_arena(jn_ctx* ctx, int what, const float* src_dev, size_t numel, void* stream) {
  return arena_copy(ctx, what, const_cast<float*>(src_dev), numel, 0, 0, stream);
}

int jn_set_freeze(jn_ctx* ctx, int freeze_detector_backbone) {
  JN_CHECK(ctx, JN_EINVAL, "null ctx");
  ctx->freeze_det_backbone = freeze_detector_backbone != 0;
  return JN_OK;
}

int jn_optimizer_steps(jn_ctx* ctx, int group, int* steps, int set) {
  JN_CHECK(ctx && steps && (group == 0 || group == 1), JN_EINVAL, "jn_optimizer_steps: bad argument");
  int& st = group == 0 ? ctx->adam_step : ctx->adam_step_yolox;
  if (set) st = *steps; else *steps = st;
  return JN_OK;
}

int jn_set_dropout(jn_ctx* ctx, float p, uint64_t seed) {
  JN_CHECK(ctx && p >= 0.0f && p < 1.0f, JN_EINVAL, "dropout probability must be in [0, 1)");
  ctx->pdrop = p; ctx->drop_seed = seed; ctx->drop_ctr = 0;
  return JN_OK;
}

}  // extern "C"
