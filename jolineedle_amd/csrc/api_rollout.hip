// C ABI of libjnroll.so, rollout unit: the glimpse loop, its switches and its read-backs.
// Host code only (compiled by hipcc as C++); kernels live in kernels_*.hip.
#include <algorithm>

#include "jn_internal.h"

namespace jnr {

// zero-fill so that columns past an early stop read as the reference's absent columns would be cut
static int zero_rollout_outputs(const RolloutBuffers& r, uint8_t* tsets, int B, int T, int C, int nA, hipStream_t s) {
  JN_HIP(hipMemsetAsync(r.rewards, 0, (size_t)B * T * sizeof(float), s));
  if (r.returns) JN_HIP(hipMemsetAsync(r.returns, 0, (size_t)B * T * sizeof(float), s));
  if (r.logprobs) JN_HIP(hipMemsetAsync(r.logprobs, 0, (size_t)B * T * sizeof(float), s));
  if (r.entropies) JN_HIP(hipMemsetAsync(r.entropies, 0, (size_t)B * T * sizeof(float), s));
  JN_HIP(hipMemsetAsync(r.masks, 0, (size_t)B * (T + 1), s));
  if (r.logit_masks) JN_HIP(hipMemsetAsync(r.logit_masks, 0, (size_t)B * T, s));
  if (r.positions) JN_HIP(hipMemsetAsync(r.positions, 0, (size_t)B * (T + 1) * 2 * sizeof(int64_t), s));
  if (r.actions) JN_HIP(hipMemsetAsync(r.actions, 0, (size_t)B * T * sizeof(int64_t), s));
  if (r.logits) JN_HIP(hipMemsetAsync(r.logits, 0, (size_t)B * T * nA * sizeof(float), s));
  if (r.final_emb) JN_HIP(hipMemsetAsync(r.final_emb, 0, (size_t)B * (T + 1) * C * sizeof(float), s));
  if (tsets) JN_HIP(hipMemsetAsync(tsets, 0, (size_t)B * T, s));
  return JN_OK;
}

// gradient buffers for as many glimpse steps as fit in ~80 % of the free HBM (the whole trajectory on a
// 288 GB MI355X at the headline sizes); the backward then runs in ceil(S / g_slots) step-batched passes
static int grad_slots_that_fit(const jn_ctx* ctx, const Net& tn, int T, int* g_want) {
  size_t free_b = 0, total_b = 0;
  JN_HIP(hipMemGetInfo(&free_b, &total_b));
  const size_t per_slot = (size_t)tn.per_image_floats * ctx->cfg.max_batch * sizeof(float) + (1u << 20);
  const long long fit = (long long)((double)free_b * 0.8 / (double)per_slot);
  *g_want = (int)std::max<long long>(1, std::min<long long>(T, fit));
  if (const char* cap = std::getenv("JN_GRAD_SLOTS")) *g_want = std::max(1, std::min(*g_want, std::atoi(cap)));
  return JN_OK;
}

int rollout_impl(jn_ctx* ctx, int mode, const int64_t* forced_actions_dev, const int64_t* start_positions_dev, uint64_t seed,
                 int do_detection, int stop_early, const jn_rollout_out* out, int train, void* stream) {
  JN_CHECK(ctx && out, JN_EINVAL, "jn_rollout: null argument");
  JN_CHECK(ctx->env.ready, JN_ESTATE, "jn_env_init has not been called");
  JN_CHECK(ctx->weights_loaded, JN_ESTATE, "jn_load_weights has not been called");
  JN_CHECK(mode >= 0 && mode <= 2, JN_EINVAL, "unknown mode %d", mode);
  JN_CHECK(mode != JN_MODE_FORCED || forced_actions_dev, JN_EINVAL, "JN_MODE_FORCED needs forced_actions");
  JN_CHECK(out->rewards_dev && out->masks_dev, JN_EINVAL, "rewards_dev and masks_dev are required outputs");
  JN_CHECK(!do_detection || (ctx->has_net[JN_NET_DETECTOR] && out->det_boxes_dev && out->det_counts_dev), JN_EINVAL,
           "do_detection needs a detector and det_boxes_dev / det_counts_dev outputs");
  const int n_keys = ctx->keys.rows();
  JN_CHECK(n_keys == 0 || n_keys == ctx->env.B, JN_EINVAL,
           "jn_set_rollout_keys armed %d agent streams, the env has %d agents", n_keys, ctx->env.B);
  const int n_classes = ctx->classes.rows();
  JN_CHECK(n_classes == 0 || n_classes == ctx->env.B, JN_EINVAL,
           "jn_set_rollout_classes armed %d class ids, the env has %d agents", n_classes, ctx->env.B);
  JN_HIP(hipSetDevice(ctx->cfg.device));
  hipStream_t s = (hipStream_t)stream;
  const jn_config& c = ctx->cfg;
  const EnvState& e = ctx->env;
  const int B = e.B, T = e.T, C = c.n_embd, P = c.patch_size, nA = c.n_actions;
  const bool by_token = ctx->pos_by_token;
  // gpt.py:427-428 in train mode re-encodes the whole prefix, BatchNorm statistics over B * (t + 1) patches: not what the
  // per-step workspace holds
  JN_CHECK(!(by_token && train), JN_ESTATE,
           "sequence token positions (jn_set_rollout_positions) are for eval rollouts: in train mode the reference "
           "re-encodes the whole prefix at every step with BatchNorm statistics over B*(t+1) patches");
  JN_CHECK(!by_token || c.decoder_pos_encoding || T <= c.pos_emb_size, JN_EINVAL,
           "sequence token positions: max_ep_len %d exceeds the %d rows of the learned position table (pos_emb_size)", T,
           c.pos_emb_size);
  uint8_t* const tsets = ctx->teacher_sets;
  const uint8_t* const ttargets = ctx->teacher_targets ? ctx->teacher_targets : e.bbox_masks;
  ctx->train_out_valid = false;       // every rollout restarts n_done / the env state the REINFORCE backward reads
  if (train) ctx->sup_valid = false;  // ... and a train-mode one the per-token buffers the supervised backward reads
  RolloutBuffers r{out->rewards_dev, out->returns_dev, out->logprobs_dev, out->entropies_dev, out->masks_dev,
                   out->logit_masks_dev, out->positions_dev, out->actions_dev, out->logits_dev, out->final_emb_dev};
  { int rz = zero_rollout_outputs(r, tsets, B, T, C, nA, s); if (rz) return rz; }
  // jn_set_rollout_action_mask: the sets of the executed steps are written by the decision; the rest read 0
  const int mask_policy = ctx->mask_policy;
  if (mask_policy) {
    JN_CHECK(nA <= 16, JN_EINVAL, "action masking: %d actions do not fit a 16-bit set", nA);
    if (!ctx->mask_sets) { int rm = dev_alloc(ctx, &ctx->mask_sets, (size_t)c.max_batch * c.block_size); if (rm) return rm; }
    JN_HIP(hipMemsetAsync(ctx->mask_sets, 0, (size_t)B * T * sizeof(uint16_t), s));
    if (ctx->mask_sets_out) JN_HIP(hipMemsetAsync(ctx->mask_sets_out, 0, (size_t)B * T * sizeof(uint16_t), s));
  }
  if (train) ctx->train_mask_policy = mask_policy;

  // per-agent streams and class ids: the context's copies go up on this rollout's stream (null: not armed)
  const uint64_t* keys = nullptr;
  const int64_t* classes = nullptr;
  { int rk = ctx->keys.upload(ctx, c.max_batch, s, &keys); if (rk) return rk; }
  { int rk = ctx->classes.upload(ctx, c.max_batch, s, &classes); if (rk) return rk; }
  // a train-mode rollout also keeps the ids it ran with for its backward
  if (train && classes) {
    if (ctx->classes_used_cap < (size_t)n_classes) {
      int rk = dev_alloc(ctx, &ctx->classes_used, (size_t)std::max(c.max_batch, n_classes));
      if (rk) return rk;
      ctx->classes_used_cap = (size_t)std::max(c.max_batch, n_classes);
    }
    JN_HIP(hipMemcpyAsync(ctx->classes_used, classes, (size_t)n_classes * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  }
  if (train) ctx->classes_used_n = n_classes;

  if (ctx->ev[0]) JN_HIP(hipEventRecord(ctx->ev[0], s));
  EnvPtrs ep = env_ptrs(ctx);
  launch_env_reset(ep, start_positions_dev, seed, keys, s);
  launch_rollout_begin(ep, r, ctx->prev_action, ctx->cache_len, ctx->n_done, s);
  const long long patch_stride = (long long)(T + 1) * 3 * P * P;
  if (out->patches_dev)
    env_gather(e, out->patches_dev, patch_stride, P, nullptr, 0, s);

  const int Kd = c.max_det_per_patch;
  if (do_detection) {
    // src/reinforce.py:141-146 (start patch) — written for every image, see DESIGN.md deviations
    JN_HIP(hipMemsetAsync(out->det_counts_dev, 0, (size_t)B * (T + 1) * sizeof(int32_t), s));
    if (!ctx->det_tmp_boxes) {
      int rc2;
      if ((rc2 = dev_alloc(ctx, &ctx->det_tmp_boxes, (size_t)c.max_batch * Kd * 7))) return rc2;
      if ((rc2 = dev_alloc(ctx, &ctx->det_tmp_counts, (size_t)c.max_batch))) return rc2;
    }
  }
  // The detector pass of a glimpse only feeds the detection outputs, so it runs on the context's second stream beside
  // the next glimpse step of the decision path: the positions it reads are snapshotted per step (the agents move on),
  // forked after the step that produced them, joined before the rollout returns.
  static const bool no_aux_det = std::getenv("JN_NO_AUX_STREAM") != nullptr;
  hipStream_t ds_stream = s;
  // (only with a separate patch encoder: when the detector's own PAFPN encodes the patches — no gpt_backbone, the
  // reference's default — both passes use the slot-0 workspace and table of the same net and must stay in stream order)
  if (do_detection && !no_aux_det && ctx->enc_net != JN_NET_DETECTOR) {
    int ra = ensure_aux_stream(ctx);
    if (ra) return ra;
    if (!ctx->det_pos || ctx->det_pos_cap < (size_t)(T + 1) * B * 2) {
      if ((ra = dev_alloc(ctx, &ctx->det_pos, (size_t)(T + 1) * B * 2))) return ra;
      ctx->det_pos_cap = (size_t)(T + 1) * B * 2;
    }
    ds_stream = ctx->aux_stream;
  }
  // view mode: column t of the staging stack holds the patches at positions[:, t].  The training backward reads the
  // columns again and the detector's second stream reads one while the decision path moves on, so both keep all of
  // them (a column nobody overwrites replaces the position snapshot); otherwise one column is reused
  const bool vm = e.view_mode;
  if (vm) {
    int rs = ensure_stage(ctx, (train || ds_stream != s) ? T + 1 : 1);
    if (rs) return rs;
    stage_fill(e, P, 0, nullptr, 0, s);
  }
  auto detect_step = [&](int col, const int* flag) -> int {
    const int64_t* pos = e.positions;
    if (ds_stream != s) {
      if (!vm) {
        int64_t* snap = ctx->det_pos + (size_t)col * B * 2;
        JN_HIP(hipMemcpyAsync(snap, e.positions, (size_t)B * 2 * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        pos = snap;
      }
      JN_HIP(hipEventRecord(ctx->aux_fork, s));
      JN_HIP(hipStreamWaitEvent(ds_stream, ctx->aux_fork, 0));
    }
    const StemSrc ds = vm ? stage_stem_src(e, P, col) : env_stem_src(e, pos);
    int r = detect_impl(ctx, ds, B, ctx->det_tmp_boxes, ctx->det_tmp_counts, nullptr, flag, B, ds_stream);
    if (r) return r;
    launch_det_scatter(ctx->det_tmp_boxes, ctx->det_tmp_counts, out->det_boxes_dev, out->det_counts_dev, B, T + 1, col, Kd,
                       flag, B, ds_stream);
    return JN_OK;
  };
  if (do_detection) { int r0 = detect_step(0, nullptr); if (r0) return r0; }
  if (ctx->profiling) {
    while ((int)ctx->conv_ev.size() < 2 * T) {
      hipEvent_t ev;
      JN_HIP(hipEventCreate(&ev));
      ctx->conv_ev.push_back(ev);
    }
  }
  ctx->conv_ev_used = 0;
  const StemSrc ss = env_stem_src(e, e.positions);
  int rc;
  // jn_set_activation_slots: a walk longer than the ring keeps `ring` activation slots besides slot 0 (step t writes
  // slot 1 + t % ring) and the backward replays every step; tables, saved statistics and sums stay one slot per step
  const int ring = train && !c.no_patch_emb && ctx->enc_net != JN_NET_DETECTOR && ctx->act_ring > 0 && ctx->act_ring < T ? ctx->act_ring : 0;
  if (train) ctx->train_ring = ring;
  if (train) {
    Net& tn = ctx->nets[ctx->enc_net];
    // (a shared detector / encoder net: the detector's training pass gets its slot behind the rollout's right away, so
    // that no growth — and copy — happens between this rollout and its backward)
    if ((rc = ensure_slots(ctx, tn, ctx->enc_net == JN_NET_DETECTOR ? c.block_size + 2 : T + 1, ring ? ring + 1 : -1))) return rc;
    int g_want = tn.g_slots;
    const int g_most = ring ? ring : T;      // a gradient mirror for a step whose activations are not there is useless
    if (ctx->enc_net == JN_NET_DETECTOR) g_want = std::max(1, g_want);   // detached encoder: no conv-stack backward
    else if (g_want < g_most && (rc = grad_slots_that_fit(ctx, tn, g_most, &g_want))) return rc;
    if ((rc = ensure_train_state(ctx, g_want))) return rc;
    if ((rc = ensure_token_train_buffers(ctx))) return rc;
  }
  if (train) ctx->drop_seed_used = ctx->drop_seed + ctx->drop_ctr++;   // dropout masks of this trajectory (regenerated in the backward)
  struct PrezeroGuard { jn_ctx* c; ~PrezeroGuard() { c->stats_prezeroed = false; } } prezero_guard{ctx};
  if (train && !c.no_patch_emb) {
    Net& tn = ctx->nets[ctx->enc_net];
    JN_HIP(hipMemsetAsync(slot_stats(tn, 1), 0, (size_t)T * JN_NREP * 2 * tn.stat_channels * sizeof(double), s));
    ctx->stats_prezeroed = true;
  }
  for (int t = 0; t < T; ++t) {
    const int* flag = stop_early ? ctx->n_done + t : nullptr;
    // the teacher's opinion of the state this step's decision sees (src/supervised.py:279-405 compares against it)
    if (tsets) launch_teacher_sets(e.positions, e.visited, ttargets, tsets + t, T, B, e.Gh, e.Gw, flag, B, s);
    if (!c.no_patch_emb) {
      if (ctx->profiling) JN_HIP(hipEventRecord(ctx->conv_ev[2 * t], s));
      const int a_slot = !train ? 0 : ring ? 1 + t % ring : t + 1;
      if ((rc = run_net(ctx, ctx->enc_net, B, vm ? stage_stem_src(e, P, t) : ss, a_slot, train, flag, B, s, false, 0, train ? t + 1 : 0))) return rc;
      if (ctx->profiling) { JN_HIP(hipEventRecord(ctx->conv_ev[2 * t + 1], s)); ctx->conv_ev_used = 2 * (t + 1); }
      if ((rc = run_embed_fpn(ctx, B, a_slot, train ? ctx->efpn_train + (size_t)t * B * ctx->efpn_h * ctx->efpn_w * C : nullptr, flag, B, s,
                              train ? t + 1 : 0)))
        return rc;
    }
    GptStepArgs a{};
    fill_gpt_weights(ctx, a);
    a.B = B; a.T = T;
    a.step = t; a.mode = mode; a.forced = forced_actions_dev; a.seed = seed; a.keys = keys;
    a.classes = classes;
    // recurrent: every new token at 1-D position 0 (gpt.py:431-449); by token: position t, the last row of the
    // reference's full-prefix forward (gpt.py:331-354, 427-428)
    a.src_mode = GPT_SRC_ENV; a.pos_index = by_token ? t : 0; a.emb_stride = T + 1;
    a.env = ep; a.out = r;
    a.skip_flag = flag; a.skip_when = B;
    a.tok_emb_out = train ? ctx->tok_emb_train : nullptr;
    a.pdrop = train ? ctx->pdrop : 0.0f; a.drop_seed = ctx->drop_seed_used;
    a.mask_policy = mask_policy; a.mask_sets = ctx->mask_sets; a.mask_sets_out = ctx->mask_sets_out;
    JN_CHECK(launch_gpt_step_routed(a, s) == 0, JN_ESTATE, "the decision step could not be launched (n_embd %d, block_size %d)", a.C, a.Tmax - 1);
    if (out->patches_dev)
      env_gather(e, out->patches_dev + (long long)(t + 1) * 3 * P * P, patch_stride, P, flag, B, s);
    if (vm && (t + 1 < T || do_detection)) stage_fill(e, P, t + 1, flag, B, s);    // read by the next step and the detector
    if (do_detection && (rc = detect_step(t + 1, flag))) return rc;     // src/reinforce.py:162-167
  }
  if (ds_stream != s) {
    JN_HIP(hipEventRecord(ctx->aux_join, ds_stream));
    JN_HIP(hipStreamWaitEvent(s, ctx->aux_join, 0));
  }
  launch_rollout_epilogue(r, ctx->n_done, B, T, stop_early ? 1 : 0, s);
  ctx->last_stop_early = stop_early != 0;
  if (ctx->ev[1]) JN_HIP(hipEventRecord(ctx->ev[1], s));
  JN_HIP(hipGetLastError());
  ctx->last_T = T;
  return JN_OK;
}

int rollout_steps_begin(jn_ctx* ctx, hipStream_t s) {
  JN_CHECK(ctx && ctx->last_T > 0, JN_ESTATE, "no rollout has run");
  JN_HIP(hipSetDevice(ctx->cfg.device));
  const int n = ctx->last_T + 1;
  if (ctx->n_done_host_n < n) {
    // (a copy of an earlier _begin that no _end waited for — an error between the two — may still be on its way there)
    if (ctx->steps_ev) JN_HIP(hipEventSynchronize(ctx->steps_ev));
    if (ctx->n_done_host) JN_HIP(hipHostFree(ctx->n_done_host));
    ctx->n_done_host = nullptr; ctx->n_done_host_n = 0;
    JN_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->n_done_host), (size_t)n * sizeof(int32_t), hipHostMallocDefault));
    ctx->n_done_host_n = n;
  }
  if (!ctx->steps_ev) JN_HIP(hipEventCreateWithFlags(&ctx->steps_ev, hipEventDisableTiming));
  JN_HIP(hipMemcpyAsync(ctx->n_done_host, ctx->n_done, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  JN_HIP(hipEventRecord(ctx->steps_ev, s));
  return JN_OK;
}

int rollout_steps_end(jn_ctx* ctx, int* n_steps) {
  JN_CHECK(ctx && n_steps && ctx->steps_ev && ctx->n_done_host, JN_ESTATE, "rollout_steps_end without rollout_steps_begin");
  JN_HIP(hipEventSynchronize(ctx->steps_ev));
  const int T = ctx->last_T, B = ctx->env.B;
  int S = T;
  if (ctx->last_stop_early)
    for (int t = 1; t <= T; ++t)
      if (ctx->n_done_host[t] >= B) { S = t; break; }
  *n_steps = S;
  return JN_OK;
}

}  // namespace jnr

using namespace jnr;

extern "C" {

int jn_rollout(jn_ctx* ctx, int mode, const int64_t* forced_actions_dev, const int64_t* start_positions_dev,
               uint64_t seed, int do_detection, int stop_early, const jn_rollout_out* out, void* stream) {
  return rollout_impl(ctx, mode, forced_actions_dev, start_positions_dev, seed, do_detection, stop_early, out, 0, stream);
}

int jn_set_rollout_positions(jn_ctx* ctx, int by_token) {
  JN_CHECK(ctx, JN_EINVAL, "null ctx");
  ctx->pos_by_token = by_token != 0;
  return JN_OK;
}

int jn_set_activation_slots(jn_ctx* ctx, int n) {
  JN_CHECK(ctx, JN_EINVAL, "jn_set_activation_slots: null ctx");
  JN_CHECK(n >= 0, JN_EINVAL, "jn_set_activation_slots: n = %d (0: one slot per glimpse step, n >= 1: a ring of n)", n);
  ctx->act_ring = n;
  ctx->train_out_valid = false;      // a rollout made under another setting is not differentiated under this one
  return JN_OK;
}

int jn_activation_slots_info(const jn_ctx* ctx, int net, int* act_slots, int* table_slots, size_t* slot_bytes, int* replayed_steps) {
  JN_CHECK(ctx && net >= 0 && net < 2 && ctx->has_net[net], JN_EINVAL, "jn_activation_slots_info: network %d is not part of this context", net);
  const Net& n = ctx->nets[net];
  if (act_slots) *act_slots = n.a_slots;
  if (table_slots) *table_slots = n.n_slots;
  if (slot_bytes) *slot_bytes = n.per_image_floats * (size_t)ctx->cfg.max_batch * act_esz(n);
  if (replayed_steps) *replayed_steps = net == ctx->enc_net ? ctx->replayed_steps : 0;
  return JN_OK;
}

int jn_set_rollout_teacher(jn_ctx* ctx, const uint8_t* targets_dev, uint8_t* sets_dev) {
  JN_CHECK(ctx, JN_EINVAL, "null ctx");
  ctx->teacher_sets = sets_dev;
  ctx->teacher_targets = sets_dev ? targets_dev : nullptr;
  return JN_OK;
}

int jn_set_rollout_action_mask(jn_ctx* ctx, int policy, uint16_t* sets_out_dev) {
  JN_CHECK(ctx, JN_EINVAL, "jn_set_rollout_action_mask: null ctx");
  JN_CHECK(policy >= JN_MASK_NONE && policy <= JN_MASK_UNVISITED, JN_EINVAL,
           "jn_set_rollout_action_mask: policy %d (0: none, 1: grid, 2: unvisited)", policy);
  ctx->mask_policy = policy;
  ctx->mask_sets_out = policy ? sets_out_dev : nullptr;
  if (policy) ctx->train_out_valid = false;   // a forward made before this arming is not differentiated after it
  return JN_OK;
}

int jn_set_rollout_keys(jn_ctx* ctx, const uint64_t* keys_host, int n) {
  JN_CHECK(ctx, JN_EINVAL, "jn_set_rollout_keys: null ctx");
  if (!keys_host) {
    ctx->keys.clear();
    return JN_OK;
  }
  JN_CHECK(n >= 1, JN_EINVAL, "jn_set_rollout_keys: n = %d with a table", n);
  for (int b = 0; b < n; ++b)
    JN_CHECK(keys_host[2 * b + 1] <= 0xFFFFFFFFull, JN_EINVAL,
             "jn_set_rollout_keys: the stream index of agent %d, %llu, does not fit 32 bits", b,
             (unsigned long long)keys_host[2 * b + 1]);
  return ctx->keys.set(keys_host, (size_t)n);
}

int jn_set_rollout_classes(jn_ctx* ctx, const int64_t* classes_host, int n) {
  JN_CHECK(ctx, JN_EINVAL, "jn_set_rollout_classes: null ctx");
  if (!classes_host) {
    ctx->classes.clear();
    return JN_OK;
  }
  JN_CHECK(n >= 1, JN_EINVAL, "jn_set_rollout_classes: n = %d with a table", n);
  for (int b = 0; b < n; ++b)
    JN_CHECK(classes_host[b] >= 0 && classes_host[b] < JN_N_CLASS_ROWS, JN_EINVAL,
             "jn_set_rollout_classes: the class id of agent %d, %lld, is outside embed_class (rows 0 .. %d)", b,
             (long long)classes_host[b], JN_N_CLASS_ROWS - 1);
  return ctx->classes.set(classes_host, (size_t)n);
}

int jn_rollout_steps(jn_ctx* ctx, int* n_steps, void* stream) {
  JN_CHECK(ctx && n_steps && ctx->last_T > 0, JN_ESTATE, "no rollout has run");
  int rc = rollout_steps_begin(ctx, (hipStream_t)stream);
  if (rc) return rc;
  return rollout_steps_end(ctx, n_steps);
}

int jn_set_profiling(jn_ctx* ctx, int enabled) {
  JN_CHECK(ctx, JN_EINVAL, "null ctx");
  ctx->profiling = enabled != 0;
  return JN_OK;
}

int jn_last_timing(jn_ctx* ctx, int what, float* ms) {
  JN_CHECK(ctx && ms && ctx->last_T > 0, JN_ESTATE, "no rollout has run");
  JN_HIP(hipSetDevice(ctx->cfg.device));
  JN_HIP(hipEventSynchronize(ctx->ev[1]));
  if (what == 0) {
    JN_HIP(hipEventElapsedTime(ms, ctx->ev[0], ctx->ev[1]));
  } else if (what == 2) {
    JN_CHECK(ctx->bwd_timed, JN_ESTATE, "no profiled jn_reinforce_step has run");
    JN_HIP(hipEventSynchronize(ctx->ev[3]));
    JN_HIP(hipEventElapsedTime(ms, ctx->ev[2], ctx->ev[3]));
  } else {
    float tot = 0.0f;
    for (int i = 0; i + 1 < ctx->conv_ev_used; i += 2) {
      float m = 0.0f;
      JN_HIP(hipEventElapsedTime(&m, ctx->conv_ev[i], ctx->conv_ev[i + 1]));
      tot += m;
    }
    *ms = tot;
  }
  return JN_OK;
}

}  // extern "C"
