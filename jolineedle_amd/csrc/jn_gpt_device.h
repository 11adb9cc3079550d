// Device helpers of the decision transformer, shared by its four units: the per-agent step (kernels_gpt.hip), the
// agents-batched step (kernels_gptwide.hip), the batched backward (kernels_gptbwd.hip) and the per-agent backward
// (kernels_train.hip).  What decides which action an agent takes, and which embedding rows a token of the forward reads,
// exists here once.  The two backwards take NewGELU and the wave sum from here and nothing else: their kernels add with
// float atomics, so no bit test can vouch for them, and they are held to the instruction streams they had — every other
// helper tried there (the executed-step count, the token info, the position accessors) moved at least an operand.
#pragma once
#include "jn_device.h"

namespace jnr {

// NewGELU (src/models/gpt.py:37-47) and its derivative.
__device__ __forceinline__ float gelu_tanh(float x) {
  return 0.5f * x * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x)));
}
__device__ __forceinline__ float gelu_tanh_grad(float x) {
  const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
  const float th = tanhf(u);
  return 0.5f * (1.0f + th) + 0.5f * x * (1.0f - th * th) * 0.7978845608028654f * (1.0f + 3.0f * 0.044715f * x * x);
}

// ---- reductions ---------------------------------------------------------------------------------------------------------
// sum over the 64 lanes of a wave, by shuffles; every lane holds the result
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// sum over the workgroup's NT threads: the waves' sums meet in LDS (red: NT / 64 floats).  `tid` is the caller's thread
// index (gpt_step_kernel passes an opaque one to keep its address arithmetic where it is used).
template <int NT>
__device__ __forceinline__ float block_sum(float v, float* red, int tid) {
  v = wave_sum(v);
  const int lane = tid & 63, wave = tid >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float s = 0.0f;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) s += red[w];
  return s;
}

// init + p[0] + p[stride] + ... (n terms, ascending: the order every consumer of split-K partials keeps), eight loads in
// flight at a time.  A plain loop waits for each load before it asks for the next, and a consumer with one workgroup per
// agent has nothing else to run meanwhile: 24 partials were 24 round trips to L2.  Terms past n are asked for at a clamped
// address and left out by a select, not by a branch around the load.
template <typename V>
__device__ __forceinline__ V sum_parts(V init, const float* __restrict__ p, long long stride, int n) {
  V s = init;
  for (int k0 = 0; k0 < n; k0 += 8) {
    V v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const V*>(p + (long long)min(k0 + u, n - 1) * stride);
#pragma unroll
    for (int u = 0; u < 8; ++u) { const V nx = s + v[u]; s = k0 + u < n ? nx : s; }
  }
  return s;
}

// ---- a step that is skipped ----------------------------------------------------------------------------------------------
__device__ __forceinline__ bool step_skipped(const int* flag, int when) { return flag && *flag >= when; }

// Prologue of the two kernels that end a step (gpt_step_kernel, gptw_tail_kernel).  True: every env was done before this
// step — stay skipped for the rest of the trajectory (n_done carries on) and return.
__device__ __forceinline__ bool gpt_step_skipped(const GptStepArgs& a) {
  if (!step_skipped(a.skip_flag, a.skip_when)) return false;
  if (blockIdx.x == 0 && threadIdx.x == 0) a.n_done[a.step + 1] = a.skip_when;
  return true;
}

// ---- token embedding (src/models/gpt.py:419-479) ------------------------------------------------------------------------
// What token `j` of a step is (j = 1 only for the first patch behind the class token at step 0 of a rollout): the class
// token and a given embedding are rows read as they are; every other token is the merge of its parts, through
// project_concat's Linear with concat_emb (to_gemm: the wide route makes that a GEMM of its own).
struct GptTokKind { bool class_tok, given, to_gemm; };
__host__ __device__ inline GptTokKind gpt_tok_kind(const GptStepArgs& a, int j) {
  GptTokKind k;
  k.class_tok = (a.src_mode == GPT_SRC_CLASS) || (a.src_mode == GPT_SRC_ENV && a.step == 0 && j == 0);
  k.given = !k.class_tok && a.src_mode == GPT_SRC_GIVEN;
  k.to_gemm = !k.class_tok && !k.given && a.concat_emb;
  return k;
}

// The token's source for agent `b`: `direct` (the finished embedding row) or, when null, the clamped action id and grid
// position its parts are looked up by — the env's state in a rollout, the teacher arrays otherwise.
struct GptTokSrc { GptTokKind kind; const float* direct; int act, row, col; };
__device__ __forceinline__ GptTokSrc gpt_tok_src(const GptStepArgs& a, int b, int j) {
  GptTokSrc r;
  r.kind = gpt_tok_kind(a, j);
  r.direct = nullptr; r.act = 0; r.row = 0; r.col = 0;
  if (r.kind.class_tok) {
    // embed_class(classes) (gpt.py:476-478); a rollout without jn_set_rollout_classes passes no ids: class 0
    // (reinforce.py:128-129)
    const int cls = a.classes ? min(max((int)a.classes[b], 0), JN_N_CLASS_ROWS - 1) : 0;
    r.direct = a.embed_class + (long long)cls * a.C;
  } else if (r.kind.given) {
    r.direct = a.given_emb + ((long long)b * a.given_stride + a.given_index) * a.C;
  } else {
    if (a.src_mode == GPT_SRC_ENV) {
      r.act = (int)a.prev_action[b];
      r.row = (int)a.env.positions[2 * b]; r.col = (int)a.env.positions[2 * b + 1];
    } else {
      const long long bi = (long long)b * a.t_stride + a.t_index;
      r.act = (int)a.t_actions[bi];
      r.row = a.t_positions ? (int)a.t_positions[2 * bi] : 0;
      r.col = a.t_positions ? (int)a.t_positions[2 * bi + 1] : 0;
    }
    r.act = min(max(r.act, 0), a.nA - 1);
    r.row = min(max(r.row, 0), 255); r.col = min(max(r.col, 0), 255);
  }
  return r;
}

// Element i of the 1-D position row p1 (the sinusoid table with decoder_pos_encoding, else the learned wpe) and of the
// 2-D sinusoid of (row, col): the column's channels first, then the row's.
__device__ __forceinline__ float gpt_pos1d(const GptStepArgs& a, int p1, int i) {
  return a.dec_pos_enc ? a.pos1d[p1 * a.C + i] : a.wpe[p1 * a.C + i];
}
__device__ __forceinline__ float gpt_pos2d(const GptStepArgs& a, int row, int col, int i) {
  return (i < a.pe2_ch) ? a.pe2[col * a.pe2_ch + i] : a.pe2[row * a.pe2_ch + (i - a.pe2_ch)];
}

// ---- decide and step ----------------------------------------------------------------------------------------------------
// One thread of agent b, behind the head's logits lg[nA] of the newest token, `len` tokens cached once this step is done:
// Categorical argmax / sample / forced action with its log-prob and entropy (src/reinforce.py:73-90), the env step, the
// rollout's bookkeeping (reinforce.py:169-179) and the n_done count.  Both step routes call this.
__device__ inline void gpt_decide_and_step(const GptStepArgs& a, int b, const float* lg, int len) {
  a.cache_len[b] = len;
  const int nA = a.nA, t = a.step;
  float m = -INFINITY;
  int best = 0;
  for (int i = 0; i < nA; ++i)
    if (lg[i] > m) { m = lg[i]; best = i; }           // first maximum, as torch.argmax
  float sum = 0.0f;
  for (int i = 0; i < nA; ++i) sum += expf(lg[i] - m);
  const float lse = m + logf(sum);
  float ent = 0.0f;
  for (int i = 0; i < nA; ++i) { const float lp = lg[i] - lse; ent -= lp * expf(lp); }
  int act = best;
  if (a.mode == JN_MODE_FORCED) {
    act = (int)a.forced[(long long)b * a.T + t];
    act = min(max(act, 0), nA - 1);
  } else if (a.mode == JN_MODE_SAMPLE) {
    // keyed (seed, agent, step, "SAMP"); with jn_set_rollout_keys the agent's own (stream seed, stream index) instead
    const uint64_t key = a.keys ? a.keys[2 * b] : a.seed;
    const uint32_t idx = a.keys ? (uint32_t)a.keys[2 * b + 1] : (uint32_t)b;
    const uint4 r = philox4x32(key, idx, (uint32_t)t, 0x53414d50u, 0u);
    const float u = u01(r.x);
    float cdf = 0.0f;
    act = nA - 1;
    for (int i = 0; i < nA; ++i) {
      cdf += expf(lg[i] - lse);
      if (u < cdf) { act = i; break; }
    }
  }
  const float logp = lg[act] - lse;
  const EnvStepResult r = env_step_one(a.env, b, act);
  a.prev_action[b] = act;
  const long long bt = (long long)b * a.T + t;
  if (a.out.rewards) a.out.rewards[bt] = r.reward;
  if (a.out.logprobs) a.out.logprobs[bt] = logp;
  if (a.out.entropies) a.out.entropies[bt] = ent;
  if (a.out.actions) a.out.actions[bt] = act;
  if (a.out.masks) a.out.masks[(long long)b * (a.T + 1) + t + 1] = r.terminated ? 0 : 1;
  if (a.out.positions) {
    a.out.positions[((long long)b * (a.T + 1) + t + 1) * 2] = r.y;
    a.out.positions[((long long)b * (a.T + 1) + t + 1) * 2 + 1] = r.x;
  }
  if (a.out.logits)
    for (int i = 0; i < nA; ++i) a.out.logits[bt * nA + i] = lg[i];
  if (r.terminated || r.truncated) atomicAdd(a.n_done + t + 1, 1);      // an integer count: order-free
}

// The same under invalid-action masking (a.mask_policy != 0, jn_set_rollout_action_mask; not in the reference): the agent's
// action set M is formed from the state the decision sees, the Categorical is the softmax over the members' logits, and a
// logit outside M is never read into the maximum, the sum or the entropy.  The sample walks the members in index order at the
// uniform the unmasked decision draws; M goes to the context's buffer and the caller's.  The step's tail is the one above.
__device__ inline void gpt_decide_and_step_masked(const GptStepArgs& a, int b, const float* lg, int len) {
  a.cache_len[b] = len;
  const int nA = a.nA, t = a.step;
  const long long bt = (long long)b * a.T + t;
  int forced = -1;
  if (a.mode == JN_MODE_FORCED) forced = min(max((int)a.forced[bt], 0), nA - 1);
  const EnvPtrs& e = a.env;
  const int gh = e.extent ? e.extent[2 * b] : e.Gh, gw = e.extent ? e.extent[2 * b + 1] : e.Gw;
  const uint32_t M = action_set_one(a.mask_policy, (int)e.positions[2 * b], (int)e.positions[2 * b + 1], gh, gw,
                                    e.visited + (long long)b * e.Gh * e.Gw, e.Gw, nA, forced);
  a.mask_sets[bt] = (uint16_t)M;
  if (a.mask_sets_out) a.mask_sets_out[bt] = (uint16_t)M;
  float m = -INFINITY;
  int best = 0, last = 0;
  for (int i = 0; i < nA; ++i) {
    if (!(M >> i & 1u)) continue;
    last = i;
    if (lg[i] > m) { m = lg[i]; best = i; }           // first maximum among the members
  }
  float sum = 0.0f;
  for (int i = 0; i < nA; ++i)
    if (M >> i & 1u) sum += expf(lg[i] - m);
  const float lse = m + logf(sum);
  float ent = 0.0f;
  for (int i = 0; i < nA; ++i)
    if (M >> i & 1u) { const float lp = lg[i] - lse; ent -= lp * expf(lp); }
  int act = best;
  if (a.mode == JN_MODE_FORCED) {
    act = forced;
  } else if (a.mode == JN_MODE_SAMPLE) {
    const uint64_t key = a.keys ? a.keys[2 * b] : a.seed;
    const uint32_t idx = a.keys ? (uint32_t)a.keys[2 * b + 1] : (uint32_t)b;
    const uint4 r = philox4x32(key, idx, (uint32_t)t, 0x53414d50u, 0u);
    const float u = u01(r.x);
    float cdf = 0.0f;
    act = last;
    for (int i = 0; i < nA; ++i) {
      if (!(M >> i & 1u)) continue;
      cdf += expf(lg[i] - lse);
      if (u < cdf) { act = i; break; }
    }
  }
  const float logp = lg[act] - lse;
  const EnvStepResult r = env_step_one(a.env, b, act);
  a.prev_action[b] = act;
  if (a.out.rewards) a.out.rewards[bt] = r.reward;
  if (a.out.logprobs) a.out.logprobs[bt] = logp;
  if (a.out.entropies) a.out.entropies[bt] = ent;
  if (a.out.actions) a.out.actions[bt] = act;
  if (a.out.masks) a.out.masks[(long long)b * (a.T + 1) + t + 1] = r.terminated ? 0 : 1;
  if (a.out.positions) {
    a.out.positions[((long long)b * (a.T + 1) + t + 1) * 2] = r.y;
    a.out.positions[((long long)b * (a.T + 1) + t + 1) * 2 + 1] = r.x;
  }
  if (a.out.logits)
    for (int i = 0; i < nA; ++i) a.out.logits[bt * nA + i] = lg[i];
  if (r.terminated || r.truncated) atomicAdd(a.n_done + t + 1, 1);
}

}  // namespace jnr
