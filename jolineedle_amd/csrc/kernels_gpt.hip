// One glimpse step of the decision model for every agent of the batch, in ONE launch:
//   token embedding (src/models/gpt.py:419-479) -> pre-LN GPT-2 blocks with a persistent
//   per-agent KV cache (the reference recomputes the whole prefix, gpt.py:525-528; with
//   dropout 0 and a causal mask the cached form is the same function) -> ln_f ->
//   ActionHead (src/models/action_head.py:24-33) -> Categorical argmax / sample / forced
//   + log-prob + entropy (src/reinforce.py:73-90) -> env step + reward
//   (src/env/general_env.py:172-233, 321-358) -> rollout bookkeeping (reinforce.py:169-179).
// One workgroup per agent; all vectors live in LDS; Linear weights are stored transposed
// ([k][n]) so lanes read consecutive n.  Nothing here returns to the host.
#include <hip/hip_runtime.h>

#include "jn_gpt_device.h"

namespace jnr {

// Threads per agent (template parameter NT of everything below): 1024 for wide models — 16 waves, every Linear splits K
// over all of them (256 threads left a 192 -> 576 layer of gpt-mini with ONE K slice: 192 dependent loads per thread) — and
// 256 for n_embd <= 64 (gpt-nano: its largest Linear is 48 x 192, the 1024-thread form only made every barrier and block
// reduction four times as wide: 95.7 -> 119.4 us per step between rounds 1 and 2, back to the 256-thread form in round 3).

//
// Latency, not arithmetic, is what a step costs (gpt-nano: ~340 FMAs per thread against 50 - 60 barrier-separated phases),
// and between two steps the encoder pass pushes every line this kernel reads out of L2 and the Infinity Cache.  So:
//   * at entry the workgroups of one XCD share out one touch per 128-byte line of the parameters (head, ln_f and every
//     layer lie in one run of the arena) and of the agent's own K / V rows; the values are only waited for once the
//     embedding is done (touch_issue / touch_sink) — what follows finds its lines in L2;
//   * a Linear's per-thread weight fragment, its bias and a LayerNorm's parameters are requested before the barriers of
//     the phase in front of them (lin_issue ... lin_run) and every load of a K slice is in flight before its first FMA;
//   * the agent's K / V rows of a layer go to LDS once (requested before ln_1), attention runs from LDS.
// None of this touches a floating-point operation: same split-K slices, same ascending k / i / s chains, same partial order.

using f4 = __attribute__((ext_vector_type(4))) float;

// The address arithmetic of the unrolled loads below depends on nothing but the thread index and the model's sizes; left
// to itself the compiler computes all of it once, in front of the token and layer loops, and keeps it: hundreds of
// registers held for the whole kernel.  A thread index taken through here is opaque, so the arithmetic stays at its use.
__device__ __forceinline__ int tid_here() {
  int v = threadIdx.x;
  asm volatile("" : "+v"(v));
  return v;
}

// ---- L2 warm-up: one 4-byte load per 32-float line of base[lo, hi), lines dealt round-robin over `nshare` workgroups ----
template <int U> struct Touch { uint32_t r[U]; uint32_t extra; };
constexpr int TOUCH_MORE = 4;

template <int NT, int U>
__device__ __forceinline__ void touch_issue(Touch<U>& t, const float* __restrict__ base, long long lo, long long hi, int share,
                                            int nshare) {
  t.extra = 0u;
#pragma unroll
  for (int u = 0; u < U; ++u) t.r[u] = 0u;
  if (hi <= lo) return;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(base + lo);
  const unsigned nl = (unsigned)((hi - lo + 31) >> 5), stride = (unsigned)nshare * NT;      // launch: < 2^30 floats
  unsigned l = (unsigned)share * NT + tid_here();
#pragma unroll
  for (int u = 0; u < U; ++u, l += stride) t.r[u] = p[min(l, nl - 1) << 5];     // clamped: no branch around a load
  // A longer share (a small batch: few workgroups per XCD; a wide model): ONE more round of TOUCH_MORE lines, all in
  // flight together and waited for here — one round trip at the most on the critical path.  What lies beyond is left to
  // the loads that need it, as before.
  if (l < nl) {
    uint32_t more[TOUCH_MORE];
#pragma unroll
    for (int u = 0; u < TOUCH_MORE; ++u) more[u] = p[min(l + u * stride, nl - 1) << 5];
    uint32_t acc = 0u;
#pragma unroll
    for (int u = 0; u < TOUCH_MORE; ++u) acc ^= more[u];
    t.extra = acc;
  }
}
template <int U>
__device__ __forceinline__ void touch_sink(const Touch<U>& t) {
  uint32_t v = t.extra;
#pragma unroll
  for (int u = 0; u < U; ++u) v ^= t.r[u];
  asm volatile("" ::"v"(v));      // the loads must happen; nothing reads their values
}

// y[n] = b[n] + sum_k x[k] * wt[k*N + n]   (x in LDS, wt transposed in global/L2).
// All threads work whatever N is: thread = (column quad, K slice); each slice walks K with stride `slices`
// (independent dwordx4 loads), partials meet in LDS scratch `part` (>= 4 * NT floats).  With one thread per column a
// 192 -> 48 layer was 192 dependent loads on 48 threads: the whole step was a chain of L2 latencies.
//
// In two halves: lin_issue requests the first U rows of the thread's K slice and its bias (it needs only the weights'
// address, so it stands in front of the barriers of the preceding phase), lin_run does the arithmetic once x is ready,
// fetching what is left of the slice in rounds of LinRound<NT>::n rows, all in flight before the round's first FMA.  Rows past K
// are requested at a clamped address and left out of the sum (a select, not a branch: a branch around a load makes the
// compiler wait for every load by itself).  Threads past the last slice request the last slice's rows and write nothing.
template <int U> struct LinFrag { f4 w[U]; float bias; int q, sl_raw; };

template <int NT> struct LinRound { static constexpr int n = NT == 256 ? 12 : 4; };

__device__ __forceinline__ bool lin_quads(int N, int NT) { return (N & 3) == 0 && N <= 4 * NT; }

template <int NT, int U>
__device__ __forceinline__ void lin_issue(LinFrag<U>& f, const float* __restrict__ wt, const float* __restrict__ b, int K, int N) {
  const int tid = tid_here();
  f.bias = b ? b[min(tid, N - 1)] : 0.0f;
  f.q = 0; f.sl_raw = 0;
  if (lin_quads(N, NT)) {
    const int nq = N >> 2, slices = NT / nq;
    f.q = tid % nq; f.sl_raw = tid / nq;
    const int sl = min(f.sl_raw, slices - 1);
#pragma unroll
    for (int u = 0; u < U; ++u) f.w[u] = *reinterpret_cast<const f4*>(wt + (unsigned)(min(sl + u * slices, K - 1) * N + 4 * f.q));
  }
}

template <int NT, int U>
__device__ __forceinline__ void lin_run(float* y, const float* x, const LinFrag<U>& f, const float* __restrict__ wt,
                                        const float* __restrict__ b, int K, int N, float* part) {
  constexpr int R = LinRound<NT>::n;
  const int tid = tid_here();
  if (lin_quads(N, NT)) {
    const int nq = N >> 2, slices = NT / nq;
    const int q = f.q, sl_raw = f.sl_raw, sl = min(sl_raw, slices - 1);
    f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = sl + u * slices;
      const f4 nx = acc + x[min(k, K - 1)] * f.w[u];
      acc = k < K ? nx : acc;
    }
    for (int k0 = sl + U * slices; k0 < K; k0 += R * slices) {
      f4 w[R];
#pragma unroll
      for (int u = 0; u < R; ++u) w[u] = *reinterpret_cast<const f4*>(wt + (unsigned)(min(k0 + u * slices, K - 1) * N + 4 * q));
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const int k = k0 + u * slices;
        const f4 nx = acc + x[min(k, K - 1)] * w[u];
        acc = k < K ? nx : acc;
      }
    }
    if (sl_raw < slices) *reinterpret_cast<f4*>(part + sl * N + 4 * q) = acc;
    __syncthreads();
    for (int n = tid; n < N; n += NT) {
      float acc1 = b ? (n == tid ? f.bias : b[n]) : 0.0f;
      for (int i = 0; i < slices; ++i) acc1 += part[i * N + n];
      y[n] = acc1;
    }
  } else if (N <= NT) {
    const int slices = NT / N;
    const int n = tid % N, sl = tid / N;
    if (sl < slices) {
      float acc = 0.0f;
      for (int k = sl; k < K; k += slices) acc = fmaf(x[k], wt[(long long)k * N + n], acc);
      part[sl * N + n] = acc;
    }
    __syncthreads();
    if (tid < N) {
      float acc = b ? f.bias : 0.0f;
      for (int i = 0; i < slices; ++i) acc += part[i * N + tid];
      y[tid] = acc;
    }
  } else {
    for (int n = tid; n < N; n += NT) {
      float acc = b ? b[n] : 0.0f;
      const float* wp = wt + n;
#pragma unroll 4
      for (int k = 0; k < K; ++k) acc = fmaf(x[k], wp[(long long)k * N], acc);
      y[n] = acc;
    }
  }
}

// a Linear with nothing in front of it to hide its first loads behind
template <int NT>
__device__ __forceinline__ void linear_t(float* y, const float* x, const float* __restrict__ wt,
                                         const float* __restrict__ b, int K, int N, float* part) {
  LinFrag<LinRound<NT>::n> f;
  lin_issue<NT>(f, wt, b, K, N);
  lin_run<NT>(y, x, f, wt, b, K, N, part);
}

// LayerNorm; its parameters are requested before the two block reductions (four barriers), not after them.
template <int NT>
__device__ __forceinline__ void layer_norm(float* y, const float* x, const float* __restrict__ w,
                                           const float* __restrict__ b, int C, float* red) {
  const int tid = tid_here();
  const float w0 = w[min(tid, C - 1)], b0 = b[min(tid, C - 1)];
  float s = 0.0f;
  for (int i = tid; i < C; i += NT) s += x[i];
  const float mean = block_sum<NT>(s, red, tid_here()) / C;
  float q = 0.0f;
  for (int i = tid; i < C; i += NT) { const float d = x[i] - mean; q += d * d; }
  const float var = block_sum<NT>(q, red, tid_here()) / C;
  const float rstd = 1.0f / sqrtf(var + 1e-5f);
  for (int i = tid; i < C; i += NT) {
    const float wi = i == tid ? w0 : w[i], bi = i == tid ? b0 : b[i];
    y[i] = (x[i] - mean) * rstd * wi + bi;
  }
  __syncthreads();
}

template <int NT>
__global__ __launch_bounds__(NT) void gpt_step_kernel(GptStepArgs a) {
  constexpr int GPT_WAVES = NT / 64;
  if (gpt_step_skipped(a)) return;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int C = a.C, tid = threadIdx.x, b = blockIdx.x;
  float* x = sm;                 // [C]   residual stream
  float* h = x + C;              // [C]   LN output / attention output
  float* qkv = h + C;            // [3C]
  float* mlp = qkv + 3 * C;      // [4C]  also the concatenated embedding parts
  float* att = mlp + 4 * C;      // [n_head * Tmax]
  float* red = att + a.n_head * a.Tmax;   // [GPT_WAVES]
  float* lg = red + GPT_WAVES;   // [16]  logits
  float* part = sm + ((9 * C + a.n_head * a.Tmax + GPT_WAVES + 16 + 3) & ~3);   // [4 * NT] split-K partials of linear_t (16-B aligned)
  float* kl = part + 4 * NT;     // [Tmax * C] the agent's K rows of the current layer
  float* vl = kl + a.Tmax * C;   // [Tmax * C] its V rows

  // first K-slice rows of a thread held in registers ahead of the Linear: all of them at n_embd = 48 (7 / 3 / 10 / 10
  // for qkv / proj / fc / fc2); the 1024-thread form has 128 VGPRs per thread and takes the rest in rounds
  constexpr int UQ = NT == 256 ? 7 : 1, UP = NT == 256 ? 3 : 1, UF = NT == 256 ? 10 : 1, UF2 = NT == 256 ? 10 : 1;
  constexpr int KVU = NT == 256 ? 2 : 1;         // K / V quads per thread requested ahead of ln_1 (covers 20 x 48 floats; the rest follows after it)
  // touch registers per thread: the entry run / the K, V rows / a layer's run (touch_issue takes one more round of a
  // run's lines on the spot; K, V lines past TK * NT are left to their own loads)
  constexpr int TU = NT == 256 ? 8 : 2, TK = NT == 256 ? 3 : 1, TL = NT == 256 ? 2 : 1;
  constexpr long long PF_ENTRY = 1 << 18;     // floats warmed at entry (1 MB: well inside one XCD's 4 MB of L2) ...

  const int t = a.step;
  const int hs = C / a.n_head;
  const float scale = 1.0f / sqrtf((float)hs);
  int len = a.cache_len[b];      // tokens already cached (0 at the start of a sequence)
  const int n_new = (a.src_mode == GPT_SRC_ENV && t == 0) ? 2 : 1;
  const GptLayerPtrs L0 = a.layers[0];
  // Workgroups are dealt to the 8 XCDs round-robin, and L2 is per XCD: the B / 8 workgroups of one XCD share the touches.
  // (Were the dealing different, some lines would be touched twice and others not: slower, not wrong.)
  const int nshare = max(1, a.B >> 3), share = (b >> 3) % nshare;
  const long long pf_entry = min(a.pf_floats, PF_ENTRY);
  // ... a wider model's remaining parameters follow layer by layer, about half a layer ahead of their use
  const long long pf_layer = a.n_layer > 0 ? (a.pf_floats - pf_entry + a.n_layer - 1) / a.n_layer : 0;
  Touch<TU> tw;
  Touch<TK> tkv;
  auto warm = [&]() {
    touch_issue<NT>(tw, a.pf_base, 0, pf_entry, share, nshare);
    // the agent's cached K / V rows [0, len) of every layer: (layer, K | V, line) flattened over the threads
    const int nlk = (len * C + 31) >> 5, total = a.n_layer * 2 * nlk;
#pragma unroll
    for (int u = 0; u < TK; ++u) {
      tkv.r[u] = 0u;
      if (total > 0) {
        const int f = min(tid + u * NT, total - 1), lyr = f / (2 * nlk), r = f - lyr * 2 * nlk, kv = r >= nlk, line = r - kv * nlk;
        const float* row = (kv ? a.vcache : a.kcache) + (((long long)lyr * a.B + b) * a.Tmax) * C;
        tkv.r[u] = reinterpret_cast<const uint32_t*>(row)[min(line * 32, len * C - 1)];
      }
    }
    tkv.extra = 0u;
  };

  for (int j = 0; j < n_new; ++j) {
    const int tid = tid_here();       // (shadows the kernel's: per-token arithmetic stays inside the loop)
    const bool warm_now = j == 0 && !a.embed_only;
    // ---------------- token embedding ----------------
    const GptTokSrc ts = gpt_tok_src(a, b, j);
    if (ts.direct) {                       // the class token or a given embedding: the row as it is
      for (int i = tid; i < C; i += NT) x[i] = ts.direct[i];
      if (warm_now) warm();
    } else {
      const int act = ts.act, row = ts.row, col = ts.col;
      float* parts = mlp;
      int p = 0;
      for (int i = tid; i < C; i += NT) parts[i] = a.wte[act * C + i];
      ++p;
      for (int i = tid; i < C; i += NT) parts[p * C + i] = gpt_pos1d(a, a.pos_index, i);
      ++p;
      if (!a.no_patch_emb) {
        if (a.src_mode == GPT_SRC_ENV) {
          for (int i = tid; i < C; i += NT) {
            const float s = sum_parts(a.efpn_lin_b[i], a.emb_part + (long long)b * a.KS * C + i, (long long)C, a.KS);   // ascending, behind the bias
            parts[p * C + i] = s;
            if (a.tok_emb_out) a.tok_emb_out[((long long)b * a.T + t) * C + i] = s;
          }
        } else {
          const float* pe = a.tok_emb + ((long long)b * a.tok_emb_stride + a.tok_emb_index) * C;
          for (int i = tid; i < C; i += NT) parts[p * C + i] = pe[i];
        }
        ++p;
      }
      if (a.use_pos_emb) {
        for (int i = tid; i < C; i += NT) parts[p * C + i] = gpt_pos2d(a, row, col, i);
        ++p;
      }
      if (warm_now) warm();      // behind the embedding's own loads: loads return in order
      __syncthreads();
      if (a.concat_emb) {
        linear_t<NT>(x, parts, a.proj_wt, a.proj_b, p * C, C, part);
      } else {
        for (int i = tid; i < C; i += NT) {
          float s = 0.0f;
          for (int q = 0; q < p; ++q) s += parts[q * C + i];
          x[i] = s / p;
        }
      }
    }
    __syncthreads();
    if (warm_now) { touch_sink(tw); touch_sink(tkv); }
    if (a.out.final_emb)
      for (int i = tid; i < C; i += NT) a.out.final_emb[((long long)b * a.emb_stride + len) * C + i] = x[i];
    if (a.embed_only) { ++len; continue; }
    const bool drop = a.pdrop > 0.0f;
    if (drop) {                                           // x = transformer.drop(final_emb), gpt.py:525
      for (int i = tid; i < C; i += NT) x[i] *= drop_scale(a.drop_seed, b, len, 0, 0, i, a.pdrop);
      __syncthreads();
    }

    // ---------------- transformer blocks ----------------
    GptLayerPtrs Ln = L0;
    for (int l = 0; l < a.n_layer; ++l) {
      const int tid = tid_here();     // (and per-layer arithmetic inside the layer)
      const GptLayerPtrs L = Ln;
      if (l + 1 < a.n_layer) Ln = a.layers[l + 1];
      float* kc = a.kcache + (((long long)l * a.B + b) * a.Tmax) * C;
      float* vc = a.vcache + (((long long)l * a.B + b) * a.Tmax) * C;
      // requested now, used after ln_1: the qkv fragment and the cached K / V rows [0, len)
      LinFrag<UQ> fq;
      lin_issue<NT>(fq, L.qkv_wt, L.qkv_b, C, 3 * C);
      const bool quads = (C & 3) == 0;
      const bool kv_lds = a.kv_lds != 0;       // the launcher's: the rows fit beside the rest (else they stay in global)
      const int n4 = quads && kv_lds ? (len * C) >> 2 : 0;
      const f4* kc4 = reinterpret_cast<const f4*>(kc);
      const f4* vc4 = reinterpret_cast<const f4*>(vc);
      f4 kr[KVU], vr[KVU];
#pragma unroll
      for (int u = 0; u < KVU; ++u) {
        kr[u] = f4{0.f, 0.f, 0.f, 0.f}; vr[u] = kr[u];
        if (n4 > 0) { const int e = min(tid + u * NT, n4 - 1); kr[u] = kc4[e]; vr[u] = vc4[e]; }
      }
      layer_norm<NT>(h, x, L.ln1_w, L.ln1_b, C, red);
      Touch<TL> tl;
      touch_issue<NT>(tl, a.pf_base, pf_entry + l * pf_layer, min(a.pf_floats, pf_entry + (l + 1) * pf_layer), share, nshare);
      if (!kv_lds) {
      } else if (quads) {
#pragma unroll
        for (int u = 0; u < KVU; ++u) {
          const int e = tid + u * NT;
          if (e < n4) { reinterpret_cast<f4*>(kl)[e] = kr[u]; reinterpret_cast<f4*>(vl)[e] = vr[u]; }
        }
        for (int e = tid + KVU * NT; e < n4; e += NT) { reinterpret_cast<f4*>(kl)[e] = kc4[e]; reinterpret_cast<f4*>(vl)[e] = vc4[e]; }
      } else {
        for (int e = tid; e < len * C; e += NT) { kl[e] = kc[e]; vl[e] = vc[e]; }
      }
      lin_run<NT>(qkv, h, fq, L.qkv_wt, L.qkv_b, C, 3 * C, part);
      touch_sink(tl);
      LinFrag<UP> fp;
      lin_issue<NT>(fp, L.proj_wt, L.proj_b, C, C);
      LinFrag<UF> ff;
      lin_issue<NT>(ff, L.fc_wt, L.fc_b, C, 4 * C);
      __syncthreads();
      for (int i = tid; i < C; i += NT) {
        const float kn = qkv[C + i], vn = qkv[2 * C + i];
        kc[len * C + i] = kn; vc[len * C + i] = vn;
        if (kv_lds) { kl[len * C + i] = kn; vl[len * C + i] = vn; }
      }
      __syncthreads();   // own-block global writes are visible to the block after the barrier
      const int nk = len + 1;
      // (the rows in LDS or, for a workgroup they do not fit into, in the cache itself: the same values in the same order)
      const float* kk = kv_lds ? kl : kc;
      const float* vv = kv_lds ? vl : vc;
      for (int e = tid; e < a.n_head * nk; e += NT) {
        const int hd = e / nk, s = e - hd * nk;
        const float* kp = kk + s * C + hd * hs;
        const float* qp = qkv + hd * hs;
        float d = 0.0f;
        for (int i = 0; i < hs; ++i) d = fmaf(qp[i], kp[i], d);
        att[hd * a.Tmax + s] = d * scale;
      }
      __syncthreads();
      if (tid < a.n_head) {
        float* ap = att + tid * a.Tmax;
        float m = -INFINITY;
        for (int s = 0; s < nk; ++s) m = fmaxf(m, ap[s]);
        float sum = 0.0f;
        for (int s = 0; s < nk; ++s) { const float ev = expf(ap[s] - m); ap[s] = ev; sum += ev; }
        const float inv = 1.0f / sum;
        for (int s = 0; s < nk; ++s) ap[s] *= inv;
        if (drop)                                         // attn_dropout on the probabilities, gpt.py:100
          for (int s = 0; s < nk; ++s) ap[s] *= drop_scale(a.drop_seed, b, len, l, 1, tid * a.Tmax + s, a.pdrop);
      }
      __syncthreads();
      for (int i = tid; i < C; i += NT) {
        const int hd = i / hs;
        float acc = 0.0f;
        for (int s = 0; s < nk; ++s) acc = fmaf(att[hd * a.Tmax + s], vv[s * C + i], acc);
        h[i] = acc;
      }
      __syncthreads();
      lin_run<NT>(qkv, h, fp, L.proj_wt, L.proj_b, C, C, part);   // qkv[0:C] reused as scratch
      LinFrag<UF2> f2;
      lin_issue<NT>(f2, L.fc2_wt, L.fc2_b, 4 * C, C);
      __syncthreads();
      for (int i = tid; i < C; i += NT) x[i] += drop ? qkv[i] * drop_scale(a.drop_seed, b, len, l, 2, i, a.pdrop) : qkv[i];
      __syncthreads();
      layer_norm<NT>(h, x, L.ln2_w, L.ln2_b, C, red);
      lin_run<NT>(mlp, h, ff, L.fc_wt, L.fc_b, C, 4 * C, part);
      __syncthreads();
      for (int i = tid; i < 4 * C; i += NT) mlp[i] = gelu_tanh(mlp[i]);
      __syncthreads();
      lin_run<NT>(qkv, mlp, f2, L.fc2_wt, L.fc2_b, 4 * C, C, part);
      __syncthreads();
      for (int i = tid; i < C; i += NT) x[i] += drop ? qkv[i] * drop_scale(a.drop_seed, b, len, l, 3, i, a.pdrop) : qkv[i];
      __syncthreads();
    }
    ++len;
  }

  if (a.embed_only) {
    if (tid == 0) a.cache_len[b] = len;
    return;
  }
  // ---------------- head on the newest token ----------------
  layer_norm<NT>(h, x, a.lnf_w, a.lnf_b, C, red);
  linear_t<NT>(lg, h, a.head_wt, nullptr, C, a.nA, part);
  __syncthreads();

  if (a.src_mode != GPT_SRC_ENV) {
    if (tid == 0) a.cache_len[b] = len;
    if (a.logits_rows && tid < a.nA) a.logits_rows[(long long)b * a.logits_stride + tid] = lg[tid];
    return;
  }
  if (tid == 0) { if (a.mask_policy) gpt_decide_and_step_masked(a, b, lg, len); else gpt_decide_and_step(a, b, lg, len); }
}

// The agent's K / V rows of a layer are staged in LDS when the workgroup then still fits a CU's 160 KB (every model of
// the zoo at its block sizes; n_embd 192 up to a block size in the high eighties).  jn_create admits more (n_embd <= 256, block_size <= 255):
// there, or if the runtime refuses the size, the rows are read from the cache in global memory — the same bits, slower.
constexpr size_t GPT_LDS_MAX = 160 * 1024;

int launch_gpt_step(const GptStepArgs& a0, hipStream_t s) {
  GptStepArgs a = a0;
  const int nt = a.C <= 64 ? 256 : 1024;
  const size_t base = (size_t)(9 * a.C + a.n_head * a.Tmax + nt / 64 + 16 + 4 + 4 * nt) * sizeof(float);
  const size_t with_kv = base + (size_t)2 * a.Tmax * a.C * sizeof(float);
  a.kv_lds = with_kv <= GPT_LDS_MAX;
  // past the default limit of dynamic LDS (gpt-mini: 2 x 33 x 192 floats -> 75 KB) the size has to be granted
  if (a.kv_lds && !(nt == 256 ? allow_lds<&gpt_step_kernel<256>>(with_kv) : allow_lds<&gpt_step_kernel<1024>>(with_kv))) {
    (void)hipGetLastError();      // refused: the launch below must not report the refusal as its own error
    a.kv_lds = 0;
  }
  const size_t smem = a.kv_lds ? with_kv : base;
  if (nt == 256) hipLaunchKernelGGL(gpt_step_kernel<256>, dim3(a.B), dim3(256), smem, s, a);
  else hipLaunchKernelGGL(gpt_step_kernel<1024>, dim3(a.B), dim3(1024), smem, s, a);
  return hipGetLastError() == hipSuccess ? 0 : 1;      // a launch that was refused is an error, not a step that did nothing
}

}  // namespace jnr
