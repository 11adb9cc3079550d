// The decision step for wide models (256 < n_embd <= 1024, a multiple of 64): the same function as gpt_step_kernel
// (kernels_gpt.hip), as a short chain of launches over ALL B agents instead of one workgroup per agent.
//
// Why another route: gpt_step_kernel streams the whole model once per agent (12 L C^2 floats: 101 MB for gopher-44m,
// 340 MB for gpt2, 1.2 GB for gpt2-medium), B times per step.  Here every Linear is one skinny fp32 GEMM
//   Y[M = B][N] = X[M][K] . Wt[K][N]
// spread over the whole GPU, so a weight element is read from HBM once per step whatever B is:
//   * a workgroup owns (K slice, 64 rows, 64 columns), multiplies on v_mfma_f32_16x16x4_f32 (fp32 operands: the kernel
//     waits for HBM, a bf16 split would buy nothing) and writes a partial [KS][M][N];
//   * the consumer — LayerNorm, attention, the next GEMM's operand load, the tail — adds the KS partials in ascending
//     slice order behind the bias.  No float atomics anywhere: two runs give the same bits.
// Per layer: ln_1 (folds the residual of the previous fc2), qkv GEMM, attention (one workgroup per agent and head,
// appends the K / V row to the cache [L][B][Tmax][C]), proj GEMM, ln_2 (folds the proj residual), fc GEMM, fc2 GEMM
// (operand = gelu(partials + bias)): 7 launches; with the embedding and the tail 7 L + 2 per token (+ 2 with concat_emb).
// Dropout: drop_scale of jn_device.h with gpt_step_kernel's keys, so the batched backward differentiates this forward.
// The token source, the skipped-step prologue and the decision with its env step are the functions of jn_gpt_device.h
// that gpt_step_kernel calls.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "jn_gpt_device.h"

namespace jnr {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int WT = 256;                     // threads of every kernel here but the attention's
constexpr int WG_KC = 32;                   // K rows staged per round; every K of the route is a multiple of 64
constexpr int WG_CH = 4;                    // rounds per K slice at most: the slice's operands wait in registers
constexpr int WG_LDX = WG_KC + 4, WG_LDW = 64 + 4;
constexpr int WIDE_WGS = 256;               // workgroups a Linear should launch at least: one per CU
constexpr int WIDE_KS_MAX = 32;
constexpr int WIDE_CQ = GPT_WIDE_MAX_C / WT;   // residual elements per thread of a row

// ---- the skinny GEMM -------------------------------------------------------------------------------------------------
struct WideGemm {
  const float* X;        // operand [M][K]; with xparts > 0 the partials [xparts][M][K] of the Linear in front
  const float* xbias;    // [K], with xparts
  int xparts;            // > 0: the operand is gelu(bias + partials in ascending order)
  const float* Wt;       // [K][N]
  float* part;           // out: [KS][M][N]
  int M, K, N, kper;     // kper: K rows per slice, 1 .. WG_CH times WG_KC
  const int* skip_flag; int skip_when;
};

__global__ __launch_bounds__(WT) void gptw_gemm_kernel(WideGemm g) {
  if (step_skipped(g.skip_flag, g.skip_when)) return;
  __shared__ __attribute__((aligned(16))) float Xs[64 * WG_LDX];
  __shared__ __attribute__((aligned(16))) float Ws[WG_KC * WG_LDW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, gq = lane >> 4;
  const int ks = blockIdx.x, m0 = blockIdx.y * 64, n0 = blockIdx.z * 64;
  const int kb = ks * g.kper, ke = min(g.K, kb + g.kper);
  const int nch = (ke - kb) / WG_KC;                          // 1 .. WG_CH whole rounds
  f32x4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  // The whole slice is requested before the first round is used: the weights come from HBM, and a round's arithmetic is
  // far too short to hide that latency round by round.  Rounds past the slice's end ask for its last round again
  // (a clamped address, not a branch around the load) and are left out below.
  f32x4 wreg[WG_CH][2], xreg[WG_CH][2];
#pragma unroll
  for (int c = 0; c < WG_CH; ++c) {
    const int k0 = kb + min(c, nch - 1) * WG_KC;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = tid + u * WT;
      wreg[c][u] = *reinterpret_cast<const f32x4*>(g.Wt + (long long)(k0 + (i >> 4)) * g.N + n0 + 4 * (i & 15));
      xreg[c][u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (g.xparts == 0)
        xreg[c][u] = *reinterpret_cast<const f32x4*>(g.X + (long long)min(m0 + (i >> 3), g.M - 1) * g.K + k0 + 4 * (i & 7));
    }
  }
#pragma unroll
  for (int c = 0; c < WG_CH; ++c) {
    if (c >= nch) break;
    const int k0 = kb + c * WG_KC;
    if (c) __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = tid + u * WT;
      *reinterpret_cast<f32x4*>(Ws + (i >> 4) * WG_LDW + 4 * (i & 15)) = wreg[c][u];
      const int r = i >> 3, q = i & 7, m = m0 + r, k = k0 + 4 * q;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (m < g.M) {                                          // rows past M are masked
        if (g.xparts == 0) {
          v = xreg[c][u];
        } else {
          v = sum_parts(*reinterpret_cast<const f32x4*>(g.xbias + k), g.X + (long long)m * g.K + k, (long long)g.M * g.K, g.xparts);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = gelu_tanh(v[e]);
        }
      }
      *reinterpret_cast<f32x4*>(Xs + r * WG_LDX + 4 * q) = v;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < WG_KC; kk += 16) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(Xs + (16 * wave + lm) * WG_LDX + kk + 4 * gq);   // A[i = row][k perm]
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float* wr = Ws + (kk + 4 * gq + j) * WG_LDW + lm;
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], wr[16 * t], acc[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + 16 * wave + 4 * gq + r, n = n0 + 16 * c + lm;
      if (m < g.M) g.part[((long long)ks * g.M + m) * g.N + n] = acc[c][r];
    }
}

struct Split { int KS, kper; };

// K slices of a Linear over M rows: enough workgroups for one resident round, slices of 1 .. WG_CH whole rounds
// (K <= 4096: at most WIDE_KS_MAX slices either way)
Split wide_split(int K, int N, int M) {
  const int tiles = ((M + 63) / 64) * (N / 64);
  int want = (WIDE_WGS + tiles - 1) / tiles;
  want = std::max(1, std::min(want, std::min(K / WG_KC, WIDE_KS_MAX)));
  Split sp;
  sp.kper = std::min(((K + want - 1) / want + WG_KC - 1) / WG_KC * WG_KC, WG_CH * WG_KC);
  sp.KS = (K + sp.kper - 1) / sp.kper;
  return sp;
}

// scratch of one step over B agents, in floats
struct WideLayout { size_t X, H, AO, E, PA, PB, total; };

WideLayout wide_layout(int C, int n_parts, int B) {
  const size_t BC = (size_t)B * C;
  WideLayout y;
  y.X = 0; y.H = BC; y.AO = 2 * BC; y.E = 3 * BC; y.PA = y.E + BC * std::max(n_parts, 1);
  const size_t pa = std::max((size_t)wide_split(C, 3 * C, B).KS * 3, (size_t)wide_split(C, 4 * C, B).KS * 4) * BC;
  size_t pb = std::max(wide_split(C, C, B).KS, wide_split(4 * C, C, B).KS);
  pb = std::max(pb, (size_t)wide_split(std::max(n_parts, 1) * C, C, B).KS) * BC;
  y.PB = y.PA + pa;
  y.total = y.PB + pb;
  return y;
}

// ---- residual + LayerNorm of one row ---------------------------------------------------------------------------------
struct WideLn {
  float* X;                                     // [B][C] residual stream, updated in place
  const float* part; int nparts; const float* pbias;   // the branch to add first: partials [nparts][B][C] + bias (null: none)
  int layer, site;                              // dropout key of that branch
  const float *w, *b;                           // LayerNorm parameters
  const int32_t* cache_len; int tok_j;          // the token's index in its sequence = cache_len[agent] + tok_j
  int B, C;
  float pdrop; uint64_t seed;
};

// x += drop(branch); out = LayerNorm(x) (gpt_step_kernel's layer_norm: two passes, biased variance, eps 1e-5).
// All WT threads of the workgroup of agent `b`; out may be LDS or global.
__device__ __forceinline__ void wide_ln_row(const WideLn& a, int b, float* out, float* red) {
  const int tid = threadIdx.x, C = a.C;
  const int len = a.cache_len[b] + a.tok_j;
  float xv[WIDE_CQ], rv[WIDE_CQ];
  // the branch's partials of all of the thread's elements together: 8 slices x WIDE_CQ elements in flight
#pragma unroll
  for (int u = 0; u < WIDE_CQ; ++u) rv[u] = a.part ? a.pbias[min(tid + u * WT, C - 1)] : 0.0f;
  if (a.part) {
    const long long st = (long long)a.B * C;
    for (int k0 = 0; k0 < a.nparts; k0 += 8) {
      float v[WIDE_CQ][8];
#pragma unroll
      for (int u = 0; u < WIDE_CQ; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) v[u][j] = a.part[(long long)min(k0 + j, a.nparts - 1) * st + (long long)b * C + min(tid + u * WT, C - 1)];
#pragma unroll
      for (int u = 0; u < WIDE_CQ; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float nx = rv[u] + v[u][j]; rv[u] = k0 + j < a.nparts ? nx : rv[u]; }
    }
  }
  float s = 0.0f;
#pragma unroll
  for (int u = 0; u < WIDE_CQ; ++u) {
    const int i = tid + u * WT;
    xv[u] = 0.0f;
    if (i < C) {
      float x = a.X[(long long)b * C + i];
      if (a.part) {
        const float r = rv[u];
        x += a.pdrop > 0.0f ? r * drop_scale(a.seed, b, len, a.layer, a.site, i, a.pdrop) : r;
        a.X[(long long)b * C + i] = x;
      }
      xv[u] = x;
      s += x;
    }
  }
  const float mean = block_sum<WT>(s, red, tid) / C;
  float q = 0.0f;
#pragma unroll
  for (int u = 0; u < WIDE_CQ; ++u)
    if (tid + u * WT < C) { const float d = xv[u] - mean; q += d * d; }
  const float var = block_sum<WT>(q, red, tid) / C;
  const float rstd = 1.0f / sqrtf(var + 1e-5f);
#pragma unroll
  for (int u = 0; u < WIDE_CQ; ++u) {
    const int i = tid + u * WT;
    if (i < C) out[i] = (xv[u] - mean) * rstd * a.w[i] + a.b[i];
  }
}

__global__ __launch_bounds__(WT) void gptw_ln_kernel(WideLn a, float* H, const int* skip_flag, int skip_when) {
  if (step_skipped(skip_flag, skip_when)) return;
  __shared__ float red[WT / 64];
  wide_ln_row(a, blockIdx.x, H + (long long)blockIdx.x * a.C, red);
}

// ---- token embedding (gpt.py:419-479), the four sources of gpt_step_kernel -------------------------------------------
// Token `j` of this step (j = 1 only for the first patch behind the class token at step 0 of a rollout).  Without
// concat_emb, and for the class and given tokens, the embedding is final here: out.final_emb, then the embedding
// dropout into X.  With concat_emb the parts go to E [B][n_parts * C] for project_concat's GEMM (gptw_embed_finish_kernel).
__global__ __launch_bounds__(WT) void gptw_embed_kernel(GptStepArgs a, int j, int last, float* X, float* E) {
  if (step_skipped(a.skip_flag, a.skip_when)) return;
  const int C = a.C, tid = threadIdx.x, b = blockIdx.x, t = a.step;
  const int len = a.cache_len[b] + j;
  const GptTokSrc ts = gpt_tok_src(a, b, j);
  const bool to_gemm = ts.kind.to_gemm;
  const int act = ts.act, row = ts.row, col = ts.col;
  const float* direct = ts.direct;
  for (int i = tid; i < C; i += WT) {
    float x;
    if (direct) {
      x = direct[i];
    } else {
      f32x4 v;       // (a vector, not an array: indexed by p, an array went to 4 KB of LDS here and the step cost 3 % more)
      int p = 0;
      v[p++] = a.wte[act * C + i];
      v[p++] = gpt_pos1d(a, a.pos_index, i);
      if (!a.no_patch_emb) {
        if (a.src_mode == GPT_SRC_ENV) {
          const float s = sum_parts(a.efpn_lin_b[i], a.emb_part + (long long)b * a.KS * C + i, (long long)C, a.KS);   // ascending, behind the bias
          if (a.tok_emb_out) a.tok_emb_out[((long long)b * a.T + t) * C + i] = s;
          v[p++] = s;
        } else {
          v[p++] = a.tok_emb[((long long)b * a.tok_emb_stride + a.tok_emb_index) * C + i];
        }
      }
      if (a.use_pos_emb) v[p++] = gpt_pos2d(a, row, col, i);
      if (to_gemm) {
        for (int q = 0; q < p; ++q) E[((long long)b * p + q) * C + i] = v[q];
        continue;
      }
      float s = 0.0f;
      for (int q = 0; q < p; ++q) s += v[q];
      x = s / p;
    }
    if (a.out.final_emb) a.out.final_emb[((long long)b * a.emb_stride + len) * C + i] = x;
    if (!a.embed_only) X[(long long)b * C + i] = a.pdrop > 0.0f ? x * drop_scale(a.drop_seed, b, len, 0, 0, i, a.pdrop) : x;
  }
  if (a.embed_only && last && !to_gemm) {
    __syncthreads();               // every thread has read cache_len
    if (tid == 0) a.cache_len[b] = len + 1;
  }
}

// project_concat's partials [nparts][B][C] + bias -> final_emb, X
__global__ __launch_bounds__(WT) void gptw_embed_finish_kernel(GptStepArgs a, int j, int last, const float* part, int nparts, float* X) {
  if (step_skipped(a.skip_flag, a.skip_when)) return;
  const int C = a.C, tid = threadIdx.x, b = blockIdx.x;
  const int len = a.cache_len[b] + j;
  for (int i = tid; i < C; i += WT) {
    const float x = sum_parts(a.proj_b[i], part + (long long)b * C + i, (long long)a.B * C, nparts);
    if (a.out.final_emb) a.out.final_emb[((long long)b * a.emb_stride + len) * C + i] = x;
    if (!a.embed_only) X[(long long)b * C + i] = a.pdrop > 0.0f ? x * drop_scale(a.drop_seed, b, len, 0, 0, i, a.pdrop) : x;
  }
  if (a.embed_only && last) {
    __syncthreads();
    if (tid == 0) a.cache_len[b] = len + 1;
  }
}

// ---- attention of the new token: one workgroup (one wave) per (head, agent) -------------------------------------------
struct WideAttn {
  const float* part; int nparts; const float* qkv_b;   // qkv partials [nparts][B][3C] + bias
  float *kc, *vc;                 // this layer's cache [B][Tmax][C]
  float* AO;                      // out [B][C]
  const int32_t* cache_len; int tok_j;
  int B, C, n_head, Tmax, layer;
  float pdrop; uint64_t seed;
  const int* skip_flag; int skip_when;
};

__global__ __launch_bounds__(64) void gptw_attn_kernel(WideAttn a) {
  if (step_skipped(a.skip_flag, a.skip_when)) return;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, hd = blockIdx.x, b = blockIdx.y, C = a.C, hs = C / a.n_head;
  const int len = a.cache_len[b] + a.tok_j, nk = len + 1;
  if (len >= a.Tmax) return;       // (the callers never decode past block_size + 1 tokens)
  float* q = sm;                   // [hs]
  float* kn = q + hs;              // [hs] the new K row's slice of this head
  float* vn = kn + hs;             // [hs]
  float* att = vn + hs;            // [Tmax]
  float* kc = a.kc + (long long)b * a.Tmax * C + hd * hs;
  float* vc = a.vc + (long long)b * a.Tmax * C + hd * hs;
  for (int i = tid; i < hs; i += 64) {
    const int c = hd * hs + i;
    const float* r = a.part + (long long)b * 3 * C + c;
    const long long st = (long long)a.B * 3 * C;
    float qv = a.qkv_b[c], kv = a.qkv_b[C + c], vv = a.qkv_b[2 * C + c];
    for (int k0 = 0; k0 < a.nparts; k0 += 8) {       // q, k and v of 8 slices in flight (sum_parts, three at a time)
      float pq[8], pk[8], pv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float* ru = r + (long long)min(k0 + u, a.nparts - 1) * st;
        pq[u] = ru[0]; pk[u] = ru[C]; pv[u] = ru[2 * C];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool in = k0 + u < a.nparts;
        const float nq = qv + pq[u], nk2 = kv + pk[u], nv = vv + pv[u];
        qv = in ? nq : qv; kv = in ? nk2 : kv; vv = in ? nv : vv;
      }
    }
    q[i] = qv; kn[i] = kv; vn[i] = vv;
    kc[(long long)len * C + i] = kv; vc[(long long)len * C + i] = vv;
  }
  __syncthreads();
  const float scale = 1.0f / sqrtf((float)hs);
  for (int s = tid; s < nk; s += 64) {
    const float* kp = s == len ? kn : kc + (long long)s * C;
    float d = 0.0f;
    for (int i = 0; i < hs; ++i) d = fmaf(q[i], kp[i], d);
    att[s] = d * scale;
  }
  __syncthreads();
  if (tid == 0) {
    float m = -INFINITY;
    for (int s = 0; s < nk; ++s) m = fmaxf(m, att[s]);
    float sum = 0.0f;
    for (int s = 0; s < nk; ++s) { const float ev = expf(att[s] - m); att[s] = ev; sum += ev; }
    const float inv = 1.0f / sum;
    for (int s = 0; s < nk; ++s) att[s] *= inv;
    if (a.pdrop > 0.0f)                                     // attn_dropout on the probabilities, gpt.py:100
      for (int s = 0; s < nk; ++s) att[s] *= drop_scale(a.seed, b, len, a.layer, 1, hd * a.Tmax + s, a.pdrop);
  }
  __syncthreads();
  for (int i = tid; i < hs; i += 64) {
    float acc = 0.0f;
    for (int s = 0; s < nk; ++s) acc = fmaf(att[s], s == len ? vn[i] : vc[(long long)s * C + i], acc);
    a.AO[(long long)b * C + hd * hs + i] = acc;
  }
}

// ---- tail: last residual, ln_f, head, decision, env step, bookkeeping; one workgroup per agent -------------------------
__global__ __launch_bounds__(WT) void gptw_tail_kernel(GptStepArgs a, WideLn ln) {
  if (gpt_step_skipped(a)) return;
  __shared__ float h[GPT_WIDE_MAX_C];
  __shared__ float red[WT / 64];
  __shared__ float hp[WT / 64][16];
  __shared__ float lg[16];
  const int tid = threadIdx.x, b = blockIdx.x, C = a.C, nA = a.nA;
  const int len = a.cache_len[b] + ln.tok_j + 1;      // tokens cached once this step is done
  wide_ln_row(ln, b, h, red);
  __syncthreads();
  float acc[9];
#pragma unroll
  for (int n = 0; n < 9; ++n) acc[n] = 0.0f;
  for (int k = tid; k < C; k += WT) {
    const float hv = h[k];
#pragma unroll
    for (int n = 0; n < 9; ++n)
      if (n < nA) acc[n] = fmaf(hv, a.head_wt[k * nA + n], acc[n]);
  }
#pragma unroll
  for (int n = 0; n < 9; ++n) {
    const float v = wave_sum(acc[n]);
    if ((tid & 63) == 0) hp[tid >> 6][n] = v;
  }
  __syncthreads();
  if (tid < nA) {
    float v = 0.0f;
#pragma unroll
    for (int w = 0; w < WT / 64; ++w) v += hp[w][tid];
    lg[tid] = v;
  }
  __syncthreads();

  if (a.src_mode != GPT_SRC_ENV) {
    if (tid == 0) a.cache_len[b] = len;
    if (a.logits_rows && tid < nA) a.logits_rows[(long long)b * a.logits_stride + tid] = lg[tid];
    return;
  }
  if (tid == 0) { if (a.mask_policy) gpt_decide_and_step_masked(a, b, lg, len); else gpt_decide_and_step(a, b, lg, len); }
}

}  // namespace

size_t gpt_wide_scratch_floats(int C, int n_parts, int max_batch) {
  // the slice count of a Linear falls as the row blocks grow: the largest layout over the row-block counts
  size_t need = 0;
  for (int rb = 1; rb <= (max_batch + 63) / 64; ++rb) need = std::max(need, wide_layout(C, n_parts, std::min(rb * 64, max_batch)).total);
  return need + 64;
}

int launch_gpt_step_wide(const GptStepArgs& a, hipStream_t s) {
  const int C = a.C, B = a.B, nL = a.n_layer;
  if (!a.wide_scratch || (nL > 0 && !a.layers_host) || B < 1 || a.nA > 9 || !gpt_wide_admits(C, a.n_head, a.Tmax - 1)) return 1;
  const WideLayout y = wide_layout(C, a.n_parts, B);
  float* sc = a.wide_scratch;
  float *X = sc + y.X, *H = sc + y.H, *AO = sc + y.AO, *E = sc + y.E, *PA = sc + y.PA, *PB = sc + y.PB;
  const int* flag = a.skip_flag;
  const int when = a.skip_when;
  // Y partials = X . Wt over the B rows; returns the slice count the consumer adds up
  auto gemm = [&](float* part, const float* x, int xparts, const float* xbias, const float* wt, int K, int N) {
    const Split sp = wide_split(K, N, B);
    WideGemm g{x, xbias, xparts, wt, part, B, K, N, sp.kper, flag, when};
    hipLaunchKernelGGL(gptw_gemm_kernel, dim3(sp.KS, (B + 63) / 64, N / 64), dim3(WT), 0, s, g);
    return sp.KS;
  };
  auto ln_args = [&](const float* part, int nparts, const float* pbias, int layer, int site, const float* w, const float* b, int j) {
    return WideLn{X, part, nparts, pbias, layer, site, w, b, a.cache_len, j, B, C, a.pdrop, a.drop_seed};
  };
  const int n_new = (a.src_mode == GPT_SRC_ENV && a.step == 0) ? 2 : 1;
  const size_t attn_lds = (size_t)(3 * (C / a.n_head) + a.Tmax) * sizeof(float);
  int pb_parts = 0;
  for (int j = 0; j < n_new; ++j) {
    const int last = j == n_new - 1;
    const bool to_gemm = gpt_tok_kind(a, j).to_gemm;
    hipLaunchKernelGGL(gptw_embed_kernel, dim3(B), dim3(WT), 0, s, a, j, last, X, E);
    if (to_gemm) {
      const int ks = gemm(PB, E, 0, nullptr, a.proj_wt, a.n_parts * C, C);
      hipLaunchKernelGGL(gptw_embed_finish_kernel, dim3(B), dim3(WT), 0, s, a, j, last, (const float*)PB, ks, X);
    }
    if (a.embed_only) continue;
    for (int l = 0; l < nL; ++l) {
      const GptLayerPtrs& L = a.layers_host[l];
      const WideLn l1 = l > 0 ? ln_args(PB, pb_parts, a.layers_host[l - 1].fc2_b, l - 1, 3, L.ln1_w, L.ln1_b, j)
                              : ln_args(nullptr, 0, nullptr, 0, 0, L.ln1_w, L.ln1_b, j);
      hipLaunchKernelGGL(gptw_ln_kernel, dim3(B), dim3(WT), 0, s, l1, H, flag, when);
      const int kq = gemm(PA, H, 0, nullptr, L.qkv_wt, C, 3 * C);
      WideAttn at{PA, kq, L.qkv_b, a.kcache + (size_t)l * B * a.Tmax * C, a.vcache + (size_t)l * B * a.Tmax * C, AO,
                  a.cache_len, j, B, C, a.n_head, a.Tmax, l, a.pdrop, a.drop_seed, flag, when};
      hipLaunchKernelGGL(gptw_attn_kernel, dim3(a.n_head, B), dim3(64), attn_lds, s, at);
      if (!last && l == nL - 1) break;       // the class token in front of the first patch: only its K / V rows are used
      const int kp = gemm(PB, AO, 0, nullptr, L.proj_wt, C, C);
      const WideLn l2 = ln_args(PB, kp, L.proj_b, l, 2, L.ln2_w, L.ln2_b, j);
      hipLaunchKernelGGL(gptw_ln_kernel, dim3(B), dim3(WT), 0, s, l2, H, flag, when);
      const int kf = gemm(PA, H, 0, nullptr, L.fc_wt, C, 4 * C);
      pb_parts = gemm(PB, PA, kf, L.fc_b, L.fc2_wt, 4 * C, C);
    }
  }
  if (!a.embed_only) {
    const WideLn lf = nL > 0 ? ln_args(PB, pb_parts, a.layers_host[nL - 1].fc2_b, nL - 1, 3, a.lnf_w, a.lnf_b, n_new - 1)
                             : ln_args(nullptr, 0, nullptr, 0, 0, a.lnf_w, a.lnf_b, n_new - 1);
    hipLaunchKernelGGL(gptw_tail_kernel, dim3(B), dim3(WT), 0, s, a, lf);
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_gpt_step_routed(const GptStepArgs& a, hipStream_t s) { return a.wide ? launch_gpt_step_wide(a, s) : launch_gpt_step(a, s); }

}  // namespace jnr
