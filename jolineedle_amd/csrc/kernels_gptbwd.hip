// Backward of the decision transformer over a whole trajectory, batched over the agents (loss.backward() through
// GPT.forward of src/models/gpt.py:308-369 with the blocks of :78-127; same mathematics as gpt_backward_kernel in
// kernels_train.hip, which gives one workgroup to each agent and therefore occupies B compute units).
//
// Here every phase is one launch over ALL tokens of ALL agents: rows m = agent * Lm + token (Lm = T + 1), the forward is
// recomputed into a row-major scratch, and each Linear is one small fp32 GEMM (tiles through LDS, FMA; the token-row
// products by gptb_tok_gemm_kernel, or gptb_gemm_kernel for K > 192, the weight gradients by gptb_wgrad_kernel):
//   forward     out[M x N]  = in[M x K] . Wt[K x N]                     (Wt: the arena's transposed Linear weight)
//   data grad   din[M x K]  = dout[M x N] . Wt^T
//   weight grad gWt[K x N] += in^T[K x M] . dout[M x N]
// The number of executed glimpse steps S is only known on the device (n_done); the first kernel publishes L = S + 1 and
// every later kernel treats token rows >= L as absent (zero operands, zero results), so launches do not depend on it.
// The workload is a few GFLOP of GEMMs with M of a few hundred rows — launch- and latency-bound, not a roofline item;
// FMA tiles keep fp32 exactness and are far from being the limit.
// The attention of a head comes in two forms: q, k, v, dY and two Lm x Lm score tiles in LDS (gptb_attn_fwd_kernel,
// gptb_attn_bwd_kernel: 4 Lm hs + 2 Lm^2 <= 16384 floats), or tiled over 16 query / key rows with LDS that does not grow
// with Lm (the gptb_attn_*_tiled / _rows / _keys kernels: Lm <= 256, head size <= 256).  gpt_backward_route picks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "jn_gpt_device.h"
#include "jn_kernels.h"
#include "jn_types.h"

namespace jnr {
namespace {

constexpr int GT = 256;

struct GemmArgs {
  const float* A; long long a_rs, a_cs;      // A(m, k) = A[m * a_rs + k * a_cs]
  const float* B; long long b_rs, b_cs;      // B(k, n)
  float* C; long long c_rs;                  // C(m, n) = C[m * c_rs + n]
  int M, N, K;
  const float* bias;                         // + bias[n]
  const float* resid;                        // + resid[m][n] (leading dimension c_rs), after the dropout of the product
  const float* mulp;                         // * gelu'(mulp[m][n])
  int a_gelu;                                // A elements pass through gelu on load
  int accumulate;                            // C += result
  int tok_dim;                               // 0: m runs over token rows (gptb_tok_gemm_kernel / gptb_gemm_kernel), 1: k does (gptb_wgrad_kernel)
  const int* L; int Lm;                      // a token row r is live iff r % Lm < *L
  float pdrop; uint64_t seed; int site, layer;   // site >= 0: dropout (jn_device.h drop_scale) of product + bias
};

// The token-row GEMM for the shapes gptb_tok_gemm_kernel does not take (K > TG_KMAX: wide models): 64 x 64 tiles, K in steps of 16.
template <bool A_KFAST, bool B_NFAST>
__global__ __launch_bounds__(GT) void gptb_gemm_kernel(GemmArgs g) {
  constexpr int BM = 64, BN = 64, BK = 16;
  __shared__ float As[BK][BM + 1], Bs[BK][BN + 1];
  const int tid = threadIdx.x, m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int L = *g.L;
  const int ty = tid >> 4, tx = tid & 15;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
  const int kend = g.K;
  for (int k0 = 0; k0 < kend; k0 += BK) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = tid + q * GT;
      int m, k;
      if (A_KFAST) { k = idx & 15; m = idx >> 4; } else { m = idx & 63; k = idx >> 6; }
      const int gm = m0 + m, gk = k0 + k;
      float v = 0.0f;
      if (gm < g.M && gk < kend) {
        if ((gm % g.Lm) < L) {
          v = g.A[(long long)gm * g.a_rs + (long long)gk * g.a_cs];
          if (g.a_gelu) v = gelu_tanh(v);
        }
      }
      As[k][m] = v;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = tid + q * GT;
      int n, k;
      if (B_NFAST) { n = idx & 63; k = idx >> 6; } else { k = idx & 15; n = idx >> 4; }
      const int gn = n0 + n, gk = k0 + k;
      float v = 0.0f;
      if (gn < g.N && gk < kend) v = g.B[(long long)gk * g.b_rs + (long long)gn * g.b_cs];
      Bs[k][n] = v;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < BK; ++kk) {
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = As[kk][ty * 4 + i]; b[i] = Bs[kk][tx * 4 + i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gm = m0 + ty * 4 + i;
    if (gm >= g.M) continue;
    const bool live = (gm % g.Lm) < L;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gn = n0 + tx * 4 + j;
      if (gn >= g.N) continue;
      const long long o = (long long)gm * g.c_rs + gn;
      float v = acc[i][j];
      if (live) {
        if (g.bias) v += g.bias[gn];
        if (g.site >= 0 && g.pdrop > 0.0f) v *= drop_scale(g.seed, gm / g.Lm, gm % g.Lm, g.layer, g.site, gn, g.pdrop);
        if (g.resid) v += g.resid[o];
        if (g.mulp) v *= gelu_tanh_grad(g.mulp[o]);
      } else {
        v = 0.0f;
      }
      g.C[o] = g.accumulate ? g.C[o] + v : v;
    }
  }
}

// Token-row GEMMs (tok_dim 0: m runs over token rows, A's rows contiguous) with K <= TG_KMAX, 28 of the 40 GEMMs of a
// backward.  gptb_gemm_kernel walks K in steps of 16 with an exposed global round trip and two barriers per step, on 21 -
// 63 workgroups.  Here a workgroup takes 32 rows x 64 columns (42 x ceil(N / 64) workgroups at the headline's 1344 rows),
// stages the WHOLE K of both operands in one round with every load in flight — 16-byte loads where the operand's fast
// axis and alignment allow (vec_a / vec_b, decided by the launcher), guarded 4-byte loads otherwise (the head: N or K =
// n_actions) — and passes ONE barrier.  A row's liveness is computed once by each of the eight threads that load it.
// Each output element is one ascending-k fmaf chain from zero, followed by gptb_gemm_kernel's epilogue in its order
// (bias, dropout, residual, gelu'), so the results equal that kernel's bit for bit.  fp32 VALU on purpose.
constexpr int TG_BM = 32, TG_BN = 64, TG_KMAX = 192;
inline int tg_lda(int K) { return ((K + 3) & ~3) + 4; }      // keeps rows 16-byte aligned, spreads the row groups over the banks
inline size_t tg_lds_bytes(int K) { return ((size_t)TG_BM * tg_lda(K) + (size_t)((K + 3) & ~3) * TG_BN) * sizeof(float); }

template <bool B_NFAST>
__global__ __launch_bounds__(GT) void gptb_tok_gemm_kernel(GemmArgs g, int vec_a, int vec_b) {
  using f4 = __attribute__((ext_vector_type(4))) float;
  extern __shared__ __attribute__((aligned(16))) float tg_sm[];
  const int K = g.K, K4 = (K + 3) & ~3, lda = K4 + 4;
  float* As = tg_sm;                       // [TG_BM][lda]   A(m, k)
  float* Bs = As + TG_BM * lda;            // [K4][TG_BN]    B(k, n)
  const int tid = threadIdx.x, m0 = blockIdx.y * TG_BM, n0 = blockIdx.x * TG_BN;
  const int L = *g.L;
  // ---- A: thread = (row, one of eight lanes of the row); a dead or absent row is zeros
  {
    const int m = tid >> 3, r = tid & 7, gm = m0 + m;
    const bool live = gm < g.M && (gm % g.Lm) < L;
    const float* ap = g.A + (long long)gm * g.a_rs;
    float* as = As + m * lda;
    if (vec_a) {
      // every load of the thread first (a dead row reads row 0 and is zeroed by a select: no branch around a load)
      constexpr int NA = TG_KMAX / 4 / 8;
      const float* src = live ? ap : g.A;
      const int KQ = K4 >> 2;
      f4 v[NA];
#pragma unroll
      for (int j = 0; j < NA; ++j) v[j] = *reinterpret_cast<const f4*>(src + 4 * min(r + 8 * j, KQ - 1));
#pragma unroll
      for (int j = 0; j < NA; ++j) {
        const int kq = r + 8 * j;
        f4 w = v[j];
        if (g.a_gelu) { w.x = gelu_tanh(w.x); w.y = gelu_tanh(w.y); w.z = gelu_tanh(w.z); w.w = gelu_tanh(w.w); }
        if (!live) w = f4{0.f, 0.f, 0.f, 0.f};
        if (kq < KQ) *reinterpret_cast<f4*>(as + 4 * kq) = w;
      }
    } else {
      for (int k = r; k < K4; k += 8) {
        float v = 0.0f;
        if (live && k < K) { v = ap[k]; if (g.a_gelu) v = gelu_tanh(v); }
        as[k] = v;
      }
    }
  }
  // ---- B: columns past N and rows past K are zeros
  if (B_NFAST) {                           // B(k, n) = B[k * b_rs + n]
    if (vec_b) {                           // K % 4 == 0 is not needed here, N % 4 == 0 is
      constexpr int NB = TG_KMAX * (TG_BN / 4) / GT;
      f4 v[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int e = tid + j * GT, k = min(e >> 4, K - 1), gn = n0 + 4 * (e & 15);
        v[j] = *reinterpret_cast<const f4*>(g.B + (long long)k * g.b_rs + (gn < g.N ? gn : 0));
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int e = tid + j * GT, k = e >> 4, nq = e & 15;
        const bool in = k < K && n0 + 4 * nq < g.N;
        if (k < K4) *reinterpret_cast<f4*>(Bs + k * TG_BN + 4 * nq) = in ? v[j] : f4{0.f, 0.f, 0.f, 0.f};
      }
    } else {
      for (int e = tid; e < K4 * TG_BN; e += GT) {
        const int k = e >> 6, n = e & 63, gn = n0 + n;
        Bs[e] = (k < K && gn < g.N) ? g.B[(long long)k * g.b_rs + gn] : 0.0f;
      }
    }
  } else {                                 // B(k, n) = B[n * b_cs + k]: lanes run over n, so the LDS writes do not collide
    if (vec_b) {                           // K % 4 == 0
      constexpr int NB = (TG_KMAX / 4) * TG_BN / GT;
      const int KQ = K >> 2;
      f4 v[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int e = tid + j * GT, kq = min(e >> 6, KQ - 1), gn = n0 + (e & 63);
        v[j] = *reinterpret_cast<const f4*>(g.B + (long long)(gn < g.N ? gn : 0) * g.b_cs + 4 * kq);
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int e = tid + j * GT, kq = e >> 6, n = e & 63;
        const f4 w = n0 + n < g.N ? v[j] : f4{0.f, 0.f, 0.f, 0.f};
        if (kq < KQ) {
          float* bs = Bs + (4 * kq) * TG_BN + n;
          bs[0] = w.x; bs[TG_BN] = w.y; bs[2 * TG_BN] = w.z; bs[3 * TG_BN] = w.w;
        }
      }
    } else {
      for (int e = tid; e < K4 * TG_BN; e += GT) {
        const int k = e >> 6, n = e & 63, gn = n0 + n;
        Bs[e] = (k < K && gn < g.N) ? g.B[(long long)gn * g.b_cs + k] : 0.0f;
      }
    }
  }
  __syncthreads();
  // ---- 2 rows x 4 columns per thread, one ascending-k chain per element (the zero padding past K is never added)
  const int ty = tid >> 4, tx = tid & 15;
  const float* a0 = As + (2 * ty) * lda;
  const float* a1 = a0 + lda;
  const float* bp = Bs + 4 * tx;
  float acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
  int k = 0;
  for (; k + 4 <= K; k += 4) {
    const f4 x0 = *reinterpret_cast<const f4*>(a0 + k), x1 = *reinterpret_cast<const f4*>(a1 + k);
    const float xa[2][4] = {{x0.x, x0.y, x0.z, x0.w}, {x1.x, x1.y, x1.z, x1.w}};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const f4 b = *reinterpret_cast<const f4*>(bp + (k + kk) * TG_BN);
      const float bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(xa[i][kk], bb[j], acc[i][j]);
    }
  }
  for (; k < K; ++k) {
    const f4 b = *reinterpret_cast<const f4*>(bp + k * TG_BN);
    const float bb[4] = {b.x, b.y, b.z, b.w};
    const float xa[2] = {a0[k], a1[k]};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(xa[i], bb[j], acc[i][j]);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int gm = m0 + 2 * ty + i;
    if (gm >= g.M) continue;
    const bool live = (gm % g.Lm) < L;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gn = n0 + tx * 4 + j;
      if (gn >= g.N) continue;
      const long long o = (long long)gm * g.c_rs + gn;
      float v = acc[i][j];
      if (live) {
        if (g.bias) v += g.bias[gn];
        if (g.site >= 0 && g.pdrop > 0.0f) v *= drop_scale(g.seed, gm / g.Lm, gm % g.Lm, g.layer, g.site, gn, g.pdrop);
        if (g.resid) v += g.resid[o];
        if (g.mulp) v *= gelu_tanh_grad(g.mulp[o]);
      } else {
        v = 0.0f;
      }
      g.C[o] = g.accumulate ? g.C[o] + v : v;
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Launches the token-row kernel when it takes the shape; false: the caller's kernel does.
bool tok_gemm(const GemmArgs& g, hipStream_t s) {
  const bool bn = g.b_cs == 1, bk = g.b_rs == 1;
  if (g.tok_dim != 0 || g.a_cs != 1 || g.K > TG_KMAX || g.K < 1 || !(bn || bk)) return false;
  const size_t lds = tg_lds_bytes(g.K);
  static bool raised = false;
  if (!raised) {
    const int most = (int)tg_lds_bytes(TG_KMAX);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gptb_tok_gemm_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, most) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&gptb_tok_gemm_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, most) != hipSuccess)
      return false;
    raised = true;
  }
  const int vec_a = (g.K & 3) == 0 && (g.a_rs & 3) == 0 && aligned16(g.A);
  const int vec_b = bn ? ((g.N & 3) == 0 && (g.b_rs & 3) == 0 && aligned16(g.B)) : ((g.K & 3) == 0 && (g.b_cs & 3) == 0 && aligned16(g.B));
  const dim3 grid((g.N + TG_BN - 1) / TG_BN, (g.M + TG_BM - 1) / TG_BM);
  if (bn) hipLaunchKernelGGL((gptb_tok_gemm_kernel<true>), grid, dim3(GT), lds, s, g, vec_a, vec_b);
  else hipLaunchKernelGGL((gptb_tok_gemm_kernel<false>), grid, dim3(GT), lds, s, g, vec_a, vec_b);
  return true;
}

// Weight gradients: gWt[Kf x N] += in^T . dout over the token rows, and the bias gradient gb[N] += column sums of dout.
// A workgroup takes 64 features x 64 columns and a slice of WG_ROWS token rows: both operand tiles (in[rows][64 features],
// dout[rows][64 columns], both contiguous along the tile's fast axis) are staged whole with every load in flight, one
// barrier, one ascending chain over the slice's rows per element, then fp32 atomics into gWt (the slices of a tile meet
// there, in no fixed order — as the 128-row slices of gptb_gemm_kernel did; these sums are held to the oracle, not to
// bits).  The workgroups of the first feature tile also add their dout tile's column sums — it is in LDS, dead rows are
// zeros in it — into gb: the separate column-sum launches that re-read dout are gone.
constexpr int WG_ROWS = 64;
__global__ __launch_bounds__(GT) void gptb_wgrad_kernel(GemmArgs g, float* __restrict__ gb, int vec_a, int vec_b) {
  using f4 = __attribute__((ext_vector_type(4))) float;
  __shared__ __attribute__((aligned(16))) float As[WG_ROWS][64], Bs[WG_ROWS][64];
  const int tid = threadIdx.x, f0 = blockIdx.y * 64, n0 = blockIdx.x * 64, r0 = blockIdx.z * WG_ROWS;
  const int L = *g.L, Kf = g.M, N = g.N, R = g.K;           // features, columns, token rows
  if (vec_a && vec_b) {
    f4 va[4], vb[4];
    bool la[4], lb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {                            // (row, quad): all eight loads first, dead / absent parts zeroed by selects
      const int e = tid + j * GT, r = e >> 4, q4 = 4 * (e & 15), gr = r0 + r;
      const bool live = gr < R && (gr % g.Lm) < L;
      la[j] = live && f0 + q4 < Kf; lb[j] = live && n0 + q4 < N;
      const long long row = live ? gr : 0;
      va[j] = *reinterpret_cast<const f4*>(g.A + row * g.a_cs + (la[j] ? f0 + q4 : 0));
      vb[j] = *reinterpret_cast<const f4*>(g.B + row * g.b_rs + (lb[j] ? n0 + q4 : 0));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = tid + j * GT, r = e >> 4, q4 = 4 * (e & 15);
      f4 a = va[j];
      if (g.a_gelu) { a.x = gelu_tanh(a.x); a.y = gelu_tanh(a.y); a.z = gelu_tanh(a.z); a.w = gelu_tanh(a.w); }
      *reinterpret_cast<f4*>(&As[r][q4]) = la[j] ? a : f4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f4*>(&Bs[r][q4]) = lb[j] ? vb[j] : f4{0.f, 0.f, 0.f, 0.f};
    }
  } else {
    for (int e = tid; e < WG_ROWS * 64; e += GT) {
      const int r = e >> 6, c = e & 63, gr = r0 + r;
      const bool live = gr < R && (gr % g.Lm) < L;
      float a = 0.0f, b = 0.0f;
      if (live && f0 + c < Kf) { a = g.A[(long long)gr * g.a_cs + f0 + c]; if (g.a_gelu) a = gelu_tanh(a); }
      if (live && n0 + c < N) b = g.B[(long long)gr * g.b_rs + n0 + c];
      As[r][c] = a; Bs[r][c] = b;
    }
  }
  __syncthreads();
  const int ty = tid >> 4, tx = tid & 15;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
#pragma unroll 8
  for (int r = 0; r < WG_ROWS; ++r) {
    const f4 a = *reinterpret_cast<const f4*>(&As[r][4 * ty]), b = *reinterpret_cast<const f4*>(&Bs[r][4 * tx]);
    const float aa[4] = {a.x, a.y, a.z, a.w}, bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(aa[i], bb[j], acc[i][j]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gf = f0 + 4 * ty + i;
    if (gf >= Kf) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gn = n0 + 4 * tx + j;
      if (gn < N && acc[i][j] != 0.0f) atomicAdd(&g.C[(long long)gf * g.c_rs + gn], acc[i][j]);
    }
  }
  if (gb && blockIdx.y == 0 && tid < 64 && n0 + tid < N) {
    float sum = 0.0f;
    for (int r = 0; r < WG_ROWS; ++r) sum += Bs[r][tid];
    if (sum != 0.0f) atomicAdd(&gb[n0 + tid], sum);
  }
}

// in: [rows][Kf] (a_cs = Kf), dout: [rows][N]; takes every shape
void wgrad(const GemmArgs& g, float* gb, hipStream_t s) {
  const int vec_a = (g.M & 3) == 0 && (g.a_cs & 3) == 0 && aligned16(g.A);
  const int vec_b = (g.N & 3) == 0 && (g.b_rs & 3) == 0 && aligned16(g.B);
  const dim3 grid((g.N + 63) / 64, (g.M + 63) / 64, (g.K + WG_ROWS - 1) / WG_ROWS);
  hipLaunchKernelGGL(gptb_wgrad_kernel, grid, dim3(GT), 0, s, g, gb, vec_a, vec_b);
}

void gemm(GemmArgs g, hipStream_t s) {
  if (tok_gemm(g, s)) return;
  dim3 grid((g.N + 63) / 64, (g.M + 63) / 64);      // shapes the token-row kernel does not take (K > TG_KMAX: wide models)
  const bool ak = g.a_cs == 1, bn = g.b_cs == 1;
  if (ak && bn) hipLaunchKernelGGL((gptb_gemm_kernel<true, true>), grid, dim3(GT), 0, s, g);
  else if (ak) hipLaunchKernelGGL((gptb_gemm_kernel<true, false>), grid, dim3(GT), 0, s, g);
  else if (bn) hipLaunchKernelGGL((gptb_gemm_kernel<false, true>), grid, dim3(GT), 0, s, g);
  else hipLaunchKernelGGL((gptb_gemm_kernel<false, false>), grid, dim3(GT), 0, s, g);
}

// L = S + 1 (S = first step at which every agent is done, gpt_backward_kernel's rule) and the embedded trajectory
// X0 = drop(final_emb) for the live token rows.
__global__ __launch_bounds__(GT) void gptb_init_kernel(GptBwdArgs a, int* Lp, float* X0, int Lm) {
  __shared__ int s_L;
  if (threadIdx.x == 0) {
    int S = a.T;
    if (a.stop_early)
      for (int t = 1; t <= a.T; ++t)
        if (a.n_done[t] >= a.B) { S = t; break; }
    s_L = S + 1;
    if (blockIdx.x == 0) *Lp = S + 1;
  }
  __syncthreads();
  const int L = s_L, C = a.C;
  const long long n = (long long)a.B * Lm * C;
  for (long long e = (long long)blockIdx.x * GT + threadIdx.x; e < n; e += (long long)gridDim.x * GT) {
    const int c = (int)(e % C);
    const long long m = e / C;
    const int b = (int)(m / Lm), i = (int)(m % Lm);
    float v = 0.0f;
    if (i < L) {
      v = a.final_emb[((long long)b * (a.T + 1) + i) * C + c];
      if (a.pdrop > 0.0f) v *= drop_scale(a.drop_seed, b, i, 0, 0, c, a.pdrop);
    }
    X0[e] = v;
  }
}

// LayerNorm (eps 1e-5) of every live row, one wave per row; mean and 1 / std are kept for the backward.
__global__ __launch_bounds__(GT) void gptb_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ b, float* __restrict__ out,
                                                         float* __restrict__ mu, float* __restrict__ rs, int M, int C,
                                                         const int* __restrict__ Lp, int Lm) {
  const int row = blockIdx.x * (GT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* xr = x + (long long)row * C;
  float* orow = out + (long long)row * C;
  if ((row % Lm) >= *Lp) {
    for (int c = lane; c < C; c += 64) orow[c] = 0.0f;
    if (lane == 0) { mu[row] = 0.0f; rs[row] = 0.0f; }
    return;
  }
  float sm = 0.0f;
  for (int c = lane; c < C; c += 64) sm += xr[c];
  const float m = wave_sum(sm) / C;
  float q = 0.0f;
  for (int c = lane; c < C; c += 64) { const float d = xr[c] - m; q += d * d; }
  const float r = 1.0f / sqrtf(wave_sum(q) / C + 1e-5f);
  for (int c = lane; c < C; c += 64) orow[c] = (xr[c] - m) * r * w[c] + b[c];
  if (lane == 0) { mu[row] = m; rs[row] = r; }
}

// din = base + LN^T(dout) per live row (base may be null or din itself); gw += sum dout * xhat, gb += sum dout.
// One wave per row, LN_RPB rows per workgroup; the parameter sums stay in registers over the rows of a wave.
constexpr int LN_RPB = 16, LN_CQ = 16;      // C <= 64 * LN_CQ
__global__ __launch_bounds__(GT) void gptb_ln_bwd_kernel(float* __restrict__ din, const float* __restrict__ base,
                                                         const float* __restrict__ dout, const float* __restrict__ x,
                                                         const float* __restrict__ w, float* __restrict__ gw,
                                                         float* __restrict__ gb, const float* __restrict__ mu,
                                                         const float* __restrict__ rs, int M, int C,
                                                         const int* __restrict__ Lp, int Lm) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, L = *Lp;
  float aw[LN_CQ], ab[LN_CQ];
#pragma unroll
  for (int q = 0; q < LN_CQ; ++q) { aw[q] = 0.0f; ab[q] = 0.0f; }
  for (int rr = wave; rr < LN_RPB; rr += GT / 64) {
    const int row = blockIdx.x * LN_RPB + rr;
    if (row >= M) break;
    float* dr = din + (long long)row * C;
    if ((row % Lm) >= L) {
      for (int c = lane; c < C; c += 64) dr[c] = 0.0f;
      continue;
    }
    const float* xr = x + (long long)row * C;
    const float* d = dout + (long long)row * C;
    const float m = mu[row], r = rs[row];
    float m1 = 0.0f, m2 = 0.0f;
#pragma unroll
    for (int q = 0; q < LN_CQ; ++q) {
      const int c = lane + 64 * q;
      if (c < C) {
        const float dv = d[c], xh = (xr[c] - m) * r, dx = dv * w[c];
        m1 += dx; m2 += dx * xh;
        aw[q] += dv * xh; ab[q] += dv;
      }
    }
    m1 = wave_sum(m1) / C; m2 = wave_sum(m2) / C;
    for (int c = lane; c < C; c += 64) {
      const float xh = (xr[c] - m) * r;
      const float v = r * (d[c] * w[c] - m1 - xh * m2);
      dr[c] = base ? base[(long long)row * C + c] + v : v;
    }
  }
#pragma unroll
  for (int q = 0; q < LN_CQ; ++q) {
    const int c = lane + 64 * q;
    if (c < C && (aw[q] != 0.0f || ab[q] != 0.0f)) { atomicAdd(&gw[c], aw[q]); atomicAdd(&gb[c], ab[q]); }
  }
}

// dst = src * dropout mask of (layer, site) on the live rows, 0 on the others
__global__ __launch_bounds__(GT) void gptb_drop_kernel(float* __restrict__ dst, const float* __restrict__ src, long long n,
                                                       int C, int layer, int site, float pdrop, uint64_t seed,
                                                       const int* __restrict__ Lp, int Lm) {
  const long long e = (long long)blockIdx.x * GT + threadIdx.x;
  if (e >= n) return;
  const long long m = e / C;
  const int c = (int)(e - m * C), b = (int)(m / Lm), i = (int)(m % Lm);
  dst[e] = i < *Lp ? src[e] * drop_scale(seed, b, i, layer, site, c, pdrop) : 0.0f;
}

// Causal attention of one (agent, head): probabilities P (kept for the backward) and Y = drop(P) . V.
__global__ __launch_bounds__(GT) void gptb_attn_fwd_kernel(const float* __restrict__ QKV, float* __restrict__ ATT,
                                                           float* __restrict__ Y, int C, int nh, int Lm,
                                                           const int* __restrict__ Lp, float pdrop, uint64_t seed, int layer,
                                                           int Tmax) {
  extern __shared__ float sm[];
  const int b = blockIdx.x / nh, h = blockIdx.x % nh, hs = C / nh, tid = threadIdx.x, L = *Lp;
  float* q = sm; float* k = q + Lm * hs; float* v = k + Lm * hs; float* p = v + Lm * hs;     // p: [Lm][Lm]
  for (int e = tid; e < L * hs; e += GT) {
    const int i = e / hs, d = e - i * hs;
    const float* src = QKV + ((long long)b * Lm + i) * 3 * C + h * hs + d;
    q[e] = src[0]; k[e] = src[C]; v[e] = src[2 * C];
  }
  __syncthreads();
  const float scale = 1.0f / sqrtf((float)hs);
  for (int e = tid; e < L * L; e += GT) {
    const int i = e / L, j = e - i * L;
    float d = -INFINITY;
    if (j <= i) {
      d = 0.0f;
      for (int t = 0; t < hs; ++t) d = fmaf(q[i * hs + t], k[j * hs + t], d);
      d *= scale;
    }
    p[i * Lm + j] = d;
  }
  __syncthreads();
  for (int i = tid; i < L; i += GT) {
    float* row = p + i * Lm;
    float m = -INFINITY;
    for (int j = 0; j <= i; ++j) m = fmaxf(m, row[j]);
    float s = 0.0f;
    for (int j = 0; j <= i; ++j) { row[j] = expf(row[j] - m); s += row[j]; }
    for (int j = 0; j < L; ++j) row[j] = j <= i ? row[j] / s : 0.0f;
  }
  __syncthreads();
  float* att = ATT + (long long)blockIdx.x * Lm * Lm;
  for (int e = tid; e < L * L; e += GT) { const int i = e / L, j = e - i * L; att[i * Lm + j] = p[i * Lm + j]; }
  for (int e = tid; e < L * hs; e += GT) {
    const int i = e / hs, d = e - i * hs;
    float acc = 0.0f;
    for (int j = 0; j <= i; ++j) {
      float pij = p[i * Lm + j];
      if (pdrop > 0.0f) pij *= drop_scale(seed, b, i, layer, 1, h * Tmax + j, pdrop);
      acc = fmaf(pij, v[j * hs + d], acc);
    }
    Y[((long long)b * Lm + i) * C + h * hs + d] = acc;
  }
}

// Backward of the same: dQKV rows of the live tokens from dY, the kept probabilities and q, k, v.
__global__ __launch_bounds__(GT) void gptb_attn_bwd_kernel(const float* __restrict__ QKV, const float* __restrict__ ATT,
                                                           const float* __restrict__ dY, float* __restrict__ dQKV, int C,
                                                           int nh, int Lm, const int* __restrict__ Lp, float pdrop,
                                                           uint64_t seed, int layer, int Tmax) {
  extern __shared__ float sm[];
  const int b = blockIdx.x / nh, h = blockIdx.x % nh, hs = C / nh, tid = threadIdx.x, L = *Lp;
  float* q = sm; float* k = q + Lm * hs; float* v = k + Lm * hs; float* dy = v + Lm * hs;
  float* p = dy + Lm * hs; float* dp = p + Lm * Lm;
  for (int e = tid; e < L * hs; e += GT) {
    const int i = e / hs, d = e - i * hs;
    const float* src = QKV + ((long long)b * Lm + i) * 3 * C + h * hs + d;
    q[e] = src[0]; k[e] = src[C]; v[e] = src[2 * C];
    dy[e] = dY[((long long)b * Lm + i) * C + h * hs + d];
  }
  const float* att = ATT + (long long)blockIdx.x * Lm * Lm;
  for (int e = tid; e < L * L; e += GT) { const int i = e / L, j = e - i * L; p[i * Lm + j] = att[i * Lm + j]; }
  __syncthreads();
  const float scale = 1.0f / sqrtf((float)hs);
  // dP[i][j] = mask(i, j) * sum_d dY[i][d] v[j][d]
  for (int e = tid; e < L * L; e += GT) {
    const int i = e / L, j = e - i * L;
    float acc = 0.0f;
    if (j <= i) {
      for (int t = 0; t < hs; ++t) acc = fmaf(dy[i * hs + t], v[j * hs + t], acc);
      if (pdrop > 0.0f) acc *= drop_scale(seed, b, i, layer, 1, h * Tmax + j, pdrop);
    }
    dp[i * Lm + j] = acc;
  }
  // dV[j][d] = sum_{i >= j} mask(i, j) P[i][j] dY[i][d]
  for (int e = tid; e < L * hs; e += GT) {
    const int j = e / hs, d = e - j * hs;
    float acc = 0.0f;
    for (int i = j; i < L; ++i) {
      float pij = p[i * Lm + j];
      if (pdrop > 0.0f) pij *= drop_scale(seed, b, i, layer, 1, h * Tmax + j, pdrop);
      acc = fmaf(pij, dy[i * hs + d], acc);
    }
    dQKV[((long long)b * Lm + j) * 3 * C + 2 * C + h * hs + d] = acc;
  }
  __syncthreads();
  // softmax backward in place: dS = P * (dP - sum_j P dP) * scale
  for (int i = tid; i < L; i += GT) {
    float* dr = dp + i * Lm;
    const float* pr = p + i * Lm;
    float dot = 0.0f;
    for (int j = 0; j <= i; ++j) dot = fmaf(pr[j], dr[j], dot);
    for (int j = 0; j < L; ++j) dr[j] = j <= i ? pr[j] * (dr[j] - dot) * scale : 0.0f;
  }
  __syncthreads();
  for (int e = tid; e < L * hs; e += GT) {
    const int i = e / hs, d = e - i * hs;
    float dq = 0.0f, dk = 0.0f;
    for (int j = 0; j <= i; ++j) dq = fmaf(dp[i * Lm + j], k[j * hs + d], dq);
    for (int ii = i; ii < L; ++ii) dk = fmaf(dp[ii * Lm + i], q[ii * hs + d], dk);
    float* dst = dQKV + ((long long)b * Lm + i) * 3 * C + h * hs + d;
    dst[0] = dq; dst[C] = dk;
  }
}

// ---- the tiled form of the two kernels above: LDS that does not grow with Lm (any Lm <= 256, head size <= 256) -------------
// A workgroup owns TR query rows of one (agent, head) for the recompute, dP, the softmax backward and dQ, or TR key rows for
// dK and dV.  The probabilities stay in ATT; dS goes through DS, a global buffer of ATT's shape (row i written for j <= i
// only).  In LDS: the TR q (or dY) rows, a 64-key x 32-column staging tile of K (or V), and the TR x jmax score tile held
// key-major, so that the products over keys read it as a broadcast.  Every output element has one writer and a fixed
// summation order: equal inputs give equal bytes, as in the LDS form.
// Precision: the score products (q . k, dY . v: sums of head-size terms) accumulate in fp64 and a row's softmax and softmax
// backward run in fp64 on that tile, so P and dS carry one fp32 rounding each; the products over keys and rows (Y, dQ, dK,
// dV) are fp32 chains in the LDS form's order.  The fp64 tile Pd is followed by its fp32 image Pf, which takes the place of
// the q rows and the staging tile once the score product is done.
constexpr int TR = 16;            // rows per workgroup: GT / 64 waves x 4 rows in the score product, GT / TR lanes per softmax row
constexpr int TRP = TR + 1;       // leading dimension of the key-major tile (odd: the softmax's column walks spread over banks)
constexpr int TKJ = 64, TKD = 32; // staging tile of the score product: keys x head columns (leading dimension TKD + 1)
constexpr int T_MAX_LM = 256, T_MAX_HS = 256;
static_assert(TR == 4 * (GT / 64) && GT % TR == 0 && GT / TR == 16, "the thread maps below");

// floats in front of the fp64 tile: the q rows + staging tile, later the fp32 tile Pf (an even count: Pd is 8-byte aligned)
__host__ __device__ inline int tiled_front_floats(int Lm, int hs) {
  const int a = TR * hs + TKJ * (TKD + 1), b = Lm * TRP;
  return ((a > b ? a : b) + 1) & ~1;
}
size_t tiled_row_lds(int Lm, int hs) { return (size_t)tiled_front_floats(Lm, hs) * sizeof(float) + (size_t)Lm * TRP * sizeof(double); }
size_t tiled_key_lds(int Lm) { return (size_t)2 * Lm * TRP * sizeof(float); }
static_assert(((size_t)TR * T_MAX_HS + TKJ * (TKD + 1)) * sizeof(float) + (size_t)T_MAX_LM * TRP * sizeof(double) <= 64 * 1024 &&
              TR * T_MAX_HS + TKJ * (TKD + 1) >= T_MAX_LM * TRP &&
              (size_t)2 * T_MAX_LM * TRP * sizeof(float) <= 64 * 1024, "the tiled form stays inside the LDS that needs no grant");

// Pd[j][r] = sum_d Xs[r][d] * Z[j][d] for the keys j < jmax and the TR rows of Xs (LDS, [TR][hs]); Z: global rows ldz apart.
// Wave w owns rows 4 w .. 4 w + 3, a lane one key of the 64 staged: the Xs reads are broadcasts, the tile reads stride
// TKD + 1.  The products are exact in fp64 and summed there, first column to last.  Ends unsynchronised.
__device__ __forceinline__ void tiled_scores(const float* __restrict__ Xs, const float* __restrict__ Z, long long ldz, int hs,
                                             int jmax, float* __restrict__ Zs, double* __restrict__ Pd) {
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  for (int j0 = 0; j0 < jmax; j0 += TKJ) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int d0 = 0; d0 < hs; d0 += TKD) {
      __syncthreads();
      for (int e = tid; e < TKJ * TKD; e += GT) {
        const int jj = e / TKD, dd = e - jj * TKD, j = j0 + jj, d = d0 + dd;
        Zs[jj * (TKD + 1) + dd] = (j < jmax && d < hs) ? Z[(long long)j * ldz + d] : 0.0f;
      }
      __syncthreads();
      const int dn = min(TKD, hs - d0);
      const float* x = Xs + (4 * w) * hs + d0;
      for (int dd = 0; dd < dn; ++dd) {
        const double z = (double)Zs[lane * (TKD + 1) + dd];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = fma((double)x[r * hs + dd], z, acc[r]);
      }
    }
    if (j0 + lane < jmax) {
#pragma unroll
      for (int r = 0; r < 4; ++r) Pd[(j0 + lane) * TRP + 4 * w + r] = acc[r];
    }
  }
}

// How the threads share a [TR][hs] output: G = GT / hs groups of hs threads (thread = one head column d), group g owns the rows
// g, g + G, ... (rpt of them at the most); threads past G * hs idle.
struct TiledCols { int g, d, G, rpt; bool on; };
__device__ __forceinline__ TiledCols tiled_cols(int hs) {
  TiledCols t;
  t.G = min(GT / hs, TR); t.g = threadIdx.x / hs; t.d = threadIdx.x - t.g * hs; t.on = t.g < t.G;
  t.rpt = (TR + t.G - 1) / t.G;
  return t;
}

// acc[r] += sum_{n < N} Wt[n][g + r G] * Z[n][d]: Wt the key-major LDS tile ([N][TRP]), Z global rows ldz apart (the lanes of
// a group read one row side by side).  One chain over n, first to last, as the LDS form sums.
__device__ __forceinline__ void tiled_accumulate(const float* __restrict__ Wt, const float* __restrict__ Z, long long ldz, int N,
                                                 const TiledCols& t, float (&acc)[TR]) {
#pragma unroll 4
  for (int n = 0; n < N; ++n) {
    const float z = Z[(long long)n * ldz + t.d];
    const float* wr = Wt + n * TRP + t.g;
#pragma unroll
    for (int r = 0; r < TR; ++r) {
      if (r >= t.rpt) break;
      acc[r] = fmaf(wr[min(r * t.G, TR - 1 - t.g)], z, acc[r]);       // (rows past TR: clamped read, never stored)
    }
  }
}

// grid (B * nh, ceil(Lm / TR)): probabilities of the query rows [i0, i0 + TR) into ATT, Y = drop(P) . V of those rows
__global__ __launch_bounds__(GT) void gptb_attn_fwd_tiled_kernel(const float* __restrict__ QKV, float* __restrict__ ATT,
                                                                 float* __restrict__ Y, int C, int nh, int Lm,
                                                                 const int* __restrict__ Lp, float pdrop, uint64_t seed,
                                                                 int layer, int Tmax) {
  extern __shared__ float sm[];
  const int b = blockIdx.x / nh, h = blockIdx.x % nh, hs = C / nh, tid = threadIdx.x, L = *Lp, i0 = blockIdx.y * TR;
  if (i0 >= L) return;
  const int i1 = min(i0 + TR, L), jmax = i1;
  float* Xs = sm; float* Zs = Xs + TR * hs; float* Pf = sm;          // Pf: after the score product
  double* Pd = reinterpret_cast<double*>(sm + tiled_front_floats(Lm, hs));
  const float* base = QKV + (long long)b * Lm * 3 * C + h * hs;
  for (int e = tid; e < TR * hs; e += GT) {
    const int r = e / hs, d = e - r * hs;
    Xs[e] = (i0 + r < i1) ? base[(long long)(i0 + r) * 3 * C + d] : 0.0f;
  }
  tiled_scores(Xs, base + C, 3LL * C, hs, jmax, Zs, Pd);
  __syncthreads();
  // softmax of row i0 + r by 16 neighbouring lanes; the undropped row goes to ATT (zeros right of the diagonal up to L)
  {
    const int r = tid / (GT / TR), part = tid % (GT / TR), i = i0 + r;
    const bool live = i < i1;
    const double scale = 1.0 / sqrt((double)hs);
    double m = -INFINITY;
    if (live) for (int j = part; j <= i; j += GT / TR) { const double v = Pd[j * TRP + r] * scale; Pd[j * TRP + r] = v; m = fmax(m, v); }
    for (int o = GT / TR / 2; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    double sum = 0.0;
    if (live) for (int j = part; j <= i; j += GT / TR) { const double v = exp(Pd[j * TRP + r] - m); Pd[j * TRP + r] = v; sum += v; }
    for (int o = GT / TR / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    float* att = ATT + ((long long)blockIdx.x * Lm + i) * Lm;
    for (int j = part; j < (live ? L : jmax); j += GT / TR) {
      float p = 0.0f;
      if (live && j <= i) p = (float)(Pd[j * TRP + r] / sum);
      if (live) att[j] = p;
      if (j < jmax) Pf[j * TRP + r] = (p != 0.0f && pdrop > 0.0f) ? p * drop_scale(seed, b, i, layer, 1, h * Tmax + j, pdrop) : p;
    }
  }
  __syncthreads();
  const TiledCols t = tiled_cols(hs);
  if (!t.on) return;
  float acc[TR];
#pragma unroll
  for (int r = 0; r < TR; ++r) acc[r] = 0.0f;
  tiled_accumulate(Pf, base + 2 * C, 3LL * C, jmax, t, acc);
#pragma unroll
  for (int r = 0; r < TR; ++r) {
    const int i = i0 + t.g + r * t.G;
    if (r < t.rpt && t.g + r * t.G < TR && i < i1) Y[((long long)b * Lm + i) * C + h * hs + t.d] = acc[r];
  }
}

// grid (B * nh, ceil(Lm / TR)): dP, the softmax backward (dS into DS, j <= i) and dQ of the query rows [i0, i0 + TR)
__global__ __launch_bounds__(GT) void gptb_attn_bwd_rows_kernel(const float* __restrict__ QKV, const float* __restrict__ ATT,
                                                                const float* __restrict__ dY, float* __restrict__ DS,
                                                                float* __restrict__ dQKV, int C, int nh, int Lm,
                                                                const int* __restrict__ Lp, float pdrop, uint64_t seed,
                                                                int layer, int Tmax) {
  extern __shared__ float sm[];
  const int b = blockIdx.x / nh, h = blockIdx.x % nh, hs = C / nh, tid = threadIdx.x, L = *Lp, i0 = blockIdx.y * TR;
  if (i0 >= L) return;
  const int i1 = min(i0 + TR, L), jmax = i1;
  float* Xs = sm; float* Zs = Xs + TR * hs; float* Pf = sm;          // Pf: after the score product
  double* Pd = reinterpret_cast<double*>(sm + tiled_front_floats(Lm, hs));
  const float* base = QKV + (long long)b * Lm * 3 * C + h * hs;
  for (int e = tid; e < TR * hs; e += GT) {
    const int r = e / hs, d = e - r * hs;
    Xs[e] = (i0 + r < i1) ? dY[((long long)b * Lm + i0 + r) * C + h * hs + d] : 0.0f;
  }
  tiled_scores(Xs, base + 2 * C, 3LL * C, hs, jmax, Zs, Pd);       // dY . V^T
  __syncthreads();
  {
    const int r = tid / (GT / TR), part = tid % (GT / TR), i = i0 + r;
    const bool live = i < i1;
    const double scale = 1.0 / sqrt((double)hs);
    const long long row = ((long long)blockIdx.x * Lm + i) * Lm;
    double dot = 0.0;
    if (live)
      for (int j = part; j <= i; j += GT / TR) {
        double dp = Pd[j * TRP + r];
        if (pdrop > 0.0f) dp *= (double)drop_scale(seed, b, i, layer, 1, h * Tmax + j, pdrop);
        Pd[j * TRP + r] = dp;
        dot = fma((double)ATT[row + j], dp, dot);
      }
    for (int o = GT / TR / 2; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    for (int j = part; j < jmax; j += GT / TR) {
      float ds = 0.0f;
      if (live && j <= i) { ds = (float)((double)ATT[row + j] * (Pd[j * TRP + r] - dot) * scale); DS[row + j] = ds; }
      Pf[j * TRP + r] = ds;
    }
  }
  __syncthreads();
  const TiledCols t = tiled_cols(hs);
  if (!t.on) return;
  float acc[TR];
#pragma unroll
  for (int r = 0; r < TR; ++r) acc[r] = 0.0f;
  tiled_accumulate(Pf, base + C, 3LL * C, jmax, t, acc);           // dQ = dS . K
#pragma unroll
  for (int r = 0; r < TR; ++r) {
    const int i = i0 + t.g + r * t.G;
    if (r < t.rpt && t.g + r * t.G < TR && i < i1) dQKV[((long long)b * Lm + i) * 3 * C + h * hs + t.d] = acc[r];
  }
}

// grid (B * nh, ceil(Lm / TR)): dV = drop(P)^T . dY and dK = dS^T . Q of the key rows [j0, j0 + TR), over the query rows j0 .. L - 1
__global__ __launch_bounds__(GT) void gptb_attn_bwd_keys_kernel(const float* __restrict__ QKV, const float* __restrict__ ATT,
                                                                const float* __restrict__ dY, const float* __restrict__ DS,
                                                                float* __restrict__ dQKV, int C, int nh, int Lm,
                                                                const int* __restrict__ Lp, float pdrop, uint64_t seed,
                                                                int layer, int Tmax) {
  extern __shared__ float sm[];
  const int b = blockIdx.x / nh, h = blockIdx.x % nh, hs = C / nh, tid = threadIdx.x, L = *Lp, j0 = blockIdx.y * TR;
  if (j0 >= L) return;
  const int N = L - j0;                                            // query rows i = j0 + n
  float* Wp = sm; float* Ws = Wp + Lm * TRP;
  const long long head = (long long)blockIdx.x * Lm * Lm;
  for (int e = tid; e < N * TR; e += GT) {
    const int n = e / TR, jj = e - n * TR, i = j0 + n, j = j0 + jj;
    float p = 0.0f, ds = 0.0f;
    if (j <= i && j < L) {
      p = ATT[head + (long long)i * Lm + j];
      if (pdrop > 0.0f) p *= drop_scale(seed, b, i, layer, 1, h * Tmax + j, pdrop);
      ds = DS[head + (long long)i * Lm + j];
    }
    Wp[n * TRP + jj] = p; Ws[n * TRP + jj] = ds;
  }
  __syncthreads();
  const TiledCols t = tiled_cols(hs);
  if (!t.on) return;
  float av[TR], ak[TR];
#pragma unroll
  for (int r = 0; r < TR; ++r) { av[r] = 0.0f; ak[r] = 0.0f; }
  tiled_accumulate(Wp, dY + ((long long)b * Lm + j0) * C + h * hs, (long long)C, N, t, av);
  tiled_accumulate(Ws, QKV + ((long long)b * Lm + j0) * 3 * C + h * hs, 3LL * C, N, t, ak);
#pragma unroll
  for (int r = 0; r < TR; ++r) {
    const int j = j0 + t.g + r * t.G;
    if (r < t.rpt && t.g + r * t.G < TR && j < L) {
      float* dst = dQKV + ((long long)b * Lm + j) * 3 * C + h * hs + t.d;
      dst[C] = ak[r]; dst[2 * C] = av[r];
    }
  }
}

// DL[m][a] = dlogits[b][i - 1][a] for the live tokens i >= 1 (token i predicts the action of step i - 1), else 0
__global__ __launch_bounds__(GT) void gptb_dl_kernel(const float* __restrict__ dlogits, float* __restrict__ DL, int B, int T,
                                                     int nA, int Lm, const int* __restrict__ Lp) {
  const int e = blockIdx.x * GT + threadIdx.x;
  if (e >= B * Lm * nA) return;
  const int m = e / nA, q = e - m * nA, b = m / Lm, i = m % Lm;
  DL[e] = (i >= 1 && i < *Lp) ? dlogits[((long long)b * T + (i - 1)) * nA + q] : 0.0f;
}

// Token embeddings (GPT.forward's embedding stage, src/models/gpt.py:308-343), batched like everything else:
//   gptb_parts_kernel   dXe = drop0(dX) with the class-token row taken out (its gradient goes to embed_class), and the
//                       concatenated embedding parts PARTS[m][p * C] of every live patch token (action, 1-D position,
//                       patch embedding, 2-D position — the order of the forward);
//   two GEMMs           dparts = dXe . proj^T,  g_proj += PARTS^T . dXe   (concat_emb; otherwise dparts = dXe / p);
//   gptb_scatter_kernel dparts -> the action / position tables (atomics) and the patch-embedding rows d_tok_emb.
struct TokInfo { int act, p1, row, col; };
__device__ __forceinline__ TokInfo tok_info(const GptBwdArgs& a, int b, int i) {
  const int t = i - 1;
  TokInfo r;
  // rollout: token i carries the action taken BEFORE its patch (BOS = 0); teacher-forced full sequence:
  // current_actions[b][t] (src/supervised.py:863-868)
  r.act = a.tok_actions ? (int)a.tok_actions[(long long)b * a.T + t] : ((i == 1) ? 0 : (int)a.actions[(long long)b * a.T + (i - 2)]);
  r.row = (int)a.positions[((long long)b * a.pos_tokens + t) * 2];
  r.col = (int)a.positions[((long long)b * a.pos_tokens + t) * 2 + 1];
  r.p1 = a.pos1d_by_token ? t : 0;                       // recurrent tokens: 1-D position 0 (gpt.py:431-449)
  return r;
}

__global__ __launch_bounds__(GT) void gptb_parts_kernel(GptBwdArgs a, const float* __restrict__ dX, float* __restrict__ dXe,
                                                        float* __restrict__ PARTS, int np, const int* __restrict__ Lp, int Lm) {
  const int m = blockIdx.x, b = m / Lm, i = m % Lm, C = a.C, tid = threadIdx.x, L = *Lp;
  const bool live = i < L;
  for (int c = tid; c < C; c += GT) {
    float v = live ? dX[(long long)m * C + c] : 0.0f;
    if (live && a.pdrop > 0.0f) v *= drop_scale(a.drop_seed, b, i, 0, 0, c, a.pdrop);     // through transformer.drop
    if (i == 0) {                                                                         // class token: row classes[b]
      const int cls = a.classes ? min(max((int)a.classes[b], 0), JN_N_CLASS_ROWS - 1) : 0;
      if (live) atomicAdd(&a.g_embed_class[(long long)cls * C + c], v);
      v = 0.0f;
    }
    dXe[(long long)m * C + c] = v;
  }
  float* pr = PARTS + (long long)m * np * C;
  if (!live || i == 0) {
    for (int e = tid; e < np * C; e += GT) pr[e] = 0.0f;
    return;
  }
  const TokInfo ti = tok_info(a, b, i);
  int p = 0;
  for (int c = tid; c < C; c += GT) pr[c] = a.wte[ti.act * C + c];
  ++p;
  for (int c = tid; c < C; c += GT) pr[p * C + c] = a.dec_pos_enc ? a.pos1d[ti.p1 * C + c] : a.wpe[ti.p1 * C + c];
  ++p;
  if (!a.no_patch_emb) {
    for (int c = tid; c < C; c += GT) pr[p * C + c] = a.tok_emb[((long long)b * a.T + (i - 1)) * C + c];
    ++p;
  }
  if (a.use_pos_emb)
    for (int c = tid; c < C; c += GT)
      pr[p * C + c] = (c < a.pe2_ch) ? a.pe2[ti.col * a.pe2_ch + c] : a.pe2[ti.row * a.pe2_ch + (c - a.pe2_ch)];
}

// one workgroup per (agent, step t): dparts row of token t + 1 (dp_ld floats per row; without concat_emb the row is dXe
// itself and every part receives 1 / np of it)
__global__ __launch_bounds__(GT) void gptb_scatter_kernel(GptBwdArgs a, const float* __restrict__ dparts, int dp_ld, int np,
                                                          const int* __restrict__ Lp, int Lm) {
  const int b = blockIdx.x / a.T, t = blockIdx.x % a.T, i = t + 1, C = a.C, tid = threadIdx.x, L = *Lp;
  float* dte = a.d_tok_emb + ((long long)b * a.dte_stride_b + (long long)t * a.dte_stride_t) * C;
  if (i >= L) {                                          // steps that were never executed: zero patch-embedding gradient
    for (int c = tid; c < C; c += GT) dte[c] = 0.0f;
    return;
  }
  const TokInfo ti = tok_info(a, b, i);
  const float* dp = dparts + ((long long)b * Lm + i) * dp_ld;
  const float sc = a.concat_emb ? 1.0f : 1.0f / np;
  const int o_pos = a.concat_emb ? C : 0, o_patch = a.concat_emb ? 2 * C : 0;
  for (int c = tid; c < C; c += GT) {
    atomicAdd(&a.g_wte[ti.act * C + c], dp[c] * sc);
    if (!a.dec_pos_enc && a.g_wpe) atomicAdd(&a.g_wpe[ti.p1 * C + c], dp[o_pos + c] * sc);
    if (!a.no_patch_emb) dte[c] = dp[o_patch + c] * sc;
  }
}

struct Layout {
  long long M, C, X, lay, lay_sz, tmp;
  long long o_H1, o_QKV, o_ATT, o_Y, o_XM, o_H2, o_Fp, o_st;   // inside a layer block
};
Layout make_layout(int C, int nh, int nL, int B, int T) {
  Layout y{};
  const long long Lm = T + 1;
  y.M = (long long)B * Lm; y.C = C;
  y.X = 16;                                            // header (L) first
  y.lay = y.X + (long long)(nL + 1) * y.M * C;
  y.o_H1 = 0; y.o_QKV = y.o_H1 + y.M * C; y.o_ATT = y.o_QKV + y.M * 3 * C; y.o_Y = y.o_ATT + (long long)B * nh * Lm * Lm;
  y.o_XM = y.o_Y + y.M * C; y.o_H2 = y.o_XM + y.M * C; y.o_Fp = y.o_H2 + y.M * C; y.o_st = y.o_Fp + y.M * 4 * C;
  y.lay_sz = y.o_st + 4 * y.M;
  y.tmp = y.lay + (long long)nL * y.lay_sz;
  return y;
}

}  // namespace

size_t gpt_backward_batched_scratch(int C, int n_head, int n_layer, int nA, int B, int T, bool tiled) {
  const Layout y = make_layout(C, n_head, n_layer, B, T);
  // temporaries: dX dXM dH dY dO HF (M*C each), dQKV (3), dF (4), DL (M*nA), ln_f statistics (2M); the tiled attention adds
  // DS, one buffer of a layer's ATT shape
  const long long Lm = T + 1, ds = tiled ? (long long)B * n_head * Lm * Lm : 0;
  return (size_t)(y.tmp + y.M * (13LL * C + nA + 2) + ds + 64);
}

// The LayerNorm backward holds C / 64 <= LN_CQ columns per lane; the attention kernels keep q, k, v, dO of a head
// (4 * Lm * hs floats) and two Lm x Lm score tiles in the 64 KB of LDS a kernel gets without asking (Lm = T + 1).
bool gpt_backward_batched_admits(int C, int n_head, int T) {
  if (C <= 0 || n_head <= 0 || C % n_head != 0 || T < 1 || C > 64 * LN_CQ) return false;
  const size_t Lm = (size_t)T + 1, hs = (size_t)(C / n_head);
  return (4 * Lm * hs + 2 * Lm * Lm) * sizeof(float) <= 64 * 1024;
}

// What the tiled attention kernels take (with the LayerNorm backward's bound on C): any head up to T_MAX_HS columns, any
// sequence up to T_MAX_LM tokens.
static bool tiled_admits(int C, int n_head, int T) {
  if (C <= 0 || n_head <= 0 || C % n_head != 0 || T < 1 || C > 64 * LN_CQ) return false;
  return T + 1 <= T_MAX_LM && C / n_head <= T_MAX_HS;
}

// JN_GPT_BWD_TILED=1 (test hook, read per launch so that a test can flip it): a per-agent-route shape that would take the LDS
// form or the per-agent kernel takes the tiled form.  (The name is held in a constant: the hook is listed in DESIGN.md §4.5.)
static const char* const kTiledHook = "JN_GPT_BWD_TILED";

GptBwdRoute gpt_backward_route(int C, int n_head, int T, int decision_route) {
  if (C <= 0 || n_head <= 0 || C % n_head != 0 || T < 1) return GPT_BWD_NONE;
  if (decision_route == 0 && tiled_admits(C, n_head, T)) {
    const char* hook = std::getenv(kTiledHook);
    if (hook && std::atoi(hook) == 1) return GPT_BWD_TILED;
  }
  if (gpt_backward_batched_admits(C, n_head, T)) return GPT_BWD_LDS;
  if (decision_route == 1) return GPT_BWD_NONE;                    // a wide context has no other backward
  if (T <= GPT_PER_AGENT_MAX_T) return C <= GPT_PER_AGENT_MAX_C ? GPT_BWD_PER_AGENT : GPT_BWD_NONE;
  return tiled_admits(C, n_head, T) ? GPT_BWD_TILED : GPT_BWD_NONE;
}

// One layer's attention on caller tensors (jn_gpt_attention_backward): the recompute (ATT, Y), then dQKV.  form 0: the LDS
// kernels, 1: the tiled ones (DS: a buffer of ATT's shape).  Returns 1 when the form does not take the shape.
int launch_gpt_attention(int form, const float* QKV, const float* dY, int B, int nh, int C, int Lm, const int* Lp, float pdrop,
                         uint64_t seed, int layer, int Tmax, float* ATT, float* Y, float* DS, float* dQKV, hipStream_t s) {
  if (C <= 0 || nh <= 0 || C % nh != 0 || Lm < 1 || B < 1) return 1;
  const int hs = C / nh;
  if (form == 0) {
    const size_t lds = ((size_t)4 * Lm * hs + (size_t)2 * Lm * Lm) * sizeof(float);
    if (lds > 64 * 1024) return 1;
    hipLaunchKernelGGL(gptb_attn_fwd_kernel, dim3(B * nh), dim3(GT), lds, s, QKV, ATT, Y, C, nh, Lm, Lp, pdrop, seed, layer, Tmax);
    hipLaunchKernelGGL(gptb_attn_bwd_kernel, dim3(B * nh), dim3(GT), lds, s, QKV, ATT, dY, dQKV, C, nh, Lm, Lp, pdrop, seed, layer, Tmax);
    return 0;
  }
  if (form != 1 || Lm > T_MAX_LM || hs > T_MAX_HS) return 1;
  const dim3 grid(B * nh, (Lm + TR - 1) / TR);
  hipLaunchKernelGGL(gptb_attn_fwd_tiled_kernel, grid, dim3(GT), tiled_row_lds(Lm, hs), s, QKV, ATT, Y, C, nh, Lm, Lp, pdrop, seed,
                     layer, Tmax);
  hipLaunchKernelGGL(gptb_attn_bwd_rows_kernel, grid, dim3(GT), tiled_row_lds(Lm, hs), s, QKV, ATT, dY, DS, dQKV, C, nh, Lm, Lp,
                     pdrop, seed, layer, Tmax);
  hipLaunchKernelGGL(gptb_attn_bwd_keys_kernel, grid, dim3(GT), tiled_key_lds(Lm), s, QKV, ATT, dY, DS, dQKV, C, nh, Lm, Lp, pdrop,
                     seed, layer, Tmax);
  return 0;
}

// Returns 0 when launched, 1 when the shape is outside what the chosen attention form takes (tiled: the tiled kernels and
// their DS buffer, which gpt_backward_batched_scratch(..., true) counts; else the LDS kernels).
int launch_gpt_backward_batched(const GptBwdArgs& a, const GptLayerPtrs* W, const GptLayerPtrs* G, hipStream_t s, bool tiled) {
  const int C = a.C, nh = a.n_head, nL = a.n_layer, B = a.B, T = a.T, Lm = T + 1, hs = C / nh, nA = a.nA;
  const size_t attn_lds = ((size_t)4 * Lm * hs + (size_t)2 * Lm * Lm) * sizeof(float);
  if (!(tiled ? tiled_admits(C, nh, T) : gpt_backward_batched_admits(C, nh, T))) return 1;
  const Layout y = make_layout(C, nh, nL, B, T);
  const int M = (int)y.M;
  float* sc = a.scratch;
  int* Lp = reinterpret_cast<int*>(sc);
  float* X = sc + y.X;
  float* tmp = sc + y.tmp;
  float* dX = tmp; float* dXM = dX + (long long)M * C; float* dH = dXM + (long long)M * C; float* dY = dH + (long long)M * C;
  float* dO = dY + (long long)M * C; float* HF = dO + (long long)M * C; float* dQKV = HF + (long long)M * C;
  float* dF = dQKV + (long long)M * 3 * C; float* DL = dF + (long long)M * 4 * C; float* muF = DL + (long long)M * nA;
  float* rsF = muF + M;
  float* DS = rsF + M;                                   // tiled attention only
  const dim3 tiled_grid(B * nh, (Lm + TR - 1) / TR);
  const bool drop = a.pdrop > 0.0f;
  const int row_blocks = (M + GT / 64 - 1) / (GT / 64), lnb_blocks = (M + LN_RPB - 1) / LN_RPB;
  const long long MC = (long long)M * C;
  auto G0 = [&]() {
    GemmArgs g{};
    g.L = Lp; g.Lm = Lm; g.site = -1; g.pdrop = a.pdrop; g.seed = a.drop_seed;
    return g;
  };
  // forward: out[M x N] = in[M x K] . Wt[K x N] (+ bias)
  auto fwd = [&](float* out, const float* in, const float* wt, const float* bias, int K, int N, const float* resid, int site,
                 int layer, int a_gelu) {
    GemmArgs g = G0();
    g.A = in; g.a_rs = K; g.a_cs = 1; g.B = wt; g.b_rs = N; g.b_cs = 1; g.C = out; g.c_rs = N; g.M = M; g.N = N; g.K = K;
    g.bias = bias; g.resid = resid; g.site = site; g.layer = layer; g.a_gelu = a_gelu; g.tok_dim = 0;
    gemm(g, s);
  };
  // data gradient: din[M x K] = dout[M x N] . Wt^T (optionally * gelu'(mulp))
  auto bwd_data = [&](float* din, const float* dout, const float* wt, int K, int N, const float* mulp) {
    GemmArgs g = G0();
    g.A = dout; g.a_rs = N; g.a_cs = 1; g.B = wt; g.b_rs = 1; g.b_cs = N; g.C = din; g.c_rs = K; g.M = M; g.N = K; g.K = N;
    g.mulp = mulp; g.tok_dim = 0;
    gemm(g, s);
  };
  // weight gradient: gwt[K x N] += in^T . dout; bias gradient: gb[N] += column sums of dout
  auto bwd_weight = [&](float* gwt, float* gb, const float* in, const float* dout, int K, int N, int a_gelu) {
    GemmArgs g = G0();
    g.A = in; g.a_rs = 1; g.a_cs = K; g.B = dout; g.b_rs = N; g.b_cs = 1; g.C = gwt; g.c_rs = N; g.M = K; g.N = N; g.K = M;
    g.a_gelu = a_gelu; g.accumulate = 1; g.tok_dim = 1;
    wgrad(g, gb, s);
  };
  auto ln_fwd = [&](float* out, const float* x, const float* w, const float* b, float* mu, float* rs) {
    hipLaunchKernelGGL(gptb_ln_fwd_kernel, dim3(row_blocks), dim3(GT), 0, s, x, w, b, out, mu, rs, M, C, Lp, Lm);
  };
  auto ln_bwd = [&](float* din, const float* base, const float* dout, const float* x, const float* w, float* gw, float* gb,
                    const float* mu, const float* rs) {
    hipLaunchKernelGGL(gptb_ln_bwd_kernel, dim3(lnb_blocks), dim3(GT), 0, s, din, base, dout, x, w, gw, gb, mu, rs, M, C, Lp, Lm);
  };
  auto dropmul = [&](float* dst, const float* src, int layer, int site) {
    hipLaunchKernelGGL(gptb_drop_kernel, dim3((unsigned)((MC + GT - 1) / GT)), dim3(GT), 0, s, dst, src, MC, C, layer, site,
                       a.pdrop, a.drop_seed, Lp, Lm);
  };

  hipLaunchKernelGGL(gptb_init_kernel, dim3((unsigned)std::min<long long>((MC + GT - 1) / GT, 1024)), dim3(GT), 0, s, a, Lp, X, Lm);
  // ---------------- forward recompute ----------------
  for (int l = 0; l < nL; ++l) {
    const GptLayerPtrs& w = W[l];
    float* x = X + (long long)l * MC;
    float* lay = sc + y.lay + (long long)l * y.lay_sz;
    float *H1 = lay + y.o_H1, *QKV = lay + y.o_QKV, *ATT = lay + y.o_ATT, *Yb = lay + y.o_Y, *XM = lay + y.o_XM,
          *H2 = lay + y.o_H2, *Fp = lay + y.o_Fp, *st = lay + y.o_st;
    ln_fwd(H1, x, w.ln1_w, w.ln1_b, st, st + M);
    fwd(QKV, H1, w.qkv_wt, w.qkv_b, C, 3 * C, nullptr, -1, l, 0);
    if (tiled)
      hipLaunchKernelGGL(gptb_attn_fwd_tiled_kernel, tiled_grid, dim3(GT), tiled_row_lds(Lm, hs), s, QKV, ATT, Yb, C, nh, Lm, Lp,
                         a.pdrop, a.drop_seed, l, a.Tmax);
    else
      hipLaunchKernelGGL(gptb_attn_fwd_kernel, dim3(B * nh), dim3(GT), attn_lds, s, QKV, ATT, Yb, C, nh, Lm, Lp, a.pdrop,
                         a.drop_seed, l, a.Tmax);
    fwd(XM, Yb, w.proj_wt, w.proj_b, C, C, x, 2, l, 0);                       // XM = x + drop(proj(Y))
    ln_fwd(H2, XM, w.ln2_w, w.ln2_b, st + 2 * M, st + 3 * M);
    fwd(Fp, H2, w.fc_wt, w.fc_b, C, 4 * C, nullptr, -1, l, 0);                // pre-activation
    fwd(x + MC, Fp, w.fc2_wt, w.fc2_b, 4 * C, C, XM, 3, l, 1);                // x' = XM + drop(fc2(gelu(F)))
  }
  float* xl = X + (long long)nL * MC;
  ln_fwd(HF, xl, a.lnf_w, a.lnf_b, muF, rsF);
  // ---------------- head + ln_f backward ----------------
  hipLaunchKernelGGL(gptb_dl_kernel, dim3((M * nA + GT - 1) / GT), dim3(GT), 0, s, a.dlogits, DL, B, T, nA, Lm, Lp);
  bwd_data(dH, DL, a.head_wt, C, nA, nullptr);                                 // dHF = DL . head_wt^T   (head_wt: [C][nA])
  bwd_weight(a.g_head_wt, nullptr, HF, DL, C, nA, 0);
  ln_bwd(dX, nullptr, dH, xl, a.lnf_w, a.g_lnf_w, a.g_lnf_b, muF, rsF);
  // ---------------- blocks, last to first ----------------
  for (int l = nL - 1; l >= 0; --l) {
    const GptLayerPtrs& w = W[l];
    const GptLayerPtrs& gr = G[l];
    float* x = X + (long long)l * MC;
    float* lay = sc + y.lay + (long long)l * y.lay_sz;
    float *H1 = lay + y.o_H1, *QKV = lay + y.o_QKV, *ATT = lay + y.o_ATT, *Yb = lay + y.o_Y, *XM = lay + y.o_XM,
          *H2 = lay + y.o_H2, *Fp = lay + y.o_Fp, *st = lay + y.o_st;
    // mlp: x' = XM + drop(fc2(gelu(fc(H2))))
    const float* dOut = dX;
    if (drop) { dropmul(dO, dX, l, 3); dOut = dO; }
    bwd_data(dF, dOut, w.fc2_wt, 4 * C, C, Fp);                                // dF = (dO . fc2^T) * gelu'(F)
    bwd_weight(gr.fc2_wt, gr.fc2_b, Fp, dOut, 4 * C, C, 1);                    // gelu(F)^T . dO
    bwd_data(dH, dF, w.fc_wt, C, 4 * C, nullptr);
    bwd_weight(gr.fc_wt, gr.fc_b, H2, dF, C, 4 * C, 0);
    ln_bwd(dXM, dX, dH, XM, w.ln2_w, gr.ln2_w, gr.ln2_b, st + 2 * M, st + 3 * M);       // dXM = dX + LN2^T(dH)
    // attention: XM = x + drop(proj(Y))
    const float* dPo = dXM;
    if (drop) { dropmul(dO, dXM, l, 2); dPo = dO; }
    bwd_data(dY, dPo, w.proj_wt, C, C, nullptr);
    bwd_weight(gr.proj_wt, gr.proj_b, Yb, dPo, C, C, 0);
    if (tiled) {
      hipLaunchKernelGGL(gptb_attn_bwd_rows_kernel, tiled_grid, dim3(GT), tiled_row_lds(Lm, hs), s, QKV, ATT, dY, DS, dQKV, C, nh,
                         Lm, Lp, a.pdrop, a.drop_seed, l, a.Tmax);
      hipLaunchKernelGGL(gptb_attn_bwd_keys_kernel, tiled_grid, dim3(GT), tiled_key_lds(Lm), s, QKV, ATT, dY, DS, dQKV, C, nh, Lm,
                         Lp, a.pdrop, a.drop_seed, l, a.Tmax);
    } else {
      hipLaunchKernelGGL(gptb_attn_bwd_kernel, dim3(B * nh), dim3(GT), attn_lds, s, QKV, ATT, dY, dQKV, C, nh, Lm, Lp, a.pdrop,
                         a.drop_seed, l, a.Tmax);
    }
    bwd_data(dH, dQKV, w.qkv_wt, C, 3 * C, nullptr);
    bwd_weight(gr.qkv_wt, gr.qkv_b, H1, dQKV, C, 3 * C, 0);
    ln_bwd(dX, dXM, dH, x, w.ln1_w, gr.ln1_w, gr.ln1_b, st, st + M);                    // dX = dXM + LN1^T(dH)
  }
  // ---------------- token embeddings ----------------
  const int np = 2 + (a.no_patch_emb ? 0 : 1) + (a.use_pos_emb ? 1 : 0);
  float* dXe = dXM;                                      // free from here on
  float* PARTS = sc + y.lay + y.o_Fp;                    // layer 0's M x 4C block, free as well
  float* dparts = dF;
  hipLaunchKernelGGL(gptb_parts_kernel, dim3(M), dim3(GT), 0, s, a, dX, dXe, PARTS, np, Lp, Lm);
  if (a.concat_emb) {
    bwd_data(dparts, dXe, a.proj_wt, np * C, C, nullptr);                      // proj_wt: [np * C][C]
    bwd_weight(a.g_proj_wt, a.g_proj_b, PARTS, dXe, np * C, C, 0);
    hipLaunchKernelGGL(gptb_scatter_kernel, dim3(B * T), dim3(GT), 0, s, a, dparts, np * C, np, Lp, Lm);
  } else {
    hipLaunchKernelGGL(gptb_scatter_kernel, dim3(B * T), dim3(GT), 0, s, a, dXe, C, np, Lp, Lm);
  }
  return 0;
}

}  // namespace jnr
