// Backward kernels of the 1x1 (pointwise) convs of the PAFPN patch encoder for gfx950: the weight gradient (step 4 of
// kernels_bwd.hip, which describes the steps and holds the other layer kinds) and the passes that fuse steps 2 + 3 + 4 of
// a layer.  Activations are fp32 (training refuses bf16 storage: run_net_backward).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "jn_kernels.h"
#include "jn_reduce.h"
#include "jn_split.h"
#include "jn_tab.h"
#include "jn_types.h"

namespace jnr {

// ---- 4a. pointwise weight gradient: dW[n][k] += sum_m gz[m][n] * T(x[m][k]) ---------------------
// Workgroup = (row chunk, 16*CTN channels of n, 16*CTK channels of k); 64 rows staged per
// iteration in LDS, each wave contracts 16 of them per iteration on v_mfma_f32_16x16x4_f32.
constexpr int WG_RB = 64;

template <int CTN, int CTK>
__global__ __launch_bounds__(256) void pw_bwd_weight_kernel(const float* __restrict__ gz, int g_ld,
                                                            const float* __restrict__ x, int x_ld, ChanTab it,
                                                            float* __restrict__ gw, int rep, long long M, int N,
                                                            int K, int rows_per_block, int chunks_per_slot,
                                                            long long gz_slot, long long x_slot, long long tab_slot) {
  constexpr int LDN = 16 * CTN + 4, LDK = 16 * CTK + 4;
  const int slot = blockIdx.x / chunks_per_slot, chunk = blockIdx.x - slot * chunks_per_slot;
  gz += slot * gz_slot; x += slot * x_slot;
  it.sc += slot * tab_slot; it.sh += slot * tab_slot; it.fl += slot * tab_slot;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* Gs = sm;                      // [WG_RB][LDN]
  float* As = sm + WG_RB * LDN;        // [WG_RB][LDK]
  float* Ts = As + WG_RB * LDK;        // [16*CTN][16*CTK] block partial
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.y * 16 * CTN, k0 = blockIdx.z * 16 * CTK;
  const long long r0 = (long long)chunk * rows_per_block;
  const long long r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  f32x4 acc[CTN][CTK];
#pragma unroll
  for (int a = 0; a < CTN; ++a)
#pragma unroll
    for (int b = 0; b < CTK; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long long rb = r0; rb < r1; rb += WG_RB) {
    __syncthreads();
    for (int i = tid; i < WG_RB * 4 * CTN; i += 256) {
      const int r = i / (4 * CTN), q = i % (4 * CTN);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (rb + r < r1 && n0 + 4 * q < N) v = *reinterpret_cast<const f32x4*>(gz + (rb + r) * g_ld + n0 + 4 * q);
      *reinterpret_cast<f32x4*>(Gs + r * LDN + 4 * q) = v;
    }
    for (int i = tid; i < WG_RB * 4 * CTK; i += 256) {
      const int r = i / (4 * CTK), q = i % (4 * CTK);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      const int kk = k0 + 4 * q;
      if (rb + r < r1 && kk < K)
        v = tf4(*reinterpret_cast<const f32x4*>(x + (rb + r) * x_ld + kk), *reinterpret_cast<const f32x4*>(it.sc + kk),
                *reinterpret_cast<const f32x4*>(it.sh + kk), *reinterpret_cast<const f32x4*>(it.fl + kk));
      *reinterpret_cast<f32x4*>(As + r * LDK + 4 * q) = v;
    }
    __syncthreads();
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const int row = wave * 16 + 4 * st + g;
      float av[CTN], bv[CTK];
#pragma unroll
      for (int a = 0; a < CTN; ++a) av[a] = Gs[row * LDN + 16 * a + lm];
#pragma unroll
      for (int b = 0; b < CTK; ++b) bv[b] = As[row * LDK + 16 * b + lm];
#pragma unroll
      for (int a = 0; a < CTN; ++a)
#pragma unroll
        for (int b = 0; b < CTK; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc[a][b], 0, 0, 0);
    }
  }
  // cross-wave sum of the four partial tiles: one wave at a time, plain LDS read-modify-write
  // (LDS float atomics cost ~3x the whole kernel here: ds_add_f32 with 4-way bank conflicts)
  for (int w = 0; w < 4; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int a = 0; a < CTN; ++a)
#pragma unroll
        for (int b = 0; b < CTK; ++b)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* tp = &Ts[(16 * a + 4 * g + r) * (16 * CTK) + 16 * b + lm];
            *tp = (w == 0 ? 0.0f : *tp) + acc[a][b][r];
          }
    }
  }
  __syncthreads();
  float* dst = rep ? gw + (blockIdx.x % JN_NREP) * JN_WPART_MAX : gw;
  for (int i = tid; i < 256 * CTN * CTK; i += 256) {
    const int n = n0 + i / (16 * CTK), k = k0 + i % (16 * CTK);
    if (n < N && k < K) atomicAdd(&dst[(long long)n * K + k], Ts[i]);
  }
}

template <int CTN, int CTK>
static void launch_pw_bw_t(const float* gz, int g_ld, const float* x, int x_ld, ChanTab it, float* gw, int rep, long long M,
                           int N, int K, hipStream_t s, const SlotBatch& sb, long long gz_slot) {
  // aim at ~768 workgroups: enough to fill 256 CUs x 3, few enough that the final atomics stay cheap
  const long long tiles = (long long)((N + 16 * CTN - 1) / (16 * CTN)) * ((K + 16 * CTK - 1) / (16 * CTK));
  long long rpb = (M * sb.n * tiles / 768 + 63) / 64 * 64;
  if (rpb < 64) rpb = 64;
  if (rpb > 4096) rpb = 4096;
  const int rows_per_block = (int)rpb;
  const int chunks_per_slot = (int)((M + rows_per_block - 1) / rows_per_block);
  const long long x_slot = sb.act, tab_slot = sb.tab;
  dim3 grid((unsigned)(chunks_per_slot * sb.n), (N + 16 * CTN - 1) / (16 * CTN), (K + 16 * CTK - 1) / (16 * CTK));
  const size_t smem = ((size_t)WG_RB * (16 * CTN + 4 + 16 * CTK + 4) + 256 * CTN * CTK) * sizeof(float);
  hipLaunchKernelGGL((pw_bwd_weight_kernel<CTN, CTK>), grid, dim3(256), smem, s, gz, g_ld, x, x_ld, it, gw, rep, M, N, K,
                     rows_per_block, chunks_per_slot, gz_slot, x_slot, tab_slot);
}

// Wide layers (N, K >= 128): workgroup tile = 128 x 128 outputs, wave w owns the 64 x 64 quadrant (w & 1, w >> 1) and
// contracts ALL 64 rows of a stage itself (no cross-wave sum).  Against the 64 x 64 tiles above every input row is
// re-read half as often: (N/128 + K/128) instead of (N/64 + K/64) passes over g_z / x.
// SP (the default; JN_WW_EXACT=1 keeps fp32 MFMA): both operands are split into two bf16 terms when they leave LDS
// (x = hi + lo to 2^-17) and each 16 x 16 x 32 block takes three v_mfma_f32_16x16x32_bf16 (hi*hi + hi*lo + lo*hi; lo*lo
// < 2^-16 of the product is dropped) — 48 matrix-pipe cycles instead of the 256 of eight fp32 MFMAs, which turns the
// kernel from matrix-bound (~40 % of the fp32 peak) into a pass at memory speed.  A weight gradient is a leaf: its ~1e-5
// relative error goes to the optimiser and nowhere else (the forward / data-gradient GEMMs stay exact).
// Lane group g of a k-step takes rows 4g + (e & 3) + 16 (e >> 2): any row order is a valid contraction order, and this
// one puts the four groups 16 banks apart (row stride 132 floats).
template <bool SP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void pw_bwd_weight_wide_kernel(const float* __restrict__ gz, int g_ld,
                                                                 const float* __restrict__ x, int x_ld, ChanTab it,
                                                                 float* __restrict__ gw, long long M, int N, int K,
                                                                 int rows_per_block, int chunks_per_slot,
                                                                 long long gz_slot, long long x_slot, long long tab_slot) {
  constexpr int LD = 128 + 4;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* Gs = sm;                 // [64][LD]
  float* As = sm + 64 * LD;       // [64][LD]
  const int slot = blockIdx.x / chunks_per_slot, chunk = blockIdx.x - slot * chunks_per_slot;
  gz += slot * gz_slot; x += slot * x_slot;
  it.sc += slot * tab_slot; it.sh += slot * tab_slot; it.fl += slot * tab_slot;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.y * 128, k0 = blockIdx.z * 128;
  const int wn = (wave & 1) * 64, wk = (wave >> 1) * 64;
  const long long r0 = (long long)chunk * rows_per_block;
  const long long r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the channel quad of a thread is fixed (256 % 32 == 0)
  const int q = tid & 31;
  f32x4 i_sc = {1.f, 1.f, 1.f, 1.f}, i_sh = {0.f, 0.f, 0.f, 0.f}, i_fl = {0.f, 0.f, 0.f, 0.f};
  if (k0 + 4 * q < K) {
    i_sc = *reinterpret_cast<const f32x4*>(it.sc + k0 + 4 * q); i_sh = *reinterpret_cast<const f32x4*>(it.sh + k0 + 4 * q);
    i_fl = *reinterpret_cast<const f32x4*>(it.fl + k0 + 4 * q);
  }
  // the next 64-row block is fetched into registers while the MFMAs of the current one run (two workgroups per CU
  // alone left the matrix pipe 50 % busy)
  f32x4 pg[8], px[8];
  auto fetch = [&](long long rb) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = (tid >> 5) + 8 * j;
      pg[j] = f32x4{0.f, 0.f, 0.f, 0.f}; px[j] = pg[j];
      if (rb + r < r1) {
        if (n0 + 4 * q < N) pg[j] = *reinterpret_cast<const f32x4*>(gz + (rb + r) * g_ld + n0 + 4 * q);
        if (k0 + 4 * q < K) px[j] = ld4(x + (rb + r) * x_ld + k0 + 4 * q);
      }
    }
  };
  if (r0 < r1) fetch(r0);
  for (long long rb = r0; rb < r1; rb += 64) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = (tid >> 5) + 8 * j;
      f32x4 u = {0.f, 0.f, 0.f, 0.f};
      if (rb + r < r1 && k0 + 4 * q < K) u = tf4(px[j], i_sc, i_sh, i_fl);
      *reinterpret_cast<f32x4*>(Gs + r * LD + 4 * q) = pg[j];
      *reinterpret_cast<f32x4*>(As + r * LD + 4 * q) = u;
    }
    __syncthreads();
    if (rb + 64 < r1) fetch(rb + 64);
    if constexpr (SP) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const float* gs = Gs + (ks * 32 + 4 * g) * LD + wn + lm;
        const float* as = As + (ks * 32 + 4 * g) * LD + wk + lm;
        bf16x8 bh[4], bl[4];
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float v = as[((e & 3) + 16 * (e >> 2)) * LD + 16 * b];
            // split2 of jn_split.h written out, here and below: through the helper this kernel's registers are allocated
            // differently (profiles/conv3_unit_ab.txt)
            const bf16_t h = (bf16_t)v;
            bh[b][e] = h; bl[b][e] = (bf16_t)(v - (float)h);
          }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          bf16x8 ah, al;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float v = gs[((e & 3) + 16 * (e >> 2)) * LD + 16 * a];
            const bf16_t h = (bf16_t)v;
            ah[e] = h; al[e] = (bf16_t)(v - (float)h);
          }
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh[b], acc[a][b], 0, 0, 0);
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl[b], acc[a][b], 0, 0, 0);
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh[b], acc[a][b], 0, 0, 0);
          }
        }
      }
    } else {
#pragma unroll 4
      for (int st = 0; st < 16; ++st) {
        const int row = 4 * st + g;
        float av[4], bv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) av[a] = Gs[row * LD + wn + 16 * a + lm];
#pragma unroll
        for (int b = 0; b < 4; ++b) bv[b] = As[row * LD + wk + 16 * b + lm];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc[a][b], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wn + 16 * a + 4 * g + r, k = k0 + wk + 16 * b + lm;
        if (n < N && k < K) atomicAdd(&gw[(long long)n * K + k], acc[a][b][r]);
      }
}

template <bool SP>
static int launch_pw_bwd_weight_wide(const float* gz, int g_ld, const float* x, int x_ld, ChanTab it, float* gw, long long M,
                                     int N, int K, hipStream_t s, const SlotBatch& sb, long long gz_slot) {
  const long long tiles = (long long)((N + 127) / 128) * ((K + 127) / 128);
  long long rpb = (M * sb.n * tiles / 1024 + 63) / 64 * 64;     // ~1024 workgroups (2 fit per CU)
  if (rpb < 256) rpb = 256;
  if (rpb > 8192) rpb = 8192;
  const int chunks_per_slot = (int)((M + rpb - 1) / rpb);
  dim3 grid((unsigned)(chunks_per_slot * sb.n), (N + 127) / 128, (K + 127) / 128);
  const size_t smem = (size_t)2 * 64 * (128 + 4) * sizeof(float);
  if (!allow_lds<&pw_bwd_weight_wide_kernel<SP>>(smem)) return -1;
  hipLaunchKernelGGL((pw_bwd_weight_wide_kernel<SP>), grid, dim3(256), smem, s, gz, g_ld, x, x_ld, it, gw, M, N, K, (int)rpb,
                     chunks_per_slot, gz_slot, sb.act, sb.tab);
  return 0;
}

int launch_pw_bwd_weight(const float* gz, int g_ld, const float* x, int x_ld, ChanTab it, float* gw_final, float* wpart,
                         long long M, int N, int K, hipStream_t s, const SlotBatch& sb, long long gz_slot_stride, int route) {
  const long long gz_slot = gz_slot_stride >= 0 ? gz_slot_stride : sb.grad;
  if (pw_bwd_weight_wide(N, K)) {
    static const bool exact_env = std::getenv("JN_WW_EXACT") != nullptr;
    const bool exact = route ? route == CW_ROUTE_EXACT : exact_env;
    return exact ? launch_pw_bwd_weight_wide<false>(gz, g_ld, x, x_ld, it, gw_final, M, N, K, s, sb, gz_slot)
                 : launch_pw_bwd_weight_wide<true>(gz, g_ld, x, x_ld, it, gw_final, M, N, K, s, sb, gz_slot);
  }
  const int rep = (wpart && N * K <= JN_WPART_MAX) ? 1 : 0;
  float* gw = rep ? wpart : gw_final;
  const int tn = (N + 15) / 16, tk = (K + 15) / 16;
  const int cn = tn >= 4 ? 4 : (tn == 3 ? 3 : tn), ck = tk >= 4 ? 4 : (tk == 3 ? 3 : tk);
#define JN_BW(A, B) if (cn == A && ck == B) { launch_pw_bw_t<A, B>(gz, g_ld, x, x_ld, it, gw, rep, M, N, K, s, sb, gz_slot); \
    if (rep) launch_wpart_reduce(gw_final, wpart, N * K, s); return 0; }
  JN_BW(1, 1) JN_BW(1, 2) JN_BW(1, 3) JN_BW(1, 4) JN_BW(2, 1) JN_BW(2, 2) JN_BW(2, 3) JN_BW(2, 4)
  JN_BW(3, 1) JN_BW(3, 2) JN_BW(3, 3) JN_BW(3, 4) JN_BW(4, 1) JN_BW(4, 2) JN_BW(4, 3) JN_BW(4, 4)
#undef JN_BW
  return -1;
}

// ---- 2+3+4 fused for pointwise layers with few channels ------------------------------------------
// One pass over (g_a, z) of the layer output and z of the layer input does the whole layer:
//   g_z = k * (g_a * silu'(y) - c1 - zhat * c2)      (never written to HBM)
//   g_in (=|+=) g_z . W                              (phase 2: the forward kernel's MFMA loop with X = g_z, W^T)
//   dW  += g_z^T . a_in                              (phase 3: contraction over the 64 pixels of the tile)
// HBM traffic 8 B/output + 8 B/input element instead of 20 + 8 for the bn_bwd_gz / data / weight kernels.
// Workgroup = 4 waves, 64 pixels per iteration, persistent over the tiles of ONE slot (blockIdx.y) so the
// per-channel constants sit in registers and dW in accumulators; Cout = 16*CTN, Cin = 16*CTK, CTN*CTK <= 16.
// RED: the layer input is the output of ONE BatchNorm conv with no other consumer: the per-channel sums of ITS backward
// (bn_bwd_reduce: sum g_a*silu'(y), sum g_a*silu'(y)*zhat) are accumulated here from the data gradient still in the
// MFMA accumulators (z of the input tile is re-read, L2-hot), so that layer's reduce pass over (g, z) never runs.
// RED2 (round 4; round 3 had it inside every RED instantiation, where its operands cost all of them a wave of occupancy:
// now its own instantiation): the first run of the input is a materialised shortcut sum silu(bn(z2)) + res; the kernel
// writes the sum's FINAL gradient, which is also the gradient of the activation of z2 — the bottleneck's last pointwise
// conv — so the sums of that run are formed with z2 / its table and go to THAT conv's BatchNorm.
template <int CTN, int CTK, bool RED, bool RED2 = false>
__global__ __launch_bounds__(256) void pw_bwd_fused_kernel(
    const float* __restrict__ g, int g_ld, const float* __restrict__ z, int z_ld, ChanTab ot,
    const float* __restrict__ save, const float* __restrict__ consts, const float* __restrict__ x, int x_ld,
    ChanTab it, const float* __restrict__ w, float* __restrict__ gx, int gx_ld, int accumulate,
    float* __restrict__ gw, int rep, long long M, SlotBatch sb, double* __restrict__ red_in, long long red_rep_stride,
    const float* __restrict__ gadd, int gadd_ld, double* __restrict__ red_in2, int red_split,
    const float* __restrict__ red2_z, int red2_ld, const float* __restrict__ red2_sc, const float* __restrict__ red2_sh) {
  constexpr int N = 16 * CTN, K = 16 * CTK;          // output / input channels
  constexpr int LDG = N + 4, LDA = K + 4, LDW = N + 4;
  constexpr int NG = 64 * (N / 4) / 256, NA = 64 * (K / 4) / 256;     // f32x4 per thread per tile (may be 0 -> 1)
  constexpr int NGq = NG > 0 ? NG : 1, NAq = NA > 0 ? NA : 1;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* Gs = sm;                       // [64][LDG]  g_z tile
  float* As = Gs + 64 * LDG;            // [64][LDA]  activated input tile
  float* Wt = As + 64 * LDA;            // [K][LDW]   W^T (cin-major, cout contiguous)
  float* Cs = Wt + K * LDW;             // [7][N] output-side constants, [3][K] input table
  float* Ts = sm;                       // [N][K]     cross-wave dW sum; reuses the tile space after the loop
  {
    const long long sl = blockIdx.y;
    g += sl * sb.grad; z += sl * sb.act; x += sl * sb.act; gx += sl * sb.grad;
    save += sl * sb.save; consts += sl * sb.consts;
    if (RED) { if (red_in) red_in += sl * sb.red; if (red_in2) red_in2 += sl * sb.red; }
    if (gadd) gadd += sl * sb.grad;
    if constexpr (RED2) { red2_z += sl * sb.act; red2_sc += sl * sb.tab; red2_sh += sl * sb.tab; }
    ot.sc += sl * sb.tab; ot.sh += sl * sb.tab;
    it.sc += sl * sb.tab; it.sh += sl * sb.tab; it.fl += sl * sb.tab;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, gq = lane >> 4;
  for (int i = tid; i < N * K; i += 256) {           // w is [N][K] row-major
    const int n = i / K, k = i - n * K;
    Wt[k * LDW + n] = w[i];
  }
  // per-thread channel quads of the staging loops never change (256 % (N/4) == 0, 256 % (K/4) == 0); the per-channel
  // constants live in LDS (7 x N + 3 x K floats) rather than in 40 registers: with them in registers the 64x64 layers
  // sat at one wave per SIMD
  const int nq = tid % (N / 4), kq = tid % (K / 4);
  for (int c = tid; c < N; c += 256) {
    Cs[c] = ot.sc[c]; Cs[N + c] = ot.sh[c]; Cs[2 * N + c] = save[2 * c]; Cs[3 * N + c] = save[2 * c + 1];
    Cs[4 * N + c] = consts[3 * c]; Cs[5 * N + c] = consts[3 * c + 1]; Cs[6 * N + c] = consts[3 * c + 2];
  }
  for (int c = tid; c < K; c += 256) { Cs[7 * N + c] = it.sc[c]; Cs[7 * N + K + c] = it.sh[c]; Cs[7 * N + 2 * K + c] = it.fl[c]; }
  if (RED) {
    for (int c = tid; c < 8 * K; c += 256) Cs[7 * N + 3 * K + c] = 0.0f;       // [4 waves][K][2] input-layer BN sums
    if constexpr (RED2)                                                         // table of the BatchNorm behind the shortcut sum
      for (int c = tid; c < K; c += 256) {
        const bool in = c < red_split;
        Cs[7 * N + 11 * K + c] = in ? red2_sc[c] : 1.0f; Cs[7 * N + 12 * K + c] = in ? red2_sh[c] : 0.0f;
      }
  }
  // weight-gradient tiles of this wave: all of them (fp32 form) or one half, split along cin when CTK is even, else cout
  constexpr bool DW_SPLIT = (CTK % 2 == 0) || (CTN % 2 == 0);
  constexpr bool DW_HALF_K = DW_SPLIT && CTK % 2 == 0;
  constexpr int DW_AN = !DW_SPLIT ? CTN : (DW_HALF_K ? CTN : CTN / 2), DW_BN = !DW_SPLIT ? CTK : (DW_HALF_K ? CTK / 2 : CTK);
  const int dw_a0 = (DW_SPLIT && !DW_HALF_K) ? (wave & 1) * DW_AN : 0, dw_b0 = DW_HALF_K ? (wave & 1) * DW_BN : 0;
  f32x4 dw[DW_AN][DW_BN];
#pragma unroll
  for (int a = 0; a < DW_AN; ++a)
#pragma unroll
    for (int b = 0; b < DW_BN; ++b) dw[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const long long n_tiles = (M + 63) / 64;
  f32x4 rg[NGq], rz[NGq], rx[NAq];
  auto fetch = [&](long long m0) {
#pragma unroll
    for (int j = 0; j < NGq; ++j) {
      const int i = tid + 256 * j, r = i / (N / 4);
      rg[j] = f32x4{0.f, 0.f, 0.f, 0.f}; rz[j] = rg[j];
      if (i < 64 * (N / 4) && m0 + r < M) {
        rg[j] = *reinterpret_cast<const f32x4*>(g + (m0 + r) * g_ld + 4 * nq);
        rz[j] = *reinterpret_cast<const f32x4*>(z + (m0 + r) * z_ld + 4 * nq);
      }
    }
#pragma unroll
    for (int j = 0; j < NAq; ++j) {
      const int i = tid + 256 * j, r = i / (K / 4);
      rx[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i < 64 * (K / 4) && m0 + r < M) rx[j] = *reinterpret_cast<const f32x4*>(x + (m0 + r) * x_ld + 4 * kq);
    }
  };
  auto stage = [&](long long m0) {
#pragma unroll
    for (int j = 0; j < NGq; ++j) {
      const int i = tid + 256 * j, r = i / (N / 4);
      if (i < 64 * (N / 4)) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (m0 + r < M) {
          const f32x4 o_sc = *reinterpret_cast<const f32x4*>(Cs + 4 * nq), o_sh = *reinterpret_cast<const f32x4*>(Cs + N + 4 * nq),
                      o_mean = *reinterpret_cast<const f32x4*>(Cs + 2 * N + 4 * nq), o_istd = *reinterpret_cast<const f32x4*>(Cs + 3 * N + 4 * nq),
                      o_c1 = *reinterpret_cast<const f32x4*>(Cs + 4 * N + 4 * nq), o_c2 = *reinterpret_cast<const f32x4*>(Cs + 5 * N + 4 * nq),
                      o_k = *reinterpret_cast<const f32x4*>(Cs + 6 * N + 4 * nq);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float zh = (rz[j][q] - o_mean[q]) * o_istd[q];
            const float gy = rg[j][q] * dsilu_(fmaf(rz[j][q], o_sc[q], o_sh[q]));
            v[q] = o_k[q] * (gy - o_c1[q] - zh * o_c2[q]);
          }
        }
        *reinterpret_cast<f32x4*>(Gs + r * LDG + 4 * nq) = v;
      }
    }
#pragma unroll
    for (int j = 0; j < NAq; ++j) {
      const int i = tid + 256 * j, r = i / (K / 4);
      if (i < 64 * (K / 4)) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (m0 + r < M) {
          if constexpr (RED) v = rx[j];     // raw z: activated where phase 3 reads it (each element once), z itself feeds the RED sums
          else v = tf4(rx[j], *reinterpret_cast<const f32x4*>(Cs + 7 * N + 4 * kq), *reinterpret_cast<const f32x4*>(Cs + 7 * N + K + 4 * kq),
                       *reinterpret_cast<const f32x4*>(Cs + 7 * N + 2 * K + 4 * kq));
        }
        *reinterpret_cast<f32x4*>(As + r * LDA + 4 * kq) = v;
      }
    }
  };

  float p_sc[RED ? CTK : 1], p_sh[RED ? CTK : 1], p_fl[RED ? CTK : 1];      // input table of channels 16 b + lm (phase 3)
  if constexpr (RED) {
#pragma unroll
    for (int b = 0; b < CTK; ++b) { p_sc[b] = it.sc[16 * b + lm]; p_sh[b] = it.sh[16 * b + lm]; p_fl[b] = it.fl[16 * b + lm]; }
  }
  long long tile = blockIdx.x;
  if (tile < n_tiles) fetch(tile * 64);
  for (; tile < n_tiles; tile += gridDim.x) {
    const long long m0 = tile * 64;
    __syncthreads();                                  // previous tile's readers are done (and Wt is in place)
    stage(m0);
    __syncthreads();
    if (tile + gridDim.x < n_tiles) fetch((tile + gridDim.x) * 64);
    // ---- phase 2: g_in[pixel][cin] = sum_cout g_z[pixel][cout] * W[cout][cin]; D = W^T . G^T, wave = 16 pixels
    {
      f32x4 acc[CTK];
#pragma unroll
      for (int b = 0; b < CTK; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
      // RED2: the raw output of the conv behind the shortcut sum, in the layout of the accumulators (this lane's pixel,
      // channels 16 b + 4 gq), requested BEFORE the matrix loop that hides its latency
      f32x4 z2v[RED2 ? CTK : 1];
      if constexpr (RED2) {
        const long long mz = m0 + wave * 16 + lm;
#pragma unroll
        for (int b = 0; b < CTK; ++b) {
          z2v[b] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (16 * b < red_split && mz < M) z2v[b] = *reinterpret_cast<const f32x4*>(red2_z + mz * red2_ld + 16 * b + 4 * gq);
        }
      }
      const float* grow = Gs + (wave * 16 + lm) * LDG + 4 * gq;
      const float* wrow = Wt + lm * LDW + 4 * gq;
#pragma unroll
      for (int kk = 0; kk < N; kk += 16) {
        const f32x4 gb = *reinterpret_cast<const f32x4*>(grow + kk);
#pragma unroll
        for (int b = 0; b < CTK; ++b) {
          const f32x4 wa = *reinterpret_cast<const f32x4*>(wrow + b * 16 * LDW + kk);
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[j], gb[j], acc[b], 0, 0, 0);
        }
      }
      const long long m = m0 + wave * 16 + lm;
      if (m < M) {
#pragma unroll
        for (int b = 0; b < CTK; ++b) {
          float* op = gx + m * gx_ld + 16 * b + 4 * gq;
          f32x4 v = acc[b];
          // shortcut of a bottleneck: the gradient of the sum joins here (the shortcut add's own backward pass is gone)
          if (gadd) v += *reinterpret_cast<const f32x4*>(gadd + m * gadd_ld + 16 * b + 4 * gq);
          if (accumulate) v += *reinterpret_cast<const f32x4*>(op);
          *reinterpret_cast<f32x4*>(op) = v;
          acc[b] = v;                                  // RED below sums the FINAL gradient of the input
        }
      }
      if constexpr (RED) {
        // this wave's 16 pixels: row sums by DPP, accumulated in the wave's own LDS slots (plain read-modify-write by
        // the row leaders) -- per-lane sums held in registers across the tiles cost a wave of occupancy
        float* rslot = Cs + 7 * N + 3 * K + wave * 2 * K;
#pragma unroll
        for (int b = 0; b < CTK; ++b) {
          const int ch = 16 * b + 4 * gq;
          f32x4 zv = *reinterpret_cast<const f32x4*>(As + (wave * 16 + lm) * LDA + ch);      // raw z of this pixel
          f32x4 i_sc = *reinterpret_cast<const f32x4*>(Cs + 7 * N + ch), i_sh = *reinterpret_cast<const f32x4*>(Cs + 7 * N + K + ch);
          if constexpr (RED2) if (16 * b < red_split) {  // (uniform) the sums of this run go to the conv behind the shortcut sum
            zv = z2v[b];
            i_sc = *reinterpret_cast<const f32x4*>(Cs + 7 * N + 11 * K + ch); i_sh = *reinterpret_cast<const f32x4*>(Cs + 7 * N + 12 * K + ch);
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float yv = fmaf(zv[q], i_sc[q], i_sh[q]);
            const float gy = m < M ? acc[b][q] * dsilu_(yv) : 0.0f;
            const float a1 = row16_sum(gy);
            // second moment against the NORMALISED value y = gamma * zhat + beta (bn_bwd_consts turns it into sum gy * zhat):
            // the raw moment sum gy * z cancels against mean * sum gy there, and its fp32 rounding comes back amplified by
            // |mean| / std of the producer's output — 1e2 .. 1e3 on the near-constant maps of a fresh network
            const float a2 = row16_sum(gy * yv);
            if (lm == 0) { rslot[2 * (ch + q)] += a1; rslot[2 * (ch + q) + 1] += a2; }
          }
        }
      }
    }
    // ---- phase 3: dW[cout][cin] += sum_pixel g_z[pixel][cout] * a[pixel][cin]
    if constexpr (DW_SPLIT) {
      // split-bf16 products (a weight gradient is a leaf, see pw_bwd_weight_wide_kernel): one 32-pixel k-step per wave —
      // waves 0, 1 take pixels 0..31, waves 2, 3 pixels 32..63 — and half of the output tiles each, so a wave holds
      // HALF the accumulators of the fp32 form.  Lane group gq, element e -> pixel 4 gq + (e & 3) + 16 (e >> 2).
      const int prow = 32 * (wave >> 1) + 4 * gq;
      bf16x8 bh[DW_BN], bl[DW_BN];
#pragma unroll
      for (int b = 0; b < DW_BN; ++b)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float v = As[(prow + (e & 3) + 16 * (e >> 2)) * LDA + 16 * (dw_b0 + b) + lm];
          if constexpr (RED) v = p_fl[dw_b0 + b] != 0.0f ? silu(fmaf(v, p_sc[dw_b0 + b], p_sh[dw_b0 + b])) : v;
          split2(v, bh[b], bl[b], e);
        }
#pragma unroll
      for (int a = 0; a < DW_AN; ++a) {
        bf16x8 ah, al;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float v = Gs[(prow + (e & 3) + 16 * (e >> 2)) * LDG + 16 * (dw_a0 + a) + lm];
          split2(v, ah, al, e);
        }
#pragma unroll
        for (int b = 0; b < DW_BN; ++b) {
          f32x4 d = dw[a][b];
          d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh[b], d, 0, 0, 0);
          d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl[b], d, 0, 0, 0);
          d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh[b], d, 0, 0, 0);
          dw[a][b] = d;
        }
      }
    } else {
      // fp32 MFMA: wave = 16 pixels = 4 k-steps, every output tile in every wave
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const int row = wave * 16 + 4 * st + gq;
        float av[CTN], bv[CTK];
#pragma unroll
        for (int a = 0; a < CTN; ++a) av[a] = Gs[row * LDG + 16 * a + lm];
#pragma unroll
        for (int b = 0; b < CTK; ++b) {
          bv[b] = As[row * LDA + 16 * b + lm];
          if constexpr (RED) bv[b] = p_fl[b] != 0.0f ? silu(fmaf(bv[b], p_sc[b], p_sh[b])) : bv[b];
        }
#pragma unroll
        for (int a = 0; a < CTN; ++a)
#pragma unroll
          for (int b = 0; b < CTK; ++b) dw[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], dw[a][b], 0, 0, 0);
      }
    }
  }
  if constexpr (RED) {
    // per-channel sums of the input layer's BN backward: the four waves' LDS slots -> fp64 atomics
    __syncthreads();
    // (two channel runs: [0, red_split) -> red_in, [red_split, K) -> red_in2 — the input of a CSP's conv3 is
    //  [bottleneck output | conv2 half of the pair]; either base may be null: that run's producer has no BatchNorm or
    //  another reader)
    const float* rs = Cs + 7 * N + 3 * K;
    if (tid < 2 * K) {
      const bool first = tid < 2 * red_split;
      double* base = first ? red_in : red_in2;
      if (base)
        atomicAdd(&base[(blockIdx.x % JN_NREP) * red_rep_stride + (first ? tid : tid - 2 * red_split)],
                  (double)(rs[tid] + rs[2 * K + tid] + rs[4 * K + tid] + rs[6 * K + tid]));
    }
  }
  // cross-wave sum of dW (plain LDS read-modify-write, one round per wave that shares tiles), then one set of atomics
  if constexpr (DW_SPLIT) {
    for (int ph = 0; ph < 2; ++ph) {                 // waves (0, 1) hold disjoint tiles, (2, 3) the same two sets
      __syncthreads();
      if ((wave >> 1) == ph) {
#pragma unroll
        for (int a = 0; a < DW_AN; ++a)
#pragma unroll
          for (int b = 0; b < DW_BN; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float* tp = &Ts[(16 * (dw_a0 + a) + 4 * gq + r) * K + 16 * (dw_b0 + b) + lm];
              *tp = (ph == 0 ? 0.0f : *tp) + dw[a][b][r];
            }
      }
    }
  } else {
    for (int wv = 0; wv < 4; ++wv) {
      __syncthreads();
      if (wave == wv) {
#pragma unroll
        for (int a = 0; a < DW_AN; ++a)
#pragma unroll
          for (int b = 0; b < DW_BN; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float* tp = &Ts[(16 * a + 4 * gq + r) * K + 16 * b + lm];
              *tp = (wv == 0 ? 0.0f : *tp) + dw[a][b][r];
            }
      }
    }
  }
  __syncthreads();
  float* dst = rep ? gw + ((blockIdx.x + 5 * blockIdx.y) % JN_NREP) * JN_WPART_MAX : gw;
  for (int i = tid; i < N * K; i += 256) atomicAdd(&dst[i], Ts[i]);
}

template <int CTN, int CTK, bool RED, bool RED2 = false>
static int launch_pw_bwd_fused_r(const PwBwdFusedArgs& a, hipStream_t s) {
  constexpr int N = 16 * CTN, K = 16 * CTK;
  constexpr size_t tiles = ((size_t)64 * (N + 4) + 64 * (K + 4) + (size_t)K * (N + 4) + 7 * N + 3 * K + (RED ? (RED2 ? 10 : 8) * K : 0)) * sizeof(float);
  constexpr size_t smem = std::max(tiles, (size_t)N * K * sizeof(float));
  if (!allow_lds<&pw_bwd_fused_kernel<CTN, CTK, RED, RED2>>(smem)) return -1;
  const long long n_tiles = (a.M + 63) / 64;
  // ~1024 persistent workgroups over all slots, in WHOLE resident rounds: an instantiation that fits 3 workgroups per CU
  // (768 places) ran 1020 of them, i.e. a second round at a third of the occupancy
  const int places = resident_per_cu<&pw_bwd_fused_kernel<CTN, CTK, RED, RED2>>(smem, 2) * JN_NUM_CU;
  const int rounds = std::max(1, (1024 + places / 2) / places);
  long long bx = (long long)rounds * places / a.sb.n;
  if (a.max_wg > 0 && bx > a.max_wg / a.sb.n) bx = a.max_wg / a.sb.n;
  if (bx < 1) bx = 1;
  if (bx > n_tiles) bx = n_tiles;
  const int rep = (a.wpart && N * K <= JN_WPART_MAX) ? 1 : 0;
  hipLaunchKernelGGL((pw_bwd_fused_kernel<CTN, CTK, RED, RED2>), dim3((unsigned)bx, a.sb.n), dim3(256), smem, s, a.g, a.g_ld, a.z,
                     a.z_ld, a.ot, a.save, a.consts, a.x, a.x_ld, a.it, a.w, a.gx, a.gx_ld, a.accumulate,
                     rep ? a.wpart : a.gw, rep, a.M, a.sb, a.red_in, a.red_rep_stride, a.gadd, a.gadd_ld, a.red_in2,
                     a.red_split > 0 ? a.red_split : K, a.red2_z, a.red2_ld, a.red2_sc, a.red2_sh);
  if (rep) launch_wpart_reduce(a.gw, a.wpart, N * K, s);
  return 0;
}

template <int CTN, int CTK>
static int launch_pw_bwd_fused_t(const PwBwdFusedArgs& a, hipStream_t s) {
  if constexpr (CTK <= 4) {
    if (a.red2_z) return launch_pw_bwd_fused_r<CTN, CTK, true, true>(a, s);
    if (a.red_in || a.red_in2) return launch_pw_bwd_fused_r<CTN, CTK, true>(a, s);
  }
  return launch_pw_bwd_fused_r<CTN, CTK, false>(a, s);
}

// ---- the same pass for 128 input channels, resident twice per CU -----------------------------------
// pw_bwd_fused_kernel<8 | 4, 8> keeps W^T in LDS (68 / 35 KB of its 140 / 89 KB) and 368+ registers: one workgroup per CU,
// one wave per SIMD, nothing to overlap a tile's load / stage / matrix / store phases with.  This form has 32-pixel tiles,
// no W^T in LDS (67 / 55 KB) and at most 256 registers, so two workgroups share a CU:
//  - W^T comes from `wf`, the weight in FRAGMENT ORDER (a pre-pass per launch), one 1 KB contiguous load per wave and
//    fragment, requested D steps ahead.  fp32 form (w_frag_t_kernel): block (b * N / 16 + s) of 64 lanes x 4 floats, lane
//    (gq, lm) holding w[16 s + 4 gq + j][16 b + lm], j = 0..3 — the A operands of the four v_mfma_f32_16x16x4_f32 of
//    k-step s.  X3: the three bf16 planes of w_split3_t_kernel, as pw_x3_kernel<.., SLOTS> streams them.
//  - phase 2: wave = all 32 pixels x a QUARTER of the input channels (2 cin tiles x 2 pixel groups = 16 accumulator
//    registers), so a workgroup requests every fragment once per tile.  fp32 form (64 output channels): the fp32 products
//    in the k order of the 64-pixel kernel, the data gradient is bit-equal to it.  X3 (128 output channels, where the fp32
//    matrix loop was the longest part of a tile): the six-product bf16 form of pw_x3_kernel on three planes of g_z.
//  - phase 3: the tile's 32 pixels are ONE k-step of v_mfma_f32_16x16x32_bf16 (three products as there); wave (cout half,
//    cin half) owns a disjoint quarter of dW across the whole loop — no cross-wave sum, each wave adds its own tiles.
//  - ONE resident round of workgroups, each a contiguous run of the tiles of all slots (a slot crossing reloads the
//    per-channel constants); the store's gadd / accumulate operands and then the next tile's (g, z, x) are requested after
//    the tile's LAST fragment: loads return in order, so a fragment requested behind them would wait for HBM, and the
//    store waits for its operands only, not for the next tile.

// a uniform global pointer pinned to scalar registers (the empty asm hides its origin from the optimiser; the address
// space is given back by the cast), and a 16-byte load at scalar base + 32-bit offset
using gfloat_p = const __attribute__((address_space(1))) float*;
__device__ __forceinline__ gfloat_p pin_uniform(const float* p) {
  asm volatile("" : "+s"(p));
  return (gfloat_p)p;
}
__device__ __forceinline__ f32x4 ldg4(gfloat_p base, unsigned off) {
  return *(const __attribute__((address_space(1))) f32x4*)(base + off);
}

__global__ __launch_bounds__(256) void w_frag_t_kernel(const float* __restrict__ w, float* __restrict__ wf, int N, int K) {
  const int i = blockIdx.x * 256 + threadIdx.x;        // (cin tile b, k-step s, lane)
  if (i >= N * K / 4) return;
  const int lane = i & 63, lm = lane & 15, gq = lane >> 4, NS = N / 16, s = (i >> 6) % NS, b = (i >> 6) / NS;
  f32x4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = w[(long long)(16 * s + 4 * gq + j) * K + 16 * b + lm];
  *reinterpret_cast<f32x4*>(wf + 4LL * i) = v;
}

template <int CTN, int D, bool X3>
__global__ __launch_bounds__(256, 2) void pw_bwd_fused128_kernel(
    const float* __restrict__ g, int g_ld, const float* __restrict__ z, int z_ld, ChanTab ot,
    const float* __restrict__ save, const float* __restrict__ consts, const float* __restrict__ x, int x_ld,
    ChanTab it, const float* __restrict__ wf, float* __restrict__ gx, int gx_ld, int accumulate,
    float* __restrict__ gw, int rep, long long M, SlotBatch sb, const float* __restrict__ gadd, int gadd_ld) {
  constexpr int N = 16 * CTN, K = 128, NS = N / 16;  // output / input channels, k-steps of phase 2
  constexpr int LDG = N + 4, LDA = K + 4;
  constexpr int NG = 32 * (N / 4) / 256, NA = 32 * (K / 4) / 256;     // f32x4 per thread per tile
  constexpr int NJ = N / 32, LDK = N + 16;           // X3: k-steps of phase 2, row stride of the bf16 planes (pw_x3_kernel)
  static_assert(NG >= 1 && D >= 1 && D < (X3 ? 2 * NJ : NS), "pw_bwd_fused128 tile mapping");
  // fp32 form: two tile buffers — a tile is staged while slower waves still read the previous one, ONE barrier per tile.
  // X3: one buffer and the three bf16 planes of g_z beside it.
  constexpr int TILE = 32 * LDG + 32 * LDA, NBUF = X3 ? 1 : 2;
  __shared__ __attribute__((aligned(16))) float sm[NBUF * TILE + 7 * N + 3 * K + (X3 ? 3 * 32 * LDK / 2 : 0)];
  float* Gs = sm;                       // [32][LDG]  g_z tile
  float* As = Gs + 32 * LDG;            // [32][LDA]  activated input tile
  float* const Cs = sm + NBUF * TILE;   // [7][N] output-side constants, [3][K] input table (of the slot being staged)
  bf16_t* const Gp = reinterpret_cast<bf16_t*>(Cs + 7 * N + 3 * K);     // X3: [3][32][LDK] h, m, l planes of the g_z tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, gq = lane >> 4;
  const int nq = tid % (N / 4), kq = tid % (K / 4);
  const long long tiles_per_slot = (M + 31) / 32, n_tiles = tiles_per_slot * sb.n;
  const long long t_begin = n_tiles * blockIdx.x / gridDim.x, t_end = n_tiles * (blockIdx.x + 1) / gridDim.x;
  if (t_begin >= t_end) return;

  // weight-gradient tiles of this wave: cout tiles dw_a0 .. + CTN / 2, cin tiles dw_b0 .. + 4
  constexpr int DW_AN = CTN / 2, DW_BN = 4;
  const int dw_a0 = (wave & 1) * DW_AN, dw_b0 = (wave >> 1) * DW_BN;
  f32x4 dw[DW_AN][DW_BN];
#pragma unroll
  for (int a = 0; a < DW_AN; ++a)
#pragma unroll
    for (int b = 0; b < DW_BN; ++b) dw[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  f32x4 rg[NG], rz[NG], rx[NA];
  long long f_slot = 0, f_m0 = 0;                   // slot and first pixel of the fetched tile
  auto fetch = [&](bool next) {                     // the tile behind the fetched one, or that one again
    if (next) {
      f_m0 += 32;
      if (f_m0 >= M) { f_m0 = 0; ++f_slot; }
    }
    // tile bases are uniform and the offsets inside a tile fit 32 bits: scalar base + one offset register per load.
    // Rows past the map re-read its last row; stage() writes zeros there.
    const gfloat_p gs = pin_uniform(g + f_slot * sb.grad + f_m0 * g_ld), zs = pin_uniform(z + f_slot * sb.act + f_m0 * z_ld),
                   xs = pin_uniform(x + f_slot * sb.act + f_m0 * x_ld);
    const int last = (int)(M - f_m0 < 32 ? M - f_m0 : 32) - 1;
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      const int r = std::min((tid + 256 * j) / (N / 4), last);
      rg[j] = ldg4(gs, r * g_ld + 4 * nq);
      rz[j] = ldg4(zs, r * z_ld + 4 * nq);
    }
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int r = std::min((tid + 256 * j) / (K / 4), last);
      rx[j] = ldg4(xs, r * x_ld + 4 * kq);
    }
  };
  // the store's operand of tile (slot, m0) in accumulator layout (pixel 16 p + lm, channels 16 (2 wave + c) + 4 gq): gadd,
  // or the gradient already in gx; with BOTH (no layer of the plan has them) the second one is read at the store
  f32x4 eo[2][2];
  auto fetch_store_operand = [&](long long slot, long long m0) {
    const gfloat_p src = pin_uniform(gadd ? gadd + slot * sb.grad + m0 * gadd_ld : gx + slot * sb.grad + m0 * gx_ld);
    const int src_ld = gadd ? gadd_ld : gx_ld;
    const int last = (int)(M - m0 < 32 ? M - m0 : 32) - 1;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int p = 0; p < 2; ++p)
        eo[c][p] = ldg4(src, std::min(16 * p + lm, last) * src_ld + 16 * (2 * wave + c) + 4 * gq);
  };
  auto load_consts = [&](long long sl) {
    // (pinned bases: hoisted out of the tile loop, the seven per-lane addresses cost 14 registers for a rare path)
    const gfloat_p o_sc = pin_uniform(ot.sc + sl * sb.tab), o_sh = pin_uniform(ot.sh + sl * sb.tab), sv = pin_uniform(save + sl * sb.save),
                   cn = pin_uniform(consts + sl * sb.consts);
    for (int c = tid; c < N; c += 256) {
      Cs[c] = o_sc[c]; Cs[N + c] = o_sh[c]; Cs[2 * N + c] = sv[2 * c]; Cs[3 * N + c] = sv[2 * c + 1];
      Cs[4 * N + c] = cn[3 * c]; Cs[5 * N + c] = cn[3 * c + 1]; Cs[6 * N + c] = cn[3 * c + 2];
    }
    const gfloat_p i_sc = pin_uniform(it.sc + sl * sb.tab), i_sh = pin_uniform(it.sh + sl * sb.tab), i_fl = pin_uniform(it.fl + sl * sb.tab);
    for (int c = tid; c < K; c += 256) { Cs[7 * N + c] = i_sc[c]; Cs[7 * N + K + c] = i_sh[c]; Cs[7 * N + 2 * K + c] = i_fl[c]; }
  };
  auto stage = [&](long long m0) {
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      const int r = (tid + 256 * j) / (N / 4);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (m0 + r < M) {
        const f32x4 o_sc = *reinterpret_cast<const f32x4*>(Cs + 4 * nq), o_sh = *reinterpret_cast<const f32x4*>(Cs + N + 4 * nq),
                    o_mean = *reinterpret_cast<const f32x4*>(Cs + 2 * N + 4 * nq), o_istd = *reinterpret_cast<const f32x4*>(Cs + 3 * N + 4 * nq),
                    o_c1 = *reinterpret_cast<const f32x4*>(Cs + 4 * N + 4 * nq), o_c2 = *reinterpret_cast<const f32x4*>(Cs + 5 * N + 4 * nq),
                    o_k = *reinterpret_cast<const f32x4*>(Cs + 6 * N + 4 * nq);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float zh = (rz[j][q] - o_mean[q]) * o_istd[q];
          const float gy = rg[j][q] * dsilu_(fmaf(rz[j][q], o_sc[q], o_sh[q]));
          v[q] = o_k[q] * (gy - o_c1[q] - zh * o_c2[q]);
        }
      }
      *reinterpret_cast<f32x4*>(Gs + r * LDG + 4 * nq) = v;
      if constexpr (X3) {
        // split3_store of jn_split.h written out, l converted where it is stored: with the helper the compiler schedules this
        // kernel differently and it measured 0.7 - 1.3 % slower (profiles/conv3_unit_ab.txt)
        const bf16x4 vh = __builtin_convertvector(v, bf16x4);
        const f32x4 r1 = v - __builtin_convertvector(vh, f32x4);
        const bf16x4 vm = __builtin_convertvector(r1, bf16x4);
        const f32x4 r2 = r1 - __builtin_convertvector(vm, f32x4);
        bf16_t* dst = Gp + r * LDK + 4 * nq;
        *reinterpret_cast<bf16x4*>(dst) = vh;
        *reinterpret_cast<bf16x4*>(dst + 32 * LDK) = vm;
        *reinterpret_cast<bf16x4*>(dst + 2 * 32 * LDK) = __builtin_convertvector(r2, bf16x4);
      }
    }
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int r = (tid + 256 * j) / (K / 4);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (m0 + r < M)
        v = tf4(rx[j], *reinterpret_cast<const f32x4*>(Cs + 7 * N + 4 * kq), *reinterpret_cast<const f32x4*>(Cs + 7 * N + K + 4 * kq),
                *reinterpret_cast<const f32x4*>(Cs + 7 * N + 2 * K + 4 * kq));
      *reinterpret_cast<f32x4*>(As + r * LDA + 4 * kq) = v;
    }
  };

  // fragment (cin tile 2 wave + c, k-step s)
  gfloat_p wbase = pin_uniform(wf);                  // re-pinned per tile: the loads must stay inside the tile loop (hoisted,
  const unsigned woff = (2 * wave * NS * 64 + lane) * 4;      // the wave's 2 NS fragments would sit in registers for good)
  auto wfrag = [&](int c, int s) -> f32x4 { return ldg4(wbase, woff + (c * NS + s) * 256); };
  // X3: plane t of fragment (cin tile 2 wave + c, k-step j) in the order of w_split3_t_kernel (offsets in floats)
  auto wfrag3 = [&](int c, int j, int t) -> bf16x8 {
    return __builtin_bit_cast(bf16x8, ldg4(wbase, (((2 * wave + c) * NJ + j) * 3 + t) * 256 + lane * 4));
  };

  long long cur_slot = -1;
  f_slot = t_begin / tiles_per_slot;
  f_m0 = (t_begin - f_slot * tiles_per_slot) * 32;
  fetch(false);
#pragma unroll 1
  for (long long tile = t_begin; tile < t_end; ++tile) {
    const long long slot = f_slot, m0 = f_m0;
    // the first fragments, requested before the staging that hides their way from L2 (behind the fetched tile in the
    // queue, so the staging's wait for that tile leaves them in flight)
    f32x4 wa[X3 ? 1 : NS][2];
    bf16x8 wx[X3 ? 2 * NJ : 1][3];                    // X3: unit u = (k-step u / 2, cin tile u % 2), requested D units ahead
    wbase = pin_uniform(wf);
#pragma unroll
    for (int s = 0; s < D; ++s) {
      if constexpr (X3) {
#pragma unroll
        for (int t = 0; t < 3; ++t) wx[s][t] = wfrag3(s & 1, s >> 1, t);
      } else {
#pragma unroll
        for (int c = 0; c < 2; ++c) wa[s][c] = wfrag(c, s);
      }
    }
    if constexpr (NBUF == 1) __syncthreads();         // previous tile's readers are done
    if (slot != cur_slot) {                           // (uniform; every wave is past the staging of the previous tile)
      load_consts(slot);
      cur_slot = slot;
      __syncthreads();
    }
    if constexpr (NBUF == 2) {
      Gs = sm + ((tile - t_begin) & 1) * TILE;
      As = Gs + 32 * LDG;
    }
    stage(m0);
    __syncthreads();                                  // (the readers of THIS buffer, two tiles back, passed the barrier between)
    // ---- phase 2: g_in[pixel][cin] = sum_cout g_z[pixel][cout] * W[cout][cin]; D = W^T . G^T
    f32x4 acc[2][2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int p = 0; p < 2; ++p) acc[c][p] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto late_loads = [&]() {                         // behind the tile's last fragment: the store's operand, the next tile
      if (gadd || accumulate) fetch_store_operand(slot, m0);
      fetch(tile + 1 < t_end);                        // (unconditional: behind a branch the loaded registers are copied at the join, which waits for them)
    };
    if constexpr (X3) {
      // the six-product bf16 form of pw_x3_kernel, (w, g) planes in the order of jn_split.h
      const bf16_t* xrow = Gp + lm * LDK + 8 * gq;
#pragma unroll
      for (int u = 0; u < 2 * NJ; ++u) {
        const int j = u >> 1, c = u & 1;
        if (u + D < 2 * NJ) {
#pragma unroll
          for (int t = 0; t < 3; ++t) wx[u + D][t] = wfrag3((u + D) & 1, (u + D) >> 1, t);
        }
        if (u + D == 2 * NJ - 1) late_loads();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int p = 0; p < 2; ++p) {                 // (the planes are read again for the second cin tile: 12 registers less)
          bf16x8 xa[3];
#pragma unroll
          for (int t = 0; t < 3; ++t) xa[t] = *reinterpret_cast<const bf16x8*>(xrow + t * 32 * LDK + p * 16 * LDK + 32 * j);
#pragma unroll
          for (int e = 0; e < X3_PRODUCTS; ++e) acc[c][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wx[u][X3_W[e]], xa[X3_X[e]], acc[c][p], 0, 0, 0);
        }
      }
    } else {
      const float* grow = Gs + lm * LDG + 4 * gq;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (s + D < NS) {
#pragma unroll
          for (int c = 0; c < 2; ++c) wa[s + D][c] = wfrag(c, s + D);
        }
        if (s + D == NS - 1) late_loads();
        __builtin_amdgcn_sched_barrier(0);
        f32x4 gb[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) gb[p] = *reinterpret_cast<const f32x4*>(grow + p * 16 * LDG + 16 * s);
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[c][p] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[s][c][j], gb[p][j], acc[c][p], 0, 0, 0);
      }
    }
    {
      float* gxs = gx + slot * sb.grad + m0 * gx_ld;
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int p = 0; p < 2; ++p)
          if (m0 + 16 * p + lm < M) {
            float* op = gxs + (unsigned)((16 * p + lm) * gx_ld + 16 * (2 * wave + c) + 4 * gq);
            // shortcut of a bottleneck: the gradient of the sum joins here, then the gradient already there
            f32x4 v = acc[c][p];
            if (gadd || accumulate) v += eo[c][p];
            if (gadd && accumulate) v += *reinterpret_cast<const f32x4*>(op);
            *reinterpret_cast<f32x4*>(op) = v;
          }
    }
    // ---- phase 3: dW[cout][cin] += sum_pixel g_z[pixel][cout] * a[pixel][cin], split-bf16 products (a weight gradient
    // is a leaf, see pw_bwd_weight_wide_kernel).  Lane group gq, element e -> pixel 4 gq + (e & 3) + 16 (e >> 2).
    {
      const int prow = 4 * gq;
      bf16x8 bh[DW_BN], bl[DW_BN];
#pragma unroll
      for (int b = 0; b < DW_BN; ++b)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float v = As[(prow + (e & 3) + 16 * (e >> 2)) * LDA + 16 * (dw_b0 + b) + lm];
          split2(v, bh[b], bl[b], e);
        }
#pragma unroll
      for (int a = 0; a < DW_AN; ++a) {
        bf16x8 ah, al;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float v = Gs[(prow + (e & 3) + 16 * (e >> 2)) * LDG + 16 * (dw_a0 + a) + lm];
          split2(v, ah, al, e);
        }
#pragma unroll
        for (int b = 0; b < DW_BN; ++b) {
          f32x4 d = dw[a][b];
          d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh[b], d, 0, 0, 0);
          d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl[b], d, 0, 0, 0);
          d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh[b], d, 0, 0, 0);
          dw[a][b] = d;
        }
      }
    }
  }
  float* dst = rep ? gw + (blockIdx.x % JN_NREP) * JN_WPART_MAX : gw;
#pragma unroll
  for (int a = 0; a < DW_AN; ++a)
#pragma unroll
    for (int b = 0; b < DW_BN; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) atomicAdd(&dst[(16 * (dw_a0 + a) + 4 * gq + r) * K + 16 * (dw_b0 + b) + lm], dw[a][b][r]);
}

template <int CTN, int D, bool X3>
static void launch_pw_bwd_fused128(const PwBwdFusedArgs& a, hipStream_t s) {
  constexpr int N = 16 * CTN, K = 128;
  if (X3) launch_w_split3_t(a.w, a.w_frag, N, K, s);
  else hipLaunchKernelGGL(w_frag_t_kernel, dim3(N * K / 4 / 256), dim3(256), 0, s, a.w, a.w_frag, N, K);
  const int places = resident_per_cu<&pw_bwd_fused128_kernel<CTN, D, X3>>(0, 2) * JN_NUM_CU;      // ONE resident round
  const long long n_tiles = (a.M + 31) / 32 * a.sb.n;
  long long bx = std::min<long long>(places, n_tiles);
  if (a.max_wg > 0) bx = std::min<long long>(bx, a.max_wg);
  const int rep = (a.wpart && N * K <= JN_WPART_MAX) ? 1 : 0;
  hipLaunchKernelGGL((pw_bwd_fused128_kernel<CTN, D, X3>), dim3((unsigned)bx), dim3(256), 0, s, a.g, a.g_ld, a.z, a.z_ld, a.ot, a.save,
                     a.consts, a.x, a.x_ld, a.it, a.w_frag, a.gx, a.gx_ld, a.accumulate, rep ? a.wpart : a.gw, rep, a.M, a.sb,
                     a.gadd, a.gadd_ld);
  if (rep) launch_wpart_reduce(a.gw, a.wpart, N * K, s);
}

// shapes and operands pw_bwd_fused128_kernel takes (cin = 128 never reduces its input: pw_bwd_fused_reduces_input)
static bool pw_bwd_fused128_takes(const PwBwdFusedArgs& a) {
  return a.w_frag && a.route != 1 && a.cin == 128 && (a.cout == 128 || a.cout == 64) && !a.red_in && !a.red_in2 && !a.red2_z &&
         a.g_ld % 4 == 0 && a.z_ld % 4 == 0 && a.x_ld % 4 == 0 && a.gx_ld % 4 == 0 && (!a.gadd || a.gadd_ld % 4 == 0) &&
         reinterpret_cast<uintptr_t>(a.w_frag) % 16 == 0;
}

bool pw_bwd_fused_reduces_input(int cout, int cin) { return pw_bwd_fused_supported(cout, cin) && cin <= 64; }   // (cin = 128 measured: the epilogue of the one-workgroup-per-CU kernels costs more than the 28x28 passes it saves, profiles/r04_ab_red128.txt)

bool pw_bwd_fused_supported(int cout, int cin) {
  if (cout % 16 || cin % 16) return false;
  const int tn = cout / 16, tk = cin / 16;
  auto pow2 = [](int v) { return v == 1 || v == 2 || v == 4 || v == 8; };
  return pow2(tn) && pow2(tk);     // up to 128 x 128 (that one since round 3: one workgroup per CU)
}

int launch_pw_bwd_fused(const PwBwdFusedArgs& a, hipStream_t s) {
  const int tn = a.cout / 16, tk = a.cin / 16;
  if (pw_bwd_fused128_takes(a)) {
    if (tn == 8) launch_pw_bwd_fused128<8, 2, true>(a, s); else launch_pw_bwd_fused128<4, 2, false>(a, s);
    return 0;
  }
#define JN_PF(A, B) if (tn == A && tk == B) return launch_pw_bwd_fused_t<A, B>(a, s);
  JN_PF(1, 1) JN_PF(1, 2) JN_PF(1, 4) JN_PF(1, 8) JN_PF(2, 1) JN_PF(2, 2) JN_PF(2, 4) JN_PF(2, 8)
  JN_PF(4, 1) JN_PF(4, 2) JN_PF(4, 4) JN_PF(4, 8) JN_PF(8, 1) JN_PF(8, 2) JN_PF(8, 4) JN_PF(8, 8)
#undef JN_PF
  return -1;
}

}  // namespace jnr
