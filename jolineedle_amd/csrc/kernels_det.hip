// Detector kernels (yolox-s style): the YOLOX head's prediction convs fused with the box decode, the class-agnostic
// postprocess (threshold, sort, NMS; capped and uncapped) and the scatter of a patch's boxes into the rollout's arrays.
// The dense 3x3 convs under the head are in kernels_conv3.hip.
// Restated from the published YOLOX head / postprocess (reference call sites
// src/models/yolox.py:55, 77-86, 93-113).
#include <hip/hip_runtime.h>

#include "jn_kernels.h"
#include "jn_tab.h"
#include "jn_types.h"

namespace jnr {

// ------------------------------------------------------------------------------------
// YOLOXHead predictors of one level + decode: raw[n][a0 + p][0..5] =
//   ((reg_xy + grid) * stride, exp(reg_wh) * stride, sigmoid(obj), sigmoid(cls))
// wp = [6][hid]: rows 0-3 reg_pred, 4 obj_pred (both read reg_feat), 5 cls_pred (reads cls_feat); bp[6].
// ------------------------------------------------------------------------------------
template <typename AT>
__global__ __launch_bounds__(256) void head_pred_kernel(const AT* __restrict__ reg, int reg_ld, ChanTab rt,
                                                        const AT* __restrict__ cls, int cls_ld, ChanTab ct,
                                                        const float* __restrict__ wp, const float* __restrict__ bp,
                                                        float* __restrict__ raw, int hid, int Hl, int Wl, int stride,
                                                        int A, int a0, int N, int logits_only) {
  extern __shared__ float sw[];     // [6][hid] + tables
  for (int i = threadIdx.x; i < 6 * hid; i += 256) sw[i] = wp[i];
  __syncthreads();
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)N * Hl * Wl) return;
  const int p = (int)(idx % (Hl * Wl));
  const long long n = idx / (Hl * Wl);
  const AT* rp = reg + idx * reg_ld;
  const AT* cp = cls + idx * cls_ld;
  float o[6] = {bp[0], bp[1], bp[2], bp[3], bp[4], bp[8]};     // bias layout: reg 0..3 | obj 4 (+pad) | cls 8 (+pad)
  for (int k = 0; k < hid; k += 4) {
    const f32x4 rv = tf4(ld4(rp + k), *reinterpret_cast<const f32x4*>(rt.sc + k),
                         *reinterpret_cast<const f32x4*>(rt.sh + k), *reinterpret_cast<const f32x4*>(rt.fl + k));
    const f32x4 cv = tf4(ld4(cp + k), *reinterpret_cast<const f32x4*>(ct.sc + k),
                         *reinterpret_cast<const f32x4*>(ct.sh + k), *reinterpret_cast<const f32x4*>(ct.fl + k));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int j = 0; j < 5; ++j) o[j] = fmaf(rv[q], sw[j * hid + k + q], o[j]);
      o[5] = fmaf(cv[q], sw[5 * hid + k + q], o[5]);
    }
  }
  const int gy = p / Wl, gx = p % Wl;
  float* dst = raw + (n * A + a0 + p) * 6;
  if (logits_only) {                 // training: raw predictor outputs, the loss kernel decodes
#pragma unroll
    for (int j = 0; j < 6; ++j) dst[j] = o[j];
    return;
  }
  dst[0] = (o[0] + (float)gx) * (float)stride;
  dst[1] = (o[1] + (float)gy) * (float)stride;
  dst[2] = expf(o[2]) * (float)stride;
  dst[3] = expf(o[3]) * (float)stride;
  dst[4] = 1.0f / (1.0f + expf(-o[4]));
  dst[5] = 1.0f / (1.0f + expf(-o[5]));
}

int launch_head_pred(const void* reg, int reg_ld, ChanTab rt, const void* cls, int cls_ld, ChanTab ct, int dtype,
                     const float* wp, const float* bp, float* raw, int hid, int Hl, int Wl, int stride, int A, int a0,
                     int N, hipStream_t s, int logits_only) {
  const long long total = (long long)N * Hl * Wl;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (dtype == JN_BF16)
    hipLaunchKernelGGL(head_pred_kernel<bf16_t>, grid, dim3(256), (size_t)6 * hid * sizeof(float), s, (const bf16_t*)reg,
                       reg_ld, rt, (const bf16_t*)cls, cls_ld, ct, wp, bp, raw, hid, Hl, Wl, stride, A, a0, N, logits_only);
  else
    hipLaunchKernelGGL(head_pred_kernel<float>, grid, dim3(256), (size_t)6 * hid * sizeof(float), s, (const float*)reg,
                       reg_ld, rt, (const float*)cls, cls_ld, ct, wp, bp, raw, hid, Hl, Wl, stride, A, a0, N, logits_only);
  return 0;
}

// ------------------------------------------------------------------------------------
// postprocess (class-agnostic, one class): cxcywh -> xyxy, keep obj*cls >= conf, sort by score
// (descending, ties by anchor index), greedy NMS (IoU > thr suppressed), clamp to [0, P-1].
// One workgroup per patch; candidates live in LDS (cap DET_CAP, lowest anchor indices kept).
// stats (nullable) [N][2]: anchors with score >= conf before the DET_CAP cut, NMS survivors before the max_out cut.
// ------------------------------------------------------------------------------------
constexpr int DET_CAP = 2048;

__global__ __launch_bounds__(256) void postprocess_kernel(const float* __restrict__ raw, int A, float conf, float nms_thr,
                                                          float clamp_max, float* __restrict__ boxes,
                                                          int* __restrict__ counts, int max_out,
                                                          int* __restrict__ stats) {
  __shared__ float sc[DET_CAP];
  __shared__ int id[DET_CAP];
  __shared__ unsigned char dead[DET_CAP];
  __shared__ int s_n, s_keep, s_pass;
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* r = raw + (long long)n * A * 6;
  if (tid == 0) { s_n = 0; s_keep = 0; s_pass = 0; }
  __syncthreads();
  // ordered compaction, chunk by chunk so that lower anchor indices win the cap
  for (int base = 0; base < A; base += 256) {
    const int a = base + tid;
    float score = -1.0f;
    if (a < A) score = r[a * 6 + 4] * r[a * 6 + 5];
    const bool ok = a < A && score >= conf;
    const unsigned long long m = __ballot(ok);
    __shared__ int wave_cnt[4];
    const int lane = tid & 63, wv = tid >> 6;
    if (lane == 0) wave_cnt[wv] = __popcll(m);
    __syncthreads();
    int off = s_n;
    for (int w2 = 0; w2 < wv; ++w2) off += wave_cnt[w2];
    off += __popcll(m & ((1ull << lane) - 1ull));
    if (ok && off < DET_CAP) { sc[off] = score; id[off] = a; }
    __syncthreads();
    if (tid == 0) {
      const int passed = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
      s_n = min(DET_CAP, s_n + passed);
      s_pass += passed;
    }
    __syncthreads();
  }
  const int cnt = s_n;
  // bitonic sort on (score desc, index asc)
  int np2 = 1;
  while (np2 < cnt) np2 <<= 1;
  for (int i = cnt + tid; i < np2; i += 256) { sc[i] = -INFINITY; id[i] = 0x7fffffff; }
  __syncthreads();
  for (int k = 2; k <= np2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < np2; i += 256) {
        const int l = i ^ j;
        if (l > i) {
          const bool up = (i & k) == 0;
          const bool before = sc[i] > sc[l] || (sc[i] == sc[l] && id[i] < id[l]);   // i should precede l
          if (up ? !before : before) {
            const float ts = sc[i]; sc[i] = sc[l]; sc[l] = ts;
            const int ti = id[i]; id[i] = id[l]; id[l] = ti;
          }
        }
      }
      __syncthreads();
    }
  for (int i = tid; i < cnt; i += 256) dead[i] = 0;
  __syncthreads();
  for (int i = 0; i < cnt; ++i) {
    if (dead[i]) continue;                          // uniform: dead[] is shared and synced
    const float* bi = r + id[i] * 6;
    const float ax1 = bi[0] - bi[2] * 0.5f, ay1 = bi[1] - bi[3] * 0.5f, ax2 = bi[0] + bi[2] * 0.5f, ay2 = bi[1] + bi[3] * 0.5f;
    const float aa = (ax2 - ax1) * (ay2 - ay1);
    if (tid == 0) {
      const int kidx = s_keep;
      if (kidx < max_out) {
        float* o = boxes + ((long long)n * max_out + kidx) * 7;
        o[0] = fminf(fmaxf(ax1, 0.0f), clamp_max); o[1] = fminf(fmaxf(ay1, 0.0f), clamp_max);
        o[2] = fminf(fmaxf(ax2, 0.0f), clamp_max); o[3] = fminf(fmaxf(ay2, 0.0f), clamp_max);
        o[4] = bi[4]; o[5] = bi[5]; o[6] = 0.0f;
      }
      s_keep = kidx + 1;
    }
    for (int j = i + 1 + tid; j < cnt; j += 256) {
      if (dead[j]) continue;
      const float* bj = r + id[j] * 6;
      const float bx1 = bj[0] - bj[2] * 0.5f, by1 = bj[1] - bj[3] * 0.5f, bx2 = bj[0] + bj[2] * 0.5f, by2 = bj[1] + bj[3] * 0.5f;
      const float iw = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.0f), ih = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.0f);
      const float inter = iw * ih;
      const float iou = inter / (aa + (bx2 - bx1) * (by2 - by1) - inter);
      if (iou > nms_thr) dead[j] = 1;
    }
    __syncthreads();
  }
  if (tid == 0) {
    counts[n] = min(s_keep, max_out);
    if (stats) { stats[n * 2] = s_pass; stats[n * 2 + 1] = s_keep; }
  }
}

int launch_postprocess(const float* raw, int A, int N, float conf, float nms_thr, float clamp_max, float* boxes,
                       int* counts, int max_out, int* stats, hipStream_t s) {
  hipLaunchKernelGGL(postprocess_kernel, dim3(N), dim3(256), 0, s, raw, A, conf, nms_thr, clamp_max, boxes, counts,
                     max_out, stats);
  return 0;
}

// ------------------------------------------------------------------------------------
// The same stage under the candidate policy "all": every anchor with obj * cls >= conf enters the sort, A <=
// POST_ALL_MAX_A.  One workgroup of 1024 threads per patch, 136,508 B of static LDS (a gfx950 workgroup may declare all
// 160 KiB).
// Sort: key[cnt] = 64-bit (descending-order image of the score, anchor index), sorted ASCENDING, which is (score
// descending, index ascending).  Only the cnt real keys are stored: the bitonic network runs over np2 = the power of two
// at or above cnt with every comparator pointing the same way (the first step of a merge pairs i with i ^ (2j - 1), the
// later ones i with i ^ j, the smaller key to the lower index), so a pad that ranks last never leaves the indices >= cnt
// and a comparator that touches one is skipped.  No pad is stored, so none can outrank a negative score.
// Greedy loop: thread t owns the sorted candidates t, t + 1024, ...: it takes their anchor indices out of the keys into
// registers, then the key buffer becomes box[] (xyxy of every sorted candidate, for the pivot of a round) and the owner
// keeps its boxes in registers as well, so a round is one LDS broadcast read, the owned IoUs (postprocess_kernel's
// expressions: the same fp32 values) and one barrier.  dead[] = one bit per sorted candidate.  Nothing is written
// inside the loop: the survivors are the live candidates below the loop's end, ranked afterwards by a prefix count over
// dead[] and written by their owners.  Without stats the loop ends once max_out boxes are kept.
// ------------------------------------------------------------------------------------
constexpr int POST_ALL_NT = 1024;
constexpr int POST_ALL_PER = (POST_ALL_MAX_A + POST_ALL_NT - 1) / POST_ALL_NT;    // sorted candidates a thread owns
constexpr int POST_ALL_WORDS = (POST_ALL_MAX_A + 31) / 32;

__global__ __launch_bounds__(POST_ALL_NT) void postprocess_all_kernel(const float* __restrict__ raw, int A, float conf,
                                                                      float nms_thr, float clamp_max,
                                                                      float* __restrict__ boxes, int* __restrict__ counts,
                                                                      int max_out, int* __restrict__ stats) {
  __shared__ float4 box[POST_ALL_MAX_A];            // the sort's keys use its first half
  __shared__ unsigned int dead[POST_ALL_WORDS];
  __shared__ int wbase[POST_ALL_WORDS];             // survivors in the words before this one
  __shared__ int s_n;
  static_assert(sizeof(box) >= POST_ALL_MAX_A * sizeof(unsigned long long), "the keys must fit into box[]");
  unsigned long long* key = reinterpret_cast<unsigned long long*>(box);
  if (A > POST_ALL_MAX_A) return;                   // the launcher refuses it; never index past the arrays
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const float* r = raw + (long long)n * A * 6;
  if (tid == 0) s_n = 0;
  for (int i = tid; i < POST_ALL_WORDS; i += POST_ALL_NT) dead[i] = 0u;
  __syncthreads();
  // compaction in any order (the sort's order is total): one LDS atomic per wave and chunk
  for (int base = 0; base < A; base += POST_ALL_NT) {
    const int a = base + tid;
    float score = -1.0f;
    if (a < A) score = r[a * 6 + 4] * r[a * 6 + 5];
    const bool ok = a < A && score >= conf;
    const unsigned long long m = __ballot(ok);
    int off = 0;
    if (lane == 0 && m) off = atomicAdd(&s_n, __popcll(m));
    off = __shfl(off, 0) + __popcll(m & ((1ull << lane) - 1ull));
    if (ok) {
      const unsigned int u = __float_as_uint(score + 0.0f);        // -0 -> +0: the two compare equal
      const unsigned int asc = u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
      key[off] = ((unsigned long long)(~asc) << 32) | (unsigned int)a;
    }
  }
  __syncthreads();
  const int cnt = s_n;                              // <= A <= POST_ALL_MAX_A
  if (cnt == 0) {                                   // uniform; the usual patch at the config's threshold
    if (tid == 0) {
      counts[n] = 0;
      if (stats) { stats[n * 2] = 0; stats[n * 2 + 1] = 0; }
    }
    return;
  }
  int np2 = 1;
  while (np2 < cnt) np2 <<= 1;
  for (int k = 2; k <= np2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int flip = (j == (k >> 1)) ? k - 1 : j;
      for (int c = tid; c < (np2 >> 1); c += POST_ALL_NT) {
        const int i = ((c & ~(j - 1)) << 1) | (c & (j - 1));       // bit j of i clear
        const int l = i ^ flip;                                    // > i
        if (l < cnt) {
          const unsigned long long ki = key[i], kl = key[l];
          if (kl < ki) { key[i] = kl; key[l] = ki; }
        }
      }
      __syncthreads();
    }
  int id[POST_ALL_PER];
  float x1[POST_ALL_PER], y1[POST_ALL_PER], x2[POST_ALL_PER], y2[POST_ALL_PER];
#pragma unroll
  for (int q = 0; q < POST_ALL_PER; ++q) {
    const int j = q * POST_ALL_NT + tid;
    id[q] = j < cnt ? (int)(unsigned int)key[j] : 0;
  }
  __syncthreads();                                  // every key is in a register: the buffer is box[] from here on
#pragma unroll
  for (int q = 0; q < POST_ALL_PER; ++q) {
    const int j = q * POST_ALL_NT + tid;
    x1[q] = y1[q] = x2[q] = y2[q] = 0.0f;
    if (j < cnt) {
      const float* bj = r + id[q] * 6;
      x1[q] = bj[0] - bj[2] * 0.5f; y1[q] = bj[1] - bj[3] * 0.5f; x2[q] = bj[0] + bj[2] * 0.5f; y2[q] = bj[1] + bj[3] * 0.5f;
      box[j] = make_float4(x1[q], y1[q], x2[q], y2[q]);
    }
  }
  __syncthreads();
  unsigned int mine = 0u;                           // bit q: my candidate q is suppressed (the copy of its dead[] bit)
  int kept = 0, end = cnt;                          // uniform: every thread takes the same path
  for (int i = 0; i < cnt; ++i) {
    if ((dead[i >> 5] >> (i & 31)) & 1u) continue;  // uniform: dead[] is shared and synced
    if (!stats && kept >= max_out) { end = i; break; }
    ++kept;
    const float4 a = box[i];
    const float ax1 = a.x, ay1 = a.y, ax2 = a.z, ay2 = a.w;
    const float aa = (ax2 - ax1) * (ay2 - ay1);
#pragma unroll
    for (int q = 0; q < POST_ALL_PER; ++q) {
      const int j = q * POST_ALL_NT + tid;
      if (j <= i || j >= cnt || ((mine >> q) & 1u)) continue;
      const float bx1 = x1[q], by1 = y1[q], bx2 = x2[q], by2 = y2[q];
      const float iw = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.0f), ih = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.0f);
      const float inter = iw * ih;
      const float iou = inter / (aa + (bx2 - bx1) * (by2 - by1) - inter);
      if (iou > nms_thr) { mine |= 1u << q; atomicOr(&dead[j >> 5], 1u << (j & 31)); }
    }
    __syncthreads();
  }
  // the survivors are the live candidates below `end` (all of them pivots of a round), in sorted order
  for (int w = tid; w < (end + 31) / 32; w += POST_ALL_NT) {
    int before = 0;
    for (int v = 0; v < w; ++v) {
      const int left = end - 32 * v;                // candidates of word v below `end`
      const unsigned int valid = left >= 32 ? 0xFFFFFFFFu : left <= 0 ? 0u : (1u << left) - 1u;
      before += __popc(~dead[v] & valid);
    }
    wbase[w] = before;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < POST_ALL_PER; ++q) {
    const int j = q * POST_ALL_NT + tid;
    if (j >= end || ((mine >> q) & 1u)) continue;
    const int rank = wbase[j >> 5] + __popc(~dead[j >> 5] & ((1u << (j & 31)) - 1u));
    if (rank >= max_out) continue;
    const float* bj = r + id[q] * 6;
    float* o = boxes + ((long long)n * max_out + rank) * 7;
    o[0] = fminf(fmaxf(x1[q], 0.0f), clamp_max); o[1] = fminf(fmaxf(y1[q], 0.0f), clamp_max);
    o[2] = fminf(fmaxf(x2[q], 0.0f), clamp_max); o[3] = fminf(fmaxf(y2[q], 0.0f), clamp_max);
    o[4] = bj[4]; o[5] = bj[5]; o[6] = 0.0f;
  }
  if (tid == 0) {
    counts[n] = min(kept, max_out);
    if (stats) { stats[n * 2] = cnt; stats[n * 2 + 1] = kept; }
  }
}

int launch_postprocess_all(const float* raw, int A, int N, float conf, float nms_thr, float clamp_max, float* boxes,
                           int* counts, int max_out, int* stats, hipStream_t s) {
  if (A > POST_ALL_MAX_A) return 1;
  if (A <= DET_CAP) return launch_postprocess(raw, A, N, conf, nms_thr, clamp_max, boxes, counts, max_out, stats, s);
  hipLaunchKernelGGL(postprocess_all_kernel, dim3(N), dim3(POST_ALL_NT), 0, s, raw, A, conf, nms_thr, clamp_max, boxes,
                     counts, max_out, stats);
  return 0;
}

// boxes [B][K][7] / counts [B] of one glimpse step -> column `col` of [B][cols][K][7] / [B][cols]
__global__ void det_scatter_kernel(const float* __restrict__ boxes, const int* __restrict__ counts,
                                   float* __restrict__ out_boxes, int* __restrict__ out_counts, int B, int cols, int col,
                                   int K, const int* __restrict__ skip_flag, int skip_when) {
  if (skip_flag && *skip_flag >= skip_when) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * K * 7) return;
  const int b = i / (K * 7), r = i % (K * 7);
  out_boxes[((long long)b * cols + col) * K * 7 + r] = (r / 7 < counts[b]) ? boxes[i] : 0.0f;
  if (r == 0) out_counts[b * cols + col] = counts[b];
}

int launch_det_scatter(const float* boxes, const int* counts, float* out_boxes, int* out_counts, int B, int cols, int col,
                       int K, const int* skip_flag, int skip_when, hipStream_t s) {
  hipLaunchKernelGGL(det_scatter_kernel, dim3((B * K * 7 + 255) / 256), dim3(256), 0, s, boxes, counts, out_boxes,
                     out_counts, B, cols, col, K, skip_flag, skip_when);
  return 0;
}

}  // namespace jnr
