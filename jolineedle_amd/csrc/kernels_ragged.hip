// Per-image assembly of a rollout's detections: Trainer.patch_bboxes2full_image (src/trainer.py:250-280) for the whole
// batch in one launch.  The per-agent grid extents of ragged mode live with the env (kernels_env.hip, jn_device.h).
#include <hip/hip_runtime.h>

#include "jn_kernels.h"

namespace jnr {

constexpr int BTI_NT = 256;

// One workgroup per image.  Pass 1: the boxes each step contributes (0 where masks[b,t] == 0 or past S), an exclusive
// prefix sum over the steps in LDS (chunks of BTI_NT steps, a carry between chunks) and the step's pixel offset.
// Pass 2: every (step, box, column) element is one thread's load, add and store: columns 0..3 + (x*P, y*P, x*P, y*P)
// as one fp32 add each (the reference's `moved[:, 0:2] += offset.to(float)`), columns 4..6 copied.
// Dynamic LDS: int32 [4][S + 1] = first output row, box count, x*P, y*P per step; the scan buffers are static.
__global__ __launch_bounds__(BTI_NT) void boxes_to_image_kernel(const float* __restrict__ det_boxes,
                                                                const int32_t* __restrict__ det_counts,
                                                                const long long* __restrict__ positions,
                                                                const uint8_t* __restrict__ masks, int T, int S, int K, int P,
                                                                float* __restrict__ out_boxes, int32_t* __restrict__ out_totals) {
  extern __shared__ int32_t bti_sm[];
  __shared__ int32_t scan[2][BTI_NT];
  __shared__ int32_t carry;
  const int b = blockIdx.x, tid = threadIdx.x, n = S + 1;
  int32_t* first = bti_sm;
  int32_t* cnt = bti_sm + n;
  int32_t* offx = bti_sm + 2 * n;
  int32_t* offy = bti_sm + 3 * n;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int t0 = 0; t0 < n; t0 += BTI_NT) {
    const int t = t0 + tid;
    int c = 0;
    if (t < n) {
      const long long bt = (long long)b * (T + 1) + t;
      if (masks[bt]) c = min(max(det_counts[bt], 0), K);
      cnt[t] = c;
      offy[t] = (int32_t)(positions[2 * bt] * P);
      offx[t] = (int32_t)(positions[2 * bt + 1] * P);
    }
    int cur = 0;
    scan[0][tid] = c;
    __syncthreads();
    for (int d = 1; d < BTI_NT; d <<= 1) {               // Hillis-Steele inclusive scan, double-buffered
      const int v = scan[cur][tid] + (tid >= d ? scan[cur][tid - d] : 0);
      scan[cur ^ 1][tid] = v;
      cur ^= 1;
      __syncthreads();
    }
    const int base = carry;
    if (t < n) first[t] = base + scan[cur][tid] - c;
    __syncthreads();
    if (tid == BTI_NT - 1) carry = base + scan[cur][tid];
    __syncthreads();
  }
  if (tid == 0) out_totals[b] = carry;
  const long long per_step = (long long)K * 7;
  const float* src = det_boxes + (long long)b * (T + 1) * per_step;
  float* dst = out_boxes + (long long)b * n * per_step;
  for (long long i = tid; i < n * per_step; i += BTI_NT) {
    const int t = (int)(i / per_step);
    const int r = (int)(i - t * per_step);
    const int k = r / 7, col = r - k * 7;
    if (k >= cnt[t]) continue;
    float v = src[i];
    if (col < 4) v += (float)((col & 1) ? offy[t] : offx[t]);
    dst[(long long)(first[t] + k) * 7 + col] = v;
  }
}

int launch_boxes_to_image(const float* det_boxes, const int32_t* det_counts, const int64_t* positions, const uint8_t* masks,
                          int B, int T, int S, int K, int P, float* out_boxes, int32_t* out_totals, hipStream_t s) {
  const size_t smem = (size_t)4 * (S + 1) * sizeof(int32_t);
  hipLaunchKernelGGL(boxes_to_image_kernel, dim3(B), dim3(BTI_NT), smem, s, det_boxes, det_counts,
                     (const long long*)positions, masks, T, S, K, P, out_boxes, out_totals);
  return 0;
}

}  // namespace jnr
