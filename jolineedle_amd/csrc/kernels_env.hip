// Environment primitives: patch gather (bit-exact), bbox -> patch-grid masks, reset,
// step/reward, and the rollout prologue / epilogue (masks roll + suffix-sum returns).
// Integer / bool work is exact; see jn_device.h for the per-agent step.
#include <hip/hip_runtime.h>

#include <climits>
#include <type_traits>

#include "jn_device.h"
#include "jn_types.h"

namespace jnr {

// out[b, c, r, :] = images[b, c, y*P + r, x*P : x*P + P]   (src/env/general_env.py:285-306)
// ST = float: a copy; ST = uint8_t: byte b -> b / 255 (u8_unit), VEC reads 4 bytes per 16-byte store
template <bool VEC, typename ST>
__global__ __launch_bounds__(256) void gather_kernel(const ST* __restrict__ images,
                                                     const long long* __restrict__ pos, float* __restrict__ out,
                                                     long long out_sample_stride, int C, int H, int W, int P,
                                                     long long total, const int* __restrict__ skip_flag,
                                                     int skip_when, const long long* __restrict__ img_idx) {
  if (skip_flag && *skip_flag >= skip_when) return;
  constexpr int V = VEC ? 4 : 1;
  const int PV = P / V;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int q = (int)(idx % PV);
    const int r = (int)((idx / PV) % P);
    const int c = (int)((idx / ((long long)PV * P)) % C);
    const int b = (int)(idx / ((long long)PV * P * C));
    const long long y = pos[2 * b], x = pos[2 * b + 1];
    const long long im = img_idx ? img_idx[b] : b;   // indexed form: several patches per image; < 0 = zero patch
    float* dp = out + b * out_sample_stride + ((long long)c * P + r) * P + q * V;
    if (im < 0) {
      if (VEC) *reinterpret_cast<f32x4*>(dp) = f32x4{0.f, 0.f, 0.f, 0.f};
      else *dp = 0.f;
      continue;
    }
    const ST* sp = images + ((im * C + c) * H + y * P + r) * W + x * P + q * V;
    if constexpr (std::is_same<ST, uint8_t>::value) {
      if (VEC) *reinterpret_cast<f32x4*>(dp) = u8x4_unit(*reinterpret_cast<const uint32_t*>(sp));
      else *dp = u8_unit(*sp);
    } else {
      if (VEC) *reinterpret_cast<f32x4*>(dp) = *reinterpret_cast<const f32x4*>(sp);
      else *dp = *sp;
    }
  }
}

// VEC: four values per thread; the source rows must be aligned to four elements (16 bytes of fp32, 4 of uint8)
template <typename ST>
static int launch_gather_t(const ST* images, const int64_t* positions, float* out, long long out_sample_stride, int B,
                           int C, int H, int W, int P, const int* skip_flag, int skip_when, hipStream_t s,
                           const int64_t* image_index) {
  const bool vec = (P % 4 == 0) && (W % 4 == 0) && (out_sample_stride % 4 == 0) &&
                   ((uintptr_t)images % (4 * sizeof(ST)) == 0) && ((uintptr_t)out % 16 == 0);
  const long long total = (long long)B * C * P * (P / (vec ? 4 : 1));
  const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 256 * 32);
  if (vec)
    hipLaunchKernelGGL((gather_kernel<true, ST>), dim3(blocks), dim3(256), 0, s, images, (const long long*)positions, out,
                       out_sample_stride, C, H, W, P, total, skip_flag, skip_when, (const long long*)image_index);
  else
    hipLaunchKernelGGL((gather_kernel<false, ST>), dim3(blocks), dim3(256), 0, s, images, (const long long*)positions, out,
                       out_sample_stride, C, H, W, P, total, skip_flag, skip_when, (const long long*)image_index);
  return 0;
}

int launch_gather(const float* images, const int64_t* positions, float* out, long long out_sample_stride, int B,
                  int C, int H, int W, int P, const int* skip_flag, int skip_when, hipStream_t s,
                  const int64_t* image_index) {
  return launch_gather_t(images, positions, out, out_sample_stride, B, C, H, W, P, skip_flag, skip_when, s, image_index);
}

int launch_gather(const uint8_t* images, const int64_t* positions, float* out, long long out_sample_stride, int B,
                  int C, int H, int W, int P, const int* skip_flag, int skip_when, hipStream_t s,
                  const int64_t* image_index) {
  return launch_gather_t(images, positions, out, out_sample_stride, B, C, H, W, P, skip_flag, skip_when, s, image_index);
}

// convert_bboxes_to_masks (src/env/general_env.py:360-379) on the patch grid: a box covers
// pixels x1..x2, y1..y2 inclusive (kornia "xyxy_plus"), clipped to the image; a patch is
// marked when it holds at least one covered pixel.  One thread per image.  With `extent` ([B][2] = (gh, gw)) the
// image a box is clipped to is the agent's own gh*P x gw*P; the mask rows keep the canvas stride.
__global__ void bbox_masks_kernel(const long long* __restrict__ bboxes, uint8_t* __restrict__ masks,
                                  int32_t* __restrict__ n_tiles, int B, int nb, int H, int W, int P,
                                  const int32_t* __restrict__ extent) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int Gh = H / P, Gw = W / P;
  if (extent) { H = extent[2 * b] * P; W = extent[2 * b + 1] * P; }
  uint8_t* m = masks + (long long)b * Gh * Gw;
  for (int i = 0; i < Gh * Gw; ++i) m[i] = 0;
  for (int k = 0; k < nb; ++k) {
    const long long* bb = bboxes + ((long long)b * nb + k) * 4;
    long long x1 = bb[0] < 0 ? 0 : bb[0], y1 = bb[1] < 0 ? 0 : bb[1];
    long long x2 = bb[2] + 1 > W ? W : bb[2] + 1, y2 = bb[3] + 1 > H ? H : bb[3] + 1;   // exclusive
    if (x2 <= x1 || y2 <= y1) continue;
    for (int gy = (int)(y1 / P); gy <= (int)((y2 - 1) / P); ++gy)
      for (int gx = (int)(x1 / P); gx <= (int)((x2 - 1) / P); ++gx) m[gy * Gw + gx] = 1;
  }
  int cnt = 0;
  for (int i = 0; i < Gh * Gw; ++i) cnt += m[i];
  n_tiles[b] = cnt;
}

int launch_bbox_masks(const int64_t* bboxes, uint8_t* masks, int32_t* n_tiles, int B, int nb, int H, int W, int P,
                      hipStream_t s, const int32_t* extent) {
  hipLaunchKernelGGL(bbox_masks_kernel, dim3((B + 63) / 64), dim3(64), 0, s, (const long long*)bboxes, masks, n_tiles,
                     B, nb, H, W, P, extent);
  return 0;
}

// The detector's training batch (NeedleGeneralEnv.get_detection_batch, src/env/general_env.py:381-546; the rule is
// stated at jnroll.h: jn_detection_cells): which cells of every image hold a piece of a box, `sample_neg` empty cells
// per image, and every row's patch-local targets.  Integer-exact.  Three launches: count (a workgroup per image), an
// exclusive scan over the images (one workgroup), select (a workgroup per image).  A row's place follows from the
// scans alone, so two calls write the same bytes.
constexpr int kDetThreads = 256;

__device__ inline long long floor_div(long long a, long long p) { return a / p - ((a % p != 0) && (a < 0)); }

// does cell (py, px) hold a piece of any of the image's nb boxes?  (a box with y2 // P < y1 // P touches nothing)
__device__ inline bool det_cell_positive(const long long* __restrict__ bb, int nb, int P, int py, int px) {
  for (int k = 0; k < nb; ++k) {
    const long long* q = bb + 4 * k;
    if (floor_div(q[1], P) <= py && py <= floor_div(q[3], P) && floor_div(q[0], P) <= px && px <= floor_div(q[2], P)) return true;
  }
  return false;
}

// Inclusive sum of v over the workgroup's kDetThreads threads (Hillis-Steele in LDS, double-buffered).  Returns the
// thread's own sum, `total` = the workgroup's.  Ends on a barrier; the caller needs one more before the next call
// rewrites the buffers that other threads may still read.
__device__ inline int32_t det_block_scan(int32_t (*scan)[kDetThreads], int tid, int32_t v, int32_t& total) {
  int cur = 0;
  scan[0][tid] = v;
  __syncthreads();
  for (int d = 1; d < kDetThreads; d <<= 1) {
    scan[cur ^ 1][tid] = scan[cur][tid] + (tid >= d ? scan[cur][tid - d] : 0);
    cur ^= 1;
    __syncthreads();
  }
  total = scan[cur][kDetThreads - 1];
  return scan[cur][tid];
}

// offsets[b + 1] = the rows of image b (its positive cells + min(sample_neg, empty cells)), n_pos[b] = the positive ones
__global__ __launch_bounds__(kDetThreads) void det_cells_count_kernel(const long long* __restrict__ bboxes,
                                                                      const int32_t* __restrict__ extents, int nb, int Gh,
                                                                      int Gw, int P, int sample_neg,
                                                                      int32_t* __restrict__ offsets,
                                                                      int32_t* __restrict__ n_pos) {
  const int b = blockIdx.x;
  const int gh = extents ? extents[2 * b] : Gh, gw = extents ? extents[2 * b + 1] : Gw;
  const int cells = gh * gw;
  const long long* bb = bboxes + (long long)b * nb * 4;
  int pos = 0;
  for (int c0 = 0; c0 < cells; c0 += kDetThreads) {        // (uniform trip count: every thread reaches the barrier)
    const int c = c0 + threadIdx.x;
    pos += __syncthreads_count(c < cells && det_cell_positive(bb, nb, P, c / gw, c % gw));
  }
  if (threadIdx.x == 0) {
    n_pos[b] = pos;
    offsets[b + 1] = pos + min(sample_neg, cells - pos);
  }
}

// in place: offsets[b + 1] (the rows of image b) -> the inclusive sum, offsets[0] = 0.  One workgroup.
__global__ __launch_bounds__(kDetThreads) void det_cells_scan_kernel(int32_t* __restrict__ offsets, int B) {
  __shared__ int32_t scan[2][kDetThreads];
  __shared__ int32_t carry;
  const int tid = threadIdx.x;
  if (tid == 0) { carry = 0; offsets[0] = 0; }
  __syncthreads();
  for (int b0 = 0; b0 < B; b0 += kDetThreads) {
    const int b = b0 + tid;
    int32_t total;
    const int32_t sum = det_block_scan(scan, tid, b < B ? offsets[b + 1] : 0, total);
    const int32_t base = carry;
    if (b < B) offsets[b + 1] = base + sum;
    __syncthreads();
    if (tid == 0) carry = base + total;
    __syncthreads();
  }
}

// Dynamic LDS: uint16 [2][cells] = the image's positive cells and its empty cells, each in row-major order.
__global__ __launch_bounds__(kDetThreads) void det_cells_select_kernel(
    const long long* __restrict__ bboxes, const int32_t* __restrict__ extents, int nb, int Gh, int Gw, int P, int sample_neg,
    uint64_t seed, int capacity, const int32_t* __restrict__ offsets, long long* __restrict__ out_cells,
    long long* __restrict__ out_targets) {
  extern __shared__ uint16_t det_lists[];
  __shared__ int32_t scan[2][kDetThreads];
  __shared__ int32_t n_positive;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int gh = extents ? extents[2 * b] : Gh, gw = extents ? extents[2 * b + 1] : Gw;
  const int cells = gh * gw;
  uint16_t* positive = det_lists;
  uint16_t* empty = det_lists + cells;
  const long long* bb = bboxes + (long long)b * nb * 4;
  int base = 0;                                              // positive cells before this pass (uniform)
  for (int c0 = 0; c0 < cells; c0 += kDetThreads) {
    const int c = c0 + tid;
    const int f = (c < cells && det_cell_positive(bb, nb, P, c / gw, c % gw)) ? 1 : 0;
    int32_t total;
    const int before = base + det_block_scan(scan, tid, f, total) - f;   // positive cells in front of c; the others there are empty
    if (c < cells) {
      if (f) positive[before] = (uint16_t)c;
      else empty[c - before] = (uint16_t)c;
    }
    base += total;
    __syncthreads();
  }
  if (tid == 0) {
    // partial Fisher-Yates over the empty list: draw j swaps E[j] with E[j + r mod (n_empty - j)]
    const int n_empty = cells - base;
    const int k = min(sample_neg, n_empty);
    for (int j = 0; j < k; ++j) {
      const uint32_t r = philox4x32(seed, (uint32_t)b, (uint32_t)j, 0x4e454753u, 0u).x;
      const int o = j + (int)(r % (uint32_t)(n_empty - j));
      const uint16_t t = empty[j]; empty[j] = empty[o]; empty[o] = t;
    }
    n_positive = base;
  }
  __syncthreads();
  const int npos = n_positive;
  const int first = offsets[b];
  const int rows = min(offsets[b + 1], capacity) - first;    // this image's rows below the capacity (may be <= 0)
  for (int i = tid; i < rows * nb; i += kDetThreads) {
    const int r = i / nb, k = i % nb;
    const int c = r < npos ? positive[r] : empty[r - npos];
    const int py = c / gw, px = c % gw;
    const long long row = (long long)first + r;
    if (k == 0) {
      long long* oc = out_cells + row * 3;
      oc[0] = b; oc[1] = py; oc[2] = px;
    }
    const long long* q = bb + 4 * k;
    const long long x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3];
    const long long ox = (long long)px * P, oy = (long long)py * P;
    const bool touch = floor_div(y1, P) <= py && py <= floor_div(y2, P) && floor_div(x1, P) <= px && px <= floor_div(x2, P);
    long long* ot = out_targets + (row * nb + k) * 5;
    ot[0] = 0;
    ot[1] = touch ? (x1 > ox ? x1 : ox) - ox : 0;
    ot[2] = touch ? (y1 > oy ? y1 : oy) - oy : 0;
    ot[3] = touch ? (x2 < ox + P - 1 ? x2 : ox + P - 1) - ox : 0;
    ot[4] = touch ? (y2 < oy + P - 1 ? y2 : oy + P - 1) - oy : 0;
  }
}

int launch_detection_cells(const int64_t* bboxes, const int32_t* extents, int B, int nb, int Gh, int Gw, int P, int sample_neg,
                           uint64_t seed, int capacity, int64_t* cells, int64_t* targets, int32_t* offsets, int32_t* n_pos,
                           hipStream_t s) {
  if (B > 0)
    hipLaunchKernelGGL(det_cells_count_kernel, dim3(B), dim3(kDetThreads), 0, s, (const long long*)bboxes, extents, nb, Gh, Gw, P,
                       sample_neg, offsets, n_pos);
  hipLaunchKernelGGL(det_cells_scan_kernel, dim3(1), dim3(kDetThreads), 0, s, offsets, B);
  if (B > 0)
    hipLaunchKernelGGL(det_cells_select_kernel, dim3(B), dim3(kDetThreads), 2 * sizeof(uint16_t) * (size_t)Gh * Gw, s,
                       (const long long*)bboxes, extents, nb, Gh, Gw, P, sample_neg, seed, capacity, offsets, (long long*)cells,
                       (long long*)targets);
  return 0;
}

// reset (src/env/general_env.py:144-170): zero state, place agents, mark the start tile.  keys ([B][2] = (stream seed,
// stream index), or null): the random start of agent b is drawn from its own stream instead of (seed, b).
__global__ void env_reset_kernel(EnvPtrs e, const long long* __restrict__ start, uint64_t seed,
                                 const uint64_t* __restrict__ keys) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= e.B) return;
  int y, x;
  if (start) { y = (int)start[2 * b]; x = (int)start[2 * b + 1]; }
  else {
    const uint4 r = keys ? philox4x32(keys[2 * b], (uint32_t)keys[2 * b + 1], 0u, 0x52455345u, 0u)
                         : philox4x32(seed, (uint32_t)b, 0u, 0x52455345u, 0u);
    const int gh = e.extent ? e.extent[2 * b] : e.Gh, gw = e.extent ? e.extent[2 * b + 1] : e.Gw;
    y = (int)(r.x % (uint32_t)gh); x = (int)(r.y % (uint32_t)gw);
  }
  e.positions[2 * b] = y; e.positions[2 * b + 1] = x;
  uint8_t* v = e.visited + (long long)b * e.Gh * e.Gw;
  for (int i = 0; i < e.Gh * e.Gw; ++i) v[i] = 0;
  const int tile = y * e.Gw + x;
  v[tile] = 1;
  e.found[b] = e.bbox_masks[(long long)b * e.Gh * e.Gw + tile] ? 1 : 0;
  e.steps[b] = 0;
  e.has_stopped[b] = 0;
}

int launch_env_reset(const EnvPtrs& e, const int64_t* start_positions, uint64_t seed, const uint64_t* keys, hipStream_t s) {
  hipLaunchKernelGGL(env_reset_kernel, dim3((e.B + 63) / 64), dim3(64), 0, s, e, (const long long*)start_positions, seed, keys);
  return 0;
}

__global__ void env_step_kernel(EnvPtrs e, const long long* __restrict__ actions, float* __restrict__ rewards,
                                uint8_t* __restrict__ terminated, uint8_t* __restrict__ truncated) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= e.B) return;
  int a = (int)actions[b];
  a = min(max(a, 0), 8);
  const EnvStepResult r = env_step_one(e, b, a);
  if (rewards) rewards[b] = r.reward;
  if (terminated) terminated[b] = r.terminated;
  if (truncated) truncated[b] = r.truncated;
}

int launch_env_step(const EnvPtrs& e, const int64_t* actions, float* rewards, uint8_t* terminated,
                    uint8_t* truncated, hipStream_t s) {
  hipLaunchKernelGGL(env_step_kernel, dim3((e.B + 63) / 64), dim3(64), 0, s, e, (const long long*)actions, rewards,
                     terminated, truncated);
  return 0;
}

// Rollout prologue (src/reinforce.py:123-139): BOS action 0, masks[:,0] = True, positions[:,0].
__global__ void rollout_begin_kernel(EnvPtrs e, RolloutBuffers r, long long* prev_action, int32_t* cache_len,
                                     int32_t* n_done) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b == 0)
    for (int t = 0; t <= e.T; ++t) n_done[t] = 0;
  if (b >= e.B) return;
  prev_action[b] = 0;
  cache_len[b] = 0;
  if (r.masks) r.masks[(long long)b * (e.T + 1)] = 1;
  if (r.positions) {
    r.positions[((long long)b * (e.T + 1)) * 2] = e.positions[2 * b];
    r.positions[((long long)b * (e.T + 1)) * 2 + 1] = e.positions[2 * b + 1];
  }
}

int launch_rollout_begin(const EnvPtrs& e, const RolloutBuffers& r, int64_t* prev_action, int32_t* cache_len,
                         int32_t* n_done, hipStream_t s) {
  hipLaunchKernelGGL(rollout_begin_kernel, dim3((e.B + 63) / 64), dim3(64), 0, s, e, r, (long long*)prev_action, cache_len,
                     n_done);
  return 0;
}

// Rollout epilogue (src/reinforce.py:186-202): logit_masks = roll(masks[:,1:], 1) with column 0
// forced True; returns[t] = sum_{k>=t} rewards[k] * logit_masks[k], accumulated from the end
// (the order of the reference's flip -> cumsum -> flip).  S = steps actually executed.
__global__ void rollout_epilogue_kernel(RolloutBuffers r, const int32_t* __restrict__ n_done, int B, int T,
                                        int stop_early) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int S = T;
  if (stop_early)
    for (int t = 1; t <= T; ++t)
      if (n_done[t] >= B) { S = t; break; }
  float run = 0.0f;
  for (int t = S - 1; t >= 0; --t) {
    const bool lm = (t == 0) ? true : (r.masks[(long long)b * (T + 1) + t] != 0);
    if (r.logit_masks) r.logit_masks[(long long)b * T + t] = lm;
    run = run + r.rewards[(long long)b * T + t] * (lm ? 1.0f : 0.0f);
    if (r.returns) r.returns[(long long)b * T + t] = run;
  }
}

int launch_rollout_epilogue(const RolloutBuffers& r, const int32_t* n_done, int B, int T, int stop_early,
                            hipStream_t s) {
  hipLaunchKernelGGL(rollout_epilogue_kernel, dim3((B + 63) / 64), dim3(64), 0, s, r, n_done, B, T, stop_early);
  return 0;
}

// The teacher's opinion of a state (NeedleSimpleEnv.build_keypoints_trajectory + move_towards, src/env/simple_env.py:
// 590-629, 84-125): the remaining targets are targets & ~visited, N = those at the minimum Manhattan distance from the
// agent, and the byte holds bit a for every action a = move_towards(agent, q), q in N — the deterministic object behind
// the reference's random.choice among N.  STOP (a target under the agent) sets no bit; no remaining target gives 0.
// One wave per agent: each lane keeps (min distance, directions at it) over its cells i = lane, lane + 64, ..., then the
// wave takes the minimum of the distances and ORs the bits of the lanes that hold it.  set_stride: bytes between agents
// in `sets` (1 for a [B] vector, T for column t of the rollout's [B,T]).
constexpr int kTeacherWaves = 4;   // agents per 256-thread block
__global__ __launch_bounds__(64 * kTeacherWaves) void teacher_sets_kernel(
    const long long* __restrict__ pos, const uint8_t* __restrict__ visited, const uint8_t* __restrict__ targets,
    uint8_t* __restrict__ sets, long long set_stride, int B, int Gh, int Gw, const int* __restrict__ skip_flag,
    int skip_when) {
  if (skip_flag && *skip_flag >= skip_when) return;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kTeacherWaves + (threadIdx.x >> 6);
  if (b >= B) return;                                    // whole waves leave: the shuffles below stay wave-uniform
  const int y = (int)pos[2 * b], x = (int)pos[2 * b + 1];
  const int cells = Gh * Gw;
  const uint8_t* tg = targets + (long long)b * cells;
  const uint8_t* vs = visited + (long long)b * cells;
  int best = INT_MAX;
  uint32_t bits = 0;
  for (int i = lane; i < cells; i += 64) {
    if (!tg[i] || vs[i]) continue;
    const int dy = i / Gw - y, dx = i % Gw - x;
    const int d = abs(dy) + abs(dx);
    const int a = kTowards[((dy > 0) - (dy < 0) + 1) * 3 + (dx > 0) - (dx < 0) + 1];
    const uint32_t bit = a < 8 ? 1u << a : 0u;
    if (d < best) { best = d; bits = bit; }
    else if (d == best) bits |= bit;
  }
  int wmin = best;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) wmin = min(wmin, __shfl_xor(wmin, o, 64));
  bits = (best == wmin && best != INT_MAX) ? bits : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bits |= (uint32_t)__shfl_xor((int)bits, o, 64);
  if (lane == 0) sets[b * set_stride] = (uint8_t)bits;
}

int launch_teacher_sets(const int64_t* positions, const uint8_t* visited, const uint8_t* targets, uint8_t* sets,
                        long long set_stride, int B, int Gh, int Gw, const int* skip_flag, int skip_when, hipStream_t s) {
  hipLaunchKernelGGL(teacher_sets_kernel, dim3((B + kTeacherWaves - 1) / kTeacherWaves), dim3(64 * kTeacherWaves), 0, s,
                     (const long long*)positions, visited, targets, sets, set_stride, B, Gh, Gw, skip_flag, skip_when);
  return 0;
}

// The action sets of N given states under a masking policy: action_set_one (jn_device.h), the function the masked decision
// of a rollout calls, on caller arrays — one thread per state.
__global__ __launch_bounds__(256) void action_sets_kernel(const long long* __restrict__ pos, const uint8_t* __restrict__ visited,
                                                          const int32_t* __restrict__ extents, const long long* __restrict__ forced,
                                                          int N, int Gh, int Gw, int policy, int nA, uint16_t* __restrict__ sets) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int gh = extents ? min(extents[2 * n], Gh) : Gh, gw = extents ? min(extents[2 * n + 1], Gw) : Gw;   // reads stay inside `visited`
  const int f = forced ? min(max((int)forced[n], 0), nA - 1) : -1;
  sets[n] = (uint16_t)action_set_one(policy, (int)pos[2 * n], (int)pos[2 * n + 1], gh, gw, visited + (long long)n * Gh * Gw, Gw, nA, f);
}

int launch_action_sets(const int64_t* positions, const uint8_t* visited, const int32_t* extents, const int64_t* forced, int N,
                       int Gh, int Gw, int policy, int nA, uint16_t* sets, hipStream_t s) {
  hipLaunchKernelGGL(action_sets_kernel, dim3((N + 255) / 256), dim3(256), 0, s, (const long long*)positions, visited, extents,
                     (const long long*)forced, N, Gh, Gw, policy, nA, sets);
  return 0;
}

// The teacher's whole walk (NeedleSimpleEnv.generate_sample_indices, src/env/simple_env.py:481-588; the rule and its two
// Philox streams are stated at jnroll.h: jn_teacher_walks and, on plain integers, by trajectory.teacher_walks).  One wave
// per image.  The draws and the walk are sequential: every lane computes the same draw and the same position, the values
// are made scalar (readfirstlane) and the control flow is wave-uniform; lane 0 writes the ring.  The nearest-target search
// and the tie rank use all 64 lanes.  Three launches: walk (also counts the image's detector rows), the exclusive scan of
// jn_detection_cells, detector rows.
constexpr uint32_t kWalkTagR = 0x54574B52u, kWalkTagY = 0x54574B59u;

struct WalkStep { uint8_t action, teacher, label, pad; uint16_t y, x; };      // one step of the LDS ring, 8 bytes

__device__ inline bool walk_box_real(const long long* q) { return (q[0] | q[1] | q[2] | q[3]) != 0; }

// bbox_positions (src/env/simple_env.py:270-321): is cell (cy, cx) one of box q's?  Its centre cell, or a cell of its own
// range holding more than 1 / 20 of a patch area: h * w / P**2 > 0.05 <=> 20 * h * w > P * P on integers.
__device__ inline bool walk_cell_target(const long long* q, long long P, int cy, int cx) {
  const long long x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3];
  if (floor_div(floor_div(y1 + y2, 2), P) == cy && floor_div(floor_div(x1 + x2, 2), P) == cx) return true;
  if (cy < floor_div(y1, P) || cy > floor_div(y2, P) || cx < floor_div(x1, P) || cx > floor_div(x2, P)) return false;
  const long long h = min((cy + 1) * P, y2) - max(cy * P, y1);
  const long long w = min((cx + 1) * P, x2) - max(cx * P, x1);
  return 20 * h * w > P * P;
}

// NeedleSimpleEnv.local_bboxes (:231-268): the part of box q inside the patch at (py, px) as (0, x1, y1, x2, y2, 1), or zeros
__device__ inline void walk_local_box(const long long* q, long long P, int py, int px, bool live, float* __restrict__ o) {
  const long long ox = px * P, oy = py * P;
  const long long cx1 = max(ox, q[0]), cy1 = max(oy, q[1]), cx2 = min(ox + P, q[2]), cy2 = min(oy + P, q[3]);
  const bool in = live && cx1 < cx2 && cy1 < cy2;
  o[0] = 0.f;
  o[1] = in ? (float)(cx1 - ox) : 0.f;
  o[2] = in ? (float)(cy1 - oy) : 0.f;
  o[3] = in ? (float)(cx2 - ox) : 0.f;
  o[4] = in ? (float)(cy2 - oy) : 0.f;
  o[5] = in ? 1.f : 0.f;
}

__device__ inline int walk_towards(int y, int x, int ty, int tx) {
  return kTowards[((ty > y) - (ty < y) + 1) * 3 + (tx > x) - (tx < x) + 1];
}

__device__ inline unsigned long long walk_lanes_below(int lane) { return (1ull << lane) - 1ull; }

// Dynamic LDS: WalkStep [T], the ring of the walk's last T steps.
__global__ __launch_bounds__(64) void teacher_walk_kernel(TeacherWalkArgs a) {
  __shared__ uint8_t s_target[JN_TWALK_MAX_CELLS];
  __shared__ uint8_t s_todo[JN_TWALK_MAX_CELLS];
  extern __shared__ WalkStep walk_ring[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Gh = a.Gh, Gw = a.Gw, cells = Gh * Gw, T = a.T, nb = a.nb;
  const long long P = a.P;
  const long long* bb = (const long long*)a.bboxes + (long long)b * nb * 4;

  // the target cells of the image, its detector rows counted on the way
  int n_target = 0;
  for (int c0 = 0; c0 < cells; c0 += 64) {
    const int c = c0 + lane;
    bool t = false;
    if (c < cells) {
      const int cy = c / Gw, cx = c % Gw;
      for (int k = 0; k < nb && !t; ++k) t = walk_box_real(bb + 4 * k) && walk_cell_target(bb + 4 * k, P, cy, cx);
      s_target[c] = t;
      s_todo[c] = t;
      a.targets[(long long)b * cells + c] = t;
    }
    n_target += __popcll(__ballot(t));
  }
  __syncthreads();

  uint32_t kr = 0;                                           // draws of stream R made so far (uniform)
  auto draw = [&]() -> uint32_t {
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)philox4x32(a.seed, (uint32_t)b, kr++, kWalkTagR, 0u).x);
  };
  if (n_target < cells) draw();                              // the negative detector cell: teacher_walk_rows_kernel redraws it
  int y, x;
  if (a.starts) {
    y = min(max((int)a.starts[2 * b], 0), Gh - 1);
    x = min(max((int)a.starts[2 * b + 1], 0), Gw - 1);
  } else {
    y = (int)(draw() % (uint32_t)Gh);
    x = (int)(draw() % (uint32_t)Gw);
  }
  y = __builtin_amdgcn_readfirstlane(y);
  x = __builtin_amdgcn_readfirstlane(x);
  int n_keypoints = __builtin_amdgcn_readfirstlane(n_target - (s_target[y * Gw + x] ? 1 : 0));
  __syncthreads();                                           // (every lane has read the start's cell)
  if (lane == 0) s_todo[y * Gw + x] = 0;
  __syncthreads();
  const bool random_keypoint = n_keypoints == 0;             // nothing to visit: one random cell
  int ry = 0, rx = 0;
  if (random_keypoint) {
    ry = (int)(draw() % (uint32_t)Gh);
    rx = (int)(draw() % (uint32_t)Gw);
    n_keypoints = 1;
  }
  const int n_extra = a.min_keypoints + (int)(draw() % (uint32_t)(a.max_keypoints + 1 - a.min_keypoints));
  // the detour table: lane j holds the keypoint in front of which detour j is walked (n_extra <= 64)
  int insert_at = -1;
  if (lane < n_extra)
    insert_at = (int)(philox4x32(a.seed, (uint32_t)b, kr + (uint32_t)lane, kWalkTagR, 0u).x % (uint32_t)n_keypoints);
  kr += (uint32_t)n_extra;

  int n = 0;                                                 // steps recorded so far
  if (lane == 0) walk_ring[0] = WalkStep{0, 0, s_target[y * Gw + x], 0, (uint16_t)y, (uint16_t)x};
  n = 1;
  const int longest = max(Gh, Gw);                           // a visit takes fewer king's moves than that

  // walk to (ty, tx) while the teacher points at (ky, kx); STOP is replaced by a random move
  auto visit = [&](int ty, int tx, int ky, int kx) {
    for (int i = 0; i < longest && (y != ty || x != tx); ++i) {
      const int act = walk_towards(y, x, ty, tx);
      y += kActionDy[act];
      x += kActionDx[act];
      int best = walk_towards(y, x, ky, kx);
      if (best == 8) best = (int)(draw() % 8u);
      if (lane == 0)
        walk_ring[n % T] = WalkStep{(uint8_t)act, (uint8_t)best, s_target[y * Gw + x], 0, (uint16_t)y, (uint16_t)x};
      ++n;
    }
  };
  auto binomial = [&](int bits) -> int {                     // set bits among `bits` random bits, 32 per draw
    int total = 0;
    for (int j = 0; 32 * j < bits; ++j) {
      uint32_t r = draw();
      if (bits - 32 * j < 32) r &= (1u << (bits - 32 * j)) - 1u;
      total += __popc(r);
    }
    return total;
  };

  for (int kid = 0; kid < n_keypoints; ++kid) {
    int ky = ry, kx = rx;
    if (!random_keypoint) {
      // the nearest cells still to visit (L1), then the (draw mod their number)-th of them in row-major order
      int best = INT_MAX, cnt = 0;
      for (int i = lane; i < cells; i += 64) {
        if (!s_todo[i]) continue;
        const int d = abs(i / Gw - y) + abs(i % Gw - x);
        if (d < best) { best = d; cnt = 1; }
        else if (d == best) ++cnt;
      }
      int wmin = best;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) wmin = min(wmin, __shfl_xor(wmin, o, 64));
      int len = best == wmin ? cnt : 0;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) len += __shfl_xor(len, o, 64);
      wmin = __builtin_amdgcn_readfirstlane(wmin);
      len = __builtin_amdgcn_readfirstlane(len);
      if (len <= 0) break;                                   // (cannot happen: n_keypoints counts the cells to visit)
      const uint32_t r = philox4x32(a.seed, (uint32_t)b, (uint32_t)kid, kWalkTagY, 0u).x;
      const int rank = __builtin_amdgcn_readfirstlane((int)(r % (uint32_t)len));
      int seen = 0, chosen = -1;
      for (int c0 = 0; c0 < cells; c0 += 64) {
        const int c = c0 + lane;
        const bool tie = c < cells && s_todo[c] && abs(c / Gw - y) + abs(c % Gw - x) == wmin;
        const unsigned long long m = __ballot(tie);
        const int pc = __popcll(m);
        if (rank < seen + pc) {
          const unsigned long long sel = __ballot(tie && __popcll(m & walk_lanes_below(lane)) == rank - seen);
          chosen = c0 + __ffsll((long long)sel) - 1;
          break;
        }
        seen += pc;
      }
      if (chosen < 0) break;                                 // (cannot happen: rank < len)
      __syncthreads();                                       // (every lane has read the todo bytes)
      if (lane == 0) s_todo[chosen] = 0;
      __syncthreads();
      ky = chosen / Gw;
      kx = chosen % Gw;
    }
    // the teacher action of the last recorded step now points at this keypoint
    int best = walk_towards(y, x, ky, kx);
    if (best == 8) best = (int)(draw() % 8u);
    if (lane == 0) walk_ring[(n - 1) % T].teacher = (uint8_t)best;
    const int n_detours = __popcll(__ballot(insert_at == kid));
    for (int d = 0; d < n_detours; ++d) {
      int ty, tx;
      if (a.binomial) {
        const int dx = binomial(Gw) - Gw / 2;
        const int dy = binomial(Gh) - Gh / 2;
        ty = ((ky + dy) % Gh + Gh) % Gh;
        tx = ((kx + dx) % Gw + Gw) % Gw;
      } else {
        ty = (int)(draw() % (uint32_t)Gh);
        tx = (int)(draw() % (uint32_t)Gw);
      }
      visit(ty, tx, ky, kx);
    }
    visit(ky, kx, ky, kx);
  }
  __syncthreads();

  // the last min(n, T) steps, zero rows behind them
  const int kept = min(n, T), first = n - kept;
  if (lane == 0) {
    a.n_steps[b] = n;
    a.offsets[b + 1] = n_target + (n_target < cells ? 1 : 0);
  }
  for (int i = lane; i < T; i += 64) {
    const bool live = i < kept;
    const WalkStep s = live ? walk_ring[(first + i) % T] : WalkStep{0, 0, 0, 0, 0, 0};
    const long long row = (long long)b * T + i;
    a.positions[2 * row] = s.y;
    a.positions[2 * row + 1] = s.x;
    a.current_actions[row] = s.action;
    a.next_actions[row] = s.teacher;
    a.labels[row] = s.label;
    a.masks[row] = live ? 1.f : 0.f;
  }
  // local boxes: column j is the j-th real (non-zero) row; a lane keeps its box and walks the T rows
  int n_real = 0;
  for (int k0 = 0; k0 < nb; k0 += 64) {
    const int k = k0 + lane;
    const bool real = k < nb && walk_box_real(bb + 4 * k);
    const unsigned long long m = __ballot(real);
    if (real) {
      const int col = n_real + __popcll(m & walk_lanes_below(lane));
      const long long q[4] = {bb[4 * k], bb[4 * k + 1], bb[4 * k + 2], bb[4 * k + 3]};
      for (int i = 0; i < T; ++i) {
        const bool live = i < kept;
        const WalkStep s = live ? walk_ring[(first + i) % T] : WalkStep{0, 0, 0, 0, 0, 0};
        walk_local_box(q, P, s.y, s.x, live, a.local_bboxes + (((long long)b * T + i) * nb + col) * 6);
      }
    }
    n_real += __popcll(m);
  }
  const int n_pad = nb - n_real;
  for (long long idx = lane; idx < (long long)T * n_pad; idx += 64) {
    float* o = a.local_bboxes + (((long long)b * T + idx / n_pad) * nb + n_real + idx % n_pad) * 6;
    for (int j = 0; j < 6; ++j) o[j] = 0.f;
  }
}

// The detector rows of image b at offsets[b]: its target cells in row-major order, then the one negative cell — the
// (draw 0 of stream R mod n_empty)-th empty cell in row-major order — each with its local boxes.
__global__ __launch_bounds__(64) void teacher_walk_rows_kernel(TeacherWalkArgs a) {
  __shared__ uint16_t s_cells[JN_TWALK_MAX_CELLS];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Gw = a.Gw, cells = a.Gh * Gw, nb = a.nb;
  const long long P = a.P;
  const long long* bb = (const long long*)a.bboxes + (long long)b * nb * 4;
  const uint8_t* tg = a.targets + (long long)b * cells;
  int n_pos = 0;
  for (int c0 = 0; c0 < cells; c0 += 64) {
    const int c = c0 + lane;
    const bool t = c < cells && tg[c];
    const unsigned long long m = __ballot(t);
    if (t) s_cells[n_pos + __popcll(m & walk_lanes_below(lane))] = (uint16_t)c;
    n_pos += __popcll(m);
  }
  int n_rows = n_pos;
  if (n_pos < cells) {
    const uint32_t r = philox4x32(a.seed, (uint32_t)b, 0u, kWalkTagR, 0u).x;
    const int rank = __builtin_amdgcn_readfirstlane((int)(r % (uint32_t)(cells - n_pos)));
    int seen = 0;
    for (int c0 = 0; c0 < cells; c0 += 64) {
      const int c = c0 + lane;
      const bool e = c < cells && !tg[c];
      const unsigned long long m = __ballot(e);
      const int pc = __popcll(m);
      if (rank < seen + pc) {
        const unsigned long long sel = __ballot(e && __popcll(m & walk_lanes_below(lane)) == rank - seen);
        if (lane == 0) s_cells[n_pos] = (uint16_t)(c0 + __ffsll((long long)sel) - 1);
        break;
      }
      seen += pc;
    }
    n_rows = n_pos + 1;
  }
  __syncthreads();
  const int first = a.offsets[b];
  const int rows = min(first + n_rows, a.capacity) - first;   // this image's rows below the capacity (may be <= 0)
  for (int r = lane; r < rows; r += 64) {
    long long* oc = (long long*)a.cells + ((long long)first + r) * 3;
    const int c = s_cells[r];
    oc[0] = b; oc[1] = c / Gw; oc[2] = c % Gw;
  }
  int n_real = 0;
  for (int k0 = 0; k0 < nb; k0 += 64) {
    const int k = k0 + lane;
    const bool real = k < nb && walk_box_real(bb + 4 * k);
    const unsigned long long m = __ballot(real);
    if (real) {
      const int col = n_real + __popcll(m & walk_lanes_below(lane));
      const long long q[4] = {bb[4 * k], bb[4 * k + 1], bb[4 * k + 2], bb[4 * k + 3]};
      for (int r = 0; r < rows; ++r) {
        const int c = s_cells[r];
        walk_local_box(q, P, c / Gw, c % Gw, true, a.bboxes_yolox + (((long long)first + r) * nb + col) * 6);
      }
    }
    n_real += __popcll(m);
  }
  const int n_pad = nb - n_real;
  for (long long idx = lane; idx < (long long)max(rows, 0) * n_pad; idx += 64) {
    float* o = a.bboxes_yolox + (((long long)first + idx / n_pad) * nb + n_real + idx % n_pad) * 6;
    for (int j = 0; j < 6; ++j) o[j] = 0.f;
  }
}

int launch_teacher_walks(const TeacherWalkArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(teacher_walk_kernel, dim3(a.B), dim3(64), sizeof(WalkStep) * (size_t)a.T, s, a);
  hipLaunchKernelGGL(det_cells_scan_kernel, dim3(1), dim3(kDetThreads), 0, s, a.offsets, a.B);
  hipLaunchKernelGGL(teacher_walk_rows_kernel, dim3(a.B), dim3(64), 0, s, a);
  return 0;
}

}  // namespace jnr
