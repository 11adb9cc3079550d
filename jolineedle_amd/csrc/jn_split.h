// fp32 operands on the bf16 matrix pipe: THE place that knows how a value is split into bf16 planes and in which order
// the partial products are summed.  Every kernel that feeds v_mfma_f32_16x16x32_bf16 with fp32 data goes through here, so
// that the splitters (weights, split once) and the kernels (operand tiles, split while staged) agree bit for bit.
//
// Three-way ("x3"): an fp32 value is exactly the sum of three bf16 values (8 + 8 + 8 significand bits),
//   h = bf16(v), m = bf16(v - h), l = bf16(v - h - m),
// so x * w = (xh + xm + xl)(wh + wm + wl).  The three products below 2^-25 |x w| (m l, l m, l l) are dropped, the other
// six go into one fp32 accumulator: the error against an fp64 sum is that of an fp32 fmaf chain.
// Two-way: h = bf16(v), l = bf16(v - h), products h h + h l + l h (~1e-5 relative).  The weight-gradient kernels use
// it: a weight gradient is a leaf, its error reaches the optimiser only.
#pragma once
#include <hip/hip_runtime.h>

#include "jn_types.h"

namespace jnr {

// m and l of a value whose h = bf16(v) the caller has formed already (a kernel that stores h at once, or h alone)
__device__ __forceinline__ void split3_low(f32x4 v, bf16x4 h, bf16x4& m, bf16x4& l) {
  const f32x4 r1 = v - __builtin_convertvector(h, f32x4);
  m = __builtin_convertvector(r1, bf16x4);
  l = __builtin_convertvector(r1 - __builtin_convertvector(m, f32x4), bf16x4);
}
// the three planes plane_stride elements apart: h at dst, m at dst + plane_stride, l at dst + 2 plane_stride
__device__ __forceinline__ void split3_store(bf16_t* dst, int plane_stride, f32x4 v) {
  const bf16x4 h = __builtin_convertvector(v, bf16x4);
  bf16x4 m, l;
  split3_low(v, h, m, l);
  *reinterpret_cast<bf16x4*>(dst) = h;
  *reinterpret_cast<bf16x4*>(dst + plane_stride) = m;
  *reinterpret_cast<bf16x4*>(dst + 2 * plane_stride) = l;
}
// one value into element e of 8-wide fragments (the weight splitters, which write 16-byte pieces of a plane)
__device__ __forceinline__ void split3(float v, bf16x8& h, bf16x8& m, bf16x8& l, int e) {
  const bf16_t vh = (bf16_t)v;
  const float r1 = v - (float)vh;
  const bf16_t vm = (bf16_t)r1;
  h[e] = vh; m[e] = vm; l[e] = (bf16_t)(r1 - (float)vm);
}
// eight consecutive values (a | b)
__device__ __forceinline__ void split3(f32x4 a, f32x4 b, bf16x8& h, bf16x8& m, bf16x8& l) {
#pragma unroll
  for (int e = 0; e < 8; ++e) split3(e < 4 ? a[e] : b[e - 4], h, m, l, e);
}

// (element e of 8-wide fragments)
__device__ __forceinline__ void split2(float v, bf16x8& h, bf16x8& l, int e) {
  const bf16_t vh = (bf16_t)v;
  h[e] = vh; l[e] = (bf16_t)(v - (float)vh);
}
__device__ __forceinline__ void split2_store(bf16_t* hi, bf16_t* lo, f32x4 v) {
  const bf16x4 h = __builtin_convertvector(v, bf16x4);
  const bf16x4 l = __builtin_convertvector(v - __builtin_convertvector(h, f32x4), bf16x4);
  *reinterpret_cast<bf16x4*>(hi) = h; *reinterpret_cast<bf16x4*>(lo) = l;
}

// The six products of the three-way scheme as (plane of w, plane of x), planes 0 / 1 / 2 = h / m / l, in the order they are
// issued: (l, h) (h, l) (m, m) (m, h) (h, m) (h, h).  Small products first: every addition into the fp32 accumulator rounds,
// so within a k-step the terms of 2^-16 |x w| and below are added in ascending size and the full-sized h h term last, as one
// would sum any list of floats; this is the order the fp64 comparisons (tools/pwxsbench.hip, the x3 tests) were made with,
// and all kernels of a layer's routes share it.  A single-plane kernel (bf16 inference) takes entry 5 alone.
constexpr int X3_PRODUCTS = 6;
constexpr int X3_W[X3_PRODUCTS] = {2, 0, 1, 1, 0, 0}, X3_X[X3_PRODUCTS] = {0, 2, 1, 0, 1, 0};

}  // namespace jnr
