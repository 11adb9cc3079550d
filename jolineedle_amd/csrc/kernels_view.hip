// Patch gather through image views: the reference's dataset rotates an image by a multiple of 90 degrees, shifts it by
// whole pixels with zero fill and pads it bottom / right to the batch canvas (src/dataset.py:95-226, 274-278, 308-347).
// Here the augmented image never exists: a per-image descriptor (jn_image_view) says how a pixel of the logical canvas
// maps to a pixel of the stored image, and the kernel that cuts the patch applies it.  Every value is a copy (or byte ->
// b / 255 with u8_unit), so the result equals slicing the materialised canvas bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "../../include/jnroll.h"
#include "jn_kernels.h"
#include "jn_types.h"

namespace jnr {

constexpr int VG_T = 64;          // output tile edge; one workgroup of 256 threads per (patch, channel, tile)
constexpr int VG_LD = VG_T + 1;   // LDS row pitch of the transposing route: both its write and its read are conflict-free

__device__ __forceinline__ void vg_conv(float v, float& o) { o = v; }
__device__ __forceinline__ void vg_conv(uint8_t b, float& o) { o = u8_unit(b); }
__device__ __forceinline__ void vg_conv(uint8_t b, uint32_t& o) { o = b; }

// out[n, c, r, q] = canvas[c, y*P + r, x*P + q] of view image_index[n] (negative: a zero patch) at positions[n] = (y, x).
// With (y1, x1) = (Y - ty, X - tx) the canvas pixel is 0 when (Y, X) or (y1, x1) lies outside the rotated image
// (bottom / right padding, zero fill of the shift), else
//   rot 0: src[y1, x1]   90: src[Hs-1-x1, y1]   180: src[Hs-1-y1, Ws-1-x1]   270: src[x1, Ws-1-y1].
// ST -> OT: float -> float, uint8 -> float (b / 255), uint8 -> uint8.
// Routes, chosen per tile (block-uniform):
//   four elements per thread: out_vec (P, the output stride and base allow it) and an unrotated view whose shift, row
//     pitch and base keep the source groups aligned too; the identity view takes it exactly when gather_kernel<true> would;
//   along the row, one element per thread: rot 0 / 180 otherwise (180 reads the row backwards: the same cache lines);
//   transposing: rot 90 / 270, where an output row walks a source column: the source tile is read along its rows into
//     LDS and written out transposed, so that loads and stores both stay coalesced;
//   a tile without an image pixel is written as zeros and nothing is read.
template <typename ST, typename OT>
__global__ __launch_bounds__(256) void view_gather_kernel(const jn_image_view* __restrict__ views,
                                                          const long long* __restrict__ img_idx,
                                                          const long long* __restrict__ pos, OT* __restrict__ out,
                                                          long long out_sample_stride, int P, int tiles,
                                                          long long total_tiles, int out_vec,
                                                          const int* __restrict__ skip_flag, int skip_when) {
  if (skip_flag && *skip_flag >= skip_when) return;
  using LT = typename std::conditional<std::is_same<OT, float>::value, float, uint32_t>::type;
  __shared__ LT tile[VG_T * VG_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (long long tl = blockIdx.x; tl < total_tiles; tl += gridDim.x) {
    const int tq = (int)(tl % tiles), tr = (int)((tl / tiles) % tiles);
    const int c = (int)((tl / ((long long)tiles * tiles)) % 3);
    const long long n = tl / ((long long)tiles * tiles * 3);
    const int r0 = tr * VG_T, q0 = tq * VG_T;
    OT* op = out + n * out_sample_stride + (long long)c * P * P;
    const long long im = img_idx ? img_idx[n] : n;
    int rot = 0, Hs = 0, Ws = 0;
    long long oy = 0, ox = 0;                     // (y1, x1) of the tile's first pixel
    int ylo = 0, yhi = 0, xlo = 0, xhi = 0;       // rows [ylo, yhi) x columns [xlo, xhi) of the tile hold image pixels
    const ST* sp = nullptr;
    bool vec = false;
    if (im >= 0) {
      const jn_image_view v = views[im];
      rot = v.rot; Hs = v.Hs; Ws = v.Ws;
      const bool turned = rot == 90 || rot == 270;
      const long long Hr = turned ? Ws : Hs, Wr = turned ? Hs : Ws;
      const long long Y0 = pos[2 * n] * P + r0, X0 = pos[2 * n + 1] * P + q0;
      oy = Y0 - v.ty; ox = X0 - v.tx;
      sp = (const ST*)v.src + (long long)c * Hs * Ws;
      // inside the rotated image both before the shift (else canvas padding) and after it (else the shift's zero fill)
      ylo = (int)std::min<long long>(VG_T, std::max<long long>(0, -oy));
      xlo = (int)std::min<long long>(VG_T, std::max<long long>(0, -ox));
      yhi = (int)std::max<long long>(0, std::min<long long>(std::min<long long>(VG_T, P - r0), Hr - std::max(Y0, oy)));
      xhi = (int)std::max<long long>(0, std::min<long long>(std::min<long long>(VG_T, P - q0), Wr - std::max(X0, ox)));
      vec = out_vec && rot == 0 && (v.tx & 3) == 0 && (Ws & 3) == 0 && ((uintptr_t)v.src & (4 * sizeof(ST) - 1)) == 0;
    }
    const bool empty = ylo >= yhi || xlo >= xhi;
    if (!empty && (rot == 90 || rot == 270)) {
      __syncthreads();                 // the readers of the previous tile are done
      for (int b = wave; b < VG_T; b += 4) {      // lanes along the source row
        LT val = LT(0);
        if (lane >= ylo && lane < yhi && b >= xlo && b < xhi) {
          const long long y1 = oy + lane, x1 = ox + b;
          const long long srow = rot == 90 ? Hs - 1 - x1 : x1, scol = rot == 90 ? y1 : Ws - 1 - y1;
          vg_conv(sp[srow * Ws + scol], val);
        }
        tile[b * VG_LD + lane] = val;
      }
      __syncthreads();
      for (int a = wave; a < VG_T; a += 4) {      // lanes along the output row
        const int r = r0 + a, q = q0 + lane;
        if (r < P && q < P) op[(long long)r * P + q] = (OT)tile[lane * VG_LD + a];
      }
    } else if (out_vec && (vec || empty)) {
      // sixteen lanes per row; the groups of an aligned view lie wholly inside or wholly outside the image
      const int g4 = 4 * (tid & 15);
      for (int a = tid >> 4; a < VG_T; a += 16) {
        const int r = r0 + a, q = q0 + g4;
        if (r >= P || q >= P) continue;
        const bool in = !empty && a >= ylo && a < yhi && g4 >= xlo && g4 < xhi;
        const ST* s4 = sp + (oy + a) * Ws + ox + g4;
        OT* d4 = op + (long long)r * P + q;
        if constexpr (std::is_same<OT, float>::value) {
          f32x4 val = f32x4{0.f, 0.f, 0.f, 0.f};
          if (in) {
            if constexpr (std::is_same<ST, uint8_t>::value) val = u8x4_unit(*reinterpret_cast<const uint32_t*>(s4));
            else val = *reinterpret_cast<const f32x4*>(s4);
          }
          *reinterpret_cast<f32x4*>(d4) = val;
        } else {
          *reinterpret_cast<uint32_t*>(d4) = in ? *reinterpret_cast<const uint32_t*>(s4) : 0u;
        }
      }
    } else {
      for (int a = wave; a < VG_T; a += 4) {
        const int r = r0 + a, q = q0 + lane;
        if (r >= P || q >= P) continue;
        LT val = LT(0);
        if (!empty && a >= ylo && a < yhi && lane >= xlo && lane < xhi) {
          const long long y1 = oy + a, x1 = ox + lane;
          vg_conv(rot == 0 ? sp[y1 * Ws + x1] : sp[(Hs - 1 - y1) * Ws + (Ws - 1 - x1)], val);
        }
        op[(long long)r * P + q] = (OT)val;
      }
    }
  }
}

template <typename ST, typename OT>
static int launch_view_gather_t(const jn_image_view* views, const int64_t* image_index, const int64_t* positions, OT* out,
                                long long out_sample_stride, int N, int P, const int* skip_flag, int skip_when,
                                hipStream_t s) {
  const int tiles = (P + VG_T - 1) / VG_T;
  const long long total = (long long)N * 3 * tiles * tiles;
  if (total == 0) return 0;
  const int out_vec = (P % 4 == 0) && (out_sample_stride % 4 == 0) && ((uintptr_t)out % (4 * sizeof(OT)) == 0);
  const unsigned blocks = (unsigned)std::min<long long>(total, 256 * 64);
  hipLaunchKernelGGL((view_gather_kernel<ST, OT>), dim3(blocks), dim3(256), 0, s, views, (const long long*)image_index,
                     (const long long*)positions, out, out_sample_stride, P, tiles, total, out_vec, skip_flag, skip_when);
  return 0;
}

int launch_view_gather(const jn_image_view* views, int src_u8, const int64_t* image_index, const int64_t* positions,
                       void* out, int out_u8, long long out_sample_stride, int N, int P, const int* skip_flag,
                       int skip_when, hipStream_t s) {
  if (!src_u8 && out_u8) return -1;     // a byte copy of fp32 values does not exist
  if (!src_u8)
    return launch_view_gather_t<float, float>(views, image_index, positions, (float*)out, out_sample_stride, N, P,
                                              skip_flag, skip_when, s);
  if (out_u8)
    return launch_view_gather_t<uint8_t, uint8_t>(views, image_index, positions, (uint8_t*)out, out_sample_stride, N, P,
                                                  skip_flag, skip_when, s);
  return launch_view_gather_t<uint8_t, float>(views, image_index, positions, (float*)out, out_sample_stride, N, P,
                                              skip_flag, skip_when, s);
}

}  // namespace jnr
