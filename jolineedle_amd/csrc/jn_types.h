// Storage types of activation buffers and the 4-wide load/store helpers every kernel uses.
// fp32 = the reference's dtype (parity mode); bf16 = MI355X performance mode (activations stored in
// bf16, accumulation / statistics / weights master copy in fp32, 1x1 convs on bf16 MFMA).
#pragma once
#include <hip/hip_runtime.h>

namespace jnr {

using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef __bf16 bf16_t;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 ld4(const bf16_t* p) {
  return __builtin_convertvector(*reinterpret_cast<const bf16x4*>(p), f32x4);
}
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void st4(bf16_t* p, f32x4 v) {
  *reinterpret_cast<bf16x4*>(p) = __builtin_convertvector(v, bf16x4);
}
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const bf16_t* p) { return (float)*p; }
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(bf16_t* p, float v) { *p = (bf16_t)v; }

// uint8 images: byte b stands for b / 255 correctly rounded (ToTensor's u8.float().div(255)).  The product with
// fl(1/255) is wrong in the last bit for 126 of the 256 bytes; one residual step (the fma residual is exact) makes it
// right for all 256 (tests/test_uint8_images_cpu.py checks the arithmetic, tests/test_gpu_uint8_images.py the device).
__device__ __forceinline__ float u8_unit(uint32_t b) {
#pragma clang fp contract(off)
  const float x = (float)b;
  const float q = x * (1.0f / 255.0f);
  return __builtin_fmaf(__builtin_fmaf(-q, 255.0f, x), 1.0f / 255.0f, q);
}
// four bytes of one 32-bit load (little endian: byte 0 = lowest address) -> four values (v_cvt_f32_ubyte0..3)
__device__ __forceinline__ f32x4 u8x4_unit(uint32_t u) {
  return f32x4{u8_unit(u & 0xffu), u8_unit((u >> 8) & 0xffu), u8_unit((u >> 16) & 0xffu), u8_unit(u >> 24)};
}
// Prefetch registers of the kernels that read the image (ST = float or uint8_t): an fp32 image is held as values, a
// uint8 image as its raw bytes (one per register, or a 32-bit group of four), converted when written to LDS so that the
// conversion does not wait for the loads in flight.
template <typename ST> struct SrcRegs { using one = float; using four = f32x4; };
template <> struct SrcRegs<uint8_t> { using one = uint32_t; using four = uint32_t; };
__device__ __forceinline__ float src_unit(float v) { return v; }
__device__ __forceinline__ float src_unit(uint32_t b) { return u8_unit(b); }
__device__ __forceinline__ f32x4 src_unit4(f32x4 v) { return v; }
__device__ __forceinline__ f32x4 src_unit4(uint32_t u) { return u8x4_unit(u); }

// One MFMA operand fragment of v_mfma_f32_16x16x32_bf16 (8 consecutive k of the lane's row / column) out of a [k][channel]
// bf16 tile in LDS: two ds_read_b64_tr_b16.  Per 16-lane group the hardware reads 4 k-rows x 16 channels and hands every
// lane ITS channel's four values; lane 4 q + p of the group supplies the address of row q, channels 4 p .. 4 p + 3
// (8-byte aligned).  r0 / r1: this lane's addresses for k 0..3 / 4..7 of its octet.  EXEC must be all ones.
typedef __attribute__((ext_vector_type(4))) short tr_s4;
__device__ __forceinline__ bf16x8 tr_frag(const bf16_t* r0, const bf16_t* r1) {
  const tr_s4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_s4 __attribute__((address_space(3)))*)r0);
  const tr_s4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_s4 __attribute__((address_space(3)))*)r1);
  typedef __attribute__((ext_vector_type(8))) short s8;
  const s8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(bf16x8, v);
}

}  // namespace jnr
