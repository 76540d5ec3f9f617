// OCP e4m3fn (torch.float8_e4m3fn: 4 exponent bits, bias 7, 3 mantissa bits, max 448, no infinity,
// NaN = 0x7f / 0xff) in registers, through gfx950's packed converts. The definition of the format's
// use here -- one fp32 scale per weight row -- is utils/fp8.py.
//
//   decode   v_cvt_pk_f32_fp8: two codes of a 32-bit word (its low or its high half) to two fp32.
//            Exact: every e4m3 value, subnormals included, is an fp32 value.
//   encode   v_cvt_pk_fp8_f32: two fp32 to two codes, round to nearest even, into one half of a
//            word. The definition's values never exceed 448 (1 + 2^-23), which rounds to 448, so
//            the instruction's overflow handling is never reached.
#pragma once

#include "common.h"

typedef float f32x2_t __attribute__((ext_vector_type(2)));

// 4 codes of one 32-bit word, byte 0 first.
__device__ __forceinline__ void fp8x4_to_f32(uint32_t w, float* f) {
  const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  f[0] = lo.x;
  f[1] = lo.y;
  f[2] = hi.x;
  f[3] = hi.y;
}

// 16 codes of one 16-byte vector, in memory order.
__device__ __forceinline__ void fp8x16_to_f32(const uint4& v, float* f) {
  fp8x4_to_f32(v.x, f);
  fp8x4_to_f32(v.y, f + 4);
  fp8x4_to_f32(v.z, f + 8);
  fp8x4_to_f32(v.w, f + 12);
}

// Two fp32 to two codes (a in the low byte), RNE. The sign of a zero result is taken from the
// operand explicitly, so -0 and every negative value that rounds to zero give 0x80 whatever the
// instruction does with the sign of a zero.
__device__ __forceinline__ uint32_t f32x2_to_fp8(float a, float b) {
  uint32_t w = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false) & 0xffffu;
  const uint32_t sa = (__float_as_uint(a) >> 24) & 0x80u, sb = (__float_as_uint(b) >> 16) & 0x8000u;
  if ((w & 0x7fu) == 0u) w = (w & 0xff00u) | sa;
  if ((w & 0x7f00u) == 0u) w = (w & 0x00ffu) | sb;
  return w;
}

// 4 fp32 to one 32-bit word of codes, f[0] in byte 0.
__device__ __forceinline__ uint32_t f32x4_to_fp8(const float* f) {
  return f32x2_to_fp8(f[0], f[1]) | (f32x2_to_fp8(f[2], f[3]) << 16);
}

// The row rule of utils/fp8.py from m, the bit pattern of the row's amax = max |x| (as an integer: for
// non-negative floats the integer order is the float order, infinity and every NaN above all finite
// values): code = e4m3_rne(x * inv), value = code * scale. amax == 0: scale 1, the codes are the signed
// zeros of the row. A non-finite row: NaN scale, and the caller stores zero codes. inv is capped at the
// largest float: below amax = 448 / FLT_MAX the quotient overflows. The weight quantizer and the KV
// cache both quantize by this, so the two formats cannot drift apart.
struct E4m3Row {
  bool finite;
  float inv, scale;
};

__device__ __forceinline__ E4m3Row e4m3_row(uint32_t m) {
  E4m3Row r{m < 0x7f800000u, 0.f, __uint_as_float(0x7fc00000u)};
  const float amax = __uint_as_float(m);
  if (r.finite) {
    r.inv = m == 0u ? 1.f : fminf(__fdiv_rn(448.f, amax), 3.402823466e+38f);
    r.scale = m == 0u ? 1.f : __fdiv_rn(amax, 448.f);
  }
  return r;
}

// s * scale (+ residual): separately rounded fp32 operations. Each result passes an opaque register
// barrier (the empty asm of common.h's pin8), so the compiler can neither contract the two into one
// fma nor merge the last of them with the caller's conversion to fp16 into a mixed-precision fma
// (v_fma_mixlo_f16), which rounds once where the definition rounds to fp32 first.
template <class E>
__device__ __forceinline__ float scaled(float s, float scale, const typename E::T* res) {
  float v = s * scale;
  asm volatile("" : "+v"(v));
  if (res != nullptr) {
    v = v + ld1<E>(res);
    asm volatile("" : "+v"(v));
  }
  return v;
}
