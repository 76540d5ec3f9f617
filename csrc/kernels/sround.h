// Stochastic rounding fp32 -> bf16 with stateless, counter-based random bits
// (--stochastic-rounding; the AdamW stores of optim.hip and torch.ops.ftamd.sr_round_bf16).
//
// THE FUNCTION (mirrored exactly, integer for integer, by
// fault_tolerant_llm_training_amd/utils/sround.py -- change both or neither):
//
//   The 16 random bits of an element depend on exactly (key, step, buffer, index):
//     key    64-bit, (key_lo, key_hi) = (key & 0xffffffff, key >> 32)
//     step   optimizer step number, taken mod 2^32
//     buffer 0 params, 1 exp_avg, 2 exp_avg_sq (3: the token sampler's stream, decode.hip: index = row,
//            step = the sampler's step, first word only -- no rounding involved)
//     index  the element's global index in the flat layout, 64-bit
//
//   One generator call serves the 8 elements of vector c = index >> 3:
//     (w0, w1, w2, w3) = Philox4x32-R(counter = (c & 0xffffffff, c >> 32, step, buffer),
//                                     key = (key_lo, key_hi)),    R = SR_ROUNDS = 6
//   with the Philox4x32 round (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
//   SC'11), all words uint32, products 32 x 32 -> 64:
//     p0 = 0xD2511F53 * c0;  p1 = 0xCD9E8D57 * c2
//     (c0, c1, c2, c3) <- (hi(p1) ^ c1 ^ k0,  lo(p1),  hi(p0) ^ c3 ^ k1,  lo(p0))
//     after each round but the last: k0 += 0x9E3779B9; k1 += 0xBB67AE85
//   Element j = index & 7 of the vector takes r = (w[j >> 1] >> (16 * (j & 1))) & 0xffff.
//
//   Rounding x (fp32, bit pattern u) with r in [0, 2^16):
//     finite x:      bf16 bits = (u + r) >> 16   (a value representable in bf16 has zero low
//                    bits and is unchanged; otherwise the magnitude goes to the upper neighbour
//                    with probability (u & 0xffff) / 2^16, so the result is exact in expectation;
//                    the largest finite values may round to infinity, as round-to-nearest does)
//     non-finite x:  the round-to-nearest conversion f2bf (Inf stays Inf, a NaN stays a NaN)
//
// Nothing depends on grid size, block index or how a buffer is cut into launches, and no generator
// state lives in memory. Cost per call: 2 * R = 12 32x32->64 multiplies (v_mad_u64_u32), of
// which the first round's c2 = step product is wave-uniform; three calls per 8 parameters in AdamW.
#pragma once

#include "common.h"

constexpr int SR_ROUNDS = 6;
enum : uint32_t { SR_BUF_PARAM = 0, SR_BUF_EXP_AVG = 1, SR_BUF_EXP_AVG_SQ = 2, SR_BUF_SAMPLE = 3 };

// (key, step, offset) of a launch; c0 = offset / 8: the vector index of the launch's first vector.
struct SrArgs {
  uint32_t key_lo, key_hi, step;
  uint64_t c0;
};

__device__ __forceinline__ uint4 sr_bits8(uint32_t key_lo, uint32_t key_hi, uint32_t step,
                                          uint32_t buffer, uint64_t c) {
  uint32_t c0 = (uint32_t)c, c1 = (uint32_t)(c >> 32), c2 = step, c3 = buffer;
  uint32_t k0 = key_lo, k1 = key_hi;
#pragma unroll
  for (int r = 0; r < SR_ROUNDS; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return make_uint4(c0, c1, c2, c3);
}

// fp32 -> bf16 with the 16 random bits r (r < 2^16).
__device__ __forceinline__ bf16_t sr_bf16(float x, uint32_t r) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7f800000u) == 0x7f800000u) return f2bf(x);
  return (bf16_t)((u + r) >> 16);
}

__device__ __forceinline__ uint32_t sr_pack2(float lo, float hi, uint32_t w) {
  return (uint32_t)sr_bf16(lo, w & 0xffffu) | ((uint32_t)sr_bf16(hi, w >> 16) << 16);
}

// 8 floats of vector c -> 8 stochastically rounded bf16 (the SR twin of pack8).
__device__ __forceinline__ uint4 sr_pack8(const float* f, uint32_t key_lo, uint32_t key_hi,
                                          uint32_t step, uint32_t buffer, uint64_t c) {
  const uint4 w = sr_bits8(key_lo, key_hi, step, buffer, c);
  uint4 r;
  r.x = sr_pack2(f[0], f[1], w.x);
  r.y = sr_pack2(f[2], f[3], w.y);
  r.z = sr_pack2(f[4], f[5], w.z);
  r.w = sr_pack2(f[6], f[7], w.w);
  return r;
}
