// What the cache kernels of decode.hip (model-dtype cache) and decode_kv8.hip (FP8 cache) share: the
// chunk size, the control block of the device-step ops, a row's key count, the RoPE rotation of the
// appends, and the merge of the per-chunk partials (acc[D] unnormalised, m, l) in chunk order. Both
// files leave their partials in the same `part` layout, [chunks, Hq, D + 2], so one merge serves both.
#pragma once

#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
// keys per workgroup of decode_attn; the chunk partials are merged in chunk order
constexpr int DECODE_CHUNK = 128;

// The control block of the device-step ops: int32 words (ops/decode.py keeps the same indices). The
// host writes it once per call; the kernels only read it, but for decode_ctl_advance_ on CTL_T.
enum : int {
  CTL_T = 0,            // the decode step: new token t of the call
  CTL_KEY_LO = 1,       // the call's sampler key (token_key is formed from it and t)
  CTL_KEY_HI = 2,
  CTL_STEP = 3,         // the sampler's step
  CTL_TEMPERATURE = 4,  // float bits
  CTL_TOP_K = 5,
  CTL_TOP_P = 6,        // float bits; 0 (what a writer that knows no top-p leaves) or >= 1: off
  CTL_WORDS = 8
};

// The key count of row b of a batch: pos0[b] + t + 1, at most max_keys (which the host checked
// against Smax; pos0 itself is never read back). Below 1 no workgroup of the row does anything.
__device__ __forceinline__ int row_keys(const int* __restrict__ pos0, int b, int t, int max_keys) {
  return (int)min((long)pos0[b] + t + 1, (long)max_keys);
}

// RoPE on 8 columns of a head, four (even, odd) pairs: c and s are the cos and sin of the four pairs'
// angles. The appends of both cache formats rotate with this, so a K row has the same bits before
// either of them stores it.
__device__ __forceinline__ void rope8(const float* x, const float4& c, const float4& s, float* r) {
  const float cc[4] = {c.x, c.y, c.z, c.w}, ss[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float a = x[2 * p], b = x[2 * p + 1];
    r[2 * p] = a * cc[p] - b * ss[p];
    r[2 * p + 1] = a * ss[p] + b * cc[p];
  }
}

// One workgroup per query head, one thread per dim: the chunk partials in chunk order.
template <class E, int D>
__device__ __forceinline__ void attn_merge(const float* __restrict__ part, typename E::T* __restrict__ o, int hq,
                                           int nchunks) {
  const int h = blockIdx.x, dd = threadIdx.x;
  float M = -INFINITY, L = 0.f, A = 0.f;
  for (int c = 0; c < nchunks; ++c) {
    const float* pr = part + ((long)c * hq + h) * (D + 2);
    const float m = pr[D], l = pr[D + 1], a = pr[dd];
    const float nM = fmaxf(M, m);
    const float f0 = exp2f((M - nM) * LOG2E), f1 = exp2f((m - nM) * LOG2E);
    A = A * f0 + a * f1;
    L = L * f0 + l * f1;
    M = nM;
  }
  o[(long)h * D + dd] = cvt1<E>(A / L);
}

template <class E, int D>
__global__ __launch_bounds__(D) void decode_attn_merge_kernel(const float* __restrict__ part,
                                                              typename E::T* __restrict__ o, int hq,
                                                              int nchunks) {
  attn_merge<E, D>(part, o, hq, nchunks);
}

// Grid (Hq, B): row b folds its own ceil(keys / DECODE_CHUNK) chunks of part [B, max_chunks, Hq, D + 2].
template <class E, int D>
__device__ __forceinline__ void attn_merge_row(const float* __restrict__ part, typename E::T* __restrict__ o,
                                               const int* __restrict__ pos0, int t, int max_keys, int max_chunks,
                                               int hq) {
  const int b = blockIdx.y;
  const int n_keys = max(row_keys(pos0, b, t, max_keys), 0);
  attn_merge<E, D>(part + (long)b * max_chunks * hq * (D + 2), o + (long)b * hq * D, hq,
                   (n_keys + DECODE_CHUNK - 1) / DECODE_CHUNK);
}

template <class E, int D>
__global__ __launch_bounds__(D) void decode_attn_merge_rows_kernel(const float* __restrict__ part,
                                                                   typename E::T* __restrict__ o,
                                                                   const int* __restrict__ pos0, int t,
                                                                   int max_keys, int max_chunks, int hq) {
  attn_merge_row<E, D>(part, o, pos0, t, max_keys, max_chunks, hq);
}

template <class E, int D>
__global__ __launch_bounds__(D) void decode_attn_merge_rows_dev_kernel(const float* __restrict__ part,
                                                                       typename E::T* __restrict__ o,
                                                                       const int* __restrict__ pos0,
                                                                       const int* __restrict__ ctl, int max_keys,
                                                                       int max_chunks, int hq) {
  attn_merge_row<E, D>(part, o, pos0, ctl[CTL_T], max_keys, max_chunks, hq);
}

}  // namespace
