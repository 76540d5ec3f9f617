// 16-byte (non-temporal) vector access and grid sizing of the streaming passes over the flat
// buffers: the optimizer pass (optim.hip) and the parameter average (ema.hip).
#pragma once

#include "torch_utils.h"
#include "sround.h"

#include <algorithm>

namespace {

// 16-B vector access; NT = non-temporal (streaming) loads/stores: every byte of the
// optimizer pass is touched exactly once, so nothing is worth keeping in L2/MALL.
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ uint4 ld16(const void* p) {
  if constexpr (NT) {
    const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
  } else {
    return *reinterpret_cast<const uint4*>(p);
  }
}

template <bool NT>
__device__ __forceinline__ void st16(void* p, uint4 v) {
  if constexpr (NT) {
    const u32x4_t w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<u32x4_t*>(p));
  } else {
    *reinterpret_cast<uint4*>(p) = v;
  }
}

// 8 elements of element type E (common.h) through 16-B (non-temporal) accesses.
template <class E, bool NT>
struct V8 {
  __device__ static void load(const typename E::T* p, float* f) {
    P8<E> r;
    r.v[0] = ld16<NT>(p);
    if constexpr (!E::is16) r.v[1] = ld16<NT>(p + 4);
    unp8<E>(r, f);
  }
  __device__ static void store(typename E::T* p, const float* f) {
    const P8<E> r = pk8<E>(f);
    st16<NT>(p, r.v[0]);
    if constexpr (!E::is16) st16<NT>(p + 4, r.v[1]);
  }
  // bf16 storage only: the 8 elements of flat vector c rounded stochastically (sround.h)
  __device__ static void store_sr(typename E::T* p, const float* f, uint32_t key_lo, uint32_t key_hi,
                                  uint32_t step, uint32_t buffer, uint64_t c) {
    static_assert(std::is_same<E, EBF16>::value, "stochastic rounding: bf16 storage only");
    st16<NT>(p, sr_pack8(f, key_lo, key_hi, step, buffer, c));
  }
};

// Non-temporal loads/stores for the optimizer-pass kernels (plain ones measured slower:
// profiles/r1_stream_nt_ab.log).
[[maybe_unused]] bool stream_nt() { return true; }

// One 8-element vector per thread where possible: short-lived blocks keep more
// loads in flight than a capped grid-stride loop (5.9 vs 5.7 TB/s on MI355X,
// scripts/bw_bench.py); huge buffers still grid-stride.
[[maybe_unused]] int stream_grid(long n8) {
  long g = (n8 + 255) / 256;
  return (int)std::max(1L, std::min(g, 65535L));
}

}  // namespace
