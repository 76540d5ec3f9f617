// Segmented one-pass statistics of a flat buffer, for gfx950.
//
// For every segment (offset, numel) of a table, over the segment's elements x:
//
//   out[s] = [ sum of x^2 over the finite x,  max |x| over the finite x (0 if none),
//              number of NaN / +-Inf,          number of +-0 ]                       (float64)
//
// The flat state (models/flat.py) keeps every parameter, gradient and moment as one contiguous range
// of a huge buffer, so the per-parameter numbers of a whole buffer are one read-only streaming pass
// with a segment table: 16-B non-temporal loads over the aligned body of each work item and scalar
// head / tail elements, like digest.hip. Elements outside every segment are never read.
//
// Squares: bf16^2 exceeds the fp32 range and a bf16 subnormal squared underflows it, so every
// element is widened to fp64, where x*x is exact for bf16 / fp16 / fp32 (at most 24 significant
// bits, exponent range +-300), and accumulated in fp64: for n elements the sum errs by at most
// (n-1) * 2^-53 relative, in any order (all terms are >= 0). |x| is compared as the integer value
// of its bits (monotonic for finite non-negative floats): exact, and no denormal mode matters.
//
// Determinism: segment_stats_plan cuts every segment into work items of at most `chunk` elements;
// one block per item writes its four partial values with plain stores, and a second kernel folds the
// items of a segment in a fixed order (one wave per segment: lane l adds items l, l+64, ... in
// item order, then a fixed xor tree). No atomics. absmax and the two counts are exact; sumsq is
// bit-reproducible for a given (segment table, chunk, 16-byte phase of the buffer's address).
//
// All positions are 64-bit (the 8B flat buffer has more than 2^32 elements).
#include <algorithm>
#include <tuple>

#include "torch_utils.h"

namespace {

constexpr int64_t TS_CHUNK = 1 << 18;  // elements per work item (profiles/tensor_stats.md)
constexpr int TS_THREADS = 256;

typedef unsigned int ts_u32x4_t __attribute__((ext_vector_type(4)));

struct TsAcc {
  double s0, s1;      // sum of squares, even / odd elements of the thread's sequence
  unsigned amax;      // largest |x| of the finite elements, as raw bits of the element type
  unsigned nonfinite;
  unsigned zeros;
};

// Element classes from raw bits. K = 0: bf16, 1: fp16, 2: fp32.
template <int K>
struct TsFmt;
template <>
struct TsFmt<0> {
  typedef uint16_t T;
  static constexpr unsigned ABS = 0x7fffu, EXP = 0x7f80u;
  static __device__ __forceinline__ double widen(unsigned a) { return (double)__uint_as_float(a << 16); }
};
template <>
struct TsFmt<1> {
  typedef uint16_t T;
  static constexpr unsigned ABS = 0x7fffu, EXP = 0x7c00u;
  static __device__ __forceinline__ double widen(unsigned a) {
    return (double)(float)__builtin_bit_cast(_Float16, (uint16_t)a);
  }
};
template <>
struct TsFmt<2> {
  typedef float T;
  static constexpr unsigned ABS = 0x7fffffffu, EXP = 0x7f800000u;
  static __device__ __forceinline__ double widen(unsigned a) { return (double)__uint_as_float(a); }
};

// one element, raw bits `b` (zero-extended); `odd` picks the accumulator
template <int K>
__device__ __forceinline__ void ts_elem(unsigned b, bool odd, TsAcc& t) {
  typedef TsFmt<K> F;
  const unsigned a = b & F::ABS;
  const bool fin = (a & F::EXP) != F::EXP;
  t.nonfinite += fin ? 0u : 1u;
  t.zeros += a == 0u ? 1u : 0u;
  const unsigned af = fin ? a : 0u;
  t.amax = af > t.amax ? af : t.amax;
  const double d = F::widen(af);  // |x| (the square is the same), 0 for a non-finite element
  if (odd)
    t.s1 = __builtin_fma(d, d, t.s1);
  else
    t.s0 = __builtin_fma(d, d, t.s0);
}

template <int K>
__device__ __forceinline__ void ts_vec(const ts_u32x4_t q, TsAcc& t) {
  const unsigned w[4] = {q.x, q.y, q.z, q.w};
  if constexpr (K == 2) {
#pragma unroll
    for (int k = 0; k < 4; ++k) ts_elem<K>(w[k], k & 1, t);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ts_elem<K>(w[k] & 0xffffu, false, t);
      ts_elem<K>(w[k] >> 16, true, t);
    }
  }
}

__device__ __forceinline__ double ts_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double ts_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// One block per work item: items[2 * i] = first element, items[2 * i + 1] = length (<= 2^31 - 1),
// inside the n elements of p.
// partial[4 * i ..] = sumsq, absmax, nonfinite, zeros of the item.
template <int K>
__global__ __launch_bounds__(TS_THREADS) void segment_stats_items_kernel(
    const typename TsFmt<K>::T* __restrict__ p, long n, const long* __restrict__ items,
    double* __restrict__ partial) {
  typedef typename TsFmt<K>::T T;
  constexpr int VEC = 16 / (int)sizeof(T);
  const long item = blockIdx.x;
  const long first = items[2 * item], want = items[2 * item + 1];
  // a table that is not this buffer's plan reads nothing rather than past the end
  const bool inside = first >= 0 && want >= 0 && want < (1L << 31) && first <= n && want <= n - first;
  const T* base = p + (inside ? first : 0);
  const int len = inside ? (int)want : 0;
  const int mis = (int)((reinterpret_cast<uintptr_t>(base) & 15) / sizeof(T));
  const int head = mis ? min(len, VEC - mis) : 0;
  const int nvec = (len - head) / VEC;
  const int tail = len - head - nvec * VEC;
  const ts_u32x4_t* body = reinterpret_cast<const ts_u32x4_t*>(base + head);
  TsAcc t = {0.0, 0.0, 0u, 0u, 0u};
  int v = threadIdx.x;
  // four independent 16-B loads in flight per thread
  for (; v + 3 * TS_THREADS < nvec; v += 4 * TS_THREADS) {
    const ts_u32x4_t q0 = __builtin_nontemporal_load(body + v);
    const ts_u32x4_t q1 = __builtin_nontemporal_load(body + v + TS_THREADS);
    const ts_u32x4_t q2 = __builtin_nontemporal_load(body + v + 2 * TS_THREADS);
    const ts_u32x4_t q3 = __builtin_nontemporal_load(body + v + 3 * TS_THREADS);
    ts_vec<K>(q0, t);
    ts_vec<K>(q1, t);
    ts_vec<K>(q2, t);
    ts_vec<K>(q3, t);
  }
  for (; v < nvec; v += TS_THREADS) ts_vec<K>(__builtin_nontemporal_load(body + v), t);
  {  // head and tail: fewer than VEC elements each
    const int i = threadIdx.x;
    unsigned b = 0;
    if (i < head) {
      __builtin_memcpy(&b, base + i, sizeof(T));
      ts_elem<K>(sizeof(T) == 2 ? (b & 0xffffu) : b, false, t);
    }
    if (i < tail) {
      __builtin_memcpy(&b, base + head + nvec * VEC + i, sizeof(T));
      ts_elem<K>(sizeof(T) == 2 ? (b & 0xffffu) : b, false, t);
    }
  }
  __shared__ double red[4][4];
  const double s = ts_wave_sum(t.s0 + t.s1);
  const double m = ts_wave_max(TsFmt<K>::widen(t.amax));
  const double nf = ts_wave_sum((double)t.nonfinite);  // integers below 2^53: exact
  const double z = ts_wave_sum((double)t.zeros);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    red[wid][0] = s;
    red[wid][1] = m;
    red[wid][2] = nf;
    red[wid][3] = z;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = partial + 4 * item;
    o[0] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    o[1] = fmax(fmax(red[0][1], red[1][1]), fmax(red[2][1], red[3][1]));
    o[2] = (red[0][2] + red[1][2]) + (red[2][2] + red[3][2]);
    o[3] = (red[0][3] + red[1][3]) + (red[2][3] + red[3][3]);
  }
}

// One wave per segment: the items seg_first[s] .. seg_first[s + 1] - 1 of segment s, folded in a
// fixed order. A segment without items (numel 0) gets zeros.
__global__ __launch_bounds__(TS_THREADS) void segment_stats_fold_kernel(const double* __restrict__ partial,
                                                                       const long* __restrict__ seg_first,
                                                                       long nseg, long nitems,
                                                                       double* __restrict__ out) {
  const long s = blockIdx.x * (long)(TS_THREADS / 64) + (threadIdx.x >> 6);
  if (s >= nseg) return;  // whole waves leave together
  const int lane = threadIdx.x & 63;
  const long lo = max(0L, seg_first[s]), hi = min(nitems, seg_first[s + 1]);
  double a = 0.0, m = 0.0, nf = 0.0, z = 0.0;
  for (long i = lo + lane; i < hi; i += 64) {
    const double* q = partial + 4 * i;
    a += q[0];
    m = fmax(m, q[1]);
    nf += q[2];
    z += q[3];
  }
  a = ts_wave_sum(a);
  m = ts_wave_max(m);
  nf = ts_wave_sum(nf);
  z = ts_wave_sum(z);
  if (lane == 0) {
    double* o = out + 4 * s;
    o[0] = a;
    o[1] = m;
    o[2] = nf;
    o[3] = z;
  }
}

void check_table(const char* what, const at::Tensor& t, const at::Tensor& buf, int64_t numel) {
  TORCH_CHECK(t.is_cuda() && t.device() == buf.device(), "segment_stats_: ", what, " must be on buf's device");
  TORCH_CHECK(t.is_contiguous(), "segment_stats_: ", what, " must be contiguous");
  TORCH_CHECK(t.numel() == numel, "segment_stats_: ", what, " has ", t.numel(), " elements, the plan needs ", numel);
}

}  // namespace

int64_t segment_stats_chunk() { return TS_CHUNK; }

// The work table of a segment table (CPU int64 tensors, [nseg] each): segments sorted by offset,
// disjoint, gaps allowed. Returns CPU int64 tensors (items [nitems, 2] = (first element, length),
// seg_first [nseg + 1]) and the end of the last segment, which segment_stats_ holds against the
// buffer's length. chunk <= 0: the built-in size.
std::tuple<at::Tensor, at::Tensor, int64_t> segment_stats_plan(const at::Tensor& offsets, const at::Tensor& numels,
                                                               int64_t chunk) {
  TORCH_CHECK(offsets.is_cpu() && numels.is_cpu(), "segment_stats_plan: offsets / numels are CPU tensors");
  TORCH_CHECK(offsets.scalar_type() == at::kLong && numels.scalar_type() == at::kLong,
              "segment_stats_plan: offsets / numels must be int64");
  TORCH_CHECK(offsets.dim() == 1 && numels.dim() == 1 && offsets.numel() == numels.numel(),
              "segment_stats_plan: offsets / numels must be 1-D and of one length");
  if (chunk <= 0) chunk = TS_CHUNK;
  TORCH_CHECK(chunk < (int64_t(1) << 31), "segment_stats_plan: chunk ", chunk, " must be below 2^31");
  const at::Tensor offc = offsets.contiguous(), numc = numels.contiguous();
  const int64_t nseg = offc.numel();
  const int64_t* off = offc.data_ptr<int64_t>();
  const int64_t* num = numc.data_ptr<int64_t>();
  int64_t end = 0, nitems = 0;
  for (int64_t s = 0; s < nseg; ++s) {
    TORCH_CHECK(off[s] >= 0 && num[s] >= 0, "segment_stats_plan: segment ", s, " has a negative offset or length");
    TORCH_CHECK(num[s] <= (int64_t(1) << 62) - off[s], "segment_stats_plan: segment ", s, " is out of range");
    TORCH_CHECK(off[s] >= end, "segment_stats_plan: segment ", s, " at ", off[s],
                " starts before the end of the segments ahead of it (", end, "): the table must be sorted by offset "
                "and disjoint");
    end = off[s] + num[s];
    nitems += (num[s] + chunk - 1) / chunk;
  }
  at::Tensor items = at::empty({nitems, 2}, at::kLong);
  at::Tensor first = at::empty({nseg + 1}, at::kLong);
  int64_t* it = items.data_ptr<int64_t>();
  int64_t* fs = first.data_ptr<int64_t>();
  int64_t k = 0;
  for (int64_t s = 0; s < nseg; ++s) {
    fs[s] = k;
    for (int64_t lo = 0; lo < num[s]; lo += chunk, ++k) {
      it[2 * k] = off[s] + lo;
      it[2 * k + 1] = std::min(chunk, num[s] - lo);
    }
  }
  fs[nseg] = k;
  return std::make_tuple(items, first, end);
}

// out[s] = the four statistics of segment s of buf, for the device copies of a segment_stats_plan
// table; `extent` is the plan's end of the last segment. partial: the plan's scratch ([nitems, 4]
// float64). Two launches on the current stream; no host sync, no copy.
void segment_stats_(const at::Tensor& buf, const at::Tensor& items, const at::Tensor& seg_first, int64_t extent,
                    const at::Tensor& partial, const at::Tensor& out) {
  FT_CHECK_CUDA(buf);
  TORCH_CHECK(buf.is_contiguous() && buf.dim() == 1, "segment_stats_: buf must be a contiguous 1-D buffer");
  const auto st = buf.scalar_type();
  TORCH_CHECK(st == at::kBFloat16 || st == at::kHalf || st == at::kFloat, "segment_stats_: unsupported dtype ", st,
              " (bf16 / fp16 / fp32)");
  TORCH_CHECK(extent >= 0 && extent <= buf.numel(), "segment_stats_: the segments end at element ", extent,
              ", past the end of the buffer (", buf.numel(), " elements)");
  TORCH_CHECK(items.scalar_type() == at::kLong && seg_first.scalar_type() == at::kLong,
              "segment_stats_: items / seg_first must be int64");
  TORCH_CHECK(partial.scalar_type() == at::kDouble && out.scalar_type() == at::kDouble,
              "segment_stats_: partial / out must be float64");
  TORCH_CHECK(seg_first.numel() >= 1, "segment_stats_: seg_first must hold nseg + 1 entries");
  const int64_t nseg = seg_first.numel() - 1;
  const int64_t nitems = items.numel() / 2;
  check_table("items", items, buf, 2 * nitems);
  check_table("seg_first", seg_first, buf, nseg + 1);
  check_table("partial", partial, buf, 4 * nitems);
  check_table("out", out, buf, 4 * nseg);
  TORCH_CHECK(nitems < (int64_t(1) << 31), "segment_stats_: too many work items (", nitems, ")");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(buf.data_ptr()) % buf.element_size() == 0,
              "segment_stats_: buf is not aligned to its element size");
  if (nseg == 0) return;
  const at::DeviceGuard guard(buf.device());
  const long* it = cptr<long>(items);
  double* part = mptr<double>(partial);
  if (nitems > 0) {
    const dim3 grid((unsigned)nitems), block(TS_THREADS);
    if (st == at::kBFloat16)
      hipLaunchKernelGGL((segment_stats_items_kernel<0>), grid, block, 0, ft_stream(), cptr<uint16_t>(buf), (long)buf.numel(), it, part);
    else if (st == at::kHalf)
      hipLaunchKernelGGL((segment_stats_items_kernel<1>), grid, block, 0, ft_stream(), cptr<uint16_t>(buf), (long)buf.numel(), it, part);
    else
      hipLaunchKernelGGL((segment_stats_items_kernel<2>), grid, block, 0, ft_stream(), cptr<float>(buf), (long)buf.numel(), it, part);
    FT_LAUNCH_CHECK();
  }
  const int per_block = TS_THREADS / 64;
  hipLaunchKernelGGL(segment_stats_fold_kernel, dim3((unsigned)((nseg + per_block - 1) / per_block)),
                     dim3(TS_THREADS), 0, ft_stream(), part, cptr<long>(seg_first), (long)nseg,
                     (long)nitems, mptr<double>(out));
  FT_LAUNCH_CHECK();
}

TORCH_LIBRARY_FRAGMENT(ftamd, m) {
  m.def("segment_stats_chunk() -> int", &segment_stats_chunk);
  m.def("segment_stats_plan(Tensor offsets, Tensor numels, int chunk=0) -> (Tensor, Tensor, int)",
        &segment_stats_plan);
  m.def("segment_stats_(Tensor buf, Tensor items, Tensor seg_first, int extent, Tensor(a!) partial, Tensor(b!) out) -> ()",
        &segment_stats_);
}
