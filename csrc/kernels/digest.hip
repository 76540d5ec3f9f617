// Position-weighted exact digest of a flat buffer's raw bits, for gfx950.
//
//   acc[slot] += sum_i bits(t[i]) * (((first_pos + i) mod 1_000_003) + 1)      (mod 2^64)
//
// bits = the element's raw bits, sign-extended (int16 view for bf16 / fp16, int32 view for
// fp32): exactly utils/digest.py's tensor_digest, which stays the CPU oracle. The checkpoint
// engine runs it over the snapshot of the training state (ckpt/engine.py) and the trainer over
// the restored buffers (ckpt/verify.py), so it is one read-only streaming pass: 16-B
// non-temporal loads like the optimizer's one-touch passes (optim.hip), integer math only, one
// 64-bit atomic add per block. Integer addition is exact and commutative, so the value does not
// depend on block order and pieces of one buffer accumulate into one slot.
//
// Positions are 64-bit everywhere (the 8B flat buffer has more than 2^32 elements). A thread
// divides once, to reduce its first position mod 1_000_003; the grid-stride loop then advances
// that residue by the stride's residue with a conditional subtract. Inside a 16-B vector the
// weights are consecutive, so unless the vector straddles a multiple of the modulus (one in
// ~125k vectors of 16-bit elements) the 8 products collapse to
// (r + 1) * sum_j b_j + sum_j j * b_j, both sums in 32 bits, and one 64-bit multiply-add.
#include "torch_utils.h"

namespace {

constexpr unsigned DIGEST_MOD = 1000003u;
constexpr int DIGEST_BLOCKS = 2048;

typedef unsigned int dg_u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ long long dg_wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// bits * weight for one element at residue r (0 <= r < DIGEST_MOD)
__device__ __forceinline__ long long dg_term(int bits, unsigned r) {
  return (long long)bits * (long long)(int)(r + 1u);
}

// One 16-B vector whose first element has residue r. I = short (8 elements) or int (4).
template <class I>
__device__ __forceinline__ long long dg_vec(const dg_u32x4_t q, unsigned r) {
  constexpr int VEC = 16 / (int)sizeof(I);
  int b[VEC];
  const unsigned w[4] = {q.x, q.y, q.z, q.w};
  if constexpr (sizeof(I) == 2) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      b[2 * k] = (int)(short)(w[k] & 0xffffu);
      b[2 * k + 1] = (int)w[k] >> 16;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] = (int)w[k];
  }
  long long s = 0;
  if (r + (unsigned)VEC <= DIGEST_MOD) {  // no wrap inside the vector: weights r+1 .. r+VEC
    if constexpr (sizeof(I) == 2) {
      int s0 = 0, s1 = 0;  // |s0| < 2^18, |s1| < 2^20
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        s0 += b[j];
        s1 += j * b[j];
      }
      s = (long long)s0 * (long long)(int)(r + 1u) + (long long)s1;
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) s += dg_term(b[j], r + (unsigned)j);
    }
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      unsigned rj = r + (unsigned)j;
      if (rj >= DIGEST_MOD) rj -= DIGEST_MOD;
      s += dg_term(b[j], rj);
    }
  }
  return s;
}

// p[0, head): elements before the first 16-B boundary; then nvec aligned vectors; then tail
// (< one vector) elements. res0 = first_pos mod DIGEST_MOD, stride_res = (grid * 256 * VEC) mod
// DIGEST_MOD.
template <class I>
__global__ __launch_bounds__(256) void digest_kernel(const I* __restrict__ p, long head, long nvec,
                                                     long tail, unsigned res0, unsigned stride_res,
                                                     unsigned long long* __restrict__ acc) {
  constexpr int VEC = 16 / (int)sizeof(I);
  long long s = 0;
  const I* body = p + head;
  long v = blockIdx.x * 256L + threadIdx.x;
  if (v < nvec) {
    // the one division of this thread: residue of element (head + v * VEC)
    unsigned r = (unsigned)(((unsigned long long)res0 + (unsigned long long)head +
                             (unsigned long long)v * VEC) % DIGEST_MOD);
    const long step = (long)gridDim.x * 256;
    for (; v < nvec; v += step) {
      const dg_u32x4_t q =
          __builtin_nontemporal_load(reinterpret_cast<const dg_u32x4_t*>(body + v * VEC));
      s += dg_vec<I>(q, r);
      r += stride_res;
      if (r >= DIGEST_MOD) r -= DIGEST_MOD;
    }
  }
  if (blockIdx.x == 0) {  // head and tail: fewer than VEC elements each
    const long i = threadIdx.x;
    if (i < head) {
      const unsigned r = (unsigned)(((unsigned long long)res0 + (unsigned long long)i) % DIGEST_MOD);
      s += dg_term((int)p[i], r);
    }
    if (i < tail) {
      const unsigned long long e = (unsigned long long)head + (unsigned long long)nvec * VEC + i;
      const unsigned r = (unsigned)(((unsigned long long)res0 + e) % DIGEST_MOD);
      s += dg_term((int)p[e], r);
    }
  }
  __shared__ long long red[4];
  s = dg_wave_sum(s);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) red[wid] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long t = (red[0] + red[1]) + (red[2] + red[3]);
    atomicAdd(acc, (unsigned long long)t);
  }
}

template <class I>
void launch_digest(const at::Tensor& t, long n, int64_t first_pos, unsigned long long* acc) {
  constexpr long VEC = 16 / (long)sizeof(I);
  const uintptr_t addr = reinterpret_cast<uintptr_t>(t.data_ptr());
  TORCH_CHECK(addr % sizeof(I) == 0, "digest_accum_: t is not aligned to its element size");
  const long mis = (long)((addr & 15) / sizeof(I));
  const long head = mis ? std::min(n, VEC - mis) : 0;
  const long nvec = (n - head) / VEC;
  const long tail = n - head - nvec * VEC;
  const int nb = (int)std::max(1L, std::min((long)DIGEST_BLOCKS, (nvec + 255) / 256));
  const unsigned res0 = (unsigned)((uint64_t)first_pos % DIGEST_MOD);
  const unsigned stride_res = (unsigned)(((uint64_t)nb * 256u * (uint64_t)VEC) % DIGEST_MOD);
  hipLaunchKernelGGL((digest_kernel<I>), dim3(nb), dim3(256), 0, ft_stream(), cptr<I>(t), head, nvec,
                     tail, res0, stride_res, acc);
}

}  // namespace

// acc[slot] += digest of t's elements at positions first_pos .. first_pos + t.numel() - 1.
// Enqueued on the current stream; no host sync.
void digest_accum_(const at::Tensor& acc, int64_t slot, const at::Tensor& t, int64_t first_pos) {
  FT_CHECK_CUDA(acc);
  FT_CHECK_CUDA(t);
  FT_CHECK_CONTIG(acc);
  FT_CHECK_CONTIG(t);
  TORCH_CHECK(acc.scalar_type() == at::kLong, "digest_accum_: acc must be int64");
  TORCH_CHECK(acc.device() == t.device(), "digest_accum_: acc and t must be on one device");
  TORCH_CHECK(slot >= 0 && slot < acc.numel(), "digest_accum_: slot ", slot, " out of range");
  TORCH_CHECK(first_pos >= 0, "digest_accum_: first_pos must be >= 0");
  const auto st = t.scalar_type();
  TORCH_CHECK(st == at::kBFloat16 || st == at::kHalf || st == at::kFloat,
              "digest_accum_: unsupported dtype ", st, " (bf16 / fp16 / fp32)");
  const long n = t.numel();
  if (n == 0) return;
  const at::DeviceGuard guard(t.device());
  unsigned long long* a = reinterpret_cast<unsigned long long*>(mptr<int64_t>(acc) + slot);
  if (st == at::kFloat)
    launch_digest<int>(t, n, first_pos, a);
  else
    launch_digest<short>(t, n, first_pos, a);
  FT_LAUNCH_CHECK();
}

TORCH_LIBRARY_FRAGMENT(ftamd, m) {
  m.def("digest_accum_(Tensor(a!) acc, int slot, Tensor t, int first_pos) -> ()", &digest_accum_);
}
