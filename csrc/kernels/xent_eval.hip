// Evaluation cross-entropy: per-row NLL and top-1 hit of [T, V] logits, summed into four int64
// counters. Forward only: the logits are read once and nothing is written per row or per element
// (no lse, no dlogits). The reference has no evaluation (its train.py only ever logs the loss of
// the batch it trained on); the math is its training loss, train.py:101-102, per token.
//
// The row's NLL repeats xent_fwd_kernel (xent.hip) operation for operation -- the same per-thread
// sweep, the same wave and block merges -- so it is bit-identical to xent_fwd's loss[row]. It is
// then rounded to fixed point, fx = rint(nll * 2^24) (the scaling is exact in fp32, the rounding to
// nearest even), and summed as an integer: integer sums are exact and independent of order, so the
// counters do not depend on block scheduling, on how the rows were chunked or on which rank saw
// which row.
//
//   acc[0] += fx    acc[1] += 1 (token)    acc[2] += hit    acc[3] += 1 for a row left out
//
// hit: the label is the LOWEST column index that attains the row maximum (bf16 logits tie often).
// Left out (acc[3] only): a row whose NLL is not finite or does not fit the fixed point
// (|nll| >= 2^38), or whose label lies outside [0, V). Rows with label == ignore_index add nothing.
// One 256-thread block per row, rows grid-strided; each block adds its counters once at the end
// with plain vector atomics.
#include <climits>

#include "torch_utils.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int EVAL_MAX_BLOCKS = 32768;
constexpr float FX_SCALE = 16777216.f;       // 2^24
constexpr float FX_NLL_LIMIT = 274877906944.f;  // 2^38: fx stays below 2^62

// Bit-identity with xent_fwd's loss[row] needs the roundings of xent_fwd_kernel as it is compiled,
// not only its source: there the compiler contracts two of the multiply-adds into one fused
// operation (the sweep's s * e + acc and the block merge's S += ssum * e) and leaves the wave
// merge's two products and their sum separate. Here those two are written as explicit fused
// multiply-adds and the merges are compiled with contraction off, so the choice does not depend
// on the code around them (tests/test_eval_gpu.py compares the two kernels bit for bit). What may
// still differ is inside exp2f: its range step for results below 2^-126 adds 64 to the argument,
// fused with the * LOG2E or not. Only terms below 2^-126 can change, and every sum they enter has
// a leading term of at least 1 (the exponential of the maximum itself), which absorbs them.
//
// Top-1 without an arg-max: the label is the lowest column of the row maximum iff no column holds
// a larger value than the label's and no lower column an equal one. The label's logit is read
// first; the sweep then needs one compare of each vector's maximum (which it has anyway) and
// looks at single columns only in a vector whose maximum equals the label's logit.
template <class E>
__global__ __launch_bounds__(256) void xent_eval_kernel(const typename E::T* __restrict__ logits,
                                                        const int64_t* __restrict__ labels,
                                                        unsigned long long* __restrict__ acc, int V, int T,
                                                        int ignore_index) {
  __shared__ float sm[4], ssum[4];
  __shared__ int sbeat[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  unsigned long long fx_sum = 0;  // thread 0's counters over the rows of this block (int64, wrapping)
  unsigned tokens = 0, hits = 0, left_out = 0;
  for (int row = blockIdx.x; row < T; row += gridDim.x) {
    const int64_t y = labels[row];  // the same for every thread of the block
    if (y == ignore_index) continue;
    if (y < 0 || y >= V) {
      ++left_out;
      continue;
    }
    const typename E::T* lr = logits + (long)row * V;
    const float xy = ld1<E>(lr + y);
    const int yc = (int)y;
    float m = -INFINITY, s = 0.f;
    bool beat = false;  // a column of this thread takes the top-1 from the label
    for (int c = threadIdx.x * 8; c < V; c += 256 * 8) {
      float x[8];
      ld8<E>(lr + c, x);
      float lm = x[0];
#pragma unroll
      for (int j = 1; j < 8; ++j) lm = fmaxf(lm, x[j]);
      const float nm = fmaxf(m, lm);
      if (nm != -INFINITY) {  // all -inf so far: s stays 0 (x - nm would be NaN), as in the merge below
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) a += exp2f((x[j] - nm) * LOG2E);
        s = __builtin_fmaf(s, exp2f((m - nm) * LOG2E), a);
        m = nm;
      }
      beat |= lm > xy;
      if (lm == xy && c < yc) {  // a tie with the label: only a lower column wins
#pragma unroll
        for (int j = 0; j < 8; ++j) beat |= (x[j] == xy) && (c + j < yc);
      }
    }
    {
#pragma clang fp contract(off)
      // wave-level merge of (m, s)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
        const float nm = fmaxf(m, om);
        s = (m == -INFINITY ? 0.f : s * exp2f((m - nm) * LOG2E)) +
            (om == -INFINITY ? 0.f : os * exp2f((om - nm) * LOG2E));
        m = nm;
      }
    }
    const bool wave_beat = __any(beat);
    if (lane == 0) {
      sm[wid] = m;
      ssum[wid] = s;
      sbeat[wid] = wave_beat;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)
      float M = sm[0];
      for (int i = 1; i < 4; ++i) M = fmaxf(M, sm[i]);
      float S = 0.f;
      for (int i = 0; i < 4; ++i) S = __builtin_fmaf(ssum[i], exp2f((sm[i] - M) * LOG2E), S);
      const float l = M + logf(S);
      const float nll = l - xy;
      if (fabsf(nll) < FX_NLL_LIMIT) {  // false for NaN and +-inf too
        fx_sum += (unsigned long long)(long long)rintf(nll * FX_SCALE);
        ++tokens;
        hits += (sbeat[0] | sbeat[1] | sbeat[2] | sbeat[3]) ? 0u : 1u;
      } else {
        ++left_out;
      }
    }
    __syncthreads();  // the next row's partials reuse the shared arrays
  }
  if (threadIdx.x == 0) {
    if (tokens) {
      atomicAdd(acc + 0, fx_sum);  // two's complement: the int64 sum
      atomicAdd(acc + 1, (unsigned long long)tokens);
    }
    if (hits) atomicAdd(acc + 2, (unsigned long long)hits);
    if (left_out) atomicAdd(acc + 3, (unsigned long long)left_out);
  }
}

}  // namespace

// acc[0..3] += (sum of fixed-point NLL, tokens, top-1 hits, rows left out) of the rows of `logits`.
void xent_eval_(const at::Tensor& logits, const at::Tensor& labels, const at::Tensor& acc,
                int64_t ignore_index) {
  FT_CHECK_CUDA(logits);
  FT_CHECK_MODEL_DTYPE(logits);
  FT_CHECK_CONTIG(logits);
  FT_CHECK_CUDA(labels);
  FT_CHECK_CONTIG(labels);
  FT_CHECK_CUDA(acc);
  FT_CHECK_CONTIG(acc);
  TORCH_CHECK(labels.scalar_type() == at::kLong, "xent_eval_: labels must be int64");
  TORCH_CHECK(acc.scalar_type() == at::kLong && acc.numel() == 4, "xent_eval_: acc must be int64 [4]");
  TORCH_CHECK(labels.device() == logits.device() && acc.device() == logits.device(),
              "xent_eval_: logits, labels and acc must be on one device");
  TORCH_CHECK(logits.dim() >= 1 && logits.size(-1) > 0, "xent_eval_: logits must be [T, V]");
  const int64_t V = logits.size(-1);
  TORCH_CHECK(V % 8 == 0, "xent_eval_: vocab must be a multiple of 8");
  const int64_t T = logits.numel() / V;
  TORCH_CHECK(V <= INT_MAX && T <= INT_MAX, "xent_eval_: T and V must fit 32 bits");
  TORCH_CHECK(labels.numel() == T, "xent_eval_: labels shape mismatch");
  const at::DeviceGuard guard(logits.device());
  if (T > 0)
    FT_DISPATCH_E(logits.scalar_type(),
                  hipLaunchKernelGGL(xent_eval_kernel<E>, dim3((unsigned)std::min<int64_t>(T, EVAL_MAX_BLOCKS)),
                                     dim3(256), 0, ft_stream(), cptr<typename E::T>(logits),
                                     cptr<int64_t>(labels), mptr<unsigned long long>(acc), (int)V, (int)T,
                                     (int)ignore_index));
  FT_LAUNCH_CHECK();
}

TORCH_LIBRARY_FRAGMENT(ftamd, m) {
  m.def("xent_eval_(Tensor logits, Tensor labels, Tensor(a!) acc, int ignore_index) -> ()", &xent_eval_);
}
