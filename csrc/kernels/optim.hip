// Flat-buffer gradient L2 norm + clip + fused AdamW for gfx950.
//
// Parity:
//  * grad norm / clipping: reference utils.py:58-63 (`get_total_norm` with
//    error_if_nonfinite, then `clip_grads_with_norm_`). The reference's clip is a
//    silent no-op (generator consumed twice); here clipping is
//    real: coef = min(1, max_norm / (norm + 1e-6)) is computed on device and fed
//    to the optimizer without a host sync.
//  * AdamW: torch.optim.AdamW defaults used by the reference (train.py:68):
//    betas (0.9, 0.999), eps 1e-8, decoupled weight decay 0.01, bias correction.
//    Math in fp32, storage in the parameter/state dtype (bf16 by default like
//    the reference's all-bf16 states; fp16 / fp32 under --model-dtype, moments
//    optionally fp32). A non-finite norm skips the update for
//    every element (the host raises the reference's error path afterwards).
//
// The whole model's parameters, gradients and both moments each live in ONE
// flat buffer, so a step is two reduction launches + one streaming launch over
// ~8e9 elements instead of ~300-tensor foreach chains.
#include "torch_utils.h"
#include "sround.h"
#include "stream_vec.h"

#include <vector>

#include <cstdlib>

namespace {

constexpr int NORM_BLOCKS = 2048;

template <class G, bool NT>
__global__ __launch_bounds__(256) void sumsq_kernel(const typename G::T* __restrict__ g, long n8,
                                                    float* __restrict__ partial) {
  float s = 0.f;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    float x[8];
    V8<G, NT>::load(g + i * 8, x);
#pragma unroll
    for (int j = 0; j < 8; ++j) s += x[j] * x[j];
  }
  __shared__ float red[4];
  s = block_sum<256>(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// stats[0] = ||g||, stats[1] = clip coefficient, stats[2] = 1 if non-finite.
// One 1024-thread block: the partial vector (tens of thousands of floats when the
// buckets' sums are taken during backward) is read with 16-B loads, so this
// serial step between backward and the optimizer stays a few microseconds.
__global__ __launch_bounds__(1024) void norm_finish_kernel(const float* __restrict__ partial,
                                                           int np, float extra_sumsq_scale,
                                                           float max_norm,
                                                           float* __restrict__ stats) {
  float s = 0.f;
  const int n4 = np >> 2;
  const float4* p4 = reinterpret_cast<const float4*>(partial);
  if ((reinterpret_cast<uintptr_t>(partial) & 15) == 0) {
    for (int i = threadIdx.x; i < n4; i += 1024) {
      const float4 v = p4[i];
      s += (v.x + v.y) + (v.z + v.w);
    }
    for (int i = 4 * n4 + threadIdx.x; i < np; i += 1024) s += partial[i];
  } else {
    for (int i = threadIdx.x; i < np; i += 1024) s += partial[i];
  }
  __shared__ float red[16];
  s = block_sum<1024>(s, red);
  if (threadIdx.x == 0) {
    const float norm = sqrtf(s * extra_sumsq_scale);
    stats[0] = norm;
    const bool bad = !isfinite(norm);
    stats[1] = (max_norm > 0.f && !bad) ? fminf(1.f, max_norm / (norm + 1e-6f)) : 1.f;
    // sticky: once a step's norm was non-finite every later update is skipped too, until
    // the host clears stats[2] (it only does so on an explicit reset). The trainer detects a
    // bad step two steps late without a host sync and rolls the counters back to it; the
    // parameters/moments are still exactly those before the bad step.
    stats[2] = (bad || stats[2] != 0.f) ? 1.f : 0.f;
  }
}

// SR: the stores whose storage type is bf16 round stochastically (sround.h) with the random bits of
// (sr.key, step, buffer, flat vector index sr.c0 + i); fp32 moments are stored as without it.
template <class P, class S, bool NT, bool SR>
__global__ __launch_bounds__(256) void adamw_kernel(typename P::T* __restrict__ p,
                                                    const typename P::T* __restrict__ g,
                                                    typename S::T* __restrict__ m,
                                                    typename S::T* __restrict__ v,
                                                    long n8, float lr, float omb1, float beta2,
                                                    float omb2, float eps, float wd, float inv_bc1,
                                                    float inv_sqrt_bc2,
                                                    const float* __restrict__ stats,
                                                    const float* __restrict__ hyper, int exact,
                                                    SrArgs sr) {
  if (stats[2] != 0.f) return;  // non-finite gradient norm: skip the whole update
  if (hyper != nullptr) {
    // [lr, 1/bc1, 1/sqrt(bc2)] from device memory: a HIP-graph replay of the optimizer reads
    // this step's values (the host fills the buffer before the replay) instead of the
    // scalars baked in at capture
    lr = hyper[0];
    inv_bc1 = hyper[1];
    inv_sqrt_bc2 = hyper[2];
  }
  const float coef = stats[1];
  const float decay = 1.f - lr * wd;
  const float step = lr * inv_bc1;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    float pf[8], gf[8], mf[8], vf[8];
    V8<P, NT>::load(p + i * 8, pf);
    V8<P, NT>::load(g + i * 8, gf);
    V8<S, NT>::load(m + i * 8, mf);
    V8<S, NT>::load(v + i * 8, vf);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float gj = gf[j] * coef;
      pf[j] *= decay;
      mf[j] += (gj - mf[j]) * omb1;
      vf[j] = vf[j] * beta2 + omb2 * gj * gj;
      if (exact) {  // IEEE division / sqrt (FT_EXACT_MATH A/B)
        const float denom = sqrtf(vf[j]) * inv_sqrt_bc2 + eps;
        pf[j] -= step * mf[j] / denom;
      } else {
        const float denom = fast_sqrt(vf[j]) * inv_sqrt_bc2 + eps;
        pf[j] -= step * mf[j] * fast_rcp(denom);
      }
    }
    if constexpr (SR) {
      const uint64_t c = sr.c0 + (uint64_t)i;
      V8<P, NT>::store_sr(p + i * 8, pf, sr.key_lo, sr.key_hi, sr.step, SR_BUF_PARAM, c);
      if constexpr (std::is_same<S, EBF16>::value) {
        V8<S, NT>::store_sr(m + i * 8, mf, sr.key_lo, sr.key_hi, sr.step, SR_BUF_EXP_AVG, c);
        V8<S, NT>::store_sr(v + i * 8, vf, sr.key_lo, sr.key_hi, sr.step, SR_BUF_EXP_AVG_SQ, c);
      } else {
        V8<S, NT>::store(m + i * 8, mf);
        V8<S, NT>::store(v + i * 8, vf);
      }
    } else {
      V8<P, NT>::store(p + i * 8, pf);
      V8<S, NT>::store(m + i * 8, mf);
      V8<S, NT>::store(v + i * 8, vf);
    }
  }
}

// out[i] = x[i] rounded with the random bits of (key, step, buffer, flat index 8 * c0 + i): the
// same sr_pack8 / sr_bits8 / sr_bf16 the AdamW stores use, on its own (tests, utils/sround.py's
// device twin). One 8-element vector per thread; a last partial vector element by element.
__global__ __launch_bounds__(256) void sr_round_kernel(const float* __restrict__ x,
                                                       bf16_t* __restrict__ out, long n,
                                                       uint32_t buffer, SrArgs sr) {
  const long n8 = n >> 3;
  for (long i = blockIdx.x * 256L + threadIdx.x; i * 8 < n; i += (long)gridDim.x * 256) {
    const uint64_t c = sr.c0 + (uint64_t)i;
    if (i < n8) {
      float f[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = x[i * 8 + j];
      *reinterpret_cast<uint4*>(out + i * 8) = sr_pack8(f, sr.key_lo, sr.key_hi, sr.step, buffer, c);
    } else {
      const uint4 w = sr_bits8(sr.key_lo, sr.key_hi, sr.step, buffer, c);
      const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
      for (long e = i * 8; e < n; ++e) {
        const int j = (int)(e & 7);
        out[e] = sr_bf16(x[e], (ws[j >> 1] >> (16 * (j & 1))) & 0xffffu);
      }
    }
  }
}

void launch_sumsq(const at::Tensor& grad, long n8, int nb, float* partial) {
  const bool nt = stream_nt();
  FT_DISPATCH_E(grad.scalar_type(), {
    if (nt)
      hipLaunchKernelGGL((sumsq_kernel<E, true>), dim3(nb), dim3(256), 0, ft_stream(),
                         cptr<typename E::T>(grad), n8, partial);
    else
      hipLaunchKernelGGL((sumsq_kernel<E, false>), dim3(nb), dim3(256), 0, ft_stream(),
                         cptr<typename E::T>(grad), n8, partial);
  });
}

SrArgs make_sr_args(int64_t key, int64_t step, int64_t offset) {
  SrArgs sr;
  sr.key_lo = (uint32_t)((uint64_t)key & 0xffffffffu);
  sr.key_hi = (uint32_t)((uint64_t)key >> 32);
  sr.step = (uint32_t)((uint64_t)step & 0xffffffffu);
  sr.c0 = (uint64_t)offset >> 3;
  return sr;
}

}  // namespace

// Writes [norm, coef, nonfinite] into stats (fp32[3], device).
void grad_norm_(const at::Tensor& grad, const at::Tensor& stats, double max_norm) {
  FT_CHECK_CUDA(grad);
  FT_CHECK_CONTIG(grad);
  FT_CHECK_F32(stats);
  TORCH_CHECK(grad.numel() % 8 == 0, "grad_norm: numel must be a multiple of 8");
  const at::DeviceGuard guard(grad.device());
  const long n8 = grad.numel() / 8;
  const int nb = std::max(1, std::min(NORM_BLOCKS, (int)((n8 + 255) / 256)));
  auto partial = at::empty({nb}, grad.options().dtype(at::kFloat));
  launch_sumsq(grad, n8, nb, mptr<float>(partial));
  FT_LAUNCH_CHECK();
  hipLaunchKernelGGL(norm_finish_kernel, dim3(1), dim3(1024), 0, ft_stream(), cptr<float>(partial), nb,
                     1.f, (float)max_norm, mptr<float>(stats));
  FT_LAUNCH_CHECK();
}

void adamw_(const at::Tensor& p, const at::Tensor& g, const at::Tensor& m, const at::Tensor& v,
            const at::Tensor& stats, double lr, double beta1, double beta2, double eps, double wd,
            int64_t step, int64_t max_blocks, const std::optional<at::Tensor>& hyper,
            bool stochastic_rounding, int64_t key, int64_t offset) {
  const float* hp = nullptr;
  if (hyper.has_value() && hyper->defined()) {
    FT_CHECK_F32((*hyper));
    TORCH_CHECK(hyper->is_cuda() && hyper->numel() >= 3, "adamw: hyper must be a device fp32[3]");
    // the step number of the random bits is a launch argument: a captured launch would replay one
    // step's noise for ever
    TORCH_CHECK(!stochastic_rounding, "adamw: stochastic rounding is not supported with device "
                "hyper-parameters (graph replay)");
    hp = cptr<float>(*hyper);
  }
  if (stochastic_rounding) {
    TORCH_CHECK(p.scalar_type() == at::kBFloat16,
                "adamw: stochastic rounding supports bf16 parameters only, got ", p.scalar_type());
    TORCH_CHECK(offset >= 0 && offset % 8 == 0,
                "adamw: offset (flat index of p[0]) must be a non-negative multiple of 8");
  }
  const SrArgs sr = make_sr_args(key, step, offset);
  FT_CHECK_CUDA(p);
  FT_CHECK_CONTIG(p);
  FT_CHECK_CONTIG(g);
  FT_CHECK_CONTIG(m);
  FT_CHECK_CONTIG(v);
  FT_CHECK_F32(stats);
  TORCH_CHECK(p.numel() == g.numel() && p.numel() == m.numel() && p.numel() == v.numel(),
              "adamw: size mismatch");
  TORCH_CHECK(p.numel() % 8 == 0, "adamw: numel must be a multiple of 8");
  TORCH_CHECK(p.scalar_type() == g.scalar_type() && m.scalar_type() == v.scalar_type(),
              "adamw: dtype mismatch");
  const at::DeviceGuard guard(p.device());
  const long n8 = p.numel() / 8;
  // The scalars are formed in double and rounded once, like torch AdamW's: in fp32, 1.f - 0.999f is
  // 1.3e-5 off and 1.f - (float)beta2^step as much at small steps, which on elements whose stored v
  // is near zero moved the update by more than fp32 rounding (tests/test_dtypes_gpu.py).
  const double bc1 = 1.0 - std::pow(beta1, (double)step);
  const double bc2 = 1.0 - std::pow(beta2, (double)step);
  const float inv_bc1 = (float)(1.0 / bc1), inv_sqrt_bc2 = (float)(1.0 / std::sqrt(bc2));
  const float omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);  // 1 - beta
  int nb = stream_grid(n8);
  // max_blocks > 0 overrides the default grid cap (both directions): small grids
  // leave CUs to a concurrent stream, large ones make every block short-lived so
  // the dispatcher can interleave a higher-priority stream's workgroups.
  if (max_blocks > 0) nb = (int)std::max(1L, std::min((n8 + 255) / 256, (long)max_blocks));
  const dim3 grid(nb), block(256);
  const bool nt = stream_nt();
  // parameter dtype P (= gradient dtype) in {bf16, fp16, fp32}; moments S either P or fp32
  TORCH_CHECK(m.scalar_type() == p.scalar_type() || m.scalar_type() == at::kFloat,
              "adamw: optimizer states must have the parameter dtype or fp32");
  // fp32 parameters (--model-dtype fp32) always take the IEEE division / square root: the
  // hardware v_rcp_f32 / v_sqrt_f32 (1 ulp) are below bf16/fp16 storage rounding but not below
  // fp32's, where torch AdamW's exact math is the parity target (docs/PARITY.md)
  const int exact = (int)ft_exact_math() || p.scalar_type() == at::kFloat;
  auto go = [&](auto ptag, auto stag, auto srtag) {
    using P = decltype(ptag);
    using S = decltype(stag);
    using PT = typename P::T;
    using ST = typename S::T;
    constexpr bool SR = decltype(srtag)::value;
    if (nt)
      hipLaunchKernelGGL((adamw_kernel<P, S, true, SR>), grid, block, 0, ft_stream(), mptr<PT>(p),
                         cptr<PT>(g), mptr<ST>(m), mptr<ST>(v), n8, (float)lr, omb1,
                         (float)beta2, omb2, (float)eps, (float)wd, inv_bc1, inv_sqrt_bc2,
                         cptr<float>(stats), hp, exact, sr);
    else
      hipLaunchKernelGGL((adamw_kernel<P, S, false, SR>), grid, block, 0, ft_stream(), mptr<PT>(p),
                         cptr<PT>(g), mptr<ST>(m), mptr<ST>(v), n8, (float)lr, omb1,
                         (float)beta2, omb2, (float)eps, (float)wd, inv_bc1, inv_sqrt_bc2,
                         cptr<float>(stats), hp, exact, sr);
  };
  if (stochastic_rounding) {  // bf16 parameters (checked above); moments bf16 or fp32
    if (m.scalar_type() == at::kFloat) go(EBF16{}, EF32{}, std::true_type{});
    else go(EBF16{}, EBF16{}, std::true_type{});
  } else {
    FT_DISPATCH_E(p.scalar_type(), {
      if (m.scalar_type() == at::kFloat) go(E{}, EF32{}, std::false_type{});
      else go(E{}, E{}, std::false_type{});
    });
  }
  FT_LAUNCH_CHECK();
}

// x (fp32) -> bf16 by stochastic rounding with the bits of (key, step, buffer, offset + i): the
// device function of the AdamW stores (sround.h) on its own.
at::Tensor sr_round_bf16(const at::Tensor& x, int64_t key, int64_t step, int64_t buffer, int64_t offset) {
  FT_CHECK_CUDA(x);
  FT_CHECK_CONTIG(x);
  FT_CHECK_F32(x);
  TORCH_CHECK(buffer >= 0 && buffer <= 2, "sr_round_bf16: buffer is 0 (params), 1 (exp_avg) or 2 (exp_avg_sq)");
  TORCH_CHECK(offset >= 0 && offset % 8 == 0, "sr_round_bf16: offset must be a non-negative multiple of 8");
  const at::DeviceGuard guard(x.device());
  auto out = at::empty(x.sizes(), x.options().dtype(at::kBFloat16));
  const long n = x.numel();
  if (n == 0) return out;
  const int nb = stream_grid((n + 7) / 8);
  hipLaunchKernelGGL(sr_round_kernel, dim3(nb), dim3(256), 0, ft_stream(), cptr<float>(x),
                     mptr<bf16_t>(out), n, (uint32_t)buffer, make_sr_args(key, step, offset));
  FT_LAUNCH_CHECK();
  return out;
}

// Per-bucket partial sums of squares, launched while backward is still running:
// block i of the launch writes partial[i] (grid = partial.numel()), so the total is
// a fixed-order sum independent of when each bucket finished (deterministic).
void sumsq_into_(const at::Tensor& grad, const at::Tensor& partial) {
  FT_CHECK_CUDA(grad);
  FT_CHECK_CONTIG(grad);
  FT_CHECK_F32(partial);
  FT_CHECK_CONTIG(partial);
  TORCH_CHECK(grad.numel() % 8 == 0, "sumsq_into: numel must be a multiple of 8");
  TORCH_CHECK(partial.numel() >= 1 && partial.numel() <= 65535, "sumsq_into: bad partial size");
  const at::DeviceGuard guard(grad.device());
  const long n8 = grad.numel() / 8;
  const int nb = (int)partial.numel();
  launch_sumsq(grad, n8, nb, mptr<float>(partial));
  FT_LAUNCH_CHECK();
}

// stats = [norm, clip coef, nonfinite] from a vector of partial sums of squares.
void norm_finish_(const at::Tensor& partial, const at::Tensor& stats, double max_norm) {
  FT_CHECK_CUDA(partial);
  FT_CHECK_F32(partial);
  FT_CHECK_F32(stats);
  const at::DeviceGuard guard(partial.device());
  hipLaunchKernelGGL(norm_finish_kernel, dim3(1), dim3(1024), 0, ft_stream(), cptr<float>(partial),
                     (int)partial.numel(), 1.f, (float)max_norm, mptr<float>(stats));
  FT_LAUNCH_CHECK();
}

// A stream whose kernels dispatch only to every `stride`-th CU (hipExtStreamCreateWithCUMask), for
// confining the optimizer's memory-bound AdamW launches to a slice of the chip while the next
// forward's GEMMs keep the rest (scripts/ab_step.py knob cumask). Returns the hipStream_t as an
// integer for torch.cuda.ExternalStream; the stream lives for the process.
int64_t cu_masked_stream(int64_t stride, int64_t phase) {
  TORCH_CHECK(stride >= 1 && phase >= 0 && phase < stride, "cu_masked_stream: 0 <= phase < stride");
  int dev = 0, ncu = 0;
  FT_HIP_CHECK(hipGetDevice(&dev));
  FT_HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
  for (int c = (int)phase; c < ncu; c += (int)stride) mask[c / 32] |= 1u << (c % 32);
  hipStream_t st = nullptr;
  FT_HIP_CHECK(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()));
  return reinterpret_cast<int64_t>(st);
}

TORCH_LIBRARY_FRAGMENT(ftamd, m) {
  m.def("cu_masked_stream(int stride, int phase=0) -> int", &cu_masked_stream);
  m.def("sumsq_into_(Tensor grad, Tensor(a!) partial) -> ()", &sumsq_into_);
  m.def("norm_finish_(Tensor partial, Tensor(a!) stats, float max_norm) -> ()", &norm_finish_);
  m.def("grad_norm_(Tensor grad, Tensor(a!) stats, float max_norm) -> ()", &grad_norm_);
  m.def(
      "adamw_(Tensor(a!) p, Tensor g, Tensor(b!) m, Tensor(c!) v, Tensor stats, float lr, float "
      "beta1, float beta2, float eps, float wd, int step, int max_blocks=0, Tensor? hyper=None, "
      "bool stochastic_rounding=False, int key=0, int offset=0) -> ()",
      &adamw_);
  m.def("sr_round_bf16(Tensor x_f32, int key, int step, int buffer, int offset) -> Tensor", &sr_round_bf16);
}
