// Exponential moving average of the flat parameter buffer (--ema-decay) for gfx950.
//
// e' = e + (p - e) * (1 - d), element by element, in three separately rounded fp32 operations
// (utils/ema.py is the definition and the CPU path; the result here equals it bit for bit). The
// average is fp32 whatever the parameter dtype: at d = 0.999 the increment is far below half a bf16
// spacing. Absent in the reference.
//
// A streaming pass like adamw_kernel (optim.hip): one 8-element vector per thread, 16-B loads of p,
// two 16-B loads and stores of e, 10 bytes per element with bf16 / fp16 parameters. It is a kernel of
// its own, not part of adamw_kernel: --ema-every lets it run less often than the optimizer, and the
// AdamW instantiations stay what they are.
#include "torch_utils.h"
#include "stream_vec.h"

namespace {

template <class P, bool NT>
__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ e,
                                                  const typename P::T* __restrict__ p, long n8,
                                                  float one_minus_decay,
                                                  const float* __restrict__ stats) {
  if (stats[2] != 0.f) return;  // non-finite gradient norm: the parameters did not move either
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    float pf[8], ef[8];
    V8<P, NT>::load(p + i * 8, pf);
    V8<EF32, NT>::load(e + i * 8, ef);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // three roundings: a multiply-add fused from these would differ from the definition
#pragma clang fp contract(off)
      const float diff = pf[j] - ef[j];
      const float prod = diff * one_minus_decay;
      ef[j] = ef[j] + prod;
    }
    V8<EF32, NT>::store(e + i * 8, ef);
  }
}

}  // namespace

void ema_update_(const at::Tensor& ema, const at::Tensor& p, const at::Tensor& stats,
                 double one_minus_decay, int64_t max_blocks) {
  FT_CHECK_CUDA(ema);
  FT_CHECK_CUDA(p);
  FT_CHECK_CUDA(stats);
  FT_CHECK_CONTIG(ema);
  FT_CHECK_CONTIG(p);
  FT_CHECK_CONTIG(stats);
  FT_CHECK_F32(ema);
  FT_CHECK_F32(stats);
  TORCH_CHECK(stats.numel() == 3, "ema_update: stats must be fp32[3] (norm, coef, nonfinite)");
  TORCH_CHECK(ema.numel() == p.numel(), "ema_update: size mismatch");
  TORCH_CHECK(p.numel() % 8 == 0, "ema_update: numel must be a multiple of 8");
  const at::DeviceGuard guard(p.device());
  const long n8 = p.numel() / 8;
  int nb = stream_grid(n8);
  if (max_blocks > 0) nb = (int)std::max(1L, std::min((n8 + 255) / 256, (long)max_blocks));  // as adamw_
  const dim3 grid(nb), block(256);
  const bool nt = stream_nt();
  const float omd = (float)one_minus_decay;
  FT_DISPATCH_E(p.scalar_type(), {
    using PT = typename E::T;
    if (nt)
      hipLaunchKernelGGL((ema_kernel<E, true>), grid, block, 0, ft_stream(), mptr<float>(ema),
                         cptr<PT>(p), n8, omd, cptr<float>(stats));
    else
      hipLaunchKernelGGL((ema_kernel<E, false>), grid, block, 0, ft_stream(), mptr<float>(ema),
                         cptr<PT>(p), n8, omd, cptr<float>(stats));
  });
  FT_LAUNCH_CHECK();
}

TORCH_LIBRARY_FRAGMENT(ftamd, m) {
  m.def("ema_update_(Tensor(a!) ema_f32, Tensor p, Tensor stats, float one_minus_decay, int max_blocks=0) -> ()",
        &ema_update_);
}
