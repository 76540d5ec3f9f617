// Document boundaries of packed sequences, for the document-masked attention kernels
// (flash_doc_* in flash_attn.hip, flash_f32_doc_* in flash_f32.hip).
//
// tokens [B, S] int64; a document starts at every token equal to `bos`:
//   doc_start[b, i] = position of the most recent bos at or before i (0 if none)
//   doc_end[b, i]   = position of the next bos after i               (S if none)
// so query i sees exactly the keys doc_start[i] <= j <= i, and key j is seen by the queries
// j <= i < doc_end[j]. Both arrays are non-decreasing in i.
//
// One block per sequence. Each thread owns a contiguous chunk: it reduces its chunk (max bos
// position / min bos position), the block scans the 1024 per-thread values in LDS (inclusive
// max scan forwards, inclusive min scan backwards), and each thread then replays its chunk from
// its neighbours' carries. No host synchronisation, no allocation besides the outputs: the op can
// be captured in a HIP graph.
#include "torch_utils.h"

namespace {

constexpr int DB_NT = 1024;

__global__ __launch_bounds__(DB_NT) void doc_bounds_kernel(const long* __restrict__ tokens,
                                                           int* __restrict__ doc_start,
                                                           int* __restrict__ doc_end, int S, long bos) {
  __shared__ int smax[DB_NT];
  __shared__ int smin[DB_NT];
  const int t = threadIdx.x;
  const long* tok = tokens + (long)blockIdx.x * S;
  int* ds = doc_start + (long)blockIdx.x * S;
  int* de = doc_end + (long)blockIdx.x * S;
  const int chunk = (S + DB_NT - 1) / DB_NT;
  const int i0 = min(t * chunk, S), i1 = min(i0 + chunk, S);

  int lmax = 0, lmin = S;  // last / first bos of this chunk
  for (int i = i1 - 1; i >= i0; --i)
    if (tok[i] == bos) {
      lmax = max(lmax, i);
      lmin = i;
    }
  smax[t] = lmax;
  smin[t] = lmin;
  __syncthreads();
  // Hillis-Steele: smax[t] <- max over threads <= t, smin[t] <- min over threads >= t
  for (int off = 1; off < DB_NT; off <<= 1) {
    const int a = t >= off ? smax[t - off] : 0;
    const int b = t + off < DB_NT ? smin[t + off] : S;
    __syncthreads();
    smax[t] = max(smax[t], a);
    smin[t] = min(smin[t], b);
    __syncthreads();
  }
  int run = t > 0 ? smax[t - 1] : 0;
  for (int i = i0; i < i1; ++i) {
    if (tok[i] == bos) run = i;
    ds[i] = run;
  }
  run = t + 1 < DB_NT ? smin[t + 1] : S;
  for (int i = i1 - 1; i >= i0; --i) {
    de[i] = run;
    if (tok[i] == bos) run = i;
  }
}

}  // namespace

// Returns (doc_start, doc_end), both int32 [B, S].
std::tuple<at::Tensor, at::Tensor> doc_bounds(const at::Tensor& tokens, int64_t bos) {
  FT_CHECK_CUDA(tokens);
  FT_CHECK_CONTIG(tokens);
  TORCH_CHECK(tokens.scalar_type() == at::kLong, "doc_bounds: tokens must be int64");
  TORCH_CHECK(tokens.dim() == 2, "doc_bounds: tokens must be [B, S]");
  const long B = tokens.size(0), S = tokens.size(1);
  TORCH_CHECK(S < (1L << 31), "doc_bounds: sequence too long");
  const at::DeviceGuard guard(tokens.device());
  auto opts = tokens.options().dtype(at::kInt);
  auto ds = at::empty({B, S}, opts);
  auto de = at::empty({B, S}, opts);
  if (B > 0 && S > 0) {
    hipLaunchKernelGGL(doc_bounds_kernel, dim3((unsigned)B), dim3(DB_NT), 0, ft_stream(),
                       reinterpret_cast<const long*>(tokens.data_ptr<int64_t>()), mptr<int>(ds), mptr<int>(de),
                       (int)S, (long)bos);
    FT_LAUNCH_CHECK();
  }
  return {ds, de};
}

TORCH_LIBRARY_FRAGMENT(ftamd, m) {
  m.def("doc_bounds(Tensor tokens, int bos) -> (Tensor, Tensor)", &doc_bounds);
}
