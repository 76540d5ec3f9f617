// Batched decode on the matrix cores: skinny GEMMs for 1 <= R <= 64 activation rows against a
// streamed [N, K] weight. The gemv kernels of decode.hip / decode_w8.hip repeat a whole dot product on
// the vector ALU for every activation row, so their time grows with R; here the R rows are the columns
// of an MFMA and a weight-bound product costs about one pass over the weight whatever R is.
//
//   gemm_rows_mma            y[R, N] = x[R, K] w[N, K]^T (+ residual[R, N])
//   gemm_swiglu_rows_mma     a[R, H] = silu(g) * u, g and u from rows h and H + h of w13 [2H, K]
//   gemm_rows_mma_w8         y = scale[n] * (decode(codes[N, K]) x^T) (+ residual)
//   gemm_swiglu_rows_mma_w8  the SwiGLU form on e4m3 codes with one fp32 scale per code row
//
// Instruction: v_mfma_f32_16x16x32_bf16 / _f16. The weight is the A operand (16 output features x 32 K),
// the activations are B (32 K x 16 batch rows). Lane l holds of A eight K-contiguous elements of weight
// row l % 16 (k-group l / 16): a plain 16-byte global load, no LDS on the weight path. The accumulator
// of lane l is then four consecutive output features 4 (l / 16) .. + 3 of batch row l % 16: one 8-byte
// store into y[r, n ...].
//
// Weight stream: K is walked in chunks of 128. A dot product does not care about the order of K as long
// as A and B agree, so inside a chunk lane (row, kg) owns the 32 contiguous elements kg * 32 .. + 31 of
// its row (64 bytes: four 16-byte loads; FP8: 32 codes, two 16-byte loads), and MFMA step j of the chunk
// takes its j-th group of 8. The four lanes of a row use every byte of the lines they fetch. The B
// fragment of step j is read with the same permutation: elements kg * 32 + 8 j .. + 7 of the chunk of
// batch row l % 16. Two chunks of weights are in flight per wave in two register sets: the loads of
// chunk c + 2 are issued as soon as the MFMAs of chunk c have consumed their set.
//
// Activations go through LDS: the 4 waves of a workgroup share a K range and differ in output features
// (16 each: a workgroup tile of 64 features), and share one double-buffered [16 NT, 128] chunk of x,
// NT = ceil(R / 16) a template parameter. Were every wave to read its B fragments from the cache, the
// activation traffic through the vector memory path would be R / 16 times the weight traffic. A staged
// row is 16 vectors of 16 bytes plus one of padding: the 16 lanes of a k-group then read 16-byte
// fragments 17 vectors apart, which covers the 64 banks once. The chunk c + 1 is loaded to registers
// before the MFMAs of chunk c and written to the other buffer after them: one barrier per chunk.
//
// Split along K: wqkv, wo and w2 of an 8B model have 64 .. 96 workgroup tiles for 256 CUs, so the grid
// is (tiles, S) and slice s takes the chunks [s nch / S, (s + 1) nch / S). S is a function of the
// weight's shape alone (mma_split), never of R. With S > 1 every workgroup stores its fp32 partial tile
// and a second small launch adds the S partials of an element in slice order and runs the epilogue: no
// workgroup waits for another, there is no flag, counter or atomic, and the pair of launches captures
// into a graph like any other (the workspace comes from the caching allocator).
//
// Edges: no load goes beyond an operand's end. In a chunk that K ends in, the vectors at and beyond K
// are zero in both operands (zeroing one alone would give 0 x Inf = NaN from whatever lies there); batch
// rows at and beyond R are staged as zeros, features at and beyond N read row N - 1, and neither is stored.
//
// Epilogue: plain: fp32 sum (+ residual in fp32), one rounding. FP8: one fp32 multiply by scale[n], then
// the residual, then one rounding, through scaled() of fp8.h. SwiGLU: g, u and silu(g) each rounded to
// the dtype as in decode.hip's gemv_kernel, so the fused op has the bits of swiglu_reference(gemm_rows_mma).
// FP8 weights are a loader variant: the codes are decoded in registers to the activation dtype (every
// e4m3 value is exact in bf16 and in fp16) and feed the same MFMA loop.
//
// The contract is batch invariance, not the bits of gemv_rows (the order of the sum differs): y[r] depends
// on x[r] and the weight alone -- not on R, on the other rows, or on the row's place in the batch; R = 1
// runs the same kernel with 15 idle columns. Every op returns the same bits from run to run.
#include "decode_host.h"  // check_vec, check_residual
#include "fp8.h"

namespace {

constexpr int MM_KC = 128;                 // K elements per chunk
constexpr int MM_LANE_K = MM_KC / 4;       // K elements of a chunk one lane owns
constexpr int MM_WAVES = 4;
constexpr int MM_THREADS = MM_WAVES * 64;
constexpr int MM_TILE = MM_WAVES * 16;     // output features per workgroup
constexpr int MM_LDS_ROW = MM_KC / 8 + 1;  // 16-byte vectors per staged activation row, one of them padding
constexpr int MM_MAX_R = 64;
constexpr int MM_MAX_SPLIT = 32;
constexpr int MM_TARGET_WGS = 512;         // two workgroups for each of the 256 CUs
constexpr int MM_MIN_SLICE_CHUNKS = 4;     // a slice is at least 512 elements of K

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

template <class E>
__device__ __forceinline__ f32x4_t mfma16(const uint4& a, const uint4& b, f32x4_t c) {
  if constexpr (std::is_same<E, EBF16>::value)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b),
                                                   c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b),
                                                  c, 0, 0, 0);
}

// The 16-byte vectors of a lane's 32 elements of one chunk: four of 8 elements, or two of 16 codes.
template <bool W8>
struct MmaRaw {
  static constexpr int N = W8 ? 2 : 4;
  uint4 v[N];
};

// p: the lane's row at the chunk's first element the lane owns, k: that element's index in the row.
template <bool W8, bool GUARD, class WT>
__device__ __forceinline__ void load_w(const WT* __restrict__ p, int k, int K, MmaRaw<W8>& r) {
  constexpr int PER = MM_LANE_K / MmaRaw<W8>::N;  // elements per vector
#pragma unroll
  for (int j = 0; j < MmaRaw<W8>::N; ++j) {
    if (!GUARD || k + j * PER < K) r.v[j] = *reinterpret_cast<const uint4*>(p + j * PER);
    else r.v[j] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// Two words of codes (8, byte 0 first) as 8 elements of the activation dtype. Exact.
template <class E>
__device__ __forceinline__ uint4 fp8x8_to_e(uint32_t w0, uint32_t w1) {
  float f[8];
  fp8x4_to_f32(w0, f);
  fp8x4_to_f32(w1, f + 4);
  return make_uint4(pk2<E>(f[0], f[1]), pk2<E>(f[2], f[3]), pk2<E>(f[4], f[5]), pk2<E>(f[6], f[7]));
}

// The A fragment of MFMA step j (0 .. 3): the lane's elements 8 j .. 8 j + 7.
template <class E, bool W8>
__device__ __forceinline__ uint4 frag_a(const MmaRaw<W8>& r, int j) {
  if constexpr (W8) {
    const uint4& c = r.v[j >> 1];
    return (j & 1) ? fp8x8_to_e<E>(c.z, c.w) : fp8x8_to_e<E>(c.x, c.y);
  } else {
    return r.v[j];
  }
}

// One output element from its fp32 sum(s): s (and t, the u sum of the SwiGLU forms) of feature n.
template <class E, bool SWIGLU, bool W8>
__device__ __forceinline__ typename E::T finish(float s, float t, const float* __restrict__ scale, int n, int N,
                                                const typename E::T* res_at) {
  if constexpr (SWIGLU) {
    float g = s, u = t;
    if constexpr (W8) {
      g = scaled<E>(s, scale[n], nullptr);
      u = scaled<E>(t, scale[n + N], nullptr);
    }
    // g, u and silu(g) each rounded to the model dtype, as in decode.hip's gemv_kernel
    g = rnd<E>(g);
    u = rnd<E>(u);
    const float sl = rnd<E>(g / (1.f + expf(-g)));
    return cvt1<E>(sl * u);
  } else if constexpr (W8) {
    return cvt1<E>(scaled<E>(s, scale[n], res_at));
  } else {
    if (res_at != nullptr) s += ld1<E>(res_at);
    return cvt1<E>(s);
  }
}

// Grid (tiles, S). part: fp32 [S][P][R][Np] (P = 2 planes g, u for SWIGLU; Np = tiles * 64), used with
// S > 1 only; with S == 1 the kernel runs the epilogue itself.
template <class E, bool SWIGLU, bool W8, int NT>
__global__ __launch_bounds__(MM_THREADS) void gemm_mma_kernel(
    const typename E::T* __restrict__ x, const void* __restrict__ wv, const float* __restrict__ scale,
    const typename E::T* __restrict__ res, typename E::T* __restrict__ y, float* __restrict__ part, int N, int K,
    int R, int S, int Np) {
  typedef typename E::T T;
  typedef typename std::conditional<W8, uint8_t, T>::type WT;
  constexpr int ROWS = 16 * NT, P = SWIGLU ? 2 : 1;
  __shared__ uint4 xs[2][ROWS * MM_LDS_ROW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, kg = lane >> 4;
  const int slice = blockIdx.y;
  const int n0 = blockIdx.x * MM_TILE + wave * 16;
  const int nch = (K + MM_KC - 1) / MM_KC, nfull = K / MM_KC;
  const int c0 = (int)((long)slice * nch / S), c1 = (int)((long)(slice + 1) * nch / S);
  const WT* w0 = reinterpret_cast<const WT*>(wv) + (long)min(n0 + fr, N - 1) * K + kg * MM_LANE_K;
  const WT* w1 = w0 + (long)N * K;  // SWIGLU only: the w3 row of the feature
  // staging: thread i moves the vector i % 16 of the rows i / 16 + 16 q
  const int srow = threadIdx.x >> 4, scol = threadIdx.x & 15;

  f32x4_t acc[NT], accu[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = accu[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  MmaRaw<W8> a0, a1, b0, b1;  // two register sets (chunks c, c + 1); b: the w3 rows
  uint4 xr[NT];

  auto loadw = [&](int c, MmaRaw<W8>& a, MmaRaw<W8>& b) {
    const int k = c * MM_KC + kg * MM_LANE_K;
    if (c < nfull) {
      load_w<W8, false>(w0 + (long)c * MM_KC, k, K, a);
      if constexpr (SWIGLU) load_w<W8, false>(w1 + (long)c * MM_KC, k, K, b);
    } else {
      load_w<W8, true>(w0 + (long)c * MM_KC, k, K, a);
      if constexpr (SWIGLU) load_w<W8, true>(w1 + (long)c * MM_KC, k, K, b);
    }
  };
  auto loadx = [&](int c) {
    const int k = c * MM_KC + scol * 8;
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int r = srow + 16 * q;
      xr[q] = (r < R && k < K) ? *reinterpret_cast<const uint4*>(x + (long)r * K + k) : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto storex = [&](int buf) {
#pragma unroll
    for (int q = 0; q < NT; ++q) xs[buf][(srow + 16 * q) * MM_LDS_ROW + scol] = xr[q];
  };
  // chunk c: its weights are in (a, b), its activations in xs[buf]
  auto step = [&](int c, int buf, MmaRaw<W8>& a, MmaRaw<W8>& b) {
    const bool more = c + 1 < c1;
    if (more) loadx(c + 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint4 fa = frag_a<E, W8>(a, j);
      uint4 fb;
      if constexpr (SWIGLU) fb = frag_a<E, W8>(b, j);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const uint4 xb = xs[buf][(16 * t + fr) * MM_LDS_ROW + kg * 4 + j];
        acc[t] = mfma16<E>(fa, xb, acc[t]);
        if constexpr (SWIGLU) accu[t] = mfma16<E>(fb, xb, accu[t]);
      }
    }
    if (c + 2 < c1) loadw(c + 2, a, b);
    if (more) storex(buf ^ 1);
    __syncthreads();  // xs[buf ^ 1] is written; xs[buf] is free for the chunk after it
  };

  if (c0 < c1) {
    loadx(c0);
    loadw(c0, a0, b0);
    if (c0 + 1 < c1) loadw(c0 + 1, a1, b1);
    storex(0);
  }
  __syncthreads();
  for (int c = c0; c < c1; c += 2) {  // c, c1: the same in every thread of the workgroup
    step(c, 0, a0, b0);
    if (c + 1 < c1) step(c + 1, 1, a1, b1);
  }

  const int n = n0 + 4 * kg;  // the lane's features n .. n + 3
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int r = 16 * t + fr;
    if (r >= R) continue;
    if (S > 1) {
      float* p = part + (((long)slice * P) * R + r) * Np + n;  // n + 3 < Np: whole tiles
      *reinterpret_cast<float4*>(p) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
      if constexpr (SWIGLU)
        *reinterpret_cast<float4*>(p + (long)R * Np) = make_float4(accu[t][0], accu[t][1], accu[t][2], accu[t][3]);
    } else {
      const long at = (long)r * N + n;
      T o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (n + i < N)
          o[i] = finish<E, SWIGLU, W8>(acc[t][i], accu[t][i], scale, n + i, N, res != nullptr ? res + at + i : nullptr);
      if ((N & 3) == 0 && n + 3 < N) {  // 8-byte aligned: y is 16-byte aligned, N and n multiples of 4
        *reinterpret_cast<uint2*>(y + at) =
            make_uint2((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16));
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (n + i < N) y[at + i] = o[i];
      }
    }
  }
}

// S > 1: one thread per output element adds its S partials in slice order and runs the epilogue.
template <class E, bool SWIGLU, bool W8>
__global__ __launch_bounds__(256) void gemm_mma_reduce_kernel(const float* __restrict__ part,
                                                              const float* __restrict__ scale,
                                                              const typename E::T* __restrict__ res,
                                                              typename E::T* __restrict__ y, int N, int R, int S,
                                                              int Np) {
  constexpr int P = SWIGLU ? 2 : 1;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)R * N) return;
  const int r = (int)(idx / N), n = (int)(idx - (long)r * N);
  const long plane = (long)R * Np;
  const float* p = part + (long)r * Np + n;
  float s = p[0], t = SWIGLU ? p[plane] : 0.f;
  for (int sl = 1; sl < S; ++sl) {
    s += p[(long)sl * P * plane];
    if constexpr (SWIGLU) t += p[((long)sl * P + 1) * plane];
  }
  y[idx] = finish<E, SWIGLU, W8>(s, t, scale, n, N, res != nullptr ? res + idx : nullptr);
}

// The split factor: a function of the weight's shape ([rows, K], rows = 2H for the SwiGLU forms, so the
// fused op and the plain op on the same weight add in the same order) and of nothing else. Enough
// slices for MM_TARGET_WGS workgroups of 64 rows, each slice at least MM_MIN_SLICE_CHUNKS chunks.
int mma_split(int64_t rows, int64_t K) {
  const int64_t tiles = (rows + MM_TILE - 1) / MM_TILE, nch = (K + MM_KC - 1) / MM_KC;
  const int64_t want = (MM_TARGET_WGS + tiles - 1) / tiles;
  const int64_t cap = std::min<int64_t>(MM_MAX_SPLIT, nch / MM_MIN_SLICE_CHUNKS);
  return (int)std::max<int64_t>(1, std::min(want, cap));
}

// x [R, K], w [rows, K] (weights in x's dtype, or uint8 codes with scale [rows]); the result is [R, N].
template <bool SWIGLU, bool W8>
at::Tensor gemm_mma_impl(const char* op, const at::Tensor& x, const at::Tensor& w,
                         const c10::optional<at::Tensor>& scale, const c10::optional<at::Tensor>& residual,
                         int64_t split) {
  check_vec(op, x, "x");
  check_vec(op, w, W8 ? "codes" : "w");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf, op, ": x must be bf16 or fp16");
  TORCH_CHECK(w.scalar_type() == (W8 ? at::kByte : x.scalar_type()), op,
              W8 ? ": codes must be uint8 (e4m3 bit patterns)" : ": w must have x's dtype");
  TORCH_CHECK(x.device() == w.device(), op, ": operands on different devices");
  TORCH_CHECK(w.dim() == 2 && x.dim() == 2 && x.size(1) == w.size(1), op, ": x [R, K], weight [N, K]");
  const int64_t R = x.size(0), rows = w.size(0), K = w.size(1);
  constexpr int VEC = W8 ? 16 : 8;
  TORCH_CHECK(K > 0 && K % VEC == 0, op, ": K must be a positive multiple of ", VEC, " (16-byte vectors)");
  TORCH_CHECK(R >= 1 && R <= MM_MAX_R, op, ": 1 <= R <= ", MM_MAX_R, " activation rows, got ", R);
  TORCH_CHECK(rows > 0 && rows <= INT_MAX - MM_TILE && K <= INT_MAX - 2 * MM_KC, op, ": N and K must fit 32 bits");
  TORCH_CHECK(!SWIGLU || rows % 2 == 0, op, ": the fused weight must be [2H, K]");
  if (W8) {
    TORCH_CHECK(scale.has_value() && scale->is_cuda() && scale->device() == w.device() &&
                    scale->scalar_type() == at::kFloat && scale->is_contiguous() && scale->dim() == 1 &&
                    scale->size(0) == rows,
                op, ": scale must be a contiguous fp32 tensor with one entry per code row, on the codes' device");
  }
  const int64_t N = SWIGLU ? rows / 2 : rows;
  const bool has_res = residual.has_value() && residual->defined();
  if (has_res) {
    check_vec(op, *residual, "residual");
    check_residual(op, *residual, x, N);
  }
  const int64_t nch = (K + MM_KC - 1) / MM_KC;
  TORCH_CHECK(split >= 0 && split <= std::min<int64_t>(nch, MM_MAX_SPLIT), op, ": split must be 0 (chosen from the "
              "weight's shape) or 1 .. min(", MM_MAX_SPLIT, ", chunks of ", MM_KC, " in K), got ", split);
  const int S = split > 0 ? (int)split : mma_split(rows, K);
  const int64_t tiles = (N + MM_TILE - 1) / MM_TILE, Np = tiles * MM_TILE;
  const int nt = (int)((R + 15) / 16);
  const at::DeviceGuard guard(x.device());
  auto y = at::empty({R, N}, x.options());
  at::Tensor part;
  if (S > 1) part = at::empty({S, SWIGLU ? 2 : 1, R, Np}, x.options().dtype(at::kFloat));
  const float* sc = W8 ? cptr<float>(*scale) : nullptr;
  float* pp = S > 1 ? mptr<float>(part) : nullptr;
#define FT_GEMM_MMA(NT)                                                                                          \
  hipLaunchKernelGGL((gemm_mma_kernel<E, SWIGLU, W8, NT>), dim3((unsigned)tiles, (unsigned)S), dim3(MM_THREADS), \
                     0, ft_stream(), cptr<typename E::T>(x), w.data_ptr(), sc,                                   \
                     has_res ? cptr<typename E::T>(*residual) : nullptr, mptr<typename E::T>(y), pp, (int)N,     \
                     (int)K, (int)R, S, (int)Np)
  FT_DISPATCH_E16(x.scalar_type(), {
    if (nt == 1) FT_GEMM_MMA(1);
    else if (nt == 2) FT_GEMM_MMA(2);
    else if (nt == 3) FT_GEMM_MMA(3);
    else FT_GEMM_MMA(4);
    FT_LAUNCH_CHECK();
    if (S > 1)
      hipLaunchKernelGGL((gemm_mma_reduce_kernel<E, SWIGLU, W8>), dim3((unsigned)((R * N + 255) / 256)), dim3(256),
                         0, ft_stream(), pp, sc, has_res ? cptr<typename E::T>(*residual) : nullptr,
                         mptr<typename E::T>(y), (int)N, (int)R, S, (int)Np);
  });
#undef FT_GEMM_MMA
  FT_LAUNCH_CHECK();
  return y;
}

at::Tensor gemm_rows_mma(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& residual,
                         int64_t split) {
  return gemm_mma_impl<false, false>("gemm_rows_mma", x, w, c10::nullopt, residual, split);
}

at::Tensor gemm_swiglu_rows_mma(const at::Tensor& x, const at::Tensor& w13, int64_t split) {
  return gemm_mma_impl<true, false>("gemm_swiglu_rows_mma", x, w13, c10::nullopt, c10::nullopt, split);
}

at::Tensor gemm_rows_mma_w8(const at::Tensor& x, const at::Tensor& codes, const at::Tensor& scale,
                            const c10::optional<at::Tensor>& residual, int64_t split) {
  return gemm_mma_impl<false, true>("gemm_rows_mma_w8", x, codes, scale, residual, split);
}

at::Tensor gemm_swiglu_rows_mma_w8(const at::Tensor& x, const at::Tensor& codes13, const at::Tensor& scale13,
                                   int64_t split) {
  return gemm_mma_impl<true, true>("gemm_swiglu_rows_mma_w8", x, codes13, scale13, c10::nullopt, split);
}

// The split factor the ops choose for a weight [rows, K] (rows = 2H for the SwiGLU forms).
int64_t gemm_mma_split(int64_t rows, int64_t K) {
  TORCH_CHECK(rows > 0 && K > 0, "gemm_mma_split: rows and K must be positive");
  return mma_split(rows, K);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(ftamd, m) {
  m.def("gemm_rows_mma(Tensor x, Tensor w, Tensor? residual, int split=0) -> Tensor", &gemm_rows_mma);
  m.def("gemm_swiglu_rows_mma(Tensor x, Tensor w13, int split=0) -> Tensor", &gemm_swiglu_rows_mma);
  m.def("gemm_rows_mma_w8(Tensor x, Tensor codes, Tensor scale, Tensor? residual, int split=0) -> Tensor",
        &gemm_rows_mma_w8);
  m.def("gemm_swiglu_rows_mma_w8(Tensor x, Tensor codes13, Tensor scale13, int split=0) -> Tensor",
        &gemm_swiglu_rows_mma_w8);
  m.def("gemm_mma_split(int rows, int K) -> int", &gemm_mma_split);
}
