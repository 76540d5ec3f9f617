// Weight-only FP8 decode: the gemv kernels of decode.hip on e4m3 codes with one fp32 scale per
// output row (the format and its definition: utils/fp8.py), and the quantizer that makes them.
// Decoding is bound by the weight bytes (profiles/generate.md); codes are half of them.
//
//   quantize_rows_e4m3   w [N, K] (bf16 / fp16) -> codes uint8 [N, K], scale fp32 [N]
//   gemv_w8              y[N] = scale[n] * (codes[N, K] x[K]) (+ residual[N])
//   gemv_swiglu_w8       a[H] = silu(g) * u from the code rows h and H + h of [w1; w3]
//   gemv_rows_w8, gemv_swiglu_rows_w8: x [R, K]; row r has the bits of the one-row op on x[r]
//
// The gemv: one wave per output row. Lane l takes the 16-byte vectors l, l + 64, ... of the code
// row: 16 weights each, so one wave step covers 1024 elements; four vectors are in flight, each
// with its own fp32 accumulator, and x is read as two 16-byte vectors per weight vector. Codes are
// decoded in registers (fp8.h) and accumulated with fmaf in element order; the lane sums are added
// as (a0 + a1) + (a2 + a3), then the xor butterfly over the wave. Lane 0 then forms
// s * scale[row] (one fp32 multiply), + residual, and rounds once to the model dtype.
//
// One kernel serves the one-row and the multi-row ops (gemv_w8_kernel<E, SWIGLU, RT>): K is walked
// in chunks of one unrolled sweep (4096 elements), and inside a chunk every lane does what the
// plain loop `for (; k + 3 STEP < K; k += 4 STEP) ...; for (; k < K; k += STEP) ...` does at that
// k, for each of the RT activation rows of its tile. RT == 1 reads x from memory (every wave reads
// the same K elements: they come from the cache). RT > 1 stages the chunk of the tile's x rows in
// LDS once per workgroup of 8 waves: with the weights at half the bytes, 8 waves each reading RT
// activation rows from the cache would move more activation than weight bytes through the vector
// memory path (RT x 2 bytes per 1-byte weight). Staging changes where x comes from, not the
// order of the adds.
//
// Plain vector code: no matrix cores, no atomics, and no inline assembly but for the empty register
// barrier (no instruction in it) in scaled() of fp8.h, which says why it is there. Every reduction has a fixed
// order, so each op returns the same bits from run to run.
#include "decode_host.h"  // check_vec, check_residual, the rows tile
#include "fp8.h"

namespace {

constexpr int W8_VEC = 16;             // codes per 16-byte vector
constexpr int W8_STEP = 64 * W8_VEC;   // elements per wave step
constexpr int W8_CHUNK = 4 * W8_STEP;  // elements per unrolled sweep: the staging unit

// acc += <16 decoded weights, 16 activations (two 16-byte vectors of the model dtype)>, in element order
template <class E>
__device__ __forceinline__ float dot16(const float* wf, const uint4& x0, const uint4& x1, float acc) {
  float xf[16];
  unpack8e<E>(x0, xf);
  unpack8e<E>(x1, xf + 8);
#pragma unroll
  for (int j = 0; j < W8_VEC; ++j) acc = fmaf(wf[j], xf[j], acc);
  return acc;
}

template <int RT>
struct W8Tile {
  static constexpr int WAVES = RT == 1 ? 4 : 8;
  static constexpr int THREADS = WAVES * 64;
};

// Grid: ceil(N / WAVES) * ntiles workgroups, the tiles of one block of output rows neighbours (the
// tiles after the first find the codes in a cache). Rows of the tile at and beyond R are computed
// on row R - 1 again and not stored; with RT > 1 a wave whose output row is at or beyond N works on
// row N - 1 and stores nothing, since every wave of the workgroup has to reach the barriers.
template <class E, bool SWIGLU, int RT>
__global__ __launch_bounds__(W8Tile<RT>::THREADS) void gemv_w8_kernel(
    const typename E::T* __restrict__ x, const uint8_t* __restrict__ codes, const float* __restrict__ scale,
    const typename E::T* __restrict__ res, typename E::T* __restrict__ y, int N, int K, int R, int ntiles) {
  typedef typename E::T T;
  constexpr int WAVES = W8Tile<RT>::WAVES, THREADS = W8Tile<RT>::THREADS;
  constexpr bool STAGE = RT > 1;
  __shared__ uint4 xs[STAGE ? RT * W8_CHUNK / 8 : 1];  // [RT][chunk], 8 elements per uint4
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x % ntiles;
  const int out_row = (blockIdx.x / ntiles) * WAVES + (threadIdx.x >> 6);
  if (!STAGE && out_row >= N) return;  // whole waves leave; RT == 1 has no block barrier
  const int row = min(out_row, N - 1);
  const int r0 = tile * RT;
  const uint8_t* c0 = codes + (long)row * K;
  const uint8_t* c1 = codes + ((long)row + N) * K;  // SWIGLU only: the w3 row of feature `row`
  const T* xr[RT];
  float a[RT][4], b[RT][4];
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    xr[r] = x + (long)min(r0 + r, R - 1) * K;
#pragma unroll
    for (int u = 0; u < 4; ++u) a[r][u] = b[r][u] = 0.f;
  }
  // the two 16-byte vectors of activation row r at element k (k - base inside the staged chunk)
  auto xvec = [&](int r, int k, int base, uint4& x0, uint4& x1) {
    if constexpr (STAGE) {
      const uint4* p = xs + r * (W8_CHUNK / 8) + (k - base) / 8;
      x0 = p[0];
      x1 = p[1];
    } else {
      x0 = *reinterpret_cast<const uint4*>(xr[r] + k);
      x1 = *reinterpret_cast<const uint4*>(xr[r] + k + 8);
    }
  };
  for (int base = 0; base < K; base += W8_CHUNK) {
    if constexpr (STAGE) {
      const int nv = min(W8_CHUNK, K - base) / 8;  // K % 16 == 0: whole vectors
      for (int i = threadIdx.x; i < RT * nv; i += THREADS) {
        const int r = i / nv, v = i - r * nv;
        xs[r * (W8_CHUNK / 8) + v] = *reinterpret_cast<const uint4*>(xr[r] + base + v * 8);
      }
      __syncthreads();
    }
    const int k = base + lane * W8_VEC;
    if (k + 3 * W8_STEP < K) {
      // the unrolled sweep: vector u into accumulator u
      uint4 wv[4], uv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        wv[u] = *reinterpret_cast<const uint4*>(c0 + k + u * W8_STEP);
        if constexpr (SWIGLU) uv[u] = *reinterpret_cast<const uint4*>(c1 + k + u * W8_STEP);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float wf[W8_VEC], uf[W8_VEC];
        fp8x16_to_f32(wv[u], wf);
        if constexpr (SWIGLU) fp8x16_to_f32(uv[u], uf);
#pragma unroll
        for (int r = 0; r < RT; ++r) {
          uint4 x0, x1;
          xvec(r, k + u * W8_STEP, base, x0, x1);
          a[r][u] = dot16<E>(wf, x0, x1, a[r][u]);
          if constexpr (SWIGLU) b[r][u] = dot16<E>(uf, x0, x1, b[r][u]);
        }
      }
    } else {
      // the tail: whole steps into accumulator 0, lanes past K idle. It ends inside this chunk:
      // k + 3 STEP >= K here.
      for (int kt = k; kt < K; kt += W8_STEP) {
        float wf[W8_VEC], uf[W8_VEC];
        fp8x16_to_f32(*reinterpret_cast<const uint4*>(c0 + kt), wf);
        if constexpr (SWIGLU) fp8x16_to_f32(*reinterpret_cast<const uint4*>(c1 + kt), uf);
#pragma unroll
        for (int r = 0; r < RT; ++r) {
          uint4 x0, x1;
          xvec(r, kt, base, x0, x1);
          a[r][0] = dot16<E>(wf, x0, x1, a[r][0]);
          if constexpr (SWIGLU) b[r][0] = dot16<E>(uf, x0, x1, b[r][0]);
        }
      }
    }
    if constexpr (STAGE) __syncthreads();  // the next chunk overwrites xs
  }
  const float sc0 = scale[row], sc1 = SWIGLU ? scale[row + N] : 0.f;
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    const float s = wave_sum((a[r][0] + a[r][1]) + (a[r][2] + a[r][3]));
    const bool store = lane == 0 && r0 + r < R && out_row < N;
    const long at = (long)(r0 + r) * N + row;
    if constexpr (SWIGLU) {
      const float t = wave_sum((b[r][0] + b[r][1]) + (b[r][2] + b[r][3]));
      if (store) {
        // g, u and silu(g) each rounded to the model dtype, as in decode.hip's gemv_kernel: the
        // composed gemv_w8 -> silu -> mul
        const float g = rnd<E>(scaled<E>(s, sc0, nullptr)), u = rnd<E>(scaled<E>(t, sc1, nullptr));
        const float sl = rnd<E>(g / (1.f + expf(-g)));
        y[at] = cvt1<E>(sl * u);
      }
    } else if (store) {
      y[at] = cvt1<E>(scaled<E>(s, sc0, res != nullptr ? res + at : nullptr));
    }
  }
}

// --------------------------------------------------------------------------------------------
// quantize_rows_e4m3. Per row: amax = max |w| (sweep 1), inv = 448 / amax and scale = amax / 448
// (IEEE divisions), code = e4m3_rne(fp32(w) * inv) (sweep 2, which finds the row in the cache:
// a row is at most tens of KB). A lane takes 16 elements at a time: two 16-byte loads, one 16-byte
// store of 16 codes.
//
// WG: one workgroup of 256 threads per row; otherwise one wave per row, four rows per workgroup.
// The host takes the wave form for K <= 2048: such a row has at most 128 vectors of 16 elements,
// so a workgroup would leave half or more of its lanes without any and pay a barrier for it. Longer
// rows take the workgroup, which puts four times the loads in flight per row and keeps each lane's
// sweep short (K = 14336: 3.5 vectors per lane instead of 14).
//
// The maximum is taken on the bit patterns of |w| as integers: for non-negative floats the integer
// order is the float order, with infinity and every NaN above all finite values, so one exact,
// order-free reduction gives amax and tells whether the row is finite.
// --------------------------------------------------------------------------------------------
template <class E>
__device__ __forceinline__ void ld16(const typename E::T* p, float* f) {
  unpack8e<E>(*reinterpret_cast<const uint4*>(p), f);
  unpack8e<E>(*reinterpret_cast<const uint4*>(p + 8), f + 8);
}

template <class E, bool WG>
__global__ __launch_bounds__(256) void quantize_rows_kernel(const typename E::T* __restrict__ w,
                                                            uint8_t* __restrict__ codes,
                                                            float* __restrict__ scale, int N, int K) {
  constexpr int LANES = WG ? 256 : 64;
  __shared__ uint32_t red[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int row = WG ? blockIdx.x : blockIdx.x * 4 + wid;
  if (row >= N) return;  // WG: never (the grid is N); else whole waves leave, and there is no barrier
  const int li = WG ? threadIdx.x : lane;
  const typename E::T* wr = w + (long)row * K;
  uint32_t m = 0u;
  for (int k = li * W8_VEC; k < K; k += LANES * W8_VEC) {
    float f[W8_VEC];
    ld16<E>(wr + k, f);
#pragma unroll
    for (int j = 0; j < W8_VEC; ++j) m = max(m, __float_as_uint(f[j]) & 0x7fffffffu);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
  if constexpr (WG) {
    if (lane == 0) red[wid] = m;
    __syncthreads();
    m = max(max(red[0], red[1]), max(red[2], red[3]));
  }
  const E4m3Row q = e4m3_row(m);
  if (li == 0) scale[row] = q.scale;
  uint8_t* cr = codes + (long)row * K;
  for (int k = li * W8_VEC; k < K; k += LANES * W8_VEC) {
    float f[W8_VEC];
    uint4 c = make_uint4(0u, 0u, 0u, 0u);
    if (q.finite) {
      ld16<E>(wr + k, f);
#pragma unroll
      for (int j = 0; j < W8_VEC; ++j) f[j] = __fmul_rn(f[j], q.inv);
      c = make_uint4(f32x4_to_fp8(f), f32x4_to_fp8(f + 4), f32x4_to_fp8(f + 8), f32x4_to_fp8(f + 12));
    }
    *reinterpret_cast<uint4*>(cr + k) = c;
  }
}

constexpr int QUANT_WAVE_MAX_K = 2048;

void quantize_rows_e4m3_out(const at::Tensor& w, at::Tensor codes, at::Tensor scale) {
  const char* op = "quantize_rows_e4m3";
  check_vec(op, w, "w");
  check_vec(op, codes, "codes");
  TORCH_CHECK(w.scalar_type() == at::kBFloat16 || w.scalar_type() == at::kHalf, op, ": w must be bf16 or fp16");
  TORCH_CHECK(w.dim() == 2, op, ": w [N, K]");
  const int64_t N = w.size(0), K = w.size(1);
  TORCH_CHECK(K > 0 && K % W8_VEC == 0, op, ": K must be a positive multiple of 16 (16-byte vectors of codes)");
  TORCH_CHECK(N > 0 && N <= INT_MAX - 4 && K <= INT_MAX - 256 * W8_VEC, op, ": N and K must fit 32 bits");
  TORCH_CHECK(codes.scalar_type() == at::kByte && codes.device() == w.device() && codes.dim() == 2 &&
                  codes.size(0) == N && codes.size(1) == K,
              op, ": codes must be uint8 [N, K] on w's device");
  TORCH_CHECK(scale.is_cuda() && scale.device() == w.device() && scale.scalar_type() == at::kFloat &&
                  scale.is_contiguous() && scale.dim() == 1 && scale.size(0) == N,
              op, ": scale must be a contiguous fp32 [N] tensor on w's device");
  const at::DeviceGuard guard(w.device());
  const bool wg = K > QUANT_WAVE_MAX_K;
  const unsigned blocks = (unsigned)(wg ? N : (N + 3) / 4);
  FT_DISPATCH_E16(w.scalar_type(), {
    if (wg)
      hipLaunchKernelGGL((quantize_rows_kernel<E, true>), dim3(blocks), dim3(256), 0, ft_stream(),
                         cptr<typename E::T>(w), mptr<uint8_t>(codes), mptr<float>(scale), (int)N, (int)K);
    else
      hipLaunchKernelGGL((quantize_rows_kernel<E, false>), dim3(blocks), dim3(256), 0, ft_stream(),
                         cptr<typename E::T>(w), mptr<uint8_t>(codes), mptr<float>(scale), (int)N, (int)K);
  });
  FT_LAUNCH_CHECK();
}

std::tuple<at::Tensor, at::Tensor> quantize_rows_e4m3(const at::Tensor& w) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 2, "quantize_rows_e4m3: w must be a GPU tensor [N, K]");
  const at::DeviceGuard guard(w.device());
  auto codes = at::empty({w.size(0), w.size(1)}, w.options().dtype(at::kByte));
  auto scale = at::empty({w.size(0)}, w.options().dtype(at::kFloat));
  quantize_rows_e4m3_out(w, codes, scale);
  return {codes, scale};
}

// The tile heights of the multi-row ops. R <= 8 takes the smallest tile that holds it; above, tiles
// of W8_ROWS_TILE rows (SWIGLU: W8_SWIGLU_ROWS_TILE, whose two accumulator sets per activation row
// would otherwise take the registers of a 512-thread workgroup past 128 per lane).
constexpr int W8_ROWS_TILE = 8;
constexpr int W8_SWIGLU_ROWS_TILE = 4;

// x [K] (rows == false) or [R, K]; the result is [N] or [R, N].
template <bool SWIGLU>
at::Tensor gemv_w8_impl(const char* op, bool rows, const at::Tensor& x, const at::Tensor& codes,
                        const at::Tensor& scale, const c10::optional<at::Tensor>& residual) {
  check_vec(op, x, "x");
  check_vec(op, codes, "codes");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf, op, ": x must be bf16 or fp16");
  TORCH_CHECK(codes.scalar_type() == at::kByte, op, ": codes must be uint8 (e4m3 bit patterns)");
  TORCH_CHECK(x.device() == codes.device(), op, ": x / codes device mismatch");
  TORCH_CHECK(codes.dim() == 2 && x.dim() == (rows ? 2 : 1) && x.size(-1) == codes.size(1), op,
              rows ? ": x [R, K], codes [N, K]" : ": x [K], codes [N, K]");
  const int64_t R = rows ? x.size(0) : 1, nrows = codes.size(0), K = codes.size(1);
  TORCH_CHECK(K > 0 && K % W8_VEC == 0, op, ": K must be a positive multiple of 16 (16-byte vectors of codes)");
  TORCH_CHECK(R >= 1 && R <= INT_MAX, op, ": x needs at least one row");
  TORCH_CHECK(nrows > 0 && nrows <= INT_MAX - 8 && K <= INT_MAX - 2 * W8_CHUNK, op, ": N and K must fit 32 bits");
  TORCH_CHECK(!SWIGLU || nrows % 2 == 0, op, ": codes13 must be [2H, K]");
  TORCH_CHECK(scale.is_cuda() && scale.device() == codes.device() && scale.scalar_type() == at::kFloat &&
                  scale.is_contiguous() && scale.dim() == 1 && scale.size(0) == nrows,
              op, ": scale must be a contiguous fp32 tensor with one entry per code row, on the codes' device");
  const int64_t N = SWIGLU ? nrows / 2 : nrows;
  const bool has_res = residual.has_value() && residual->defined();
  if (has_res) check_residual(op, *residual, x, N);
  constexpr int TOP = SWIGLU ? W8_SWIGLU_ROWS_TILE : W8_ROWS_TILE;
  const int rt = rows_tile(R, TOP);
  const int waves = rt == 1 ? 4 : 8;
  const int64_t ntiles = (R + rt - 1) / rt;
  const int64_t blocks = (N + waves - 1) / waves * ntiles;
  TORCH_CHECK(blocks <= INT_MAX, op, ": too many workgroups (output rows x row tiles)");
  const at::DeviceGuard guard(x.device());
  auto y = rows ? at::empty({R, N}, x.options()) : at::empty({N}, x.options());
  FT_DISPATCH_E16(x.scalar_type(), FT_ROWS_TILE(rt, TOP, {
    hipLaunchKernelGGL((gemv_w8_kernel<E, SWIGLU, RT>), dim3((unsigned)blocks), dim3(W8Tile<RT>::THREADS), 0,
                       ft_stream(), cptr<typename E::T>(x), cptr<uint8_t>(codes), cptr<float>(scale),
                       has_res ? cptr<typename E::T>(*residual) : nullptr, mptr<typename E::T>(y), (int)N, (int)K,
                       (int)R, (int)ntiles);
  }));
  FT_LAUNCH_CHECK();
  return y;
}

at::Tensor gemv_w8(const at::Tensor& x, const at::Tensor& codes, const at::Tensor& scale,
                   const c10::optional<at::Tensor>& residual) {
  return gemv_w8_impl<false>("gemv_w8", false, x, codes, scale, residual);
}

at::Tensor gemv_swiglu_w8(const at::Tensor& x, const at::Tensor& codes13, const at::Tensor& scale13) {
  return gemv_w8_impl<true>("gemv_swiglu_w8", false, x, codes13, scale13, c10::nullopt);
}

// y[R, N]; row r has the bits of gemv_w8(x[r], codes, scale, residual[r]).
at::Tensor gemv_rows_w8(const at::Tensor& x, const at::Tensor& codes, const at::Tensor& scale,
                        const c10::optional<at::Tensor>& residual) {
  return gemv_w8_impl<false>("gemv_rows_w8", true, x, codes, scale, residual);
}

// a[R, H]; row r has the bits of gemv_swiglu_w8(x[r], codes13, scale13).
at::Tensor gemv_swiglu_rows_w8(const at::Tensor& x, const at::Tensor& codes13, const at::Tensor& scale13) {
  return gemv_w8_impl<true>("gemv_swiglu_rows_w8", true, x, codes13, scale13, c10::nullopt);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(ftamd, m) {
  m.def("quantize_rows_e4m3(Tensor w) -> (Tensor, Tensor)", &quantize_rows_e4m3);
  m.def("quantize_rows_e4m3_out(Tensor w, Tensor(a!) codes, Tensor(b!) scale) -> ()", &quantize_rows_e4m3_out);
  m.def("gemv_w8(Tensor x, Tensor codes, Tensor scale, Tensor? residual) -> Tensor", &gemv_w8);
  m.def("gemv_swiglu_w8(Tensor x, Tensor codes13, Tensor scale13) -> Tensor", &gemv_swiglu_w8);
  m.def("gemv_rows_w8(Tensor x, Tensor codes, Tensor scale, Tensor? residual) -> Tensor", &gemv_rows_w8);
  m.def("gemv_swiglu_rows_w8(Tensor x, Tensor codes13, Tensor scale13) -> Tensor", &gemv_swiglu_rows_w8);
}
