// Weight-only MXFP4 decode: the gemv kernels of decode.hip on OCP MXFP4 weights -- e2m1 codes, two
// per byte, with one e8m0 scale byte per block of 32 elements along K (the format and its definition:
// utils/mxfp4.py) -- and the quantizer that makes them. Decoding is bound by the weight bytes
// (profiles/generate.md); these are 0.53 bytes per weight.
//
//   quantize_rows_mxfp4  w [N, K] (bf16 / fp16) -> codes uint8 [N, K / 2], scales uint8 [N, K / 32]
//   gemv_mx4             y[N] = dequant(codes, scales)[N, K] x[K] (+ residual[N])
//   gemv_swiglu_mx4      a[H] = silu(g) * u from the code rows h and H + h of [w1; w3]
//   gemv_rows_mx4, gemv_swiglu_rows_mx4: x [R, K]; row r has the bits of the one-row op on x[r]
//
// How the work is split. A 16-byte vector of codes is one block: 32 weights, one scale byte. A lane
// takes a *unit* of four consecutive blocks -- 64 contiguous bytes of codes, 128 weights, and their
// four scale bytes as one dword -- and half a wave (32 lanes) takes one output row, so one sweep
// covers a *chunk* of 4096 elements and a wave works on two output rows. (A whole wave per row would
// leave half its lanes without a unit at K = 4096, the K of four of Llama-3-8B's five products, and
// the vector ALU is the budget here, see below.) A workgroup is 8 waves: 16 output rows.
//
// The activations go through LDS in every form, the one-row ops included: a unit needs 256 bytes of
// x for its 64 bytes of codes, so sixteen half waves each reading x through the vector memory path
// would move four times the weight bytes there. Per chunk the workgroup stages the chunk of its RT
// activation rows once, 16-byte vectors swizzled inside each unit (vector j of unit u at j ^ (u & 15))
// so that the 32 lanes of a half wave, which read at a 256-byte stride, hit distinct banks. Each
// lane issues its code and scale loads before the staging barrier, so they are in flight while x is
// staged.
//
// Arithmetic. The codes are converted with scale 1.0 to packed pairs of the activation dtype
// (v_cvt_scalef32_pk_{bf16,f16}_fp4: one instruction per byte, exact, e2m1 values are 0 .. 6) and
// multiplied into fp32 with the two-element dot instruction (v_dot2c_f32_{bf16,f16}) against the
// activation pair as it lies in memory: no unpacking of x. Keeping the block scale out of the
// convert makes every scale byte valid for both dtypes (2^p * 6 need not fit fp16) and never hands
// the convert an all-ones exponent. The order of the sums, the same in every instantiation:
//
//   block sum  s_b = (chain of dot2 over byte pairs 0 .. 7) + (chain over pairs 8 .. 15), from 0
//   lane sum   acc = fmaf(s_b, 2^(e_b - 127), acc) over the blocks of the lane's units, in K order
//              (the factor is formed as e_b << 23: a power of two, the product is exact)
//   row sum    xor butterfly over the 32 lanes of the half wave (offsets 16, 8, 4, 2, 1)
//
// then + residual and one rounding to the model dtype. A scale byte 0xFF (a block that held a
// non-finite weight) is tested for on the dword and poisons the lane's sum with NaN.
//
// Vector instructions per weight byte, read off the assembly (-save-temps of this file). The
// arithmetic of a unit in gemv_mx4_kernel<EBF16, false, 1>: 64 v_cvt_scalef32_pk_bf16_fp4 + 64
// v_dot2c_f32_bf16 + 4 v_fma + 4 v_add + the scale shifts for 64 bytes, 2.2 per byte; the converts
// are shared by the rows of a tile (RT = 8: 64 converts, 512 dot2). The whole one-row kernel is 314
// vector instructions per lane, so with one chunk (K = 4096) everything around the arithmetic --
// addresses, staging, the in-K predicates, the reduction -- brings it to 4.9 per byte; the 8-row
// kernel is 998 for 8 rows. The decode_w8 recipe (convert to fp32, unpack x, fmaf) would be 5 per
// byte in the arithmetic alone. Registers (profiles/mxfp4_decode.md): 75 .. 102 VGPRs for the plain
// forms, 113 .. 148 for SwiGLU, no scratch, packed fp32 left on.
//
// Plain vector code: no matrix cores, no atomics, no inline assembly. Every reduction has a fixed
// order, so each op returns the same bits from run to run.
#include "decode_host.h"  // check_vec, check_residual, the rows tile

namespace {

constexpr int MX_BLOCK = 32;                   // elements per scale byte: one 16-byte vector of codes
constexpr int MX_UNIT = 4 * MX_BLOCK;          // elements per lane and sweep: 64 bytes of codes, one scale dword
constexpr int MX_GROUP = 32;                   // lanes per output row
constexpr int MX_CHUNK = MX_GROUP * MX_UNIT;   // elements per sweep: the staging unit (4096)
constexpr int MX_WAVES = 8;
constexpr int MX_THREADS = MX_WAVES * 64;
constexpr int MX_WG_ROWS = MX_WAVES * (64 / MX_GROUP);  // output rows per workgroup
constexpr int MX_CHUNK_VECS = MX_CHUNK / 8;    // 16-byte vectors of x per staged row and chunk

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));

// 4 code bytes (8 weights) of one dword to 4 packed pairs of E's type, unscaled; byte 0 first, the
// low nibble of a byte in the low half of its pair.
template <class E>
__device__ __forceinline__ void fp4x8_to_pairs(uint32_t w, uint32_t* p) {
  if constexpr (std::is_same<E, EBF16>::value) {
    p[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 0));
    p[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 1));
    p[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 2));
    p[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 3));
  } else {
    p[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 0));
    p[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 1));
    p[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 2));
    p[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 3));
  }
}

// One 16-byte vector of codes (a block) to its 16 pairs.
template <class E>
__device__ __forceinline__ void block_to_pairs(const uint4& v, uint32_t* p) {
  fp4x8_to_pairs<E>(v.x, p);
  fp4x8_to_pairs<E>(v.y, p + 4);
  fp4x8_to_pairs<E>(v.z, p + 8);
  fp4x8_to_pairs<E>(v.w, p + 12);
}

// acc + w.lo * x.lo + w.hi * x.hi on packed pairs of E's type, in fp32
template <class E>
__device__ __forceinline__ float dot2(uint32_t w, uint32_t x, float acc) {
  if constexpr (std::is_same<E, EBF16>::value)
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, w), __builtin_bit_cast(bf16x2_t, x), acc,
                                           false);
  else
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2_t, w), __builtin_bit_cast(f16x2_t, x), acc, false);
}

// The block sum: 16 weight pairs against the block's 32 activations (four 16-byte vectors).
template <class E>
__device__ __forceinline__ float block_dot(const uint32_t* wp, const uint4* xv) {
  float lo = 0.f, hi = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    lo = dot2<E>(wp[4 * j + 0], xv[j].x, lo);
    lo = dot2<E>(wp[4 * j + 1], xv[j].y, lo);
    lo = dot2<E>(wp[4 * j + 2], xv[j].z, lo);
    lo = dot2<E>(wp[4 * j + 3], xv[j].w, lo);
    hi = dot2<E>(wp[4 * j + 8], xv[j + 2].x, hi);
    hi = dot2<E>(wp[4 * j + 9], xv[j + 2].y, hi);
    hi = dot2<E>(wp[4 * j + 10], xv[j + 2].z, hi);
    hi = dot2<E>(wp[4 * j + 11], xv[j + 2].w, hi);
  }
  return lo + hi;
}

// The sum over the 32 lanes of a half wave (both halves at once), in every lane of it.
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = MX_GROUP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Whether a dword of scale bytes holds 0xFF: a zero byte of its complement.
__device__ __forceinline__ bool has_ff(uint32_t s) {
  const uint32_t v = ~s;
  return ((v - 0x01010101u) & ~v & 0x80808080u) != 0u;
}

// Where vector j (0 .. 15) of unit u of a staged row lies.
__device__ __forceinline__ int xs_at(int u, int j) { return u * 16 + (j ^ (u & 15)); }

// Grid: ceil(N / 16) * ntiles workgroups, the tiles of one block of output rows neighbours (the
// tiles after the first find the codes in a cache). Rows of the tile at and beyond R are computed on
// row R - 1 again and not stored; a half wave whose output row is at or beyond N works on row N - 1
// and stores nothing, since every wave of the workgroup has to reach the barriers.
template <class E, bool SWIGLU, int RT>
__global__ __launch_bounds__(MX_THREADS) void gemv_mx4_kernel(
    const typename E::T* __restrict__ x, const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales,
    const typename E::T* __restrict__ res, typename E::T* __restrict__ y, int N, int K, int R, int ntiles) {
  typedef typename E::T T;
  constexpr int NW = SWIGLU ? 2 : 1;  // weight rows per output: g and u
  __shared__ uint4 xs[RT * MX_CHUNK_VECS];
  const int gl = threadIdx.x & (MX_GROUP - 1);  // the lane's place in its half wave: its unit of a chunk
  const int tile = blockIdx.x % ntiles;
  const int out_row = (blockIdx.x / ntiles) * MX_WG_ROWS + threadIdx.x / MX_GROUP;
  const int row = min(out_row, N - 1);
  const int r0 = tile * RT;
  const int kb = K / MX_BLOCK;  // scale bytes per row
  // whole-dword scale loads need every row's scales dword-aligned and every unit whole
  const bool dwords = (kb & 3) == 0;
  const uint8_t* cw[NW];
  const uint8_t* sw[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    cw[w] = codes + ((long)row + (long)w * N) * (K / 2);
    sw[w] = scales + ((long)row + (long)w * N) * kb;
  }
  const T* xr[RT];
  float acc[NW][RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    xr[r] = x + (long)min(r0 + r, R - 1) * K;
#pragma unroll
    for (int w = 0; w < NW; ++w) acc[w][r] = 0.f;
  }
  bool poison = false;
  for (int base = 0; base < K; base += MX_CHUNK) {
    // this lane's unit: nb of its four blocks lie inside K
    const int k0 = base + gl * MX_UNIT;
    const int nb = min(max((K - k0) / MX_BLOCK, 0), 4);
    uint4 wv[NW][4];
    uint32_t se[NW];  // four scale bytes; a block outside K: 127 (a factor of 1 on a zero sum)
#pragma unroll
    for (int w = 0; w < NW; ++w) {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        wv[w][b] = b < nb ? *reinterpret_cast<const uint4*>(cw[w] + k0 / 2 + b * 16) : make_uint4(0u, 0u, 0u, 0u);
      if (dwords) {
        se[w] = nb > 0 ? *reinterpret_cast<const uint32_t*>(sw[w] + k0 / MX_BLOCK) : 0x7f7f7f7fu;
      } else {
        se[w] = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) se[w] |= (b < nb ? (uint32_t)sw[w][k0 / MX_BLOCK + b] : 127u) << (8 * b);
      }
      poison = poison || has_ff(se[w]);
    }
    // stage the chunk of the tile's activation rows (K % 32 == 0: whole vectors)
    const int nv = min(MX_CHUNK, K - base) / 8;
    for (int i = threadIdx.x; i < RT * nv; i += MX_THREADS) {
      const int r = i / nv, v = i - r * nv;
      xs[r * MX_CHUNK_VECS + xs_at(v >> 4, v & 15)] = *reinterpret_cast<const uint4*>(xr[r] + base + v * 8);
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (b < nb) {  // the vectors of a block outside K were not staged
        uint32_t wp[NW][16];
        float f[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          block_to_pairs<E>(wv[w][b], wp[w]);
          f[w] = __uint_as_float(((se[w] >> (8 * b)) & 0xffu) << 23);
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
          uint4 xv[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) xv[j] = xs[r * MX_CHUNK_VECS + xs_at(gl, 4 * b + j)];
#pragma unroll
          for (int w = 0; w < NW; ++w) acc[w][r] = fmaf(block_dot<E>(wp[w], xv), f[w], acc[w][r]);
        }
      }
    }
    __syncthreads();  // the next chunk overwrites xs
  }
  const float nan = __uint_as_float(0x7fc00000u);
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    const float s = group_sum(poison ? nan : acc[0][r]);
    const bool store = gl == 0 && r0 + r < R && out_row < N;
    const long at = (long)(r0 + r) * N + row;
    if constexpr (SWIGLU) {
      const float t = group_sum(poison ? nan : acc[1][r]);
      if (store) {
        // g, u and silu(g) each rounded to the model dtype, as in decode.hip's gemv_kernel: the
        // composed gemv_mx4 -> silu -> mul
        const float g = rnd<E>(s), u = rnd<E>(t);
        const float sl = rnd<E>(g / (1.f + expf(-g)));
        y[at] = cvt1<E>(sl * u);
      }
    } else if (store) {
      y[at] = cvt1<E>(res != nullptr ? s + ld1<E>(res + at) : s);
    }
  }
}

// --------------------------------------------------------------------------------------------
// quantize_rows_mxfp4. Blocks do not depend on each other, and [N, K] is contiguous, so the kernel is
// flat over the N K / 32 blocks: one lane per block reads its 32 weights (four 16-byte loads), finds
// amax on the bit patterns of |w| (for non-negative floats the integer order is the float order, with
// infinity and every NaN above all finite values), derives the scale byte from amax's exponent and
// mantissa fields, and writes 16 bytes of codes and the byte. The code of v = |w| 2^-p is counted out
// against the seven midpoints, a tie going to the even code: v > 0.25, >= 0.75, > 1.25, >= 1.75,
// > 2.5, >= 3.5, > 5.
// --------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t e2m1_code(float w, float inv) {
  const float v = fabsf(w) * inv;  // exact: inv is a power of two
  const uint32_t c = (uint32_t)(v > 0.25f) + (uint32_t)(v >= 0.75f) + (uint32_t)(v > 1.25f) + (uint32_t)(v >= 1.75f) +
                     (uint32_t)(v > 2.5f) + (uint32_t)(v >= 3.5f) + (uint32_t)(v > 5.f);
  return c | ((__float_as_uint(w) >> 28) & 8u);
}

template <class E>
__global__ __launch_bounds__(256) void quantize_mxfp4_kernel(const typename E::T* __restrict__ w,
                                                             uint8_t* __restrict__ codes,
                                                             uint8_t* __restrict__ scales, long nblocks) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= nblocks) return;
  float f[MX_BLOCK];
#pragma unroll
  for (int j = 0; j < 4; ++j) unpack8e<E>(*reinterpret_cast<const uint4*>(w + g * MX_BLOCK + j * 8), f + j * 8);
  uint32_t m = 0u;
#pragma unroll
  for (int j = 0; j < MX_BLOCK; ++j) m = max(m, __float_as_uint(f[j]) & 0x7fffffffu);
  uint4 c = make_uint4(0u, 0u, 0u, 0u);
  uint32_t e = 255u;
  if (m < 0x7f800000u) {
    // amax = (1 + M / 2^23) 2^(E - 127) = m' 2^(E - 126) with m' in [0.5, 1), m' <= 0.75 where
    // M <= 2^22: p = E - 129 (+ 1 above), e = p + 127. An fp32 subnormal amax (E = 0) clamps to 1.
    const int ee = (int)(m >> 23) - 2 + (int)((m & 0x7fffffu) > 0x400000u);
    e = m == 0u ? 127u : (uint32_t)min(max(ee, 1), 254);
    const float inv = __uint_as_float((254u - e) << 23);  // 2^(127 - e), e <= 253 here: amax < 2^128
    uint32_t d[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      d[i] = 0u;
#pragma unroll
      for (int j = 0; j < 8; ++j) d[i] |= e2m1_code(f[8 * i + j], inv) << (4 * j);
    }
    c = make_uint4(d[0], d[1], d[2], d[3]);
  }
  *reinterpret_cast<uint4*>(codes + g * (MX_BLOCK / 2)) = c;
  scales[g] = (uint8_t)e;
}

// codes uint8 [rows, K / 2] and scales uint8 [rows, K / 32] of one weight, on `dev`
void check_pair(const char* op, const at::Tensor& codes, const at::Tensor& scales, c10::Device dev) {
  check_vec(op, codes, "codes");
  check_vec(op, scales, "scales");
  TORCH_CHECK(codes.scalar_type() == at::kByte && scales.scalar_type() == at::kByte, op,
              ": codes (two e2m1 codes per byte) and scales (e8m0) must be uint8");
  TORCH_CHECK(codes.device() == dev && scales.device() == dev, op, ": device mismatch");
  TORCH_CHECK(codes.dim() == 2 && codes.size(0) > 0 && codes.size(1) > 0 && codes.size(1) % (MX_BLOCK / 2) == 0, op,
              ": codes [N, K / 2] with K a positive multiple of 32 (one 16-byte vector of codes per scale)");
  TORCH_CHECK(scales.dim() == 2 && scales.size(0) == codes.size(0) && scales.size(1) * (MX_BLOCK / 2) == codes.size(1),
              op, ": scales must be [N, K / 32]");
}

void quantize_rows_mxfp4_out(const at::Tensor& w, at::Tensor codes, at::Tensor scales) {
  const char* op = "quantize_rows_mxfp4";
  check_vec(op, w, "w");
  TORCH_CHECK(w.scalar_type() == at::kBFloat16 || w.scalar_type() == at::kHalf, op, ": w must be bf16 or fp16");
  TORCH_CHECK(w.dim() == 2 && w.size(0) > 0 && w.size(1) > 0 && w.size(1) % MX_BLOCK == 0, op,
              ": w [N, K] with K a positive multiple of 32");
  check_pair(op, codes, scales, w.device());
  TORCH_CHECK(codes.size(0) == w.size(0) && codes.size(1) * 2 == w.size(1), op, ": codes must be [N, K / 2]");
  const int64_t nblocks = w.numel() / MX_BLOCK;
  const int64_t grid = (nblocks + 255) / 256;
  TORCH_CHECK(grid <= INT_MAX, op, ": too many blocks");
  const at::DeviceGuard guard(w.device());
  FT_DISPATCH_E16(w.scalar_type(), {
    hipLaunchKernelGGL((quantize_mxfp4_kernel<E>), dim3((unsigned)grid), dim3(256), 0, ft_stream(),
                       cptr<typename E::T>(w), mptr<uint8_t>(codes), mptr<uint8_t>(scales), (long)nblocks);
  });
  FT_LAUNCH_CHECK();
}

std::tuple<at::Tensor, at::Tensor> quantize_rows_mxfp4(const at::Tensor& w) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 2 && w.size(1) % MX_BLOCK == 0,
              "quantize_rows_mxfp4: w must be a GPU tensor [N, K] with K a multiple of 32");
  const at::DeviceGuard guard(w.device());
  auto codes = at::empty({w.size(0), w.size(1) / 2}, w.options().dtype(at::kByte));
  auto scales = at::empty({w.size(0), w.size(1) / MX_BLOCK}, w.options().dtype(at::kByte));
  quantize_rows_mxfp4_out(w, codes, scales);
  return {codes, scales};
}

// The tile height of the multi-row ops: R <= 8 takes the smallest of 1, 2, 4, 8 that holds it; above,
// tiles of 8 rows (64 KB of staged activations, two workgroups per CU).
constexpr int MX_ROWS_TILE = 8;

// x [K] (rows == false) or [R, K]; the result is [N] or [R, N].
template <bool SWIGLU>
at::Tensor gemv_mx4_impl(const char* op, bool rows, const at::Tensor& x, const at::Tensor& codes,
                         const at::Tensor& scales, const c10::optional<at::Tensor>& residual) {
  check_vec(op, x, "x");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf, op, ": x must be bf16 or fp16");
  check_pair(op, codes, scales, x.device());
  const int64_t R = rows ? x.size(0) : 1, nrows = codes.size(0), K = codes.size(1) * 2;
  TORCH_CHECK(x.dim() == (rows ? 2 : 1) && x.size(-1) == K, op,
              rows ? ": x [R, K], codes [N, K / 2]" : ": x [K], codes [N, K / 2]");
  TORCH_CHECK(R >= 1 && R <= INT_MAX, op, ": x needs at least one row");
  TORCH_CHECK(nrows <= INT_MAX - MX_WG_ROWS && K <= INT_MAX - 2 * MX_CHUNK, op, ": N and K must fit 32 bits");
  TORCH_CHECK(!SWIGLU || nrows % 2 == 0, op, ": codes13 must be [2H, K / 2]");
  const int64_t N = SWIGLU ? nrows / 2 : nrows;
  const bool has_res = residual.has_value() && residual->defined();
  if (has_res) check_residual(op, *residual, x, N);
  const int rt = rows_tile(R, MX_ROWS_TILE);
  const int64_t ntiles = (R + rt - 1) / rt;
  const int64_t blocks = (N + MX_WG_ROWS - 1) / MX_WG_ROWS * ntiles;
  TORCH_CHECK(blocks <= INT_MAX, op, ": too many workgroups (output rows x row tiles)");
  const at::DeviceGuard guard(x.device());
  auto y = rows ? at::empty({R, N}, x.options()) : at::empty({N}, x.options());
  FT_DISPATCH_E16(x.scalar_type(), FT_ROWS_TILE(rt, MX_ROWS_TILE, {
    hipLaunchKernelGGL((gemv_mx4_kernel<E, SWIGLU, RT>), dim3((unsigned)blocks), dim3(MX_THREADS), 0, ft_stream(),
                       cptr<typename E::T>(x), cptr<uint8_t>(codes), cptr<uint8_t>(scales),
                       has_res ? cptr<typename E::T>(*residual) : nullptr, mptr<typename E::T>(y), (int)N, (int)K,
                       (int)R, (int)ntiles);
  }));
  FT_LAUNCH_CHECK();
  return y;
}

at::Tensor gemv_mx4(const at::Tensor& x, const at::Tensor& codes, const at::Tensor& scales,
                    const c10::optional<at::Tensor>& residual) {
  return gemv_mx4_impl<false>("gemv_mx4", false, x, codes, scales, residual);
}

at::Tensor gemv_swiglu_mx4(const at::Tensor& x, const at::Tensor& codes13, const at::Tensor& scales13) {
  return gemv_mx4_impl<true>("gemv_swiglu_mx4", false, x, codes13, scales13, c10::nullopt);
}

// y[R, N]; row r has the bits of gemv_mx4(x[r], codes, scales, residual[r]).
at::Tensor gemv_rows_mx4(const at::Tensor& x, const at::Tensor& codes, const at::Tensor& scales,
                         const c10::optional<at::Tensor>& residual) {
  return gemv_mx4_impl<false>("gemv_rows_mx4", true, x, codes, scales, residual);
}

// a[R, H]; row r has the bits of gemv_swiglu_mx4(x[r], codes13, scales13).
at::Tensor gemv_swiglu_rows_mx4(const at::Tensor& x, const at::Tensor& codes13, const at::Tensor& scales13) {
  return gemv_mx4_impl<true>("gemv_swiglu_rows_mx4", true, x, codes13, scales13, c10::nullopt);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(ftamd, m) {
  m.def("quantize_rows_mxfp4(Tensor w) -> (Tensor, Tensor)", &quantize_rows_mxfp4);
  m.def("quantize_rows_mxfp4_out(Tensor w, Tensor(a!) codes, Tensor(b!) scales) -> ()", &quantize_rows_mxfp4_out);
  m.def("gemv_mx4(Tensor x, Tensor codes, Tensor scales, Tensor? residual) -> Tensor", &gemv_mx4);
  m.def("gemv_swiglu_mx4(Tensor x, Tensor codes13, Tensor scales13) -> Tensor", &gemv_swiglu_mx4);
  m.def("gemv_rows_mx4(Tensor x, Tensor codes, Tensor scales, Tensor? residual) -> Tensor", &gemv_rows_mx4);
  m.def("gemv_swiglu_rows_mx4(Tensor x, Tensor codes13, Tensor scales13) -> Tensor", &gemv_swiglu_rows_mx4);
}
