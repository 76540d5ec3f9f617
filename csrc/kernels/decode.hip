// Text generation: the one-row (decode) kernels. The reference has no generation path at all; the
// math is its model (model.py:179-215, :253-254, :379) applied to one new token against a cache of
// the earlier tokens' rotated K and V.
//
// Decoding is a different regime from every other file here: one activation row against all the
// weights, so every kernel is bound by HBM bandwidth and is plain vector code -- 16-byte loads
// straight into registers, several in flight per lane, fp32 accumulation, no LDS staging of the
// streamed operand, no matrix cores, no inline assembly.
//
//   gemv                y[N] = W[N, K] x[K] (+ residual[N])        one wave per output row
//   gemv_swiglu         a[H] = silu(w1 x) * (w3 x) from [w1; w3]    one wave per feature, both rows
//   decode_qkv_append_  RoPE at `pos` on Q (in place) and K (into k_cache[:, pos]); V into v_cache[:, pos]
//   decode_attn         one query over keys 0 .. n_keys-1 of the cache, GQA indexed in place
//   sample_             one token per row of logits: greedy, or temperature / top-k / top-p sampling
//
// Batched generation (B sequences per pass over the weights) has a `_rows` form of the first four:
// gemv_rows, gemv_swiglu_rows, decode_qkv_append_rows_, decode_attn_rows. Each returns for row r the
// bits the one-row op returns for that row alone: the per-row arithmetic is shared code (dotf,
// qkv_append_vec, attn_chunk, attn_merge) run in the same order.
//
// Reproducibility: nothing on a result path is accumulated with atomics and every reduction has a
// fixed order (per-lane sweep, xor butterfly over the wave, waves in index order, key chunks in
// chunk order), so each op returns the same bits from run to run. The sampler's top-k threshold is
// found with integer histograms in LDS (integer counts do not depend on the order of the adds), and
// its top-p threshold with histograms of 64-bit fixed-point weights (integer adds again).
//
// Positions, key counts and the sampler's step are host integers (kernel arguments); the `_rows` ops
// take each row's start position from a device tensor `pos0` plus one host integer `t`.
//
// The device-step forms (decode_qkv_append_rows_dev_, decode_attn_rows_dev, sample_dev_) are the
// `_rows` ops and the sampler with every per-token value read from a control block `ctl` in device
// memory (CTL_* below) and with grids that do not depend on it, so one captured launch of each is
// right for any token of any call (generation.DecodeGraph). They run the same per-row code and
// return the same bits. decode_ctl_advance_ steps the counter in a launch of its own, after every
// reader of the pass.
#include <climits>
#include <type_traits>

#include "sround.h"
#include "torch_utils.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
// keys per workgroup of decode_attn; the chunk partials are merged in chunk order
constexpr int DECODE_CHUNK = 128;
constexpr int SAMPLE_MAX_BLOCKS = 32768;

// The control block of the device-step ops: int32 words (ops/decode.py keeps the same indices). The
// host writes it once per call; the kernels only read it, but for decode_ctl_advance_ on CTL_T.
enum : int {
  CTL_T = 0,            // the decode step: new token t of the call
  CTL_KEY_LO = 1,       // the call's sampler key (token_key is formed from it and t)
  CTL_KEY_HI = 2,
  CTL_STEP = 3,         // the sampler's step
  CTL_TEMPERATURE = 4,  // float bits
  CTL_TOP_K = 5,
  CTL_TOP_P = 6,        // float bits; 0 (what a writer that knows no top-p leaves) or >= 1: off
  CTL_WORDS = 8
};

// ---- one 16-byte vector of the model dtype: 8 elements (bf16 / fp16) or 4 (fp32)
template <class E>
struct V16 {
  static constexpr int N = E::is16 ? 8 : 4;
};

template <class E>
__device__ __forceinline__ void unpv(const uint4& v, float* f) {
  if constexpr (E::is16) {
    unpack8e<E>(v, f);
  } else {
    f[0] = __uint_as_float(v.x);
    f[1] = __uint_as_float(v.y);
    f[2] = __uint_as_float(v.z);
    f[3] = __uint_as_float(v.w);
  }
}

// --------------------------------------------------------------------------------------------
// gemv / gemv_swiglu. One wave per output row (SWIGLU: rows h and H + h of [w1; w3]); lane l takes
// the 16-byte vectors l, l + 64, ... of the row, four of them in flight per row, each into its own
// fp32 accumulator; x comes from the cache (every wave reads the same K elements). The lane sums
// are added as (a0 + a1) + (a2 + a3), then the xor butterfly over the wave.
// --------------------------------------------------------------------------------------------
template <int VN>
__device__ __forceinline__ float dotf(const float* wf, const float* xf, float acc) {
#pragma unroll
  for (int j = 0; j < VN; ++j) acc = fmaf(wf[j], xf[j], acc);
  return acc;
}

template <class E, int VN>
__device__ __forceinline__ float dotv(const uint4& wv, const float* xf, float acc) {
  float wf[8];
  unpv<E>(wv, wf);
  return dotf<VN>(wf, xf, acc);
}

template <class E, bool SWIGLU>
__global__ __launch_bounds__(256) void gemv_kernel(const typename E::T* __restrict__ x,
                                                   const typename E::T* __restrict__ w,
                                                   const typename E::T* __restrict__ res,
                                                   typename E::T* __restrict__ y, int N, int K) {
  constexpr int VN = V16<E>::N;
  constexpr int STEP = 64 * VN;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;  // whole waves leave; the kernel has no block barrier
  const typename E::T* w0 = w + (long)row * K;
  const typename E::T* w1 = w + ((long)row + N) * K;  // SWIGLU only: the w3 row of feature `row`
  float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
  int k = lane * VN;
  for (; k + 3 * STEP < K; k += 4 * STEP) {
    uint4 wv[4], uv[4], xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      wv[u] = *reinterpret_cast<const uint4*>(w0 + k + u * STEP);
      if constexpr (SWIGLU) uv[u] = *reinterpret_cast<const uint4*>(w1 + k + u * STEP);
      xv[u] = *reinterpret_cast<const uint4*>(x + k + u * STEP);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float xf[8];
      unpv<E>(xv[u], xf);
      a[u] = dotv<E, VN>(wv[u], xf, a[u]);
      if constexpr (SWIGLU) b[u] = dotv<E, VN>(uv[u], xf, b[u]);
    }
  }
  for (; k < K; k += STEP) {
    float xf[8];
    unpv<E>(*reinterpret_cast<const uint4*>(x + k), xf);
    a[0] = dotv<E, VN>(*reinterpret_cast<const uint4*>(w0 + k), xf, a[0]);
    if constexpr (SWIGLU) b[0] = dotv<E, VN>(*reinterpret_cast<const uint4*>(w1 + k), xf, b[0]);
  }
  float s = wave_sum((a[0] + a[1]) + (a[2] + a[3]));
  if constexpr (SWIGLU) {
    const float t = wave_sum((b[0] + b[1]) + (b[2] + b[3]));
    if (lane == 0) {
      // g, u and silu(g) each rounded to the model dtype: the composed gemv -> silu -> mul
      const float g = rnd<E>(s), u = rnd<E>(t);
      const float sl = rnd<E>(g / (1.f + expf(-g)));
      y[row] = cvt1<E>(sl * u);
    }
  } else if (lane == 0) {
    if (res != nullptr) s += ld1<E>(res + row);
    y[row] = cvt1<E>(s);
  }
}

// --------------------------------------------------------------------------------------------
// gemv_rows / gemv_swiglu_rows: x [R, K]. The wave of gemv_kernel, with every 16-byte weight vector
// used for a tile of RT activation rows r0 .. r0 + RT - 1 (r0 = tile * RT); per activation row the
// accumulators a[r][u], the k each of them sees, the tail into a[r][0] and the final adds are those
// of gemv_kernel, so y[r] has the bits of gemv on x[r]. Rows of the tile at and beyond R are computed
// on row R - 1 again and not stored (no divergence in the sweep). The tiles of one block of output
// rows are neighbours in the grid, so the tiles after the first find the weights in a cache.
// --------------------------------------------------------------------------------------------
template <class E, bool SWIGLU, int RT>
__global__ __launch_bounds__(256) void gemv_rows_kernel(const typename E::T* __restrict__ x,
                                                        const typename E::T* __restrict__ w,
                                                        const typename E::T* __restrict__ res,
                                                        typename E::T* __restrict__ y, int N, int K, int R,
                                                        int ntiles) {
  constexpr int VN = V16<E>::N;
  constexpr int STEP = 64 * VN;
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x % ntiles;
  const int row = (blockIdx.x / ntiles) * 4 + (threadIdx.x >> 6);
  if (row >= N) return;  // whole waves leave; the kernel has no block barrier
  const int r0 = tile * RT;
  const typename E::T* w0 = w + (long)row * K;
  const typename E::T* w1 = w + ((long)row + N) * K;  // SWIGLU only: the w3 row of feature `row`
  const typename E::T* xr[RT];
  float a[RT][4], b[RT][4];
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    xr[r] = x + (long)min(r0 + r, R - 1) * K;
#pragma unroll
    for (int u = 0; u < 4; ++u) a[r][u] = b[r][u] = 0.f;
  }
  int k = lane * VN;
  for (; k + 3 * STEP < K; k += 4 * STEP) {
    uint4 wv[4], uv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      wv[u] = *reinterpret_cast<const uint4*>(w0 + k + u * STEP);
      if constexpr (SWIGLU) uv[u] = *reinterpret_cast<const uint4*>(w1 + k + u * STEP);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float wf[8], uf[8];
      unpv<E>(wv[u], wf);
      if constexpr (SWIGLU) unpv<E>(uv[u], uf);
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        float xf[8];
        unpv<E>(*reinterpret_cast<const uint4*>(xr[r] + k + u * STEP), xf);
        a[r][u] = dotf<VN>(wf, xf, a[r][u]);
        if constexpr (SWIGLU) b[r][u] = dotf<VN>(uf, xf, b[r][u]);
      }
    }
  }
  for (; k < K; k += STEP) {
    float wf[8], uf[8];
    unpv<E>(*reinterpret_cast<const uint4*>(w0 + k), wf);
    if constexpr (SWIGLU) unpv<E>(*reinterpret_cast<const uint4*>(w1 + k), uf);
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      float xf[8];
      unpv<E>(*reinterpret_cast<const uint4*>(xr[r] + k), xf);
      a[r][0] = dotf<VN>(wf, xf, a[r][0]);
      if constexpr (SWIGLU) b[r][0] = dotf<VN>(uf, xf, b[r][0]);
    }
  }
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    float s = wave_sum((a[r][0] + a[r][1]) + (a[r][2] + a[r][3]));
    const bool store = lane == 0 && r0 + r < R;
    const long at = (long)(r0 + r) * N + row;
    if constexpr (SWIGLU) {
      const float t = wave_sum((b[r][0] + b[r][1]) + (b[r][2] + b[r][3]));
      if (store) {
        // g, u and silu(g) each rounded to the model dtype, as in gemv_kernel
        const float g = rnd<E>(s), u = rnd<E>(t);
        const float sl = rnd<E>(g / (1.f + expf(-g)));
        y[at] = cvt1<E>(sl * u);
      }
    } else if (store) {
      if (res != nullptr) s += ld1<E>(res + at);
      y[at] = cvt1<E>(s);
    }
  }
}

// --------------------------------------------------------------------------------------------
// decode_qkv_append_: qkv [(Hq + 2 Hkv) D] of the new token. One thread per 8 columns (4 pairs).
// --------------------------------------------------------------------------------------------
template <class E>
__device__ __forceinline__ void qkv_append_vec(int i, typename E::T* __restrict__ qkv,
                                               const float* __restrict__ cos_row,
                                               const float* __restrict__ sin_row, typename E::T* __restrict__ kc,
                                               typename E::T* __restrict__ vc, int hq, int hkv, int d, long smax,
                                               long pos) {
  const int col = i * 8, head = col / d, within = col - head * d;
  float x[8];
  ld8<E>(qkv + col, x);
  if (head < hq + hkv) {
    const float4 c = *reinterpret_cast<const float4*>(cos_row + (within >> 1));
    const float4 s = *reinterpret_cast<const float4*>(sin_row + (within >> 1));
    const float cc[4] = {c.x, c.y, c.z, c.w}, ss[4] = {s.x, s.y, s.z, s.w};
    float r[8];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float a = x[2 * p], b = x[2 * p + 1];
      r[2 * p] = a * cc[p] - b * ss[p];
      r[2 * p + 1] = a * ss[p] + b * cc[p];
    }
    if (head < hq) st8<E>(qkv + col, r);
    else st8<E>(kc + ((long)(head - hq) * smax + pos) * d + within, r);
  } else {
    st8<E>(vc + ((long)(head - hq - hkv) * smax + pos) * d + within, x);
  }
}

template <class E>
__global__ __launch_bounds__(256) void qkv_append_kernel(typename E::T* __restrict__ qkv,
                                                         const float* __restrict__ cos_row,
                                                         const float* __restrict__ sin_row,
                                                         typename E::T* __restrict__ kc,
                                                         typename E::T* __restrict__ vc, int hq, int hkv, int d,
                                                         long smax, long pos) {
  const int nvec = (hq + 2 * hkv) * d / 8;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  qkv_append_vec<E>(i, qkv, cos_row, sin_row, kc, vc, hq, hkv, d, smax, pos);
}

// decode_qkv_append_rows_: qkv [B, (Hq + 2 Hkv) D], caches [B, Hkv, Smax, D]; blockIdx.y is the row b,
// rotated and stored at pos0[b] + t. A position outside [0, limit) -- the host checked the largest one
// the caller named, not pos0 itself -- writes nothing.
template <class E>
__device__ __forceinline__ void qkv_append_row(typename E::T* __restrict__ qkv, const float* __restrict__ cos_t,
                                               const float* __restrict__ sin_t, const int* __restrict__ pos0, int t,
                                               typename E::T* __restrict__ kc, typename E::T* __restrict__ vc, int hq,
                                               int hkv, int d, long smax, long limit) {
  const int nvec = (hq + 2 * hkv) * d / 8;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  const long pos = (long)pos0[b] + t;
  if (i >= nvec || pos < 0 || pos >= limit) return;
  const long cstride = (long)hkv * smax * d;
  qkv_append_vec<E>(i, qkv + (long)b * nvec * 8, cos_t + pos * (d / 2), sin_t + pos * (d / 2), kc + b * cstride,
                    vc + b * cstride, hq, hkv, d, smax, pos);
}

template <class E>
__global__ __launch_bounds__(256) void qkv_append_rows_kernel(typename E::T* __restrict__ qkv,
                                                              const float* __restrict__ cos_t,
                                                              const float* __restrict__ sin_t,
                                                              const int* __restrict__ pos0, int t,
                                                              typename E::T* __restrict__ kc,
                                                              typename E::T* __restrict__ vc, int hq, int hkv,
                                                              int d, long smax, long limit) {
  qkv_append_row<E>(qkv, cos_t, sin_t, pos0, t, kc, vc, hq, hkv, d, smax, limit);
}

// decode_qkv_append_rows_dev_: t from the control block; limit is the capacity (the cache and the
// RoPE tables), the only bound the host can name without knowing t.
template <class E>
__global__ __launch_bounds__(256) void qkv_append_rows_dev_kernel(typename E::T* __restrict__ qkv,
                                                                  const float* __restrict__ cos_t,
                                                                  const float* __restrict__ sin_t,
                                                                  const int* __restrict__ pos0,
                                                                  const int* __restrict__ ctl,
                                                                  typename E::T* __restrict__ kc,
                                                                  typename E::T* __restrict__ vc, int hq, int hkv,
                                                                  int d, long smax, long limit) {
  qkv_append_row<E>(qkv, cos_t, sin_t, pos0, ctl[CTL_T], kc, vc, hq, hkv, d, smax, limit);
}

// --------------------------------------------------------------------------------------------
// decode_attn. Workgroup (kv head, chunk of DECODE_CHUNK keys), 256 threads. D / 8 lanes share a key
// row (16 bytes of it each), so a pass covers 256 / (D / 8) keys; every K and V row is loaded once
// and used for all the G = Hq / Hkv query heads of the group (in tiles of GT heads: one tile for
// G <= 8). Per head the workgroup leaves (acc[D] unnormalised, m, l) of its chunk; the merge
// kernel folds the chunks in chunk order. Keys at and beyond n_keys are never loaded.
//
// attn_chunk is the workgroup's work on one sequence (q [Hq D], caches [Hkv, Smax, D], part
// [chunks, Hq, D + 2]); decode_attn_kernel runs it on the one sequence, decode_attn_rows_kernel on
// sequence blockIdx.z of a batch.
// --------------------------------------------------------------------------------------------
template <class E, int D, int GT>
__device__ __forceinline__ void attn_chunk(const typename E::T* __restrict__ q,
                                           const typename E::T* __restrict__ kc,
                                           const typename E::T* __restrict__ vc, float* __restrict__ part,
                                           int hq, int hkv, long smax, int n_keys, float scale) {
  constexpr int LPK = D / 8;     // lanes per key row
  constexpr int KPP = 256 / LPK;  // keys per pass
  __shared__ float sq[GT * D];
  __shared__ float sp[GT][DECODE_CHUNK];
  __shared__ float sred[4][GT][D];
  __shared__ float s_m[GT], s_l[GT];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int sub = tid % LPK, kslot = tid / LPK;
  const int kvh = blockIdx.x, chunk = blockIdx.y;
  const int G = hq / hkv;
  const int k0 = chunk * DECODE_CHUNK;
  const int nk = min(DECODE_CHUNK, n_keys - k0);  // >= 1: the grid covers ceil(n_keys / chunk) chunks
  const typename E::T* kbase = kc + ((long)kvh * smax + k0) * D;
  const typename E::T* vbase = vc + ((long)kvh * smax + k0) * D;
  for (int g0 = 0; g0 < G; g0 += GT) {
    for (int i = tid; i < GT * D; i += 256)
      sq[i] = (g0 + i / D < G) ? ld1<E>(q + ((long)kvh * G + g0) * D + i) : 0.f;
    __syncthreads();
    // scores of the chunk: sp[g][key] = scale * <q_g, k_key>, -inf beyond the live keys
    for (int kk = kslot; kk < DECODE_CHUNK; kk += KPP) {
      const bool live = kk < nk;
      float kx[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (live) ld8<E>(kbase + (long)kk * D + sub * 8, kx);
#pragma unroll
      for (int g = 0; g < GT; ++g) {
        float dp = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) dp = fmaf(kx[j], sq[g * D + sub * 8 + j], dp);
#pragma unroll
        for (int o = LPK / 2; o > 0; o >>= 1) dp += __shfl_xor(dp, o, 64);
        if (sub == 0) sp[g][kk] = live ? dp * scale : -INFINITY;
      }
    }
    __syncthreads();
    // per head: chunk maximum, p = exp(s - m), l = sum p (one wave per head)
    for (int g = wid; g < GT; g += 4) {
      float m = -INFINITY;
#pragma unroll
      for (int i = 0; i < DECODE_CHUNK / 64; ++i) m = fmaxf(m, sp[g][lane + 64 * i]);
      m = wave_max(m);
      float l = 0.f;
#pragma unroll
      for (int i = 0; i < DECODE_CHUNK / 64; ++i) {
        const float p = exp2f((sp[g][lane + 64 * i] - m) * LOG2E);
        sp[g][lane + 64 * i] = p;
        l += p;
      }
      l = wave_sum(l);
      if (lane == 0) {
        s_m[g] = m;
        s_l[g] = l;
      }
    }
    __syncthreads();
    // acc[g][8 dims of this thread] over the thread's keys, then over the key slots
    float acc[GT][8];
#pragma unroll
    for (int g = 0; g < GT; ++g)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[g][j] = 0.f;
    for (int kk = kslot; kk < nk; kk += KPP) {
      float vx[8];
      ld8<E>(vbase + (long)kk * D + sub * 8, vx);
#pragma unroll
      for (int g = 0; g < GT; ++g) {
        const float p = sp[g][kk];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[g][j] = fmaf(p, vx[j], acc[g][j]);
      }
    }
#pragma unroll
    for (int g = 0; g < GT; ++g)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = acc[g][j];
#pragma unroll
        for (int o = LPK; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
        if (lane < LPK) sred[wid][g][sub * 8 + j] = v;
      }
    __syncthreads();
    for (int i = tid; i < GT * D; i += 256) {
      const int g = i / D, dd = i - g * D;
      if (g0 + g < G) {
        const float v = ((sred[0][g][dd] + sred[1][g][dd]) + sred[2][g][dd]) + sred[3][g][dd];
        part[((long)chunk * hq + (long)kvh * G + g0 + g) * (D + 2) + dd] = v;
      }
    }
    if (tid < GT && g0 + tid < G) {
      float* pr = part + ((long)chunk * hq + (long)kvh * G + g0 + tid) * (D + 2) + D;
      pr[0] = s_m[tid];
      pr[1] = s_l[tid];
    }
    __syncthreads();  // the next tile reuses the shared arrays
  }
}

template <class E, int D, int GT>
__global__ __launch_bounds__(256) void decode_attn_kernel(const typename E::T* __restrict__ q,
                                                          const typename E::T* __restrict__ kc,
                                                          const typename E::T* __restrict__ vc,
                                                          float* __restrict__ part, int hq, int hkv, long smax,
                                                          int n_keys, float scale) {
  attn_chunk<E, D, GT>(q, kc, vc, part, hq, hkv, smax, n_keys, scale);
}

// The key count of row b of a batch: pos0[b] + t + 1, at most max_keys (which the host checked
// against Smax; pos0 itself is never read back). Below 1 no workgroup of the row does anything.
__device__ __forceinline__ int row_keys(const int* __restrict__ pos0, int b, int t, int max_keys) {
  return (int)min((long)pos0[b] + t + 1, (long)max_keys);
}

// Grid (Hkv, ceil(max_keys / DECODE_CHUNK), B); q rows q_stride elements apart (the Q columns of a
// qkv buffer, in place); part [B, gridDim.y, Hq, D + 2]. A workgroup whose chunk
// starts at or beyond its row's key count leaves here, all of it, before the first barrier: its
// slice of `part` stays unwritten and the merge below never reads it.
template <class E, int D, int GT>
__device__ __forceinline__ void attn_rows_chunk(const typename E::T* __restrict__ q,
                                                const typename E::T* __restrict__ kc,
                                                const typename E::T* __restrict__ vc, float* __restrict__ part,
                                                const int* __restrict__ pos0, int t, int max_keys, long q_stride,
                                                int hq, int hkv, long smax, float scale) {
  const int b = blockIdx.z;
  const int n_keys = row_keys(pos0, b, t, max_keys);
  if ((int)blockIdx.y * DECODE_CHUNK >= n_keys) return;  // uniform over the workgroup
  const long cstride = (long)hkv * smax * D;
  attn_chunk<E, D, GT>(q + b * q_stride, kc + b * cstride, vc + b * cstride,
                       part + (long)b * gridDim.y * hq * (D + 2), hq, hkv, smax, n_keys, scale);
}

template <class E, int D, int GT>
__global__ __launch_bounds__(256) void decode_attn_rows_kernel(const typename E::T* __restrict__ q,
                                                               const typename E::T* __restrict__ kc,
                                                               const typename E::T* __restrict__ vc,
                                                               float* __restrict__ part,
                                                               const int* __restrict__ pos0, int t, int max_keys,
                                                               long q_stride, int hq, int hkv, long smax,
                                                               float scale) {
  attn_rows_chunk<E, D, GT>(q, kc, vc, part, pos0, t, max_keys, q_stride, hq, hkv, smax, scale);
}

// decode_attn_rows_dev: t from the control block, the grid over the whole capacity (max_keys = Smax),
// so most workgroups of a short row leave at the test above.
template <class E, int D, int GT>
__global__ __launch_bounds__(256) void decode_attn_rows_dev_kernel(const typename E::T* __restrict__ q,
                                                                   const typename E::T* __restrict__ kc,
                                                                   const typename E::T* __restrict__ vc,
                                                                   float* __restrict__ part,
                                                                   const int* __restrict__ pos0,
                                                                   const int* __restrict__ ctl, long q_stride,
                                                                   int hq, int hkv, long smax, float scale) {
  attn_rows_chunk<E, D, GT>(q, kc, vc, part, pos0, ctl[CTL_T], (int)smax, q_stride, hq, hkv, smax, scale);
}

// One workgroup per query head, one thread per dim: the chunk partials in chunk order.
template <class E, int D>
__device__ __forceinline__ void attn_merge(const float* __restrict__ part, typename E::T* __restrict__ o, int hq,
                                           int nchunks) {
  const int h = blockIdx.x, dd = threadIdx.x;
  float M = -INFINITY, L = 0.f, A = 0.f;
  for (int c = 0; c < nchunks; ++c) {
    const float* pr = part + ((long)c * hq + h) * (D + 2);
    const float m = pr[D], l = pr[D + 1], a = pr[dd];
    const float nM = fmaxf(M, m);
    const float f0 = exp2f((M - nM) * LOG2E), f1 = exp2f((m - nM) * LOG2E);
    A = A * f0 + a * f1;
    L = L * f0 + l * f1;
    M = nM;
  }
  o[(long)h * D + dd] = cvt1<E>(A / L);
}

template <class E, int D>
__global__ __launch_bounds__(D) void decode_attn_merge_kernel(const float* __restrict__ part,
                                                              typename E::T* __restrict__ o, int hq,
                                                              int nchunks) {
  attn_merge<E, D>(part, o, hq, nchunks);
}

// Grid (Hq, B): row b folds its own ceil(keys / DECODE_CHUNK) chunks of part [B, max_chunks, Hq, D + 2].
template <class E, int D>
__device__ __forceinline__ void attn_merge_row(const float* __restrict__ part, typename E::T* __restrict__ o,
                                               const int* __restrict__ pos0, int t, int max_keys, int max_chunks,
                                               int hq) {
  const int b = blockIdx.y;
  const int n_keys = max(row_keys(pos0, b, t, max_keys), 0);
  attn_merge<E, D>(part + (long)b * max_chunks * hq * (D + 2), o + (long)b * hq * D, hq,
                   (n_keys + DECODE_CHUNK - 1) / DECODE_CHUNK);
}

template <class E, int D>
__global__ __launch_bounds__(D) void decode_attn_merge_rows_kernel(const float* __restrict__ part,
                                                                   typename E::T* __restrict__ o,
                                                                   const int* __restrict__ pos0, int t,
                                                                   int max_keys, int max_chunks, int hq) {
  attn_merge_row<E, D>(part, o, pos0, t, max_keys, max_chunks, hq);
}

template <class E, int D>
__global__ __launch_bounds__(D) void decode_attn_merge_rows_dev_kernel(const float* __restrict__ part,
                                                                       typename E::T* __restrict__ o,
                                                                       const int* __restrict__ pos0,
                                                                       const int* __restrict__ ctl, int max_keys,
                                                                       int max_chunks, int hq) {
  attn_merge_row<E, D>(part, o, pos0, ctl[CTL_T], max_keys, max_chunks, hq);
}

// --------------------------------------------------------------------------------------------
// sample_. One 256-thread workgroup per row, rows grid-strided. The row is swept in vectors of 8
// columns, thread t taking vectors t, t + 256, ... (coalesced); "in ascending column order" is kept
// by a block scan per sweep of 2048 columns and a running prefix over the sweeps.
//
//   pass A      row maximum and its lowest column (greedy ends here)
//   passes B    top-k only: the k-th largest value by a 4 x 8-bit radix select over an
//               order-preserving integer image of the logits (NaN lowest, -0 = +0), and how many of
//               the columns equal to it are taken; then, if not all of them, the column of the last
//               one taken (ties go to the lower index)
//   passes P    top-p only (0 < top_p < 1): the nucleus, the shortest prefix of the candidates in
//               descending order (equal values by ascending column) whose weight reaches top_p * W,
//               W the candidates' total. Weights are monotone in the logit, so the nucleus has the
//               form of the top-k set, and a second 4 x 8-bit radix select over the same integer
//               image finds it, by mass instead of by count: per pass the candidates' weight per
//               bucket, the buckets walked from the top with the mass still needed carried along.
//               It ends at a value thr_p with `need` still to cover there; the cnt_eq candidates
//               equal to it weigh w_thr each, so the n = ceil(need / w_thr) lowest columns of them
//               are taken, found by the tie scan of passes B.
//               The masses are 64-bit fixed point, added with integer LDS atomics: a weight
//               w = expf(.) in [0, 1] becomes rint(w * 2^s), s = 62 - ceil(log2 V), so V weights
//               cannot overflow 2^62 and every sum is exact whatever the order of the adds. Each
//               weight is off by at most half a unit, 2^-(s+1), and all of them together by at most
//               V * 2^-(s+1): at V = 131072, s = 45 and that is 2^17 * 2^-46 = 1.9e-9 (twice that,
//               3.7e-9, had the weights been truncated), below 1e-8 * W since W >= 1: the row
//               maximum weighs 1. At smaller V the scale grows and the bound shrinks. W itself is the sum of the
//               first pass's buckets, so no sweep is spent on it and `need <= W` holds exactly: the
//               walk always ends in a bucket of positive mass.
//   pass C      total = sum of the candidates' weights exp((x - max) / temperature): fp32 weights,
//               summed in fp64 (its rounding is far below the weights' own)
//   pass D      the first candidate, in column order, whose cumulative weight reaches u * total
// --------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t okey(float f) {
  if (f != f) return 0u;
  f += 0.f;  // -0 -> +0
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Exclusive prefix of v over the 256 threads in thread order (`total`: the sum of all of them).
template <class T>
__device__ __forceinline__ T block_scan(T v, T* sh, T& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  T ex = __shfl_up(inc, 1, 64);
  if (lane == 0) ex = T(0);
  if (lane == 63) sh[wid] = inc;
  __syncthreads();
  T off = T(0);
  for (int i = 0; i < wid; ++i) off += sh[i];
  total = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  __syncthreads();
  return off + ex;
}

__device__ __forceinline__ int block_min(int v, int* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = min(min(sh[0], sh[1]), min(sh[2], sh[3]));
  __syncthreads();
  return v;
}

// The passes, on rows blockIdx.x, blockIdx.x + gridDim.x, ...: row r's token goes to out[r] and, where
// `col` is given, to col[r * col_stride] as well (sample_dev_: column t of the call's token table).
template <class E>
__device__ __forceinline__ void sample_rows(const typename E::T* __restrict__ logits, int64_t* __restrict__ out,
                                            int64_t* __restrict__ col, long col_stride, int V, int R,
                                            float temperature, int top_k, float top_p, uint32_t key_lo,
                                            uint32_t key_hi, uint32_t step) {
  __shared__ float sh_m[4];
  __shared__ int sh_i[4];
  __shared__ double sh_d[4];
  __shared__ int hist[256];
  __shared__ uint32_t s_prefix;
  __shared__ int s_kk, s_cnt, s_tie;
  __shared__ unsigned long long mass[256];
  __shared__ unsigned long long s_need;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const bool all_k = top_k <= 0 || top_k >= V;
  const bool nucleus = top_p > 0.f && top_p < 1.f;
  // the fixed-point scale of the passes P: 2^(62 - ceil(log2 V))
  const double fx_scale = (double)(1ull << (62 - (V > 1 ? 32 - __clz(V - 1) : 0)));
  for (int row = blockIdx.x; row < R; row += gridDim.x) {
    const typename E::T* lr = logits + (long)row * V;
    // ---- pass A: the maximum and the lowest column that attains it
    float m = -INFINITY;
    int mi = INT_MAX;
    for (int c = tid * 8; c < V; c += 2048) {
      float x[8];
      ld8<E>(lr + c, x);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (x[j] > m || (x[j] == m && c + j < mi)) {
          m = x[j];
          mi = c + j;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(m, o, 64);
      const int oi = __shfl_xor(mi, o, 64);
      if (om > m || (om == m && oi < mi)) {
        m = om;
        mi = oi;
      }
    }
    if (lane == 0) {
      sh_m[wid] = m;
      sh_i[wid] = mi;
    }
    __syncthreads();
    m = sh_m[0];
    mi = sh_i[0];
    for (int i = 1; i < 4; ++i)
      if (sh_m[i] > m || (sh_m[i] == m && sh_i[i] < mi)) {
        m = sh_m[i];
        mi = sh_i[i];
      }
    __syncthreads();
    if (mi == INT_MAX) mi = 0;  // a row without a single ordered value (all NaN)
    if (temperature == 0.f) {
      if (tid == 0) {
        out[row] = mi;
        if (col != nullptr) col[(long)row * col_stride] = mi;
      }
      continue;
    }
    // the column of the kk-th (1-based, in column order) of the columns whose key equals `eq_key`
    // (V where there are fewer than kk of them)
    auto nth_equal = [&](uint32_t eq_key, int kk) -> int {
      if (tid == 0) s_tie = V;
      __syncthreads();
      int run = 0;
      for (int c0 = 0; c0 < V; c0 += 2048) {
        const int c = c0 + tid * 8;
        uint32_t eq = 0u;
        if (c < V) {
          float x[8];
          ld8<E>(lr + c, x);
#pragma unroll
          for (int j = 0; j < 8; ++j) eq |= (okey(x[j]) == eq_key ? 1u : 0u) << j;
        }
        const int cnt = __popc(eq);
        int tot;
        const int before = run + block_scan<int>(cnt, sh_i, tot);
        if (before < kk && kk <= before + cnt) {
          int r = before;
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if ((eq >> j) & 1u) {
              if (++r == kk) s_tie = c + j;
            }
        }
        run += tot;
        __syncthreads();
        if (run >= kk) break;  // uniform: run is the same in every thread
      }
      return s_tie;
    };
    // ---- passes B: candidates are key > thr, or key == thr at a column <= tie_last
    bool all = all_k;
    uint32_t thr = 0u;
    int tie_last = V;
    if (!all) {
      uint32_t prefix = 0u;
      int kk = top_k, cnt_eq = 0;
      for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const uint32_t hi_mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
        hist[tid] = 0;
        __syncthreads();
        for (int c = tid * 8; c < V; c += 2048) {
          float x[8];
          ld8<E>(lr + c, x);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const uint32_t key = okey(x[j]);
            if ((key & hi_mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
          }
        }
        __syncthreads();
        if (tid == 0) {
          int cum = 0, b = 255;
          for (; b > 0; --b) {
            if (cum + hist[b] >= kk) break;
            cum += hist[b];
          }
          s_prefix = prefix | ((uint32_t)b << shift);
          s_kk = kk - cum;
          s_cnt = hist[b];
        }
        __syncthreads();
        prefix = s_prefix;
        kk = s_kk;
        cnt_eq = s_cnt;
      }
      thr = prefix;
      if (kk < cnt_eq) tie_last = nth_equal(thr, kk);  // only the kk lowest columns of those equal to it
    }
    // ---- passes P: the nucleus, as a new (thr, tie_last) inside the top-k candidates
    if (nucleus) {
      const uint32_t thr_k = thr;
      const int tie_k = tie_last;
      // the weight of a top-k candidate in fixed point, 0 for every other column
      auto weight_fx = [&](float x, uint32_t key, int col) -> unsigned long long {
        if (!(x == x)) return 0ull;
        if (!all_k && !(key > thr_k || (key == thr_k && col <= tie_k))) return 0ull;
        return (unsigned long long)__double2ll_rn((double)expf((x - m) / temperature) * fx_scale);
      };
      uint32_t prefix = 0u;
      unsigned long long need = 0ull, m_eq = 0ull;
      // a bf16 value has 16 low zero bits, so its key's low half is 0x0000 (value >= 0) or 0xffff
      // (value < 0, whose key is the complement): two passes find the high half, the sign gives the rest
      constexpr int PASSES = std::is_same<E, EBF16>::value ? 2 : 4;
      for (int pass = 0; pass < PASSES; ++pass) {
        const int shift = 24 - 8 * pass;
        const uint32_t hi_mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
        mass[tid] = 0ull;
        __syncthreads();
        {
          // runs of equal buckets are summed in registers first: one atomic per run
          int cur_b = 0;
          unsigned long long cur = 0ull;
          for (int c = tid * 8; c < V; c += 2048) {
            float x[8];
            ld8<E>(lr + c, x);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const uint32_t key = okey(x[j]);
              if ((key & hi_mask) != prefix) continue;
              const unsigned long long w = weight_fx(x[j], key, c + j);
              const int b = (int)((key >> shift) & 255u);
              if (b != cur_b) {
                if (cur != 0ull) atomicAdd(&mass[cur_b], cur);
                cur_b = b;
                cur = 0ull;
              }
              cur += w;
            }
          }
          if (cur != 0ull) atomicAdd(&mass[cur_b], cur);
        }
        __syncthreads();
        if (tid == 0) {
          unsigned long long nd = need;
          if (pass == 0) {  // W = the sum of every bucket; need = ceil(top_p * W) in [1, W]
            unsigned long long wsum = 0ull;
            for (int i = 0; i < 256; ++i) wsum += mass[i];
            nd = (unsigned long long)ceil((double)top_p * (double)wsum);  // top_p < 1, wsum <= 2^62
            nd = nd > wsum ? wsum : nd;
            nd = nd < 1ull ? 1ull : nd;  // wsum == 0 (no ordered weight at all) is caught below
          }
          unsigned long long cum = 0ull;
          int b = 255;
          for (; b > 0; --b) {
            if (cum + mass[b] >= nd) break;
            cum += mass[b];
          }
          s_prefix = prefix | ((uint32_t)b << shift);
          s_need = nd - cum;
          mass[0] = mass[b];  // the chosen bucket's mass, read back behind the barrier
        }
        __syncthreads();
        prefix = s_prefix;
        need = s_need;
        m_eq = mass[0];
        __syncthreads();
      }
      if (PASSES == 2 && !(prefix & 0x80000000u)) prefix |= 0xffffu;
      // every candidate equal to the threshold weighs w_thr; m_eq is their total
      const uint32_t ub = (prefix & 0x80000000u) ? (prefix ^ 0x80000000u) : ~prefix;
      const unsigned long long w_thr =
          (unsigned long long)__double2ll_rn((double)expf((__uint_as_float(ub) - m) / temperature) * fx_scale);
      // The walk ends in a bucket of positive mass with 1 <= need <= m_eq = cnt_eq * w_thr, so this
      // holds for every row with some weight; a row without any (W = 0: no ordered value, or an
      // infinite maximum, whose weights are NaN) has no nucleus to take and keeps the top-k candidates.
      if (w_thr > 0ull && m_eq >= w_thr && need >= 1ull && need <= m_eq) {
        const unsigned long long cnt_eq = m_eq / w_thr;
        unsigned long long n = (need + w_thr - 1ull) / w_thr;
        n = n < 1ull ? 1ull : (n > cnt_eq ? cnt_eq : n);
        const bool at_k = !all_k && prefix == thr_k;
        thr = prefix;
        tie_last = n < cnt_eq ? nth_equal(thr, (int)n) : (at_k ? tie_k : V);
        all = false;
      }
    }
    auto weight = [&](float x, int col) -> float {
      if (!(x == x)) return 0.f;
      if (!all) {
        const uint32_t key = okey(x);
        if (!(key > thr || (key == thr && col <= tie_last))) return 0.f;
      }
      return expf((x - m) / temperature);
    };
    // ---- pass C: the total weight
    double total = 0.0;
    for (int c0 = 0; c0 < V; c0 += 2048) {
      const int c = c0 + tid * 8;
      double loc = 0.0;
      if (c < V) {
        float x[8];
        ld8<E>(lr + c, x);
#pragma unroll
        for (int j = 0; j < 8; ++j) loc += (double)weight(x[j], c + j);
      }
      double tot;
      block_scan<double>(loc, sh_d, tot);
      total += tot;
    }
    const uint32_t w0 = sr_bits8(key_lo, key_hi, step, SR_BUF_SAMPLE, (uint64_t)row).x;
    const double target = ((double)w0 + 0.5) * (1.0 / 4294967296.0) * total;
    // ---- pass D: the first candidate whose cumulative weight reaches the target
    double run = 0.0;
    int found = INT_MAX, last = -1;
    for (int c0 = 0; c0 < V; c0 += 2048) {
      const int c = c0 + tid * 8;
      float wv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      double loc = 0.0;
      if (c < V) {
        float x[8];
        ld8<E>(lr + c, x);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          wv[j] = weight(x[j], c + j);
          loc += (double)wv[j];
          if (wv[j] > 0.f) last = c + j;
        }
      }
      double tot;
      const double ex = block_scan<double>(loc, sh_d, tot);
      if (run + tot >= target) {  // uniform
        int mine = INT_MAX;
        double cum = run + ex;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          cum += (double)wv[j];
          if (wv[j] > 0.f && cum >= target && mine == INT_MAX) mine = c + j;
        }
        found = block_min(mine, sh_i);
        if (found != INT_MAX) break;
      }
      run += tot;
    }
    if (found == INT_MAX) {  // rounding left the last cumulative sum a hair below the target
      last = -block_min(-last, sh_i);
      found = last >= 0 ? last : mi;
    }
    if (tid == 0) {
      out[row] = found;
      if (col != nullptr) col[(long)row * col_stride] = found;
    }
    __syncthreads();
  }
}

template <class E>
__global__ __launch_bounds__(256) void sample_kernel(const typename E::T* __restrict__ logits,
                                                     int64_t* __restrict__ out, int V, int R, float temperature,
                                                     int top_k, float top_p, uint32_t key_lo, uint32_t key_hi,
                                                     uint32_t step) {
  sample_rows<E>(logits, out, nullptr, 0, V, R, temperature, top_k, top_p, key_lo, key_hi, step);
}

// sample_dev_: the sampling arguments from the control block, and the per-token key
// token_key(key, t) = (key + (t + 1) * 0x9E3779B97F4A7C15) mod 2^63 formed here (generation.token_key).
// Tokens go to tok[R] and to column t of out [R, n_cap]; a t outside [0, n_cap) writes tok alone.
template <class E>
__global__ __launch_bounds__(256) void sample_dev_kernel(const typename E::T* __restrict__ logits,
                                                         const int* __restrict__ ctl, int64_t* __restrict__ tok,
                                                         int64_t* __restrict__ out, long n_cap, int V, int R) {
  const int t = ctl[CTL_T];
  const uint64_t key = (uint64_t)(uint32_t)ctl[CTL_KEY_LO] | ((uint64_t)(uint32_t)ctl[CTL_KEY_HI] << 32);
  const uint64_t tk = (key + ((uint64_t)(int64_t)t + 1ull) * 0x9E3779B97F4A7C15ull) & 0x7FFFFFFFFFFFFFFFull;
  const float temperature = __int_as_float(ctl[CTL_TEMPERATURE]);
  const int top_k = min(max(ctl[CTL_TOP_K], 0), V);
  const float top_p = __int_as_float(ctl[CTL_TOP_P]);  // word 0 is 0.f: off, as is anything not in (0, 1)
  int64_t* col = (t >= 0 && t < n_cap) ? out + t : nullptr;
  sample_rows<E>(logits, tok, col, n_cap, V, R, temperature, top_k, top_p, (uint32_t)tk, (uint32_t)(tk >> 32),
                 (uint32_t)ctl[CTL_STEP]);
}

// decode_ctl_advance_: t <- t + 1, one thread, a plain load and store. A launch of its own behind
// every kernel of the pass: each of their workgroups reads t, so none of them may write it.
__global__ void ctl_advance_kernel(int* __restrict__ ctl) {
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl[CTL_T] = ctl[CTL_T] + 1;
}

void check_vec(const char* op, const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, op, ": ", name, " must be 16-byte aligned");
}

template <bool SWIGLU>
at::Tensor gemv_impl(const char* op, const at::Tensor& x, const at::Tensor& w,
                     const c10::optional<at::Tensor>& residual) {
  FT_CHECK_MODEL_DTYPE(w);
  check_vec(op, x, "x");
  check_vec(op, w, "w");
  TORCH_CHECK(x.scalar_type() == w.scalar_type() && x.device() == w.device(), op, ": x / w dtype or device mismatch");
  TORCH_CHECK(w.dim() == 2 && x.dim() == 1 && x.size(0) == w.size(1), op, ": x [K], w [N, K]");
  const int64_t rows = w.size(0), K = w.size(1);
  const int vn = w.scalar_type() == at::kFloat ? 4 : 8;
  TORCH_CHECK(K > 0 && K % vn == 0, op, ": K must be a positive multiple of ", vn, " (16-byte row vectors)");
  TORCH_CHECK(rows > 0 && rows <= INT_MAX && K <= INT_MAX, op, ": N and K must fit 32 bits");
  TORCH_CHECK(!SWIGLU || rows % 2 == 0, op, ": w13 must be [2H, K]");
  const int64_t N = SWIGLU ? rows / 2 : rows;
  const bool has_res = residual.has_value() && residual->defined();
  if (has_res) {
    TORCH_CHECK(residual->is_cuda() && residual->is_contiguous() && residual->scalar_type() == w.scalar_type() &&
                    residual->device() == w.device() && residual->numel() == N,
                op, ": residual must be a contiguous [N] tensor of w's dtype and device");
  }
  const at::DeviceGuard guard(w.device());
  auto y = at::empty({N}, w.options());
  FT_DISPATCH_E(w.scalar_type(),
                hipLaunchKernelGGL((gemv_kernel<E, SWIGLU>), dim3((unsigned)((N + 3) / 4)), dim3(256), 0, ft_stream(),
                                   cptr<typename E::T>(x), cptr<typename E::T>(w),
                                   has_res ? cptr<typename E::T>(*residual) : nullptr, mptr<typename E::T>(y),
                                   (int)N, (int)K));
  FT_LAUNCH_CHECK();
  return y;
}

// The tile heights of gemv_rows_kernel. R <= 8 takes the smallest tile that holds it; above, tiles
// of GEMV_ROWS_TILE (SWIGLU: GEMV_SWIGLU_ROWS_TILE) rows.
constexpr int GEMV_ROWS_TILE = 8;
constexpr int GEMV_SWIGLU_ROWS_TILE = 8;

template <bool SWIGLU>
at::Tensor gemv_rows_impl(const char* op, const at::Tensor& x, const at::Tensor& w,
                          const c10::optional<at::Tensor>& residual) {
  FT_CHECK_MODEL_DTYPE(w);
  check_vec(op, x, "x");
  check_vec(op, w, "w");
  TORCH_CHECK(x.scalar_type() == w.scalar_type() && x.device() == w.device(), op, ": x / w dtype or device mismatch");
  TORCH_CHECK(w.dim() == 2 && x.dim() == 2 && x.size(1) == w.size(1), op, ": x [R, K], w [N, K]");
  const int64_t R = x.size(0), rows = w.size(0), K = w.size(1);
  const int vn = w.scalar_type() == at::kFloat ? 4 : 8;
  TORCH_CHECK(K > 0 && K % vn == 0, op, ": K must be a positive multiple of ", vn, " (16-byte row vectors)");
  TORCH_CHECK(R >= 1 && R <= INT_MAX, op, ": x needs at least one row");
  TORCH_CHECK(rows > 0 && rows <= INT_MAX && K <= INT_MAX, op, ": N and K must fit 32 bits");
  TORCH_CHECK(!SWIGLU || rows % 2 == 0, op, ": w13 must be [2H, K]");
  const int64_t N = SWIGLU ? rows / 2 : rows;
  const bool has_res = residual.has_value() && residual->defined();
  if (has_res) {
    TORCH_CHECK(residual->is_cuda() && residual->is_contiguous() && residual->scalar_type() == w.scalar_type() &&
                    residual->device() == w.device() && residual->dim() == 2 && residual->size(0) == R &&
                    residual->size(1) == N,
                op, ": residual must be a contiguous [R, N] tensor of w's dtype and device");
  }
  constexpr int TOP = SWIGLU ? GEMV_SWIGLU_ROWS_TILE : GEMV_ROWS_TILE;
  const int rt = R == 1 ? 1 : R == 2 ? 2 : (R <= 4 || TOP == 4) ? 4 : 8;
  const int64_t ntiles = (R + rt - 1) / rt;
  const int64_t blocks = (N + 3) / 4 * ntiles;
  TORCH_CHECK(blocks <= INT_MAX, op, ": too many workgroups (N / 4 x row tiles)");
  const at::DeviceGuard guard(w.device());
  auto y = at::empty({R, N}, w.options());
#define FT_GEMV_ROWS(RT)                                                                                       \
  hipLaunchKernelGGL((gemv_rows_kernel<E, SWIGLU, RT>), dim3((unsigned)blocks), dim3(256), 0, ft_stream(),     \
                     cptr<typename E::T>(x), cptr<typename E::T>(w),                                           \
                     has_res ? cptr<typename E::T>(*residual) : nullptr, mptr<typename E::T>(y), (int)N, (int)K, \
                     (int)R, (int)ntiles)
  FT_DISPATCH_E(w.scalar_type(), {
    if (rt == 1) FT_GEMV_ROWS(1);
    else if (rt == 2) FT_GEMV_ROWS(2);
    else if (rt == 4) FT_GEMV_ROWS(4);
    else FT_GEMV_ROWS(TOP);
  });
#undef FT_GEMV_ROWS
  FT_LAUNCH_CHECK();
  return y;
}

void check_cache(const char* op, const at::Tensor& c, const at::Tensor& like, int64_t hkv, int64_t d) {
  TORCH_CHECK(c.is_cuda() && c.device() == like.device() && c.scalar_type() == like.scalar_type(), op,
              ": the caches must be on qkv's device, in its dtype");
  TORCH_CHECK(c.is_contiguous() && c.dim() == 3 && c.size(0) == hkv && c.size(2) == d, op,
              ": a cache is a contiguous [Hkv, Smax, D] tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(c.data_ptr()) % 16 == 0, op, ": a cache must be 16-byte aligned");
}

template <class E, int D>
void launch_attn(const at::Tensor& q, const at::Tensor& kc, const at::Tensor& vc, const at::Tensor& part,
                 const at::Tensor& o, int hq, int hkv, int n_keys, int nchunks) {
  const int G = hq / hkv;
  const dim3 grid(hkv, nchunks);
  const float scale = 1.f / sqrtf((float)D);
  const long smax = kc.size(1);
#define FT_ATTN(GT)                                                                                        \
  hipLaunchKernelGGL((decode_attn_kernel<E, D, GT>), grid, dim3(256), 0, ft_stream(), cptr<typename E::T>(q), \
                     cptr<typename E::T>(kc), cptr<typename E::T>(vc), mptr<float>(part), hq, hkv, smax, n_keys, scale)
  if (G == 1) FT_ATTN(1);
  else if (G == 2) FT_ATTN(2);
  else if (G <= 4) FT_ATTN(4);
  else FT_ATTN(8);
#undef FT_ATTN
  FT_LAUNCH_CHECK();
  hipLaunchKernelGGL((decode_attn_merge_kernel<E, D>), dim3(hq), dim3(D), 0, ft_stream(), cptr<float>(part),
                     mptr<typename E::T>(o), hq, nchunks);
}

template <class E, int D>
void launch_attn_rows(const at::Tensor& q, const at::Tensor& kc, const at::Tensor& vc, const at::Tensor& part,
                      const at::Tensor& o, const at::Tensor& pos0, int t, int max_keys, int max_chunks, int B,
                      int hq, int hkv) {
  const int G = hq / hkv;
  const dim3 grid(hkv, max_chunks, B);
  const float scale = 1.f / sqrtf((float)D);
  const long smax = kc.size(2);
#define FT_ATTN(GT)                                                                                             \
  hipLaunchKernelGGL((decode_attn_rows_kernel<E, D, GT>), grid, dim3(256), 0, ft_stream(), cptr<typename E::T>(q), \
                     cptr<typename E::T>(kc), cptr<typename E::T>(vc), mptr<float>(part), cptr<int>(pos0), t,   \
                     max_keys, (long)q.stride(0), hq, hkv, smax, scale)
  if (G == 1) FT_ATTN(1);
  else if (G == 2) FT_ATTN(2);
  else if (G <= 4) FT_ATTN(4);
  else FT_ATTN(8);
#undef FT_ATTN
  FT_LAUNCH_CHECK();
  hipLaunchKernelGGL((decode_attn_merge_rows_kernel<E, D>), dim3(hq, B), dim3(D), 0, ft_stream(), cptr<float>(part),
                     mptr<typename E::T>(o), cptr<int>(pos0), t, max_keys, max_chunks, hq);
}

template <class E, int D>
void launch_attn_rows_dev(const at::Tensor& q, const at::Tensor& kc, const at::Tensor& vc, const at::Tensor& part,
                          const at::Tensor& o, const at::Tensor& pos0, const at::Tensor& ctl, int max_chunks, int B,
                          int hq, int hkv) {
  const int G = hq / hkv;
  const dim3 grid(hkv, max_chunks, B);
  const float scale = 1.f / sqrtf((float)D);
  const long smax = kc.size(2);
#define FT_ATTN(GT)                                                                                       \
  hipLaunchKernelGGL((decode_attn_rows_dev_kernel<E, D, GT>), grid, dim3(256), 0, ft_stream(),            \
                     cptr<typename E::T>(q), cptr<typename E::T>(kc), cptr<typename E::T>(vc), mptr<float>(part), \
                     cptr<int>(pos0), cptr<int>(ctl), (long)q.stride(0), hq, hkv, smax, scale)
  if (G == 1) FT_ATTN(1);
  else if (G == 2) FT_ATTN(2);
  else if (G <= 4) FT_ATTN(4);
  else FT_ATTN(8);
#undef FT_ATTN
  FT_LAUNCH_CHECK();
  hipLaunchKernelGGL((decode_attn_merge_rows_dev_kernel<E, D>), dim3(hq, B), dim3(D), 0, ft_stream(),
                     cptr<float>(part), mptr<typename E::T>(o), cptr<int>(pos0), cptr<int>(ctl), (int)smax, max_chunks,
                     hq);
}

// The operands the two batched cache ops share: caches [B, Hkv, Smax, D] of x's dtype, pos0 int32 [B].
void check_rows(const char* op, const at::Tensor& x, const at::Tensor& k_cache, const at::Tensor& v_cache,
                const at::Tensor& pos0) {
  FT_CHECK_MODEL_DTYPE(x);
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.size(0) >= 1, op, ": the activation is a GPU tensor [B, width], B >= 1");
  TORCH_CHECK(x.stride(1) == 1 && x.stride(0) >= x.size(1) && x.stride(0) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              op, ": the activation's rows must be dense, 16-byte aligned, a multiple of 8 elements apart");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(0) == x.size(0), op, ": a cache is [B, Hkv, Smax, D]");
  for (const at::Tensor* c : {&k_cache, &v_cache}) {
    TORCH_CHECK(c->is_cuda() && c->device() == x.device() && c->scalar_type() == x.scalar_type(), op,
                ": the caches must be on the activation's device, in its dtype");
    TORCH_CHECK(c->is_contiguous() && c->sizes() == k_cache.sizes(), op,
                ": the caches are contiguous [B, Hkv, Smax, D] tensors of one shape");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(c->data_ptr()) % 16 == 0, op, ": a cache must be 16-byte aligned");
  }
  TORCH_CHECK(pos0.is_cuda() && pos0.device() == x.device() && pos0.scalar_type() == at::kInt &&
                  pos0.is_contiguous() && pos0.dim() == 1 && pos0.size(0) == x.size(0),
              op, ": pos0 must be a contiguous int32 [B] tensor on the activation's device");
  TORCH_CHECK(x.size(0) <= 65535 && k_cache.size(2) <= INT_MAX, op, ": B or Smax too large");
}

void check_ctl(const char* op, const at::Tensor& ctl, const at::Tensor& like) {
  TORCH_CHECK(ctl.is_cuda() && ctl.device() == like.device() && ctl.scalar_type() == at::kInt && ctl.is_contiguous() &&
                  ctl.dim() == 1 && ctl.size(0) >= CTL_WORDS,
              op, ": ctl must be a contiguous int32 tensor of at least ", (int)CTL_WORDS, " words on the operands' device");
}

}  // namespace

// decode_qkv_append_rows_ with t read from ctl[CTL_T] on the device: row b goes to position
// pos0[b] + t. The host does not know t, so the only bound here is the capacity: a position outside
// the cache or the RoPE tables writes nothing (the caller checks its own count of steps).
void decode_qkv_append_rows_dev_(const at::Tensor& qkv, const at::Tensor& cos_t, const at::Tensor& sin_t,
                                 const at::Tensor& pos0, const at::Tensor& ctl, const at::Tensor& k_cache,
                                 const at::Tensor& v_cache) {
  const char* op = "decode_qkv_append_rows_dev_";
  check_rows(op, qkv, k_cache, v_cache, pos0);
  check_ctl(op, ctl, qkv);
  TORCH_CHECK(qkv.is_contiguous(), op, ": qkv must be contiguous");
  const int64_t B = qkv.size(0), hkv = k_cache.size(1), smax = k_cache.size(2), d = k_cache.size(3);
  TORCH_CHECK(d > 0 && d % 8 == 0, op, ": head_dim must be a multiple of 8");
  TORCH_CHECK(qkv.size(1) % d == 0 && qkv.size(1) / d > 2 * hkv, op, ": qkv width");
  const int64_t hq = qkv.size(1) / d - 2 * hkv;
  for (const at::Tensor* c : {&cos_t, &sin_t}) {
    TORCH_CHECK(c->is_cuda() && c->device() == qkv.device() && c->scalar_type() == at::kFloat && c->is_contiguous() &&
                    c->dim() == 2 && c->size(1) == d / 2 && c->size(0) == cos_t.size(0),
                op, ": cos / sin must be fp32 [S, D / 2] on qkv's device");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(c->data_ptr()) % 16 == 0, op, ": cos / sin alignment");
  }
  const at::DeviceGuard guard(qkv.device());
  const int nvec = (int)(qkv.size(1) / 8);
  FT_DISPATCH_E(qkv.scalar_type(),
                hipLaunchKernelGGL(qkv_append_rows_dev_kernel<E>, dim3((nvec + 255) / 256, (unsigned)B), dim3(256), 0,
                                   ft_stream(), mptr<typename E::T>(qkv), cptr<float>(cos_t), cptr<float>(sin_t),
                                   cptr<int>(pos0), cptr<int>(ctl), mptr<typename E::T>(k_cache),
                                   mptr<typename E::T>(v_cache), (int)hq, (int)hkv, (int)d, (long)smax,
                                   (long)std::min<int64_t>(smax, cos_t.size(0))));
  FT_LAUNCH_CHECK();
}

// decode_attn_rows with t read from ctl[CTL_T] on the device, into the caller's buffers: part fp32
// [B, ceil(Smax / DECODE_CHUNK), hq, d + 2] and o [B, hq d]. The grid covers the capacity, a row's
// merge folds the chunks its key count min(pos0[b] + t + 1, Smax) needs: the bits of decode_attn_rows.
void decode_attn_rows_dev(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                          const at::Tensor& pos0, const at::Tensor& ctl, const at::Tensor& part, const at::Tensor& o) {
  const char* op = "decode_attn_rows_dev";
  check_rows(op, q, k_cache, v_cache, pos0);
  check_ctl(op, ctl, q);
  const int64_t B = q.size(0), hkv = k_cache.size(1), smax = k_cache.size(2), d = k_cache.size(3);
  TORCH_CHECK(d == 64 || d == 128, op, ": head_dim must be 64 or 128");
  TORCH_CHECK(q.size(1) % d == 0, op, ": q width");
  const int64_t hq = q.size(1) / d;
  TORCH_CHECK(hq > 0 && hq % hkv == 0, op, ": Hq must be a multiple of Hkv");
  TORCH_CHECK(smax >= 1, op, ": empty cache");
  const int64_t max_chunks = (smax + DECODE_CHUNK - 1) / DECODE_CHUNK;
  TORCH_CHECK(max_chunks <= 65535, op, ": too many key chunks");
  TORCH_CHECK(part.is_cuda() && part.device() == q.device() && part.scalar_type() == at::kFloat &&
                  part.is_contiguous() && part.numel() == B * max_chunks * hq * (d + 2),
              op, ": part must be a contiguous fp32 [B, ceil(Smax / ", DECODE_CHUNK, "), Hq, D + 2] tensor");
  TORCH_CHECK(o.is_cuda() && o.device() == q.device() && o.scalar_type() == q.scalar_type() && o.is_contiguous() &&
                  o.dim() == 2 && o.size(0) == B && o.size(1) == hq * d,
              op, ": o must be a contiguous [B, Hq D] tensor of q's dtype");
  const at::DeviceGuard guard(q.device());
  FT_DISPATCH_E(q.scalar_type(), {
    if (d == 64)
      launch_attn_rows_dev<E, 64>(q, k_cache, v_cache, part, o, pos0, ctl, (int)max_chunks, (int)B, (int)hq, (int)hkv);
    else
      launch_attn_rows_dev<E, 128>(q, k_cache, v_cache, part, o, pos0, ctl, (int)max_chunks, (int)B, (int)hq,
                                   (int)hkv);
  });
  FT_LAUNCH_CHECK();
}

// sample_ with (temperature, top_k, top_p, key, step) and the token number t read from ctl on the device:
// row r draws what sample_(logits, ., temperature, top_k, token_key(key, t), step, top_p) draws for it, into
// tok[r] and out[r, t] (out int64 [R, n_cap]).
void sample_dev_(const at::Tensor& logits, const at::Tensor& ctl, const at::Tensor& tok, const at::Tensor& out) {
  const char* op = "sample_dev_";
  FT_CHECK_CUDA(logits);
  FT_CHECK_MODEL_DTYPE(logits);
  FT_CHECK_CONTIG(logits);
  check_ctl(op, ctl, logits);
  TORCH_CHECK(logits.dim() == 2 && logits.size(0) > 0 && logits.size(1) > 0, op, ": logits must be [R, V]");
  const int64_t R = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V % 8 == 0, op, ": vocab must be a multiple of 8");
  TORCH_CHECK(V <= INT_MAX && R <= INT_MAX, op, ": R and V must fit 32 bits");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0, op, ": logits must be 16-byte aligned");
  for (const at::Tensor* x : {&tok, &out})
    TORCH_CHECK(x->is_cuda() && x->device() == logits.device() && x->scalar_type() == at::kLong && x->is_contiguous(),
                op, ": tok and out must be contiguous int64 tensors on logits' device");
  TORCH_CHECK(tok.numel() == R, op, ": tok holds one token per row");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == R && out.size(1) >= 1, op, ": out must be [R, n_cap]");
  const at::DeviceGuard guard(logits.device());
  FT_DISPATCH_E(logits.scalar_type(),
                hipLaunchKernelGGL(sample_dev_kernel<E>, dim3((unsigned)std::min<int64_t>(R, SAMPLE_MAX_BLOCKS)),
                                   dim3(256), 0, ft_stream(), cptr<typename E::T>(logits), cptr<int>(ctl),
                                   mptr<int64_t>(tok), mptr<int64_t>(out), (long)out.size(1), (int)V, (int)R));
  FT_LAUNCH_CHECK();
}

// ctl[CTL_T] += 1 on the device, in stream order behind the pass that read it.
void decode_ctl_advance_(const at::Tensor& ctl) {
  check_ctl("decode_ctl_advance_", ctl, ctl);
  const at::DeviceGuard guard(ctl.device());
  hipLaunchKernelGGL(ctl_advance_kernel, dim3(1), dim3(64), 0, ft_stream(), mptr<int>(ctl));
  FT_LAUNCH_CHECK();
}

// y[R, N] = x[R, K] w[N, K]^T (+ residual[R, N]); row r has the bits of gemv(x[r], w, residual[r]).
at::Tensor gemv_rows(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& residual) {
  return gemv_rows_impl<false>("gemv_rows", x, w, residual);
}

// a[R, H]: row r has the bits of gemv_swiglu(x[r], w13).
at::Tensor gemv_swiglu_rows(const at::Tensor& x, const at::Tensor& w13) {
  return gemv_rows_impl<true>("gemv_swiglu_rows", x, w13, c10::nullopt);
}

// decode_qkv_append_ on row b of qkv [B, (hq + 2 hkv) d] at position pos0[b] + t of caches
// [B, hkv, Smax, d]. max_pos is the caller's largest pos0[b] + t: the op checks it against Smax and
// the RoPE tables and does not read pos0 back (a row beyond max_pos is left unwritten).
void decode_qkv_append_rows_(const at::Tensor& qkv, const at::Tensor& cos_t, const at::Tensor& sin_t,
                             const at::Tensor& pos0, int64_t t, int64_t max_pos, const at::Tensor& k_cache,
                             const at::Tensor& v_cache) {
  const char* op = "decode_qkv_append_rows_";
  check_rows(op, qkv, k_cache, v_cache, pos0);
  TORCH_CHECK(qkv.is_contiguous(), op, ": qkv must be contiguous");
  const int64_t B = qkv.size(0), hkv = k_cache.size(1), smax = k_cache.size(2), d = k_cache.size(3);
  TORCH_CHECK(d > 0 && d % 8 == 0, op, ": head_dim must be a multiple of 8");
  TORCH_CHECK(qkv.size(1) % d == 0 && qkv.size(1) / d > 2 * hkv, op, ": qkv width");
  const int64_t hq = qkv.size(1) / d - 2 * hkv;
  TORCH_CHECK(t >= 0 && t <= INT_MAX && max_pos >= t && max_pos < smax, op, ": largest position ", max_pos,
              " (t = ", t, ") outside the cache [0, ", smax, ")");
  for (const at::Tensor* c : {&cos_t, &sin_t}) {
    TORCH_CHECK(c->is_cuda() && c->device() == qkv.device() && c->scalar_type() == at::kFloat && c->is_contiguous() &&
                    c->dim() == 2 && c->size(1) == d / 2 && c->size(0) > max_pos,
                op, ": cos / sin must be fp32 [S > largest position, D / 2] on qkv's device");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(c->data_ptr()) % 16 == 0, op, ": cos / sin alignment");
  }
  const at::DeviceGuard guard(qkv.device());
  const int nvec = (int)(qkv.size(1) / 8);
  FT_DISPATCH_E(qkv.scalar_type(),
                hipLaunchKernelGGL(qkv_append_rows_kernel<E>, dim3((nvec + 255) / 256, (unsigned)B), dim3(256), 0,
                                   ft_stream(), mptr<typename E::T>(qkv), cptr<float>(cos_t), cptr<float>(sin_t),
                                   cptr<int>(pos0), (int)t, mptr<typename E::T>(k_cache),
                                   mptr<typename E::T>(v_cache), (int)hq, (int)hkv, (int)d, (long)smax,
                                   (long)(max_pos + 1)));
  FT_LAUNCH_CHECK();
}

// o[B, hq d]: q [B, hq d] may be a column slice of a wider buffer (rows stride(0) apart); row b is
// decode_attn of q[b] over keys 0 .. pos0[b] + t of its caches [B, hkv, Smax, d],
// bit for bit. max_keys is the caller's largest key count (pos0 is not read back).
at::Tensor decode_attn_rows(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                            const at::Tensor& pos0, int64_t t, int64_t max_keys) {
  const char* op = "decode_attn_rows";
  check_rows(op, q, k_cache, v_cache, pos0);
  const int64_t B = q.size(0), hkv = k_cache.size(1), smax = k_cache.size(2), d = k_cache.size(3);
  TORCH_CHECK(d == 64 || d == 128, op, ": head_dim must be 64 or 128");
  TORCH_CHECK(q.size(1) % d == 0, op, ": q width");
  const int64_t hq = q.size(1) / d;
  TORCH_CHECK(hq > 0 && hq % hkv == 0, op, ": Hq must be a multiple of Hkv");
  TORCH_CHECK(t >= 0 && t <= INT_MAX && max_keys > t && max_keys <= smax, op, ": max_keys ", max_keys, " (t = ", t,
              ") outside [t + 1, Smax = ", smax, "]");
  const at::DeviceGuard guard(q.device());
  const int max_chunks = (int)((max_keys + DECODE_CHUNK - 1) / DECODE_CHUNK);
  TORCH_CHECK(max_chunks <= 65535, op, ": too many key chunks");
  auto part = at::empty({B, max_chunks, hq, d + 2}, q.options().dtype(at::kFloat));
  auto o = at::empty({B, hq * d}, q.options());
  FT_DISPATCH_E(q.scalar_type(), {
    if (d == 64)
      launch_attn_rows<E, 64>(q, k_cache, v_cache, part, o, pos0, (int)t, (int)max_keys, max_chunks, (int)B, (int)hq,
                              (int)hkv);
    else
      launch_attn_rows<E, 128>(q, k_cache, v_cache, part, o, pos0, (int)t, (int)max_keys, max_chunks, (int)B, (int)hq,
                               (int)hkv);
  });
  FT_LAUNCH_CHECK();
  return o;
}

// y[N] = w[N, K] x[K] (+ residual[N]), fp32 accumulation, one rounding per output.
at::Tensor gemv(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& residual) {
  return gemv_impl<false>("gemv", x, w, residual);
}

// a[H] = silu(w1 x) * (w3 x) from the fused [w1; w3] view [2H, K].
at::Tensor gemv_swiglu(const at::Tensor& x, const at::Tensor& w13) {
  return gemv_impl<true>("gemv_swiglu", x, w13, c10::nullopt);
}

// qkv [(hq + 2 hkv) d] of the token at `pos`: Q rotated in place, K rotated into k_cache[:, pos],
// V copied into v_cache[:, pos]. Caches: [hkv, Smax, d].
void decode_qkv_append_(const at::Tensor& qkv, const at::Tensor& cos_t, const at::Tensor& sin_t, int64_t pos,
                        const at::Tensor& k_cache, const at::Tensor& v_cache) {
  FT_CHECK_MODEL_DTYPE(qkv);
  check_vec("decode_qkv_append_", qkv, "qkv");
  TORCH_CHECK(k_cache.dim() == 3, "decode_qkv_append_: a cache is [Hkv, Smax, D]");
  const int64_t hkv = k_cache.size(0), smax = k_cache.size(1), d = k_cache.size(2);
  check_cache("decode_qkv_append_", k_cache, qkv, hkv, d);
  check_cache("decode_qkv_append_", v_cache, qkv, hkv, d);
  TORCH_CHECK(v_cache.size(1) == smax, "decode_qkv_append_: k_cache / v_cache length mismatch");
  TORCH_CHECK(d > 0 && d % 8 == 0, "decode_qkv_append_: head_dim must be a multiple of 8");
  TORCH_CHECK(qkv.numel() % d == 0 && qkv.numel() / d > 2 * hkv, "decode_qkv_append_: qkv width");
  const int64_t hq = qkv.numel() / d - 2 * hkv;
  TORCH_CHECK(pos >= 0 && pos < smax, "decode_qkv_append_: pos ", pos, " outside the cache [0, ", smax, ")");
  for (const at::Tensor* t : {&cos_t, &sin_t}) {
    TORCH_CHECK(t->is_cuda() && t->device() == qkv.device() && t->scalar_type() == at::kFloat && t->is_contiguous() &&
                    t->dim() == 2 && t->size(1) == d / 2 && t->size(0) > pos,
                "decode_qkv_append_: cos / sin must be fp32 [S > pos, D / 2] on qkv's device");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "decode_qkv_append_: cos / sin alignment");
  }
  const at::DeviceGuard guard(qkv.device());
  const int nvec = (int)(qkv.numel() / 8);
  FT_DISPATCH_E(qkv.scalar_type(),
                hipLaunchKernelGGL(qkv_append_kernel<E>, dim3((nvec + 255) / 256), dim3(256), 0, ft_stream(),
                                   mptr<typename E::T>(qkv), cptr<float>(cos_t) + pos * (d / 2),
                                   cptr<float>(sin_t) + pos * (d / 2), mptr<typename E::T>(k_cache),
                                   mptr<typename E::T>(v_cache), (int)hq, (int)hkv, (int)d, (long)smax, (long)pos));
  FT_LAUNCH_CHECK();
}

// o[hq d] = softmax(q K^T / sqrt(d)) V over keys 0 .. n_keys-1 of the caches [hkv, Smax, d].
at::Tensor decode_attn(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache, int64_t n_keys) {
  FT_CHECK_MODEL_DTYPE(q);
  check_vec("decode_attn", q, "q");
  TORCH_CHECK(k_cache.dim() == 3, "decode_attn: a cache is [Hkv, Smax, D]");
  const int64_t hkv = k_cache.size(0), smax = k_cache.size(1), d = k_cache.size(2);
  check_cache("decode_attn", k_cache, q, hkv, d);
  check_cache("decode_attn", v_cache, q, hkv, d);
  TORCH_CHECK(v_cache.size(1) == smax, "decode_attn: k_cache / v_cache length mismatch");
  TORCH_CHECK(d == 64 || d == 128, "decode_attn: head_dim must be 64 or 128");
  TORCH_CHECK(q.numel() % d == 0, "decode_attn: q width");
  const int64_t hq = q.numel() / d;
  TORCH_CHECK(hq > 0 && hq % hkv == 0, "decode_attn: Hq must be a multiple of Hkv");
  TORCH_CHECK(n_keys >= 1 && n_keys <= smax && smax <= INT_MAX, "decode_attn: n_keys ", n_keys,
              " outside [1, Smax = ", smax, "]");
  const at::DeviceGuard guard(q.device());
  const int nchunks = (int)((n_keys + DECODE_CHUNK - 1) / DECODE_CHUNK);
  TORCH_CHECK(nchunks <= 65535, "decode_attn: too many key chunks");
  auto part = at::empty({nchunks, hq, d + 2}, q.options().dtype(at::kFloat));
  auto o = at::empty({hq * d}, q.options());
  FT_DISPATCH_E(q.scalar_type(), {
    if (d == 64) launch_attn<E, 64>(q, k_cache, v_cache, part, o, (int)hq, (int)hkv, (int)n_keys, nchunks);
    else launch_attn<E, 128>(q, k_cache, v_cache, part, o, (int)hq, (int)hkv, (int)n_keys, nchunks);
  });
  FT_LAUNCH_CHECK();
  return o;
}

// Keys per workgroup of decode_attn (the tests place n_keys around its multiples).
int64_t decode_attn_chunk() { return DECODE_CHUNK; }

// out[r] = one token drawn from row r of logits [R, V]; a pure function of
// (logits, temperature, top_k, top_p, key, step, r). temperature 0: the lowest column of the row maximum.
// top_p in (0, 1]; 1 (the default) runs no nucleus pass.
void sample_(const at::Tensor& logits, const at::Tensor& out, double temperature, int64_t top_k, int64_t key,
             int64_t step, double top_p) {
  FT_CHECK_CUDA(logits);
  FT_CHECK_MODEL_DTYPE(logits);
  FT_CHECK_CONTIG(logits);
  FT_CHECK_CUDA(out);
  FT_CHECK_CONTIG(out);
  TORCH_CHECK(out.scalar_type() == at::kLong && out.device() == logits.device(), "sample_: out must be int64 on logits' device");
  TORCH_CHECK(logits.dim() >= 1 && logits.size(-1) > 0, "sample_: logits must be [R, V]");
  const int64_t V = logits.size(-1);
  TORCH_CHECK(V % 8 == 0, "sample_: vocab must be a multiple of 8");
  const int64_t R = logits.numel() / V;
  TORCH_CHECK(V <= INT_MAX && R <= INT_MAX, "sample_: R and V must fit 32 bits");
  TORCH_CHECK(out.numel() == R, "sample_: out shape mismatch");
  TORCH_CHECK(temperature >= 0.0 && temperature < INFINITY, "sample_: temperature must be finite and >= 0");
  TORCH_CHECK(top_k >= 0, "sample_: top_k must be >= 0 (0: all columns)");
  TORCH_CHECK(top_p > 0.0 && top_p <= 1.0 && (float)top_p > 0.f, "sample_: top_p must be in (0, 1]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0, "sample_: logits must be 16-byte aligned");
  const at::DeviceGuard guard(logits.device());
  const uint64_t k64 = (uint64_t)key;
  if (R > 0)
    FT_DISPATCH_E(logits.scalar_type(),
                  hipLaunchKernelGGL(sample_kernel<E>, dim3((unsigned)std::min<int64_t>(R, SAMPLE_MAX_BLOCKS)), dim3(256),
                                     0, ft_stream(), cptr<typename E::T>(logits), mptr<int64_t>(out), (int)V, (int)R,
                                     (float)temperature, (int)std::min<int64_t>(top_k, V), (float)top_p,
                                     (uint32_t)k64, (uint32_t)(k64 >> 32), (uint32_t)(uint64_t)step));
  FT_LAUNCH_CHECK();
}

TORCH_LIBRARY_FRAGMENT(ftamd, m) {
  m.def("gemv(Tensor x, Tensor w, Tensor? residual) -> Tensor", &gemv);
  m.def("gemv_swiglu(Tensor x, Tensor w13) -> Tensor", &gemv_swiglu);
  m.def("decode_qkv_append_(Tensor(a!) qkv, Tensor cos, Tensor sin, int pos, Tensor(b!) k_cache, "
        "Tensor(c!) v_cache) -> ()",
        &decode_qkv_append_);
  m.def("decode_attn(Tensor q, Tensor k_cache, Tensor v_cache, int n_keys) -> Tensor", &decode_attn);
  m.def("decode_attn_chunk() -> int", &decode_attn_chunk);
  m.def("gemv_rows(Tensor x, Tensor w, Tensor? residual) -> Tensor", &gemv_rows);
  m.def("gemv_swiglu_rows(Tensor x, Tensor w13) -> Tensor", &gemv_swiglu_rows);
  m.def("decode_qkv_append_rows_(Tensor(a!) qkv, Tensor cos, Tensor sin, Tensor pos0, int t, int max_pos, "
        "Tensor(b!) k_cache, Tensor(c!) v_cache) -> ()",
        &decode_qkv_append_rows_);
  m.def("decode_attn_rows(Tensor q, Tensor k_cache, Tensor v_cache, Tensor pos0, int t, int max_keys) -> Tensor",
        &decode_attn_rows);
  m.def("sample_(Tensor logits, Tensor(a!) out, float temperature, int top_k, int key, int step, "
        "float top_p=1.0) -> ()",
        &sample_);
  m.def("decode_qkv_append_rows_dev_(Tensor(a!) qkv, Tensor cos, Tensor sin, Tensor pos0, Tensor ctl, "
        "Tensor(b!) k_cache, Tensor(c!) v_cache) -> ()",
        &decode_qkv_append_rows_dev_);
  m.def("decode_attn_rows_dev(Tensor q, Tensor k_cache, Tensor v_cache, Tensor pos0, Tensor ctl, Tensor(a!) part, "
        "Tensor(b!) o) -> ()",
        &decode_attn_rows_dev);
  m.def("sample_dev_(Tensor logits, Tensor ctl, Tensor(a!) tok, Tensor(b!) out) -> ()", &sample_dev_);
  m.def("decode_ctl_advance_(Tensor(a!) ctl) -> ()", &decode_ctl_advance_);
}
