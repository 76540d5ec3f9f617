// FP8 (e4m3) KV cache for decode: the cache ops of decode.hip on caches of e4m3 codes with one fp32
// scale per stored head row -- the D values of K (rotated) or V of one (sequence, kv head, position).
// The format is utils/fp8.py's, a "row" of its quantize_rows being one head row. A row is written
// once and never requantized. At long batched decodes the cache is the larger stream of a step
// (README, "FP8 KV cache"); codes and scales are (D + 4) / 2D of the model-dtype bytes.
//
//   decode_qkv_append_kv8_ (+ _rows_, _rows_dev_)  RoPE on Q in place; K rotated, rounded to the
//                          model dtype (what the model-dtype cache would hold) and quantized; V quantized
//   kv_quantize_prefill_   the rotated K and V of a prompt [P, Hkv D] into positions 0 .. P-1
//   decode_attn_kv8 (+ _rows, _rows_dev)           one query over keys 0 .. n-1 of such a cache
//
// Quantizing: a thread owns 8 columns, so a head row is D / 8 adjacent lanes of one wave. The row's
// amax is an xor butterfly over those lanes on the bit patterns of |x| (integer order = float order
// for non-negative floats, NaN and infinity on top), inv and the scale come from it by fp8.h's e4m3_row
// (the rule of decode_w8.hip's weight quantizer), each lane stores its 8 codes as one 8-byte store and
// the row's first lane the scale. No LDS, no barrier.
//
// Attention: the grid, the chunks of DECODE_CHUNK keys, the (acc, m, l) partials and the `part` layout
// are decode.hip's, so its merge kernels (decode_attn.h) fold the chunks. The chunk kernel is written
// for one-byte elements: a lane takes 16 codes (one 16-byte load), a key row is D / 16 lanes, and a
// pass of the 256 threads covers 256 / (D / 16) keys. Codes become fp32 in registers (exactly) and are
// never multiplied by a scale: the K scale enters once per (head, key) on the reduced dot product,
// s = (dp * k_scale[key]) * scale, the V scale once per (head, key) on the probability before the P V
// loop (l is the sum of the unscaled p). The chunk's 2 x 128 scales are loaded coalesced into LDS when
// the chunk starts. The query slice of a lane stays in registers over the chunk's keys. The P V
// partials of the 64 / (D / 16) key slots of a wave are folded by a halving exchange: at each step a
// lane keeps one half of its values and adds its partner's copy of them, so 16 values per head cost
// 8 + 4 + 2 (+ 1) shuffles instead of 16 per step, and every lane ends with 128 / 64 (or 1) of the
// D sums; the four waves are then added in wave order through LDS. Nothing is accumulated with
// atomics and every order is fixed: equal bits from run to run, and row b of a `_rows` op has the
// bits of the one-row op on that row. Keys, codes and scales at and beyond the key count are never
// loaded.
//
// The q K and P V products stay on the vector ALU in fp32: an FP8 MFMA would need the query (and the
// probabilities) quantized as well, which is another numerics contract.
#include "decode_host.h"  // the operand checks and dispatch macros; decode_attn.h
#include "fp8.h"

namespace {

// --------------------------------------------------------------------------------------------
// One head row of D values, 8 per lane over D / 8 adjacent lanes, to codes and a scale. Every lane of
// the row must be here (the butterfly reads its partners).
// --------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ void quantize_head_row(const float* x, uint8_t* __restrict__ codes8,
                                                  float* __restrict__ scale, bool first) {
  constexpr int LPR = D / 8;  // lanes per head row
  uint32_t m = 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j) m = max(m, __float_as_uint(x[j]) & 0x7fffffffu);
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
  const E4m3Row q = e4m3_row(m);
  uint2 c = make_uint2(0u, 0u);
  if (q.finite) {
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = __fmul_rn(x[j], q.inv);
    c = make_uint2(f32x4_to_fp8(f), f32x4_to_fp8(f + 4));
  }
  *reinterpret_cast<uint2*>(codes8) = c;
  if (first) *scale = q.scale;
}

// decode_qkv_append_kv8_: vector i (8 columns) of qkv [(Hq + 2 Hkv) D] of the token at `pos`. The
// rotation is decode.hip's qkv_append_vec's (rope8); K is then rounded to the model dtype, as the
// model-dtype cache stores it, before it is quantized.
template <class E, int D>
__device__ __forceinline__ void qkv_append_kv8_vec(int i, typename E::T* __restrict__ qkv,
                                                   const float* __restrict__ cos_row,
                                                   const float* __restrict__ sin_row, uint8_t* __restrict__ kc,
                                                   uint8_t* __restrict__ vc, float* __restrict__ ks,
                                                   float* __restrict__ vs, int hq, int hkv, long smax, long pos) {
  const int col = i * 8, head = col / D, within = col - head * D;
  float x[8];
  ld8<E>(qkv + col, x);
  if (head < hq + hkv) {
    float r[8];
    rope8(x, *reinterpret_cast<const float4*>(cos_row + (within >> 1)),
          *reinterpret_cast<const float4*>(sin_row + (within >> 1)), r);
    if (head < hq) {
      st8<E>(qkv + col, r);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = rnd<E>(r[j]);
      const long row = (long)(head - hq) * smax + pos;
      quantize_head_row<D>(r, kc + row * D + within, ks + row, within == 0);
    }
  } else {
    const long row = (long)(head - hq - hkv) * smax + pos;
    quantize_head_row<D>(x, vc + row * D + within, vs + row, within == 0);
  }
}

// Grid ceil(nvec / 256): the vector count is a multiple of D / 8, which divides 64, so the lanes of a
// head row are in one wave and leave or stay together.
template <class E, int D>
__global__ __launch_bounds__(256) void qkv_append_kv8_kernel(typename E::T* __restrict__ qkv,
                                                             const float* __restrict__ cos_row,
                                                             const float* __restrict__ sin_row,
                                                             uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                             float* __restrict__ ks, float* __restrict__ vs, int hq,
                                                             int hkv, long smax, long pos) {
  const int nvec = (hq + 2 * hkv) * D / 8;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  qkv_append_kv8_vec<E, D>(i, qkv, cos_row, sin_row, kc, vc, ks, vs, hq, hkv, smax, pos);
}

// Row b = blockIdx.y of qkv [B, (Hq + 2 Hkv) D] at position pos0[b] + t of caches [B, Hkv, Smax, D] /
// scales [B, Hkv, Smax]. A position outside [0, limit) writes nothing (uniform over the workgroup).
template <class E, int D>
__device__ __forceinline__ void qkv_append_kv8_row(typename E::T* __restrict__ qkv, const float* __restrict__ cos_t,
                                                   const float* __restrict__ sin_t, const int* __restrict__ pos0,
                                                   int t, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                   float* __restrict__ ks, float* __restrict__ vs, int hq, int hkv,
                                                   long smax, long limit) {
  const int nvec = (hq + 2 * hkv) * D / 8;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  const long pos = (long)pos0[b] + t;
  if (i >= nvec || pos < 0 || pos >= limit) return;
  const long sstride = (long)hkv * smax, cstride = sstride * D;
  qkv_append_kv8_vec<E, D>(i, qkv + (long)b * nvec * 8, cos_t + pos * (D / 2), sin_t + pos * (D / 2),
                           kc + b * cstride, vc + b * cstride, ks + b * sstride, vs + b * sstride, hq, hkv, smax,
                           pos);
}

template <class E, int D>
__global__ __launch_bounds__(256) void qkv_append_rows_kv8_kernel(
    typename E::T* __restrict__ qkv, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    const int* __restrict__ pos0, int t, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, float* __restrict__ ks,
    float* __restrict__ vs, int hq, int hkv, long smax, long limit) {
  qkv_append_kv8_row<E, D>(qkv, cos_t, sin_t, pos0, t, kc, vc, ks, vs, hq, hkv, smax, limit);
}

template <class E, int D>
__global__ __launch_bounds__(256) void qkv_append_rows_dev_kv8_kernel(
    typename E::T* __restrict__ qkv, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    const int* __restrict__ pos0, const int* __restrict__ ctl, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
    float* __restrict__ ks, float* __restrict__ vs, int hq, int hkv, long smax, long limit) {
  qkv_append_kv8_row<E, D>(qkv, cos_t, sin_t, pos0, ctl[CTL_T], kc, vc, ks, vs, hq, hkv, smax, limit);
}

// kv_quantize_prefill_: src [P, Hkv D], rows `stride` elements apart (the K and V columns of a qkv
// buffer, in place; blockIdx.y 0: the rotated K, 1: V), into positions 0 .. P-1 of
// codes [Hkv, Smax, D] / scale [Hkv, Smax]. Vector i is 8 columns of head row (p, h) = i / (D / 8): a
// wave takes 64 / (D / 8) head rows at a time.
template <class E, int D>
__global__ __launch_bounds__(256) void kv_quantize_prefill_kernel(
    const typename E::T* __restrict__ k, const typename E::T* __restrict__ v, uint8_t* __restrict__ kc,
    uint8_t* __restrict__ vc, float* __restrict__ ks, float* __restrict__ vs, long nvec, int hkv, long smax,
    long k_stride, long v_stride) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;  // nvec is a multiple of D / 8: a head row's lanes leave together
  const bool is_v = blockIdx.y != 0;
  const long hrow = i / (D / 8);
  const int within = (int)(i - hrow * (D / 8)) * 8;
  const long p = hrow / hkv, h = hrow - p * hkv;
  float x[8];
  ld8<E>((is_v ? v + p * v_stride : k + p * k_stride) + h * D + within, x);
  const long row = h * smax + p;
  quantize_head_row<D>(x, (is_v ? vc : kc) + row * D + within, (is_v ? vs : ks) + row, within == 0);
}

// --------------------------------------------------------------------------------------------
// Attention. Workgroup (kv head, chunk), 256 threads; sub = the lane's 16 columns of a key row,
// kslot = the key of a pass it takes.
// --------------------------------------------------------------------------------------------
// One step of the halving exchange over the key slots: of its N values a lane keeps the lower half
// (bit O of its lane index clear) or the upper half (set) and adds its partner's copy of that half;
// the kept half ends in v[0 .. N/2).
template <int N, int O>
__device__ __forceinline__ void halve(float* v, int lane) {
  const bool up = (lane & O) != 0;
#pragma unroll
  for (int j = 0; j < N / 2; ++j) {
    const float lo = v[j], hi = v[j + N / 2];
    const float got = __shfl_xor(up ? lo : hi, O, 64);
    v[j] = (up ? hi : lo) + got;
  }
}

template <class E, int D, int GT>
__device__ __forceinline__ void attn_chunk_kv8(const typename E::T* __restrict__ q, const uint8_t* __restrict__ kc,
                                               const uint8_t* __restrict__ vc, const float* __restrict__ ks,
                                               const float* __restrict__ vs, float* __restrict__ part, int hq,
                                               int hkv, long smax, int n_keys, float scale) {
  constexpr int LPK = D / 16;      // lanes per key row
  constexpr int KPP = 256 / LPK;   // keys per pass
  constexpr int FIN = 16 * LPK / 64;  // sums a lane holds after the exchange: 2 (D = 128) or 1 (D = 64)
  __shared__ float sks[DECODE_CHUNK], svs[DECODE_CHUNK];
  __shared__ float sp[GT][DECODE_CHUNK];
  __shared__ float sred[4][GT][D];
  __shared__ float s_m[GT], s_l[GT];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int sub = tid % LPK, kslot = tid / LPK;
  const int kvh = blockIdx.x, chunk = blockIdx.y;
  const int G = hq / hkv;
  const int k0 = chunk * DECODE_CHUNK;
  const int nk = min(DECODE_CHUNK, n_keys - k0);  // >= 1: the grid covers ceil(n_keys / chunk) chunks
  const long row0 = (long)kvh * smax + k0;
  const uint8_t* kbase = kc + row0 * D;
  const uint8_t* vbase = vc + row0 * D;
  // the chunk's scales: threads 0 .. 127 the K scales, 128 .. 255 the V scales, live keys only
  {
    const int kk = tid & (DECODE_CHUNK - 1);
    if (kk < nk) {
      if (tid < DECODE_CHUNK) sks[kk] = ks[row0 + kk];
      else svs[kk] = vs[row0 + kk];
    }
  }
  __syncthreads();
  // where the lane's FIN sums land after the exchange: bit LPK << s of the lane picks a half at step s
  int fin = 0;
#pragma unroll
  for (int o = LPK, n = 8; o < 64; o <<= 1, n >>= 1) fin += (lane & o) ? n : 0;
  for (int g0 = 0; g0 < G; g0 += GT) {
    // the lane's 16 columns of the tile's queries (zero beyond the group)
    float qr[GT][16];
#pragma unroll
    for (int g = 0; g < GT; ++g) {
      if (g0 + g < G) {
        const typename E::T* qp = q + ((long)kvh * G + g0 + g) * D + sub * 16;
        unpack8e<E>(*reinterpret_cast<const uint4*>(qp), qr[g]);
        unpack8e<E>(*reinterpret_cast<const uint4*>(qp + 8), qr[g] + 8);
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) qr[g][j] = 0.f;
      }
    }
    // scores of the chunk: sp[g][key] = scale * k_scale[key] * <q_g, codes_key>, -inf beyond the live keys
    for (int kk = kslot; kk < DECODE_CHUNK; kk += KPP) {
      const bool live = kk < nk;
      float kx[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) kx[j] = 0.f;
      if (live) fp8x16_to_f32(*reinterpret_cast<const uint4*>(kbase + (long)kk * D + sub * 16), kx);
#pragma unroll
      for (int g = 0; g < GT; ++g) {
        float dp = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) dp = fmaf(kx[j], qr[g][j], dp);
#pragma unroll
        for (int o = LPK / 2; o > 0; o >>= 1) dp += __shfl_xor(dp, o, 64);
        if (sub == 0) sp[g][kk] = live ? (dp * sks[kk]) * scale : -INFINITY;
      }
    }
    __syncthreads();
    // per head: chunk maximum, p = exp(s - m), l = sum p; sp becomes p * v_scale (one wave per head)
    for (int g = wid; g < GT; g += 4) {
      float m = -INFINITY;
#pragma unroll
      for (int i = 0; i < DECODE_CHUNK / 64; ++i) m = fmaxf(m, sp[g][lane + 64 * i]);
      m = wave_max(m);
      float l = 0.f;
#pragma unroll
      for (int i = 0; i < DECODE_CHUNK / 64; ++i) {
        const int kk = lane + 64 * i;
        const float p = exp2f((sp[g][kk] - m) * LOG2E);
        sp[g][kk] = kk < nk ? p * svs[kk] : 0.f;
        l += p;
      }
      l = wave_sum(l);
      if (lane == 0) {
        s_m[g] = m;
        s_l[g] = l;
      }
    }
    __syncthreads();
    // acc[g][16 dims of this lane] over the lane's keys, then over the key slots
    float acc[GT][16];
#pragma unroll
    for (int g = 0; g < GT; ++g)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[g][j] = 0.f;
    for (int kk = kslot; kk < nk; kk += KPP) {
      float vx[16];
      fp8x16_to_f32(*reinterpret_cast<const uint4*>(vbase + (long)kk * D + sub * 16), vx);
#pragma unroll
      for (int g = 0; g < GT; ++g) {
        const float p = sp[g][kk];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[g][j] = fmaf(p, vx[j], acc[g][j]);
      }
    }
#pragma unroll
    for (int g = 0; g < GT; ++g) {
      halve<16, LPK>(acc[g], lane);
      halve<8, 2 * LPK>(acc[g], lane);
      halve<4, 4 * LPK>(acc[g], lane);
      if constexpr (LPK == 4) halve<2, 8 * LPK>(acc[g], lane);
#pragma unroll
      for (int j = 0; j < FIN; ++j) sred[wid][g][sub * 16 + fin + j] = acc[g][j];
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
__global__ __launch_bounds__(256) void decode_attn_kv8_kernel(const typename E::T* __restrict__ q,
                                                              const uint8_t* __restrict__ kc,
                                                              const uint8_t* __restrict__ vc,
                                                              const float* __restrict__ ks,
                                                              const float* __restrict__ vs, float* __restrict__ part,
                                                              int hq, int hkv, long smax, int n_keys, float scale) {
  attn_chunk_kv8<E, D, GT>(q, kc, vc, ks, vs, part, hq, hkv, smax, n_keys, scale);
}

// Grid (Hkv, max_chunks, B), as decode.hip's attn_rows_chunk: a workgroup whose chunk starts at or
// beyond its row's key count leaves, all of it, before the first barrier.
template <class E, int D, int GT>
__device__ __forceinline__ void attn_rows_chunk_kv8(const typename E::T* __restrict__ q,
                                                    const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
                                                    const float* __restrict__ ks, const float* __restrict__ vs,
                                                    float* __restrict__ part, const int* __restrict__ pos0, int t,
                                                    int max_keys, long q_stride, int hq, int hkv, long smax,
                                                    float scale) {
  const int b = blockIdx.z;
  const int n_keys = row_keys(pos0, b, t, max_keys);
  if ((int)blockIdx.y * DECODE_CHUNK >= n_keys) return;  // uniform over the workgroup
  const long sstride = (long)hkv * smax, cstride = sstride * D;
  attn_chunk_kv8<E, D, GT>(q + b * q_stride, kc + b * cstride, vc + b * cstride, ks + b * sstride, vs + b * sstride,
                           part + (long)b * gridDim.y * hq * (D + 2), hq, hkv, smax, n_keys, scale);
}

template <class E, int D, int GT>
__global__ __launch_bounds__(256) void decode_attn_rows_kv8_kernel(
    const typename E::T* __restrict__ q, const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
    const float* __restrict__ ks, const float* __restrict__ vs, float* __restrict__ part,
    const int* __restrict__ pos0, int t, int max_keys, long q_stride, int hq, int hkv, long smax, float scale) {
  attn_rows_chunk_kv8<E, D, GT>(q, kc, vc, ks, vs, part, pos0, t, max_keys, q_stride, hq, hkv, smax, scale);
}

template <class E, int D, int GT>
__global__ __launch_bounds__(256) void decode_attn_rows_dev_kv8_kernel(
    const typename E::T* __restrict__ q, const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
    const float* __restrict__ ks, const float* __restrict__ vs, float* __restrict__ part,
    const int* __restrict__ pos0, const int* __restrict__ ctl, long q_stride, int hq, int hkv, long smax,
    float scale) {
  attn_rows_chunk_kv8<E, D, GT>(q, kc, vc, ks, vs, part, pos0, ctl[CTL_T], (int)smax, q_stride, hq, hkv, smax,
                                scale);
}

// --------------------------------------------------------------------------------------------
// Host side
// --------------------------------------------------------------------------------------------
// check_kv of decode_host.h for a cache of codes uint8 [lead.., Hkv, Smax, D], with what the FP8 cache
// adds: a 16-bit activation, the scales fp32 [lead.., Hkv, Smax], and head_dim 64 or 128 for every op.
KvShape check_kv8(const char* op, const at::Tensor& x, const at::Tensor& kc, const at::Tensor& vc,
                  const at::Tensor& ks, const at::Tensor& vs, bool rows) {
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf, op,
              ": the activation must be a bf16 or fp16 GPU tensor");
  const KvShape r = check_kv(op, x, kc, vc, at::kByte, rows);
  for (const at::Tensor* s : {&ks, &vs}) {
    TORCH_CHECK(s->is_cuda() && s->device() == x.device() && s->scalar_type() == at::kFloat && s->is_contiguous() &&
                    s->sizes() == kc.sizes().slice(0, kc.dim() - 1),
                op, ": the scales are contiguous fp32 tensors of the caches' shape without D, on their device");
  }
  TORCH_CHECK(r.d == 64 || r.d == 128, op, ": head_dim must be 64 or 128");
  return r;
}

void append_kv8(const at::Tensor& qkv, const at::Tensor& cos_t, const at::Tensor& sin_t, int64_t pos,
                const at::Tensor& kc, const at::Tensor& vc, const at::Tensor& ks, const at::Tensor& vs) {
  const char* op = "decode_qkv_append_kv8_";
  const KvShape s = check_kv8(op, qkv, kc, vc, ks, vs, false);
  const int64_t hq = qkv_heads(op, qkv.numel(), s);
  TORCH_CHECK(pos >= 0 && pos < s.smax, op, ": pos ", pos, " outside the cache [0, ", s.smax, ")");
  check_rope(op, cos_t, sin_t, qkv, s.d, pos + 1);
  const at::DeviceGuard guard(qkv.device());
  const int nvec = (int)(qkv.numel() / 8);
  FT_DISPATCH_E16(qkv.scalar_type(), FT_DECODE_D(s.d, {
    hipLaunchKernelGGL((qkv_append_kv8_kernel<E, D>), dim3((nvec + 255) / 256), dim3(256), 0, ft_stream(),
                       mptr<typename E::T>(qkv), cptr<float>(cos_t) + pos * (D / 2),
                       cptr<float>(sin_t) + pos * (D / 2), mptr<uint8_t>(kc), mptr<uint8_t>(vc), mptr<float>(ks),
                       mptr<float>(vs), (int)hq, (int)s.hkv, (long)s.smax, (long)pos);
  }));
  FT_LAUNCH_CHECK();
}

// t from the host (ctl undefined; the positions are checked up to max_pos) or from ctl[CTL_T] (the
// bound is the capacity of the cache and the RoPE tables).
void append_rows_kv8(const char* op, const at::Tensor& qkv, const at::Tensor& cos_t, const at::Tensor& sin_t,
                     const at::Tensor& pos0, const at::Tensor* ctl, int64_t t, int64_t max_pos, const at::Tensor& kc,
                     const at::Tensor& vc, const at::Tensor& ks, const at::Tensor& vs) {
  const KvShape s = check_kv8(op, qkv, kc, vc, ks, vs, true);
  check_pos0(op, pos0, qkv);
  TORCH_CHECK(qkv.is_contiguous(), op, ": qkv must be contiguous");
  const int64_t B = qkv.size(0), hq = qkv_heads(op, qkv.size(1), s);
  const long limit = check_append_rows(op, qkv, cos_t, sin_t, ctl, t, max_pos, s);
  const at::DeviceGuard guard(qkv.device());
  const int nvec = (int)(qkv.size(1) / 8);
  const dim3 grid((nvec + 255) / 256, (unsigned)B);
  FT_DISPATCH_E16(qkv.scalar_type(), FT_DECODE_D(s.d, {
    if (ctl != nullptr)
      hipLaunchKernelGGL((qkv_append_rows_dev_kv8_kernel<E, D>), grid, dim3(256), 0, ft_stream(),
                         mptr<typename E::T>(qkv), cptr<float>(cos_t), cptr<float>(sin_t), cptr<int>(pos0),
                         cptr<int>(*ctl), mptr<uint8_t>(kc), mptr<uint8_t>(vc), mptr<float>(ks), mptr<float>(vs),
                         (int)hq, (int)s.hkv, (long)s.smax, limit);
    else
      hipLaunchKernelGGL((qkv_append_rows_kv8_kernel<E, D>), grid, dim3(256), 0, ft_stream(),
                         mptr<typename E::T>(qkv), cptr<float>(cos_t), cptr<float>(sin_t), cptr<int>(pos0), (int)t,
                         mptr<uint8_t>(kc), mptr<uint8_t>(vc), mptr<float>(ks), mptr<float>(vs), (int)hq, (int)s.hkv,
                         (long)s.smax, limit);
  }));
  FT_LAUNCH_CHECK();
}

void append_rows_kv8_host(const at::Tensor& qkv, const at::Tensor& cos_t, const at::Tensor& sin_t,
                          const at::Tensor& pos0, int64_t t, int64_t max_pos, const at::Tensor& kc,
                          const at::Tensor& vc, const at::Tensor& ks, const at::Tensor& vs) {
  append_rows_kv8("decode_qkv_append_rows_kv8_", qkv, cos_t, sin_t, pos0, nullptr, t, max_pos, kc, vc, ks, vs);
}

void append_rows_kv8_dev(const at::Tensor& qkv, const at::Tensor& cos_t, const at::Tensor& sin_t,
                         const at::Tensor& pos0, const at::Tensor& ctl, const at::Tensor& kc, const at::Tensor& vc,
                         const at::Tensor& ks, const at::Tensor& vs) {
  append_rows_kv8("decode_qkv_append_rows_dev_kv8_", qkv, cos_t, sin_t, pos0, &ctl, 0, 0, kc, vc, ks, vs);
}

void kv_quantize_prefill(const at::Tensor& k, const at::Tensor& v, const at::Tensor& kc, const at::Tensor& vc,
                         const at::Tensor& ks, const at::Tensor& vs) {
  const char* op = "kv_quantize_prefill_";
  TORCH_CHECK(k.dim() == 2 && v.sizes() == k.sizes() && v.scalar_type() == k.scalar_type() && k.is_cuda() &&
                  v.is_cuda() && v.device() == k.device(),
              op, ": k and v are [P, Hkv D] GPU tensors of one dtype and device");
  for (const at::Tensor* x : {&k, &v})
    TORCH_CHECK(x->stride(1) == 1 && x->stride(0) >= x->size(1) && x->stride(0) % 8 == 0 &&
                    reinterpret_cast<uintptr_t>(x->data_ptr()) % 16 == 0,
                op, ": the rows of k and v must be dense, 16-byte aligned, a multiple of 8 elements apart");
  const KvShape s = check_kv8(op, k.select(0, 0), kc, vc, ks, vs, false);
  const int64_t P = k.size(0);
  TORCH_CHECK(P >= 1 && P <= s.smax && k.size(1) == s.hkv * s.d, op, ": k is [P <= Smax, Hkv D]");
  const at::DeviceGuard guard(k.device());
  const long nvec = (long)(k.numel() / 8);
  TORCH_CHECK((nvec + 255) / 256 <= INT_MAX, op, ": too many workgroups");
  FT_DISPATCH_E16(k.scalar_type(), FT_DECODE_D(s.d, {
    hipLaunchKernelGGL((kv_quantize_prefill_kernel<E, D>), dim3((unsigned)((nvec + 255) / 256), 2), dim3(256), 0,
                       ft_stream(), cptr<typename E::T>(k), cptr<typename E::T>(v), mptr<uint8_t>(kc),
                       mptr<uint8_t>(vc), mptr<float>(ks), mptr<float>(vs), nvec, (int)s.hkv, (long)s.smax, (long)k.stride(0),
                       (long)v.stride(0));
  }));
  FT_LAUNCH_CHECK();
}

at::Tensor attn_kv8(const at::Tensor& q, const at::Tensor& kc, const at::Tensor& vc, const at::Tensor& ks,
                    const at::Tensor& vs, int64_t n_keys) {
  const char* op = "decode_attn_kv8";
  const KvShape s = check_kv8(op, q, kc, vc, ks, vs, false);
  const int64_t hq = q_heads(op, q.numel(), s);
  TORCH_CHECK(n_keys >= 1 && n_keys <= s.smax, op, ": n_keys ", n_keys, " outside [1, Smax = ", s.smax, "]");
  const at::DeviceGuard guard(q.device());
  const int nchunks = (int)((n_keys + DECODE_CHUNK - 1) / DECODE_CHUNK);
  TORCH_CHECK(nchunks <= 65535, op, ": too many key chunks");
  auto part = at::empty({nchunks, hq, s.d + 2}, q.options().dtype(at::kFloat));
  auto o = at::empty({hq * s.d}, q.options());
  const int G = (int)(hq / s.hkv);
  FT_DISPATCH_E16(q.scalar_type(), FT_DECODE_D(s.d, {
    const float scale = 1.f / sqrtf((float)D);
    FT_DECODE_GT(G, hipLaunchKernelGGL((decode_attn_kv8_kernel<E, D, GT>), dim3((unsigned)s.hkv, nchunks), dim3(256), 0,
                                    ft_stream(), cptr<typename E::T>(q), cptr<uint8_t>(kc), cptr<uint8_t>(vc),
                                    cptr<float>(ks), cptr<float>(vs), mptr<float>(part), (int)hq, (int)s.hkv,
                                    (long)s.smax, (int)n_keys, scale));
    FT_LAUNCH_CHECK();
    hipLaunchKernelGGL((decode_attn_merge_kernel<E, D>), dim3((unsigned)hq), dim3(D), 0, ft_stream(),
                       cptr<float>(part), mptr<typename E::T>(o), (int)hq, nchunks);
  }));
  FT_LAUNCH_CHECK();
  return o;
}

// The rows forms into the caller's part [B, max_chunks, Hq, D + 2] and o [B, Hq D]; t from the host
// (ctl == nullptr, the grid over max_keys) or from ctl[CTL_T] (the grid over the capacity).
void attn_rows_kv8_into(const char* op, const at::Tensor& q, const at::Tensor& kc, const at::Tensor& vc,
                        const at::Tensor& ks, const at::Tensor& vs, const at::Tensor& pos0, const at::Tensor* ctl,
                        int t, int max_keys, int max_chunks, const KvShape& s, int64_t hq, const at::Tensor& part,
                        const at::Tensor& o) {
  const int B = (int)q.size(0), G = (int)(hq / s.hkv);
  const dim3 grid((unsigned)s.hkv, max_chunks, B);
  FT_DISPATCH_E16(q.scalar_type(), FT_DECODE_D(s.d, {
    const float scale = 1.f / sqrtf((float)D);
    if (ctl != nullptr) {
      FT_DECODE_GT(G, hipLaunchKernelGGL((decode_attn_rows_dev_kv8_kernel<E, D, GT>), grid, dim3(256), 0, ft_stream(),
                                      cptr<typename E::T>(q), cptr<uint8_t>(kc), cptr<uint8_t>(vc), cptr<float>(ks),
                                      cptr<float>(vs), mptr<float>(part), cptr<int>(pos0), cptr<int>(*ctl),
                                      (long)q.stride(0), (int)hq, (int)s.hkv, (long)s.smax, scale));
      FT_LAUNCH_CHECK();
      hipLaunchKernelGGL((decode_attn_merge_rows_dev_kernel<E, D>), dim3((unsigned)hq, B), dim3(D), 0, ft_stream(),
                         cptr<float>(part), mptr<typename E::T>(o), cptr<int>(pos0), cptr<int>(*ctl), (int)s.smax,
                         max_chunks, (int)hq);
    } else {
      FT_DECODE_GT(G, hipLaunchKernelGGL((decode_attn_rows_kv8_kernel<E, D, GT>), grid, dim3(256), 0, ft_stream(),
                                      cptr<typename E::T>(q), cptr<uint8_t>(kc), cptr<uint8_t>(vc), cptr<float>(ks),
                                      cptr<float>(vs), mptr<float>(part), cptr<int>(pos0), t, max_keys,
                                      (long)q.stride(0), (int)hq, (int)s.hkv, (long)s.smax, scale));
      FT_LAUNCH_CHECK();
      hipLaunchKernelGGL((decode_attn_merge_rows_kernel<E, D>), dim3((unsigned)hq, B), dim3(D), 0, ft_stream(),
                         cptr<float>(part), mptr<typename E::T>(o), cptr<int>(pos0), t, max_keys, max_chunks,
                         (int)hq);
    }
  }));
  FT_LAUNCH_CHECK();
}

at::Tensor attn_rows_kv8(const at::Tensor& q, const at::Tensor& kc, const at::Tensor& vc, const at::Tensor& ks,
                         const at::Tensor& vs, const at::Tensor& pos0, int64_t t, int64_t max_keys) {
  const char* op = "decode_attn_rows_kv8";
  const KvShape s = check_kv8(op, q, kc, vc, ks, vs, true);
  check_pos0(op, pos0, q);
  const int64_t hq = q_heads(op, q.size(1), s);
  TORCH_CHECK(t >= 0 && t <= INT_MAX && max_keys > t && max_keys <= s.smax, op, ": max_keys ", max_keys, " (t = ", t,
              ") outside [t + 1, Smax = ", s.smax, "]");
  const at::DeviceGuard guard(q.device());
  const int max_chunks = (int)((max_keys + DECODE_CHUNK - 1) / DECODE_CHUNK);
  TORCH_CHECK(max_chunks <= 65535, op, ": too many key chunks");
  auto part = at::empty({q.size(0), max_chunks, hq, s.d + 2}, q.options().dtype(at::kFloat));
  auto o = at::empty({q.size(0), hq * s.d}, q.options());
  attn_rows_kv8_into(op, q, kc, vc, ks, vs, pos0, nullptr, (int)t, (int)max_keys, max_chunks, s, hq, part, o);
  return o;
}

void attn_rows_dev_kv8(const at::Tensor& q, const at::Tensor& kc, const at::Tensor& vc, const at::Tensor& ks,
                       const at::Tensor& vs, const at::Tensor& pos0, const at::Tensor& ctl, const at::Tensor& part,
                       const at::Tensor& o) {
  const char* op = "decode_attn_rows_dev_kv8";
  const KvShape s = check_kv8(op, q, kc, vc, ks, vs, true);
  check_pos0(op, pos0, q);
  check_ctl(op, ctl, q);
  const int64_t hq = q_heads(op, q.size(1), s);
  const int64_t max_chunks = (s.smax + DECODE_CHUNK - 1) / DECODE_CHUNK;
  TORCH_CHECK(max_chunks <= 65535, op, ": too many key chunks");
  check_attn_out(op, q, part, o, max_chunks, hq, s.d);
  const at::DeviceGuard guard(q.device());
  attn_rows_kv8_into(op, q, kc, vc, ks, vs, pos0, &ctl, 0, (int)s.smax, (int)max_chunks, s, hq, part, o);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(ftamd, m) {
  m.def("decode_qkv_append_kv8_(Tensor(a!) qkv, Tensor cos, Tensor sin, int pos, Tensor(b!) k_codes, "
        "Tensor(c!) v_codes, Tensor(d!) k_scale, Tensor(e!) v_scale) -> ()",
        &append_kv8);
  m.def("decode_qkv_append_rows_kv8_(Tensor(a!) qkv, Tensor cos, Tensor sin, Tensor pos0, int t, int max_pos, "
        "Tensor(b!) k_codes, Tensor(c!) v_codes, Tensor(d!) k_scale, Tensor(e!) v_scale) -> ()",
        &append_rows_kv8_host);
  m.def("decode_qkv_append_rows_dev_kv8_(Tensor(a!) qkv, Tensor cos, Tensor sin, Tensor pos0, Tensor ctl, "
        "Tensor(b!) k_codes, Tensor(c!) v_codes, Tensor(d!) k_scale, Tensor(e!) v_scale) -> ()",
        &append_rows_kv8_dev);
  m.def("kv_quantize_prefill_(Tensor k, Tensor v, Tensor(a!) k_codes, Tensor(b!) v_codes, Tensor(c!) k_scale, "
        "Tensor(d!) v_scale) -> ()",
        &kv_quantize_prefill);
  m.def("decode_attn_kv8(Tensor q, Tensor k_codes, Tensor v_codes, Tensor k_scale, Tensor v_scale, int n_keys) "
        "-> Tensor",
        &attn_kv8);
  m.def("decode_attn_rows_kv8(Tensor q, Tensor k_codes, Tensor v_codes, Tensor k_scale, Tensor v_scale, "
        "Tensor pos0, int t, int max_keys) -> Tensor",
        &attn_rows_kv8);
  m.def("decode_attn_rows_dev_kv8(Tensor q, Tensor k_codes, Tensor v_codes, Tensor k_scale, Tensor v_scale, "
        "Tensor pos0, Tensor ctl, Tensor(a!) part, Tensor(b!) o) -> ()",
        &attn_rows_dev_kv8);
}
