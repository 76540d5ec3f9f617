// What the host sides of the decode ops share (decode.hip, decode_w8.hip, decode_mx4.hip, decode_mma.hip,
// decode_kv8.hip): the operand checks, each written once, and the dispatch from a runtime head_dim,
// GQA group or row count to the template parameter that serves it. Every message starts with the op's
// name.
#pragma once

#include <climits>

#include "decode_attn.h"  // CTL_WORDS
#include "torch_utils.h"

namespace {

inline void check_vec(const char* op, const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, op, ": ", name, " must be 16-byte aligned");
}

// The residual of a product on x [K] or [R, K]: x's shape with N for K, its dtype and device.
inline void check_residual(const char* op, const at::Tensor& residual, const at::Tensor& x, int64_t N) {
  TORCH_CHECK(residual.is_cuda() && residual.is_contiguous() && residual.scalar_type() == x.scalar_type() &&
                  residual.device() == x.device() && residual.dim() == x.dim() && residual.size(-1) == N &&
                  residual.numel() == x.numel() / x.size(-1) * N,
              op, ": residual must be a contiguous [N] (x [R, K]: [R, N]) tensor of x's dtype, on its device");
}

// The tile of activation rows of a gemv launch: the smallest of 1, 2, 4, 8 that holds R; beyond `top`
// (4 or 8) rows, tiles of `top`.
inline int rows_tile(int64_t R, int top) { return R == 1 ? 1 : R == 2 ? 2 : (R <= 4 || top == 4) ? 4 : 8; }

// Runs the body with RT = rt, a result of rows_tile(R, TOP). TOP takes the last branch, so a kernel
// whose top tile is 4 is never instantiated for 8.
#define FT_ROWS_TILE(rt, TOP, ...)  \
  do {                              \
    if ((rt) == 1) {                \
      constexpr int RT = 1;         \
      __VA_ARGS__;                  \
    } else if ((rt) == 2) {         \
      constexpr int RT = 2;         \
      __VA_ARGS__;                  \
    } else if ((rt) == 4) {         \
      constexpr int RT = 4;         \
      __VA_ARGS__;                  \
    } else {                        \
      constexpr int RT = (TOP);     \
      __VA_ARGS__;                  \
    }                               \
  } while (0)

// Runs the body with D = d, a head_dim the caller has checked to be 64 or 128.
#define FT_DECODE_D(d, ...)         \
  do {                              \
    if ((d) == 64) {                \
      constexpr int D = 64;         \
      __VA_ARGS__;                  \
    } else {                        \
      constexpr int D = 128;        \
      __VA_ARGS__;                  \
    }                               \
  } while (0)

// the GQA tile: the smallest of 1, 2, 4, 8 that holds the group, 8 beyond
#define FT_DECODE_GT(G, ...)        \
  do {                              \
    if ((G) == 1) {                 \
      constexpr int GT = 1;         \
      __VA_ARGS__;                  \
    } else if ((G) == 2) {          \
      constexpr int GT = 2;         \
      __VA_ARGS__;                  \
    } else if ((G) <= 4) {          \
      constexpr int GT = 4;         \
      __VA_ARGS__;                  \
    } else {                        \
      constexpr int GT = 8;         \
      __VA_ARGS__;                  \
    }                               \
  } while (0)

struct KvShape {
  int64_t hkv, smax, d;
};

// The activation x ([width] for rows == false, else [B, width], which may be a column slice of a wider
// buffer) and the caches of one layer, [Hkv, Smax, D] or [B, Hkv, Smax, D] of element type `ctype`, on
// x's device. x's dtype and the head_dim are the caller's to check. Returns (Hkv, Smax, D).
inline KvShape check_kv(const char* op, const at::Tensor& x, const at::Tensor& kc, const at::Tensor& vc,
                        at::ScalarType ctype, bool rows) {
  TORCH_CHECK(x.is_cuda() && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, op,
              ": the activation must be a 16-byte aligned GPU tensor");
  const int lead = rows ? 1 : 0;
  if (rows) {
    TORCH_CHECK(x.dim() == 2 && x.size(0) >= 1 && x.size(0) <= 65535 && x.stride(1) == 1 &&
                    x.stride(0) >= x.size(1) && x.stride(0) % 8 == 0,
                op, ": the activation is [B, width], 1 <= B <= 65535, rows dense and a multiple of 8 elements apart");
  } else {
    TORCH_CHECK(x.dim() == 1 && x.is_contiguous(), op, ": the activation is a contiguous [width] tensor");
  }
  TORCH_CHECK(kc.dim() == 3 + lead, op, rows ? ": a cache is [B, Hkv, Smax, D]" : ": a cache is [Hkv, Smax, D]");
  for (const at::Tensor* c : {&kc, &vc}) {
    TORCH_CHECK(c->is_cuda() && c->device() == x.device() && c->scalar_type() == ctype && c->is_contiguous() &&
                    c->sizes() == kc.sizes(),
                op, ": the caches are contiguous ", c10::toString(ctype), " tensors of one shape on the activation's device");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(c->data_ptr()) % 16 == 0, op, ": a cache must be 16-byte aligned");
  }
  TORCH_CHECK(!rows || kc.size(0) == x.size(0), op, ": the caches hold one sequence per activation row");
  const KvShape r{kc.size(lead), kc.size(lead + 1), kc.size(lead + 2)};
  TORCH_CHECK(r.hkv >= 1 && r.smax >= 1 && r.smax <= INT_MAX, op, ": empty cache, or Smax beyond 32 bits");
  return r;
}

inline void check_pos0(const char* op, const at::Tensor& pos0, const at::Tensor& x) {
  TORCH_CHECK(pos0.is_cuda() && pos0.device() == x.device() && pos0.scalar_type() == at::kInt &&
                  pos0.is_contiguous() && pos0.dim() == 1 && pos0.size(0) == x.size(0),
              op, ": pos0 must be a contiguous int32 [B] tensor on the activation's device");
}

inline void check_ctl(const char* op, const at::Tensor& ctl, const at::Tensor& like) {
  TORCH_CHECK(ctl.is_cuda() && ctl.device() == like.device() && ctl.scalar_type() == at::kInt && ctl.is_contiguous() &&
                  ctl.dim() == 1 && ctl.size(0) >= CTL_WORDS,
              op, ": ctl must be a contiguous int32 tensor of at least ", (int)CTL_WORDS, " words on the operands' device");
}

// cos / sin: fp32 [S >= need, D / 2] on qkv's device
inline void check_rope(const char* op, const at::Tensor& cos_t, const at::Tensor& sin_t, const at::Tensor& qkv,
                       int64_t d, int64_t need) {
  for (const at::Tensor* c : {&cos_t, &sin_t}) {
    TORCH_CHECK(c->is_cuda() && c->device() == qkv.device() && c->scalar_type() == at::kFloat && c->is_contiguous() &&
                    c->dim() == 2 && c->size(1) == d / 2 && c->size(0) == cos_t.size(0) && c->size(0) >= need,
                op, ": cos / sin must be fp32 [S, D / 2] on qkv's device, S beyond the largest position");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(c->data_ptr()) % 16 == 0, op, ": cos / sin alignment");
  }
}

// Hq of a qkv row of `width` elements
inline int64_t qkv_heads(const char* op, int64_t width, const KvShape& s) {
  TORCH_CHECK(width % s.d == 0 && width / s.d > 2 * s.hkv, op, ": qkv width");
  return width / s.d - 2 * s.hkv;
}

inline int64_t q_heads(const char* op, int64_t width, const KvShape& s) {
  TORCH_CHECK(width % s.d == 0 && width > 0 && (width / s.d) % s.hkv == 0, op,
              ": q is [.., Hq D] with Hq a positive multiple of Hkv");
  return width / s.d;
}

// The positions of a `_rows` append: t from the host, checked with the caller's largest position max_pos
// (ctl == nullptr), or read from ctl[CTL_T] on the device, where the only bound the host can name is the
// capacity of the cache and the RoPE tables. Returns the bound the kernel holds every row's position to.
inline long check_append_rows(const char* op, const at::Tensor& qkv, const at::Tensor& cos_t, const at::Tensor& sin_t,
                              const at::Tensor* ctl, int64_t t, int64_t max_pos, const KvShape& s) {
  if (ctl != nullptr) {
    check_ctl(op, *ctl, qkv);
    check_rope(op, cos_t, sin_t, qkv, s.d, 0);
    return (long)std::min<int64_t>(s.smax, cos_t.size(0));
  }
  TORCH_CHECK(t >= 0 && t <= INT_MAX && max_pos >= t && max_pos < s.smax, op, ": largest position ", max_pos,
              " (t = ", t, ") outside the cache [0, ", s.smax, ")");
  check_rope(op, cos_t, sin_t, qkv, s.d, max_pos + 1);
  return (long)(max_pos + 1);
}

// part and o of the `_rows_dev` attention ops, which the caller allocates for the cache's capacity.
inline void check_attn_out(const char* op, const at::Tensor& q, const at::Tensor& part, const at::Tensor& o,
                           int64_t max_chunks, int64_t hq, int64_t d) {
  const int64_t B = q.size(0);
  TORCH_CHECK(part.is_cuda() && part.device() == q.device() && part.scalar_type() == at::kFloat &&
                  part.is_contiguous() && part.numel() == B * max_chunks * hq * (d + 2),
              op, ": part must be a contiguous fp32 [B, ceil(Smax / ", DECODE_CHUNK, "), Hq, D + 2] tensor");
  TORCH_CHECK(o.is_cuda() && o.device() == q.device() && o.scalar_type() == q.scalar_type() && o.is_contiguous() &&
                  o.dim() == 2 && o.size(0) == B && o.size(1) == hq * d,
              op, ": o must be a contiguous [B, Hq D] tensor of q's dtype");
}

}  // namespace
