"""One-row (decode) ops of text generation and their multi-row forms: wrappers of
csrc/kernels/decode.hip.

GPU tensors of a kernel dtype run the HIP kernels (``kernels()`` raises if the library is
missing); CPU tensors and fp64 take the composed-PyTorch definition of the same math, as in
``ops.functional``. ``generation.py`` is the caller.

The device-step forms at the end (``qkv_append_rows_dev_``, ``attn_rows_dev``, ``sample_dev_``,
``ctl_advance_``) take the per-token state -- the step ``t`` and the sampling arguments -- from a
small control block ``ctl`` in device memory instead of from host arguments, so a captured launch of
them serves every token of every call (``generation.DecodeGraph``).
"""
from __future__ import annotations

import math
import struct
from typing import Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from .._native import kernels, native
from .attention import rope_reference
from .functional import swiglu_reference


def _gemv_ok(x: torch.Tensor, w: torch.Tensor) -> bool:
    """The kernel's preconditions: 16-byte vectors along K (K % 8, fp32: K % 4) of contiguous,
    16-byte aligned operands. Anything else goes to ``torch.mv`` (the route ``f32_route`` leaves to
    hipBLASLt for the same reason)."""
    vn = 4 if w.dtype == torch.float32 else 8
    return (native(w) and native(x) and x.dtype == w.dtype and w.dim() == 2 and x.dim() == 1
            and w.shape[1] % vn == 0 and w.shape[1] > 0 and w.shape[0] > 0 and w.is_contiguous()
            and x.is_contiguous() and w.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0)


def gemv(x: torch.Tensor, w: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[N] = w[N, K] x[K] (+ residual[N])."""
    if _gemv_ok(x, w):
        return kernels().gemv(x, w, None if residual is None else residual.contiguous())
    y = torch.mv(w, x)
    return y if residual is None else y + residual


def gemv_swiglu(x: torch.Tensor, w13: torch.Tensor) -> torch.Tensor:
    """a[H] = silu(w1 x) * (w3 x) on the fused [w1; w3] view [2H, K]."""
    if _gemv_ok(x, w13) and w13.shape[0] % 2 == 0:
        return kernels().gemv_swiglu(x, w13)
    return swiglu_reference(torch.mv(w13, x))


def qkv_append_(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: int, k_cache: torch.Tensor,
                v_cache: torch.Tensor) -> None:
    """RoPE at ``pos`` on Q (in place) and K (into ``k_cache[:, pos]``), V into ``v_cache[:, pos]``.
    qkv: [(Hq + 2 Hkv) D]; caches: [Hkv, Smax, D]."""
    if native(qkv):
        kernels().decode_qkv_append_(qkv, cos, sin, int(pos), k_cache, v_cache)
        return
    hkv, _, d = k_cache.shape
    hq = qkv.numel() // d - 2 * hkv
    c, s = cos[pos : pos + 1], sin[pos : pos + 1]
    qk = rope_reference(qkv[: (hq + hkv) * d].view(1, 1, hq + hkv, d), c, s).view(hq + hkv, d)
    qkv[: hq * d] = qk[:hq].reshape(-1)
    k_cache[:, pos] = qk[hq:]
    v_cache[:, pos] = qkv[(hq + hkv) * d :].view(hkv, d)


def attn(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, n_keys: int) -> torch.Tensor:
    """o[Hq D]: one (rotated) query over keys ``0 .. n_keys - 1`` of the caches; GQA."""
    if native(q):
        return kernels().decode_attn(q, k_cache, v_cache, int(n_keys))
    hkv, _, d = k_cache.shape
    hq = q.numel() // d
    k = k_cache[:, :n_keys].repeat_interleave(hq // hkv, dim=0)  # [Hq, n, D]
    v = v_cache[:, :n_keys].repeat_interleave(hq // hkv, dim=0)
    s = torch.einsum("hd,hnd->hn", q.view(hq, d), k) / math.sqrt(d)
    return torch.einsum("hn,hnd->hd", F.softmax(s, dim=-1), v).reshape(-1)


# ---------------------------------------------------------------------------------------------
# The multi-row forms (batched generation). Row r of each result has the bits the one-row op above
# returns for that row alone, on either route: the kernels keep the per-row arithmetic order, and
# the composed definition is a loop over rows of the one-row definitions.
# ---------------------------------------------------------------------------------------------
def _gemv_rows_ok(x: torch.Tensor, w: torch.Tensor) -> bool:
    """``_gemv_ok`` for x [R, K], R >= 1."""
    return x.dim() == 2 and x.shape[0] >= 1 and x.is_contiguous() and _gemv_ok(x[0], w)


def gemv_rows(x: torch.Tensor, w: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[R, N] = x[R, K] w[N, K]^T (+ residual[R, N]); row r equals ``gemv(x[r], w, residual[r])``."""
    if _gemv_rows_ok(x, w):
        return kernels().gemv_rows(x, w, None if residual is None else residual.contiguous())
    return torch.stack([gemv(x[r], w, None if residual is None else residual[r]) for r in range(x.shape[0])])


def gemv_swiglu_rows(x: torch.Tensor, w13: torch.Tensor) -> torch.Tensor:
    """a[R, H]; row r equals ``gemv_swiglu(x[r], w13)``."""
    if _gemv_rows_ok(x, w13) and w13.shape[0] % 2 == 0:
        return kernels().gemv_swiglu_rows(x, w13)
    return torch.stack([gemv_swiglu(x[r], w13) for r in range(x.shape[0])])


def qkv_append_rows_(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos0: torch.Tensor, t: int,
                     k_cache: torch.Tensor, v_cache: torch.Tensor, positions: Sequence[int]) -> None:
    """``qkv_append_`` on row b of qkv [B, (Hq + 2 Hkv) D] at position ``pos0[b] + t`` of the caches
    [B, Hkv, Smax, D]. ``positions`` is the host's copy of ``pos0``: the kernel route takes only its
    maximum from it (the bound the op checks), so the device tensor is never read back."""
    if native(qkv):
        kernels().decode_qkv_append_rows_(qkv, cos, sin, pos0, int(t), max(positions) + int(t), k_cache, v_cache)
        return
    for b, p in enumerate(positions):
        qkv_append_(qkv[b], cos, sin, int(p) + int(t), k_cache[b], v_cache[b])


def attn_rows(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos0: torch.Tensor, t: int,
              positions: Sequence[int]) -> torch.Tensor:
    """o[B, Hq D]; row b equals ``attn(q[b], k_cache[b], v_cache[b], pos0[b] + t + 1)``."""
    if native(q):
        return kernels().decode_attn_rows(q, k_cache, v_cache, pos0, int(t), max(positions) + int(t) + 1)
    return torch.stack([attn(q[b], k_cache[b], v_cache[b], int(p) + int(t) + 1) for b, p in enumerate(positions)])


def _check_top_p(top_p: float) -> float:
    """``top_p`` unchanged, after the definition's check (the kernel takes it as float32: a value that
    rounds to 0 there is as wrong as 0)."""
    from ..utils.sampling import check_top_p

    check_top_p(top_p)
    return float(top_p)


def sample(logits: torch.Tensor, temperature: float, top_k: int, key: int, step: int,
           top_p: float = 1.0) -> torch.Tensor:
    """One token per row of ``logits`` ([V] or [R, V]): int64 tensor [R] on ``logits``' device.
    The definition is ``utils.sampling.sample_reference``."""
    top_p = _check_top_p(top_p)
    x2 = logits.reshape(-1, logits.shape[-1])
    if native(x2) and x2.shape[1] % 8 == 0:
        out = torch.empty(x2.shape[0], dtype=torch.int64, device=x2.device)
        kernels().sample_(x2.contiguous(), out, float(temperature), int(top_k), int(key), int(step), top_p)
        return out
    from ..utils.sampling import sample_reference

    return sample_reference(x2, temperature, top_k, key, step, top_p=top_p).to(x2.device)


# ---------------------------------------------------------------------------------------------
# The device-step forms. ``ctl`` is an int32 tensor of CTL_WORDS words on the operands' device (the
# indices of csrc/kernels/decode.hip); the host writes it once per call with ``write_ctl`` and the
# kernel route never reads it back. The composed route (CPU, fp64) reads it on the host and calls the
# definitions above.
# ---------------------------------------------------------------------------------------------
CTL_T, CTL_KEY_LO, CTL_KEY_HI, CTL_STEP, CTL_TEMPERATURE, CTL_TOP_K, CTL_TOP_P = range(7)
CTL_WORDS = 8
_M32 = 0xFFFFFFFF


def new_ctl(device) -> torch.Tensor:
    return torch.zeros(CTL_WORDS, dtype=torch.int32, device=device)


def write_ctl(ctl: torch.Tensor, t: int, temperature: float, top_k: int, key: int, step: int,
              top_p: float = 1.0) -> None:
    """Fill the control block: step counter ``t``, and the sampling arguments of ``sample`` -- the
    temperature as the float32 the kernel takes, the call's key (not a token's) as two words, and
    ``top_p`` as float32 bits, 0 standing for 1.0 (off)."""
    top_p = _check_top_p(top_p)
    if not (0.0 <= float(temperature) < math.inf) or int(top_k) < 0 or int(t) < 0:
        raise ValueError("temperature must be finite and >= 0, top_k and t >= 0")
    tbits = struct.unpack("<I", struct.pack("<f", float(temperature)))[0]
    pbits = 0 if top_p == 1.0 else struct.unpack("<I", struct.pack("<f", top_p))[0]
    words = [int(t) & _M32, int(key) & _M32, (int(key) >> 32) & _M32, int(step) & _M32, tbits,
             min(int(top_k), 0x7FFFFFFF), pbits, 0]
    ctl.copy_(torch.tensor(struct.unpack("<8i", struct.pack("<8I", *words)), dtype=torch.int32))


def read_ctl(ctl: torch.Tensor) -> Tuple[int, float, int, int, int]:
    """``(t, temperature, top_k, key, step)`` of a control block, on the host (the composed route)."""
    w = [int(x) & _M32 for x in ctl.tolist()]
    t = w[CTL_T] - (1 << 32) if w[CTL_T] >> 31 else w[CTL_T]
    temperature = struct.unpack("<f", struct.pack("<I", w[CTL_TEMPERATURE]))[0]
    return t, temperature, w[CTL_TOP_K], w[CTL_KEY_LO] | (w[CTL_KEY_HI] << 32), w[CTL_STEP]


def read_ctl_top_p(ctl: torch.Tensor) -> float:
    """``top_p`` of a control block, as the kernel reads it: the float32 in word CTL_TOP_P, and 1.0 (off)
    for a word of 0 or a value that is not inside (0, 1)."""
    w = int(ctl[CTL_TOP_P]) & _M32
    p = struct.unpack("<f", struct.pack("<I", w))[0]
    return p if 0.0 < p < 1.0 else 1.0


def ctl_advance_(ctl: torch.Tensor) -> None:
    """``t += 1``: on the device in stream order, behind every op of the pass that read ``t``."""
    if ctl.is_cuda:
        kernels().decode_ctl_advance_(ctl)
    else:
        ctl[CTL_T] += 1


def qkv_append_rows_dev_(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos0: torch.Tensor,
                         ctl: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor) -> None:
    """``qkv_append_rows_`` with ``t`` taken from ``ctl``: row b at position ``pos0[b] + t``. A position
    outside the cache or the RoPE tables writes nothing (and leaves that row's Q unrotated)."""
    if native(qkv):
        kernels().decode_qkv_append_rows_dev_(qkv, cos, sin, pos0, ctl, k_cache, v_cache)
        return
    t = read_ctl(ctl)[0]
    limit = min(k_cache.shape[2], cos.shape[0])
    for b, p in enumerate(pos0.tolist()):
        if 0 <= p + t < limit:
            qkv_append_(qkv[b], cos, sin, p + t, k_cache[b], v_cache[b])


def attn_rows_dev(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos0: torch.Tensor,
                  ctl: torch.Tensor, part: torch.Tensor, o: torch.Tensor) -> torch.Tensor:
    """``attn_rows`` with ``t`` taken from ``ctl``, into the caller's ``o`` [B, Hq D]; ``part`` is the
    kernel's workspace, fp32 ``[B, ceil(Smax / chunk), Hq, D + 2]`` (``attn_part``). Returns ``o``."""
    if native(q):
        kernels().decode_attn_rows_dev(q, k_cache, v_cache, pos0, ctl, part, o)
        return o
    t = read_ctl(ctl)[0]
    o.copy_(attn_rows(q, k_cache, v_cache, pos0, t, pos0.tolist()))
    return o


def attn_part(batch: int, hq: int, smax: int, d: int, device) -> torch.Tensor:
    """The workspace of ``attn_rows_dev`` for caches of capacity ``smax`` (one element where the composed
    route runs, which needs none)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        return torch.empty(1, dtype=torch.float32, device=dev)
    chunk = int(kernels().decode_attn_chunk())
    return torch.empty(batch, (smax + chunk - 1) // chunk, hq, d + 2, dtype=torch.float32, device=dev)


def sample_dev_(logits: torch.Tensor, ctl: torch.Tensor, tok: torch.Tensor, out: torch.Tensor) -> None:
    """``sample(logits, temperature, top_k, token_key(key, t), step, top_p)`` with all six taken from ``ctl``:
    row b's token goes to ``tok[b]`` (int64, B elements) and to ``out[b, t]`` (int64 ``[B, n_cap]``)."""
    if native(logits) and logits.dim() == 2 and logits.shape[1] % 8 == 0:
        kernels().sample_dev_(logits, ctl, tok, out)
        return
    from ..utils.sampling import token_key

    t, temperature, top_k, key, step = read_ctl(ctl)
    nxt = sample(logits, temperature, top_k, token_key(key, t), step, read_ctl_top_p(ctl)).to(tok.device)
    tok.copy_(nxt.view_as(tok))
    if 0 <= t < out.shape[1]:
        out[:, t] = nxt
