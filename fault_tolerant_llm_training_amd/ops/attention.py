"""Causal GQA flash attention on packed projections (gfx950 HIP kernels).

Q and K come rotated (reference model.py:100-126) from one of two producers:
by default the QKV projection's GEMM epilogue (``gemm_qkv_rope_w4``, csrc/kernels/gemm_w4.hip)
rotates them in place, so ``qk`` IS the packed ``qkv`` projection ``[T, (Hq+2Hkv)*D]``; on the
paths without that epilogue (fp32, GPT-2-sized models, set_qkv_rope(False)) the RoPE kernel
(csrc/kernels/rope.hip) writes a separate rotated ``qk`` buffer ``[T, (Hq+Hkv)*D]``. V is always
read in place from ``qkv``. KV heads are indexed as ``h // (Hq/Hkv)`` inside the kernels, so
the reference's materialised ``repeat_kv`` (model.py:129-138) and the transpose/contiguous
copies (model.py:207-213) never exist. This module picks the kernel family by dtype
(bf16/fp16: csrc/kernels/flash_attn.hip, fp32: csrc/kernels/flash_f32.hip) and exposes the
deterministic / non-deterministic backward switch; and the autograd functions of RoPE +
attention on the packed projection (reference model.py:179-215).
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn.functional as F

from .._native import kernels, native

# Backward variant: 1 = deterministic (default): KV-major dK/dV kernel + Q-major dQ
# kernel, no atomics, bit-reproducible — GPU resume is bit-exact with it and it runs
# as fast as 0 = dQ accumulated with fp32 atomics in the KV-major kernel (Llama-3-8B
# layer shape: profiles/r1_flash_kernels.md).
_BWD_MODE = int(os.environ.get("FT_FLASH_BWD_MODE", "1"))
if _BWD_MODE not in (0, 1):
    raise ValueError(f"FT_FLASH_BWD_MODE must be 0 (dQ by atomics) or 1 (deterministic), got {_BWD_MODE}")


def set_deterministic(flag: bool) -> None:
    global _BWD_MODE
    _BWD_MODE = 1 if flag else 0


def doc_bounds(tokens: torch.Tensor, bos: int):
    """Document boundaries of packed sequences. tokens: [B, S] integer ids; a document starts at
    every ``bos``. Returns int32 ``(doc_start, doc_end)`` [B, S]: ``doc_start[i]`` = position of
    the most recent BOS at or before ``i`` (0 if none), ``doc_end[i]`` = position of the next BOS
    after ``i`` (S if none). Query ``i`` sees key ``j`` iff ``doc_start[i] <= j <= i``. On the GPU
    one scan kernel (csrc/kernels/doc_bounds.hip; no host sync, graph-capturable); elsewhere the
    same scans composed from cummax / cummin."""
    if tokens.is_cuda:
        return tuple(kernels().doc_bounds(tokens.long().contiguous(), int(bos)))
    B, S = tokens.shape
    pos = torch.arange(S, device=tokens.device).expand(B, S)
    is_bos = tokens == bos
    start = torch.where(is_bos, pos, torch.zeros_like(pos)).cummax(dim=1).values
    # next BOS strictly after i: a reversed running minimum, shifted by one
    nxt = torch.where(is_bos, pos, torch.full_like(pos, S)).flip(1).cummin(dim=1).values.flip(1)
    end = torch.cat([nxt[:, 1:], torch.full_like(pos[:, :1], S)], dim=1)
    return start.to(torch.int32), end.to(torch.int32)


def flash_attn_fwd(qk, qkv, S, hq, hkv, d, doc=None):
    """Returns (o [T, Hq*D], lse [B, Hq, S'] fp32) in the model dtype. The HIP kernels only, no
    fallback (``kernels()`` raises if the extension is missing): the MFMA kernels for bf16 / fp16
    (csrc/kernels/flash_attn.hip), the fp32 vector-ALU kernels for fp32 models (flash_f32.hip).
    ``doc = (doc_start, doc_end)`` (:func:`doc_bounds`): the document-masked kernels."""
    if doc is not None:
        if qk.dtype == torch.float32:
            return tuple(kernels().flash_f32_doc_fwd(qk, qkv, doc[0], doc[1], S, hq, hkv, d))
        return tuple(kernels().flash_doc_fwd(qk, qkv, doc[0], doc[1], S, hq, hkv, d))
    if qk.dtype == torch.float32:
        return tuple(kernels().flash_f32_fwd(qk, qkv, S, hq, hkv, d))
    return tuple(kernels().flash_fwd(qk, qkv, S, hq, hkv, d))


def flash_attn_bwd(do, qk, qkv, o, lse, S, hq, hkv, d, cos=None, sin=None, doc=None):
    """Returns dqkv [T, (Hq+2Hkv)*D]. With ``cos`` / ``sin`` the dQ / dK columns are rotated back
    (RoPE backward, reference model.py:100-126): the gradient of the UNROTATED projection — on the
    16-bit path inside the kernel pass that folds the GQA dK / dV partials (no separate RoPE
    pass); without them dQ / dK stay in the rotated frame. Both variants are deterministic (fp32:
    always; bf16 / fp16: unless FT_FLASH_BWD_MODE=0). ``doc``: the document-masked kernels
    (deterministic only)."""
    if doc is not None:
        if qk.dtype == torch.float32:
            dqkv = kernels().flash_f32_doc_bwd(do, qk, qkv, o, lse, doc[0], doc[1], S, hq, hkv, d)
            if cos is not None:
                kernels().rope_bwd_(dqkv, cos, sin, S, hq, hkv, d)
            return dqkv
        return kernels().flash_doc_bwd(do, qk, qkv, o, lse, doc[0], doc[1], S, hq, hkv, d, cos, sin)
    if qk.dtype == torch.float32:
        dqkv = kernels().flash_f32_bwd(do, qk, qkv, o, lse, S, hq, hkv, d)
        if cos is not None:
            kernels().rope_bwd_(dqkv, cos, sin, S, hq, hkv, d)
        return dqkv
    return kernels().flash_bwd(do, qk, qkv, o, lse, S, hq, hkv, d, _BWD_MODE, cos, sin)


# --------------------------------------------------------------------------------------
# RoPE + causal GQA attention on the fused QKV projection (autograd)
# --------------------------------------------------------------------------------------


def rope_reference(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """x: [B, S, H, D] interleaved pairs; cos/sin: [S, D/2] fp32."""
    xf = x.float().reshape(*x.shape[:-1], -1, 2)
    a, b = xf[..., 0], xf[..., 1]
    c = cos[: x.shape[1]].view(1, x.shape[1], 1, -1)
    s = sin[: x.shape[1]].view(1, x.shape[1], 1, -1)
    out = torch.stack((a * c - b * s, a * s + b * c), dim=-1).flatten(-2)
    return out.type_as(x)


def attention_reference(qkv, cos, sin, seq_len, hq, hkv, d, doc_start=None):
    """Reference math: RoPE → repeat_kv → causal SDPA (model.py:179-215). qkv: [B*S, W].
    ``doc_start`` [B, S]: the document mask (query i sees doc_start[i] <= j <= i) as a boolean
    SDPA mask instead of ``is_causal``."""
    T = qkv.shape[0]
    B = T // seq_len
    q = qkv[:, : hq * d].reshape(B, seq_len, hq, d)
    k = qkv[:, hq * d : (hq + hkv) * d].reshape(B, seq_len, hkv, d)
    v = qkv[:, (hq + hkv) * d :].reshape(B, seq_len, hkv, d)
    q = rope_reference(q, cos, sin)
    k = rope_reference(k, cos, sin)
    rep = hq // hkv
    if rep > 1:
        k = k.repeat_interleave(rep, dim=2)
        v = v.repeat_interleave(rep, dim=2)
    if doc_start is None:
        o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), is_causal=True)
    else:
        pos = torch.arange(seq_len, device=qkv.device)
        mask = (pos.view(1, 1, -1) <= pos.view(1, -1, 1)) & (pos.view(1, 1, -1) >= doc_start.view(B, -1, 1))
        o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                                           attn_mask=mask.view(B, 1, seq_len, seq_len))
    return o.transpose(1, 2).reshape(T, hq * d)


class AttentionKeep:
    """Per-block holder of the attention output kept across a recomputed block (selective
    activation checkpointing): the first forward of a checkpointed block stores (o, lse) here
    tagged with the model's forward generation; the recompute in backward (same generation)
    reuses them instead of running the flash forward again. A stale entry (a forward whose
    backward never ran) carries an older generation and is simply overwritten."""

    __slots__ = ("gen", "o", "lse")

    def __init__(self):
        self.gen, self.o, self.lse = -1, None, None


class RopeAttentionFn(torch.autograd.Function):
    """RoPE + causal GQA attention on the packed projection. ``rotated``: Q/K of ``qkv`` were
    already rotated by the QKV projection's epilogue (:class:`QKVRopeFn`, GPU only): the flash
    kernels then read Q/K straight from ``qkv``. Either way backward returns the gradient of the
    UNROTATED projection: the flash backward rotates dQ/dK back in the pass that folds the GQA
    dK/dV partials (so neither this node nor the projection's backward runs a RoPE pass)."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, seq_len, hq, hkv, d, keep=None, gen=-1, rotated=False, doc=None):
        ctx.cfg = (seq_len, hq, hkv, d)
        ctx.rotated = rotated
        # (doc_start, doc_end) int32, no gradient. Kept on ctx rather than through save_for_backward
        # on purpose: a checkpointed block is re-run with the same tensors as arguments (checkpoint
        # holds its inputs), nothing writes them after doc_bounds made them, and as non-float
        # side inputs they need neither the saved-tensor hooks nor version checks.
        ctx.doc = doc
        hit = keep is not None and keep.gen == gen and keep.o is not None
        if native(qkv):
            qkv = qkv.contiguous()
            qk = qkv if rotated else kernels().rope_fwd(qkv, cos, sin, seq_len, hq, hkv, d)
            if hit:  # recompute pass of a checkpointed block: the kept output (bit-identical)
                o, lse = keep.o, keep.lse
                keep.o = keep.lse = None
            else:
                o, lse = flash_attn_fwd(qk, qkv, seq_len, hq, hkv, d, doc)
                if keep is not None:
                    keep.gen, keep.o, keep.lse = gen, o, lse
            ctx.save_for_backward(qkv, qk, o, lse, cos, sin)
            return o
        ctx.save_for_backward(qkv, cos, sin)
        if hit:
            o = keep.o
            keep.o = None
        else:
            o = attention_reference(qkv, cos, sin, seq_len, hq, hkv, d, None if doc is None else doc[0])
            if keep is not None:
                keep.gen, keep.o = gen, o
        return o

    @staticmethod
    def backward(ctx, do):
        seq_len, hq, hkv, d = ctx.cfg
        if native(do):
            qkv, qk, o, lse, cos, sin = ctx.saved_tensors
            dqkv = flash_attn_bwd(do.contiguous(), qk, qkv, o, lse, seq_len, hq, hkv, d, cos, sin, ctx.doc)
            return dqkv, None, None, None, None, None, None, None, None, None, None
        qkv, cos, sin = ctx.saved_tensors
        with torch.enable_grad():
            x = qkv.detach().requires_grad_(True)
            o = attention_reference(x, cos, sin, seq_len, hq, hkv, d, None if ctx.doc is None else ctx.doc[0])
            (dx,) = torch.autograd.grad(o, (x,), do)
        return dx, None, None, None, None, None, None, None, None, None, None


def rope_attention(qkv, cos, sin, seq_len, hq, hkv, d, keep: Optional[AttentionKeep] = None, gen: int = -1,
                   rotated: bool = False, doc=None):
    """RoPE on the packed projection, then causal GQA attention. ``keep``/``gen``: selective
    activation checkpointing (see :class:`AttentionKeep`). ``doc = (doc_start, doc_end)``
    (:func:`doc_bounds`): attention within each packed document only. RoPE positions stay the
    in-sequence ones: rotary scores depend on i - j alone, so resetting them per document would
    give the same attention."""
    return RopeAttentionFn.apply(qkv, cos, sin, seq_len, hq, hkv, d, keep, gen, rotated, doc)


# QKV projection with RoPE in the GEMM epilogue (csrc/kernels/gemm_w4.hip, gemm_qkv_rope_w4): the
# hand-written 4-wave GEMM writes qkv with Q/K already rotated, so neither the separate RoPE
# kernel nor the rotated [T, (Hq + Hkv) D] copy exists; the flash kernels read Q/K from qkv.
# Default on (8B step: 1.001-1.003x, the RoPE forward kernel and the rotated copy gone; the
# kernel alone runs the Llama-3-8B QKV shape at 1.10-1.14x hipBLASLt, profiles/r3_gemm_w4_investigation.md);
# set_qkv_rope(False) restores the plain projection + the RoPE kernel (A/B).
_QKV_ROPE = True
# model dim from which the fused projection wins (see _qkv_rope_ok; FT_QKV_ROPE_MIN_K: A/B)
_QKV_ROPE_MIN_K = int(os.environ.get("FT_QKV_ROPE_MIN_K", "2048"))
# output tiles its grid needs: half the chip (the kernel takes no K split; see _qkv_rope_ok)
_QKV_ROPE_MIN_TILES = 128


def set_qkv_rope(on: bool) -> None:
    global _QKV_ROPE
    _QKV_ROPE = bool(on)


def _qkv_rope_ok(x2: torch.Tensor, w: torch.Tensor, d: int) -> bool:
    if not (_QKV_ROPE and Fx._W4_FWD and w.is_contiguous()):
        return False
    # K >= 2048 (the 8B-class projections): at GPT-2 sizes (K = 768 / 1024) the epilogue kernel
    # loses ~1 % of the step to hipBLASLt + the RoPE kernel (profiles/r3_gpt2_w4_ab.log). The
    # kernel takes no K split: the tile grid alone must fill half the chip.
    T, K = x2.shape
    N = w.shape[0]
    if d % 8 or K < _QKV_ROPE_MIN_K or not Fx.w4_route(T, N, K, False, False, x2, w):
        return False
    nj = kernels().gemm_w4_pick(T, N)
    return nj > 0 and (T // 256) * (N // (32 * nj)) >= _QKV_ROPE_MIN_TILES


class QKVRopeFn(torch.autograd.Function):
    """qkv = x W^T with Q/K rotated (reference model.py:195 then :100-126). Backward receives the
    gradient of the unrotated projection (the attention backward already rotated dQ/dK back,
    :class:`RopeAttentionFn`), then dW / dX."""

    @staticmethod
    def forward(ctx, x2, w, sink, cos, sin, seq_len, hq, hkv, d):
        ctx.sink = sink
        ctx.cfg = (seq_len, hq, hkv, d)
        ctx.save_for_backward(x2, w, cos, sin)
        return kernels().gemm_qkv_rope_w4(x2, w, cos, sin, seq_len, hq, hkv, d)

    @staticmethod
    def backward(ctx, dq):
        x2, w, cos, sin = ctx.saved_tensors
        seq_len, hq, hkv, d = ctx.cfg
        dq = dq.contiguous()
        dw = Fx.weight_grad_async(dq, x2, ctx.sink)
        dx = Fx.mm_dx(dq, w)
        return dx, dw, None, None, None, None, None, None, None


def qkv_rope_attention(xn, wqkv, sink, cos, sin, seq_len, hq, hkv, d, keep: Optional[AttentionKeep] = None,
                       gen: int = -1, doc=None):
    """QKV projection + RoPE + causal GQA attention (reference model.py:179-212). Returns o [.., Hq D]."""
    x2 = xn.reshape(-1, xn.shape[-1])
    if _qkv_rope_ok(x2, wqkv, d):
        qkv = QKVRopeFn.apply(x2.contiguous(), wqkv, sink, cos, sin, seq_len, hq, hkv, d)
        return rope_attention(qkv, cos, sin, seq_len, hq, hkv, d, keep, gen, rotated=True, doc=doc)
    qkv = Fx.linear(xn, wqkv, sink)
    return rope_attention(qkv.view(-1, qkv.shape[-1]), cos, sin, seq_len, hq, hkv, d, keep, gen, doc=doc)


@torch.no_grad()
def qkv_rope_attention_kv(xn, wqkv, cos, sin, seq_len, hq, hkv, d):
    """:func:`qkv_rope_attention` for the prefill of text generation (forward only, plain causal
    attention): the same projection, RoPE and flash forward on the same route, and besides o the
    rotated K and the V of every row, ``[T, Hkv D]`` each, for the KV cache. On the QKV-epilogue
    route the rotated K is a slice of ``qkv``, on the other one a slice of the RoPE kernel's output;
    V is a slice of ``qkv`` on both."""
    x2 = xn.reshape(-1, xn.shape[-1])
    a, b = hq * d, (hq + hkv) * d
    if not native(x2):
        qkv = Fx.linear(xn, wqkv, None).view(x2.shape[0], -1)
        B = x2.shape[0] // seq_len
        k = rope_reference(qkv[:, a:b].reshape(B, seq_len, hkv, d), cos, sin).reshape(-1, hkv * d)
        return attention_reference(qkv, cos, sin, seq_len, hq, hkv, d), k, qkv[:, b:]
    if _qkv_rope_ok(x2, wqkv, d):
        qkv = QKVRopeFn.apply(x2.contiguous(), wqkv, None, cos, sin, seq_len, hq, hkv, d)
        qk = qkv
    else:
        qkv = Fx.linear(xn, wqkv, None).view(x2.shape[0], -1).contiguous()
        qk = kernels().rope_fwd(qkv, cos, sin, seq_len, hq, hkv, d)
    o, _ = flash_attn_fwd(qk, qkv, seq_len, hq, hkv, d)
    return o, qk[:, a:b], qkv[:, b:]


# functional.py re-exports this module's names at its end and this module calls into functional at
# run time: imported last, so either module can be imported first
from . import functional as Fx  # noqa: E402
