"""Bit-level fingerprints of the training state, for resume-equivalence checks at full scale.

A Llama-3-8B state is 48 GB per copy; comparing an uninterrupted run with an interrupted-and-resumed
one through checkpoint files needs three of them on disk. Instead each run logs a digest of its
final parameters and AdamW moments (``--state-digest``) and only the interruption's checkpoint is
written. The digest is an order-independent exact integer sum, so it is deterministic on any
device: every element's raw bits (int16 view for 16-bit dtypes, int32 for fp32) times a
position-dependent weight, summed in int64 with wrap-around. Any bit flip or displaced element
changes it; equal states give equal digests.

The weight of an element is ``(position mod 1_000_003) + 1``, with the position counted from
``first_pos``: digests of disjoint pieces of a buffer add up (mod 2^64) to the digest of the
whole, which is how sharded saves and ZeRO-1 resumes form it. On a GPU tensor of a kernel dtype
the sum is one streaming pass of ``csrc/kernels/digest.hip``; the PyTorch composition below stays
the CPU path and the oracle, and gives the same value bit for bit. Every checkpoint stores these
digests and a resume checks them (``ckpt/verify.py``).
"""
from __future__ import annotations

import torch

_CHUNK = 1 << 27
_MOD = 1_000_003


MASK64 = 0xFFFFFFFFFFFFFFFF
# dtypes the gfx950 kernel (csrc/kernels/digest.hip) covers; others take the composition
_KERNEL_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _composed(flat: torch.Tensor, first_pos: int) -> int:
    if flat.dtype in (torch.bfloat16, torch.float16):
        bits = flat.view(torch.int16)
    elif flat.dtype == torch.float32:
        bits = flat.view(torch.int32)
    elif flat.dtype == torch.float64:
        bits = flat.view(torch.int64)
    else:
        bits = flat
    total = torch.zeros((), dtype=torch.int64, device=flat.device)
    for lo in range(0, bits.numel(), _CHUNK):
        b = bits[lo : lo + _CHUNK].to(torch.int64)
        p0 = first_pos + lo
        w = torch.arange(p0, p0 + b.numel(), dtype=torch.int64, device=b.device).remainder_(_MOD).add_(1)
        total += (b * w).sum()
    return int(total.item()) & MASK64


def digest_accum(acc: torch.Tensor, slot: int, t: torch.Tensor, first_pos: int = 0) -> None:
    """``acc[slot] +=`` the digest of ``t`` (contiguous, on ``acc``'s GPU, bf16 / fp16 / fp32) with
    its first element at position ``first_pos`` of the buffer it is a piece of. One streaming
    kernel on the current stream, no host sync: the form the checkpoint engine uses."""
    from .._native import kernels

    kernels().digest_accum_(acc, int(slot), t.detach().reshape(-1), int(first_pos))


def digest_int(t: torch.Tensor, first_pos: int = 0) -> int:
    """The digest of ``t`` as an int in [0, 2^64). ``first_pos`` is the position of ``t``'s first
    element in the buffer it is a piece of: digests of disjoint pieces add up (mod 2^64) to the
    digest of the whole buffer."""
    flat = t.detach().reshape(-1)
    if flat.is_cuda and flat.dtype in _KERNEL_DTYPES:
        acc = torch.zeros(1, dtype=torch.int64, device=flat.device)
        digest_accum(acc, 0, flat, first_pos)
        return int(acc.item()) & MASK64
    return _composed(flat, int(first_pos))


def tensor_digest(t: torch.Tensor, first_pos: int = 0) -> str:
    """16-hex-digit digest of the raw bits of ``t`` (any shape, contiguous or not)."""
    return f"{digest_int(t, first_pos):016x}"


def state_digest(params: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor) -> dict:
    return {"params": tensor_digest(params), "exp_avg": tensor_digest(exp_avg),
            "exp_avg_sq": tensor_digest(exp_avg_sq)}
