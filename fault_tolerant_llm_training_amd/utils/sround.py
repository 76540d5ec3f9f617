"""Stochastic rounding fp32 -> bf16 with stateless, counter-based random bits.

The exact twin, integer for integer, of ``csrc/kernels/sround.h`` (the function is written down
there; change both or neither). It is the CPU training path's implementation
(``optim.adamw._adamw_reference`` under ``--stochastic-rounding``) and the tests' oracle for the
device code (``torch.ops.ftamd.sr_round_bf16`` and the AdamW kernel's stores).

The 16 random bits of an element are a function of exactly ``(key, step, buffer, index)``:
``key`` 64-bit (from ``--seed``), ``step`` the optimizer step number (mod 2^32), ``buffer`` 0 for
params / 1 for ``exp_avg`` / 2 for ``exp_avg_sq``, ``index`` the element's global index in the flat
layout. One Philox4x32-6 call on counter ``(c & 0xffffffff, c >> 32, step, buffer)``, ``c = index >> 3``,
with key ``(key & 0xffffffff, key >> 32)`` yields four words ``w``; element ``j = index & 7`` takes
``r = (w[j >> 1] >> (16 * (j & 1))) & 0xffff``. A finite ``x`` with bit pattern ``u`` becomes
``(u + r) >> 16``; a non-finite ``x`` goes through the round-to-nearest conversion.
"""
from __future__ import annotations

import numpy as np
import torch

ROUNDS = 6
BUF_PARAM, BUF_EXP_AVG, BUF_EXP_AVG_SQ = 0, 1, 2
BUF_SAMPLE = 3  # the token sampler's stream (utils/sampling.py; csrc/kernels/decode.hip)

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def key_from_seed(seed: int) -> int:
    """The 64-bit key of a run from ``--seed`` (splitmix64's finalizer of seed + 1, kept to 63 bits
    so that it travels as a signed 64-bit operator argument): nearby seeds give unrelated keys."""
    m = (1 << 64) - 1
    z = (int(seed) + 1) * 0x9E3779B97F4A7C15 & m
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 & m
    z = (z ^ (z >> 27)) * 0x94D049BB133111EB & m
    z ^= z >> 31
    return z & ((1 << 63) - 1)


def philox_words(key: int, step: int, buffer: int, c: np.ndarray) -> np.ndarray:
    """Philox4x32-``ROUNDS`` of counter (c_lo, c_hi, step, buffer): uint64 array [len(c), 4] of 32-bit words."""
    c = np.ascontiguousarray(c, dtype=np.uint64)
    c0, c1 = c & _LO, c >> _S32
    c2 = np.full_like(c0, int(step) & 0xFFFFFFFF)
    c3 = np.full_like(c0, int(buffer) & 0xFFFFFFFF)
    k0, k1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    for _ in range(ROUNDS):
        p0 = _M0 * c0  # < 2^64: exact in uint64
        p1 = _M1 * c2
        n0 = (p1 >> _S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> _S32) ^ c3 ^ np.uint64(k1)
        c1, c3 = p1 & _LO, p0 & _LO
        c0, c2 = n0, n2
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1)


def random_bits(n: int, key: int, step: int, buffer: int, offset: int = 0) -> np.ndarray:
    """The 16 random bits (uint32 array, values < 2^16) of flat elements ``offset .. offset + n``."""
    if n <= 0:
        return np.zeros(0, dtype=np.uint32)
    offset = int(offset)
    first, last = offset >> 3, (offset + n - 1) >> 3
    # one generator call per vector: its 8 values are (w0 lo, w0 hi, w1 lo, ..., w3 hi)
    w = philox_words(key, step, buffer, np.arange(last - first + 1, dtype=np.uint64) + np.uint64(first))
    halves = np.stack([w & np.uint64(0xFFFF), w >> np.uint64(16)], axis=2).reshape(-1)
    lead = offset & 7
    return halves[lead : lead + n].astype(np.uint32)


def sr_round_bf16(x: torch.Tensor, key: int, step: int, buffer: int, offset: int = 0) -> torch.Tensor:
    """``x`` (fp32, CPU, any shape) -> bf16, element ``i`` (row-major) rounded with the random bits of
    ``(key, step, buffer, offset + i)``."""
    if x.dtype != torch.float32:
        raise TypeError(f"sr_round_bf16 rounds fp32 values, got {x.dtype}")
    xf = x.detach().contiguous().reshape(-1)
    u = xf.view(torch.int32).numpy().view(np.uint32)
    r = random_bits(u.size, key, step, buffer, offset)
    bits = ((u + r) >> np.uint32(16)).astype(np.uint16)  # finite: no carry out of bit 31
    nonfinite = (u & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
    if nonfinite.any():
        rn = xf.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        bits = np.where(nonfinite, rn, bits)
    out = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)
    return out.reshape(x.shape)
