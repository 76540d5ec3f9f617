"""The weight-only MXFP4 format of the decode path, as plain torch arithmetic: the definition that
``csrc/kernels/decode_mx4.hip`` is tested against.

A weight ``w [N, K]`` (K % 32 == 0) is stored as OCP MXFP4: e2m1 elements, two per byte, with one
e8m0 power-of-two scale per block of 32 consecutive elements of a row.

* ``codes uint8 [N, K / 2]``: element ``2j`` in bits 0-3 of byte ``j``, element ``2j + 1`` in bits 4-7.
  Bit 3 of a code is the sign, bits 0-2 select ``{0, 0.5, 1, 1.5, 2, 3, 4, 6}``.
* ``scales uint8 [N, K / 32]``: the value ``2^(e - 127)``.
* The block scale is the smallest power of two ``2^p`` with ``amax <= 6 * 2^p`` (``amax`` the block's
  largest ``|w|`` in fp32), so nothing saturates. In integers: ``amax = m 2^ex`` with m in [0.5, 1) gives
  ``p = ex - 3`` if ``m <= 0.75``, else ``ex - 2``. ``e = clamp(p + 127, 1, 254)``; the codes are taken
  with the clamped scale.
* ``code = e2m1_rne(fp32(w) * 2^-(e - 127))``: the product is exact, and it is rounded to the nearest
  value, a tie to the even code.
* An all-zero block has ``e = 127`` and codes that keep each weight's sign bit (0x0 / 0x8).
* A block that holds a non-finite weight has the scale byte 0xFF and zero codes; every output whose
  weight row contains such a block is NaN.

``dequant(codes, scales)`` is the float64 value ``code * scale`` the products are sums over.
"""
from __future__ import annotations

from typing import Tuple

import torch

BLOCK = 32
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def e2m1_rne(v: torch.Tensor) -> torch.Tensor:
    """Finite fp32 values to e2m1 codes (int64 in [0, 15]), round to nearest, ties to the even code;
    magnitudes above 6 give the code of 6."""
    a = v.double().abs()
    _, ex = torch.frexp(a)  # a = m 2^ex, m in [0.5, 1)
    e = (ex - 1).clamp(min=0, max=2)  # below 1 the values share the spacing of [1, 2)
    q = torch.round(torch.ldexp(a, 1 - e)).to(e.dtype)  # half to even; below 1: the code itself
    code = torch.where(a < 1, q, 2 * e + q).clamp(max=7)  # q = 4 carries into the next exponent
    return code + 8 * torch.signbit(v).to(code.dtype)


def quantize_rows(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(codes uint8 [N, K / 2], scales uint8 [N, K / 32])`` of ``w [N, K]`` (any float dtype; the values
    are taken to fp32 first, exactly for bf16 and fp16)."""
    if w.dim() != 2 or w.shape[1] == 0 or w.shape[1] % BLOCK:
        raise ValueError(f"mxfp4.quantize_rows: w [N, K] with K a positive multiple of {BLOCK}, got {tuple(w.shape)}")
    n, k = w.shape
    f = w.detach().float().view(n, k // BLOCK, BLOCK)
    amax = f.abs().amax(dim=2)  # propagates NaN
    finite = torch.isfinite(amax)
    m, ex = torch.frexp(torch.where(finite, amax, torch.ones_like(amax)))
    p = torch.where(m <= 0.75, ex - 3, ex - 2)
    e = torch.where(amax == 0, torch.full_like(p, 127), (p + 127).clamp(1, 254))
    v = torch.ldexp(f.double(), (127 - e)[:, :, None]).float()  # exact: a power-of-two factor
    c = e2m1_rne(torch.where(finite[:, :, None], v, torch.zeros_like(v)))
    c = torch.where(finite[:, :, None], c, torch.zeros_like(c)).view(n, k // 2, 2)
    codes = (c[:, :, 0] | (c[:, :, 1] << 4)).to(torch.uint8)
    scales = torch.where(finite, e, torch.full_like(e, 255)).to(torch.uint8)
    return codes, scales


def decode(codes: torch.Tensor) -> torch.Tensor:
    """The e2m1 values of ``codes [N, K / 2]`` as float64 ``[N, K]``, on their device."""
    table = torch.tensor(E2M1_VALUES + tuple(-x for x in E2M1_VALUES), dtype=torch.float64, device=codes.device)
    c = codes.long()
    return table[torch.stack((c & 15, c >> 4), dim=-1)].view(codes.shape[0], -1)


def dequant(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """float64 ``code * 2^(e - 127)``, block by block; NaN throughout a block whose scale byte is 0xFF."""
    e = scales.long()
    s = torch.ldexp(torch.ones_like(e, dtype=torch.float64), e - 127)
    s = torch.where(e == 255, torch.full_like(s, float("nan")), s)
    return decode(codes) * s.repeat_interleave(BLOCK, dim=1)
