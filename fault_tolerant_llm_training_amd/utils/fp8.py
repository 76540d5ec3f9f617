"""The weight-only FP8 format of the decode path, as plain torch arithmetic: the definition that
``csrc/kernels/decode_w8.hip`` is tested against.

A weight ``w [N, K]`` is stored as OCP e4m3fn codes (``torch.float8_e4m3fn``: bias 7, 3 mantissa
bits, largest value 448, no infinity), one ``uint8`` per element, with one fp32 scale per output
row:

* ``amax[n] = max_k |w[n, k]|``, in fp32;
* ``inv[n] = 448 / amax[n]`` and ``scale[n] = amax[n] / 448``, IEEE fp32 divisions (``inv`` capped at
  the largest float, which only a row with ``amax < 448 / FLT_MAX`` reaches);
* ``code[n, k] = e4m3_rne(fp32(w[n, k]) * inv[n])``: the product rounded to fp32, then to nearest
  even into e4m3. ``|w * inv| <= 448 (1 + 2^-23)``, which rounds to 448: nothing overflows;
* a row with ``amax == 0`` has ``scale = 1`` and codes that keep the sign bit of each weight
  (0x00 / 0x80);
* a row that holds a non-finite weight (an infinity or a NaN) has a NaN scale and zero codes, so
  every output computed from it is NaN.

``dequant(codes, scale)`` is the float64 value ``code * scale`` the products are sums over.
"""
from __future__ import annotations

from typing import Tuple

import torch

E4M3_MAX = 448.0


def e4m3_rne(v: torch.Tensor) -> torch.Tensor:
    """fp32 values (|v| <= 464, or NaN) to e4m3 codes (uint8), round to nearest even. Values above
    the range and NaN give the NaN code 0x7f."""
    a = v.double().abs()
    _, ex = torch.frexp(a)  # a = m 2^ex, m in [0.5, 1)
    e = torch.where(a > 0, ex - 1, torch.full_like(ex, -6)).clamp(min=-6)  # subnormals share 2^-6's spacing
    q = torch.round(torch.ldexp(a, 3 - e))  # in [0, 16]: half to even; 16 carries into the exponent
    code = (e + 6) * 8 + q.to(e.dtype)
    code = torch.where(torch.isnan(v) | (code > 126), torch.full_like(code, 127), code)
    return (code + 128 * torch.signbit(v).to(code.dtype)).to(torch.uint8)


def quantize_rows(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(codes uint8 [N, K], scale fp32 [N])`` of ``w [N, K]`` (any float dtype; the values are taken
    to fp32 first, exactly for bf16 and fp16)."""
    f = w.detach().float()
    amax = f.abs().amax(dim=1)
    finite = torch.isfinite(amax)  # amax propagates NaN
    zero = amax == 0
    one = torch.ones_like(amax)
    safe = torch.where(finite & ~zero, amax, one)
    # tensor / tensor: one IEEE division (`448 / tensor` would be reciprocal-then-multiply, two roundings)
    inv = torch.where(zero, one, (E4M3_MAX * one / safe).clamp(max=torch.finfo(torch.float32).max))
    scale = torch.where(zero, one, safe / E4M3_MAX)
    scale = torch.where(finite, scale, torch.full_like(scale, float("nan")))
    codes = e4m3_rne(f * inv[:, None])
    codes = torch.where(finite[:, None], codes, torch.zeros_like(codes))
    return codes, scale


_TABLE = None


def decode_table() -> torch.Tensor:
    """The float64 value of each of the 256 codes (NaN for 0x7f and 0xff)."""
    global _TABLE
    if _TABLE is None:
        c = torch.arange(256)
        e, m = (c >> 3) & 15, (c & 7).double()
        mag = torch.where(e == 0, m * 2.0 ** -9, torch.ldexp(1 + m / 8, e - 7))
        mag = torch.where((c & 127) == 127, torch.full_like(mag, float("nan")), mag)
        _TABLE = torch.where(c >= 128, -mag, mag)
    return _TABLE


def decode(codes: torch.Tensor) -> torch.Tensor:
    """The e4m3 values of ``codes`` as float64, on their device."""
    return decode_table().to(codes.device)[codes.long()]


def dequant(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """float64 ``code * scale``, row by row."""
    return decode(codes) * scale.double()[:, None]
