"""Exponential moving average of the parameters (``--ema-decay``): the definition.

Absent in the reference. One update of one element with parameter ``p`` (model dtype, widened
exactly to float32) and average ``e`` (float32)::

    omd  = float32(1 - d_K)        # d_K = decay ** every, in Python float (double), rounded once
    diff = float32(p - e)
    prod = float32(diff * omd)
    e'   = float32(e + prod)

Three separately rounded operations, no fused multiply-add: a numpy float32 loop gives the same
bits, and so does the ``ema_update_`` kernel (csrc/kernels/ema.hip). The average starts as
``float32(p_0)``, so it needs no bias correction. fp64 models keep a float64 average by the same
three operations in float64.

This module is the CPU (and fp64 composed) path of :class:`..optim.adamw.FlatAdamW` and the
oracle of the tests.
"""
from __future__ import annotations

import numpy as np
import torch


def ema_dtype(param_dtype: torch.dtype) -> torch.dtype:
    """Storage dtype of the average: fp32, or fp64 for an fp64 model."""
    return torch.float64 if param_dtype == torch.float64 else torch.float32


def one_minus_decay(decay: float, every: int = 1, dtype: torch.dtype = torch.float32) -> float:
    """``1 - decay ** every`` formed in double and rounded once to the average's dtype, as a
    Python float (exactly representable in that dtype)."""
    omd = 1.0 - float(decay) ** int(every)
    return float(omd) if dtype == torch.float64 else float(np.float32(omd))


def check(decay: float, every: int) -> None:
    if not (0.0 <= float(decay) < 1.0):
        raise ValueError(f"ema_decay must be 0 (off) or in (0, 1), got {decay}")
    if int(every) < 1:
        raise ValueError(f"ema_every must be >= 1, got {every}")


@torch.no_grad()
def ema_update_(ema: torch.Tensor, p: torch.Tensor, omd: float) -> torch.Tensor:
    """In place ``ema += (p - ema) * omd`` by the definition: each of the three operations is one
    PyTorch op and rounds on its own (in ``ema``'s dtype)."""
    diff = torch.sub(p.to(ema.dtype), ema)  # (a new tensor: p.to() is p itself for an fp32 model)
    diff.mul_(omd)
    return ema.add_(diff)


def ema_update_numpy(e: np.ndarray, p: np.ndarray, omd: float) -> np.ndarray:
    """The same update on float32 (or float64) numpy arrays; returns the new average."""
    t = e.dtype.type
    diff = (p.astype(e.dtype) - e).astype(e.dtype)
    prod = (diff * t(omd)).astype(e.dtype)
    return (e + prod).astype(e.dtype)
