"""Token sampling: the definition, in float64.

One token per row of ``logits [R, V]``, a pure function of ``(logits, temperature, top_k, key, step,
row)``; no generator state lives anywhere. This module is the CPU / fp64 path of
``generation.generate`` and the tests' oracle for the device sampler
(``torch.ops.ftamd.sample_``, csrc/kernels/decode.hip).

* ``temperature == 0``: greedy, the LOWEST column that attains the row maximum (the tie rule of the
  evaluation's top-1, utils/evalacc.py).
* otherwise the candidates are the ``top_k`` largest logits (``top_k == 0``: all ``V`` columns), ties
  at the k-th value going to the lower column; candidate ``i`` weighs
  ``exp((x_i - max) / temperature)``; ``u = (w + 0.5) * 2^-32`` with ``w`` the first word of the
  Philox4x32-6 call of ``utils/sround.py`` on counter ``(row, step, BUF_SAMPLE)`` under ``key``; the
  token is the first candidate, in ascending column order, whose cumulative weight reaches
  ``u * total``.
"""
from __future__ import annotations

import numpy as np
import torch

from .sround import BUF_SAMPLE, philox_words

_CHUNK_ELEMS = 1 << 24  # rows are processed in chunks of about this many float64 logits
_MASK63 = (1 << 63) - 1


def token_key(key: int, t: int) -> int:
    """The sampler key of the ``t``-th new token of a call (63 bits: a signed operator argument).
    ``sample_dev_`` (csrc/kernels/decode.hip) forms the same number on the device."""
    return (int(key) + (int(t) + 1) * 0x9E3779B97F4A7C15) & _MASK63


def uniforms(key: int, step: int, rows: int, row0: int = 0) -> np.ndarray:
    """``u`` of rows ``row0 .. row0 + rows``: float64 in (0, 1)."""
    c = np.arange(rows, dtype=np.uint64) + np.uint64(row0)
    w = philox_words(key, step, BUF_SAMPLE, c)[:, 0]
    return (w.astype(np.float64) + 0.5) * 2.0 ** -32


def candidates(x: np.ndarray, top_k: int) -> np.ndarray:
    """Boolean [R, V]: the ``top_k`` largest values of every row, ties at the k-th value to the
    lower column (``top_k == 0`` or ``>= V``: every column that is not NaN)."""
    R, V = x.shape
    ok = ~np.isnan(x)
    if top_k <= 0 or top_k >= V:
        return ok
    xs = np.where(ok, x, -np.inf)
    kth = np.partition(xs, V - top_k, axis=1)[:, V - top_k : V - top_k + 1]  # the k-th largest value
    above = xs > kth
    equal = xs == kth
    need = top_k - above.sum(axis=1, keepdims=True)
    return ok & (above | (equal & (np.cumsum(equal, axis=1) <= need)))


def _sample_chunk(x: np.ndarray, temperature: float, top_k: int, u: np.ndarray, dtype):
    if temperature == 0:
        xs = np.where(np.isnan(x), -np.inf, x)
        return np.argmax(xs, axis=1).astype(np.int64), np.full(x.shape[0], np.inf)
    cand = candidates(x, top_k)
    cols = None
    if 0 < top_k < x.shape[1] and (cand.sum(axis=1) == top_k).all():
        # the same sums over the candidates alone, in column order (the other columns weigh nothing)
        cols = np.nonzero(cand)[1].reshape(x.shape[0], top_k)
        x = np.take_along_axis(x, cols, axis=1)
        cand = np.ones_like(x, dtype=bool)
    x = x.astype(dtype)
    m = np.max(np.where(cand, x, -np.inf), axis=1, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(cand, np.exp(((x - m) / dtype(temperature)).astype(dtype)), dtype(0)).astype(dtype)
    cum = np.cumsum(w, axis=1, dtype=dtype)
    total = cum[:, -1:]
    target = (u.astype(dtype).reshape(-1, 1) * total).astype(dtype)
    tok = np.argmax(cum >= target, axis=1).astype(np.int64)
    rows = np.arange(x.shape[0])
    hi = cum[rows, tok].astype(np.float64)
    lo = np.where(tok > 0, cum[rows, np.maximum(tok - 1, 0)], 0).astype(np.float64)
    t = target[:, 0].astype(np.float64)
    margin = np.minimum(hi - t, t - lo) / total[:, 0].astype(np.float64)
    if cols is not None:
        tok = cols[rows, tok].astype(np.int64)
    return tok, margin


def sample_reference(logits: torch.Tensor, temperature: float, top_k: int, key: int, step: int,
                     return_margin: bool = False, dtype=np.float64):
    """Tokens (int64 tensor [R]) of ``logits`` ([R, V] or [V], any float dtype, any device; the math
    runs on the CPU in ``dtype``, float64 being the definition). ``return_margin``: also the distance
    of every row's ``u * total`` from the nearer of the two cumulative sums around it, relative to
    ``total`` (inf for greedy rows): rows with a margin near zero are the ones a lower-precision
    implementation may legitimately decide the other way."""
    if temperature < 0 or top_k < 0:
        raise ValueError("temperature and top_k must be >= 0")
    x2 = logits.detach().reshape(-1, logits.shape[-1])
    R, V = x2.shape
    rows_per = max(1, _CHUNK_ELEMS // V)
    toks, margins = [], []
    for r0 in range(0, R, rows_per):
        x = x2[r0 : r0 + rows_per].to("cpu", torch.float64).numpy()
        tok, mar = _sample_chunk(x, float(temperature), int(top_k), uniforms(key, step, x.shape[0], r0), dtype)
        toks.append(tok)
        margins.append(mar)
    out = torch.from_numpy(np.concatenate(toks)) if toks else torch.zeros(0, dtype=torch.int64)
    return (out, np.concatenate(margins)) if return_margin else out
