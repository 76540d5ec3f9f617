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
* ``top_p < 1`` (nucleus sampling) narrows the candidates after top-k: order them by descending
  logit, equal logits by ascending column; the nucleus is the shortest prefix of that order whose
  cumulative weight is ``>= top_p * W``, ``W`` being the candidates' total, and always holds the
  lowest column of the row maximum. The draw is the one above over the nucleus alone (``total`` its
  weight). ``top_p`` counts as the float32 the kernel receives; ``top_p == 1`` is the path without
  it, and greedy stays greedy.
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


def check_top_p(top_p: float) -> float:
    """``top_p`` as the float32 the kernel receives, back in float64; ValueError outside (0, 1] (a value
    that rounds to 0 in float32 included). The one check of every layer that takes a ``top_p``."""
    p = float(top_p)
    if not (0.0 < p <= 1.0) or float(np.float32(p)) == 0.0:
        raise ValueError(f"top_p must be in (0, 1], got {top_p}")
    return float(np.float32(p))


def _nucleus_of(x: np.ndarray, cand: np.ndarray, m: np.ndarray, temperature, top_p: float, dtype):
    """The nucleus of candidates ``cand`` of ``x`` (row maxima ``m``) as boolean [R, V], and its margin
    per row. A prefix of the descending order is a threshold value plus the lowest-column ``n`` of the
    candidates equal to it, so the values alone are sorted."""
    xs = np.where(cand, x, -np.inf)
    sv = torch.sort(torch.from_numpy(np.ascontiguousarray(xs)), dim=1, descending=True).values.numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        ws = np.exp(((sv - m) / dtype(temperature)).astype(dtype)).astype(dtype)
    ws = np.where(np.isnan(ws), dtype(0), ws)
    cs = np.cumsum(ws, axis=1, dtype=dtype)
    W = cs[:, -1:]
    target = (dtype(top_p) * W).astype(dtype)
    idx = np.argmax(cs >= target, axis=1)  # rows where nothing reaches it (W is NaN) give 0: the maximum
    rows = np.arange(x.shape[0])
    vthr = sv[rows, idx].reshape(-1, 1)
    n_tie = (idx + 1 - (sv > vthr).sum(axis=1)).reshape(-1, 1)
    equal = cand & (xs == vthr)
    nuc = cand & ((xs > vthr) | (equal & (np.cumsum(equal, axis=1) <= n_tie)))
    hi = cs[rows, idx].astype(np.float64)
    lo = np.where(idx > 0, cs[rows, np.maximum(idx - 1, 0)], 0).astype(np.float64)
    t = target[:, 0].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = np.minimum(hi - t, t - lo) / W[:, 0].astype(np.float64)
    return nuc, margin


def nucleus(x: np.ndarray, temperature: float, top_k: int, top_p: float) -> np.ndarray:
    """Boolean [R, V]: the columns a row's token is drawn from under ``(temperature, top_k, top_p)``:
    ``candidates(x, top_k)`` narrowed to the nucleus (greedy: the lowest column of the maximum alone)."""
    p = check_top_p(top_p)
    x = np.asarray(x, dtype=np.float64)
    if temperature == 0:
        xs = np.where(np.isnan(x), -np.inf, x)
        out = np.zeros(x.shape, dtype=bool)
        out[np.arange(x.shape[0]), np.argmax(xs, axis=1)] = True
        return out
    cand = candidates(x, top_k)
    if p == 1.0:
        return cand
    m = np.max(np.where(cand, x, -np.inf), axis=1, keepdims=True)
    return _nucleus_of(x, cand, m, temperature, p, np.float64)[0]


def _sample_chunk(x: np.ndarray, temperature: float, top_k: int, u: np.ndarray, dtype, top_p: float = 1.0):
    """``(tokens, draw margin, nucleus margin)`` of the rows of ``x``."""
    if temperature == 0:
        xs = np.where(np.isnan(x), -np.inf, x)
        inf = np.full(x.shape[0], np.inf)
        return np.argmax(xs, axis=1).astype(np.int64), inf, inf
    cand = candidates(x, top_k)
    cols = None
    if 0 < top_k < x.shape[1] and (cand.sum(axis=1) == top_k).all():
        # the same sums over the candidates alone, in column order (the other columns weigh nothing)
        cols = np.nonzero(cand)[1].reshape(x.shape[0], top_k)
        x = np.take_along_axis(x, cols, axis=1)
        cand = np.ones_like(x, dtype=bool)
    x = x.astype(dtype)
    m = np.max(np.where(cand, x, -np.inf), axis=1, keepdims=True)
    nuc_margin = np.full(x.shape[0], np.inf)
    if top_p < 1.0:
        cand, nuc_margin = _nucleus_of(x, cand, m, temperature, top_p, dtype)
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
    return tok, margin, nuc_margin


def sample_reference(logits: torch.Tensor, temperature: float, top_k: int, key: int, step: int,
                     return_margin: bool = False, dtype=np.float64, top_p: float = 1.0,
                     return_nucleus_margin: bool = False):
    """Tokens (int64 tensor [R]) of ``logits`` ([R, V] or [V], any float dtype, any device; the math
    runs on the CPU in ``dtype``, float64 being the definition). ``return_margin``: also the distance
    of every row's ``u * total`` from the nearer of the two cumulative sums around it, relative to
    ``total`` (inf for greedy rows): rows with a margin near zero are the ones a lower-precision
    implementation may legitimately decide the other way. ``top_p`` in (0, 1]: nucleus sampling (1: off);
    the draw margin is then the one on the nucleus, and ``return_nucleus_margin`` appends a third
    result, the distance of ``top_p * W`` from the nearer of the two sorted cumulative sums around it,
    relative to ``W`` (inf when ``top_p == 1`` or the row is greedy): rows where it is near zero may
    legitimately get a nucleus one token longer or shorter."""
    if temperature < 0 or top_k < 0:
        raise ValueError("temperature and top_k must be >= 0")
    top_p = check_top_p(top_p)
    x2 = logits.detach().reshape(-1, logits.shape[-1])
    R, V = x2.shape
    rows_per = max(1, _CHUNK_ELEMS // V)
    toks, margins, nuc_margins = [], [], []
    for r0 in range(0, R, rows_per):
        x = x2[r0 : r0 + rows_per].to("cpu", torch.float64).numpy()
        tok, mar, nmar = _sample_chunk(x, float(temperature), int(top_k), uniforms(key, step, x.shape[0], r0), dtype,
                                       top_p)
        toks.append(tok)
        margins.append(mar)
        nuc_margins.append(nmar)
    out = torch.from_numpy(np.concatenate(toks)) if toks else torch.zeros(0, dtype=torch.int64)
    res = (out,)
    if return_margin:
        res += (np.concatenate(margins),)
    if return_nucleus_margin:
        res += (np.concatenate(nuc_margins),)
    return res if len(res) > 1 else out
