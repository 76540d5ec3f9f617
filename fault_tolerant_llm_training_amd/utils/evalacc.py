"""Evaluation counters in pure PyTorch: the definition the ``xent_eval_`` kernel implements.

Four int64 counters are accumulated over token rows::

    acc[0] += fx = round(nll * 2^24)   fixed-point NLL (fp32 product, exact; round to nearest even)
    acc[1] += 1                        tokens
    acc[2] += hit                      the label is the LOWEST column that attains the row maximum
    acc[3] += 1                        rows left out of acc[0..2]: NLL not finite or |nll| >= 2^38
                                       (fx would not fit), or a label outside [0, V)

Rows with ``label == ignore_index`` add nothing. Integer sums are exact and independent of
order, so the totals do not depend on chunking, micro-batch order or the number of ranks.
This is the ``--device cpu`` / fp64 path of evaluation (``csrc/kernels/xent_eval.hip`` on the
GPU) and the structure the GPU tests compare the kernel with.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

FX_BITS = 24
FX_ONE = float(1 << FX_BITS)
NLL_LIMIT = float(1 << 38)
IGNORE_INDEX = -100


def row_counters(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = IGNORE_INDEX):
    """Per-row (fx int64, counted bool, hit bool, left_out bool) of ``logits`` [T, V], ``labels`` [T]."""
    V = logits.shape[-1]
    lf = logits.reshape(-1, V).float()
    lab = labels.reshape(-1)
    live = lab != ignore_index
    in_range = live & (lab >= 0) & (lab < V)
    safe = torch.where(in_range, lab, torch.zeros_like(lab))
    nll = F.cross_entropy(lf, safe, reduction="none")
    counted = in_range & (nll.abs() < NLL_LIMIT)  # false for NaN / inf too
    fx = torch.round(torch.where(counted, nll, torch.zeros_like(nll)) * FX_ONE).to(torch.int64)
    first = lf.argmax(dim=-1)  # torch.argmax returns the first index of the maximum
    hit = counted & (first == safe)
    return fx, counted, hit, live & ~counted


def xent_eval_reference_(logits: torch.Tensor, labels: torch.Tensor, acc: torch.Tensor,
                         ignore_index: int = IGNORE_INDEX) -> torch.Tensor:
    """``acc`` (int64 [4]) += the counters of these rows. Returns ``acc``."""
    fx, counted, hit, left = row_counters(logits, labels, ignore_index)
    add = torch.stack([fx[counted].sum(), counted.sum(), hit.sum(), left.sum()]).to(torch.int64)
    acc.add_(add.to(acc.device))
    return acc


def summarize(acc) -> dict:
    """Loss (float64 from the integer), perplexity and accuracy of four summed counters."""
    fx, tokens, correct, nonfinite = (int(v) for v in acc)
    loss = fx / FX_ONE / tokens if tokens else float("nan")
    try:
        ppl = math.exp(loss)
    except OverflowError:
        ppl = float("inf")
    return {"loss": loss, "perplexity": ppl, "accuracy": (correct / tokens) if tokens else float("nan"),
            "loss_fx": fx, "tokens": tokens, "correct": correct, "nonfinite": nonfinite}
