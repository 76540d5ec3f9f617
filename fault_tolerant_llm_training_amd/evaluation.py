"""Held-out evaluation during training (``--eval-every``).

The reference has no evaluation: its ``train.py`` logs the loss of the batch it just trained on
and nothing else. Here a fixed set of ``--eval-sequences`` sequences is evaluated at step
boundaries with a forward-only pass (``Transformer.evaluate``) that leaves the training state
untouched bit for bit, and summed in integers so the result is reproducible:

* the set is the same ``M`` sequences at every evaluation, independent of the training
  loader's position and not part of any checkpoint. It is prepared once, pinned on the host;
* micro-batches are ``--batch-size`` sequences (the shape of a training micro-batch, so every
  GEMM takes the plan it takes in training); micro-batch ``i`` runs on rank ``i % W``;
* the forward issues no collective. Each rank accumulates four int64 counters on its device
  (``utils/evalacc.py``: fixed-point NLL sum, tokens, top-1 hits, rows left out); at the end
  they are summed over the control (gloo) group. Integer sums do not depend on order, so the
  record is identical for every number of ranks, head chunking and micro-batch order;
* between micro-batches every rank takes a short vote (signal, error). If any rank has either,
  all ranks abandon the evaluation together and emit nothing: the caller stops through its
  normal path, the checkpoint is at this same step, and the resumed job runs the evaluation
  again. An interrupted evaluation is never half-reported.
"""
from __future__ import annotations

import collections
import time
from typing import Callable, List, Optional, Tuple

import torch

from .parallel import dist as fdist
from .utils.evalacc import summarize

# SyntheticTokens draws sample g from the generator seed ``seed * 1_000_003 + g``; the held-out set
# uses ``seed + 2^40``, whose samples lie 2^40 * 1_000_003 generator seeds away from the training
# stream's: no training run reaches them
SYNTHETIC_SEED_OFFSET = 1 << 40
MAX_AHEAD = 2  # evaluation micro-batches the host may enqueue ahead of the GPU


def should_evaluate(step: int, every: int) -> bool:
    """An evaluation is due at the boundary before ``step``."""
    return every > 0 and step > 0 and step % every == 0


class EvalSet:
    """The fixed evaluation set of one rank: its micro-batches ``i % W == rank`` of the ``M / B``
    micro-batches, as (inputs, labels) int64 [B, S] host tensors (pinned for a GPU run)."""

    def __init__(self, batches: List[Tuple[torch.Tensor, torch.Tensor]], rounds: int, sequences: int,
                 seq_len: int, source: str):
        self.batches = batches
        self.rounds = rounds  # micro-batches of the busiest rank = votes every rank takes
        self.sequences = sequences
        self.seq_len = seq_len
        self.source = source

    def describe(self, every: int) -> str:
        return (f"Evaluation set: {self.source} | {self.sequences} sequences of {self.seq_len} | "
                f"{self.sequences * self.seq_len} tokens | every {every} steps and after the last step")


def _synthetic_batches(args, vocab: int, mine):
    from .data.synthetic import SyntheticTokens

    ds = SyntheticTokens(vocab, args.sequence_length, seed=args.seed + SYNTHETIC_SEED_OFFSET, pin=False)
    return [ds.batch(i, args.batch_size) for i in mine], f"synthetic (seed {args.seed} + 2^40)"


def _parquet_batches(args, n_mb: int, mine):
    from .data.parquet import CollatorForCLM, IterableParquetDataset, ParquetDataset
    from .data.tokenizer import load_tokenizer, pad_token_id

    tok = load_tokenizer(args.tokenizer_name_or_path)
    B, S = args.batch_size, args.sequence_length
    if args.iterable_dataset:
        # the packing dataset has no random access: every rank packs the whole set from the first
        # document and keeps its own micro-batches
        bos = getattr(tok, "bos_token_id", None)
        it = iter(IterableParquetDataset(args.eval_dataset, tok, S, bos_token_id=1 if bos is None else int(bos)))
        keep = set(mine)
        out = []
        for i in range(n_mb):
            xs, ys = zip(*(next(it) for _ in range(B)))
            if i in keep:
                out.append((torch.stack(xs), torch.stack(ys)))
        return out, f"{args.eval_dataset} (packed)"
    ds = ParquetDataset(args.eval_dataset, tok, S, n_mb * B)
    coll = CollatorForCLM(S, pad_token_id(tok))
    return [coll([ds[i * B + j] for j in range(B)]) for i in mine], str(args.eval_dataset)


def build_eval_set(args, vocab: int, rank: int, world: int, pin: bool) -> EvalSet:
    """This rank's share of the evaluation set, read from the beginning of its source."""
    B, M = args.batch_size, args.eval_sequences
    if M <= 0 or M % B:
        raise ValueError(f"--eval-sequences ({M}) must be a positive multiple of --batch-size ({B})")
    n_mb = M // B
    mine = [i for i in range(n_mb) if i % world == rank]
    if args.eval_dataset:
        batches, source = _parquet_batches(args, n_mb, mine)
    elif args.synthetic_data:
        batches, source = _synthetic_batches(args, vocab, mine)
    else:
        raise ValueError("--eval-every needs --eval-dataset (or --synthetic-data)")
    if pin:
        batches = [(x.pin_memory(), y.pin_memory()) for x, y in batches]
    return EvalSet(batches, -(-n_mb // world), M, args.sequence_length, source)


def run_evaluation(model, eval_set: EvalSet, device: torch.device, group=None,
                   pending_signal: Callable[[], int] = lambda: 0, has_error: Callable[[], bool] = lambda: False):
    """One evaluation of ``eval_set`` with ``model`` (every rank calls it at the same boundary).

    Returns ``(summary, error)``: ``summary`` is the dict of :func:`utils.evalacc.summarize` plus
    ``seconds``, the same on every rank, or None when the ranks abandoned the evaluation (a signal
    or an error on any rank); ``error`` is this rank's own exception, if it had one. ``group``:
    the gloo group the counters are summed over (None: one rank)."""
    t0 = time.perf_counter()
    acc =torch.zeros(4, dtype=torch.int64, device=device)
    error: Optional[BaseException] = None
    inflight = collections.deque()
    cuda = device.type == "cuda"
    for r in range(eval_set.rounds):
        if r < len(eval_set.batches) and error is None:
            try:
                x, y = eval_set.batches[r]
                model.evaluate(x.to(device, non_blocking=True), y.to(device, non_blocking=True), acc)
                if cuda:  # bound the host's run-ahead: a stop never waits for a queue of micro-batches
                    ev = torch.cuda.Event()
                    ev.record()
                    inflight.append(ev)
                    while len(inflight) > MAX_AHEAD:
                        inflight.popleft().synchronize()
            except Exception as e:  # noqa: BLE001 - becomes this rank's vote; the caller stops with it
                error = e
        # after every round, the last included: the boundary's vote with the signal and error
        # columns only (every rank takes `rounds` votes, whatever its share of the micro-batches)
        table = fdist.vote([float(pending_signal()), 1.0 if (error is not None or has_error()) else 0.0])
        if table.max() > 0:
            return None, error
    total = acc.cpu()  # waits for this rank's micro-batches
    if group is not None:
        torch.distributed.all_reduce(total, group=group)
    out = summarize(total.tolist())
    out["seconds"] = time.perf_counter() - t0
    return out, None


def metrics_record(step: int, s: dict, ema: Optional[dict] = None) -> dict:
    """``ema``: the summary of the same set on the averaged weights (--eval-ema), added as ``ema_*``
    fields; the other fields are those of a record without it."""
    rec = {"eval_step": step, "eval_loss": s["loss"], "eval_loss_fx": s["loss_fx"], "eval_tokens": s["tokens"],
           "eval_correct": s["correct"], "eval_nonfinite": s["nonfinite"], "eval_s": s["seconds"]}
    if ema is not None:
        rec.update(ema_loss=ema["loss"], ema_loss_fx=ema["loss_fx"], ema_perplexity=ema["perplexity"],
                   ema_accuracy=ema["accuracy"], ema_correct=ema["correct"], ema_nonfinite=ema["nonfinite"],
                   ema_s=ema["seconds"])
    return rec


def log_line(step: int, s: dict, ema: Optional[dict] = None) -> str:
    line = (f"Evaluation at step {step} | Loss: {s['loss']:.4f} | Perplexity: {s['perplexity']:.2f} | "
            f"Accuracy: {s['accuracy']:.4f} | Tokens: {s['tokens']} | {s['seconds']:.2f}s")
    if s["nonfinite"]:
        line += f" | Non-finite rows left out: {s['nonfinite']}"
    if ema is not None:
        line += (f" | ema_loss: {ema['loss']:.4f} | ema_perplexity: {ema['perplexity']:.2f} | "
                 f"ema_accuracy: {ema['accuracy']:.4f} | ema_s: {ema['seconds']:.2f}")
        if ema["nonfinite"]:
            line += f" | ema_nonfinite: {ema['nonfinite']}"
    return line
