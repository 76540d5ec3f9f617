#!/usr/bin/env python
"""What held-out evaluation (--eval-every) costs, measured in one process on one GPU.

For a model preset (default Llama-3-8B, seq 2048, batch 1, bf16):

* one evaluation micro-batch (``Transformer.evaluate``): median of several after warm-up,
  timed with events on the stream;
* one full training step (forward, backward, clip, AdamW), the same way;
* ``xent_eval_`` against ``xent_fwd`` on the same [2048, 131072] bf16 logits;
* peak allocated memory of a training loop without and with evaluations between its steps.

Each phase runs under its own time limit (a watchdog ends the process with status 124), and
the first failure ends the script. The report is printed as markdown (``--out`` also writes it
to a file); ``profiles/eval.md`` holds one run of it.

    python scripts/eval_bench.py [--model llama3-8b] [--out report.md]
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import statistics
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


@contextlib.contextmanager
def phase(name: str, limit_s: float):
    """Run one phase under a time limit: a GPU call that never returns cannot be interrupted from
    Python, so the watchdog ends the whole process."""
    def expire():
        print(f"[eval_bench] phase {name!r} exceeded its {limit_s:.0f}s limit", flush=True)
        os._exit(124)

    t = threading.Timer(limit_s, expire)
    t.daemon = True
    t.start()
    print(f"[eval_bench] {name} ...", flush=True)
    try:
        yield
        torch.cuda.synchronize()
    finally:
        t.cancel()


def timed(fn, n: int, warmup: int):
    """Per-call GPU milliseconds of ``fn`` (events on the current stream), after ``warmup`` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    evs[0].record()
    for i in range(n):
        fn()
        evs[i + 1].record()
    torch.cuda.synchronize()
    return [evs[i].elapsed_time(evs[i + 1]) for i in range(n)]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--seq-len", type=int, default=2048)
    ap.add_argument("--batch-size", type=int, default=1)
    ap.add_argument("--vocab-size", type=int, default=131072)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=float, default=180.0, help="time limit of each phase, seconds")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    from fault_tolerant_llm_training_amd._native import kernels
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for
    from fault_tolerant_llm_training_amd.optim.adamw import FlatAdamW
    from fault_tolerant_llm_training_amd.parallel.ddp import GradReducer

    K = kernels()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, S, V = a.batch_size, a.seq_len, a.vocab_size
    res = {"model": a.model, "seq_len": S, "batch_size": B, "vocab": V, "device": torch.cuda.get_device_name(dev)}

    with phase("setup", a.limit):
        model = build_model(model_args_for(a.model, vocab_size=V, seq_len=S), dev, torch.bfloat16, seed=1234)
        red = GradReducer(model.flat, model.sinks_in_backward_order())
        opt = FlatAdamW(model.parameters(), model.flat, lr=5e-5, max_grad_norm=1.0, reducer=red)
        model.gate = opt.gate
        g = torch.Generator().manual_seed(0)
        tok = torch.randint(0, V, (B, S), generator=g).to(dev)
        lab = torch.randint(0, V, (B, S), generator=g).to(dev)
        inv = torch.full((1,), 1.0 / (B * S), dtype=torch.float32, device=dev)
        acc = torch.zeros(4, dtype=torch.int64, device=dev)

    def train_step():
        loss = model(tok, lab, inv)
        loss.backward()
        red.finish()
        opt.clip_grad_norm_(1.0)
        opt.step()

    def eval_mb():
        model.evaluate(tok, lab, acc)

    with phase("training step", a.limit):
        ts = timed(train_step, a.iters, a.warmup)
        res["train_step_ms"] = statistics.median(ts)
        res["train_step_ms_all"] = [round(t, 3) for t in ts]
    with phase("evaluation micro-batch", a.limit):
        opt.gate.wait_all()
        es = timed(eval_mb, a.iters, a.warmup)
        res["eval_microbatch_ms"] = statistics.median(es)
        res["eval_microbatch_ms_all"] = [round(t, 3) for t in es]
        res["eval_over_step"] = res["eval_microbatch_ms"] / res["train_step_ms"]

    with phase("peak memory, training only", a.limit):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        for _ in range(4):
            train_step()
        torch.cuda.synchronize()
        res["peak_train_GiB"] = torch.cuda.max_memory_allocated(dev) / 2**30
    with phase("peak memory, training with evaluations", a.limit):
        torch.cuda.reset_peak_memory_stats(dev)
        for _ in range(4):
            train_step()
            eval_mb()
            eval_mb()
        torch.cuda.synchronize()
        res["peak_train_eval_GiB"] = torch.cuda.max_memory_allocated(dev) / 2**30
    with phase("peak memory, evaluation alone", a.limit):
        opt.gate.wait_all()
        torch.cuda.synchronize()
        res["resident_GiB"] = torch.cuda.memory_allocated(dev) / 2**30
        torch.cuda.reset_peak_memory_stats(dev)
        eval_mb()
        torch.cuda.synchronize()
        res["peak_eval_GiB"] = torch.cuda.max_memory_allocated(dev) / 2**30

    with phase("xent_eval_ against xent_fwd", a.limit):
        T = 2048
        gg = torch.Generator(device=dev).manual_seed(1)
        logits = (3 * torch.randn(T, V, device=dev, generator=gg)).bfloat16()
        labels = torch.randint(0, V, (T,), device=dev)
        kacc = torch.zeros(4, dtype=torch.int64, device=dev)
        n = max(20, a.iters)
        fwd = timed(lambda: K.xent_fwd(logits, labels, -100), n, 5)
        ev = timed(lambda: K.xent_eval_(logits, labels, kacc, -100), n, 5)
        res["xent_fwd_us"] = statistics.median(fwd) * 1e3
        res["xent_eval_us"] = statistics.median(ev) * 1e3
        res["xent_eval_over_fwd"] = res["xent_eval_us"] / res["xent_fwd_us"]
        res["xent_logits_GB_s_eval"] = T * V * 2 / (statistics.median(ev) * 1e-3) / 1e9

    lines = [
        f"Model {res['model']}, seq {S}, batch {B}, vocab {V}, bf16, one {res['device']}; medians of {a.iters} "
        f"after {a.warmup} warm-up calls, events on the stream, one process.",
        "",
        "| measurement | value |",
        "|---|---|",
        f"| training step | {res['train_step_ms']:.2f} ms |",
        f"| evaluation micro-batch (`Transformer.evaluate`) | {res['eval_microbatch_ms']:.2f} ms |",
        f"| evaluation micro-batch / training step | {res['eval_over_step']:.3f} |",
        f"| `xent_fwd`, 2048 x {V} bf16 logits | {res['xent_fwd_us']:.1f} us |",
        f"| `xent_eval_`, same logits | {res['xent_eval_us']:.1f} us "
        f"({res['xent_logits_GB_s_eval']:.0f} GB/s of logits) |",
        f"| `xent_eval_` / `xent_fwd` | {res['xent_eval_over_fwd']:.3f} |",
        f"| peak allocated, 4 training steps | {res['peak_train_GiB']:.2f} GiB |",
        f"| peak allocated, 4 training steps with 2 evaluation micro-batches after each | "
        f"{res['peak_train_eval_GiB']:.2f} GiB |",
        f"| resident (parameters, gradients, moments) | {res['resident_GiB']:.2f} GiB |",
        f"| peak allocated during one evaluation micro-batch alone | {res['peak_eval_GiB']:.2f} GiB |",
        "",
        "```json",
        json.dumps(res),
        "```",
    ]
    report = "\n".join(lines)
    print(report, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(report + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
