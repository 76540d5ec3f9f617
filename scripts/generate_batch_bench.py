"""Batched-decode measurements on one MI355X (record: profiles/generate_batch.md). The protocol is
that of scripts/generate_bench.py: alternating rounds in one process, HIP event times, every call of a
round on the next of several copies of the weight (together at least 1 GB), so the rates are HBM rates.

1. ``gemv_rows`` / ``gemv_swiglu_rows`` on the five Llama-3-8B products at R = 1, 2, 4, 8, 16 activation
   rows, beside ``gemv`` / ``gemv_swiglu`` (one row, the kernel the one-sequence path runs) and beside
   ``torch.nn.functional.linear(X[R, K], W)`` on the same operands. Rates are weight bytes over time.
2. Llama-3-8B ``decode_step_rows`` milliseconds per step and aggregate tokens per second at B = 1, 2, 4,
   8, 16 with 128 cached keys per row, beside ``decode_step`` (one sequence).

    python scripts/generate_batch_bench.py [--rounds 7] [--skip-model]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fault_tolerant_llm_training_amd._native import kernels  # noqa: E402

PRODUCTS = [("wqkv", 6144, 4096, False), ("wo", 4096, 4096, False), ("w13+swiglu", 28672, 4096, True),
            ("w2", 4096, 14336, False), ("head", 131072, 4096, False)]
ROWS = [1, 2, 4, 8, 16]
CACHE_BYTES = 1 << 30  # copies of a weight cycled through: 4x the 256 MB last-level cache


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def summary(ts, nbytes):
    med = statistics.median(ts)
    return {"median_us": med * 1e6, "min_us": min(ts) * 1e6, "max_us": max(ts) * 1e6, "median_gbps": nbytes / med / 1e9}


def bench_products(rounds):
    k = kernels()
    dev = torch.device("cuda:0")
    out = {}
    for name, N, K, swiglu in PRODUCTS:
        nbytes = N * K * 2
        copies = max(2, -(-CACHE_BYTES // nbytes))
        ws = [(torch.randn(N, K, device=dev) * 0.02).bfloat16() for _ in range(copies)]
        xs = {R: torch.randn(R, K, device=dev).bfloat16() for R in ROWS}
        one = k.gemv_swiglu if swiglu else (lambda x, w: k.gemv(x, w, None))
        rows = k.gemv_swiglu_rows if swiglu else (lambda x, w: k.gemv_rows(x, w, None))
        arms = {"gemv": lambda: [one(xs[1][0], w) for w in ws]}
        for R in ROWS:
            arms[f"gemv_rows R={R}"] = lambda R=R: [rows(xs[R], w) for w in ws]
            arms[f"F.linear R={R}"] = lambda R=R: [F.linear(xs[R], w) for w in ws]
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
        times = {a: [] for a in arms}
        for _ in range(rounds):
            for a, fn in arms.items():
                times[a].append(timed(fn) / copies)
        same = all(torch.equal(rows(xs[R], ws[0]), torch.stack([one(xs[R][r], ws[0]) for r in range(R)])) for R in ROWS)
        out[name] = {"N": N, "K": K, "mbytes": nbytes / 1e6, "copies": copies, "rows_equal_one_row_bitwise": same,
                     **{a: summary(ts, nbytes) for a, ts in times.items()}}
        del ws
        torch.cuda.empty_cache()
    return out


def bench_model(rounds):
    from fault_tolerant_llm_training_amd import generation
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    dev = torch.device("cuda:0")
    margs = model_args_for("llama3-8b", vocab_size=131072, seq_len=4096)
    model = build_model(margs, dev, torch.bfloat16)
    n_keys, steps = 128, 8
    arms = {}
    one = generation.KVCache(margs, n_keys + steps + 1, dev, torch.bfloat16)
    one.k.normal_()
    one.v.normal_()

    def run_one():
        one.length = n_keys
        for _ in range(steps):
            generation.decode_step(model, 5, one)

    arms["decode_step"] = run_one
    for B in ROWS:
        cache = generation.BatchKVCache(margs, B, n_keys + steps + 1, dev, torch.bfloat16)
        cache.k.normal_()
        cache.v.normal_()
        for b in range(B):
            cache.set_length(b, n_keys)
        tok = torch.full((B,), 5, dtype=torch.int64, device=dev)

        def run_rows(cache=cache, tok=tok):
            cache.steps = 0
            for t in range(steps):
                generation.decode_step_rows(model, tok, cache, t)

        arms[f"decode_step_rows B={B}"] = run_rows
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    times = {a: [] for a in arms}
    for _ in range(rounds):
        for a, fn in arms.items():
            times[a].append(timed(fn) / steps)
    out = {"cached_keys": n_keys, "steps_per_window": steps}
    for a, ts in times.items():
        B = int(a.split("=")[1]) if "=" in a else 1
        med = statistics.median(ts)
        out[a] = {"ms_per_step": med * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3, "tokens_per_s": B / med}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-products", action="store_true")
    a = ap.parse_args()
    out = {"rounds": a.rounds}
    if not a.skip_products:
        out["products"] = bench_products(a.rounds)
    if not a.skip_model:
        out["llama3_8b"] = bench_model(a.rounds)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
