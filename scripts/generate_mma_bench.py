"""Matrix-core batched decode measurements on one MI355X (record: profiles/decode_mma.md), after the
protocol of scripts/generate_batch_bench.py: alternating rounds in one process, HIP event times, every
call of a round on the next of several copies of the weight (together more than the 256 MB last-level
cache), medians with the spread.

1. The five Llama-3-8B products at R in {1, 4, 8, 16, 32, 64}, bf16 and FP8 weights: ``gemm_rows_mma(_w8)``
   against ``gemv_rows(_w8)`` and ``F.linear`` on the same operands, and the floor: the weight bytes over
   the stream rate of ``sumsq_into_`` measured here.
2. The split factor the ops choose per product and the times of its neighbours (R = 16).
3. Llama-3-8B ms per step at B in {1, 4, 16, 64} with 128 and 2048 cached keys, with and without ``mma``,
   eager (``decode_step_rows``) and replayed (``DecodeGraph``), bf16 and FP8 weights.

    python scripts/generate_mma_bench.py [--rounds 7] [--skip-model] [--skip-products] [--skip-splits]
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
            ("w2", 4096, 14336, False), ("head", 128256, 4096, False)]
CACHE_BYTES = 1 << 30
ROWS = (1, 4, 8, 16, 32, 64)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def summary(ts):
    return {"median_us": statistics.median(ts) * 1e6, "min_us": min(ts) * 1e6, "max_us": max(ts) * 1e6}


def rounds_of(arms, rounds, copies):
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    times = {a: [] for a in arms}
    for _ in range(rounds):
        for a, fn in arms.items():
            times[a].append(timed(fn) / copies)
    return {a: summary(ts) for a, ts in times.items()}


def stream_rate(rounds):
    """Bytes per second of ``sumsq_into_`` over 1 Gi bf16 elements (2 GiB, past every cache)."""
    k = kernels()
    g = torch.zeros(1 << 30, dtype=torch.bfloat16, device="cuda")
    part = torch.zeros(2048, device="cuda")
    k.sumsq_into_(g, part)
    torch.cuda.synchronize()
    return g.numel() * 2 / statistics.median([timed(lambda: k.sumsq_into_(g, part)) for _ in range(rounds)])


def weights_of(N, K):
    k = kernels()
    copies = max(2, -(-CACHE_BYTES // (N * K)))  # sized for the smaller (FP8) arm
    ws = [(torch.randn(N, K, device="cuda") * 0.02).bfloat16() for _ in range(copies)]
    return copies, ws, [k.quantize_rows_e4m3(w) for w in ws]


def bench_products(rounds, rate):
    k = kernels()
    out = {}
    for name, N, K, swiglu in PRODUCTS:
        copies, ws, qs = weights_of(N, K)
        out[name] = {"N": N, "K": K, "copies": copies, "split": int(k.gemm_mma_split(N, K)),
                     "floor_us": {"bf16": 2 * N * K / rate * 1e6, "fp8": N * K / rate * 1e6}}
        for R in ROWS:
            x = torch.randn(R, K, device="cuda").bfloat16()
            if swiglu:
                arms = {"mma": lambda: [k.gemm_swiglu_rows_mma(x, w) for w in ws],
                        "gemv": lambda: [k.gemv_swiglu_rows(x, w) for w in ws],
                        "linear": lambda: [F.linear(x, w) for w in ws],  # without the SwiGLU epilogue
                        "mma_w8": lambda: [k.gemm_swiglu_rows_mma_w8(x, c, s) for c, s in qs],
                        "gemv_w8": lambda: [k.gemv_swiglu_rows_w8(x, c, s) for c, s in qs]}
            else:
                arms = {"mma": lambda: [k.gemm_rows_mma(x, w, None) for w in ws],
                        "gemv": lambda: [k.gemv_rows(x, w, None) for w in ws],
                        "linear": lambda: [F.linear(x, w) for w in ws],
                        "mma_w8": lambda: [k.gemm_rows_mma_w8(x, c, s, None) for c, s in qs],
                        "gemv_w8": lambda: [k.gemv_rows_w8(x, c, s, None) for c, s in qs]}
            out[name][f"R{R}"] = rounds_of(arms, rounds, copies)
        del ws, qs
        torch.cuda.empty_cache()
    return out


def bench_splits(rounds, R=16):
    k = kernels()
    out = {}
    for name, N, K, swiglu in PRODUCTS:
        copies, ws, qs = weights_of(N, K)
        x = torch.randn(R, K, device="cuda").bfloat16()
        chosen = int(k.gemm_mma_split(N, K))
        arms = {}
        for s in sorted({1, max(1, chosen // 2), max(1, chosen - 1), chosen, chosen + 1, 2 * chosen}):
            if swiglu:
                arms[f"S{s}"] = lambda s=s: [k.gemm_swiglu_rows_mma(x, w, s) for w in ws]
                arms[f"S{s}_w8"] = lambda s=s: [k.gemm_swiglu_rows_mma_w8(x, c, sc, s) for c, sc in qs]
            else:
                arms[f"S{s}"] = lambda s=s: [k.gemm_rows_mma(x, w, None, s) for w in ws]
                arms[f"S{s}_w8"] = lambda s=s: [k.gemm_rows_mma_w8(x, c, sc, None, s) for c, sc in qs]
        out[name] = {"chosen": chosen, "R": R, **rounds_of(arms, rounds, copies)}
        del ws, qs
        torch.cuda.empty_cache()
    return out


def bench_model(rounds):
    from fault_tolerant_llm_training_amd import generation
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    dev = torch.device("cuda:0")
    margs = model_args_for("llama3-8b", vocab_size=128256, seq_len=4096)
    model = build_model(margs, dev, torch.bfloat16)
    w8 = generation.Fp8Weights(model)
    torch.cuda.synchronize()
    out, steps = {}, 8
    for n_keys in (128, 2048):
        for B in (1, 4, 16, 64):
            prompts = [[5] * n_keys] * B
            cap = n_keys + steps + 2
            arms = {}
            for label, w in (("bf16", None), ("fp8", w8)):
                for mma in (False, True):
                    g = generation.DecodeGraph(model, B, cap, w, mma=mma)

                    def graph_run(g=g):
                        for _ in range(steps):
                            g.replay()

                    cache = generation.BatchKVCache(margs, B, cap, dev, torch.bfloat16)
                    tok = torch.full((B,), 5, dtype=torch.int64, device=dev)

                    def eager_run(cache=cache, w=w, mma=mma):
                        for t in range(steps):
                            generation.decode_step_rows(model, tok, cache, t, w, mma=mma)

                    def eager_reset(cache=cache):
                        cache.reset()
                        generation._prefill_rows(model, prompts, cache)

                    tag = f"{label}_{'mma' if mma else 'gemv'}"
                    arms[f"{tag}_graph"] = (lambda g=g: g.begin(prompts, steps + 1), graph_run)
                    arms[f"{tag}_eager"] = (eager_reset, eager_run)
            times = {a: [] for a in arms}
            for r in range(rounds + 1):  # round 0 warms every code object
                for a, (reset, run) in arms.items():
                    reset()
                    torch.cuda.synchronize()
                    t = timed(run) / steps
                    if r:
                        times[a].append(t * 1e3)
            out[f"keys_{n_keys}_B{B}"] = {a: {"ms_per_step": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
                                          for a, ts in times.items()}
            del arms
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-products", action="store_true")
    ap.add_argument("--skip-splits", action="store_true")
    a = ap.parse_args()
    rate = stream_rate(a.rounds)
    out = {"rounds": a.rounds, "stream_tbps": rate / 1e12}
    if not a.skip_products:
        out["products"] = bench_products(a.rounds, rate)
    if not a.skip_splits:
        out["splits"] = bench_splits(a.rounds)
    if not a.skip_model:
        out["llama3_8b"] = bench_model(a.rounds)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
