"""Decode-path measurements on one MI355X (record: profiles/generate.md).

1. ``gemv`` / ``gemv_swiglu`` on the five Llama-3-8B one-row products, in GB/s of weight bytes,
   beside ``torch.nn.functional.linear`` on the same operands (the path a one-row product takes
   without these kernels) and beside ``sumsq_into_`` over the same bytes (the project's stream-rate
   yardstick). Alternating rounds in one process, HIP event times. Every call of a round works on
   the next of several copies of the weight (together more than the 256 MB last-level cache), so
   the figure is an HBM rate.
2. Llama-3-8B decode milliseconds per token at 128 and 2048 cached keys, beside the floor
   (parameter bytes over the measured stream rate) and the share of the time outside the gemv
   kernels (a step against the same step's gemv calls alone).
3. One ``--sample-every`` boundary: ``generate`` of 64 tokens from a one-token prompt.

    python scripts/generate_bench.py [--rounds 7] [--skip-model]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fault_tolerant_llm_training_amd._native import kernels  # noqa: E402

PRODUCTS = [("wqkv", 6144, 4096, False), ("wo", 4096, 4096, False), ("w13+swiglu", 28672, 4096, True),
            ("w2", 4096, 14336, False), ("head", 131072, 4096, False)]
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
    return {"median_us": med * 1e6, "min_us": min(ts) * 1e6, "max_us": max(ts) * 1e6,
            "median_gbps": nbytes / med / 1e9, "best_gbps": nbytes / min(ts) / 1e9, "worst_gbps": nbytes / max(ts) / 1e9}


def bench_products(rounds):
    k = kernels()
    dev = torch.device("cuda:0")
    out = {}
    partial = torch.empty(4096, dtype=torch.float32, device=dev)
    for name, N, K, swiglu in PRODUCTS:
        nbytes = N * K * 2
        copies = max(2, -(-CACHE_BYTES // nbytes))
        ws = [(torch.randn(N, K, device=dev) * 0.02).bfloat16() for _ in range(copies)]
        x = torch.randn(K, device=dev).bfloat16()
        x2 = x.view(1, K)
        arms = {
            "gemv": (lambda: [k.gemv_swiglu(x, w) for w in ws]) if swiglu else (lambda: [k.gemv(x, w, None) for w in ws]),
            "F.linear": lambda: [F.linear(x2, w) for w in ws],
            "sumsq_into_": lambda: [k.sumsq_into_(w.view(-1), partial) for w in ws],
        }
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
        times = {a: [] for a in arms}
        for _ in range(rounds):
            for a, fn in arms.items():
                times[a].append(timed(fn) / copies)
        y = k.gemv(x, ws[0], None).float()
        ref = F.linear(x2, ws[0]).float().view(-1)
        out[name] = {"N": N, "K": K, "mbytes": nbytes / 1e6, "copies": copies,
                     "rel_diff_vs_linear": float((y - ref).norm() / ref.norm()),
                     **{a: summary(ts, nbytes) for a, ts in times.items()}}
        del ws
        torch.cuda.empty_cache()
    return out


def bench_model(rounds):
    from fault_tolerant_llm_training_amd import generation
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for
    from fault_tolerant_llm_training_amd.ops import decode as D

    k = kernels()
    dev = torch.device("cuda:0")
    margs = model_args_for("llama3-8b", vocab_size=131072, seq_len=4096)
    model = build_model(margs, dev, torch.bfloat16)
    flat = model.flat.params
    nbytes = flat.numel() * 2
    partial = torch.empty(8192, dtype=torch.float32, device=dev)
    k.sumsq_into_(flat, partial)
    stream = [timed(lambda: k.sumsq_into_(flat, partial)) for _ in range(rounds)]
    rate = nbytes / statistics.median(stream)
    out = {"param_gbytes": nbytes / 1e9, "stream_tbps": rate / 1e12, "floor_ms": nbytes / rate * 1e3}

    def gemv_only():  # the gemv calls of one decode step, on the step's weights
        x = torch.zeros(margs.dim, dtype=torch.bfloat16, device=dev)
        xf = torch.zeros(margs.ffn_hidden, dtype=torch.bfloat16, device=dev)
        for layer in model.layers.values():
            at, ff = layer.attention, layer.feed_forward
            D.gemv(x, at.wqkv)
            D.gemv(x, at.wo.weight)
            D.gemv_swiglu(x, ff.w13)
            D.gemv(xf, ff.w2.weight)
        D.gemv(x, model.output.weight)

    steps = 8
    for n_keys in (128, 2048):
        cache = generation.KVCache(margs, n_keys + steps * (rounds + 1) + 1, dev, torch.bfloat16)
        cache.k.normal_()
        cache.v.normal_()
        cache.length = n_keys

        def run():
            for _ in range(steps):
                generation.decode_step(model, 5, cache)

        run()  # warm-up (also of every code object)
        gemv_only()
        torch.cuda.synchronize()
        ts, tg = [], []
        for _ in range(rounds):
            cache.length = n_keys
            ts.append(timed(run) / steps)
            tg.append(timed(lambda: [gemv_only() for _ in range(steps)]) / steps)
        ms, mg = statistics.median(ts) * 1e3, statistics.median(tg) * 1e3
        out[f"keys_{n_keys}"] = {"ms_per_token": ms, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3,
                                 "gemv_only_ms": mg, "share_outside_gemv": 1.0 - mg / ms,
                                 "over_floor": ms / out["floor_ms"]}
        del cache
    # one --sample-every boundary with the defaults: BOS alone, 64 tokens, greedy
    generation.generate(model, [1], 8)
    torch.cuda.synchronize()
    tb = []
    for _ in range(3):
        t0 = time.perf_counter()
        ids = generation.generate(model, [1], 64)
        tb.append(time.perf_counter() - t0)  # generate returns host integers: the device is done
    out["sample_boundary_64_tokens_s"] = {"median": statistics.median(tb), "min": min(tb), "max": max(tb),
                                          "tokens": len(ids)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    out = {"rounds": a.rounds, "products": bench_products(a.rounds)}
    if not a.skip_model:
        out["llama3_8b"] = bench_model(a.rounds)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
