"""The sampler with and without top-p on one MI355X (record: profiles/sample_top_p.md).

1. ``sample_`` at V = 131072 and 50304, bf16, R = 1, 16 and 64 rows, for (temperature, top_k, top_p) =
   (0.8, 0, 1.0), (0.8, 40, 1.0), (0.8, 0, 0.9) and (0.8, 40, 0.9): alternating rounds in one
   process, HIP event times, microseconds per call (median, min, max of the rounds). The top-p arms
   are also given as a ratio to the arm with the same top-k and top_p = 1. ``--no-top-p`` leaves the
   top-p arms out and makes six-argument calls only, which a build from before top-p takes too:
   run it on both builds on one box to compare the top_p = 1 arms (``--root`` names the other tree).
2. Decode milliseconds per token of ``generate_batch(..., graph=True)`` with ``top_p`` 1.0 and 0.9,
   on ``--model`` (default llama3-8b; a smaller preset where the time does not allow it).

    python scripts/sample_top_p_bench.py [--rounds 9] [--model llama3-8b | --skip-model] [--no-top-p] [--root DIR]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ARMS = [("T0.8 k0 p1", 0.8, 0, 1.0), ("T0.8 k40 p1", 0.8, 40, 1.0), ("T0.8 k0 p0.9", 0.8, 0, 0.9),
        ("T0.8 k40 p0.9", 0.8, 40, 0.9)]
SHAPES = [(V, R) for V in (131072, 50304) for R in (1, 16, 64)]
CALLS = 20  # calls per timed round, each on the next of several logits tensors


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def bench_sampler(k, rounds, with_top_p):
    dev = torch.device("cuda:0")
    out = {}
    arms = [a for a in ARMS if with_top_p or a[3] == 1.0]
    for V, R in SHAPES:
        torch.manual_seed(V + R)
        xs = [(2.5 * torch.randn(R, V, device=dev)).bfloat16() for _ in range(4)]
        tok = torch.empty(R, dtype=torch.int64, device=dev)

        def call(temperature, top_k, top_p):
            def run():
                for i in range(CALLS):
                    if top_p == 1.0:  # the six-argument call: also what an older build takes
                        k.sample_(xs[i % 4], tok, temperature, top_k, 0x5EED, i)
                    else:
                        k.sample_(xs[i % 4], tok, temperature, top_k, 0x5EED, i, top_p)
            return run

        fns = {name: call(t, tk, p) for name, t, tk, p in arms}
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        times = {a: [] for a in fns}
        for _ in range(rounds):
            for a, fn in fns.items():
                times[a].append(timed(fn) / CALLS)
        rec = {a: {"median_us": statistics.median(ts) * 1e6, "min_us": min(ts) * 1e6, "max_us": max(ts) * 1e6}
               for a, ts in times.items()}
        if with_top_p:
            for tk in (0, 40):
                rec[f"T0.8 k{tk} p0.9"]["ratio_to_p1"] = (rec[f"T0.8 k{tk} p0.9"]["median_us"]
                                                          / rec[f"T0.8 k{tk} p1"]["median_us"])
        out[f"V{V}_R{R}"] = rec
    return out


def bench_model(name, rounds):
    from fault_tolerant_llm_training_amd import generation
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    dev = torch.device("cuda:0")
    margs = model_args_for(name, vocab_size=131072, seq_len=4096)
    model = build_model(margs, dev, torch.bfloat16)
    n_new, prompts = 64, [[1]]
    g = generation.DecodeGraph(model, 1, 1 + n_new)
    out = {"model": name, "tokens": n_new}
    kw = dict(temperature=0.8, top_k=0, key=0x5EED, step=0)
    for p in (1.0, 0.9):
        g.run(prompts, 8, top_p=p, **kw)
    torch.cuda.synchronize()
    times = {1.0: [], 0.9: []}
    for _ in range(rounds):
        for p in (1.0, 0.9):
            t0 = time.perf_counter()
            ids = g.run(prompts, n_new, top_p=p, **kw)  # returns host integers: the device is done
            times[p].append((time.perf_counter() - t0) / len(ids[0]))
    for p, ts in times.items():
        out[f"top_p_{p:g}"] = {"ms_per_token": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3,
                               "max_ms": max(ts) * 1e3}
    out["extra_ms_per_token"] = out["top_p_0.9"]["ms_per_token"] - out["top_p_1"]["ms_per_token"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--no-top-p", action="store_true", help="only the top_p = 1 arms, as six-argument calls")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the tree whose build is measured (default: this one)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from fault_tolerant_llm_training_amd._native import kernels

    out = {"rounds": a.rounds, "sample_": bench_sampler(kernels(), a.rounds, not a.no_top_p)}
    if not a.skip_model and not a.no_top_p:
        out["decode"] = bench_model(a.model, a.rounds)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
