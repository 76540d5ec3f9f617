"""Graph-replayed decoding against the eager loop on one MI355X (record: profiles/generate_graph.md).

The protocol of scripts/generate_bench.py: alternating rounds in one process, HIP event times, medians
with their spread. The weights of Llama-3-8B (16 GB) are far past the 256 MB last-level cache, so
every pass streams them from HBM.

1. Milliseconds per token at B = 1, 4 and 16 with 128 and 2048 cached keys: the eager arm is the
   loop body of ``generate_batch`` without its copy to the host (``sample`` then ``decode_step_rows``),
   the graph arm one ``DecodeGraph.replay()`` (the same work as one captured graph), both in a cache of
   the same capacity. At 128 keys a third arm replays in a cache of the 2048-key arm's capacity: what
   the capacity-sized attention grid costs when few keys are live.
2. The one-off cost of building a ``DecodeGraph`` (warm-up pass and capture).
3. One ``--sample-every`` boundary, 64 tokens from a one-token prompt: eager ``generate``,
   ``generate(graph=True)`` (captures on every call) and a kept ``DecodeGraph`` (``--sample-graph``).

    python scripts/generate_graph_bench.py [--rounds 7] [--model llama3-8b]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fault_tolerant_llm_training_amd import generation  # noqa: E402
from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for  # noqa: E402
from fault_tolerant_llm_training_amd.ops import decode as D  # noqa: E402

STEPS = 8  # tokens per timed round


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def stats_ms(ts):
    return {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}


def graph_arm(model, B, n_keys, capacity):
    """A DecodeGraph whose rows hold ``n_keys`` random keys; returns (run, seconds to build it)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g = generation.DecodeGraph(model, B, capacity)
    torch.cuda.synchronize()
    built = time.perf_counter() - t0
    g.cache.k.normal_()
    g.cache.v.normal_()
    g.pos0.fill_(n_keys)
    g._longest = n_keys

    def run():
        D.write_ctl(g.ctl, 0, 0.0, 0, 0, 0)
        g._t = 0
        for _ in range(STEPS):
            g.replay()

    return run, built


def eager_arm(model, B, n_keys, capacity):
    margs = model.model_args
    cache = generation.BatchKVCache(margs, B, capacity, model.flat.device, model.flat.dtype)
    cache.k.normal_()
    cache.v.normal_()
    for b in range(B):
        cache.set_length(b, n_keys)
    logits0 = torch.zeros(B, margs.vocab_size, dtype=model.flat.dtype, device=model.flat.device)

    def run():
        cache.steps = 0
        logits = logits0
        for t in range(STEPS):
            nxt = D.sample(logits, 0.0, 0, generation.token_key(0, t), 0)
            logits = generation.decode_step_rows(model, nxt, cache, t)

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--model", type=str, default="llama3-8b")
    ap.add_argument("--vocab-size", type=int, default=131072)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    margs = model_args_for(a.model, vocab_size=a.vocab_size, seq_len=4096)
    model = build_model(margs, dev, torch.bfloat16)
    out = {"model": a.model, "rounds": a.rounds, "steps_per_round": STEPS, "points": {}, "build_s": []}
    cap_long = 2048 + STEPS + 1
    for B in (1, 4, 16):
        for n_keys in (128, 2048):
            capacity = n_keys + STEPS + 1
            arms = {"eager": eager_arm(model, B, n_keys, capacity)}
            arms["graph"], built = graph_arm(model, B, n_keys, capacity)
            out["build_s"].append(built)
            if n_keys == 128:
                arms["graph_in_2048_capacity"], built = graph_arm(model, B, n_keys, cap_long)
                out["build_s"].append(built)
            for fn in arms.values():
                fn()
            torch.cuda.synchronize()
            times = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, fn in arms.items():
                    times[k].append(timed(fn) / STEPS)
            out["points"][f"B{B}_keys{n_keys}"] = {k: stats_ms(ts) for k, ts in times.items()}
            del arms
            torch.cuda.empty_cache()
    # one --sample-every boundary with the defaults: BOS alone, 64 tokens, greedy
    kept = generation.DecodeGraph(model, 1, 65)
    arms = {"eager": lambda: generation.generate(model, [1], 64),
            "graph_captured_per_call": lambda: generation.generate(model, [1], 64, graph=True),
            "graph_kept": lambda: kept.run([[1]], 64)[0]}
    ids = {k: fn() for k, fn in arms.items()}
    assert ids["eager"] == ids["graph_captured_per_call"] == ids["graph_kept"]
    tb = {k: [] for k in arms}
    for _ in range(3):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()  # returns host integers: the device is done
            tb[k].append(time.perf_counter() - t0)
    out["sample_boundary_64_tokens_s"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)}
                                          for k, v in tb.items()}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
