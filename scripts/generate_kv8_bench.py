"""FP8 KV cache measurements on one MI355X (record: profiles/kv8_decode.md), after the protocol of
scripts/generate_fp8_bench.py: the two arms alternating in one process, HIP event times, every call of
a round on the next of several copies of the cache (as the 32 layers of a step are), medians with the
spread. Llama-3-8B shapes: Hq 32, Hkv 8, D 128.

1. ``decode_attn_rows`` against ``decode_attn_rows_kv8`` at B in {1, 16, 64} x keys in {128, 2048}: us,
   beside the byte floor of each arm at the project's measured stream rate (6.35 TB/s, README).
2. ``decode_qkv_append_rows_`` against its ``_kv8`` form at the same B.
3. Llama-3-8B ms per step with ``mma=True`` at the same points, bf16 cache against FP8 cache.
4. Fidelity on the random-init model: over 256 greedy tokens of the bf16-cache decode, the share of steps
   where the FP8-cache decode of the same tokens picks the same token, and the relative logit error.

    python scripts/generate_kv8_bench.py [--rounds 7] [--skip-model] [--out profiles/kv8_decode.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fault_tolerant_llm_training_amd._native import kernels  # noqa: E402

HQ, HKV, HD = 32, 8, 128
STREAM_TBPS = 6.35
POINTS = [(B, n) for n in (128, 2048) for B in (1, 16, 64)]
CYCLE_BYTES = 1 << 30  # the copies of a round hold at least this much (beyond the 256 MB last-level cache)
MAX_COPIES = 32        # ... but no more than a step has layers


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def summary(ts, nbytes=None):
    med = statistics.median(ts)
    r = {"median_us": med * 1e6, "min_us": min(ts) * 1e6, "max_us": max(ts) * 1e6}
    if nbytes is not None:
        r["floor_us"] = nbytes / (STREAM_TBPS * 1e12) * 1e6
        r["median_tbps"] = nbytes / med / 1e12
    return r


def alternate(arms, rounds, per):
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    times = {a: [] for a in arms}
    for _ in range(rounds):
        for a, fn in arms.items():
            times[a].append(timed(fn) / per)
    return times


def bench_ops(rounds):
    k = kernels()
    dev = torch.device("cuda:0")
    from fault_tolerant_llm_training_amd.models.llama import rope_tables

    out = {}
    for B, n in POINTS:
        fp8_bytes = 2 * B * HKV * n * (HD + 4)
        copies = min(MAX_COPIES, max(2, -(-CYCLE_BYTES // fp8_bytes)))
        shape = (copies, B, HKV, n, HD)
        km, vm = (torch.randn(shape, device=dev).bfloat16() for _ in range(2))
        kc, vc = (torch.randint(0, 120, shape, device=dev, dtype=torch.uint8) for _ in range(2))
        ks, vs = (torch.rand(shape[:-1], device=dev) + 0.5 for _ in range(2))
        q = torch.randn(B, HQ * HD, device=dev).bfloat16()
        pos0 = torch.full((B,), n - 1, dtype=torch.int32, device=dev)
        arms = {"bf16": lambda: [k.decode_attn_rows(q, km[c], vm[c], pos0, 0, n) for c in range(copies)],
                "fp8": lambda: [k.decode_attn_rows_kv8(q, kc[c], vc[c], ks[c], vs[c], pos0, 0, n) for c in range(copies)]}
        times = alternate(arms, rounds, copies)
        res = {"copies": copies, "bf16": summary(times["bf16"], 2 * B * HKV * n * HD * 2),
               "fp8": summary(times["fp8"], fp8_bytes)}
        res["speedup"] = res["bf16"]["median_us"] / res["fp8"]["median_us"]
        if n == 128:  # the append does not depend on the key count
            cos, sin = (t.to(dev) for t in rope_tables(HD, n, 500000.0))
            qkv = torch.randn(B, (HQ + 2 * HKV) * HD, device=dev).bfloat16()
            ap = {"bf16": lambda: [k.decode_qkv_append_rows_(qkv, cos, sin, pos0, 0, n - 1, km[c], vm[c])
                                   for c in range(copies)],
                  "fp8": lambda: [k.decode_qkv_append_rows_kv8_(qkv, cos, sin, pos0, 0, n - 1, kc[c], vc[c], ks[c], vs[c])
                                  for c in range(copies)]}
            res["append"] = {a: summary(ts) for a, ts in alternate(ap, rounds, copies).items()}
        out[f"B{B}_keys{n}"] = res
        del km, vm, kc, vc, ks, vs
        torch.cuda.empty_cache()
    return out


def bench_model(rounds):
    from fault_tolerant_llm_training_amd import generation
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    dev = torch.device("cuda:0")
    margs = model_args_for("llama3-8b", vocab_size=131072, seq_len=4096)
    model = build_model(margs, dev, torch.bfloat16)
    torch.cuda.synchronize()
    out, steps = {}, 8
    for B, n in POINTS:
        prompts = [[5] * n] * B
        arms = {}
        for kv in ("model", "fp8"):
            cache = generation.BatchKVCache(margs, B, n + steps + 2, dev, torch.bfloat16, kv_dtype=kv)
            tok = torch.full((B,), 5, dtype=torch.int64, device=dev)

            def run(cache=cache):
                for t in range(steps):
                    generation.decode_step_rows(model, tok, cache, t, None, True)

            def reset(cache=cache):
                cache.reset()
                generation._prefill_rows(model, prompts, cache)

            arms[kv] = (reset, run, cache.nbytes)
        times = {a: [] for a in arms}
        for r in range(rounds + 1):  # round 0 warms every code object
            for a, (reset, run, _) in arms.items():
                reset()
                torch.cuda.synchronize()
                t = timed(run) / steps
                if r:
                    times[a].append(t * 1e3)
        out[f"B{B}_keys{n}"] = {a: {"ms_per_step": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts),
                                    "cache_gbytes": arms[a][2] / 1e9} for a, ts in times.items()}
        del arms
        torch.cuda.empty_cache()
    prompt = [1, 5, 9, 200, 3, 77, 410, 8, 2]
    ids = generation.generate(model, prompt, 256)
    ca, cb = (generation.KVCache(margs, len(prompt) + 256, dev, torch.bfloat16, kv_dtype=kv) for kv in ("model", "fp8"))
    generation.prefill(model, prompt, ca)
    generation.prefill(model, prompt, cb)
    same, rels = 0, []
    for t in ids[:-1]:
        la = generation.decode_step(model, t, ca).float()
        lb = generation.decode_step(model, t, cb).float()
        same += int(la.argmax() == lb.argmax())
        rels.append(float((lb - la).norm() / la.norm()))
    out["fidelity_random_init"] = {"steps": len(rels), "same_token_share": same / len(rels),
                                   "rel_logit_err_median": statistics.median(rels), "rel_logit_err_max": max(rels)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-ops", action="store_true")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON result to this file")
    a = ap.parse_args()
    out = {"rounds": a.rounds, "stream_tbps": STREAM_TBPS}
    if not a.skip_ops:
        out["ops"] = bench_ops(a.rounds)
    if not a.skip_model:
        out["llama3_8b_mma"] = bench_model(a.rounds)
    text = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
