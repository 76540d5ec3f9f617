"""Weight-only MXFP4 decode measurements on one MI355X (record: profiles/mxfp4_decode.md), after the
protocol of scripts/generate_fp8_bench.py: alternating rounds in one process, HIP event times, every
call of a round on the next of several copies of the weight (together more than the 256 MB
last-level cache even for the 4-bit arm), medians with the spread.

1. ``gemv_mx4`` / ``gemv_swiglu_mx4`` against the ``_w8`` and the model-dtype ops on the five
   Llama-3-8B products at R = 1, and the ``_rows`` forms at R = 8: time, and TB/s over the weight
   bytes each arm reads.
2. ``quantize_rows_mxfp4`` over the same weights: TB/s over bytes read + written.
3. Llama-3-8B ms per token (``decode_step_rows``), bf16 / FP8 / MXFP4, B in {1, 4, 16} at 128 and 2048
   cached keys; quantization time and ``nbytes``.
4. Fidelity on the random-init model: over 256 greedy tokens of the model-dtype decode, the share of
   steps where the MXFP4 decode of the same tokens picks the same token, and the relative logit error.

    python scripts/generate_mxfp4_bench.py [--rounds 7] [--skip-model] [--skip-products]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fault_tolerant_llm_training_amd._native import kernels  # noqa: E402

PRODUCTS = [("wqkv", 6144, 4096, False), ("wo", 4096, 4096, False), ("w13+swiglu", 28672, 4096, True),
            ("w2", 4096, 14336, False), ("head", 131072, 4096, False)]
CACHE_BYTES = 1 << 30
ROWS = (1, 8)
BYTES_PER_WEIGHT = {"model": 2.0, "fp8": 1.0, "mxfp4": 0.5 + 1 / 32}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def summary(ts, nbytes):
    med = statistics.median(ts)
    return {"median_us": med * 1e6, "min_us": min(ts) * 1e6, "max_us": max(ts) * 1e6, "median_tbps": nbytes / med / 1e12}


def bench_products(rounds):
    k = kernels()
    dev = torch.device("cuda:0")
    out = {}
    for name, N, K, swiglu in PRODUCTS:
        copies = max(2, -(-CACHE_BYTES // (N * K // 2)))  # sized for the smallest (MXFP4) arm
        ws = [(torch.randn(N, K, device=dev) * 0.02).bfloat16() for _ in range(copies)]
        q8 = [k.quantize_rows_e4m3(w) for w in ws]
        q4 = [k.quantize_rows_mxfp4(w) for w in ws]
        tq = [timed(lambda: [k.quantize_rows_mxfp4_out(w, c, s) for w, (c, s) in zip(ws, q4)]) / copies
              for _ in range(rounds)]
        out[name] = {"N": N, "K": K, "copies": copies, "quantize": summary(tq, (2 + 0.5 + 1 / 32) * N * K)}
        for R in ROWS:
            x = torch.randn(R, K, device=dev).bfloat16()
            if R == 1 and swiglu:
                arms = {"model": lambda: [k.gemv_swiglu(x[0], w) for w in ws],
                        "fp8": lambda: [k.gemv_swiglu_w8(x[0], c, s) for c, s in q8],
                        "mxfp4": lambda: [k.gemv_swiglu_mx4(x[0], c, s) for c, s in q4]}
            elif R == 1:
                arms = {"model": lambda: [k.gemv(x[0], w, None) for w in ws],
                        "fp8": lambda: [k.gemv_w8(x[0], c, s, None) for c, s in q8],
                        "mxfp4": lambda: [k.gemv_mx4(x[0], c, s, None) for c, s in q4]}
            elif swiglu:
                arms = {"model": lambda: [k.gemv_swiglu_rows(x, w) for w in ws],
                        "fp8": lambda: [k.gemv_swiglu_rows_w8(x, c, s) for c, s in q8],
                        "mxfp4": lambda: [k.gemv_swiglu_rows_mx4(x, c, s) for c, s in q4]}
            else:
                arms = {"model": lambda: [k.gemv_rows(x, w, None) for w in ws],
                        "fp8": lambda: [k.gemv_rows_w8(x, c, s, None) for c, s in q8],
                        "mxfp4": lambda: [k.gemv_rows_mx4(x, c, s, None) for c, s in q4]}
            for fn in arms.values():
                fn()
            torch.cuda.synchronize()
            times = {a: [] for a in arms}
            for _ in range(rounds):
                for a, fn in arms.items():
                    times[a].append(timed(fn) / copies)
            res = {a: summary(ts, N * K * BYTES_PER_WEIGHT[a]) for a, ts in times.items()}
            res["mxfp4_over_fp8"] = res["fp8"]["median_us"] / res["mxfp4"]["median_us"]
            out[name][f"R{R}"] = res
            print(f"{name} R={R} done", file=sys.stderr, flush=True)
        del ws, q8, q4
        torch.cuda.empty_cache()
    return out


def bench_model(rounds):
    from fault_tolerant_llm_training_amd import generation
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    dev = torch.device("cuda:0")
    margs = model_args_for("llama3-8b", vocab_size=131072, seq_len=4096)
    model = build_model(margs, dev, torch.bfloat16)
    torch.cuda.synchronize()
    w8 = generation.Fp8Weights(model)
    w4 = None
    tq = []
    for _ in range(3):
        def build():
            nonlocal w4
            w4 = generation.Mxfp4Weights(model) if w4 is None else (w4.requantize() or w4)
        tq.append(timed(build))
    out = {"fp8_gbytes": w8.nbytes / 1e9, "mxfp4_gbytes": w4.nbytes / 1e9,
           "quantize_s": {"median": statistics.median(tq), "min": min(tq), "max": max(tq)}}
    steps = 8
    for n_keys in (128, 2048):
        for B in (1, 4, 16):
            prompts = [[5] * n_keys] * B
            cap = n_keys + steps + 2
            cache = generation.BatchKVCache(margs, B, cap, dev, torch.bfloat16)
            tok = torch.full((B,), 5, dtype=torch.int64, device=dev)
            times = {"model": [], "fp8": [], "mxfp4": []}
            for r in range(rounds + 1):  # round 0 warms every code object
                for a, w in (("model", None), ("fp8", w8), ("mxfp4", w4)):
                    cache.reset()
                    generation._prefill_rows(model, prompts, cache)
                    torch.cuda.synchronize()
                    t = timed(lambda: [generation.decode_step_rows(model, tok, cache, s, w) for s in range(steps)])
                    if r:
                        times[a].append(t / steps * 1e3)
            print(f"keys {n_keys} B {B} done", file=sys.stderr, flush=True)
            out[f"keys_{n_keys}_B{B}"] = {a: {"ms_per_token": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
                                          for a, ts in times.items()}
            del cache
            torch.cuda.empty_cache()
    # fidelity: teacher-forced on the model-dtype greedy tokens
    prompt = [1, 5, 9, 200, 3, 77, 410, 8, 2]
    ids = generation.generate(model, prompt, 256)
    ca, cb = (generation.KVCache(margs, len(prompt) + 256, dev, torch.bfloat16) for _ in range(2))
    generation.prefill(model, prompt, ca)
    generation.prefill(model, prompt, cb)
    same, rels = 0, []
    for t in ids[:-1]:
        la = generation.decode_step(model, t, ca).float()
        lb = generation.decode_step(model, t, cb, w4).float()
        same += int(la.argmax() == lb.argmax())
        rels.append(float((lb - la).norm() / la.norm()))
    out["fidelity_random_init"] = {"steps": len(rels), "same_token_share": same / len(rels),
                                   "rel_logit_err_median": statistics.median(rels), "rel_logit_err_max": max(rels)}
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
