#!/usr/bin/env python3
"""AdamW with and without stochastic rounding (--stochastic-rounding) on one MI355X.

Two shapes, each timed in alternating windows (off, on, off, on, ...) in one process, so clock and
box drift hit both arms alike:

  bucket -- the per-bucket launches of the pipelined optimizer: one adamw_ launch per 64 MiB bucket
            (32 Mi bf16 elements), walking consecutive buckets of the flat buffers so every launch
            reads HBM, not the Infinity Cache (one bucket's 4 x 64 MiB would fit in it)
  pass   -- the whole 8B-sized flat buffer (8,030,261,248 elements) in one launch

Reported per window: time, and bytes / time with 14 B per parameter (bf16 p, g, m, v read; p, m, v
written). The summary gives each arm's median, the flag-off windows' spread, and on / off.

Usage: python scripts/adamw_sr_bench.py [--numel N] [--rounds 5] [--iters 10] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

LLAMA3_8B_NUMEL = 8_030_261_248
BUCKET = 32 << 20  # elements: 64 MiB of bf16
BYTES_PER_PARAM = 14


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--numel", type=int, default=LLAMA3_8B_NUMEL)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10, help="whole passes per timing window")
    ap.add_argument("--out", default="", help="also write the summary as JSON here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adamw_sr_bench: needs a GPU")
    from fault_tolerant_llm_training_amd._native import kernels
    from fault_tolerant_llm_training_amd.utils.sround import key_from_seed

    K = kernels()
    n = a.numel // 8 * 8
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)

    def filled(scale):
        t = torch.empty(n, dtype=torch.bfloat16, device=dev)
        for lo in range(0, n, 1 << 28):  # in pieces: no fp32 temporary of the whole buffer
            hi = min(n, lo + (1 << 28))
            t[lo:hi] = (torch.randn(hi - lo, generator=g, device=dev) * scale).to(torch.bfloat16)
        return t

    p, gr, m, v = filled(0.02), filled(1e-3), filled(1e-3), filled(1e-3).abs_()
    stats = torch.tensor([1.0, 1.0, 0.0], device=dev)
    key = key_from_seed(1234)
    hp = (5e-5, 0.9, 0.999, 1e-8, 0.01)
    step = [0]

    def whole(sr):
        step[0] += 1
        K.adamw_(p, gr, m, v, stats, *hp, step[0], 0, None, sr, key, 0)

    def buckets(sr):
        step[0] += 1
        for lo in range(0, n - BUCKET + 1, BUCKET):
            hi = lo + BUCKET
            K.adamw_(p[lo:hi], gr[lo:hi], m[lo:hi], v[lo:hi], stats, *hp, step[0], 0, None, sr, key, lo)

    nb = max(1, n // BUCKET)

    def window(fn, sr):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn(sr)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters  # ms per walk over the buffer

    res = {}
    for name, fn, per in (("bucket", buckets, nb), ("pass", whole, 1)):
        for sr in (False, True):  # warm both arms
            fn(sr)
        torch.cuda.synchronize()
        arms = {False: [], True: []}
        for r in range(a.rounds):
            for sr in (False, True):
                ms = window(fn, sr)
                arms[sr].append(ms)
                elems = per * BUCKET if name == "bucket" else n
                print(f"[sr-bench] {name} round {r} sr={'on ' if sr else 'off'} {ms / per:9.3f} ms per launch  "
                      f"{BYTES_PER_PARAM * elems / (ms * 1e-3) / 1e12:5.2f} TB/s", flush=True)
        med = {k: sorted(x)[len(x) // 2] for k, x in arms.items()}
        elems = per * BUCKET if name == "bucket" else n
        res[name] = {
            "launches_per_walk": per, "elements": elems,
            "off_ms": med[False] / per, "on_ms": med[True] / per,
            "off_TBps": BYTES_PER_PARAM * elems / (med[False] * 1e-3) / 1e12,
            "on_TBps": BYTES_PER_PARAM * elems / (med[True] * 1e-3) / 1e12,
            "off_spread": (max(arms[False]) - min(arms[False])) / med[False],
            "on_over_off": med[True] / med[False],
            "windows_off_ms": [x / per for x in arms[False]], "windows_on_ms": [x / per for x in arms[True]],
        }
        s = res[name]
        print(f"[sr-bench] {name}: off {s['off_ms']:.3f} ms ({s['off_TBps']:.2f} TB/s, spread {100 * s['off_spread']:.1f} %)  "
              f"on {s['on_ms']:.3f} ms ({s['on_TBps']:.2f} TB/s)  on/off {s['on_over_off']:.3f}", flush=True)
    assert torch.isfinite(p[: 1 << 20].float()).all()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"numel": n, "time": time.strftime("%Y-%m-%d %H:%M:%S"), **res}, f, indent=1)


if __name__ == "__main__":
    main()
