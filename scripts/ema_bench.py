#!/usr/bin/env python3
"""The parameter average (--ema-decay) on one MI355X: the kernel, the 8B step, the weight swap.

  kernels -- ema_update_ over the Llama-3-8B flat buffer (8,030,261,248 bf16 parameters, fp32 average:
             10 B per element), beside sumsq_into_ over the same parameters (2 B per element) and one
             adamw_ launch per 64 MiB bucket (14 B per element), in the same process. Alternating
             windows (ema, sumsq, adamw, ema, ...), HIP event times.
  step    -- the Llama-3-8B bench step (seq 2048, batch 1) with the average off, updated every step and
             every 10th step, in alternating windows of one process (the protocol of scripts/ab_step.py);
             then one ema_weights() enter + exit.

Usage: python scripts/ema_bench.py [--part kernels|step|all] [--rounds 5] [--iters 10] [--steps 10] [--out FILE]
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


def _median(x):
    return sorted(x)[len(x) // 2]


def kernels_part(a, dev):
    from fault_tolerant_llm_training_amd._native import kernels
    from fault_tolerant_llm_training_amd.utils.ema import one_minus_decay

    K = kernels()
    n = a.numel // 8 * 8
    g = torch.Generator(device=dev).manual_seed(0)

    def filled(scale, dtype=torch.bfloat16):
        t = torch.empty(n, dtype=dtype, device=dev)
        for lo in range(0, n, 1 << 28):  # in pieces: no temporary of the whole buffer
            hi = min(n, lo + (1 << 28))
            t[lo:hi] = (torch.randn(hi - lo, generator=g, device=dev) * scale).to(dtype)
        return t

    p, gr, m, v = filled(0.02), filled(1e-3), filled(1e-3), filled(1e-3).abs_()
    e = filled(0.02, torch.float32)
    stats = torch.tensor([1.0, 1.0, 0.0], device=dev)
    omd = one_minus_decay(0.999)
    partial = torch.zeros(2048, dtype=torch.float32, device=dev)
    nb = max(1, n // BUCKET)
    step = [0]

    def ema():
        K.ema_update_(e, p, stats, omd, 0)

    def ema_buckets():
        for lo in range(0, nb * BUCKET, BUCKET):
            K.ema_update_(e[lo : lo + BUCKET], p[lo : lo + BUCKET], stats, omd, 0)

    def sumsq():
        K.sumsq_into_(p, partial)

    def adamw_buckets():
        step[0] += 1
        for lo in range(0, nb * BUCKET, BUCKET):
            hi = lo + BUCKET
            K.adamw_(p[lo:hi], gr[lo:hi], m[lo:hi], v[lo:hi], stats, 5e-5, 0.9, 0.999, 1e-8, 0.01, step[0], 0)

    arms = [("ema_update_ whole buffer", ema, n, 10, 1), ("ema_update_ per 64 MiB bucket", ema_buckets, nb * BUCKET, 10, nb),
            ("sumsq_into_ whole buffer", sumsq, n, 2, 1), ("adamw_ per 64 MiB bucket", adamw_buckets, nb * BUCKET, 14, nb)]

    def window(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    for _name, fn, *_ in arms:
        fn()
    times = {name: [] for name, *_ in arms}
    for r in range(a.rounds):
        for name, fn, elems, bpe, launches in arms:
            ms = window(fn)
            times[name].append(ms)
            print(f"[ema-bench] round {r} {name:32s} {ms:9.3f} ms per walk  {bpe * elems / (ms * 1e-3) / 1e12:5.2f} TB/s",
                  flush=True)
    res = {}
    for name, _fn, elems, bpe, launches in arms:
        med = _median(times[name])
        res[name] = {"elements": elems, "bytes_per_element": bpe, "launches_per_walk": launches, "median_ms": med,
                     "ms_per_launch": med / launches, "TBps": bpe * elems / (med * 1e-3) / 1e12,
                     "spread": (max(times[name]) - min(times[name])) / med, "windows_ms": times[name]}
        print(f"[ema-bench] {name:32s} median {med:9.3f} ms ({med / launches:.4f} ms per launch)  "
              f"{res[name]['TBps']:.2f} TB/s  spread {100 * res[name]['spread']:.2f} %", flush=True)
    assert torch.isfinite(e[: 1 << 20]).all()
    return res


def step_part(a, dev):
    from fault_tolerant_llm_training_amd.data.synthetic import SyntheticTokens
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for
    from fault_tolerant_llm_training_amd.optim.adamw import FlatAdamW
    from fault_tolerant_llm_training_amd.parallel.ddp import GradReducer
    from fault_tolerant_llm_training_amd.utils.ema import one_minus_decay
    from fault_tolerant_llm_training_amd.utils.lr import build_lr_scheduler

    V, S = 131072, a.seq_len
    model = build_model(model_args_for(a.model, vocab_size=V, seq_len=S), dev, torch.bfloat16, seed=1234)
    red = GradReducer(model.flat, model.sinks_in_backward_order())  # bench.py's default buckets
    opt = FlatAdamW(model.parameters(), model.flat, lr=5e-5, max_grad_norm=1.0, reducer=red, ema_decay=0.999)
    model.gate = opt.gate
    sched = build_lr_scheduler(opt, 100)
    data = SyntheticTokens(V, S, seed=4321)
    inv = torch.full((1,), 1.0 / S, dtype=torch.float32, device=dev)
    it = [0]

    def step():
        tok, lab = data.batch(it[0], 1)
        it[0] += 1
        loss = model(tok.to(dev, non_blocking=True), lab.to(dev, non_blocking=True), inv)
        loss.backward()
        red.finish()
        opt.clip_grad_norm_(1.0)
        opt.step()
        sched.step()
        return loss

    def set_every(k):  # 0: never (the launches of a run without the flag)
        opt.gate.wait_all()
        torch.cuda.synchronize()
        opt.ema_every = k if k else 1 << 62
        opt._ema_omd = one_minus_decay(0.999, k or 1)

    def window(n):
        opt.gate.wait_all()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            step()
        opt.gate.wait_all()
        opt.wait_ema()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n * 1e3

    arms = [("off", 0), ("every 1", 1), ("every 10", 10)]
    for _name, k in arms:
        set_every(k)
        for _ in range(a.warmup):
            step()
    times = {name: [] for name, _ in arms}
    for r in range(a.rounds):
        for name, k in arms:
            set_every(k)
            ms = window(a.steps)
            times[name].append(ms)
            print(f"[ema-bench] step round {r} ema {name:8s} {ms:8.2f} ms/step", flush=True)
    res = {}
    for name, _k in arms:
        med = _median(times[name])
        res[name] = {"median_ms": med, "windows_ms": times[name], "tok_s": S * 1000 / med}
        print(f"[ema-bench] step ema {name:8s} median {med:8.2f} ms/step  windows "
              + ", ".join(f"{x:.2f}" for x in times[name])
              + f"  ratio to off {med / _median(times['off']):.4f}", flush=True)
    swaps = []
    for _ in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        with opt.ema_weights():
            torch.cuda.synchronize()
            t_in = time.perf_counter()
        torch.cuda.synchronize()
        swaps.append(((t_in - t) * 1e3, (time.perf_counter() - t_in) * 1e3))
    res["ema_weights"] = {"enter_ms": [s[0] for s in swaps], "exit_ms": [s[1] for s in swaps]}
    print("[ema-bench] ema_weights() enter / exit ms: " + ", ".join(f"{i:.2f} / {o:.2f}" for i, o in swaps), flush=True)
    loss = step()
    torch.cuda.synchronize()
    print(f"[ema-bench] final loss {float(loss.detach()):.4f}  peak HBM {torch.cuda.max_memory_allocated(dev) / 2**30:.1f} GiB",
          flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["kernels", "step", "all"])
    ap.add_argument("--numel", type=int, default=LLAMA3_8B_NUMEL)
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--seq-len", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10, help="walks over the buffer per kernel timing window")
    ap.add_argument("--steps", type=int, default=10, help="steps per step timing window (a multiple of 10)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="", help="also write the summary as JSON here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ema_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"time": time.strftime("%Y-%m-%d %H:%M:%S")}
    if a.part in ("kernels", "all"):
        res["kernels"] = kernels_part(a, dev)
        torch.cuda.empty_cache()
    if a.part in ("step", "all"):
        res["step"] = step_part(a, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
