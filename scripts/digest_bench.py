"""Rate of the digest kernel (csrc/kernels/digest.hip) next to sumsq_into_, the project's other
single-pass read-only reduction, on one flat buffer in one process: interleaved rounds, HIP event
times. Also times the PyTorch composition the kernel replaces on the same buffer (the old
--state-digest cost) and checks that both give the same digest.

    python scripts/digest_bench.py [--numel 8030261248] [--dtype bf16] [--rounds 10]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fault_tolerant_llm_training_amd._native import kernels  # noqa: E402
from fault_tolerant_llm_training_amd.utils.digest import _composed, digest_accum, digest_int  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--numel", type=int, default=8_030_261_248)  # Llama-3-8B flat parameter buffer
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--no-composed", action="store_true")
    a = ap.parse_args()
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    dev = torch.device("cuda:0")
    n = a.numel // 8 * 8
    buf = torch.empty(n, dtype=dtype, device=dev)
    step = 1 << 28
    for lo in range(0, n, step):  # values like trained weights, in place
        buf[lo : lo + step].normal_(0.0, 0.02)
    nbytes = n * buf.element_size()
    k = kernels()
    partial = torch.empty(2048, dtype=torch.float32, device=dev)
    acc = torch.zeros(1, dtype=torch.int64, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    arms = {"sumsq_into_": lambda: k.sumsq_into_(buf, partial),
            "digest_accum_": lambda: digest_accum(acc, 0, buf, 0)}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(a.rounds):
        for name, fn in arms.items():
            times[name].append(timed(fn))
    out = {"numel": n, "dtype": a.dtype, "gbytes": nbytes / 1e9, "rounds": a.rounds}
    for name, ts in times.items():
        out[name] = {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3,
                     "median_tbps": nbytes / statistics.median(ts) / 1e12,
                     "best_tbps": nbytes / min(ts) / 1e12, "worst_tbps": nbytes / max(ts) / 1e12}
    t0 = time.perf_counter()
    dk = digest_int(buf)
    out["tensor_digest_kernel_s"] = time.perf_counter() - t0
    out["digest"] = f"{dk:016x}"
    if not a.no_composed:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dc = _composed(buf, 0)
        out["tensor_digest_composed_s"] = time.perf_counter() - t0
        out["composed_peak_gb"] = torch.cuda.max_memory_allocated(dev) / 1e9
        out["composed_equal"] = dc == dk
    print(json.dumps(out))
    return 0 if out.get("composed_equal", True) else 1


if __name__ == "__main__":
    sys.exit(main())
