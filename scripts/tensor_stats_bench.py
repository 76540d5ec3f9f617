"""Rate of the segmented statistics pass (csrc/kernels/tensor_stats.hip) over the Llama-3-8B flat
buffer with its slot table, next to digest_accum_ and sumsq_into_ -- the project's other one-touch
read-only streams -- on the same buffer in one process: alternating rounds, HIP event times. Also
the work-item sizes (chunk) tried, and the host-visible cost of one whole record (four buffers,
results on the host) beside the 8B step time.

    python scripts/tensor_stats_bench.py [--rounds 10] [--step-ms 99.9] [--out FILE]
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
from fault_tolerant_llm_training_amd.models.flat import ALIGN  # noqa: E402
from fault_tolerant_llm_training_amd.models.llama import Transformer, model_args_for  # noqa: E402
from fault_tolerant_llm_training_amd.utils.digest import digest_accum  # noqa: E402
from fault_tolerant_llm_training_amd.utils.tensor_stats import SegmentStatsPlan, chunk  # noqa: E402


def slot_table(preset: str, vocab: int, seq: int):
    """(offsets, numels, buffer length) of the preset's flat layout, from shapes alone."""
    model = Transformer(model_args_for(preset, vocab_size=vocab, seq_len=seq))  # parameters on meta
    named = dict(model.named_parameters())
    off, num, pos = [], [], 0
    for name in model.flat_layout():
        n = named[name].numel()
        off.append(pos)
        num.append(n)
        pos += (n + ALIGN - 1) // ALIGN * ALIGN
    return off, num, (pos + ALIGN - 1) // ALIGN * ALIGN


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--vocab-size", type=int, default=131072)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--chunks", default="65536,131072,262144,524288,1048576")
    ap.add_argument("--step-ms", type=float, default=99.9, help="the model's step time the record is set beside")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    off, num, n = slot_table(a.model, a.vocab_size, 2048)
    buf = torch.empty(n, dtype=torch.bfloat16, device=dev)
    for lo in range(0, n, 1 << 28):  # values like trained weights, in place
        buf[lo : lo + (1 << 28)].normal_(0.0, 0.02)
    other = buf.clone()
    nbytes = n * buf.element_size()
    k = kernels()
    partial = torch.empty(2048, dtype=torch.float32, device=dev)
    acc = torch.zeros(1, dtype=torch.int64, device=dev)
    built_in = chunk()
    sizes = sorted({int(c) for c in a.chunks.split(",")} | {built_in})
    plans = {c: SegmentStatsPlan(off, num, dev, chunk=c) for c in sizes}
    outs = {c: torch.empty(len(off), 4, dtype=torch.float64, device=dev) for c in sizes}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    arms = {"sumsq_into_": lambda: k.sumsq_into_(buf, partial),
            "digest_accum_": lambda: digest_accum(acc, 0, buf, 0)}
    for c in sizes:
        arms[f"segment_stats chunk={c}"] = (lambda c=c: plans[c].run(buf, outs[c]))
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(a.rounds):
        for name, fn in arms.items():
            times[name].append(timed(fn))
    res = {"model": a.model, "segments": len(off), "numel": n, "gbytes": nbytes / 1e9, "rounds": a.rounds,
           "built_in_chunk": built_in, "arms": {}}
    for name, ts in times.items():
        med = statistics.median(ts)
        res["arms"][name] = {"median_ms": med * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3,
                             "median_tbps": nbytes / med / 1e12}
    dg = res["arms"]["digest_accum_"]["median_ms"]
    for c in sizes:
        arm = res["arms"][f"segment_stats chunk={c}"]
        arm["items"] = int(plans[c].items.shape[0])
        arm["vs_digest"] = arm["median_ms"] / dg
    # the chunk sizes must agree on everything but the last bits of sumsq
    ref = outs[built_in].cpu()
    for c in sizes:
        o = outs[c].cpu()
        assert torch.equal(o[:, 1:], ref[:, 1:]), c
        assert torch.allclose(o[:, 0], ref[:, 0], rtol=1e-12, atol=0.0), c
    # one whole record: four passes (two buffers, alternating) and the results on the host
    plan = plans[built_in]
    four = [torch.empty(len(off), 4, dtype=torch.float64, device=dev) for _ in range(4)]
    record = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, o in enumerate(four):
            plan.run(buf if i % 2 == 0 else other, o)
        host = torch.stack(four).cpu()
        record.append(time.perf_counter() - t0)
    assert host.shape == (4, len(off), 4)
    med = statistics.median(record)
    res["record"] = {"buffers": 4, "gbytes": 4 * nbytes / 1e9, "median_ms": med * 1e3, "min_ms": min(record) * 1e3,
                     "max_ms": max(record) * 1e3, "step_ms": a.step_ms, "steps_worth": med * 1e3 / a.step_ms}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
