"""Document-masked flash attention (flash_doc_fwd / flash_doc_bwd) against the plain causal kernels
on the same tensors: the Llama-3-8B layer shape (B=1, 32/8 heads, d=128) at S = 2048, 8192, 16384,
with one document (the mask costs only its loads) and with equal documents of S/8.

Plain kernels timed: the default forward (pipelined) and deterministic backward (dQ key split on),
and the unsplit, unpipelined ones the doc kernels extend (flash_set_fwd_pipe(0) / flash_set_dq_split(0) / flash_set_kv_split(0)).

    python scripts/flash_doc_bench.py [d=128|d=64] [S ...]      # prints one markdown table

d=64: the same lengths with 12 / 12 heads of 64 (the GPT-2-small layer: 2-wave backward blocks).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fault_tolerant_llm_training_amd._native import kernels

K = kernels()
ARGS = sys.argv[1:]
Hq, Hkv, D = (12, 12, 64) if "d=64" in ARGS else (32, 8, 128)
LENGTHS = [int(v) for v in ARGS if v.isdigit()] or [2048, 8192, 16384]
print(f"heads {Hq}/{Hkv}, head_dim {D}")


NSETS = 4  # rotating input sets: successive launches do not re-read the same (cache-warm) tensors


def t(fn, reps=5, window_us=20000.0):
    """fn(i) launches on input set i % NSETS. Best and worst of `reps` means, in us, each over a
    window of launches sized to ~20 ms of GPU time (at least 20 launches)."""
    for i in range(2 * NSETS):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(NSETS):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    it = max(20, int(window_us / (a.elapsed_time(b) / NSETS * 1e3)))
    it = (it + NSETS - 1) // NSETS * NSETS
    out = []
    for _ in range(reps):
        a.record()
        for i in range(it):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / it * 1e3)
    return min(out), max(out)


def bounds(S, L):
    pos = torch.arange(S, dtype=torch.int32, device="cuda")
    ds = (pos // L * L).view(1, S).contiguous()
    return ds, (ds + L).clamp(max=S).contiguous()


def fmt(v):
    return f"{v[0]:8.1f} (max {v[1]:8.1f})"


print("| S | documents | kernel | forward us | deterministic backward us |")
print("|---|---|---|---|---|")
for S in LENGTHS:
    torch.manual_seed(0)
    sets = []
    for _ in range(NSETS):
        qkv = torch.randn(S, (Hq + 2 * Hkv) * D, device="cuda").bfloat16()
        qk = torch.randn(S, (Hq + Hkv) * D, device="cuda").bfloat16()
        do = torch.randn(S, Hq * D, device="cuda").bfloat16()
        o, lse = K.flash_fwd(qk, qkv, S, Hq, Hkv, D)
        sets.append((qk, qkv, do, o, lse))

    def fwd(i):
        qk, qkv, _, _, _ = sets[i % NSETS]
        K.flash_fwd(qk, qkv, S, Hq, Hkv, D)

    def bwd(i):
        qk, qkv, do, o, lse = sets[i % NSETS]
        K.flash_bwd(do, qk, qkv, o, lse, S, Hq, Hkv, D, 1)

    pf, pb = t(fwd), t(bwd)
    print(f"| {S} | - | plain, default (pipelined fwd, dQ key split) | {fmt(pf)} | {fmt(pb)} |")
    try:
        K.flash_set_fwd_pipe(0)
        K.flash_set_fwd_split(0)
        K.flash_set_dq_split(0)
        K.flash_set_kv_split(0)
        uf, ub = t(fwd), t(bwd)
    finally:
        K.flash_set_fwd_pipe(1)
        K.flash_set_fwd_split(-1)
        K.flash_set_dq_split(-1)
        K.flash_set_kv_split(-1)
    print(f"| {S} | - | plain, unsplit unpipelined | {fmt(uf)} | {fmt(ub)} |")
    for name, L in (("1", S), ("8 x S/8", S // 8)):
        ds, de = bounds(S, L)
        outs = [K.flash_doc_fwd(qk, qkv, ds, de, S, Hq, Hkv, D) for qk, qkv, _, _, _ in sets]

        def dfwd(i):
            qk, qkv, _, _, _ = sets[i % NSETS]
            K.flash_doc_fwd(qk, qkv, ds, de, S, Hq, Hkv, D)

        def dbwd(i):
            qk, qkv, do, _, _ = sets[i % NSETS]
            od, lsed = outs[i % NSETS]
            K.flash_doc_bwd(do, qk, qkv, od, lsed, ds, de, S, Hq, Hkv, D)

        df, db = t(dfwd), t(dbwd)
        print(f"| {S} | {name} | doc | {fmt(df)} | {fmt(db)} |")
        print(f"| {S} | {name} | doc / plain default | {df[0] / pf[0]:.3f} | {db[0] / pb[0]:.3f} |")
        print(f"| {S} | {name} | doc / plain unsplit unpipelined | {df[0] / uf[0]:.3f} | {db[0] / ub[0]:.3f} |")
