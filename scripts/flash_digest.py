"""SHA-256 digests of the flash attention outputs on seeded inputs: does another build of the kernel
library compute the same bits?

    FT_KERNELS_SO=<build A>/_kernels.so python scripts/flash_digest.py > a.jsonl
    python scripts/flash_digest.py > b.jsonl                  (a fresh process per build)
    python scripts/flash_digest.py --compare a.jsonl b.jsonl  (a markdown table; exit 1 on a difference)

One JSON line per shape (B, S, Hq, Hkv, D): digests of o and lse (flash_fwd, flash_doc_fwd; the valid
lse entries only) and of dqkv (flash_bwd mode 1 and flash_doc_bwd, without and with RoPE tables). Mode 0
adds dQ with atomics, so it has no digest: its relative distance to mode 1 is printed and must be below
1e-2 in each build.
"""
import hashlib
import json
import os
import sys

SHAPES = [(2, 320, 8, 2, 128), (1, 1000, 4, 1, 128), (2, 512, 8, 2, 64), (1, 100, 6, 2, 64), (1, 512, 16, 1, 128),
          (1, 777, 16, 2, 128), (1, 2048, 32, 8, 128), (1, 2048, 12, 12, 64), (8, 512, 16, 4, 64), (1, 33, 2, 2, 128)]
MODE0_REL = 1e-2


def compare(pa, pb):
    rows = [[json.loads(line) for line in open(p) if line.startswith("{")] for p in (pa, pb)]
    bad = len(rows[0]) != len(rows[1]) or not rows[0]
    print("| shape (B, S, Hq, Hkv, D) | digests: SHA-256 over them, A / B | equal | mode 0 vs 1, rel (A / B) |")
    print("|---|---|---|---|")
    for a, b in zip(*rows):
        same = a["shape"] == b["shape"] and a["sha"] == b["sha"]
        rels = [max(r["rel0"].values()) for r in (a, b)]
        bad |= not same or max(rels) >= MODE0_REL
        both = [hashlib.sha256(json.dumps(r["sha"], sort_keys=True).encode()).hexdigest()[:16] for r in (a, b)]
        print(f"| {tuple(a['shape'])} | {len(a['sha'])}: `{both[0]}` / `{both[1]}` | {'yes' if same else 'NO'} | "
              f"{rels[0]:.2e} / {rels[1]:.2e} |")
        if not same:
            print("  differing:", [k for k in a["sha"] if a["sha"][k] != b["sha"].get(k)], file=sys.stderr)
    print("all digests equal, mode 0 within %g of mode 1" % MODE0_REL if not bad else "DIFFERENT")
    return 1 if bad else 0


def main():
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fault_tolerant_llm_training_amd._native import kernels
    from fault_tolerant_llm_training_amd.models.llama import rope_tables

    K = kernels()

    def sha(t):
        return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()

    def rel(a, b):
        return ((a.float() - b.float()).norm() / b.float().norm()).item()

    for B, S, Hq, Hkv, D in SHAPES:
        g = torch.Generator().manual_seed(1000 * S + Hq)  # CPU generator: the same inputs in every process
        T = B * S
        qkv = torch.randn(T, (Hq + 2 * Hkv) * D, generator=g).bfloat16().cuda()
        qk = torch.randn(T, (Hq + Hkv) * D, generator=g).bfloat16().cuda()
        do = torch.randn(T, Hq * D, generator=g).bfloat16().cuda()
        tok = torch.randint(0, 48, (B, S), generator=g).cuda()  # a document boundary every ~48 tokens
        ds, de = K.doc_bounds(tok, 0)
        cos, sin = (t.cuda() for t in rope_tables(D, S, 500000.0))
        out, rel0 = {}, {}
        o, lse = K.flash_fwd(qk, qkv, S, Hq, Hkv, D)
        od, lsed = K.flash_doc_fwd(qk, qkv, ds, de, S, Hq, Hkv, D)
        out["fwd.o"], out["fwd.lse"] = sha(o), sha(lse[..., :S])
        out["doc_fwd.o"], out["doc_fwd.lse"] = sha(od), sha(lsed[..., :S])
        for name, cs in (("", (None, None)), ("+rope", (cos, sin))):
            g1 = K.flash_bwd(do, qk, qkv, o, lse, S, Hq, Hkv, D, 1, *cs)
            out["bwd1" + name] = sha(g1)
            out["doc_bwd" + name] = sha(K.flash_doc_bwd(do, qk, qkv, od, lsed, ds, de, S, Hq, Hkv, D, *cs))
            rel0["bwd0" + name] = rel(K.flash_bwd(do, qk, qkv, o, lse, S, Hq, Hkv, D, 0, *cs), g1)
        print(json.dumps({"shape": [B, S, Hq, Hkv, D], "sha": out, "rel0": rel0}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main()
