"""Batched generation on the GPU: the multi-row decode kernels (csrc/kernels/decode.hip) against the
one-row kernels looped over rows, bit for bit; generate_batch against per-prompt generate; the
batched decode path of a model against its full forward; --sample-count runs of train.py.
"""
import json
import math
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
RS = [1, 2, 3, 5, 8, 9, 17]  # partial tiles of every height, a full tile, a second and a third tile
R_MAX = max(RS)


@pytest.fixture(scope="module")
def K():
    from fault_tolerant_llm_training_amd._native import kernels

    return kernels()


def _ks(dtype):
    """One active lane, exactly one unrolled sweep, a sweep plus tail, two sweeps plus tail."""
    return [4, 1024, 1028, 2308] if dtype == torch.float32 else [8, 2048, 2056, 4616]


# ------------------------------------------------------------------------------- gemv_rows
@pytest.mark.parametrize("dt", list(DTYPES))
def test_gemv_rows_equals_gemv_per_row_bit_for_bit(K, dt):
    dtype = DTYPES[dt]
    gen = torch.Generator(device="cuda").manual_seed(21)
    for N in (1, 5, 64, 257):
        for Kd in _ks(dtype):
            x = torch.randn(R_MAX, Kd, generator=gen, device="cuda").to(dtype)
            w = (torch.randn(N, Kd, generator=gen, device="cuda") / math.sqrt(Kd)).to(dtype)
            res = torch.randn(R_MAX, N, generator=gen, device="cuda").to(dtype)
            want = torch.stack([K.gemv(x[r], w, None) for r in range(R_MAX)])
            want_res = torch.stack([K.gemv(x[r], w, res[r]) for r in range(R_MAX)])
            for R in RS:
                y = K.gemv_rows(x[:R], w, None)
                assert y.shape == (R, N) and y.dtype == dtype
                assert torch.equal(y, want[:R]), (N, Kd, R)
                assert torch.equal(K.gemv_rows(x[:R], w, res[:R].contiguous()), want_res[:R]), (N, Kd, R)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_gemv_swiglu_rows_equals_gemv_swiglu_per_row_bit_for_bit(K, dt):
    dtype = DTYPES[dt]
    gen = torch.Generator(device="cuda").manual_seed(22)
    for H in (1, 6, 130):
        for Kd in _ks(dtype):
            x = torch.randn(R_MAX, Kd, generator=gen, device="cuda").to(dtype)
            w13 = (2 * torch.randn(2 * H, Kd, generator=gen, device="cuda") / math.sqrt(Kd)).to(dtype)
            want = torch.stack([K.gemv_swiglu(x[r], w13) for r in range(R_MAX)])
            for R in RS:
                a = K.gemv_swiglu_rows(x[:R], w13)
                assert a.shape == (R, H) and a.dtype == dtype
                assert torch.equal(a, want[:R]), (H, Kd, R)


def _ints(shape, lo, hi, dtype, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen, device="cuda").to(dtype)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_gemv_rows_small_integers_are_exact(K, dt):
    """The construction of test_generate_gpu.py::test_gemv_small_integers_are_exact: every product and
    partial sum is exact in fp32, so each row is the integer product rounded once to the output dtype.
    (The bitwise tests above could not see a defect gemv_rows shares with gemv.)"""
    dtype = DTYPES[dt]
    gen = torch.Generator(device="cuda").manual_seed(11)
    for N in (1, 5, 257, 4096):
        for Kd in (8, 264, 4096):
            for R in (5, 9):
                x, w = _ints((R, Kd), -4, 4, dtype, gen), _ints((N, Kd), -4, 4, dtype, gen)
                res = _ints((R, N), -64, 64, dtype, gen)
                ref = (x.long().cpu() @ w.long().cpu().T).cuda()  # the int64 product (no such GEMM on the GPU)
                assert int(ref.abs().max()) < 2 ** 24
                assert torch.equal(K.gemv_rows(x, w, None), ref.double().to(dtype)), (N, Kd, R)
                assert torch.equal(K.gemv_rows(x, w, res), (ref + res.long()).double().to(dtype)), (N, Kd, R)


def test_gemv_rows_refuses_what_gemv_refuses_and_the_wrapper_loops(K):
    from fault_tolerant_llm_training_amd.ops.decode import gemv, gemv_rows

    x, w = torch.randn(3, 12, device="cuda").bfloat16(), torch.randn(5, 12, device="cuda").bfloat16()
    with pytest.raises(RuntimeError):
        K.gemv_rows(x, w, None)  # K % 8
    assert torch.equal(gemv_rows(x, w), torch.stack([gemv(x[r], w) for r in range(3)]))
    with pytest.raises(RuntimeError):
        K.gemv_rows(torch.empty(0, 16, device="cuda").bfloat16(), torch.randn(5, 16, device="cuda").bfloat16(), None)
    with pytest.raises(RuntimeError):
        K.gemv_rows(torch.randn(16, device="cuda").bfloat16(), torch.randn(5, 16, device="cuda").bfloat16(), None)


# ------------------------------------------------------------------------------- decode_qkv_append_rows_
@pytest.mark.parametrize("hq,hkv,d", [(4, 2, 64), (4, 1, 128)])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_qkv_append_rows_equals_three_one_row_calls(K, hq, hkv, d, dt):
    from fault_tolerant_llm_training_amd.models.llama import rope_tables

    dtype, smax, B, t = DTYPES[dt], 24, 3, 1
    positions = [0, 5, smax - 2]
    pos0 = torch.tensor(positions, dtype=torch.int32, device="cuda")
    cos, sin = (x.cuda() for x in rope_tables(d, smax, 500000.0))
    torch.manual_seed(25)
    qkv = torch.randn(B, (hq + 2 * hkv) * d, device="cuda").to(dtype)
    kc = torch.full((B, hkv, smax, d), -7.0, device="cuda").to(dtype)  # a sentinel in every slot
    vc = torch.full((B, hkv, smax, d), 9.0, device="cuda").to(dtype)
    q1, k1, v1 = qkv.clone(), kc.clone(), vc.clone()
    K.decode_qkv_append_rows_(qkv, cos, sin, pos0, t, max(positions) + t, kc, vc)
    for b, p in enumerate(positions):
        K.decode_qkv_append_(q1[b], cos, sin, p + t, k1[b], v1[b])
    assert torch.equal(qkv, q1)
    assert torch.equal(kc, k1) and torch.equal(vc, v1)  # the whole caches: nothing outside [b, :, pos]
    for b, p in enumerate(positions):
        assert not (kc[b, :, p + t] == -7.0).all() and torch.equal(vc[b, :, p + t].reshape(-1), qkv[b, (hq + hkv) * d :])
    with pytest.raises(RuntimeError):
        K.decode_qkv_append_rows_(qkv, cos, sin, pos0, t, smax, kc, vc)  # the largest position is outside
    with pytest.raises(RuntimeError):
        K.decode_qkv_append_rows_(qkv, cos, sin, pos0.long(), t, smax - 1, kc, vc)


# ------------------------------------------------------------------------------- decode_attn_rows
@pytest.mark.parametrize("hq,hkv,d", [(4, 2, 64), (4, 1, 128), (4, 4, 64)])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_attn_rows_equals_decode_attn_per_row(K, hq, hkv, d, dt):
    dtype, B, smax = DTYPES[dt], 4, 304
    C = int(K.decode_attn_chunk())
    assert C == 128
    torch.manual_seed(26)
    kc, vc = (torch.randn(B, hkv, smax, d, device="cuda").to(dtype) for _ in range(2))
    qkv = torch.randn(B, (hq + 2 * hkv) * d, device="cuda").to(dtype)
    for counts, t in (([1, 128, 129, 300], 0), ([3, 128, 129, 300], 2), ([300, 1, 129, 2], 0)):
        pos0 = torch.tensor([n - 1 - t for n in counts], dtype=torch.int32, device="cuda")
        for q in (qkv[:, : hq * d].contiguous(), qkv[:, : hq * d]):  # dense, and the Q columns of qkv in place
            want = torch.stack([K.decode_attn(q[b].contiguous(), kc[b], vc[b], n) for b, n in enumerate(counts)])
            o = K.decode_attn_rows(q, kc, vc, pos0, t, max(counts))
            assert o.shape == (B, hq * d) and o.dtype == dtype
            assert torch.equal(o, want), (counts, t)
            # the partials come from an uninitialised allocation: leave NaN where the next one is likely to
            # land (best effort), so that a merge reading a chunk its row never wrote would show
            junk = torch.full((B * ((max(counts) + C - 1) // C) * hq * (d + 2),), float("nan"), device="cuda")
            del junk
            assert torch.equal(K.decode_attn_rows(q, kc, vc, pos0, t, max(counts)), want), (counts, t)
    kn, vn = kc.clone(), vc.clone()
    for b, n in enumerate(counts):
        kn[b, :, n:] = float("nan")
        vn[b, :, n:] = float("nan")
    assert torch.equal(K.decode_attn_rows(q, kn, vn, pos0, t, max(counts)), want)  # keys beyond a row's count: unread
    with pytest.raises(RuntimeError):
        K.decode_attn_rows(q, kc, vc, pos0, t, smax + 1)
    with pytest.raises(RuntimeError):
        K.decode_attn_rows(q, kc, vc, pos0, 5, 5)  # max_keys must exceed t


# ------------------------------------------------------------------------------- generate_batch
PROMPT_LENS = [1, 2, 17, 40, 17]
N_NEW = 12


@pytest.fixture(scope="module")
def tiny():
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    return build_model(model_args_for("tiny", vocab_size=512, seq_len=64), "cuda", torch.bfloat16, seed=3)


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(31)
    ps = [torch.randint(0, 512, (n,), generator=g).tolist() for n in PROMPT_LENS]
    ps[4] = list(ps[2])  # two identical prompts: prefilled once
    return ps


@pytest.fixture(scope="module")
def singles(tiny, prompts):
    """Greedy generate() of every prompt alone: computed once, left unchanged."""
    from fault_tolerant_llm_training_amd.generation import generate

    return [generate(tiny, p, N_NEW) for p in prompts]


def test_generate_batch_greedy_equals_generate_per_prompt(tiny, prompts, singles):
    from fault_tolerant_llm_training_amd.generation import generate_batch

    assert all(len(s) == N_NEW for s in singles)
    assert generate_batch(tiny, prompts, N_NEW) == singles
    assert generate_batch(tiny, prompts[::-1], N_NEW) == singles[::-1]
    for p, s in zip(prompts, singles):
        assert generate_batch(tiny, [p], N_NEW) == [s]


def test_sampled_rows_are_the_samplers_rows_of_per_row_decode_steps(tiny, prompts):
    from fault_tolerant_llm_training_amd.generation import (KVCache, decode_step, generate, generate_batch, prefill,
                                                            token_key)
    from fault_tolerant_llm_training_amd.ops import decode as D

    kw = dict(temperature=0.8, top_k=40, key=0x5EED, step=7)
    batch = [prompts[1], prompts[2], prompts[1], prompts[0]]
    got = generate_batch(tiny, batch, N_NEW, **kw)
    assert got[0] == generate(tiny, batch[0], N_NEW, **kw)
    assert got[0] != got[2]  # the same prompt in another row: another draw
    caches = [KVCache(tiny.model_args, len(p) + N_NEW, "cuda", torch.bfloat16) for p in batch]
    logits = torch.stack([prefill(tiny, p, c) for p, c in zip(batch, caches)])
    want = [[] for _ in batch]
    for t in range(N_NEW):
        nxt = D.sample(logits, kw["temperature"], kw["top_k"], token_key(kw["key"], t), kw["step"])
        for b, tok in enumerate(nxt.tolist()):
            want[b].append(tok)
        if t < N_NEW - 1:
            logits = torch.stack([decode_step(tiny, int(nxt[b]), caches[b]) for b in range(len(batch))])
    assert got == want


def test_a_finished_row_ends_and_the_others_do_not_move(tiny, prompts, singles):
    from fault_tolerant_llm_training_amd.generation import generate_batch

    eos = singles[3][N_NEW // 2]  # a token the greedy run of row 3 emits mid-way
    got = generate_batch(tiny, prompts, N_NEW, eos_id=eos)
    assert got[3] == singles[3][: singles[3].index(eos) + 1] and got[3][-1] == eos and len(got[3]) < N_NEW
    for row, full in zip(got, singles):
        assert row == (full[: full.index(eos) + 1] if eos in full else full)


def test_batched_decode_logits_are_as_close_to_fp32_as_the_full_forward():
    """The check of test_generate_gpu.py::test_decode_logits_are_as_close_to_fp32_as_the_full_forward on
    decode_step_rows: two rows teacher-forced with the same 40 tokens, one from a prefill of 1 token, one
    from a prefill of 17 (ragged positions in every step); e_dec_rows <= 2 e_full for both."""
    from fault_tolerant_llm_training_amd.generation import BatchKVCache, decode_step_rows, prefill
    from fault_tolerant_llm_training_amd.models.llama import model_args_for
    from test_generate_gpu import _model_pair, rel

    margs = model_args_for("tiny", vocab_size=512, seq_len=64)
    gpu, cpu = _model_pair(margs)
    torch.manual_seed(9)
    P = 40
    tokens = torch.randint(0, 512, (P,))
    with torch.no_grad():
        ref = cpu(tokens.view(1, -1))[0]
        full = gpu(tokens.view(1, -1).cuda())[0]
    e_full = rel(full.cpu(), ref)
    starts = [1, 17]

    def run():
        cache = BatchKVCache(margs, 2, 64, "cuda", torch.bfloat16)
        rows = [[prefill(gpu, tokens[:s], cache.row(b))] for b, s in enumerate(starts)]
        for t in range(P - 1):  # row 1 runs past the 40 tokens on token 0; those logits are dropped
            feed = [int(tokens[s + t]) if s + t < P else 0 for s in starts]
            lg = decode_step_rows(gpu, feed, cache, t)
            for b, s in enumerate(starts):
                if s + t < P:
                    rows[b].append(lg[b])
        return [torch.stack(r).cpu() for r in rows]

    dec = run()
    assert dec[0].shape[0] == P and dec[1].shape[0] == P - 16
    e0, e1 = rel(dec[0], ref), rel(dec[1], ref[16:])
    print(f"model tiny: e_full {e_full:.3e} e_dec_rows (prefill 1) {e0:.3e} (prefill 17) {e1:.3e}")
    assert e0 <= 2 * e_full
    assert e1 <= 2 * e_full
    again = run()
    assert torch.equal(again[0], dec[0]) and torch.equal(again[1], dec[1])  # bit-reproducible end to end


# ------------------------------------------------------------------------------- train.py
GPU = ["--device", "cuda", "--model", "tiny", "--synthetic-data", "--vocab-size", "1024", "--sequence-length", "128",
       "--batch-size", "2", "--training-steps", "6", "--logging-frequency", "1", "--state-digest", "--prefetch", "1"]
SAMPLE = ["--sample-every", "2", "--sample-tokens", "16", "--sample-temperature", "0.8", "--sample-top-k", "40"]


@pytest.fixture(scope="module")
def train_runs(tmp_path_factory):
    from helpers import run_train

    out = {}
    for name, extra in (("off", []), ("one", SAMPLE), ("three", SAMPLE + ["--sample-count", "3"])):
        d = str(tmp_path_factory.mktemp(name))
        rc, log = run_train(d, "1", GPU + extra + ["--metrics-file", "m.jsonl", "--checkpoint-path",
                                                   os.path.join(d, "ck")], timeout=240)
        assert rc == 0, log
        recs = [json.loads(ln) for ln in open(os.path.join(d, "m.jsonl")).read().splitlines() if ln.strip()]
        out[name] = (log, [r for r in recs if "sample_step" in r])
    return out


def test_training_is_unchanged_by_sample_count(train_runs):
    losses = lambda log: re.findall(r"Training step: (\d+) \| Loss: ([-\d.naninf]+) .*?grad_norm: ([-\d.naninf]+)", log)
    digest = lambda log: re.search(r"State digest at step 6: (params=\w+ exp_avg=\w+ exp_avg_sq=\w+ "
                                   r"optimizer_step=\d+ data_loader=.*)", log).group(1)
    off, three = train_runs["off"][0], train_runs["three"][0]
    assert len(losses(off)) == 6 and losses(off) == losses(three)
    assert digest(off) == digest(three)


def test_three_samples_per_boundary_and_the_first_is_the_single_sample(train_runs):
    log, three = train_runs["three"]
    one = train_runs["one"][1]
    assert [r["sample_step"] for r in three] == [r["sample_step"] for r in one] == [2, 4, 6]
    for a, r in zip(one, three):
        assert len(r["sample_ids"]) == 3 and len(r["sample_text"]) == 3
        assert all(len(ids) == 16 and all(0 <= i < 1024 for i in ids) for ids in r["sample_ids"])
        assert r["sample_ids"][0] == a["sample_ids"] and r["sample_text"][0] == a["sample_text"]
        for b in range(3):
            assert f"Sample {b} at step {r['sample_step']} | {r['sample_text'][b]!r} | 16 tokens | " in log
