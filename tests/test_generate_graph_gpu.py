"""Graph-replayed decoding on the GPU: the device-step ops (step state read from the control block in
device memory, capacity-sized attention grid) against the host-argument ops, bit for bit; DecodeGraph
against the eager loop -- logits per replay, ids, reuse of one capture, EOS, capacity; --sample-graph
runs of train.py.
"""
import json
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
MASK63 = (1 << 63) - 1
KEYS = [0, MASK63, 0x8000000000000001 & MASK63, 0x243F6A8885A308D3 & MASK63]


@pytest.fixture(scope="module")
def K():
    from fault_tolerant_llm_training_amd._native import kernels

    return kernels()


# ------------------------------------------------------------------------------- the cache ops
@pytest.mark.parametrize("hq,hkv,d", [(4, 2, 64), (4, 1, 128)])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_dev_cache_ops_equal_the_host_argument_ops_bit_for_bit(K, hq, hkv, d, dt):
    from fault_tolerant_llm_training_amd.models.llama import rope_tables
    from fault_tolerant_llm_training_amd.ops import decode as D

    dtype, B = DTYPES[dt], 3
    C = int(K.decode_attn_chunk())
    smax = 3 * C + 8  # a grid of 4 chunks, the last one of 8 keys
    cos, sin = (x.cuda() for x in rope_tables(d, smax, 500000.0))
    torch.manual_seed(41)
    kc, vc = (torch.randn(B, hkv, smax, d, device="cuda").to(dtype) for _ in range(2))
    k1, v1 = kc.clone(), vc.clone()
    ctl = D.new_ctl("cuda")
    part = D.attn_part(B, hq, smax, d, "cuda")
    assert part.shape == (B, 4, hq, d + 2)
    o = torch.empty(B, hq * d, device="cuda", dtype=dtype)
    # per-row key counts after the append: a row in 1 chunk of the 4, a row in all of them, rows at a boundary
    for counts, t in (([1, 2 * C + 1, smax], 0), ([C - 1, C, C + 1], 3), ([C + 1, smax, 2 * C + 1], 1),
                      ([C, 3, smax], 2)):
        positions = [n - 1 - t for n in counts]
        pos0 = torch.tensor(positions, dtype=torch.int32, device="cuda")
        D.write_ctl(ctl, t, 0.0, 0, 0, 0)  # the same buffer, rewritten between the calls
        qkv = torch.randn(B, (hq + 2 * hkv) * d, device="cuda").to(dtype)
        q1 = qkv.clone()
        K.decode_qkv_append_rows_dev_(qkv, cos, sin, pos0, ctl, kc, vc)
        K.decode_qkv_append_rows_(q1, cos, sin, pos0, t, max(positions) + t, k1, v1)
        assert torch.equal(qkv, q1), (counts, t)
        assert torch.equal(kc, k1) and torch.equal(vc, v1), (counts, t)  # the whole caches
        part.fill_(float("nan"))  # a merge that read a chunk its row never wrote would show
        o.fill_(float("nan"))
        K.decode_attn_rows_dev(qkv[:, : hq * d], kc, vc, pos0, ctl, part, o)
        want = K.decode_attn_rows(q1[:, : hq * d], k1, v1, pos0, t, max(counts))
        assert torch.equal(o, want), (counts, t)
        for b, n in enumerate(counts):
            assert torch.equal(o[b], K.decode_attn(q1[b, : hq * d].contiguous(), k1[b], v1[b], n)), (counts, t, b)
            used = (n + C - 1) // C
            assert torch.isnan(part[b, used:]).all() and not torch.isnan(part[b, :used]).any()
    assert D.read_ctl(ctl.cpu())[0] == 2  # the ops only read the block
    K.decode_ctl_advance_(ctl)
    assert ctl.tolist() == [3, 0, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("dt", list(DTYPES))
def test_a_position_outside_the_capacity_writes_nothing(K, dt):
    from fault_tolerant_llm_training_amd.models.llama import rope_tables
    from fault_tolerant_llm_training_amd.ops import decode as D

    dtype, B, hq, hkv, d, smax = DTYPES[dt], 4, 4, 2, 64, 40
    cos, sin = (x.cuda() for x in rope_tables(d, smax, 500000.0))
    torch.manual_seed(42)
    kc = torch.full((B, hkv, smax, d), -7.0, device="cuda").to(dtype)
    vc = torch.full((B, hkv, smax, d), 9.0, device="cuda").to(dtype)
    qkv = torch.randn(B, (hq + 2 * hkv) * d, device="cuda").to(dtype)
    q0 = qkv.clone()
    ctl = D.new_ctl("cuda")
    D.write_ctl(ctl, 2, 0.0, 0, 0, 0)
    pos0 = torch.tensor([5, smax - 2, smax + 3, smax - 3], dtype=torch.int32, device="cuda")  # -> 7, 40, 45, 39
    K.decode_qkv_append_rows_dev_(qkv, cos, sin, pos0, ctl, kc, vc)
    for b in (1, 2):  # positions smax and smax + 5: the caches and the row's Q are as they were
        assert (kc[b] == -7.0).all() and (vc[b] == 9.0).all() and torch.equal(qkv[b], q0[b])
    for b, p in ((0, 7), (3, smax - 1)):
        assert torch.equal(vc[b, :, p].reshape(-1), q0[b, (hq + hkv) * d :])
        rest = torch.ones(smax, dtype=torch.bool)
        rest[p] = False
        assert (kc[b][:, rest] == -7.0).all() and (vc[b][:, rest] == 9.0).all() and not (kc[b, :, p] == -7.0).all()
    # RoPE tables shorter than the cache bound the position as well: t = 0 -> 5, 38, 43, 37 against 30 rows
    D.write_ctl(ctl, 0, 0.0, 0, 0, 0)
    K.decode_qkv_append_rows_dev_(qkv, cos[:30].contiguous(), sin[:30].contiguous(), pos0, ctl, kc, vc)
    assert (kc[1] == -7.0).all() and (kc[3, :, 37] == -7.0).all() and (vc[3, :, 37] == 9.0).all()
    assert not (kc[0, :, 5] == -7.0).all()
    with pytest.raises(RuntimeError):
        K.decode_qkv_append_rows_dev_(qkv, cos, sin, pos0, ctl[:4], kc, vc)
    with pytest.raises(RuntimeError):
        K.decode_qkv_append_rows_dev_(qkv, cos, sin, pos0, ctl.long(), kc, vc)
    with pytest.raises(RuntimeError):
        K.decode_attn_rows_dev(qkv[:, : hq * d], kc, vc, pos0, ctl, torch.empty(8, device="cuda"),
                               torch.empty(B, hq * d, device="cuda", dtype=dtype))


# ------------------------------------------------------------------------------- the sampler
@pytest.mark.parametrize("temperature,top_k", [(0.0, 0), (0.8, 0), (0.8, 1), (0.8, 40)])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_sample_dev_draws_what_sample_draws_under_the_token_key(K, dt, temperature, top_k):
    from fault_tolerant_llm_training_amd.generation import token_key
    from fault_tolerant_llm_training_amd.ops import decode as D

    R, V, n_cap, step = 5, 512, 1001, 11
    torch.manual_seed(43)
    logits = (3 * torch.randn(R, V, device="cuda")).to(DTYPES[dt])
    ctl = D.new_ctl("cuda")
    tok = torch.empty(R, 1, dtype=torch.int64, device="cuda")
    out = torch.empty(R, n_cap, dtype=torch.int64, device="cuda")
    want = torch.empty(R, dtype=torch.int64, device="cuda")
    draws = set()
    for key in KEYS:
        for t in (0, 1, 1000):
            tok.fill_(-1)
            out.fill_(-1)
            D.write_ctl(ctl, t, temperature, top_k, key, step)
            K.sample_dev_(logits, ctl, tok, out)
            K.sample_(logits, want, temperature, top_k, token_key(key, t), step)
            assert torch.equal(tok.view(-1), want), (key, t)
            assert torch.equal(out[:, t], want), (key, t)
            out[:, t] = -1
            assert (out == -1).all()
            draws.add(tuple(want.tolist()))
    if temperature > 0 and top_k != 1:
        assert len(draws) > 6  # the keys and token numbers do reach the generator
    else:
        assert len(draws) == 1
    D.write_ctl(ctl, n_cap, temperature, top_k, 0, step)  # a token number outside `out`: tok alone
    out.fill_(-1)
    K.sample_dev_(logits, ctl, tok, out)
    assert (out == -1).all() and (tok >= 0).all()


# ------------------------------------------------------------------------------- DecodeGraph
LENS = [1, 7, 120, 127, 7]  # rows 2 and 3 cross the 128-key chunk boundary while replaying
N_NEW = 40
SAMPLED = dict(temperature=0.8, top_k=40, key=0x5EED, step=7)


def _model(dtype):
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    return build_model(model_args_for("tiny", vocab_size=512, seq_len=320), "cuda", dtype, seed=3)


@pytest.fixture(scope="module")
def tiny():
    return _model(torch.bfloat16)


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(31)
    ps = [torch.randint(0, 512, (n,), generator=g).tolist() for n in LENS]
    ps[4] = list(ps[1])  # two identical prompts: prefilled once
    return ps


@pytest.fixture(scope="module")
def eager(tiny, prompts):
    """The eager loop's ids, greedy and sampled: computed once, left unchanged."""
    from fault_tolerant_llm_training_amd.generation import generate_batch

    return {"greedy": generate_batch(tiny, prompts, N_NEW), "sampled": generate_batch(tiny, prompts, N_NEW, **SAMPLED)}


@pytest.fixture(scope="module")
def dg(tiny):
    from fault_tolerant_llm_training_amd.generation import DecodeGraph

    return DecodeGraph(tiny, len(LENS), max(LENS) + N_NEW)


def _logits_per_replay(model, prompts, n, kw):
    from fault_tolerant_llm_training_amd.generation import (BatchKVCache, DecodeGraph, decode_step_rows, prefill,
                                                            token_key)
    from fault_tolerant_llm_training_amd.ops import decode as D

    g = DecodeGraph(model, len(prompts), max(len(p) for p in prompts) + N_NEW)
    g.begin(prompts, N_NEW, **kw)
    twin = BatchKVCache(model.model_args, len(prompts), g.max_len, "cuda", model.flat.dtype)
    logits = torch.stack([prefill(model, p, twin.row(b)) for b, p in enumerate(prompts)])
    assert torch.equal(g.logits, logits)
    for t in range(n):
        nxt = D.sample(logits, kw.get("temperature", 0.0), kw.get("top_k", 0), token_key(kw.get("key", 0), t),
                       kw.get("step", 0))
        logits = decode_step_rows(model, nxt, twin, t)
        g.replay()
        assert torch.equal(g.tok.view(-1), nxt), t
        assert torch.equal(g.logits, logits), t
    assert torch.equal(g.cache.k, twin.k) and torch.equal(g.cache.v, twin.v)
    assert g.captures == 1 and g.replays == n


def test_logits_after_each_replay_equal_decode_step_rows_bf16(tiny, prompts):
    _logits_per_replay(tiny, prompts, 12, SAMPLED)


def test_logits_after_each_replay_equal_decode_step_rows_fp32(prompts):
    _logits_per_replay(_model(torch.float32), prompts, 12, {})


def test_generate_batch_graph_equals_eager(tiny, prompts, eager):
    from fault_tolerant_llm_training_amd.generation import generate_batch

    assert all(len(r) == N_NEW for r in eager["greedy"])
    assert generate_batch(tiny, prompts, N_NEW, graph=True) == eager["greedy"]
    assert generate_batch(tiny, prompts, N_NEW, graph=True, **SAMPLED) == eager["sampled"]
    assert eager["sampled"][1] != eager["sampled"][4]  # the same prompt in another row: another draw


def test_generate_graph_equals_eager_at_one_row(tiny, prompts, eager):
    from fault_tolerant_llm_training_amd.generation import generate

    for p in (prompts[0], prompts[3]):
        assert generate(tiny, p, N_NEW, graph=True) == generate(tiny, p, N_NEW)
        assert generate(tiny, p, N_NEW, graph=True, **SAMPLED) == generate(tiny, p, N_NEW, **SAMPLED)
    assert generate(tiny, prompts[0], N_NEW, graph=True, **SAMPLED) == eager["sampled"][0]
    assert generate(tiny, prompts[0], 1, graph=True) == eager["greedy"][0][:1]  # the sampler alone, no replay


def test_the_loop_is_a_replay_and_one_capture_serves_other_calls(tiny, prompts, eager, dg, monkeypatch):
    from fault_tolerant_llm_training_amd.generation import generate_batch
    from fault_tolerant_llm_training_amd.ops import decode as D

    other = [prompts[3][:50], prompts[2], prompts[0], prompts[2][:9], prompts[3]]
    kw = dict(temperature=1.1, top_k=0, key=KEYS[3], step=123)
    want_other = generate_batch(tiny, other, 25, **kw)
    want_three = generate_batch(tiny, other[:3], 25, **kw)

    def boom(*a, **k):
        raise AssertionError("an eager decode launch during a replayed loop")

    monkeypatch.setattr(D, "gemv_rows", boom)
    monkeypatch.setattr(D, "gemv_swiglu_rows", boom)
    assert dg.captures == 1
    before = dg.replays
    assert dg.run(prompts, N_NEW, **SAMPLED) == eager["sampled"]
    assert dg.run(prompts, N_NEW) == eager["greedy"]
    assert dg.run(other, 25, **kw) == want_other  # other prompts, key, step, temperature, fewer tokens
    assert dg.run(other[:3], 25, **kw) == want_three  # fewer rows than the capture's batch
    assert dg.run(prompts, N_NEW, **SAMPLED) == eager["sampled"]  # the stale cache of the calls between is unread
    assert dg.captures == 1 and dg.replays - before == 3 * (N_NEW - 1) + 2 * 24


def test_eos_ends_rows_as_the_eager_loop_does(tiny, prompts, eager, dg):
    from fault_tolerant_llm_training_amd.generation import generate_batch

    full = eager["sampled"]
    # a token some row emits first at an index that is no multiple of 16 (between two of the host's looks)
    eos = next(tok for r in full for i, tok in enumerate(r) if i % 16 not in (0, 15) and r.index(tok) == i and i > 2)
    want = generate_batch(tiny, prompts, N_NEW, eos_id=eos, **SAMPLED)
    assert any(len(r) < N_NEW and r[-1] == eos for r in want)
    assert dg.run(prompts, N_NEW, eos_id=eos, **SAMPLED) == want
    assert generate_batch(tiny, prompts, N_NEW, eos_id=eos, graph=True, **SAMPLED) == want
    # an id every row emits: greedy copies of one prompt are identical rows
    same = [prompts[2]] * 3
    rows = generate_batch(tiny, same, N_NEW)
    eos = rows[0][5]
    want = generate_batch(tiny, same, N_NEW, eos_id=eos)
    assert all(r == want[0] and r[-1] == eos and len(r) <= 6 for r in want)
    before = dg.replays
    assert dg.run(same, N_NEW, eos_id=eos) == want
    assert dg.replays - before == 16  # ended at the first look, not after N_NEW tokens


def test_a_request_over_the_capacity_is_refused_before_any_replay(tiny, prompts, dg):
    before = dg.replays
    with pytest.raises(ValueError):
        dg.run(prompts, N_NEW + 1)
    with pytest.raises(ValueError):
        dg.run([prompts[3] + [1]], N_NEW)
    with pytest.raises(ValueError):
        dg.run(prompts + [[1]], 4)  # more rows than the capture's batch
    with pytest.raises(ValueError):
        dg.run([[]], 4)
    assert dg.replays == before and dg.captures == 1
    dg.begin(prompts, N_NEW)
    dg._t = N_NEW  # a host count at the capacity: replay() refuses, as decode_step_rows does
    with pytest.raises(ValueError):
        dg.replay()
    assert dg.replays == before


def test_an_unaligned_vocabulary_decodes_eagerly_under_the_graph_flag(prompts):
    """The device sampler takes rows of a multiple of 8 columns; another vocabulary (the byte tokenizer's
    259) goes to the float64 definition on the host, which no capture can hold: graph=True is the eager
    loop there, and DecodeGraph refuses the model before it opens a capture."""
    from fault_tolerant_llm_training_amd.generation import DecodeGraph, generate, generate_batch, graph_supported
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    model = build_model(model_args_for("tiny", vocab_size=259, seq_len=64), "cuda", torch.bfloat16, seed=3)
    assert not graph_supported(model)
    ps = [[t % 259 for t in p[:9]] for p in prompts[:3]]
    for kw in ({}, SAMPLED):
        want = generate_batch(model, ps, 8, graph=False, **kw)
        assert all(len(r) == 8 and all(0 <= i < 259 for i in r) for r in want)
        assert generate_batch(model, ps, 8, graph=True, **kw) == want
        assert generate(model, ps[1], 8, graph=True, **kw) == generate(model, ps[1], 8, **kw)
    with pytest.raises(ValueError, match="multiple of 8"):
        DecodeGraph(model, 3, 32)
    assert not torch.cuda.is_current_stream_capturing()


# ------------------------------------------------------------------------------- train.py
GPU = ["--device", "cuda", "--model", "tiny", "--synthetic-data", "--vocab-size", "1024", "--sequence-length", "128",
       "--batch-size", "2", "--training-steps", "4", "--logging-frequency", "1", "--state-digest", "--prefetch", "1"]
SAMPLE = ["--sample-every", "2", "--sample-count", "3", "--sample-tokens", "16", "--sample-temperature", "0.8"]


def _train(tmp_path_factory, name, extra):
    from helpers import run_train

    d = str(tmp_path_factory.mktemp(name))
    rc, log = run_train(d, "1", GPU + SAMPLE + extra + ["--metrics-file", "m.jsonl", "--checkpoint-path",
                                                        os.path.join(d, "ck")], timeout=240)
    assert rc == 0, log
    recs = [json.loads(ln) for ln in open(os.path.join(d, "m.jsonl")).read().splitlines() if ln.strip()]
    digest = re.search(r"State digest at step 4: (params=\w+ exp_avg=\w+ exp_avg_sq=\w+ optimizer_step=\d+ "
                       r"data_loader=.*)", log).group(1)
    lines = re.findall(r"(Sample \d at step \d+ \| .* \| \d+ tokens) \|", log)
    return log, [(r["sample_step"], r["sample_ids"], r["sample_text"]) for r in recs if "sample_step" in r], digest, lines


@pytest.mark.parametrize("hip_graph", [[], ["--hip-graph"]], ids=["eager-step", "hip-graph"])
def test_sample_graph_leaves_samples_and_training_state_as_they_were(tmp_path_factory, hip_graph):
    log0, recs0, digest0, lines0 = _train(tmp_path_factory, "plain", hip_graph)
    log1, recs1, digest1, lines1 = _train(tmp_path_factory, "graph", hip_graph + ["--sample-graph"])
    assert "--sample-graph" in log1 and "--sample-graph" not in log0
    # the trainer really replays: one capture at the first boundary, 15 replays for its 16 tokens, and no
    # second capture at the later boundaries
    captured = re.findall(r"Sampling: decode graph captured at step (\d+) \((\d+) rows, capacity (\d+)\); "
                          r"captures (\d+), replays (\d+)", log1)
    assert captured == [("2", "3", "17", "1", "15")], captured
    assert "decode graph captured" not in log0
    assert [r[0] for r in recs0] == [2, 4] and all(len(r[1]) == 3 and len(r[1][0]) == 16 for r in recs0)
    assert recs1 == recs0
    assert lines1 == lines0 and len(lines0) == 6
    assert digest1 == digest0
