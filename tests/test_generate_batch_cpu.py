"""Batched generation on the CPU path: the composed multi-row ops against loops of the one-row
definitions, generate_batch against per-prompt generate in float64, the batch cache, the refusals,
the generate command line with --num-samples and the --sample-count flag of train.py.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from helpers import ROOT, TINY, env_for, run_train

SYN = TINY + ["--synthetic-data", "--vocab-size", "256"]
PROMPTS = [[7], [3, 250], list(range(20, 37)), [5, 9, 200, 1, 1, 8, 77, 131, 12], list(range(20, 37))]


@pytest.fixture(scope="module")
def tiny64():
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    return build_model(model_args_for("tiny", vocab_size=264, seq_len=32), "cpu", torch.float64, seed=7)


@pytest.fixture(scope="module")
def singles(tiny64):
    """generate() of every prompt alone, greedy, 10 tokens: computed once, never changed."""
    from fault_tolerant_llm_training_amd.generation import generate

    return [generate(tiny64, p, 10) for p in PROMPTS]


# ------------------------------------------------------------------------------- composed row ops
def test_composed_row_ops_equal_loops_of_the_one_row_definitions():
    from fault_tolerant_llm_training_amd.models.llama import rope_tables
    from fault_tolerant_llm_training_amd.ops import decode as D

    torch.manual_seed(0)
    R, Kd, N = 5, 24, 7
    x, w, res = torch.randn(R, Kd).double(), torch.randn(N, Kd).double(), torch.randn(R, N).double()
    y = D.gemv_rows(x, w)
    assert y.shape == (R, N)
    assert torch.equal(y, torch.stack([D.gemv(x[r], w) for r in range(R)]))
    assert torch.equal(D.gemv_rows(x, w, res), torch.stack([D.gemv(x[r], w, res[r]) for r in range(R)]))
    w13 = torch.randn(2 * N, Kd).double()
    assert torch.equal(D.gemv_swiglu_rows(x, w13), torch.stack([D.gemv_swiglu(x[r], w13) for r in range(R)]))

    hq, hkv, d, smax, B = 4, 2, 8, 12, 3
    cos, sin = rope_tables(d, smax, 500000.0)
    cos, sin = cos.double(), sin.double()
    positions, t = [0, 5, smax - 2], 1
    pos0 = torch.tensor(positions, dtype=torch.int32)
    qkv = torch.randn(B, (hq + 2 * hkv) * d).double()
    kc, vc = torch.randn(B, hkv, smax, d).double(), torch.randn(B, hkv, smax, d).double()
    q1, k1, v1 = qkv.clone(), kc.clone(), vc.clone()
    D.qkv_append_rows_(qkv, cos, sin, pos0, t, kc, vc, positions)
    for b, p in enumerate(positions):
        D.qkv_append_(q1[b], cos, sin, p + t, k1[b], v1[b])
    assert torch.equal(qkv, q1) and torch.equal(kc, k1) and torch.equal(vc, v1)
    o = D.attn_rows(qkv[:, : hq * d], kc, vc, pos0, t, positions)
    assert o.shape == (B, hq * d)
    want = torch.stack([D.attn(q1[b, : hq * d], k1[b], v1[b], p + t + 1) for b, p in enumerate(positions)])
    assert torch.equal(o, want)


# ------------------------------------------------------------------------------- the batch cache
def test_a_batch_cache_row_filled_by_prefill_equals_a_plain_cache(tiny64):
    from fault_tolerant_llm_training_amd.generation import BatchKVCache, KVCache, prefill

    a = tiny64.model_args
    batch = BatchKVCache(a, 3, 30, "cpu", torch.float64)
    assert batch.k.shape == (a.n_layers, 3, a.kv_heads, 30, a.head_dim) and batch.k[1].is_contiguous()
    plain = KVCache(a, 30, "cpu", torch.float64)
    row = batch.row(1)
    got = prefill(tiny64, PROMPTS[2], row)
    want = prefill(tiny64, PROMPTS[2], plain)
    assert torch.equal(got, want)
    assert row.length == plain.length == batch.lengths[1] == 17 and batch.lengths == [0, 17, 0]
    assert torch.equal(batch.k[:, 1], plain.k) and torch.equal(batch.v[:, 1], plain.v)
    assert not batch.k[:, 0].any() and not batch.k[:, 2].any()  # the other rows are untouched
    batch.copy_row(2, 1)
    assert torch.equal(batch.k[:, 2], plain.k) and batch.lengths == [0, 17, 17]
    assert batch.pos0.dtype == torch.int32 and batch.pos0.tolist() == [0, 17, 17]
    with pytest.raises(ValueError):
        prefill(tiny64, [1], row)  # not empty any more
    with pytest.raises(ValueError):
        BatchKVCache(a, 2, a.seq_len + 1, "cpu", torch.float64)
    with pytest.raises(ValueError):
        BatchKVCache(a, 0, 8, "cpu", torch.float64)


def test_decode_step_rows_equals_decode_step_per_row(tiny64):
    from fault_tolerant_llm_training_amd.generation import BatchKVCache, KVCache, decode_step, decode_step_rows, prefill

    a = tiny64.model_args
    prompts, toks = [PROMPTS[1], PROMPTS[2], PROMPTS[0]], [[4, 9], [100, 3], [263, 0]]
    batch = BatchKVCache(a, 3, 24, "cpu", torch.float64)
    plain = [KVCache(a, 24, "cpu", torch.float64) for _ in prompts]
    for b, p in enumerate(prompts):
        prefill(tiny64, p, batch.row(b))
        prefill(tiny64, p, plain[b])
    for t in range(2):
        got = decode_step_rows(tiny64, [r[t] for r in toks], batch, t)
        want = torch.stack([decode_step(tiny64, toks[b][t], plain[b]) for b in range(3)])
        assert got.shape == (3, a.vocab_size)
        assert torch.equal(got, want), t
    with pytest.raises(ValueError):
        decode_step_rows(tiny64, [1, 1, 1], batch, 5)  # steps are taken in order


# ------------------------------------------------------------------------------- generate_batch
def test_generate_batch_equals_generate_per_prompt(tiny64, singles):
    from fault_tolerant_llm_training_amd.generation import generate_batch

    assert generate_batch(tiny64, PROMPTS, 10) == singles
    assert generate_batch(tiny64, PROMPTS[::-1], 10) == singles[::-1]
    for p, s in zip(PROMPTS, singles):
        assert generate_batch(tiny64, [p], 10) == [s]
    assert generate_batch(tiny64, PROMPTS, 0) == [[] for _ in PROMPTS]


def test_a_finished_row_keeps_its_slot(tiny64, singles):
    from fault_tolerant_llm_training_amd.generation import generate, generate_batch

    eos = singles[3][4]  # emitted mid-way by row 3
    got = generate_batch(tiny64, PROMPTS, 10, eos_id=eos)
    for row, full in zip(got, singles):
        assert row == (full[: full.index(eos) + 1] if eos in full else full)
    assert got[3][-1] == eos and len(got[3]) <= 5
    assert got == [generate(tiny64, p, 10, eos_id=eos) for p in PROMPTS]
    assert generate_batch(tiny64, PROMPTS[::-1], 10, eos_id=eos) == got[::-1]


def test_sampled_rows_are_the_samplers_rows(tiny64):
    from fault_tolerant_llm_training_amd.generation import generate, generate_batch

    kw = dict(temperature=0.8, top_k=40, key=1234, step=3)
    rows = generate_batch(tiny64, [PROMPTS[1]] * 4, 10, **kw)
    assert rows[0] == generate(tiny64, PROMPTS[1], 10, **kw)
    assert len({tuple(r) for r in rows}) > 1  # copies of one prompt: different draws
    assert rows == generate_batch(tiny64, [PROMPTS[1]] * 4, 10, **kw)


def test_refusals(tiny64):
    from fault_tolerant_llm_training_amd.generation import generate_batch

    a = tiny64.model_args
    for bad in ([], [[1]] * 65, [[1], []], [[1], [2] * (a.seq_len - 3)], [[1], [a.vocab_size]], [[1], [-1]]):
        with pytest.raises(ValueError):
            generate_batch(tiny64, bad, 4)
    assert len(generate_batch(tiny64, [[1]] * 64, 1)) == 64
    assert len(generate_batch(tiny64, [[1], [2] * (a.seq_len - 4)], 4)[1]) == 4


# ------------------------------------------------------------------------------- command line
def _run_generate(d, argv):
    r = subprocess.run([sys.executable, "-m", "fault_tolerant_llm_training_amd.generate"] + argv, cwd=ROOT,
                       env=env_for(d, "1"), capture_output=True, text=True, timeout=300)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.slow
def test_cli_num_samples_prints_one_row_per_sample(tmp_path):
    d = str(tmp_path)
    rc, out = run_train(d, "55", SYN + ["--training-steps", "4", "--model-dtype", "fp32", "--save-every", "3",
                                        "--no-async-checkpoint",
                                        "--checkpoint-path", os.path.join(d, "ck")])
    assert rc == 0, out
    path = os.path.join(d, "ck", "checkpoint_55.ckpt")
    assert os.path.exists(path), out
    common = ["--checkpoint", path, "--model", "tiny", "--vocab-size", "256", "--model-dtype", "fp32", "--device",
              "cpu", "--max-new-tokens", "6", "--temperature", "0.9", "--top-k", "20", "--seed", "4"]
    one = ["--prompt-ids", "1,17,200"]
    rc, out, err = _run_generate(d, common + one + ["--json"])
    assert rc == 0, err
    single = json.loads(out.strip().splitlines()[-1])
    assert "row" not in single
    rc, out, err = _run_generate(d, common + one + ["--num-samples", "3", "--json"])
    assert rc == 0, err
    recs = [json.loads(ln) for ln in out.strip().splitlines()]
    assert [r["row"] for r in recs] == [0, 1, 2]
    assert all(r["prompt_ids"] == [1, 17, 200] and len(r["ids"]) == 6 for r in recs)
    assert recs[0]["ids"] == single["ids"]
    assert len({tuple(r["ids"]) for r in recs}) > 1
    # a file of prompts, each repeated; the text mode separates the rows
    pf = os.path.join(d, "prompts.txt")
    with open(pf, "w") as f:
        f.write("1,17,200\n9\n")
    rc, out, err = _run_generate(d, common + ["--prompts-file", pf, "--prompt-ids-file", "--num-samples", "2"])
    assert rc == 0, err
    lines = out.strip().splitlines()
    assert lines[0::2] == [f"--- sample {b} ---" for b in range(4)]
    assert lines[1] == ",".join(str(i) for i in single["ids"])
    rc, out, err = _run_generate(d, common + one + ["--prompts-file", pf])
    assert rc != 0  # the prompt sources exclude each other
    rc, out, err = _run_generate(d, common + one + ["--num-samples", "65"])
    assert rc != 0 and "generate: error:" in err


# ------------------------------------------------------------------------------- trainer flag
def test_sample_count_is_validated_by_the_parser(capsys):
    from fault_tolerant_llm_training_amd.utils.config import get_args

    assert get_args([]).sample_count == 1
    assert get_args(["--sample-every", "5", "--sample-count", "16"]).sample_count == 16
    for bad in (["--sample-every", "5", "--sample-count", "0"], ["--sample-every", "5", "--sample-count", "17"],
                ["--sample-count", "3"]):
        with pytest.raises(SystemExit):
            get_args(bad)
        assert "--sample-count" in capsys.readouterr().err


@pytest.mark.slow
def test_trainer_logs_sample_count_samples_and_trains_the_same(tmp_path):
    sample = ["--sample-every", "2", "--sample-tokens", "8", "--sample-temperature", "0.8", "--sample-top-k", "50"]
    recs, losses = {}, {}
    for name, extra in (("one", sample), ("three", sample + ["--sample-count", "3"])):
        d = str(tmp_path / name)
        os.makedirs(d)
        rc, out = run_train(d, "1", SYN + ["--training-steps", "4", "--logging-frequency", "1", "--model-dtype",
                                           "fp32", "--checkpoint-path", os.path.join(d, "ck"), "--metrics-file",
                                           "m.jsonl"] + extra)
        assert rc == 0, out
        losses[name] = [ln.split("|")[1] for ln in out.splitlines() if "Training step:" in ln]
        recs[name] = [r for r in (json.loads(ln) for ln in open(os.path.join(d, "m.jsonl")) if ln.strip())
                      if "sample_step" in r]
        if name == "three":
            for r in recs[name]:
                for b in range(3):
                    assert f"Sample {b} at step {r['sample_step']} | {r['sample_text'][b]!r} | 8 tokens | " in out
    assert len(losses["one"]) == 4 and losses["one"] == losses["three"]
    assert [r["sample_step"] for r in recs["three"]] == [r["sample_step"] for r in recs["one"]] == [2, 4]
    for one, three in zip(recs["one"], recs["three"]):
        assert len(three["sample_ids"]) == 3 and len(three["sample_text"]) == 3
        assert three["sample_ids"][0] == one["sample_ids"] and three["sample_text"][0] == one["sample_text"]
