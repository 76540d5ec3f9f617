"""Text generation on the CPU path: the KV-cache decode against the full forward in float64, the
sampler's definition, the generate command line, and --sample-every runs of train.py against runs
without it (training untouched, the boundaries, a preempted and resumed chain, the refusals).
"""
import json
import os
import re
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import ROOT, TINY, env_for, kill_group, run_train, start_train, wait_for_log, write_fake_sbatch

SYN = TINY + ["--synthetic-data", "--vocab-size", "256"]
P_LEN = 24


# ------------------------------------------------------------------------------- KV cache
@pytest.fixture(scope="module")
def tiny64():
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    torch.manual_seed(3)
    model = build_model(model_args_for("tiny", vocab_size=264, seq_len=32), "cpu", torch.float64, seed=7)
    tokens = torch.randint(0, 264, (P_LEN,))
    with torch.no_grad():
        full = model(tokens.view(1, -1))[0]  # [P, V]
    return model, tokens, full


def _relerr(a, b):
    return float((a - b).norm() / b.norm())


def _decode_all(model, tokens, prefix: int):
    """Logits at positions prefix-1 .. P-1 (prefix >= 1: prefill of `prefix` tokens first; 0: every
    token through decode_step)."""
    from fault_tolerant_llm_training_amd.generation import KVCache, decode_step, prefill

    cache = KVCache(model.model_args, len(tokens), "cpu", torch.float64)
    rows = []
    if prefix:
        rows.append(prefill(model, tokens[:prefix], cache))
    for t in range(prefix, len(tokens)):
        rows.append(decode_step(model, int(tokens[t]), cache))
    assert cache.length == len(tokens)
    return torch.stack(rows)


def test_teacher_forced_decode_equals_the_full_forward(tiny64):
    model, tokens, full = tiny64
    dec = _decode_all(model, tokens, 0)
    assert dec.shape == full.shape
    for t in range(P_LEN):  # the same math in another order: fp64 epsilon
        assert _relerr(dec[t], full[t]) < 1e-10, t


@pytest.mark.parametrize("P", [1, 7, 23])
def test_prefill_then_decode_equals_decode_from_an_empty_cache(tiny64, P):
    model, tokens, full = tiny64
    got = _decode_all(model, tokens, P)
    want = _decode_all(model, tokens, 0)[P - 1 :]
    assert got.shape == want.shape
    for a, b, f in zip(got, want, full[P - 1 :]):
        assert _relerr(a, b) < 1e-10 and _relerr(a, f) < 1e-10


def test_cache_longer_than_the_rope_tables_is_refused(tiny64):
    from fault_tolerant_llm_training_amd.generation import KVCache, generate

    model = tiny64[0]
    with pytest.raises(ValueError):
        KVCache(model.model_args, model.model_args.seq_len + 1, "cpu", torch.float64)
    with pytest.raises(ValueError):
        generate(model, [1, 2, 3], model.model_args.seq_len - 2)
    assert len(generate(model, [1, 2, 3], model.model_args.seq_len - 3)) == model.model_args.seq_len - 3


def test_generate_greedy_follows_the_full_forward(tiny64):
    from fault_tolerant_llm_training_amd.generation import generate

    model = tiny64[0]
    ids = generate(model, [5, 9], 6)
    seq = [5, 9]
    for _ in range(6):  # greedy by re-running the whole forward
        with torch.no_grad():
            seq.append(int(model(torch.tensor([seq]))[0, -1].argmax()))
    assert ids == seq[2:]
    assert generate(model, [5, 9], 6, eos_id=ids[2]) == ids[: ids.index(ids[2]) + 1]


# ------------------------------------------------------------------------------- sampler oracle
def test_greedy_takes_the_lowest_index_of_a_tie():
    from fault_tolerant_llm_training_amd.utils.sampling import sample_reference

    x = torch.zeros(3, 16)
    x[0, 5] = x[0, 11] = 2.0
    x[1, 15] = x[1, 0] = 1.0
    x[2, 7] = 3.0
    assert sample_reference(x, 0.0, 0, key=1, step=0).tolist() == [5, 0, 7]
    assert sample_reference(x.bfloat16(), 0.0, 4, key=9, step=3).tolist() == [5, 0, 7]


@pytest.mark.parametrize("temperature", [0.1, 0.7, 5.0])
def test_top_k_1_is_greedy_at_any_temperature(temperature):
    from fault_tolerant_llm_training_amd.utils.sampling import sample_reference

    torch.manual_seed(0)
    x = torch.randn(200, 64).bfloat16()  # bf16: ties at the maximum do occur
    x[0, 3] = x[0, 40] = 9.0
    greedy = sample_reference(x, 0.0, 0, key=5, step=1)
    assert torch.equal(sample_reference(x, temperature, 1, key=5, step=1), greedy)


def test_frequencies_match_the_probabilities():
    from fault_tolerant_llm_training_amd.utils.sampling import candidates, sample_reference

    torch.manual_seed(1)
    V, R, T, K = 64, 20000, 0.7, 5
    x = torch.randn(V).double()
    x[10] = x[50] = x.topk(K).values[-1]  # a tie at the k-th value: the lower columns are taken
    cand = candidates(x.numpy()[None], K)[0]
    assert cand.sum() == K
    tied = np.flatnonzero(x.numpy() == float(x[10]))
    assert cand[tied[0]] and not cand[tied[-1]]
    p = np.where(cand, np.exp((x.numpy() - x.numpy().max()) / T), 0.0)
    p /= p.sum()
    tok = sample_reference(x.expand(R, V), T, K, key=0x1234ABCD5678, step=17).numpy()
    counts = np.bincount(tok, minlength=V)
    assert counts[~cand].sum() == 0  # no non-candidate is ever drawn
    for i in np.flatnonzero(cand):
        sigma = (R * p[i] * (1 - p[i])) ** 0.5
        assert abs(counts[i] - R * p[i]) <= 5 * sigma, (i, counts[i], R * p[i], sigma)


def test_the_draw_is_a_function_of_key_step_and_row():
    from fault_tolerant_llm_training_amd.utils.sampling import sample_reference, uniforms

    torch.manual_seed(2)
    x = torch.randn(64, 128)
    a = sample_reference(x, 1.0, 0, key=77, step=5)
    assert torch.equal(a, sample_reference(x, 1.0, 0, key=77, step=5))
    # row r of a batch draws what the same row draws alone at that row index
    u = uniforms(77, 5, 64)
    assert np.array_equal(u[10:20], uniforms(77, 5, 10, row0=10))
    assert 0.0 < u.min() and u.max() < 1.0
    b = sample_reference(x, 1.0, 0, key=77, step=6)  # another step: another stream
    c = sample_reference(x, 1.0, 0, key=78, step=5)
    assert not torch.equal(a, b) and not torch.equal(a, c)
    assert not np.array_equal(u, uniforms(77, 6, 64))


def test_sample_buffer_id_is_mirrored():
    from fault_tolerant_llm_training_amd.utils import sround

    assert sround.BUF_SAMPLE == 3
    src = open(os.path.join(ROOT, "csrc", "kernels", "sround.h")).read()
    assert "SR_BUF_SAMPLE = 3" in src


# ------------------------------------------------------------------------------- command line
def _run_generate(d, argv):
    r = subprocess.run([sys.executable, "-m", "fault_tolerant_llm_training_amd.generate"] + argv, cwd=ROOT,
                       env=env_for(d, "1"), capture_output=True, text=True, timeout=300)
    return r.returncode, r.stdout, r.stderr


@pytest.fixture(scope="module")
def tiny_checkpoint(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gen_ckpt"))
    rc, out = run_train(d, "55", SYN + ["--training-steps", "4", "--model-dtype", "fp32", "--save-every", "3",
                                        "--no-async-checkpoint",
                                        "--checkpoint-path", os.path.join(d, "ck")])
    assert rc == 0, out
    path = os.path.join(d, "ck", "checkpoint_55.ckpt")
    assert os.path.exists(path), out
    return d, path


@pytest.mark.slow
def test_cli_returns_what_generate_returns_on_the_restored_model(tiny_checkpoint):
    from fault_tolerant_llm_training_amd.ckpt.format import load_checkpoint
    from fault_tolerant_llm_training_amd.ckpt.state import restore_model
    from fault_tolerant_llm_training_amd.generation import generate
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for
    from fault_tolerant_llm_training_amd.utils.sround import key_from_seed

    d, path = tiny_checkpoint
    common = ["--checkpoint", path, "--model", "tiny", "--vocab-size", "256", "--model-dtype", "fp32", "--device",
              "cpu", "--prompt-ids", "1,17,200", "--max-new-tokens", "9", "--json"]
    model = build_model(model_args_for("tiny", vocab_size=256, seq_len=32), "cpu", torch.float32)
    restore_model(model, load_checkpoint(path)["model"])
    for extra, kw in ((["--seed", "4"], {}),
                      (["--seed", "4", "--temperature", "0.9", "--top-k", "20"], dict(temperature=0.9, top_k=20))):
        rc, out, err = _run_generate(d, common + extra)
        assert rc == 0, err
        rec = json.loads(out.strip().splitlines()[-1])
        assert set(rec) == {"prompt_ids", "ids", "text", "seconds", "tokens_per_s"}
        assert rec["prompt_ids"] == [1, 17, 200]
        assert rec["ids"] == generate(model, [1, 17, 200], 9, key=key_from_seed(4), **kw)
        assert len(rec["ids"]) == 9 and rec["seconds"] > 0
    # with the byte tokenizer the text is printed; its vocabulary (259) is not the file's
    rc, out, err = _run_generate(d, ["--checkpoint", path, "--model", "tiny", "--vocab-size", "256", "--model-dtype",
                                     "fp32", "--device", "cpu", "--tokenizer-name-or-path", "byte", "--prompt", "ab",
                                     "--max-new-tokens", "4"])
    assert rc == 0, err


@pytest.mark.slow
def test_cli_reports_a_layout_mismatch_as_one_error_line(tiny_checkpoint):
    d, path = tiny_checkpoint
    for bad in (["--model", "gpt2-small", "--vocab-size", "256"], ["--model", "tiny", "--vocab-size", "512"]):
        rc, out, err = _run_generate(d, ["--checkpoint", path, "--model-dtype", "fp32", "--device", "cpu",
                                         "--prompt-ids", "1,2", "--max-new-tokens", "2"] + bad)
        assert rc != 0 and out.strip() == ""
        lines = [ln for ln in err.splitlines() if ln.strip()]
        assert len(lines) == 1 and lines[0].startswith("generate: error:") and "does not fit" in lines[0], err


# ------------------------------------------------------------------------------- trainer
def _losses(out):
    return re.findall(r"Training step: (\d+) \| Loss: ([-\d.naninf]+) .*?grad_norm: ([-\d.naninf]+)", out)


def _digest(out):
    m = re.search(r"State digest at step (\d+): (params=\w+ exp_avg=\w+ exp_avg_sq=\w+ optimizer_step=\d+ "
                  r"data_loader=.*)", out)
    assert m, out
    return m.group(1), m.group(2)


def _samples(out):
    """{step: the line without its timing}."""
    return {int(s): body for s, body in re.findall(r"Sample at step (\d+) \| (.* \| \d+ tokens) \| [\d.]+ s", out)}


SAMPLE = ["--sample-every", "2", "--sample-tokens", "8", "--sample-temperature", "0.8", "--sample-top-k", "50"]


@pytest.mark.slow
def test_training_is_unchanged_by_sampling(tmp_path):
    outs = {}
    for name, extra in (("off", []), ("on", SAMPLE)):
        d = str(tmp_path / name)
        os.makedirs(d)
        rc, out = run_train(d, "1", SYN + ["--training-steps", "5", "--logging-frequency", "1", "--state-digest",
                                           "--model-dtype", "fp32", "--save-every", "3", "--no-async-checkpoint",
                                           "--checkpoint-path", os.path.join(d, "ck"), "--metrics-file", "m.jsonl"]
                            + extra)
        assert rc == 0, out
        outs[name] = (out, d)
    (o0, d0), (o1, d1) = outs["off"], outs["on"]
    assert len(_losses(o0)) == 5 and _losses(o0) == _losses(o1)
    assert _digest(o0) == _digest(o1)
    assert "Sample at step" not in o0 and "Sampling: every 2 steps" in o1
    # boundaries n > 0 with n % 2 == 0, and after the last step
    assert sorted(_samples(o1)) == [2, 4, 5]
    recs = [r for r in (json.loads(ln) for ln in open(os.path.join(d1, "m.jsonl")) if ln.strip()) if "sample_step" in r]
    assert [r["sample_step"] for r in recs] == [2, 4, 5]
    for r in recs:
        assert set(r) == {"sample_step", "sample_ids", "sample_text", "sample_s"} and len(r["sample_ids"]) == 8
        assert _samples(o1)[r["sample_step"]] == f"{r['sample_text']!r} | 8 tokens"
    ca, cb = (torch.load(os.path.join(d_, "ck", "checkpoint_1.ckpt"), map_location="cpu", weights_only=True)
              for d_ in (d0, d1))
    assert ca["training_step"] == cb["training_step"] == 3
    for k in ca["model"]:
        assert torch.equal(ca["model"][k], cb["model"][k]), k
    for i in ca["optimizer"]["state"]:
        for f in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(ca["optimizer"]["state"][i][f], cb["optimizer"]["state"][i][f]), (i, f)
    assert ca["lr_scheduler"] == cb["lr_scheduler"] and ca["data_loader"] == cb["data_loader"]
    assert torch.equal(ca["rng"]["torch"], cb["rng"]["torch"])
    assert set(ca) == set(cb) and ca["meta"].keys() == cb["meta"].keys()  # nothing about it in the file


@pytest.mark.slow
def test_a_resumed_chain_prints_the_samples_of_an_uninterrupted_run(tmp_path):
    base = SYN + ["--training-steps", "6", "--model-dtype", "fp32", "--logging-frequency", "1"] + SAMPLE
    ref_d = str(tmp_path / "ref")
    os.makedirs(ref_d)
    rc, out = run_train(ref_d, "1", base + ["--checkpoint-path", os.path.join(ref_d, "ck")])
    assert rc == 0, out
    ref = _samples(out)
    assert sorted(ref) == [2, 4, 6]
    assert len(set(ref.values())) == 3  # another step: another sample

    d = str(tmp_path / "chain")
    os.makedirs(d)
    write_fake_sbatch(d)
    ck = ["--checkpoint-path", os.path.join(d, "ck")]
    # a SIGUSR1 after the first sample stops the first job at some later boundary
    p = start_train(d, "7001", base + ck + ["--training-steps", "400"])
    try:
        assert wait_for_log(p._log_path, "Sample at step 2"), open(p._log_path).read()
        os.kill(p.pid, signal.SIGUSR1)
        assert p.wait(timeout=120) == 0
    finally:
        kill_group(p)
    out1 = open(p._log_path).read()
    m = re.search(r"Checkpoint saved at step (\d+)", out1)
    assert m, out1
    stopped = int(m.group(1))
    assert 2 <= stopped < 400
    rc, out2 = run_train(d, "7002", base + ck + ["--checkpoint-id", "7001", "--training-steps", str(stopped + 3)])
    assert rc == 0, out2
    # the uninterrupted run of the same length
    rc, out3 = run_train(ref_d, "2", base + ["--checkpoint-path", os.path.join(ref_d, "ck2"), "--training-steps",
                                             str(stopped + 3)])
    assert rc == 0, out3
    want = _samples(out3)
    got = dict(_samples(out1))
    got.update(_samples(out2))
    assert _samples(out2), out2
    for s, body in _samples(out1).items():
        assert want[s] == body, s
    for s, body in _samples(out2).items():
        assert want[s] == body, s
    assert sorted(got) == sorted(want)


def test_refusals(capsys):
    from fault_tolerant_llm_training_amd.utils.config import get_args

    a = get_args([])
    assert (a.sample_every, a.sample_prompt, a.sample_tokens, a.sample_temperature, a.sample_top_k) == \
        (0, None, 64, 0.0, 0)
    assert get_args(["--sample-every", "10", "--sample-tokens", "1024"]).sample_tokens == 1024
    for bad, needle in ((["--sample-every", "-1"], "--sample-every"),
                        (["--sample-every", "5", "--sample-tokens", "0"], "--sample-tokens"),
                        (["--sample-every", "5", "--sample-tokens", "1025"], "--sample-tokens"),
                        (["--sample-every", "5", "--sample-tokens", "64", "--sequence-length", "64"],
                         "--sequence-length")):
        with pytest.raises(SystemExit):
            get_args(bad)
        assert needle in capsys.readouterr().err
    assert get_args(["--sample-every", "5", "--sample-tokens", "63", "--sequence-length", "64"])


@pytest.mark.slow
def test_a_text_prompt_longer_than_the_sequence_is_refused_at_startup(tmp_path):
    from helpers import make_parquet

    d = str(tmp_path)
    pq = os.path.join(d, "t.parquet")
    make_parquet(pq)
    rc, out = run_train(d, "1", TINY + ["--dataset", pq, "--tokenizer-name-or-path", "byte", "--training-steps", "2",
                                        "--sample-every", "1", "--sample-tokens", "20", "--sample-prompt",
                                        "a prompt of more than twelve bytes", "--checkpoint-path",
                                        os.path.join(d, "ck")])
    assert "exceed --sequence-length" in out and "Training step" not in out
