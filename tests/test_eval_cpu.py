"""Held-out evaluation (--eval-every) on the CPU path: the counters' definition, argument
checking, training left untouched, independence of the number of ranks, preemption in the
middle of an evaluation, and the packing dataset as the evaluation set.
"""
import argparse
import json
import os
import re
import signal
import socket

import pytest
import torch
import torch.nn.functional as F

from helpers import TINY, kill_group, make_parquet, run_train, sbatch_calls, start_train, wait_for_log, \
    write_fake_sbatch

SYN = TINY + ["--synthetic-data", "--vocab-size", "256"]
EPS32 = 2.0 ** -23


def _records(path):
    if not os.path.exists(path):
        return []
    return [r for r in (json.loads(ln) for ln in open(path).read().splitlines() if ln.strip()) if "eval_step" in r]


# ------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("T,V", [(1, 8), (5, 24), (37, 50), (64, 264)])
def test_twin_matches_float64_cross_entropy(T, V):
    from fault_tolerant_llm_training_amd.utils.evalacc import FX_ONE, summarize, xent_eval_reference_

    torch.manual_seed(T * 1000 + V)
    logits = (3 * torch.randn(T, V)).bfloat16()
    labels = torch.randint(0, V, (T,))
    labels[0], labels[-1] = 0, V - 1
    if T > 3:
        labels[2] = -100
    acc = torch.zeros(4, dtype=torch.int64)
    xent_eval_reference_(logits, labels, acc)
    live = labels != -100
    ref = F.cross_entropy(logits.double(), labels, reduction="none", ignore_index=-100)
    # first index of the maximum, from its definition
    x = logits.double()
    first = torch.tensor([int((row == row.max()).nonzero()[0]) for row in x])
    assert acc[1].item() == int(live.sum())
    assert acc[2].item() == int((first == labels)[live].sum())
    assert acc[3].item() == 0
    # fp32 rounding of one row's NLL: the V-term sum of exponentials carries at most V eps of
    # relative error (an absolute V eps after the log) and the max / log / two subtractions a few
    # ulps at the magnitude of the logits; the fixed point adds half a unit, 2^-25, per row
    per_row = 2.0 ** -25 + EPS32 * (V + 8) * (1.0 + float(x.abs().max()))
    n = int(live.sum())
    assert abs(acc[0].item() / FX_ONE - float(ref.sum())) <= n * per_row
    s = summarize(acc.tolist())
    assert s["tokens"] == n and s["loss_fx"] == acc[0].item()
    assert abs(s["loss"] - float(ref.sum()) / n) <= per_row


def test_twin_edge_rows_and_accumulation():
    from fault_tolerant_llm_training_amd.utils.evalacc import xent_eval_reference_

    V = 16
    logits = torch.zeros(5, V).bfloat16()
    logits[0, 3] = logits[0, 9] = 2.0   # tie, label at the lower index: a hit
    logits[1, 3] = logits[1, 9] = 2.0   # tie, label at the higher index: not a hit
    logits[2, 5] = float("inf")         # +inf at a non-label column: left out
    logits[3, 1] = 1.0                  # ignored row
    logits[4, 7] = 4.0                  # plain hit
    labels = torch.tensor([3, 9, 2, -100, 7])
    acc = torch.zeros(4, dtype=torch.int64)
    xent_eval_reference_(logits, labels, acc)
    assert acc[1:].tolist() == [3, 2, 1]
    first = acc.clone()
    xent_eval_reference_(logits, labels, acc)  # accumulated, not overwritten
    assert torch.equal(acc, 2 * first)
    ign = torch.full((5,), -100)
    xent_eval_reference_(logits, ign, acc)
    assert torch.equal(acc, 2 * first)


# ------------------------------------------------------------------------------- argument checking
def test_real_data_without_eval_dataset_is_refused(capsys):
    from fault_tolerant_llm_training_amd.utils.config import get_args

    with pytest.raises(SystemExit):
        get_args(["--eval-every", "10"])
    assert "--eval-dataset" in capsys.readouterr().err
    assert get_args(["--eval-every", "10", "--eval-dataset", "held_out.parquet"]).eval_every == 10
    assert get_args(["--eval-every", "10", "--synthetic-data"]).eval_dataset == ""
    a = get_args([])  # off by default; nothing is checked then
    assert a.eval_every == 0 and a.eval_sequences == 32


def test_eval_sequences_must_be_a_multiple_of_batch_size(capsys):
    from fault_tolerant_llm_training_amd.utils.config import get_args

    with pytest.raises(SystemExit):
        get_args(["--eval-every", "10", "--synthetic-data", "--batch-size", "4", "--eval-sequences", "6"])
    assert "--eval-sequences" in capsys.readouterr().err
    assert get_args(["--eval-every", "10", "--synthetic-data", "--batch-size", "4", "--eval-sequences", "8"])


# ------------------------------------------------------------------------------- training unchanged
def _losses(out):
    return re.findall(r"Training step: (\d+) \| Loss: ([-\d.naninf]+) .*?grad_norm: ([-\d.naninf]+)", out)


def _digest(out):
    m = re.search(r"State digest at step (\d+): (params=\w+ exp_avg=\w+ exp_avg_sq=\w+ optimizer_step=\d+ "
                  r"data_loader=.*)", out)
    assert m, out
    return m.group(1), m.group(2)


@pytest.mark.slow
def test_training_is_unchanged_by_evaluation(tmp_path):
    outs = {}
    for every in (0, 2):
        d = str(tmp_path / f"e{every}")
        os.makedirs(d)
        rc, out = run_train(d, "1", SYN + ["--training-steps", "6", "--logging-frequency", "1", "--state-digest",
                                           "--model-dtype", "fp32", "--save-every", "3", "--no-async-checkpoint",
                                           "--checkpoint-path", os.path.join(d, "ck"), "--metrics-file", "m.jsonl",
                                           "--eval-every", str(every), "--eval-sequences", "6"])
        assert rc == 0, out
        outs[every] = (out, d)
    (o0, d0), (o2, d2) = outs[0], outs[2]
    assert len(_losses(o0)) == 6 and _losses(o0) == _losses(o2)
    assert _digest(o0) == _digest(o2)  # params / moments / optimizer step / loader position
    assert _records(os.path.join(d0, "m.jsonl")) == []
    recs = _records(os.path.join(d2, "m.jsonl"))
    assert [r["eval_step"] for r in recs] == [2, 4, 6]
    for r in recs:
        assert set(r) == {"eval_step", "eval_loss", "eval_loss_fx", "eval_tokens", "eval_correct",
                          "eval_nonfinite", "eval_s"}
        assert r["eval_tokens"] == 6 * 32 and r["eval_nonfinite"] == 0
        assert isinstance(r["eval_loss_fx"], int) and r["eval_loss"] == r["eval_loss_fx"] / 2 ** 24 / r["eval_tokens"]
        assert f"Evaluation at step {r['eval_step']} | Loss: {r['eval_loss']:.4f} | Perplexity: " in o2
    assert "Evaluation set: synthetic" in o2 and "Evaluation" not in o0
    # the periodic checkpoint taken at the boundary of step 3 (between the evaluations): same state,
    # LR schedule, loader position and RNG state
    ca, cb = (torch.load(os.path.join(d_, "ck", "checkpoint_1.ckpt"), map_location="cpu", weights_only=True)
              for d_ in (d0, d2))
    assert ca["training_step"] == cb["training_step"]
    for k in ca["model"]:
        assert torch.equal(ca["model"][k], cb["model"][k]), k
    for i in ca["optimizer"]["state"]:
        for f in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(ca["optimizer"]["state"][i][f], cb["optimizer"]["state"][i][f]), (i, f)
    assert ca["lr_scheduler"] == cb["lr_scheduler"] and ca["data_loader"] == cb["data_loader"]
    assert torch.equal(ca["rng"]["torch"], cb["rng"]["torch"])


# ------------------------------------------------------------------------------- rank-count independence
def _eval_args(**kw):
    a = dict(batch_size=2, sequence_length=16, eval_sequences=6, eval_dataset="", synthetic_data=True, seed=11,
             iterable_dataset=False, tokenizer_name_or_path="byte")
    a.update(kw)
    return argparse.Namespace(**a)


def _evaluate_once(rank, world, group, vocab=128, **kw):
    from fault_tolerant_llm_training_amd import evaluation
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    args = _eval_args(**kw)
    m = build_model(model_args_for("tiny", vocab_size=vocab, seq_len=args.sequence_length), "cpu", torch.float32, seed=5)
    es = evaluation.build_eval_set(args, vocab, rank, world, pin=False)
    s, err = evaluation.run_evaluation(m, es, torch.device("cpu"), group=group)
    assert err is None
    return s, es, m


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    from fault_tolerant_llm_training_amd.parallel import dist as fdist

    info = fdist.init_distributed("cpu")
    s, es, _ = _evaluate_once(rank, world, info.ctrl_group)
    s["micro_batches"] = len(es.batches)
    with open(os.path.join(out_dir, f"s{rank}.json"), "w") as f:
        json.dump(s, f)
    fdist.destroy()


@pytest.mark.slow
def test_result_is_independent_of_the_number_of_ranks(tmp_path):
    """3 micro-batches: at W = 2 rank 0 runs two of them and rank 1 one. The parameters are equal
    by construction before any step (same seed), so the step-0 evaluation must agree exactly."""
    import torch.multiprocessing as mp

    one, es, _ = _evaluate_once(0, 1, None)
    assert len(es.batches) == 3 and one["tokens"] == 6 * 16
    mp.start_processes(_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, start_method="spawn")
    two = [json.load(open(tmp_path / f"s{r}.json")) for r in range(2)]
    assert [t["micro_batches"] for t in two] == [2, 1]
    for t in two:  # every rank holds the summed counters
        for k in ("loss_fx", "tokens", "correct", "nonfinite", "loss"):
            assert t[k] == one[k], (k, t[k], one[k])


# ------------------------------------------------------------------------------- preemption
@pytest.mark.slow
def test_sigusr1_during_an_evaluation_abandons_it_and_the_resumed_job_reruns_it(tmp_path):
    """A real SIGUSR1 while the evaluation of step 2 runs: no record for step 2, a checkpoint at step
    2, the normal USR1 exit; the resumed job logs the evaluation of step 2 and every later one with
    the values of an uninterrupted run, and the chain's metrics file has one record per step."""
    base = SYN + ["--training-steps", "4", "--eval-every", "2", "--eval-sequences", "800", "--model-dtype", "fp32",
                  "--metrics-file", "m.jsonl"]
    ref_d = str(tmp_path / "ref")
    os.makedirs(ref_d)
    rc, out = run_train(ref_d, "1", base + ["--checkpoint-path", os.path.join(ref_d, "ck")])
    assert rc == 0, out
    ref = _records(os.path.join(ref_d, "m.jsonl"))
    assert [r["eval_step"] for r in ref] == [2, 4]

    d = str(tmp_path / "chain")
    os.makedirs(d)
    write_fake_sbatch(d)
    ck = ["--checkpoint-path", os.path.join(d, "ck")]
    p = start_train(d, "7001", base + ck)
    try:
        assert wait_for_log(p._log_path, "Evaluating at step 2"), open(p._log_path).read()
        os.kill(p.pid, signal.SIGUSR1)
        assert p.wait(timeout=120) == 0
    finally:
        kill_group(p)
    out1 = open(p._log_path).read()
    assert "Evaluation at step 2 abandoned" in out1, out1
    assert "Evaluation at step 2 | Loss" not in out1
    assert "[EXIT HANDLER] Job timed out, saving checkpoint." in out1
    assert "[EXIT HANDLER] Checkpoint saved at step 2" in out1
    assert sbatch_calls(d) == [[os.path.join(d, "train.sh"), "7001"]]
    assert _records(os.path.join(d, "m.jsonl")) == []
    rc, out2 = run_train(d, "7002", base + ck + ["--checkpoint-id", "7001"])
    assert rc == 0, out2
    assert "Resuming training from training_step 2" in out2
    assert "Evaluation at step 2 | Loss" in out2
    got = _records(os.path.join(d, "m.jsonl"))
    assert [r["eval_step"] for r in got] == [2, 4]  # exactly one record per evaluated step
    for g, r in zip(got, ref):
        for k in ("eval_loss_fx", "eval_tokens", "eval_correct", "eval_nonfinite", "eval_loss"):
            assert g[k] == r[k], (g, r)


# ------------------------------------------------------------------------------- packing dataset
def test_packing_dataset_is_read_from_its_start_at_every_evaluation(tmp_path):
    from fault_tolerant_llm_training_amd import evaluation
    from fault_tolerant_llm_training_amd.data.parquet import IterableParquetDataset
    from fault_tolerant_llm_training_amd.data.tokenizer import ByteTokenizer

    pq = str(tmp_path / "held_out.parquet")
    make_parquet(pq, n_docs=30, seed=4)
    kw = dict(eval_dataset=pq, synthetic_data=False, iterable_dataset=True)
    a, es, m = _evaluate_once(0, 1, None, vocab=264, **kw)
    # the set is the first 6 packed sequences of the file
    it = iter(IterableParquetDataset(pq, ByteTokenizer(), 16, bos_token_id=1))
    want = [next(it) for _ in range(6)]
    assert torch.equal(torch.cat([x for x, _ in es.batches]), torch.stack([x for x, _ in want]))
    assert torch.equal(torch.cat([y for _, y in es.batches]), torch.stack([y for _, y in want]))
    assert 0 < a["tokens"] < 6 * 16  # BOS positions are masked
    # a second evaluation with no training step in between, and one on a set built anew
    b, _ = evaluation.run_evaluation(m, es, torch.device("cpu"))
    c, _ = evaluation.run_evaluation(m, evaluation.build_eval_set(_eval_args(**kw), 264, 0, 1, pin=False),
                                     torch.device("cpu"))
    for other in (b, c):
        for k in ("loss_fx", "tokens", "correct", "nonfinite"):
            assert other[k] == a[k]
    # map-style reading of the same file: micro-batch i of rank r is samples of micro-batch i
    kw["iterable_dataset"] = False
    whole = evaluation.build_eval_set(_eval_args(**kw), 264, 0, 1, pin=False)
    parts = [evaluation.build_eval_set(_eval_args(**kw), 264, r, 2, pin=False) for r in range(2)]
    assert torch.equal(whole.batches[0][0], parts[0].batches[0][0])
    assert torch.equal(whole.batches[1][0], parts[1].batches[0][0])
    assert torch.equal(whole.batches[2][1], parts[0].batches[1][1])
