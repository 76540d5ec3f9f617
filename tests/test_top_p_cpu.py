"""Nucleus (top-p) sampling on the CPU path: the float64 definition (utils/sampling.py), the control
block, the composed ops, generate / generate_batch on the tiny preset, the parsers, and a
--sample-top-p run of train.py against a run without sampling.
"""
import math
import os
import re
import struct

import numpy as np
import pytest
import torch

from helpers import TINY, run_train

SYN = TINY + ["--synthetic-data", "--vocab-size", "256"]
BAD_TOP_P = [0.0, -0.1, 1.5, float("nan")]


@pytest.fixture(scope="module")
def logits():
    torch.manual_seed(17)
    return 2.5 * torch.randn(64, 512, dtype=torch.float64)


# ------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("temperature,top_k", [(0.0, 0), (0.8, 40), (1.0, 0)])
def test_top_p_1_is_the_call_without_the_keyword(logits, temperature, top_k):
    from fault_tolerant_llm_training_amd.utils.sampling import sample_reference

    tok, margin = sample_reference(logits, temperature, top_k, 0x5EED, 9, return_margin=True)
    tok1, margin1 = sample_reference(logits, temperature, top_k, 0x5EED, 9, return_margin=True, top_p=1.0)
    assert torch.equal(tok, tok1) and np.array_equal(margin, margin1)
    assert torch.equal(sample_reference(logits, temperature, top_k, 0x5EED, 9, top_p=1.0), tok)
    res = sample_reference(logits, temperature, top_k, 0x5EED, 9, return_margin=True, top_p=1.0,
                           return_nucleus_margin=True)
    assert len(res) == 3 and np.array_equal(res[1], margin) and np.isinf(res[2]).all()


@pytest.mark.parametrize("top_k", [0, 7])
@pytest.mark.parametrize("temperature", [0.3, 5.0])
def test_a_tiny_top_p_is_greedy(logits, temperature, top_k):
    """top_p * W <= 1e-6 * 512 < 1, the weight of the row maximum: the nucleus is that column alone."""
    from fault_tolerant_llm_training_amd.utils.sampling import nucleus, sample_reference

    greedy = sample_reference(logits, 0.0, 0, 1, 2)
    assert torch.equal(sample_reference(logits, temperature, top_k, 1, 2, top_p=1e-6), greedy)
    nuc = nucleus(logits.numpy(), temperature, top_k, 1e-6)
    assert (nuc.sum(axis=1) == 1).all() and nuc[np.arange(64), greedy.numpy()].all()
    # greedy stays greedy whatever top_p is
    assert torch.equal(sample_reference(logits, 0.0, top_k, 1, 2, top_p=0.5), greedy)


def test_a_row_checked_by_hand():
    from fault_tolerant_llm_training_amd.utils.sampling import nucleus, sample_reference

    p = [0.5, 0.25, 0.125, 0.0625, 0.0625]
    row = torch.full((8,), -math.inf, dtype=torch.float64)
    row[:5] = torch.tensor(p, dtype=torch.float64).log()
    for top_p, size in ((0.4, 1), (0.6, 2), (0.8, 3), (0.9, 4)):
        nuc = nucleus(row.view(1, -1).numpy(), 1.0, 0, top_p)
        assert nuc.shape == (1, 8) and nuc[0].tolist() == [True] * size + [False] * (8 - size), top_p
    R = 4096
    tok, margin, nmargin = sample_reference(row.expand(R, 8), 1.0, 0, 0xABCDEF, 5, return_margin=True, top_p=0.8,
                                            return_nucleus_margin=True)
    # 0.8 lies between the cumulative sums 0.75 and 0.875
    assert np.allclose(nmargin, 0.05, atol=1e-6) and (margin >= 0).all()
    freq = np.bincount(tok.numpy(), minlength=8) / R
    assert freq[3:].sum() == 0
    for i, q in enumerate((4 / 7, 2 / 7, 1 / 7)):
        assert abs(freq[i] - q) <= 4 * math.sqrt(q * (1 - q) / R), (i, freq[i], q)


TIED = [3, 9, 10, 21, 33, 40, 58, 63]


def tied_row(V, cols=TIED, dtype=torch.float64):
    row = torch.full((V,), -100.0, dtype=dtype)
    row[cols] = 0.0
    return row


def test_ties_at_the_nucleus_boundary_go_to_the_lower_columns():
    from fault_tolerant_llm_training_amd.utils.sampling import nucleus, sample_reference

    row = tied_row(64)
    nuc = nucleus(row.view(1, -1).numpy(), 1.0, 0, 0.45)  # 0.45 * 8 = 3.6: four of the eight
    assert np.nonzero(nuc[0])[0].tolist() == TIED[:4]
    tok = sample_reference(row.expand(2048, 64), 1.0, 0, 77, 1, top_p=0.45)
    assert sorted(set(tok.tolist())) == TIED[:4]
    # the top-k tie rule comes first: of the 6 lowest tied columns, 0.45 * 6 = 2.7 takes three
    nuc = nucleus(row.view(1, -1).numpy(), 1.0, 6, 0.45)
    assert np.nonzero(nuc[0])[0].tolist() == TIED[:3]


def test_nan_columns_never_enter_and_top_k_comes_first():
    from fault_tolerant_llm_training_amd.utils.sampling import candidates, nucleus

    torch.manual_seed(2)
    x = torch.randn(16, 64, dtype=torch.float64).numpy()
    x[:, 5] = np.nan
    for top_k in (0, 9):
        nuc = nucleus(x, 0.7, top_k, 0.8)
        cand = candidates(x, top_k)
        assert not nuc[:, 5].any() and (nuc <= cand).all() and (nuc.sum(axis=1) >= 1).all()
        # a prefix of the descending order: every column inside is >= every candidate left outside
        for r in range(16):
            assert x[r][nuc[r]].min() >= np.where(cand[r] & ~nuc[r], x[r], -np.inf).max()
            w = np.where(cand[r], np.exp((x[r] - np.nanmax(x[r])) / 0.7), 0.0)
            inside = w[nuc[r]]
            assert inside.sum() >= np.float32(0.8) * w.sum() * (1 - 1e-12)
            assert inside.sum() - inside.min() < np.float32(0.8) * w.sum()  # the shortest such prefix


# ------------------------------------------------------------------------------- validation
@pytest.mark.parametrize("bad", BAD_TOP_P)
def test_a_top_p_outside_0_1_is_refused(bad, capsys):
    from fault_tolerant_llm_training_amd import generate as G
    from fault_tolerant_llm_training_amd.ops import decode as D
    from fault_tolerant_llm_training_amd.utils.config import get_args
    from fault_tolerant_llm_training_amd.utils.sampling import nucleus, sample_reference

    x = torch.zeros(2, 8, dtype=torch.float64)
    with pytest.raises(ValueError):
        sample_reference(x, 0.8, 0, 1, 2, top_p=bad)
    with pytest.raises(ValueError):
        nucleus(x.numpy(), 0.8, 0, bad)
    with pytest.raises(ValueError):
        D.write_ctl(D.new_ctl("cpu"), 0, 0.8, 0, 1, 2, top_p=bad)
    with pytest.raises(ValueError):
        D.sample(x, 0.8, 0, 1, 2, top_p=bad)
    with pytest.raises(SystemExit):
        get_args(["--sample-every", "5", f"--sample-top-p={bad}"])
    assert "--sample-top-p" in capsys.readouterr().err
    # generate.py reports its refusals as one error line and exit status 2, before it opens the file
    rc = G.main(["--checkpoint", "/nonexistent.ckpt", "--prompt-ids", "1", "--vocab-size", "256", "--temperature", "0.8",
                 f"--top-p={bad}"])
    assert rc == 2 and "--top-p" in capsys.readouterr().err


def test_a_top_p_that_rounds_to_zero_in_float32_is_refused_by_the_parsers_too(capsys):
    from fault_tolerant_llm_training_amd import generate as G
    from fault_tolerant_llm_training_amd.ops import decode as D
    from fault_tolerant_llm_training_amd.utils.config import get_args

    with pytest.raises(ValueError):
        D.write_ctl(D.new_ctl("cpu"), 0, 0.8, 0, 1, 2, top_p=1e-50)
    with pytest.raises(SystemExit):
        get_args(["--sample-every", "5", "--sample-top-p", "1e-50"])
    assert "--sample-top-p" in capsys.readouterr().err
    rc = G.main(["--checkpoint", "/nonexistent.ckpt", "--prompt-ids", "1", "--vocab-size", "256", "--top-p", "1e-50"])
    assert rc == 2 and "--top-p" in capsys.readouterr().err
    assert get_args(["--sample-every", "5", "--sample-top-p", "1e-30"]).sample_top_p == 1e-30


def test_the_flags_exist_and_default_to_off():
    from fault_tolerant_llm_training_amd import generate as G
    from fault_tolerant_llm_training_amd.utils.config import get_args

    assert get_args([]).sample_top_p == 1.0
    assert get_args(["--sample-every", "5", "--sample-top-p", "0.9"]).sample_top_p == 0.9
    assert G.build_parser().parse_args(["--checkpoint", "x"]).top_p == 1.0
    assert G.build_parser().parse_args(["--checkpoint", "x", "--top-p", "0.9"]).top_p == 0.9


# ------------------------------------------------------------------------------- control block
def test_control_block_carries_top_p_in_word_6():
    from fault_tolerant_llm_training_amd.ops import decode as D

    assert D.CTL_TOP_P == 6 and D.CTL_WORDS == 8
    ctl = D.new_ctl("cpu")
    D.write_ctl(ctl, 3, 0.8, 40, 0x1234567890ABCDEF & ((1 << 63) - 1), 11)
    assert int(ctl[6]) == 0 and int(ctl[7]) == 0 and D.read_ctl_top_p(ctl) == 1.0
    before = D.read_ctl(ctl)
    D.write_ctl(ctl, 3, 0.8, 40, 0x1234567890ABCDEF & ((1 << 63) - 1), 11, top_p=0.9)
    f32 = struct.unpack("<f", struct.pack("<f", 0.9))[0]
    assert D.read_ctl_top_p(ctl) == f32 == float(np.float32(0.9))
    assert (int(ctl[6]) & 0xFFFFFFFF) == struct.unpack("<I", struct.pack("<f", 0.9))[0] and int(ctl[7]) == 0
    assert len(before) == 5 and D.read_ctl(ctl) == before  # the 5-tuple is what it was
    D.write_ctl(ctl, 3, 0.8, 40, 1, 11, top_p=1.0)
    assert int(ctl[6]) == 0


@pytest.mark.parametrize("temperature,top_k", [(0.0, 0), (0.8, 0), (0.8, 40)])
def test_composed_sample_dev_equals_sample_with_the_token_key(temperature, top_k):
    from fault_tolerant_llm_training_amd.generation import token_key
    from fault_tolerant_llm_training_amd.ops import decode as D
    from fault_tolerant_llm_training_amd.utils.sampling import sample_reference

    torch.manual_seed(43)
    R, V, n_cap, step, key = 5, 512, 6, 11, 0x243F6A8885A308D3 & ((1 << 63) - 1)
    x = 3 * torch.randn(R, V, dtype=torch.float64)
    ctl = D.new_ctl("cpu")
    tok = torch.empty(R, 1, dtype=torch.int64)
    out = torch.full((R, n_cap), -1, dtype=torch.int64)
    differs = False
    for t in range(4):
        D.write_ctl(ctl, t, temperature, top_k, key, step, top_p=0.9)
        D.sample_dev_(x, ctl, tok, out)
        want = D.sample(x, temperature, top_k, token_key(key, t), step, top_p=0.9)
        assert torch.equal(want, sample_reference(x, temperature, top_k, token_key(key, t), step, top_p=0.9))
        assert torch.equal(tok.view(-1), want) and torch.equal(out[:, t], want), t
        differs |= not torch.equal(want, D.sample(x, temperature, top_k, token_key(key, t), step))
        D.write_ctl(ctl, t, temperature, top_k, key, step)  # word 6 left at 0: the call without top_p
        D.sample_dev_(x, ctl, tok, out)
        assert torch.equal(tok.view(-1), D.sample(x, temperature, top_k, token_key(key, t), step)), t
    assert differs == (temperature > 0)  # 20 draws: top_p does reach the sampler


# ------------------------------------------------------------------------------- the model level
PROMPTS = [[7], [3, 250], list(range(20, 37)), [3, 250]]
N_NEW = 10


@pytest.fixture(scope="module")
def tiny64():
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    return build_model(model_args_for("tiny", vocab_size=264, seq_len=32), "cpu", torch.float64, seed=7)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph-flag"])
def test_batch_rows_draw_as_the_samplers_rows_under_top_p(tiny64, graph):
    from fault_tolerant_llm_training_amd.generation import (KVCache, decode_step, generate, generate_batch, prefill,
                                                            token_key)
    from fault_tolerant_llm_training_amd.utils.sampling import sample_reference

    kw = dict(temperature=0.8, top_k=0, key=0x5EED, step=7)
    got = generate_batch(tiny64, PROMPTS, N_NEW, graph=graph, top_p=0.9, **kw)
    assert got[0] == generate(tiny64, PROMPTS[0], N_NEW, graph=graph, top_p=0.9, **kw)
    assert got[1] != got[3]  # the same prompt in another row: another draw
    assert got != generate_batch(tiny64, PROMPTS, N_NEW, **kw)  # and not the draws without top_p
    caches = [KVCache(tiny64.model_args, len(p) + N_NEW, "cpu", torch.float64) for p in PROMPTS]
    logits = torch.stack([prefill(tiny64, p, c) for p, c in zip(PROMPTS, caches)])
    want = [[] for _ in PROMPTS]
    for t in range(N_NEW):
        nxt = sample_reference(logits, kw["temperature"], kw["top_k"], token_key(kw["key"], t), kw["step"], top_p=0.9)
        for b, tok in enumerate(nxt.tolist()):
            want[b].append(tok)
        if t < N_NEW - 1:
            logits = torch.stack([decode_step(tiny64, int(nxt[b]), caches[b]) for b in range(len(PROMPTS))])
    assert got == want


# ------------------------------------------------------------------------------- trainer
def _losses(out):
    return re.findall(r"Training step: (\d+) \| Loss: ([-\d.naninf]+) .*?grad_norm: ([-\d.naninf]+)", out)


def _digest(out):
    m = re.search(r"State digest at step (\d+): (params=\w+ exp_avg=\w+ exp_avg_sq=\w+ optimizer_step=\d+ "
                  r"data_loader=.*)", out)
    assert m, out
    return m.group(1), m.group(2)


def _samples(out):
    return {int(s): body for s, body in re.findall(r"Sample at step (\d+) \| (.* \| \d+ tokens) \| [\d.]+ s", out)}


SAMPLE = ["--sample-every", "2", "--sample-tokens", "8", "--sample-temperature", "0.8"]


@pytest.mark.slow
def test_training_is_unchanged_by_top_p_sampling_and_the_log_names_it(tmp_path):
    outs = {}
    for name, extra in (("off", []), ("plain", SAMPLE), ("top_p", SAMPLE + ["--sample-top-p", "0.9"])):
        d = str(tmp_path / name)
        os.makedirs(d)
        rc, out = run_train(d, "1", SYN + ["--training-steps", "4", "--logging-frequency", "1", "--state-digest",
                                           "--model-dtype", "fp32", "--save-every", "3", "--no-async-checkpoint",
                                           "--checkpoint-path", os.path.join(d, "ck")] + extra)
        assert rc == 0, out
        outs[name] = (out, d)
    o_off, o_plain, o_p = outs["off"][0], outs["plain"][0], outs["top_p"][0]
    assert len(_losses(o_off)) == 4 and _losses(o_off) == _losses(o_plain) == _losses(o_p)
    assert _digest(o_off) == _digest(o_plain) == _digest(o_p)
    assert "(temperature 0.8, top-k 0, top-p 0.9; key " in o_p
    assert "(temperature 0.8, top-k 0; key " in o_plain and "top-p" not in o_plain  # today's line
    assert sorted(_samples(o_p)) == sorted(_samples(o_plain)) == [2, 4]
    assert _samples(o_p) != _samples(o_plain)
    ca, cb = (torch.load(os.path.join(outs[n][1], "ck", "checkpoint_1.ckpt"), map_location="cpu", weights_only=True)
              for n in ("off", "top_p"))
    assert ca["training_step"] == cb["training_step"] == 3
    for k in ca["model"]:
        assert torch.equal(ca["model"][k], cb["model"][k]), k
    for i in ca["optimizer"]["state"]:
        for f in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(ca["optimizer"]["state"][i][f], cb["optimizer"]["state"][i][f]), (i, f)
    assert torch.equal(ca["rng"]["torch"], cb["rng"]["torch"]) and set(ca) == set(cb)
