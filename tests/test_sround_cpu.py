"""Stochastic rounding of the bf16 AdamW stores (--stochastic-rounding), the layers that run without
a GPU: the oracle (utils/sround.py, the twin of csrc/kernels/sround.h), the CPU optimizer path
(_adamw_reference), the stagnation this flag cures, and train.py end to end on the tiny preset
(resume, data parallel over gloo, argument checking, checkpoint meta)."""
import math
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import ROOT, TINY, env_for, run_train, write_fake_sbatch

from fault_tolerant_llm_training_amd.optim.adamw import _adamw_reference
from fault_tolerant_llm_training_amd.utils import sround
from fault_tolerant_llm_training_amd.utils.sround import key_from_seed, sr_round_bf16

KEY = key_from_seed(1234)
OK_STATS = torch.tensor([0.0, 1.0, 0.0])  # [norm, clip coefficient 1, finite]


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16)


# ------------------------------------------------------------------ the oracle
def test_philox_known_answer():
    """The generator is Philox4x32: at the full 10 rounds it reproduces Random123's known answer
    for the all-zero counter and key (the product runs it at sround.ROUNDS)."""
    old = sround.ROUNDS
    try:
        sround.ROUNDS = 10
        w = sround.philox_words(0, 0, 0, np.zeros(1, dtype=np.uint64))[0]
    finally:
        sround.ROUNDS = old
    assert [int(v) for v in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert sround.ROUNDS == 6


def test_representable_values_and_non_finite_are_preserved():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(4096, generator=g) * 3).to(torch.bfloat16)
    x[:4] = torch.tensor([0.0, -0.0, 1.0, -2.5]).to(torch.bfloat16)
    y = sr_round_bf16(x.float(), KEY, 7, 0, 0)
    assert torch.equal(_bits(y), _bits(x))
    special = torch.tensor([float("inf"), float("-inf"), float("nan"), -float("nan")])
    y = sr_round_bf16(special, KEY, 7, 1, 8)
    assert y[0] == float("inf") and y[1] == float("-inf") and torch.isnan(y[2:]).all()


def test_result_is_one_of_the_two_neighbours():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1 << 16, generator=g) * torch.logspace(-20, 20, 1 << 16, base=2.0)
    y = sr_round_bf16(x, KEY, 3, 2, 0).float()
    u = x.view(torch.int32)
    down = (u & ~0xFFFF).view(torch.float32)          # truncation: the neighbour towards zero
    up = ((u & ~0xFFFF) + 0x10000).view(torch.float32)  # one bf16 step away from zero
    assert ((y == down) | (y == up)).all()
    assert (y == down).any() and (y == up).any()


def test_bits_are_a_function_of_key_step_buffer_index():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(4096, generator=g)
    base = sr_round_bf16(x, KEY, 5, 0, 64)
    assert torch.equal(_bits(base), _bits(sr_round_bf16(x.clone(), KEY, 5, 0, 64)))
    # the bits belong to the global index, not to the position in the call: a piece in the middle
    assert torch.equal(_bits(base[100:1000]), _bits(sr_round_bf16(x[100:1000], KEY, 5, 0, 164)))
    # each of the four inputs matters. Two independent roundings of one value differ with probability
    # 2 f (1 - f), f the fractional position between the neighbours: 1/3 on average over uniform f,
    # so about 1365 of 4096; a quarter of that is far below any chance fluctuation (sigma ~ 30)
    others = [sr_round_bf16(x, key_from_seed(1235), 5, 0, 64), sr_round_bf16(x, KEY, 6, 0, 64),
              sr_round_bf16(x, KEY, 5, 1, 64), sr_round_bf16(x, KEY, 5, 0, 72),
              sr_round_bf16(x, KEY, 5, 0, 64 + (1 << 35))]
    for o in others:
        assert (_bits(o) != _bits(base)).sum().item() > 340


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_unbiased_at_one_eighth(sign):
    """2^20 copies of +-(1 + 2^-10): 1/8 of the way from 1.0 to the next bf16 (1 + 2^-7). The count
    rounded away from zero is Binomial(N, 1/8) if the bits are uniform: 5 sigma of that."""
    n = 1 << 20
    x = torch.full((n,), sign * (1.0 + 2.0 ** -10))
    y = sr_round_bf16(x, KEY, 11, 0, 0).float()
    p = 1.0 / 8.0
    sigma = math.sqrt(p * (1 - p) / n)  # 3.2e-4
    frac = (y.abs() > 1.0).float().mean().item()
    assert set(y.abs().unique().tolist()) <= {1.0, 1.0 + 2.0 ** -7}
    assert abs(frac - p) <= 5 * sigma, (frac, sigma)


# ------------------------------------------------------------------ the CPU optimizer path
def _state(n, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    p = (torch.randn(n, generator=g) * 0.02).to(dtype)
    gr = (torch.randn(n, generator=g) * 1e-3).to(dtype)
    m = (torch.randn(n, generator=g) * 1e-3).to(dtype)
    v = (torch.rand(n, generator=g) * 1e-6).to(dtype)
    return p, gr, m, v


def test_reference_partition_invariance():
    n = 3 * 2048 + 8
    hp = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, step=4)
    p, g, m, v = _state(n, 3)
    _adamw_reference(p, g, m, v, OK_STATS, sr=(KEY, 0), **hp)
    q, g2, m2, v2 = _state(n, 3)
    for lo, hi in ((0, 2048), (2048, 4096), (4096, n)):
        _adamw_reference(q[lo:hi], g2[lo:hi], m2[lo:hi], v2[lo:hi], OK_STATS, sr=(KEY, lo), **hp)
    for a, b in ((p, q), (m, m2), (v, v2)):
        assert torch.equal(_bits(a), _bits(b))
    # and it is not the round-to-nearest result
    r, g3, m3, v3 = _state(n, 3)
    _adamw_reference(r, g3, m3, v3, OK_STATS, **hp)
    assert not torch.equal(_bits(r), _bits(p))


def test_reference_refuses_other_parameter_dtypes():
    for dt in (torch.float16, torch.float32, torch.float64):
        p, g, m, v = _state(64, 4, dt)
        with pytest.raises(ValueError, match="bf16 parameters only"):
            _adamw_reference(p, g, m, v, OK_STATS, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, sr=(KEY, 0))


def test_reference_fp32_moments_are_stored_as_without_the_flag():
    hp = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, step=2)
    p, g, m, v = _state(1024, 5)
    m, v = m.float(), v.float()
    q, _, m2, v2 = p.clone(), None, m.clone(), v.clone()
    _adamw_reference(p, g, m, v, OK_STATS, sr=(KEY, 0), **hp)
    _adamw_reference(q, g, m2, v2, OK_STATS, **hp)
    assert torch.equal(m, m2) and torch.equal(v, v2) and not torch.equal(_bits(p), _bits(q))


# ------------------------------------------------------------------ stagnation
STAG_N, STAG_STEPS, STAG_LR, STAG_G = 65536, 200, 5e-5, 1e-3


def stagnation_start():
    g = torch.Generator().manual_seed(1234)
    return (torch.randn(STAG_N, generator=g) * 0.02).to(torch.bfloat16)


def stagnation_bound(w0: torch.Tensor) -> float:
    """Allowed |mean change (SR, bf16 state) - mean change (fp32 state)| after STAG_STEPS steps.

    Rounding noise of the parameter store: each step's error is zero-mean with variance
    f (1 - f) s^2 <= s^2 / 4, s the bf16 spacing at the parameter (2^-7 of its binade), independent
    over steps and elements. An element stays below |w0| + T lr (1 + 2^-6) (the step is lr m^/sqrt(v^),
    within 2^-6 of lr under the moments' rounding), so s_i <= spacing there, and the mean over n
    elements has sigma <= sqrt(T mean(s_i^2) / 4 / n). 5 sigma of that.

    The bf16 moments add a second-order bias: m^ is exact in expectation (linear), but
    1/sqrt(v (1 + d)) ~ 1 - d/2 + 3/8 d^2 has mean 1 + 3/8 E[d^2]; d accumulates at most T roundings
    of relative variance <= (2^-7)^2 / 4, so the mean step is off by <= 3/8 T 2^-14 / 4 relative."""
    T = STAG_STEPS
    reach = w0.float().abs() + T * STAG_LR * (1 + 2.0 ** -6)
    spacing = torch.exp2(torch.floor(torch.log2(reach)) - 7).double()
    sigma = math.sqrt(T * spacing.pow(2).mean().item() / 4 / w0.numel())
    bias = 3.0 / 8.0 * T * 2.0 ** -14 / 4 * (T * STAG_LR)
    return 5 * sigma + bias


def run_recipe(w0, update, sr: bool, fp32_state: bool = False):
    """STAG_STEPS AdamW steps of the stagnation recipe through ``update(p, g, m, v, step, sr)``."""
    dt = torch.float32 if fp32_state else torch.bfloat16
    p = w0.to(dt).clone()
    g = torch.full_like(p, STAG_G)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(1, STAG_STEPS + 1):
        update(p, g, m, v, step, sr)
    return p


def cpu_update(p, g, m, v, step, sr):
    _adamw_reference(p, g, m, v, OK_STATS, STAG_LR, 0.9, 0.999, 1e-8, 0.0, step, sr=(KEY, 0) if sr else None)


_cache = {}


def stagnation_reference():
    """(w0, fp32-state final parameters, CPU stochastic-rounding final parameters), computed once."""
    if not _cache:
        w0 = stagnation_start()
        _cache["v"] = (w0, run_recipe(w0, cpu_update, False, fp32_state=True), run_recipe(w0, cpu_update, True))
    return _cache["v"]


def test_round_to_nearest_stagnates():
    """The defect: at lr 5e-5 a full-size step is below half a bf16 spacing for every |w| >= 2^-6."""
    w0 = stagnation_start()
    p = run_recipe(w0, cpu_update, False)
    same = (_bits(p) == _bits(w0)).float().mean().item()
    print(f"round-to-nearest: {same:.3f} of the parameters bit-identical after {STAG_STEPS} steps")
    assert same > 1.0 / 3.0


def test_stochastic_rounding_moves_every_parameter_by_the_right_amount():
    w0, p32, psr = stagnation_reference()
    want = (p32 - w0.float()).double().mean().item()  # ~ -200 * 5e-5 = -0.01
    got = (psr.float() - w0.float()).double().mean().item()
    bound = stagnation_bound(w0)
    same = (_bits(psr) == _bits(w0)).float().mean().item()
    print(f"mean change: fp32 state {want:.6e}, stochastic rounding {got:.6e}, bound {bound:.2e}; unchanged {same:.4f}")
    assert abs(want + STAG_STEPS * STAG_LR) < 1e-4  # the recipe itself: 200 full-size steps
    assert bound < 0.01 * STAG_STEPS * STAG_LR  # the check resolves 1 % of the movement
    assert abs(got - want) <= bound
    assert same < 0.01


def test_exp_avg_sq_decays_only_with_the_flag():
    n, steps = 4096, 2000
    out = {}
    for sr in (False, True):
        p = torch.zeros(n, dtype=torch.bfloat16)
        g, m = torch.zeros_like(p), torch.zeros_like(p)
        v = torch.ones_like(p)
        for step in range(1, steps + 1):
            _adamw_reference(p, g, m, v, OK_STATS, STAG_LR, 0.9, 0.999, 1e-8, 0.0, step,
                             sr=(KEY, 0) if sr else None)
        out[sr] = v.float()
    assert (out[False] == 1.0).all()  # bf16(0.999 * 1.0) == 1.0, for ever
    want = 0.999 ** steps  # 0.135
    assert abs(out[True].double().mean().item() - want) <= 0.05 * want


# ------------------------------------------------------------------ arguments
def test_flag_parses_and_refuses_other_dtypes(capsys):
    from fault_tolerant_llm_training_amd.utils.config import get_args

    assert get_args([]).stochastic_rounding is False
    assert get_args(["--stochastic-rounding"]).stochastic_rounding is True
    for dt in ("fp32", "fp16", "fp64"):
        with pytest.raises(SystemExit) as e:
            get_args(["--stochastic-rounding", "--model-dtype", dt])
        assert e.value.code != 0
        assert "--stochastic-rounding supports bf16 parameters only" in capsys.readouterr().err
    for graph in ("--hip-graph", "--compile"):
        with pytest.raises(SystemExit):
            get_args(["--stochastic-rounding", graph])
        assert "not supported under whole-step graph replay" in capsys.readouterr().err


def test_graphed_step_refuses_an_optimizer_with_the_flag():
    from types import SimpleNamespace

    from fault_tolerant_llm_training_amd.graphs import GraphedStep

    with pytest.raises(ValueError, match="not supported under whole-step graph replay"):
        GraphedStep(None, SimpleNamespace(comm=False), SimpleNamespace(stochastic_rounding=True), None, None)


def test_optimizer_refuses_other_dtypes_and_derives_the_key_from_the_seed():
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for
    from fault_tolerant_llm_training_amd.optim.adamw import FlatAdamW

    a = model_args_for("tiny", vocab_size=64, seq_len=16)
    m = build_model(a, "cpu", torch.float32, seed=0)
    with pytest.raises(ValueError, match="bf16 parameters only"):
        FlatAdamW(m.parameters(), m.flat, stochastic_rounding=True)
    m = build_model(a, "cpu", torch.bfloat16, seed=0)
    o1 = FlatAdamW(m.parameters(), m.flat, stochastic_rounding=True, sr_seed=1)
    o2 = FlatAdamW(m.parameters(), m.flat, stochastic_rounding=True, sr_seed=2)
    assert o1.sr_key == key_from_seed(1) != o2.sr_key and 0 <= o1.sr_key < 1 << 63


# ------------------------------------------------------------------ train.py end to end (CPU)
SYN = TINY + ["--synthetic-data", "--vocab-size", "256"]


def _digests(out, tag=""):
    m = re.search(r"State digest at step (\d+)" + re.escape(tag) + r": (.*)", out)
    assert m, out[-3000:]
    return int(m.group(1)), m.group(2).strip()


@pytest.mark.slow
def test_train_py_resume_is_bit_exact_and_meta_carries_the_key(tmp_path):
    d = str(tmp_path)
    write_fake_sbatch(d)
    ck = os.path.join(d, "ck")
    base = SYN + ["--checkpoint-path", ck, "--training-steps", "9", "--lr-warmup-steps", "3", "--state-digest"]
    sr = ["--stochastic-rounding"]
    rc, out = run_train(d, "10", base + sr)
    assert rc == 0 and "Training completed" in out, out[-3000:]
    assert "Stochastic rounding: on -- " in out and f"key {key_from_seed(1234):#018x}" in out
    ref = _digests(out)
    # error-step save, then a resume: same bits as the uninterrupted run
    rc, out = run_train(d, "20", base + sr + ["--raise-error", "--error-step", "4"])
    assert rc == 0 and "Checkpoint saved at step 4" in out, out[-3000:]
    meta = torch.load(os.path.join(ck, "checkpoint_20.ckpt"), map_location="cpu", weights_only=True)["meta"]
    assert meta["stochastic_rounding"] is True and meta["sr_key"] == key_from_seed(1234)
    rc, out = run_train(d, "30", base + sr + ["--checkpoint-id", "20"])
    assert rc == 0 and "Resuming training from training_step 4" in out, out[-3000:]
    assert _digests(out) == ref and ref[0] == 9
    assert "continuing with the recorded key" not in out  # --seed agrees with the file
    # a second uninterrupted run under another --seed (another key): a different run
    rc, out = run_train(d, "40", base + sr + ["--seed", "77"])
    assert rc == 0 and _digests(out)[1] != ref[1]
    # without the flag: no start-up line, no key in the file, and other digests than with it
    rc, out = run_train(d, "50", base + ["--raise-error", "--error-step", "4"])
    assert rc == 0 and "Stochastic rounding" not in out
    meta = torch.load(os.path.join(ck, "checkpoint_50.ckpt"), map_location="cpu", weights_only=True)["meta"]
    assert "sr_key" not in meta and "stochastic_rounding" not in meta
    # resuming that file with the flag derives the key from --seed
    rc, out = run_train(d, "60", base + sr + ["--checkpoint-id", "50"])
    assert rc == 0 and "the checkpoint records no key" in out and "Training completed" in out, out[-3000:]
    assert _digests(out)[1] != ref[1]


@pytest.mark.slow
def test_train_py_resume_logs_a_seed_that_disagrees_with_the_recorded_key(tmp_path):
    d = str(tmp_path)
    write_fake_sbatch(d)
    base = SYN + ["--checkpoint-path", os.path.join(d, "ck"), "--training-steps", "4", "--stochastic-rounding"]
    rc, out = run_train(d, "1", base + ["--raise-error", "--error-step", "2"])
    assert rc == 0 and "Checkpoint saved at step 2" in out, out[-3000:]
    rc, out = run_train(d, "2", base + ["--checkpoint-id", "1", "--seed", "5"])
    assert rc == 0 and "continuing with the recorded key" in out, out[-3000:]
    assert f"key {key_from_seed(1234):#018x}" in out  # the start-up line shows the key in use


def test_train_py_refuses_the_flag_with_fp32(tmp_path):
    rc, out = run_train(str(tmp_path), "1", SYN + ["--stochastic-rounding", "--model-dtype", "fp32",
                                                   "--training-steps", "1"])
    assert rc != 0 and "--stochastic-rounding supports bf16 parameters only" in out


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.slow
def test_data_parallel_modes_round_alike(tmp_path):
    """ZeRO-1 (each rank updates its shard of every bucket) and all-reduce (every rank updates whole
    buckets) draw the same bits for the same flat element: bitwise-equal parameters after 3 steps.
    --grad-max-norm 0: the clip coefficient is exactly 1 in both modes."""
    d = str(tmp_path)
    write_fake_sbatch(d)
    digests = {}
    for mode in ("zero1", "allreduce"):
        args = SYN + ["--checkpoint-path", os.path.join(d, "ck_" + mode), "--training-steps", "3", "--state-digest",
                      "--stochastic-rounding", "--grad-max-norm", "0", "--dp-mode", mode, "--dp-bucket-mb", "0.1",
                      "--save-every", "0"]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "train.py")] + args
        r = subprocess.run(cmd, cwd=d, env=env_for(d, mode, {"OMP_NUM_THREADS": "1"}), capture_output=True,
                           text=True, timeout=600)
        out = r.stdout + r.stderr
        assert r.returncode == 0 and "Training completed" in out, out[-3000:]
        # (rank 0 logs; the parameter buffer is whole on every rank in both modes)
        m = re.search(r"\[rank 0\] State digest at step 3: params=(\S+)", out)
        assert m, out[-3000:]
        digests[mode] = m.group(1)
    assert digests["zero1"] == digests["allreduce"]
