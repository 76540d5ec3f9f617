"""Per-parameter tensor statistics (--tensor-stats-every) on the CPU path: the definition against
hand-computed values, argument checking, training left untouched, and ZeRO-1 against the
replicated all-reduce mode over two gloo ranks.
"""
import json
import os
import re
import socket
import subprocess
import sys

import pytest
import torch

from helpers import ROOT, TINY, env_for, run_train

SYN = TINY + ["--synthetic-data", "--vocab-size", "256"]
BUFFERS = ("params", "grads", "exp_avg", "exp_avg_sq")


def _records(path):
    return [r for r in (json.loads(ln) for ln in open(path).read().splitlines() if ln.strip())
            if "tensor_stats_step" in r]


def test_reference_against_hand_computed_values():
    from fault_tolerant_llm_training_amd.utils.tensor_stats import FIELDS, segment_stats_reference

    assert FIELDS == ("sumsq", "absmax", "nonfinite", "zeros")
    sub = 2.0 ** -133  # the smallest bf16 subnormal: its square, 2^-266, underflows fp32
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([1.0, -2.0, nan, 0.0,      # 0..3   segment 0
                      9.0,                      # 4      a gap element
                      inf, -inf, -0.0, 0.5,     # 5..8   segment 1
                      sub, -3.0, 0.0, nan,      # 9..12  segment 3 (segment 2 is empty, at 9)
                      7.0, 7.0, 7.0,            # 13..15 gap
                      nan, inf,                 # 16, 17 segment 4: nothing finite
                      -4.0, 0.25],              # 18, 19 segment 5 up to the end of the buffer
                     dtype=torch.float64).bfloat16()
    assert x.numel() == 20 and x[9].item() == sub and x[9].item() != 0.0
    got = segment_stats_reference(x, [0, 5, 9, 9, 16, 18], [4, 4, 0, 4, 2, 2])
    want = torch.tensor([[5.0, 2.0, 1, 1],
                         [0.25, 0.5, 2, 1],
                         [0.0, 0.0, 0, 0],
                         [9.0 + 2.0 ** -266, 3.0, 1, 1],
                         [0.0, 0.0, 2, 0],
                         [16.0625, 4.0, 0, 0]], dtype=torch.float64)
    assert got.dtype == torch.float64 and torch.equal(got, want)
    # the subnormal alone: counted in sumsq and absmax, not a zero
    one = segment_stats_reference(x, [9], [1])
    assert one.tolist() == [[2.0 ** -266, sub, 0.0, 0.0]]
    for dtype in (torch.float16, torch.float32, torch.float64):
        y = torch.tensor([3.0, -0.0, inf, 2.0 ** -24], dtype=dtype)  # 2^-24: an fp16 subnormal
        assert segment_stats_reference(y, [0], [4]).tolist() == [[9.0 + 2.0 ** -48, 3.0, 1.0, 1.0]]
    with pytest.raises(ValueError):
        segment_stats_reference(x, [0, 3], [4, 4])       # overlapping
    with pytest.raises(ValueError):
        segment_stats_reference(x, [5, 0], [4, 4])       # unsorted
    with pytest.raises(ValueError):
        segment_stats_reference(x, [0, 18], [4, 3])      # past the end
    with pytest.raises(ValueError):
        segment_stats_reference(x.view(4, 5).t(), [0], [4])


def test_plan_on_cpu_runs_the_reference():
    from fault_tolerant_llm_training_amd.utils.tensor_stats import SegmentStatsPlan, segment_stats_reference

    g = torch.Generator().manual_seed(3)
    x = torch.randint(-32768, 32768, (5000,), generator=g, dtype=torch.int16).view(torch.bfloat16)
    off, num = [3, 100, 100, 4097], [64, 0, 2500, 903]
    plan = SegmentStatsPlan(off, num)
    assert torch.equal(plan.run(x), segment_stats_reference(x, off, num))
    assert plan.run(x)[:, 2].sum() > 0  # random bits: NaN / Inf occur
    with pytest.raises(ValueError):
        SegmentStatsPlan([0, 3], [4, 4])


def test_argument_parsing(capsys):
    from fault_tolerant_llm_training_amd.utils.config import get_args

    assert get_args([]).tensor_stats_every == 0
    assert get_args(["--tensor-stats-every", "25"]).tensor_stats_every == 25
    with pytest.raises(SystemExit):
        get_args(["--tensor-stats-every", "-1"])
    assert "--tensor-stats-every" in capsys.readouterr().err


def _losses(out):
    return re.findall(r"Training step: (\d+) \| Loss: ([-\d.naninf]+) .*?grad_norm: ([-\d.naninf]+)", out)


def _digest(out, step=6):
    m = re.search(rf"State digest at step {step}: (params=\w+ exp_avg=\w+ exp_avg_sq=\w+ optimizer_step=\d+)", out)
    assert m, out
    return m.group(1)


def test_training_is_unchanged_and_records_describe_the_model(tmp_path):
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    outs = {}
    for every in (0, 2):
        d = str(tmp_path / f"s{every}")
        os.makedirs(d)
        rc, out = run_train(d, "1", SYN + ["--training-steps", "6", "--logging-frequency", "1", "--state-digest",
                                           "--checkpoint-path", os.path.join(d, "ck"), "--metrics-file", "m.jsonl",
                                           "--tensor-stats-every", str(every)])
        assert rc == 0, out
        outs[every] = (out, _records(os.path.join(d, "m.jsonl")))
    (off, none), (on, recs) = outs[0], outs[2]
    assert none == [] and "Tensor stats" not in off
    assert len(_losses(off)) == 6 and _losses(off) == _losses(on)
    assert _digest(off) == _digest(on)
    assert [r["tensor_stats_step"] for r in recs] == [2, 4, 6]
    model = build_model(model_args_for("tiny", vocab_size=256, seq_len=32), "cpu", torch.bfloat16, seed=0)
    keys = set(model.state_dict().keys())
    assert keys == set(model.flat.slots)
    n_params = sum(p.numel() for p in model.parameters())
    for r in recs:
        assert r["fields"] == ["sumsq", "absmax", "nonfinite", "zeros"]
        assert set(r["numel"]) == keys and sum(r["numel"].values()) == n_params
        for b in BUFFERS:
            assert set(r[b]) == keys
            assert all(len(v) == 4 and v[2] == 0 and 0 <= v[3] <= r["numel"][n] for n, v in r[b].items())
        assert all(v[0] > 0 and v[1] > 0 for v in r["params"].values())
        assert any(v[0] > 0 for v in r["grads"].values())
        assert f"Tensor stats at step {r['tensor_stats_step']}: {len(keys)} parameters" in on


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.slow
def test_zero1_records_equal_the_replicated_ones(tmp_path):
    """Two gloo ranks, fp32. At W = 2 a two-term sum is commutative, so both modes hold bit-equal
    gradients and states; only the fold order of sumsq differs (ZeRO-1 adds two ranks' partial sums):
    each side errs by at most (n-1) 2^-53 relative, hence 2 n 2^-53 between them. (The clipping
    threshold is out of reach: the two modes sum the gradient norm in different orders, and a clip
    coefficient that differs in its last bit would make the states differ too.)"""
    recs = {}
    for mode in ("allreduce", "zero1"):
        d = str(tmp_path / mode)
        os.makedirs(d)
        args = SYN + ["--training-steps", "4", "--model-dtype", "fp32", "--dp-mode", mode, "--dp-bucket-mb", "0.1",
                      "--grad-max-norm", "1e9", "--tensor-stats-every", "2", "--metrics-file", "m.jsonl",
                      "--checkpoint-path", os.path.join(d, "ck")]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
               "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "train.py")] + args
        r = subprocess.run(cmd, cwd=d, env=env_for(d, "1", {"OMP_NUM_THREADS": "1"}), capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"Data parallel over 2 ranks: {mode}" in r.stdout + r.stderr
        recs[mode] = _records(os.path.join(d, "m.jsonl"))
    a, z = recs["allreduce"], recs["zero1"]
    assert [r["tensor_stats_step"] for r in a] == [2, 4] == [r["tensor_stats_step"] for r in z]
    for ra, rz in zip(a, z):
        assert ra["numel"] == rz["numel"]
        for b in BUFFERS:
            assert list(ra[b]) == list(rz[b])
            for name, va in ra[b].items():
                vz, n = rz[b][name], ra["numel"][name]
                assert va[1:] == vz[1:], (b, name, va, vz)
                print(f"{b} {name}: sumsq {va[0]!r} / {vz[0]!r}")
                assert abs(va[0] - vz[0]) <= 2 * n * 2.0 ** -53 * va[0], (b, name, va, vz)
        assert any(v[0] > 0 for v in rz["grads"].values()) and any(v[0] > 0 for v in rz["exp_avg_sq"].values())
