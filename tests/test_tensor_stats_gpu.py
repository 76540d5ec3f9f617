"""Per-parameter tensor statistics on the GPU: the segmented kernel (csrc/kernels/tensor_stats.hip)
against its float64 definition (utils/tensor_stats.py), 64-bit indexing, what the op refuses, the
model-level collection, and --tensor-stats-every runs of train.py against runs without it.

sumsq tolerance: squares are exact in float64 for bf16 / fp16 / fp32, and a float64 sum of n
non-negative terms errs by at most (n-1) 2^-53 relative in any order; the kernel and the oracle
each err by that much, so they agree to 2 (n-1) 2^-53 relative. The other three columns are exact.
"""
import json
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -53
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
BUFFERS = ("params", "grads", "exp_avg", "exp_avg_sq")


@pytest.fixture(scope="module")
def TS():
    from fault_tolerant_llm_training_amd.utils import tensor_stats

    return tensor_stats


def _raw(seed, n, dtype):
    """n elements with uniformly random raw bits (NaNs, infinities, subnormals), on the CPU."""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32:
        return torch.randint(-2**31, 2**31, (n,), generator=g, dtype=torch.int32).view(dtype)
    return torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int16).view(dtype)


def _agree(got, want, numels, what):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == torch.float64
    assert torch.equal(got[:, 1:], want[:, 1:]), (what, got[:, 1:], want[:, 1:])
    for s, n in enumerate(numels):
        g, w = got[s, 0].item(), want[s, 0].item()
        assert abs(g - w) <= 2 * max(0, n - 1) * U * w, (what, s, n, g, w)


def _layout(lengths, gaps):
    off, pos = [], 0
    for i, n in enumerate(lengths):
        off.append(pos)
        pos += n + gaps[i % len(gaps)]
    return off, pos


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_matches_the_definition(TS, dtype):
    C = TS.chunk()
    lengths = [0, 1, 7, 8, 9, 255, 256 * 8 + 3, C - 1, C, C + 1, 3 * C + 17]
    off, end = _layout(lengths, [0, 1, 3, 64])
    total = end + 70  # the last gap, and some more after it
    inside = torch.zeros(total, dtype=torch.bool)
    for o, n in zip(off, lengths):
        inside[o : o + n] = True
    assert int(inside.sum()) == sum(lengths)
    for start in (0, 1, 3):  # 1 and 3: the view is not 16-byte aligned
        host = _raw(31 + start, total + 3, dtype)
        view = host[start : start + total]
        view[~inside] = float("nan")  # one stray read changes a count
        for i, (o, n) in enumerate(zip(off, lengths)):
            if n >= 7:  # random 32-bit patterns hold no zero: one +-0 in the middle of every segment
                view[o + n // 2] = 0.0 if i % 2 else -0.0
        host[:start] = float("nan")
        host[start + total :] = float("nan")
        dev = host.to(DEV)
        assert dev.data_ptr() % 16 == 0
        plan = TS.SegmentStatsPlan(off, lengths, DEV)
        got = plan.run(dev[start : start + total])
        want = TS.segment_stats_reference(view, off, lengths)
        assert want[:, 2].sum() > 0 and want[:, 3].sum() > 0  # NaN / Inf and zeros occur naturally
        _agree(got, want, lengths, (dtype, start))
        assert torch.equal(dev.cpu().view(torch.uint8), host.view(torch.uint8))  # read-only


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_segment_of_subnormals(TS, dtype):
    n, lead = 1000, 5
    g = torch.Generator().manual_seed(7)
    if dtype == torch.float32:
        bits = torch.randint(1, 1 << 23, (n,), generator=g, dtype=torch.int32)
        bits[::2] |= -2**31
    else:
        top = 1 << (7 if dtype == torch.bfloat16 else 10)
        bits = torch.randint(1, top, (n,), generator=g, dtype=torch.int32)
        bits[::2] += 32768
        bits = torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16)
    host = torch.full((n + 2 * lead,), float("nan"), dtype=dtype)
    host[lead : lead + n] = bits.view(dtype)
    want = TS.segment_stats_reference(host, [lead], [n])
    assert want[0, 0].item() > 0 and want[0, 1].item() > 0 and want[0, 2:].tolist() == [0, 0]
    got = TS.SegmentStatsPlan([lead], [n], DEV).run(host.to(DEV))
    assert got[0, 3].item() == 0 and got[0, 0].item() > 0
    _agree(got, want, [n], dtype)


def test_many_small_segments_an_empty_table_and_two_runs(TS):
    nseg = 1000
    host = _raw(41, 64 * nseg, torch.bfloat16)
    dev = host.to(DEV)
    off, num = [64 * i for i in range(nseg)], [64] * nseg
    plan = TS.SegmentStatsPlan(off, num, DEV)
    a = plan.run(dev).clone()
    b = plan.run(dev)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    _agree(a, TS.segment_stats_reference(host, off, num), num, "1000 x 64")
    C = TS.chunk()  # ... and of a table with multi-item segments
    big = _raw(42, 5 * C + 9, torch.float32).to(DEV)
    plan = TS.SegmentStatsPlan([1, 2 * C + 2], [2 * C + 1, 3 * C + 5], DEV)
    a = plan.run(big).clone()
    assert torch.equal(a.view(torch.int64), plan.run(big).view(torch.int64))
    empty = TS.SegmentStatsPlan([], [], DEV).run(dev)
    assert tuple(empty.shape) == (0, 4) and empty.dtype == torch.float64


def test_64_bit_indexing(TS):
    N = 2**32 + 2**16
    buf = torch.full((N,), 0.5, dtype=torch.bfloat16, device=DEV)  # 8.6 GB
    for b in (2**31, 2**32):
        buf[b - 3 : b + 3] = torch.tensor([float("inf"), 0.0, 3.0, 3.0, 0.0, float("inf")], dtype=torch.bfloat16, device=DEV)
    off = [2**31 - 1_000_003, 2**32 - 70_001]
    num = [2_000_007, 70_001 + 2**16 - 5]
    assert off[1] + num[1] <= N and off[0] + num[0] > 2**31 and off[0] + num[0] < off[1]
    got = TS.SegmentStatsPlan(off, num, DEV).run(buf).cpu()
    # closed form: 0.25 per plain element, two 3.0, two zeros, two infinities in each segment
    # (every partial sum is a multiple of 0.25 far below 2^53: the kernel's value is exact)
    want = [[0.25 * (n - 6) + 18.0, 3.0, 2.0, 2.0] for n in num]
    assert got.tolist() == want
    del buf


def test_op_refuses_what_it_does_not_cover(TS):
    from fault_tolerant_llm_training_amd._native import kernels

    K = kernels()
    buf = torch.ones(4096, dtype=torch.bfloat16, device=DEV)
    off, num = torch.tensor([0, 100]), torch.tensor([64, 3996])
    items, first, extent = K.segment_stats_plan(off, num, 0)
    assert extent == 4096 and first.tolist() == [0, 1, 2]
    items, first = items.to(DEV), first.to(DEV)
    partial = torch.full((items.shape[0], 4), -1.0, dtype=torch.float64, device=DEV)
    out = torch.full((2, 4), -1.0, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError):  # a dtype without a kernel
        K.segment_stats_(buf.double(), items, first, extent, partial, out)
    with pytest.raises(RuntimeError):  # non-contiguous
        K.segment_stats_(torch.ones(8192, dtype=torch.bfloat16, device=DEV)[::2], items, first, extent, partial, out)
    with pytest.raises(RuntimeError):  # the last segment ends past the end of the buffer
        K.segment_stats_(buf[:4095], items, first, extent, partial, out)
    with pytest.raises(RuntimeError):  # table tensors on another device
        K.segment_stats_(buf, items.cpu(), first, extent, partial, out)
    with pytest.raises(RuntimeError):  # overlapping
        K.segment_stats_plan(torch.tensor([0, 63]), torch.tensor([64, 10]), 0)
    with pytest.raises(RuntimeError):  # unsorted
        K.segment_stats_plan(torch.tensor([100, 0]), torch.tensor([10, 10]), 0)
    with pytest.raises(ValueError):    # the plan class refuses the same table before the op sees it
        TS.SegmentStatsPlan([0, 63], [64, 10], DEV)
    with pytest.raises(RuntimeError):  # past the end, through the plan class
        TS.SegmentStatsPlan([0, 100], [64, 3996], DEV).run(buf[:4095])
    torch.cuda.synchronize()
    assert bool((out == -1.0).all()) and bool((partial == -1.0).all())  # untouched
    K.segment_stats_(buf, items, first, extent, partial, out)  # and the accepted call works
    assert out.cpu().tolist() == [[64.0, 1.0, 0.0, 0.0], [3996.0, 1.0, 0.0, 0.0]]


# ------------------------------------------------------------------------------- model level
def test_collect_on_the_tiny_model(TS):
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for
    from fault_tolerant_llm_training_amd.optim.adamw import FlatAdamW
    from fault_tolerant_llm_training_amd.parallel.ddp import GradReducer
    from fault_tolerant_llm_training_amd.utils.digest import tensor_digest

    m = build_model(model_args_for("tiny", vocab_size=1024, seq_len=128), DEV, torch.bfloat16, seed=0)
    red = GradReducer(m.flat, m.sinks_in_backward_order(), bucket_mb=1.0)
    opt = FlatAdamW(m.parameters(), m.flat, lr=1e-3, max_grad_norm=1.0, reducer=red)
    m.gate = opt.gate
    tok = torch.randint(0, 1024, (2, 128), generator=torch.Generator().manual_seed(0)).to(DEV)
    m(tok, tok).backward()
    red.finish()
    opt.clip_grad_norm_(1.0)
    opt.step()
    bufs = {"params": m.flat.params, "grads": m.flat.grads, "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq}
    rec = TS.collect(m, opt)
    torch.cuda.synchronize()
    before = {k: tensor_digest(v) for k, v in bufs.items()}
    rec2 = TS.collect(m, opt)
    torch.cuda.synchronize()
    assert {k: tensor_digest(v) for k, v in bufs.items()} == before and rec2 == rec  # read-only, reproducible
    slots = sorted(m.flat.slots.values(), key=lambda s: s.offset)
    names = [s.name for s in slots]
    assert set(names) == set(m.state_dict().keys()) and list(rec["numel"]) == names
    assert rec["numel"] == {s.name: s.numel for s in slots}
    assert sum(rec["numel"].values()) == sum(p.numel() for p in m.parameters())
    for b in BUFFERS:
        want = TS.segment_stats_reference(bufs[b].cpu(), [s.offset for s in slots], [s.numel for s in slots])
        got = torch.tensor([rec[b][n] for n in names], dtype=torch.float64)
        _agree(got, want, [s.numel for s in slots], b)
    norm = opt.last_norm()
    mine = sum(v[0] for v in rec["grads"].values()) ** 0.5
    print(f"gradient norm: optimizer {norm!r}, sqrt(sum of sumsq) {mine!r}")
    assert norm > 0 and abs(mine - norm) <= 2.0 ** -8 * norm


# ------------------------------------------------------------------------------- train.py
GPU = ["--device", "cuda", "--model", "tiny", "--synthetic-data", "--vocab-size", "1024", "--sequence-length", "128",
       "--batch-size", "2", "--training-steps", "6", "--logging-frequency", "1", "--state-digest", "--prefetch", "1"]
MODES = {"eager": [], "graph": ["--hip-graph"]}


@pytest.fixture(scope="module")
def train_runs(tmp_path_factory):
    """(mode, every) -> (log, tensor-stats records) of one 6-step run; each run happens once."""
    from helpers import run_train

    cache = {}

    def get(mode, every):
        if (mode, every) not in cache:
            d = str(tmp_path_factory.mktemp(f"{mode}{every}"))
            rc, out = run_train(d, "1", GPU + MODES[mode] + ["--tensor-stats-every", str(every), "--metrics-file",
                                                             "m.jsonl", "--checkpoint-path", os.path.join(d, "ck")],
                                timeout=240)
            assert rc == 0, out
            recs = [json.loads(ln) for ln in open(os.path.join(d, "m.jsonl")).read().splitlines() if ln.strip()]
            cache[(mode, every)] = (out, [r for r in recs if "tensor_stats_step" in r])
        return cache[(mode, every)]

    return get


def _losses(out):
    return re.findall(r"Training step: (\d+) \| Loss: ([-\d.naninf]+) .*?grad_norm: ([-\d.naninf]+)", out)


def _digest(out):
    m = re.search(r"State digest at step 6: (params=\w+ exp_avg=\w+ exp_avg_sq=\w+ optimizer_step=\d+ data_loader=.*)",
                  out)
    assert m, out
    return m.group(1)


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_training_is_unchanged_by_the_statistics(train_runs, mode):
    off, none = train_runs(mode, 0)
    on, recs = train_runs(mode, 2)
    assert none == [] and "Tensor stats" not in off
    assert len(_losses(off)) == 6 and _losses(off) == _losses(on)
    assert _digest(off) == _digest(on)
    assert [r["tensor_stats_step"] for r in recs] == [2, 4, 6]
    for r in recs:
        assert r["fields"] == ["sumsq", "absmax", "nonfinite", "zeros"]
        assert all(set(r[b]) == set(r["numel"]) for b in BUFFERS)
        assert sum(v[2] for b in BUFFERS for v in r[b].values()) == 0
        assert all(v[0] > 0 for v in r["grads"].values())
        assert f"Tensor stats at step {r['tensor_stats_step']}: {len(r['numel'])} parameters" in on
    # the logged gradient norm of step n-1 is the norm of the buffer the record at boundary n describes
    norms = {int(s): float(g) for s, _, g in _losses(on)}
    for r in recs:
        mine = sum(v[0] for v in r["grads"].values()) ** 0.5
        want = norms[r["tensor_stats_step"] - 1]
        assert abs(mine - want) <= 2.0 ** -8 * want + 0.5e-3  # (+ the log line's three decimals)


def test_eager_and_graph_runs_write_equal_records(train_runs):
    _, eager = train_runs("eager", 2)
    _, graph = train_runs("graph", 2)
    assert len(eager) == 3 and eager == graph


def test_nonfinite_stop_names_the_parameters_and_saves_the_same_file(tmp_path):
    from helpers import run_train, write_fake_sbatch

    base = ["--device", "cuda", "--model", "tiny", "--synthetic-data", "--vocab-size", "1024", "--sequence-length",
            "256", "--batch-size", "2", "--learning-rate", "1e30", "--lr-warmup-steps", "3", "--logging-frequency",
            "1", "--training-steps", "30"]
    files = {}
    for flag in (0, 2):
        d = str(tmp_path / f"f{flag}")
        os.makedirs(d)
        write_fake_sbatch(d)
        rc, out = run_train(d, "730", base + ["--checkpoint-path", os.path.join(d, "ck"), "--tensor-stats-every",
                                              str(flag)], timeout=240)
        assert rc == 0 and "is non-finite at optimizer step" in out, out[-3000:]
        assert "Checkpoint saved at step" in out, out[-3000:]
        m = re.search(r"Non-finite gradients in (\d+) of (\d+) parameters \(gradient buffer of step (\d+).*?\): (.*)",
                      out)
        if flag:
            assert m, out[-3000:]
            print(m.group(0))
            k, total = int(m.group(1)), int(m.group(2))
            assert 1 <= k <= total
            first = re.match(r"([\w.]+) \((\d+)/(\d+)\)", m.group(4))
            assert first and 1 <= int(first.group(2)) <= int(first.group(3))
            saved = int(re.search(r"Checkpoint saved at step (\d+)", out).group(1))
            assert saved <= int(m.group(3)) <= saved + 2
        else:
            assert m is None and "Tensor stats" not in out
        files[flag] = torch.load(os.path.join(d, "ck", "checkpoint_730.ckpt"), map_location="cpu", weights_only=True)
    a, c = files[0], files[2]
    assert a["training_step"] == c["training_step"] > 0
    for k in a["model"]:
        assert torch.equal(a["model"][k], c["model"][k]), k
    for i in a["optimizer"]["state"]:
        for key in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(a["optimizer"]["state"][i][key], c["optimizer"]["state"][i][key]), (i, key)
