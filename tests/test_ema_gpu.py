"""Parameter EMA (--ema-decay) on the MI355X: the ``ema_update_`` kernel against the definition
(utils/ema.py), its skip flag and launch partitioning, the pipelined optimizer and the whole-step
HIP graph against the CPU-oracle recurrence, and train.py (read-only to training, resume, digest,
--hip-graph, --eval-ema / --sample-ema). Every comparison is bit for bit.
"""
import contextlib
import io
import json
import os
import re

import numpy as np
import pytest
import torch

from helpers import run_train, write_fake_sbatch

from fault_tolerant_llm_training_amd.utils import ema as E

pytestmark = pytest.mark.gpu

DECAY = 0.999
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


@pytest.fixture(scope="module")
def K():
    from fault_tolerant_llm_training_amd._native import kernels

    return kernels()


def _stats(nonfinite=0.0):
    return torch.tensor([0.0, 1.0, nonfinite], device="cuda")


def _oracle(e, p, omd):
    return torch.from_numpy(E.ema_update_numpy(e.cpu().numpy().copy(), p.cpu().float().numpy(), omd))


def _case(n, dtype, seed):
    """Weights ~N(0, 0.02) in ``dtype``; averages at distance 0, 1 ulp (fp32) and 1e-3 from them, interleaved."""
    g = torch.Generator().manual_seed(seed)
    p = (0.02 * torch.randn(n, generator=g)).to(dtype)
    pf = p.float()
    e = pf.clone()
    e[1::3] = torch.nextafter(pf[1::3], torch.full_like(pf[1::3], 1.0))
    e[2::3] = pf[2::3] + 1e-3
    return p, e


# ------------------------------------------------------------------------------- 1. kernel == definition
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,max_blocks", [(8, 0), (8 * 255, 0), (8 * 257, 0), (8 * 1000, 2)])
def test_kernel_equals_the_definition(K, dtype, n, max_blocks):
    p, e = _case(n, dtype, seed=n)
    omd = E.one_minus_decay(DECAY)
    want = _oracle(e, p, omd)
    pd, ed = p.cuda(), e.cuda()
    K.ema_update_(ed, pd, _stats(), omd, max_blocks)
    assert torch.equal(ed.cpu(), want)
    assert torch.equal(pd.cpu(), p)
    if n >= 8 * 255:  # elements moved, and a fused multiply-add would have shown
        assert not torch.equal(want, e)
        fused = (e.double() + (p.float() - e).double() * float(np.float32(omd))).float()
        print(f"elements where an fma rounds differently: {int((fused != want).sum())} of {n}")
    # a second update from the kernel's own output
    K.ema_update_(ed, pd, _stats(), omd, max_blocks)
    assert torch.equal(ed.cpu(), _oracle(want, p, omd))


def test_kernel_preconditions(K):
    p, e = _case(64, torch.bfloat16, 1)
    pd, ed = p.cuda(), e.cuda()
    for bad in (lambda: K.ema_update_(ed[:56], pd, _stats(), 0.001, 0),          # sizes differ
                lambda: K.ema_update_(ed[:60], pd[:60], _stats(), 0.001, 0),     # not a multiple of 8
                lambda: K.ema_update_(ed.half(), pd, _stats(), 0.001, 0),        # average not fp32
                lambda: K.ema_update_(ed, pd, torch.zeros(2, device="cuda"), 0.001, 0),
                lambda: K.ema_update_(ed[::2], pd[:32], _stats(), 0.001, 0)):    # not contiguous
        with pytest.raises(RuntimeError):
            bad()
    torch.cuda.synchronize()
    assert torch.equal(ed.cpu(), e)


# ------------------------------------------------------------------------------- 2. skip flag
@pytest.mark.parametrize("dtype", DTYPES)
def test_nonfinite_flag_leaves_the_average_untouched(K, dtype):
    p, e = _case(8 * 257, dtype, seed=5)
    ed = e.cuda()
    K.ema_update_(ed, p.cuda(), _stats(nonfinite=1.0), E.one_minus_decay(DECAY), 0)
    assert torch.equal(ed.cpu(), e)


# ------------------------------------------------------------------------------- harness: tiny model
def _setup(dtype=torch.bfloat16, **kw):
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for
    from fault_tolerant_llm_training_amd.optim.adamw import FlatAdamW
    from fault_tolerant_llm_training_amd.parallel.ddp import GradReducer
    from fault_tolerant_llm_training_amd.utils.lr import build_lr_scheduler

    m = build_model(model_args_for("tiny", vocab_size=1024, seq_len=128), "cuda", dtype, seed=3)
    red = GradReducer(m.flat, m.sinks_in_backward_order(), bucket_mb=1.0)
    opt = FlatAdamW(m.parameters(), m.flat, lr=3e-3, max_grad_norm=1.0, reducer=red, **kw)
    m.gate = opt.gate
    return m, red, opt, build_lr_scheduler(opt, 4)


def _batches(n):
    from fault_tolerant_llm_training_amd.data.synthetic import SyntheticTokens

    data = SyntheticTokens(1024, 128, seed=11)
    return [tuple(t.cuda() for t in data.batch(i, 2)) for i in range(n)]


# ------------------------------------------------------------------------------- 3. pieces == whole
def test_launches_over_the_bucket_pieces_equal_one_launch(K):
    m, red, _opt, _ = _setup()
    assert len(red.buckets) > 1
    p = m.flat.params
    e0 = p.float() + 1e-3
    omd = E.one_minus_decay(DECAY)
    whole, pieces = e0.clone(), e0.clone()
    K.ema_update_(whole, p, _stats(), omd, 0)
    for b in red.buckets:
        K.ema_update_(pieces[b.lo : b.hi], p[b.lo : b.hi], _stats(), omd, 3)
    assert torch.equal(whole, pieces)
    assert torch.equal(whole.cpu(), _oracle(e0, p, omd))


# ------------------------------------------------------------------------------- 4. pipelined optimizer
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_optimizer_read_only_and_recurrence_on_the_gpus_parameters(dtype):
    inv = torch.full((1,), 1.0 / (2 * 128), device="cuda")
    batches = _batches(5)
    (m0, r0, o0, s0), (m1, r1, o1, s1) = _setup(dtype), _setup(dtype, ema_decay=DECAY)
    omd = E.one_minus_decay(DECAY)
    e = m1.flat.params.float().cpu()
    assert torch.equal(o1.ema.cpu(), e)
    for i, (tok, lab) in enumerate(batches):
        for m, r, o, s in ((m0, r0, o0, s0), (m1, r1, o1, s1)):
            m(tok, lab, inv).backward()
            r.finish()
            o.step()
            s.step()
        torch.cuda.synchronize()
        assert torch.equal(m0.flat.params, m1.flat.params), i
        assert torch.equal(o0.exp_avg, o1.exp_avg) and torch.equal(o0.exp_avg_sq, o1.exp_avg_sq), i
        e = _oracle(e, m1.flat.params, omd)
        assert torch.equal(o1.ema.cpu(), e), i
    assert o1.ema_updates == 5 and o1.check_finite(block=True) is not None
    # the swap: the cast average inside, the old bits after
    old = m1.flat.params.clone()
    with o1.ema_weights():
        assert torch.equal(m1.flat.params.cpu(), e.to(dtype))
    torch.cuda.synchronize()
    assert torch.equal(m1.flat.params, old) and torch.equal(o1.ema.cpu(), e)


# ------------------------------------------------------------------------------- 5. whole-step graph
def test_graphed_steps_keep_the_eager_average():
    from fault_tolerant_llm_training_amd.graphs import GraphedStep

    inv = torch.full((1,), 1.0 / (2 * 128), device="cuda")
    batches = _batches(7)
    m, red, opt, sched = _setup(ema_decay=DECAY)
    for tok, lab in batches:
        m(tok, lab, inv).backward()
        red.finish()
        opt.step()
        sched.step()
    torch.cuda.synchronize()
    pe, ee = m.flat.params.clone(), opt.ema.clone()

    m2, red2, opt2, sched2 = _setup(ema_decay=DECAY)

    def fwd_bwd(tok, lab):
        loss = m2(tok, lab, inv)
        loss.backward()
        red2.finish()
        return loss

    gs = GraphedStep(m2, red2, opt2, sched2, fwd_bwd)
    for tok, lab in batches[:2]:
        fwd_bwd(tok, lab)
        opt2.step()
        sched2.step()
    gs.prime(*batches[2])
    for tok, lab in batches[3:]:
        gs.step(tok, lab)
    gs.finish()
    torch.cuda.synchronize()
    assert opt2.step_count == 7 and opt2.ema_updates == 7
    assert torch.equal(m2.flat.params, pe) and torch.equal(opt2.ema, ee)
    assert not torch.equal(ee, pe.float())
    with pytest.raises(ValueError, match="ema-every"):
        m3, red3, opt3, sched3 = _setup(ema_decay=DECAY, ema_every=2)
        GraphedStep(m3, red3, opt3, sched3, fwd_bwd)


# ------------------------------------------------------------------------------- train.py
GPU = ["--device", "cuda", "--model", "tiny", "--synthetic-data", "--vocab-size", "1024", "--sequence-length", "128",
       "--batch-size", "2", "--learning-rate", "1e-3", "--lr-warmup-steps", "3", "--logging-frequency", "5",
       "--prefetch", "1", "--training-steps", "20", "--raise-error"]
EMA = ["--ema-decay", str(DECAY)]


def _load(d, job):
    return torch.load(os.path.join(d, "ck", f"checkpoint_{job}.ckpt"), map_location="cpu", weights_only=True)


def _flat(sd):
    return torch.cat([t.reshape(-1) for t in sd.values()])


def _same_training_state(a, b):
    assert a["training_step"] == b["training_step"]
    assert torch.equal(_flat(a["model"]), _flat(b["model"]))
    for i in a["optimizer"]["state"]:
        for key in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(a["optimizer"]["state"][i][key], b["optimizer"]["state"][i][key]), (i, key)
    assert a["lr_scheduler"] == b["lr_scheduler"] and a["data_loader"] == b["data_loader"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """One directory; run(job, extra) trains once per job id and returns (checkpoint, log)."""
    d = str(tmp_path_factory.mktemp("ema_gpu"))
    write_fake_sbatch(d)
    done = {}

    def run(job, extra):
        if job not in done:
            rc, out = run_train(d, job, GPU + ["--checkpoint-path", os.path.join(d, "ck")] + extra, timeout=240)
            assert rc == 0 and "Checkpoint saved at step" in out, out[-3000:]
            done[job] = (_load(d, job), out)
        return done[job]

    run.dir = d
    return run


def test_train_py_flag_leaves_training_identical_and_resumes_bit_exact(runs):
    off, _ = runs("900", ["--error-step", "12"])
    on, out = runs("901", EMA + ["--error-step", "12"])
    assert "Parameter EMA: on -- decay 0.999" in out
    assert "ema" not in off and "ema" not in off["meta"]
    _same_training_state(on, off)
    assert on["meta"]["ema"] == {"decay": DECAY, "every": 1, "updates": 12}
    assert list(on["ema"]) == list(on["model"]) and all(t.dtype == torch.float32 for t in on["ema"].values())
    assert not torch.equal(_flat(on["ema"]), _flat(on["model"]).float())
    _part, _ = runs("902", EMA + ["--error-step", "5"])
    res, out = runs("903", EMA + ["--error-step", "12", "--checkpoint-id", "902"])
    assert "Resuming training from training_step 5" in out and "Parameter EMA loaded from checkpoint (5 updates)" in out
    dg = next(ln for ln in out.splitlines() if "Checkpoint digest verified:" in ln)
    assert re.search(r" ema=[0-9a-f]{16}", dg), dg
    _same_training_state(res, on)
    assert torch.equal(_flat(res["ema"]), _flat(on["ema"])) and res["meta"]["ema"] == on["meta"]["ema"]


def test_train_py_hip_graph_ends_with_the_eager_average(runs):
    eager, _ = runs("901", EMA + ["--error-step", "12"])
    graph, out = runs("904", EMA + ["--error-step", "12", "--hip-graph"])
    assert "HIP graph" in out
    _same_training_state(graph, eager)
    assert torch.equal(_flat(graph["ema"]), _flat(eager["ema"])) and graph["meta"]["ema"] == eager["meta"]["ema"]


def _generate(argv):
    from fault_tolerant_llm_training_amd import generate

    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        rc = generate.main(argv)
    return rc, out.getvalue(), err.getvalue()


def test_train_py_sample_ema_and_eval_ema_are_read_only_and_match_generate_use_ema(runs):
    """A periodic save at step 6 (blocking), then the boundary's evaluation and sample on the average;
    the run stops at step 7 with the file of a run without the two flags."""
    plain, _ = runs("905", EMA + ["--error-step", "7"])
    extra = ["--eval-every", "6", "--eval-sequences", "4", "--eval-ema", "--sample-every", "6", "--sample-ema",
             "--sample-tokens", "12", "--sample-temperature", "0.8", "--sample-top-k", "40", "--metrics-file",
             "m906.jsonl", "--save-every", "6", "--no-async-checkpoint"]
    d = runs.dir
    both, out = runs("906", EMA + ["--error-step", "7"] + extra)
    _same_training_state(both, plain)
    assert torch.equal(_flat(both["ema"]), _flat(plain["ema"]))
    recs = [json.loads(ln) for ln in open(os.path.join(d, "m906.jsonl")).read().splitlines() if ln.strip()]
    ev = next(r for r in recs if r.get("eval_step") == 6)
    assert "ema_loss_fx" in ev and ev["ema_loss_fx"] != ev["eval_loss_fx"]
    sample = next(r for r in recs if r.get("sample_step") == 6)
    line = next(ln for ln in out.splitlines() if "Sample at step 6 |" in ln)
    assert line.endswith("| from the parameter EMA"), line
    # the exit save at step 7 replaced the periodic file of step 6: a job stopped at step 6 wrote the same state
    runs("907", EMA + ["--error-step", "6"])
    argv = ["--checkpoint", os.path.join(d, "ck", "checkpoint_907.ckpt"), "--model", "tiny", "--vocab-size", "1024",
            "--device", "cuda", "--prompt-ids", "1", "--max-new-tokens", "12", "--temperature", "0.8", "--top-k", "40",
            "--seed", "1234", "--sampler-step", "6", "--json"]
    rc, js, err = _generate(argv + ["--use-ema"])
    assert rc == 0, err
    assert json.loads(js)["ids"] == sample["sample_ids"]
