"""Parameter EMA (--ema-decay) on the CPU path: the definition, training left untouched, the
recurrence over a trainer run, --ema-every, the non-finite guard, checkpoint entry / digest /
resume, flag mismatches across a resume, data parallelism under gloo, the weight swap
(ema_weights, --eval-ema, generate --use-ema) and argument checking. Every comparison is
bit for bit.
"""
import contextlib
import io
import json
import os
import shutil
import socket
import struct
import subprocess
import sys
import zipfile

import numpy as np
import pytest
import torch

from helpers import ROOT, TINY, env_for, make_parquet, run_train

from fault_tolerant_llm_training_amd.ckpt.format import checkpoint_file
from fault_tolerant_llm_training_amd.utils import ema as E

DECAY = 0.99
SYN = TINY + ["--synthetic-data", "--vocab-size", "256", "--learning-rate", "1e-3", "--lr-warmup-steps", "2",
              "--training-steps", "10"]
EMA = ["--ema-decay", str(DECAY)]


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def _flat(sd):
    return torch.cat([t.reshape(-1) for t in sd.values()])


def _moments(ck):
    st = ck["optimizer"]["state"]
    return [torch.cat([st[i][f].reshape(-1) for i in sorted(st)]) for f in ("exp_avg", "exp_avg_sq", "step")]


def _oracle(e, p, omd):
    """One update by the numpy float32 definition."""
    return torch.from_numpy(E.ema_update_numpy(e.numpy().copy(), p.float().numpy(), omd))


def _stop_at(d, job, k, extra=(), base=SYN):
    """A trainer run that stops with the injected error at step ``k`` and saves there."""
    ck = os.path.join(d, "ck")
    rc, out = run_train(d, job, base + ["--checkpoint-path", ck, "--raise-error", "--error-step", str(k)] + list(extra))
    path = checkpoint_file(ck, job)
    assert rc == 0 and os.path.exists(path), out[-3000:]
    return path, out


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """Flag-on runs stopped at steps 0..3 (their files hold p_k and e_k) and a flag-off run stopped at 3."""
    d = str(tmp_path_factory.mktemp("ema_chain"))
    files = {k: _stop_at(d, f"10{k}", k, EMA)[0] for k in range(4)}
    files["off"] = _stop_at(d, "200", 3)[0]
    return d, files


# ------------------------------------------------------------------------------- 1. the definition
def test_definition_against_a_hand_written_float32_loop():
    rng = np.random.default_rng(0)
    n = 4096
    p = torch.from_numpy((0.02 * rng.standard_normal(n)).astype(np.float32)).bfloat16()
    e = torch.from_numpy((0.02 * rng.standard_normal(n)).astype(np.float32))
    omd = E.one_minus_decay(0.999)
    assert omd == float(np.float32(1.0 - 0.999)) and E.one_minus_decay(0.999, 3) == float(np.float32(1.0 - 0.999 ** 3))
    pf, ef = p.float().numpy(), e.numpy()
    want = np.empty(n, dtype=np.float32)
    fused = np.empty(n, dtype=np.float32)
    o32 = np.float32(omd)
    for i in range(n):
        diff = np.float32(pf[i] - ef[i])
        prod = np.float32(diff * o32)
        want[i] = np.float32(ef[i] + prod)
        # what a fused multiply-add gives: the exact product (48 bits, exact in double) added once
        fused[i] = np.float32(np.float64(diff) * np.float64(o32) + np.float64(ef[i]))
    assert (fused != want).any(), "the data holds no element where a fused multiply-add rounds differently"
    got = E.ema_update_(e.clone(), p, omd)
    assert torch.equal(got, torch.from_numpy(want))
    assert np.array_equal(E.ema_update_numpy(ef.copy(), pf, omd), want)
    # fp64 models: the same three operations in float64
    e64 = e.double()
    got64 = E.ema_update_(e64.clone(), p.double(), E.one_minus_decay(0.999, 1, torch.float64))
    assert got64.dtype == torch.float64 and torch.equal(got64, e64 + (p.double() - e64) * (1.0 - 0.999))


# ------------------------------------------------------------------------------- 2, 3. trainer runs
def test_training_state_is_unchanged_by_the_flag(chain):
    _, files = chain
    on, off = _load(files[3]), _load(files["off"])
    assert "ema" in on and "ema" not in off and "ema" not in off["meta"]
    assert torch.equal(_flat(on["model"]), _flat(off["model"]))
    for a, b in zip(_moments(on), _moments(off)):
        assert torch.equal(a, b)
    assert on["data_loader"] == off["data_loader"] and on["lr_scheduler"] == off["lr_scheduler"]


def test_average_follows_the_recurrence_over_the_runs_parameters(chain):
    _, files = chain
    cks = [_load(files[k]) for k in range(4)]
    omd = E.one_minus_decay(DECAY)
    e = _flat(cks[0]["model"]).float()  # e_0 = float32(p_0)
    assert torch.equal(_flat(cks[0]["ema"]), e) and cks[0]["meta"]["ema"] == {"decay": DECAY, "every": 1, "updates": 0}
    for k in range(1, 4):
        p = _flat(cks[k]["model"])
        assert p.dtype == torch.bfloat16 and not torch.equal(p, _flat(cks[k - 1]["model"]))
        e = _oracle(e, p, omd)
        assert torch.equal(_flat(cks[k]["ema"]), e), k
        assert cks[k]["meta"]["ema"]["updates"] == k


# ------------------------------------------------------------------------------- in-process harness
def _mini(dtype=torch.bfloat16, **kw):
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for
    from fault_tolerant_llm_training_amd.optim.adamw import FlatAdamW
    from fault_tolerant_llm_training_amd.parallel.ddp import GradReducer

    m = build_model(model_args_for("tiny", vocab_size=96, seq_len=16), "cpu", dtype, seed=3)
    red = GradReducer(m.flat, m.sinks_in_backward_order(), bucket_mb=0.05)
    opt = FlatAdamW(m.parameters(), m.flat, lr=1e-2, max_grad_norm=1.0, reducer=red, **kw)
    m.gate = opt.gate
    assert len(red.buckets) > 1
    return m, red, opt


def _step(m, red, opt, i, poison=False):
    tok = torch.randint(0, 96, (2, 16), generator=torch.Generator().manual_seed(100 + i))
    m(tok, tok).backward()
    if poison:
        m.flat.grads[5] = float("nan")
    red.finish()
    opt.step()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
def test_optimizer_level_read_only_and_recurrence(dtype):
    """fp32 / fp64 parameters have the average's own dtype: the update must not write through them."""
    (m0, r0, o0), (m1, r1, o1) = _mini(dtype), _mini(dtype, ema_decay=DECAY)
    assert o1.ema.dtype == (torch.float64 if dtype == torch.float64 else torch.float32)
    e = m1.flat.params.to(o1.ema.dtype).clone()
    omd = E.one_minus_decay(DECAY, 1, o1.ema.dtype)
    for i in (1, 2, 3):
        _step(m0, r0, o0, i)
        _step(m1, r1, o1, i)
        assert torch.equal(m0.flat.params, m1.flat.params), i
        assert all(torch.equal(a, b) for a, b in zip(o0.moments(), o1.moments())), i
        e = torch.from_numpy(E.ema_update_numpy(e.numpy().copy(), m1.flat.params.to(e.dtype).numpy(), omd))
        assert torch.equal(o1.ema, e), i
    assert not torch.equal(e, m1.flat.params.to(e.dtype))


# ------------------------------------------------------------------------------- 4. --ema-every
def test_ema_every_moves_the_average_at_every_third_step_with_d_cubed(tmp_path, chain):
    m, red, opt = _mini(ema_decay=DECAY, ema_every=3)
    omd = E.one_minus_decay(DECAY, 3)
    assert omd != E.one_minus_decay(DECAY)
    e = m.flat.params.float().clone()
    for i in range(1, 7):
        before = opt.ema.clone()
        _step(m, red, opt, i)
        if i % 3:
            assert torch.equal(opt.ema, before), i
        else:
            e = _oracle(e, m.flat.params, omd)
            assert torch.equal(opt.ema, e) and not torch.equal(e, before), i
        assert opt.ema_updates == i // 3
    # the trainer: stopped at step 3, one update with d**3 from p_0 on the parameters of step 3
    _, files = chain
    path, _out = _stop_at(str(tmp_path), "300", 3, EMA + ["--ema-every", "3"])
    ck, p0 = _load(path), _flat(_load(files[0])["model"]).float()
    assert ck["meta"]["ema"] == {"decay": DECAY, "every": 3, "updates": 1}
    assert torch.equal(_flat(ck["model"]), _flat(_load(files[3])["model"]))
    assert torch.equal(_flat(ck["ema"]), _oracle(p0, _flat(ck["model"]), omd))
    two, _out = _stop_at(str(tmp_path), "301", 2, EMA + ["--ema-every", "3"])
    assert torch.equal(_flat(_load(two)["ema"]), p0) and _load(two)["meta"]["ema"]["updates"] == 0


# ------------------------------------------------------------------------------- 5. non-finite guard
def test_nonfinite_step_leaves_the_average_of_the_step_before(tmp_path, chain):
    m, red, opt = _mini(ema_decay=DECAY)
    for i in (1, 2):
        _step(m, red, opt, i)
    e2, p2 = opt.ema.clone(), m.flat.params.clone()
    _step(m, red, opt, 3, poison=True)
    _step(m, red, opt, 4)  # the flag is sticky
    assert opt.first_nonfinite(block=True) == 3
    assert torch.equal(opt.ema, e2) and torch.equal(m.flat.params, p2)
    opt.rollback_steps(2)
    assert opt.step_count == 2 and opt.ema_updates == 2
    # the trainer with the existing injection: step 2 fails in its forward, completes poisoned, the
    # update is skipped and the run stops at step 2 -- with the file of a run stopped at step 2
    _, files = chain
    d = str(tmp_path)
    ckd = os.path.join(d, "ck")
    rc, out = run_train(d, "400", SYN + EMA + ["--checkpoint-path", ckd], extra_env={"FT_INJECT_FAULT": "0:2:forward"})
    assert rc == 0 and "Checkpoint saved at step 2" in out, out[-3000:]
    bad, good = _load(checkpoint_file(ckd, "400")), _load(files[2])
    assert torch.equal(_flat(bad["ema"]), _flat(good["ema"])) and torch.equal(_flat(bad["model"]), _flat(good["model"]))
    assert bad["meta"]["ema"] == good["meta"]["ema"]


# ------------------------------------------------------------------------------- 6. resume
@pytest.mark.parametrize("kind", ["map", "iterable"])
def test_resumed_chain_ends_with_the_average_of_an_uninterrupted_run(tmp_path, kind):
    d = str(tmp_path)
    pq = os.path.join(d, "train.parquet")
    make_parquet(pq, n_docs=200, seed=1)
    base = TINY + ["--dataset", pq, "--tokenizer-name-or-path", "byte", "--learning-rate", "1e-3",
                   "--lr-warmup-steps", "2", "--training-steps", "10"] + EMA
    if kind == "iterable":
        base = base + ["--iterable-dataset"]
    whole, _ = _stop_at(d, "501", 4, base=base)
    _stop_at(d, "502", 2, base=base)
    part, out = _stop_at(d, "503", 4, ["--checkpoint-id", "502"], base=base)
    assert "Parameter EMA loaded from checkpoint (2 updates)" in out
    dg = next(ln for ln in out.splitlines() if "Checkpoint digest verified:" in ln)
    assert " ema=" in dg and " params=" in dg, dg
    a, b = _load(whole), _load(part)
    assert torch.equal(_flat(a["ema"]), _flat(b["ema"])) and torch.equal(_flat(a["model"]), _flat(b["model"]))
    assert a["meta"]["ema"] == b["meta"]["ema"] == {"decay": DECAY, "every": 1, "updates": 4}
    assert not torch.equal(_flat(a["ema"]), _flat(a["model"]).float())


# ------------------------------------------------------------------------------- 7. the file
def _storage_span(path, tail):
    with zipfile.ZipFile(path) as z:
        zi = next(i for i in z.infolist() if i.filename.split("/", 1)[-1] == tail)
    with open(path, "rb") as f:
        f.seek(zi.header_offset)
        hdr = f.read(30)
    nlen, xlen = struct.unpack_from("<HH", hdr, 26)
    return zi.header_offset + 30 + nlen + xlen, zi.file_size


def _verify_cmd(path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "fault_tolerant_llm_training_amd.ckpt", "verify", path],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    return r.returncode, r.stdout + r.stderr


def test_file_with_an_ema_entry_loads_verifies_and_detects_a_flipped_byte(tmp_path, chain):
    from fault_tolerant_llm_training_amd.ckpt.verify import read_digest_record

    _, files = chain
    d = str(tmp_path)
    ckd = os.path.join(d, "ck")
    os.makedirs(ckd)
    path = checkpoint_file(ckd, "600")
    shutil.copy(files[3], path)
    ck = _load(path)  # weights_only=True
    assert list(ck["ema"]) == list(ck["model"])
    assert all(t.dtype == torch.float32 and t.shape == ck["model"][k].shape for k, t in ck["ema"].items())
    rec = {e.name: e for e in read_digest_record(path)}
    assert set(rec) == {"params", "exp_avg", "exp_avg_sq", "ema"}
    assert rec["ema"].dtype == "float32" and rec["ema"].numel == rec["params"].numel
    rc, out = _verify_cmd(path)
    assert rc == 0 and out.count(": ok ") == 4 and ": ema: ok " in out, out
    off, size = _storage_span(path, rec["ema"].record)
    with open(path, "r+b") as f:
        f.seek(off + size // 2)
        b = f.read(1)
        f.seek(off + size // 2)
        f.write(bytes([b[0] ^ 0xFF]))
    rc, out = _verify_cmd(path)
    bad = [ln for ln in out.splitlines() if "MISMATCH" in ln]
    assert rc == 1 and len(bad) == 1 and ": ema: " in bad[0], out
    rc, out = run_train(d, "601", SYN + EMA + ["--checkpoint-path", ckd, "--checkpoint-id", "600"])
    assert rc != 0 and "CheckpointCorrupt" in out and "Resuming training" not in out, out[-3000:]
    line = next(ln for ln in out.splitlines() if "[CHECKPOINT]" in ln)
    assert "buffer ema" in line, line


# ------------------------------------------------------------------------------- 8. flag mismatches
def test_flag_mismatches_across_a_resume(tmp_path, chain):
    _, files = chain
    d = str(tmp_path)
    ckd = os.path.join(d, "ck")
    os.makedirs(ckd)
    shutil.copy(files["off"], checkpoint_file(ckd, "700"))
    shutil.copy(files[3], checkpoint_file(ckd, "701"))
    # a flag-off file resumed with the flag: the average starts from the restored parameters
    path, out = _stop_at(d, "702", 3, EMA + ["--checkpoint-id", "700"])
    assert out.count("the checkpoint has no ema entry") == 1 and "Checkpoint digest of ema" not in out, out[-3000:]
    ck = _load(path)
    assert torch.equal(_flat(ck["ema"]), _flat(ck["model"]).float()) and ck["meta"]["ema"]["updates"] == 0
    one, _ = _stop_at(d, "703", 4, EMA + ["--checkpoint-id", "700"])
    ck1 = _load(one)
    assert ck1["meta"]["ema"]["updates"] == 1
    assert torch.equal(_flat(ck1["ema"]), _oracle(_flat(ck["ema"]), _flat(ck1["model"]), E.one_minus_decay(DECAY)))
    # a file with the entry resumed without the flag: ignored, and this job's file has none
    path, out = _stop_at(d, "704", 4, ["--checkpoint-id", "701"])
    assert out.count("--ema-decay is not set") == 1 and "ignored" in out, out[-3000:]
    assert "ema" not in _load(path)
    # changed settings are allowed and logged in one line
    path, out = _stop_at(d, "705", 4, ["--ema-decay", "0.9", "--checkpoint-id", "701"])
    assert out.count("settings differ from the checkpoint's (decay 0.99 -> 0.9)") == 1, out[-3000:]
    ck9 = _load(path)
    assert ck9["meta"]["ema"] == {"decay": 0.9, "every": 1, "updates": 4}
    assert torch.equal(_flat(ck9["ema"]), _oracle(_flat(_load(files[3])["ema"]), _flat(ck9["model"]),
                                                  E.one_minus_decay(0.9)))


# ------------------------------------------------------------------------------- 9. data parallel (gloo)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _torchrun(d, job, args, world=2):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "train.py")] + args
    r = subprocess.run(cmd, cwd=d, env=env_for(d, job, {"OMP_NUM_THREADS": "1"}), capture_output=True, text=True,
                       timeout=600)
    return r.returncode, r.stdout + r.stderr


@pytest.mark.slow
def test_zero1_and_allreduce_under_gloo_follow_the_recurrence_and_resume_on_one_rank(tmp_path):
    """W = 2 (one sequence per rank, fp32 model) in both gradient modes: the average, its ZeRO-1 shards
    assembled by the sharded save, is the oracle recurrence over that run's own parameters, starting
    from the parameters every world size initialises alike; the W = 2 ZeRO-1 file resumed by one
    process carries the same average.

    Equality with the single-process run of the same global batch cannot hold bit for bit, with or
    without the average: the parameters themselves differ across world sizes after the first step
    (another summation order of the gradient; measured after 3 steps of this configuration:
    max |p - p_single| = 2.7e-6 under all-reduce and 2.5e-6 under ZeRO-1, max |ema - ema_single| =
    1.2e-7 in both). So each run's average is held to its own parameters, which is what that
    equality would establish if the parameters agreed."""
    d = str(tmp_path)
    ckd = os.path.join(d, "ck")
    common = ["--device", "cpu", "--model", "tiny", "--sequence-length", "32", "--logging-frequency", "5",
              "--prefetch", "1", "--synthetic-data", "--vocab-size", "256", "--learning-rate", "1e-3",
              "--lr-warmup-steps", "2", "--training-steps", "10", "--model-dtype", "fp32", "--checkpoint-path", ckd,
              "--raise-error"] + EMA
    rc, out = run_train(d, "800", common + ["--batch-size", "2", "--error-step", "0"])
    assert rc == 0, out[-3000:]
    p0 = _flat(_load(checkpoint_file(ckd, "800"))["model"])
    omd = E.one_minus_decay(DECAY)
    last = {}
    for mode, jobs in (("zero1", ("811", "812")), ("allreduce", ("821", "822"))):
        e = p0.clone()
        for k, job in enumerate(jobs, start=1):
            rc, out = _torchrun(d, job, common + ["--batch-size", "1", "--dp-mode", mode, "--dp-bucket-mb", "0.1",
                                                  "--error-step", str(k)])
            assert rc == 0 and f"Data parallel over 2 ranks: {mode}" in out, out[-3000:]
            assert ("sharded like the AdamW moments" in out) == (mode == "zero1")
            ck = _load(checkpoint_file(ckd, job))
            e = _oracle(e, _flat(ck["model"]), omd)
            assert torch.equal(_flat(ck["ema"]), e), (mode, k)
            assert ck["meta"]["ema"] == {"decay": DECAY, "every": 1, "updates": k}
        assert not torch.equal(e, p0)
        last[mode] = ck
    rc, out = _verify_cmd(checkpoint_file(ckd, "812"))
    assert rc == 0 and ": ema: ok " in out, out
    # the W = 2 ZeRO-1 file resumed by one process: the same average, digest verified
    rc, out = run_train(d, "830", common + ["--batch-size", "2", "--error-step", "2", "--checkpoint-id", "812"])
    assert rc == 0 and "Parameter EMA loaded from checkpoint (2 updates)" in out, out[-3000:]
    assert " ema=" in next(ln for ln in out.splitlines() if "Checkpoint digest verified:" in ln)
    assert torch.equal(_flat(_load(checkpoint_file(ckd, "830"))["ema"]), _flat(last["zero1"]["ema"]))


# ------------------------------------------------------------------------------- 10. the swap
def test_ema_weights_swaps_in_the_cast_average_and_puts_the_weights_back():
    m, red, opt = _mini(ema_decay=DECAY)
    for i in (1, 2, 3):
        _step(m, red, opt, i)
    old, avg = m.flat.params.clone(), opt.ema.clone()
    moments = [t.clone() for t in opt.moments()]
    assert not torch.equal(avg.to(old.dtype), old)
    with opt.ema_weights():
        assert torch.equal(m.flat.params, avg.to(torch.bfloat16))
        assert torch.equal(opt.ema, avg)
    assert torch.equal(m.flat.params, old) and torch.equal(opt.ema, avg)
    assert all(torch.equal(a, b) for a, b in zip(moments, opt.moments()))
    with pytest.raises(ZeroDivisionError):  # an error inside still restores the weights
        with opt.ema_weights():
            1 / 0
    assert torch.equal(m.flat.params, old)
    _m2, _r2, plain = _mini()
    assert plain.ema is None
    with pytest.raises(RuntimeError, match="ema_decay"):
        with plain.ema_weights():
            pass


def _eval_records(path):
    return [r for r in (json.loads(ln) for ln in open(path).read().splitlines() if ln.strip()) if "eval_step" in r]


def test_eval_ema_adds_fields_and_leaves_the_others(tmp_path):
    recs, cks = {}, {}
    for name, extra in (("plain", []), ("ema", ["--eval-ema"])):
        d = str(tmp_path / name)
        os.makedirs(d)
        path, out = _stop_at(d, "1", 5, EMA + ["--eval-every", "2", "--eval-sequences", "4", "--metrics-file",
                                               "m.jsonl"] + extra)
        recs[name], cks[name] = _eval_records(os.path.join(d, "m.jsonl")), _load(path)
        if extra:
            assert "| ema_loss: " in next(ln for ln in out.splitlines() if "Evaluation at step 2 |" in ln)
    assert [r["eval_step"] for r in recs["plain"]] == [r["eval_step"] for r in recs["ema"]] == [2, 4]
    for a, b in zip(recs["plain"], recs["ema"]):
        new = set(b) - set(a)
        assert new == {"ema_loss", "ema_loss_fx", "ema_perplexity", "ema_accuracy", "ema_correct", "ema_nonfinite",
                       "ema_s"}
        assert {k: v for k, v in a.items() if k != "eval_s"} == {k: b[k] for k in a if k != "eval_s"}
        assert isinstance(b["ema_loss_fx"], int) and b["ema_loss"] == b["ema_loss_fx"] / 2 ** 24 / b["eval_tokens"]
        assert b["ema_loss_fx"] != b["eval_loss_fx"]
    for key in ("model", "ema"):
        assert torch.equal(_flat(cks["plain"][key]), _flat(cks["ema"][key]))
    for x, y in zip(_moments(cks["plain"]), _moments(cks["ema"])):
        assert torch.equal(x, y)


def _generate(argv):
    from fault_tolerant_llm_training_amd import generate

    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        rc = generate.main(argv)
    return rc, out.getvalue(), err.getvalue()


def test_generate_use_ema_reads_the_cast_average(chain):
    from fault_tolerant_llm_training_amd.ckpt.state import restore_model
    from fault_tolerant_llm_training_amd.generation import generate
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for
    from fault_tolerant_llm_training_amd.utils.sround import key_from_seed

    _, files = chain
    argv = ["--checkpoint", files[3], "--model", "tiny", "--vocab-size", "256", "--device", "cpu", "--prompt-ids",
            "1,7,9", "--max-new-tokens", "6", "--temperature", "0.8", "--seed", "5", "--json"]
    rc, out, err = _generate(argv + ["--use-ema"])
    assert rc == 0, err
    ck = _load(files[3])
    m = build_model(model_args_for("tiny", vocab_size=256, seq_len=32), "cpu", torch.bfloat16)
    restore_model(m, {k: v.to(torch.bfloat16) for k, v in ck["ema"].items()})
    m.eval()
    want = generate(m, [1, 7, 9], 6, temperature=0.8, top_k=0, key=key_from_seed(5), eos_id=None)
    assert json.loads(out)["ids"] == want
    assert not torch.equal(_flat(ck["ema"]).bfloat16(), _flat(ck["model"]))
    rc, out, err = _generate([files["off"] if a == files[3] else a for a in argv] + ["--use-ema"])
    assert rc == 2 and "has no ema entry" in err and out == "", (rc, out, err)


# ------------------------------------------------------------------------------- 11. argument checks
@pytest.mark.parametrize("argv,needle", [
    (["--ema-decay", "0.99", "--ema-every", "2", "--hip-graph"], "--ema-every"),
    (["--ema-decay", "0.99", "--ema-every", "2", "--compile"], "--ema-every"),
    (["--eval-ema", "--eval-every", "2", "--synthetic-data"], "--eval-ema"),
    (["--eval-ema", "--ema-decay", "0.99"], "--eval-ema"),
    (["--sample-ema", "--sample-every", "2", "--synthetic-data"], "--sample-ema"),
    (["--ema-decay", "1.0"], "--ema-decay"),
    (["--ema-decay", "-0.1"], "--ema-decay"),
    (["--ema-decay", "0.99", "--ema-every", "0"], "--ema-every"),
])
def test_bad_flag_combinations_are_refused(argv, needle, capsys):
    from fault_tolerant_llm_training_amd.utils.config import get_args

    with pytest.raises(SystemExit):
        get_args(argv)
    assert needle in capsys.readouterr().err


def test_flags_default_to_off_and_accept_the_documented_forms():
    from fault_tolerant_llm_training_amd.utils.config import get_args

    a = get_args([])
    assert a.ema_decay == 0.0 and a.ema_every == 1 and not a.eval_ema and not a.sample_ema
    a = get_args(["--ema-decay", "0.999", "--ema-every", "10"])
    assert a.ema_decay == 0.999 and a.ema_every == 10
    assert get_args(["--ema-decay", "0.99", "--hip-graph"]).hip_graph
    assert get_args(["--ema-decay", "0.99", "--eval-ema", "--eval-every", "5", "--synthetic-data"]).eval_ema
    assert get_args(["--ema-decay", "0.99", "--sample-ema", "--sample-every", "5", "--synthetic-data",
                     "--sequence-length", "128"]).sample_ema
