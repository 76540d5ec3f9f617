"""Checkpoint state digests on the CPU: tensor_digest(first_pos), the state_digest record the
engine writes, the offline verify command, the resume check in train.py and the sharded save."""
import os
import socket
import struct
import subprocess
import sys
import zipfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fault_tolerant_llm_training_amd._native import runtime_available
from fault_tolerant_llm_training_amd.ckpt.engine import CheckpointEngine
from fault_tolerant_llm_training_amd.ckpt.format import checkpoint_file, load_checkpoint
from fault_tolerant_llm_training_amd.ckpt.state import build_checkpoint, restore_model
from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for
from fault_tolerant_llm_training_amd.optim.adamw import FlatAdamW
from fault_tolerant_llm_training_amd.utils.digest import tensor_digest
from fault_tolerant_llm_training_amd.utils.lr import build_lr_scheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOD = 1_000_003
M64 = (1 << 64) - 1

needs_runtime = pytest.mark.skipif(not runtime_available(), reason="native runtime not built")


def _raw(seed, n, dtype):
    """n elements of ``dtype`` with uniformly random raw bits (negative views, NaNs, infinities)."""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32:
        return torch.randint(-2**31, 2**31, (n,), generator=g, dtype=torch.int32).view(dtype)
    return torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int16).view(dtype)


def _brute(t, first_pos):
    bits = t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).tolist()
    return sum(b * (((first_pos + i) % MOD) + 1) for i, b in enumerate(bits)) & M64


# ------------------------------------------------------------------ tensor_digest
# computed with the tensor_digest(t) of the commit before first_pos existed, same seeds
PINNED = [
    (0, 1000, torch.bfloat16, "ffffffffe30de9be"),
    (1, 2_500_007, torch.float16, "0000060f02ea0a2a"),
    (2, 1_000_010, torch.float32, "f37397f3d0bc4d95"),
    (3, 0, torch.float32, "0000000000000000"),
]


@pytest.mark.parametrize("seed,n,dtype,want", PINNED)
def test_first_pos_zero_is_the_old_digest(seed, n, dtype, want):
    t = _raw(seed, n, dtype)
    assert tensor_digest(t) == want
    assert tensor_digest(t, 0) == want
    assert tensor_digest(t, first_pos=0) == want


def test_other_dtypes_keep_their_old_digest():
    g = torch.Generator().manual_seed(4)
    assert tensor_digest(torch.randn(33, generator=g, dtype=torch.float64)) == "88a22e23985dd4c5"
    g = torch.Generator().manual_seed(5)
    assert tensor_digest(torch.randint(-1000, 1000, (17,), generator=g, dtype=torch.int32)) == "ffffffffffff636f"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_pieces_sum_to_the_whole(dtype):
    n = MOD + 50
    t = _raw(7, n, dtype)
    whole = int(tensor_digest(t), 16)
    for cut in (0, 1, 7, MOD - 1, MOD, MOD + 1):
        a = int(tensor_digest(t[:cut], 0), 16)
        b = int(tensor_digest(t[cut:], cut), 16)
        assert (a + b) & M64 == whole, cut


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_large_first_pos_against_python_ints(dtype):
    t = _raw(8, 50, dtype)
    for fp in (2**33 + 5, MOD - 3, 5 * MOD - 1):
        assert int(tensor_digest(t, fp), 16) == _brute(t, fp), fp


# ------------------------------------------------------------------ the record in the file
def _setup(seed=0, dtype=torch.bfloat16):
    a = model_args_for("tiny", vocab_size=96, seq_len=16)
    m = build_model(a, "cpu", dtype, seed=seed)
    opt = FlatAdamW(m.parameters(), m.flat, lr=1e-3, max_grad_norm=1.0)
    s = build_lr_scheduler(opt, 3)
    tok = torch.randint(0, 96, (2, 16))
    m(tok, tok).backward()
    opt.step()
    s.step()
    return m, opt, s


def _buffers(m, opt):
    return {"params": m.flat.params, "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq}


def _save(tmp_path, m, opt, s, name="checkpoint_7.ckpt", **kw):
    path = str(tmp_path / name)
    CheckpointEngine(_buffers(m, opt), **kw).save(path, lambda host: build_checkpoint(m, opt, s, 5, host),
                                                  step=5, blocking=True)
    return path


def _storage_span(path, tail):
    """(file offset, size) of the bytes of archive member ``*/<tail>`` (stored, so they follow the
    local header at ZipInfo.header_offset)."""
    with zipfile.ZipFile(path) as z:
        zi = next(i for i in z.infolist() if i.filename.split("/", 1)[-1] == tail)
    with open(path, "rb") as f:
        f.seek(zi.header_offset)
        hdr = f.read(30)
    nlen, xlen = struct.unpack_from("<HH", hdr, 26)
    return zi.header_offset + 30 + nlen + xlen, zi.file_size


def _flip_bit(path, buffer):
    """Flip one bit in the middle of the storage that holds ``buffer``."""
    from fault_tolerant_llm_training_amd.ckpt.verify import read_digest_record

    e = next(e for e in read_digest_record(path) if e.name == buffer)
    off, size = _storage_span(path, e.record)
    with open(path, "r+b") as f:
        f.seek(off + size // 2)
        b = f.read(1)
        f.seek(off + size // 2)
        f.write(bytes([b[0] ^ 0x10]))


@needs_runtime
def test_engine_writes_a_record_zipfile_can_read(tmp_path):
    m, opt, s = _setup()
    path = _save(tmp_path, m, opt, s)
    # zipfile + struct alone
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None
        name = next(n for n in z.namelist() if n.endswith("/state_digest"))
        assert "/data/" not in name
        raw = z.read(name)
        big = [i for i in z.infolist() if "/data/" in i.filename and i.file_size > 1000]
        assert len(big) == 3
    magic, version, count = struct.unpack_from("<8sII", raw, 0)
    assert (magic, version, count) == (b"FTDIGEST", 1, 3) and len(raw) == 16 + 3 * 128
    bufs = _buffers(m, opt)
    seen = {}
    for i in range(count):
        nm, rec, dt, numel, dg = struct.unpack_from("<32s64s16sQQ", raw, 16 + i * 128)
        nm, rec, dt = (x.rstrip(b"\0").decode() for x in (nm, rec, dt))
        assert dt == "bfloat16" and numel == bufs[nm].numel()
        assert f"{dg:016x}" == tensor_digest(bufs[nm]), nm
        # the named archive record is that buffer
        off, size = _storage_span(path, rec)
        assert rec.startswith("data/") and size == numel * 2
        with open(path, "rb") as f:
            f.seek(off)
            assert f.read(size) == bufs[nm].view(torch.int16).numpy().tobytes()
        seen[nm] = rec
    assert list(seen) == ["params", "exp_avg", "exp_avg_sq"] and len(set(seen.values())) == 3
    c = torch.load(path, map_location="cpu", weights_only=True)
    assert c["training_step"] == 5
    for k, v in m.state_dict().items():
        assert torch.equal(c["model"][k], v), k

    from fault_tolerant_llm_training_amd.ckpt.verify import read_digest_record

    rec = read_digest_record(path)
    assert [e.name for e in rec] == list(seen) and [e.record for e in rec] == list(seen.values())


@needs_runtime
def test_no_record_when_switched_off_or_without_the_native_writer(tmp_path):
    from fault_tolerant_llm_training_amd.ckpt.verify import read_digest_record

    m, opt, s = _setup()
    assert read_digest_record(_save(tmp_path, m, opt, s, "checkpoint_1.ckpt", digest=False)) is None
    eng = CheckpointEngine(_buffers(m, opt))
    eng.native = False
    eng.digest = False
    p = str(tmp_path / "checkpoint_2.ckpt")
    eng.save(p, lambda host: build_checkpoint(m, opt, s, 5, host), blocking=True)
    assert read_digest_record(p) is None


@needs_runtime
def test_verify_restored_in_process(tmp_path):
    from fault_tolerant_llm_training_amd.ckpt.verify import CheckpointCorrupt, read_digest_record, verify_restored

    m, opt, s = _setup()
    path = _save(tmp_path, m, opt, s)
    m2, opt2, _ = _setup(seed=3)
    c = load_checkpoint(path)
    restore_model(m2, c["model"])
    opt2.load_state_dict(c["optimizer"])
    ok = verify_restored(read_digest_record(path), _buffers(m2, opt2), path=path)
    assert ok == {k: tensor_digest(v) for k, v in _buffers(m, opt).items()}
    del c
    _flip_bit(path, "exp_avg_sq")
    c = load_checkpoint(path)
    opt2.load_state_dict(c["optimizer"])
    with pytest.raises(CheckpointCorrupt) as ei:
        verify_restored(read_digest_record(path), _buffers(m2, opt2), path=path)
    assert ei.value.buffer == "exp_avg_sq" and ei.value.path == path and ei.value.want != ei.value.got
    assert f"{ei.value.want:016x}" in str(ei.value) and f"{ei.value.got:016x}" in str(ei.value)


@needs_runtime
@pytest.mark.parametrize("src,dst", [(torch.float16, torch.float32), (torch.float32, torch.float16)])
def test_converted_moment_dtype_is_skipped_not_failed(tmp_path, src, dst):
    from fault_tolerant_llm_training_amd.ckpt.verify import read_digest_record, verify_restored

    a = model_args_for("tiny", vocab_size=96, seq_len=16)
    m = build_model(a, "cpu", torch.float16, seed=4)
    opt = FlatAdamW(m.parameters(), m.flat, lr=1e-3, max_grad_norm=1.0, state_dtype=src)
    tok = torch.randint(0, 96, (2, 16))
    m(tok, tok).backward()
    opt.step()
    s = build_lr_scheduler(opt, 3)
    path = _save(tmp_path, m, opt, s)
    c = load_checkpoint(path)
    m2 = build_model(a, "cpu", torch.float16, seed=5)
    opt2 = FlatAdamW(m2.parameters(), m2.flat, lr=1e-3, max_grad_norm=1.0, state_dtype=dst)
    restore_model(m2, c["model"])
    opt2.load_state_dict(c["optimizer"])
    lines = []
    ok = verify_restored(read_digest_record(path), _buffers(m2, opt2), path=path, log=lines.append)
    assert list(ok) == ["params"]
    assert len(lines) == 2 and "exp_avg " in lines[0] and "exp_avg_sq " in lines[1]
    assert all("not verified" in ln for ln in lines)


# ------------------------------------------------------------------ offline command
def _verify_cmd(*files):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "fault_tolerant_llm_training_amd.ckpt", "verify", *files],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    return r.returncode, r.stdout + r.stderr


@needs_runtime
def test_verify_command(tmp_path):
    m, opt, s = _setup()
    path = _save(tmp_path, m, opt, s)
    rc, out = _verify_cmd(path)
    assert rc == 0 and out.count(": ok ") == 3, out
    _flip_bit(path, "exp_avg")
    rc, out = _verify_cmd(path)
    assert rc == 1, out
    bad = [ln for ln in out.splitlines() if "MISMATCH" in ln]
    assert len(bad) == 1 and ": exp_avg: " in bad[0], out
    plain = str(tmp_path / "plain.ckpt")
    torch.save({"model": m.state_dict()}, plain)
    rc, out = _verify_cmd(plain)
    assert rc == 2 and "no digest record" in out, out


# ------------------------------------------------------------------ train.py
def _train_base(d):
    from helpers import TINY

    return TINY + ["--synthetic-data", "--vocab-size", "256", "--training-steps", "8", "--lr-warmup-steps", "2"]


@needs_runtime
def test_resume_refuses_a_damaged_checkpoint(tmp_path):
    from helpers import run_train, sbatch_calls, write_fake_sbatch

    d = str(tmp_path)
    write_fake_sbatch(d)
    ck, alt = os.path.join(d, "ck"), os.path.join(d, "alt")
    base = _train_base(d) + ["--checkpoint-path", ck]
    rc, out = run_train(d, "5101", base + ["--raise-error", "--error-step", "3"])
    good = checkpoint_file(ck, "5101")
    assert os.path.exists(good), out[-2000:]

    # the untouched file resumes, verified
    rc, out = run_train(d, "5102", base + ["--checkpoint-id", "5101", "--training-steps", "5"])
    assert rc == 0 and "Checkpoint digest verified: params=" in out and "Resuming training" in out, out[-2000:]
    assert out.index("Checkpoint digest verified") < out.index("Resuming training")

    _flip_bit(good, "params")
    before = sorted(os.listdir(ck))
    n_sbatch = len(sbatch_calls(d))
    rc, out = run_train(d, "5103", base + ["--checkpoint-id", "5101", "--checkpoint-alt-path", alt,
                                           "--prune-consumed", "--save-every", "2"])
    assert rc != 0, out[-2000:]
    line = next(ln for ln in out.splitlines() if "[CHECKPOINT]" in ln)
    assert good in line and "params" in line and "digest" in line, line
    assert "Resuming training" not in out and "Training completed" not in out
    assert sorted(os.listdir(ck)) == before and os.path.exists(good)  # not pruned, nothing new
    assert not os.path.exists(checkpoint_file(alt, "5103")) and not os.path.exists(checkpoint_file(ck, "5103"))
    assert len(sbatch_calls(d)) == n_sbatch  # no resubmission

    # the escape hatch resumes the damaged file as before
    rc, out = run_train(d, "5104", base + ["--checkpoint-id", "5101", "--training-steps", "5",
                                           "--no-verify-checkpoint"])
    assert rc == 0 and "Resuming training" in out and "Checkpoint digest" not in out, out[-2000:]


@needs_runtime
def test_resume_with_converted_moments_logs_the_skip(tmp_path):
    from helpers import run_train, write_fake_sbatch

    d = str(tmp_path)
    write_fake_sbatch(d)
    base = _train_base(d) + ["--checkpoint-path", os.path.join(d, "ck"), "--model-dtype", "fp16"]
    rc, out = run_train(d, "5201", base + ["--optimizer-state-dtype", "fp16", "--raise-error", "--error-step", "2"])
    assert os.path.exists(checkpoint_file(os.path.join(d, "ck"), "5201")), out[-2000:]
    rc, out = run_train(d, "5202", base + ["--checkpoint-id", "5201", "--training-steps", "3"])
    assert rc == 0 and "Resuming training" in out, out[-2000:]
    assert "Checkpoint digest of exp_avg not verified: saved as float16, restored as float32" in out
    assert "Checkpoint digest of exp_avg_sq not verified" in out
    assert "Checkpoint digest verified: params=" in out


# ------------------------------------------------------------------ sharded save, two gloo ranks
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    group = dist.new_group(backend="gloo")
    from fault_tolerant_llm_training_amd.ckpt.engine import Region
    from fault_tolerant_llm_training_amd.ckpt.verify import CheckpointCorrupt, read_digest_record, verify_restored

    n = MOD + 4321  # positions wrap inside the buffer; not a multiple of the piece size
    full = {"params": _raw(11, n, torch.bfloat16), "exp_avg": _raw(12, n, torch.float32)}
    regions = []
    for k, t in full.items():  # ZeRO-1-like: many small pieces per rank, interleaved across ranks
        step, pieces, data, off = 1000, [], [], 0
        for j, lo in enumerate(range(0, n, step)):
            if j % world == rank:
                hi = min(n, lo + step)
                pieces.append((lo, off, hi - lo))
                data.append(t[lo:hi])
                off += hi - lo
        regions.append(Region(k, torch.cat(data), pieces, n))
    eng = CheckpointEngine(regions, group=group, rank=rank, world=world)
    eng.save(path, lambda host: {"model": {"w": host["params"]}, "opt": {"m": host["exp_avg"]}, "training_step": 7},
             blocking=True)
    dist.barrier()
    rec = read_digest_record(path)
    assert [(e.name, e.dtype, e.numel) for e in rec] == [("params", "bfloat16", n), ("exp_avg", "float32", n)]
    for e in rec:
        assert f"{e.digest:016x}" == tensor_digest(full[e.name]), e.name
    live = {r.name: [(r.data[off : off + ln], lo) for lo, off, ln in r.pieces] for r in regions}
    numels = {r.name: n for r in regions}
    ok = verify_restored(rec, live, group=group, path=path, numels=numels)
    assert ok == {k: tensor_digest(v) for k, v in full.items()}
    if rank == 1:  # one element of one rank's shard
        bits = regions[1].data.view(torch.int32)
        bits[bits.numel() // 2] ^= 1
    try:
        verify_restored(rec, live, group=group, path=path, numels=numels)
    except CheckpointCorrupt as e:
        assert e.buffer == "exp_avg"
    else:
        raise AssertionError(f"rank {rank}: a changed shard element went unnoticed")
    dist.barrier()
    dist.destroy_process_group()


@needs_runtime
def test_sharded_record_and_group_verify(tmp_path):
    path = str(tmp_path / "checkpoint_9.ckpt")
    mp.start_processes(_worker, args=(2, _port(), path), nprocs=2, start_method="spawn")
    c = torch.load(path, map_location="cpu", weights_only=True)
    assert c["training_step"] == 7 and torch.equal(c["model"]["w"].view(torch.int16),
                                                   _raw(11, MOD + 4321, torch.bfloat16).view(torch.int16))
    assert zipfile.ZipFile(path).testzip() is None  # the record's CRC too
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "fault_tolerant_llm_training_amd.ckpt", "verify", path],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
