"""The digest kernel (csrc/kernels/digest.hip) against the CPU tensor_digest, and the digest
record of checkpoints the engine writes from GPU buffers."""
import pytest
import torch

from fault_tolerant_llm_training_amd.utils.digest import digest_accum, tensor_digest

pytestmark = pytest.mark.gpu

MOD = 1_000_003
M64 = (1 << 64) - 1
DEV = "cuda:0"
SIZES = [0, 1, 7, 8, 9, 255, 256 * 8 + 3, MOD - 1, MOD, MOD + 1, 2**24 + 5]
FIRST = [0, 3 * MOD - 2, 2**33 + 5]  # just below a multiple of the modulus; beyond 2^32


def _raw(seed, n, dtype):
    """n elements with uniformly random raw bits (negative views, NaNs, infinities), on the CPU."""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32:
        return torch.randint(-2**31, 2**31, (n,), generator=g, dtype=torch.int32).view(dtype)
    return torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int16).view(dtype)


def _kernel(t, first_pos=0, acc=None, slot=0):
    if acc is None:
        acc = torch.zeros(1, dtype=torch.int64, device=t.device)
    digest_accum(acc, slot, t, first_pos)
    return acc


def _u64(acc, slot=0):
    return int(acc[slot].item()) & M64


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_kernel_matches_cpu_digest(dtype):
    nmax = max(SIZES)
    host = _raw(21, nmax + 3, dtype)   # one storage; views start 0, 1 and 3 elements into it
    dev = host.to(DEV)
    assert dev.data_ptr() % 16 == 0
    for n in SIZES:
        for start in (0, 1, 3):        # 1 and 3: the head is not 16-byte aligned
            for fp in (FIRST if n in (9, 256 * 8 + 3, MOD + 1) else FIRST[:1]):
                want = int(tensor_digest(host[start : start + n], fp), 16)
                got = _u64(_kernel(dev[start : start + n], fp))
                assert got == want, (dtype, n, start, fp)


def test_pieces_slots_and_accumulation():
    n = 3 * MOD + 17
    host = _raw(22, n, torch.bfloat16)
    dev = host.to(DEV)
    whole = int(tensor_digest(host), 16)
    acc = torch.zeros(3, dtype=torch.int64, device=DEV)
    cuts = [0, 12_345, MOD + 2, n]     # three unequal pieces into one slot
    for lo, hi in zip(cuts, cuts[1:]):
        digest_accum(acc, 1, dev[lo:hi], lo)
    assert _u64(acc, 1) == whole
    assert _u64(acc, 0) == 0 and _u64(acc, 2) == 0           # slots are kept apart
    other = _raw(23, 4099, torch.float32)
    digest_accum(acc, 2, other.to(DEV), 5)
    assert _u64(acc, 2) == int(tensor_digest(other, 5), 16) and _u64(acc, 1) == whole
    digest_accum(acc, 1, dev, 0)                              # no zeroing in between: adds
    assert _u64(acc, 1) == (2 * whole) & M64
    a, b = _kernel(dev, 7), _kernel(dev, 7)                   # two runs, equal bits
    assert torch.equal(a, b)


def test_tensor_digest_on_the_gpu_is_the_cpu_value():
    for dtype, n in ((torch.bfloat16, 100_003), (torch.float16, 4097), (torch.float32, MOD + 9)):
        host = _raw(24, n, dtype)
        assert tensor_digest(host.to(DEV)) == tensor_digest(host)
        assert tensor_digest(host.to(DEV), 2**33 + 5) == tensor_digest(host, 2**33 + 5)
    # a non-contiguous view and a dtype the kernel does not cover take their old paths
    host = _raw(25, 4096, torch.float32).view(64, 64)
    assert tensor_digest(host.to(DEV).t()) == tensor_digest(host.t())
    d = torch.arange(1000, dtype=torch.float64)
    assert tensor_digest(d.to(DEV)) == tensor_digest(d)


def test_op_refuses_what_it_does_not_cover():
    acc = torch.zeros(2, dtype=torch.int64, device=DEV)
    t = torch.zeros(16, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        torch.ops.ftamd.digest_accum_(acc, 0, torch.zeros(16, dtype=torch.float64, device=DEV), 0)
    with pytest.raises(RuntimeError):
        torch.ops.ftamd.digest_accum_(acc, 2, t, 0)
    with pytest.raises(RuntimeError):
        torch.ops.ftamd.digest_accum_(acc, 0, t, -1)
    with pytest.raises(RuntimeError):
        torch.ops.ftamd.digest_accum_(acc.to(torch.int32), 0, t, 0)
    torch.cuda.synchronize()
    assert _u64(acc, 0) == 0 and _u64(acc, 1) == 0


# ------------------------------------------------------------------ engine
def _setup(seed):
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for
    from fault_tolerant_llm_training_amd.optim.adamw import FlatAdamW
    from fault_tolerant_llm_training_amd.parallel.ddp import GradReducer
    from fault_tolerant_llm_training_amd.utils.lr import build_lr_scheduler

    a = model_args_for("tiny", vocab_size=1024, seq_len=128)
    m = build_model(a, DEV, torch.bfloat16, seed=seed)
    red = GradReducer(m.flat, m.sinks_in_backward_order(), bucket_mb=1.0)
    opt = FlatAdamW(m.parameters(), m.flat, lr=1e-3, max_grad_norm=1.0, reducer=red)
    m.gate = opt.gate
    s = build_lr_scheduler(opt, 3)
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(0, 1024, (2, 128), generator=g).to(DEV)

    def fwd_bwd():
        m(tok, tok).backward()
        red.finish()
        opt.clip_grad_norm_(1.0)

    fwd_bwd()
    opt.step()
    s.step()
    return m, opt, s, fwd_bwd


def _buffers(m, opt):
    return {"params": m.flat.params, "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq}


@pytest.mark.parametrize("mode", ["hbm", "host"])
@pytest.mark.parametrize("blocking", [True, False])
def test_engine_record_describes_the_snapshot(tmp_path, mode, blocking):
    from test_digest_cpu import _flip_bit

    from fault_tolerant_llm_training_amd._native import runtime_available
    from fault_tolerant_llm_training_amd.ckpt.engine import CheckpointEngine
    from fault_tolerant_llm_training_amd.ckpt.format import load_checkpoint
    from fault_tolerant_llm_training_amd.ckpt.state import build_checkpoint, restore_model
    from fault_tolerant_llm_training_amd.ckpt.verify import CheckpointCorrupt, read_digest_record, verify_restored

    assert runtime_available()
    m, opt, s, fwd_bwd = _setup(0)
    fwd_bwd()                          # gradients for the step that follows the save
    opt.gate.wait_all()
    torch.cuda.synchronize()
    before = {k: tensor_digest(v.cpu()) for k, v in _buffers(m, opt).items()}
    eng = CheckpointEngine(_buffers(m, opt), mode=mode)
    path = str(tmp_path / "checkpoint_3.ckpt")
    eng.save(path, lambda host: build_checkpoint(m, opt, s, 2, host), step=2, blocking=blocking)
    eng.fence()                        # as the trainer does ahead of optimizer.step
    opt.step()                         # the record must describe the state before this step
    eng.wait()
    torch.cuda.synchronize()
    assert tensor_digest(m.flat.params) != before["params"]
    rec = read_digest_record(path)
    assert {e.name: f"{e.digest:016x}" for e in rec} == before
    assert all(e.dtype == "bfloat16" and e.numel == m.flat.numel and e.record.startswith("data/") for e in rec)

    m2, opt2, _, _ = _setup(1)
    c = load_checkpoint(path)
    restore_model(m2, c["model"])
    opt2.load_state_dict(c["optimizer"])
    assert verify_restored(rec, _buffers(m2, opt2), path=path) == before
    del c
    _flip_bit(path, "exp_avg")
    c = load_checkpoint(path)
    restore_model(m2, c["model"])
    opt2.load_state_dict(c["optimizer"])
    with pytest.raises(CheckpointCorrupt) as ei:
        verify_restored(read_digest_record(path), _buffers(m2, opt2), path=path)
    assert ei.value.buffer == "exp_avg"
