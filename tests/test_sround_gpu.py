"""Stochastic rounding of the bf16 AdamW stores on the MI355X: the device primitive against the
oracle (utils/sround.py), the AdamW kernel with the flag (partition / grid invariance, graph-mode refusal,
skip guard, fp32 moments, flag off = today's bits), the tiny model (pipelined = serial)
and the stagnation recipe of test_sround_cpu.py on the device."""
import pytest
import torch

from test_sround_cpu import (KEY, STAG_LR, _bits, run_recipe, stagnation_bound, stagnation_reference)

from fault_tolerant_llm_training_amd.utils.sround import sr_round_bf16

pytestmark = pytest.mark.gpu

HP = (1e-3, 0.9, 0.999, 1e-8, 0.01)  # lr, beta1, beta2, eps, weight decay


def K():
    from fault_tolerant_llm_training_amd._native import kernels

    return kernels()


def _stats(nonfinite=0.0):
    return torch.tensor([0.0, 1.0, nonfinite], device="cuda")


def _state(n, seed, pdt=torch.bfloat16, sdt=None):
    g = torch.Generator().manual_seed(seed)
    p = (torch.randn(n, generator=g) * 0.02).to(pdt).cuda()
    gr = (torch.randn(n, generator=g) * 1e-3).to(pdt).cuda()
    m = (torch.randn(n, generator=g) * 1e-3).to(sdt or pdt).cuda()
    v = (torch.rand(n, generator=g) * 1e-6).to(sdt or pdt).cuda()
    return p, gr, m, v


def _same(a, b):
    return all(torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x,
                           y.view(torch.int16) if y.dtype == torch.bfloat16 else y) for x, y in zip(a, b))


# ------------------------------------------------------------------ the primitive
@pytest.mark.parametrize("offset", [0, (1 << 33) + 8])
@pytest.mark.parametrize("buffer", [0, 1, 2])
def test_primitive_equals_the_oracle(offset, buffer):
    n = 8 * (256 * 3 + 1)  # three whole blocks of 8-element vectors and one more vector
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n, generator=g) * torch.logspace(-30, 30, n, base=2.0)
    x[:6] = torch.tensor([float("inf"), float("-inf"), float("nan"), 1.0, -0.0, 3.3895314e38])
    x[8:16] = torch.randn(8, generator=g).to(torch.bfloat16).float()  # already representable
    want = sr_round_bf16(x, KEY, 9, buffer, offset)
    got = K().sr_round_bf16(x.cuda(), KEY, 9, buffer, offset).cpu()
    nan = torch.isnan(want.float())
    assert torch.equal(torch.isnan(got.float()), nan) and nan.sum() == 1
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan])
    assert torch.equal(got[8:16].float(), x[8:16]) and got[0] == float("inf") and got[1] == float("-inf")


def test_primitive_partial_last_vector():
    x = torch.randn(8 * 5 + 3)
    got = K().sr_round_bf16(x.cuda(), KEY, 2, 0, 16).cpu()
    assert torch.equal(_bits(got), _bits(sr_round_bf16(x, KEY, 2, 0, 16)))


# ------------------------------------------------------------------ adamw_ with the flag
def test_adamw_partition_and_grid_invariance():
    n = 3 * 2048 * 8 + 8
    base = 1 << 33  # flat indices past 2^32: the 8B model has 8.03e9 elements
    whole = _state(n, 1)
    K().adamw_(*whole, _stats(), *HP, 3, 4, None, True, KEY, base)  # 4 blocks: every thread strides 7 times
    flat = _state(n, 1)
    K().adamw_(*flat, _stats(), *HP, 3, 0, None, True, KEY, base)  # one vector per thread
    pieces = _state(n, 1)
    for lo, hi in ((0, 2048 * 8), (2048 * 8, 2 * 2048 * 8), (2 * 2048 * 8, n)):
        K().adamw_(*(t[lo:hi] for t in pieces), _stats(), *HP, 3, 0, None, True, KEY, base + lo)
    torch.cuda.synchronize()
    assert _same(whole, flat) and _same(whole, pieces)
    # the index is global: the same data at another offset rounds differently
    moved = _state(n, 1)
    K().adamw_(*moved, _stats(), *HP, 3, 0, None, True, KEY, base + 8)
    assert not torch.equal(_bits(moved[2]), _bits(whole[2]))


def test_adamw_same_call_same_bits_other_step_other_bits():
    n = 4096
    a, b, c, d = _state(n, 2), _state(n, 2), _state(n, 2), _state(n, 2)
    K().adamw_(*a, _stats(), *HP, 5, 0, None, True, KEY, 0)
    K().adamw_(*b, _stats(), *HP, 5, 0, None, True, KEY, 0)
    K().adamw_(*c, _stats(), *HP, 6, 0, None, True, KEY, 0)
    K().adamw_(*d, _stats(), *HP, 5, 0, None, True, KEY + 1, 0)
    assert _same(a, b)
    # exp_avg does not see the bias corrections: between steps 5 and 6 only its random bits change
    # (two independent roundings of a value differ with probability 2 f (1 - f), 1/3 on average)
    assert (_bits(a[2]) != _bits(c[2])).sum().item() > n // 12
    assert (_bits(a[2]) != _bits(d[2])).sum().item() > n // 12
    # the stored moments are neighbours of the exact fp32 result, not always the nearest
    r = _state(n, 2)
    K().adamw_(*r, _stats(), *HP, 5)
    diff = (a[2].float() - r[2].float()).abs()
    spacing = torch.exp2(torch.floor(torch.log2(r[2].float().abs().clamp_min(1e-30))) - 7)
    assert (diff <= spacing * 1.0001).all() and (diff > 0).any()


def test_adamw_flag_refuses_device_hyper_parameters():
    """Graph replay reads lr and the bias corrections from device memory; the step number of the
    random bits is a launch argument, so the flag is refused there instead of replaying one step's noise."""
    with pytest.raises(RuntimeError, match="graph replay"):
        K().adamw_(*_state(64, 3), _stats(), *HP, 2, 0, torch.zeros(3, device="cuda"), True, KEY, 0)


def test_adamw_nonfinite_skip_leaves_state_untouched():
    a, b = _state(4096, 4), _state(4096, 4)
    K().adamw_(*a, _stats(nonfinite=1.0), *HP, 2, 0, None, True, KEY, 0)
    assert _same(a, b)


def test_adamw_fp32_moments_are_stored_as_without_the_flag():
    a, b = _state(4096, 5, sdt=torch.float32), _state(4096, 5, sdt=torch.float32)
    K().adamw_(*a, _stats(), *HP, 2, 0, None, True, KEY, 0)
    K().adamw_(*b, _stats(), *HP, 2)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert not torch.equal(_bits(a[0]), _bits(b[0]))


@pytest.mark.parametrize("pdt,sdt", [(torch.bfloat16, None), (torch.bfloat16, torch.float32),
                                     (torch.float16, torch.float32), (torch.float32, None)])
def test_adamw_flag_off_defaults_equal_the_old_call(pdt, sdt):
    a, b = _state(4096 + 8, 6, pdt, sdt), _state(4096 + 8, 6, pdt, sdt)
    K().adamw_(*a, _stats(), *HP, 2)
    K().adamw_(*b, _stats(), *HP, 2, 0, None, False, KEY, 1 << 20)  # key / offset unused when off
    assert _same(a, b)


@pytest.mark.parametrize("pdt", [torch.float16, torch.float32])
def test_adamw_flag_refuses_other_parameter_dtypes(pdt):
    a = _state(64, 7, pdt, torch.float32)
    with pytest.raises(RuntimeError, match="bf16 parameters only"):
        K().adamw_(*a, _stats(), *HP, 2, 0, None, True, KEY, 0)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        K().adamw_(*_state(64, 7), _stats(), *HP, 2, 0, None, True, KEY, 4)


# ------------------------------------------------------------------ tiny model, 3 steps
def test_pipelined_optimizer_matches_serial_with_the_flag():
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for
    from fault_tolerant_llm_training_amd.optim.adamw import FlatAdamW
    from fault_tolerant_llm_training_amd.parallel.ddp import GradReducer

    a = model_args_for("tiny", vocab_size=512, seq_len=64)
    g = torch.Generator().manual_seed(0)
    tok = torch.randint(0, 512, (2, 64), generator=g).cuda()
    lab = torch.randint(0, 512, (2, 64), generator=g).cuda()
    out = []
    for pipelined, sr in ((False, True), (True, True), (True, False)):
        m = build_model(a, "cuda", torch.bfloat16, seed=11)
        red = GradReducer(m.flat, m.sinks_in_backward_order(), bucket_mb=0.25) if pipelined else None
        opt = FlatAdamW(m.parameters(), m.flat, lr=1e-2, max_grad_norm=0.0, reducer=red,
                        stochastic_rounding=sr, sr_seed=3)
        m.gate = opt.gate
        for _ in range(3):
            loss = m(tok, lab)
            loss.backward()
            if red is not None:
                red.finish()
            opt.step()
        opt.gate.wait_all()
        torch.cuda.synchronize()
        if pipelined:
            assert len(red.buckets) > 3
        out.append((m.flat.params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()))
    assert _same(out[0], out[1])
    assert not torch.equal(_bits(out[1][0]), _bits(out[2][0]))  # and the flag does something


# ------------------------------------------------------------------ stagnation on the device
def test_stagnation_recipe_on_the_device():
    """The recipe of test_sround_cpu.py through adamw_: same statistics as the CPU oracle, within the
    bound derived there (not bitwise: the bf16 path divides with v_rcp_f32 / v_sqrt_f32)."""
    w0, p32, psr = stagnation_reference()
    stats = _stats()

    def gpu_update(p, g, m, v, step, sr):
        K().adamw_(p, g, m, v, stats, STAG_LR, 0.9, 0.999, 1e-8, 0.0, step, 0, None, sr, KEY, 0)

    off = run_recipe(w0.cuda(), gpu_update, False).cpu()
    on = run_recipe(w0.cuda(), gpu_update, True).cpu()
    want = (p32 - w0.float()).double().mean().item()
    cpu = (psr.float() - w0.float()).double().mean().item()
    got = (on.float() - w0.float()).double().mean().item()
    bound = stagnation_bound(w0)
    same_on = (_bits(on) == _bits(w0)).float().mean().item()
    same_off = (_bits(off) == _bits(w0)).float().mean().item()
    print(f"mean change: fp32 state {want:.6e}, CPU oracle {cpu:.6e}, device {got:.6e}, bound {bound:.2e}; "
          f"unchanged {same_on:.4f} with the flag, {same_off:.3f} without")
    assert same_off > 1.0 / 3.0
    assert abs(got - want) <= bound and abs(got - cpu) <= bound
    assert same_on < 0.01
