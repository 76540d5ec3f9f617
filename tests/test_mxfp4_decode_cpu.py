"""Weight-only MXFP4 decode without a GPU: the format's definition (utils/mxfp4.py), the composed route
of the ``_mx4`` ops, generation with ``Mxfp4Weights`` on that route, and the refusals."""
import pytest
import torch

VALUES = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
TIES = {0.25: 0.0, 0.75: 1.0, 1.25: 1.0, 1.75: 2.0, 2.5: 2.0, 3.5: 4.0, 5.0: 4.0}


def _block(head, fill=0.0):
    """One block of 32 weights: ``head``, then ``fill``."""
    return torch.tensor(list(head) + [fill] * (32 - len(head)))


@pytest.mark.parametrize("p", [-126, -20, 0, 9, 120])
def test_representable_values_times_a_power_of_two_survive_exactly(p):
    from fault_tolerant_llm_training_amd.utils import mxfp4

    w = torch.ldexp(torch.cat([VALUES, -VALUES]).repeat(2), torch.tensor(p)).view(1, 32)
    codes, scales = mxfp4.quantize_rows(w)
    assert scales.tolist() == [[p + 127]]
    assert codes.view(-1)[:8].tolist() == [0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE]  # low nibble first
    assert torch.equal(mxfp4.dequant(codes, scales), w.double())


def test_ties_zero_blocks_and_non_finite_blocks():
    from fault_tolerant_llm_training_amd.ops import decode as D
    from fault_tolerant_llm_training_amd.utils import mxfp4

    ties = torch.tensor(list(TIES))
    w = torch.stack([_block([6.0, *ties, *-ties]) / 8, _block([0.0, -0.0, 0.0, -0.0]),
                     _block([1.0, float("inf")]), _block([float("nan")], 2.0)]).view(2, 64)
    codes, scales = mxfp4.quantize_rows(w)
    deq = mxfp4.dequant(codes, scales)
    want = torch.tensor(list(TIES.values()), dtype=torch.float64) / 8
    assert torch.equal(deq[0, 1:8], want) and torch.equal(deq[0, 8:15], -want)
    assert scales.tolist() == [[124, 127], [255, 255]]
    assert codes[0, 16:18].tolist() == [0x80, 0x80] and int(codes[0, 18:].sum()) == 0  # the zero block keeps its signs
    assert int(codes[1].sum()) == 0 and bool(torch.isnan(deq[1]).all())
    y = D.gemv_mx4(torch.ones(64, dtype=torch.float64), codes, scales)
    assert bool(torch.isnan(y[1])) and float(y[0]) == float(deq[0].sum())


@pytest.mark.parametrize("edge", [6.0, 4.0])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_scale_is_the_smallest_power_of_two_that_holds_amax(dtype, edge):
    """amax just below, at and just above ``edge * 2^p``: only the float above 6 * 2^p needs 2^(p + 1)."""
    from fault_tolerant_llm_training_amd.utils import mxfp4

    at = torch.tensor(edge * 2.0 ** -5, dtype=dtype)
    lo, hi = (torch.nextafter(at.float(), torch.tensor(s)).to(dtype) for s in (0.0, 1.0))
    if dtype == torch.bfloat16:  # the neighbours in bf16: one ulp of 2^-7 relative
        lo, hi = at * (1 - 2.0 ** -8), at * (1 + 2.0 ** -7)
    w = torch.stack([_block([0.001, -float(a)], 0.01) for a in (lo, at, hi)]).to(dtype)
    _, scales = mxfp4.quantize_rows(w)
    assert scales.view(-1).tolist() == [122, 122, 123 if edge == 6.0 else 122]
    amax = w.float().abs().amax(dim=1).double()
    s = torch.ldexp(torch.ones(3, dtype=torch.float64), scales.view(-1).long() - 127)
    assert bool((amax <= 6 * s).all()) and bool((amax > 3 * s).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_error_is_below_a_third_of_the_block_amax(dtype):
    """The widest code spacing is 2 (between 4 and 6), so the error is at most one scale, and scale < amax / 3."""
    from fault_tolerant_llm_training_amd.utils import mxfp4

    gen = torch.Generator().manual_seed(1)
    w = (torch.randn(9, 256, generator=gen) * torch.logspace(-6, 3, 9)[:, None]).to(dtype)
    err = (mxfp4.dequant(*mxfp4.quantize_rows(w)) - w.double()).abs().view(9, 8, 32)
    amax = w.double().abs().view(9, 8, 32).amax(dim=2, keepdim=True)
    assert bool((err < amax / 3).all())


def test_composed_ops_obey_the_contract_identities():
    from fault_tolerant_llm_training_amd.ops import decode as D
    from fault_tolerant_llm_training_amd.ops.functional import swiglu_reference
    from fault_tolerant_llm_training_amd.utils import mxfp4

    gen = torch.Generator().manual_seed(2)
    w, x, res = (torch.randn(s, generator=gen, dtype=torch.float64) for s in ((10, 64), (3, 64), (3, 10)))
    codes, scales = D.quantize_rows_mx4(w)
    assert torch.equal(codes, mxfp4.quantize_rows(w)[0]) and codes.shape == (10, 32) and scales.shape == (10, 2)
    y = D.gemv_mx4(x[0], codes, scales)
    assert torch.equal(y, torch.mv(mxfp4.dequant(codes, scales), x[0]))
    assert torch.equal(D.gemv_mx4(x[0], codes, scales, res[0]), y + res[0])
    assert torch.equal(D.gemv_swiglu_mx4(x[0], codes, scales), swiglu_reference(y))
    rows, rows_res, act = (D.gemv_rows_mx4(x, codes, scales), D.gemv_rows_mx4(x, codes, scales, res),
                           D.gemv_swiglu_rows_mx4(x, codes, scales))
    for r in range(3):
        assert torch.equal(rows[r], D.gemv_mx4(x[r], codes, scales))
        assert torch.equal(rows_res[r], D.gemv_mx4(x[r], codes, scales, res[r]))
        assert torch.equal(act[r], D.gemv_swiglu_mx4(x[r], codes, scales))


def test_generation_with_mxfp4_weights_and_its_refusals():
    from fault_tolerant_llm_training_amd.generation import Mxfp4Weights, generate, generate_batch
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    margs = model_args_for("tiny", vocab_size=264, seq_len=32)
    model = build_model(margs, "cpu", torch.float64, seed=7)
    w4 = Mxfp4Weights(model)
    prompts = [[5, 9, 100, 3], [7]]
    one = [generate(model, p, 6, weights=w4) for p in prompts]
    assert generate_batch(model, prompts, 6, weights=w4) == one
    assert generate_batch(model, prompts, 6, weights=w4, graph=True) == one
    codes = w4.head[0]
    w4.requantize()
    assert w4.head[0] is codes and w4.nbytes == sum(
        w.numel() // 2 + w.numel() // 32 for _, w in w4._sources())
    with pytest.raises(ValueError, match="Mxfp4Weights"):
        Mxfp4Weights(build_model(margs, "cpu", torch.float32, seed=7))
    with pytest.raises(ValueError, match="MXFP4"):
        generate_batch(model, prompts, 2, weights=w4, mma=True)


@pytest.mark.parametrize("extra, message", [(["--model-dtype", "fp32"], "--weight-dtype mxfp4"),
                                            (["--model-dtype", "bf16", "--decode-mma", "--num-samples", "2"],
                                             "--decode-mma has no MXFP4")])
def test_cli_refusals(capsys, extra, message):
    from fault_tolerant_llm_training_amd.generate import main

    rc = main(["--checkpoint", "none.ckpt", "--model", "tiny", "--vocab-size", "256", "--device", "cpu",
               "--prompt-ids", "1,2", "--weight-dtype", "mxfp4", *extra])
    assert rc == 2 and capsys.readouterr().err.startswith("generate: error: " + message)
