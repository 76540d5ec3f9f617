"""Weight-only FP8 decode without a GPU: the format's definition (utils/fp8.py) against torch's
float8_e4m3fn conversion, generation with ``Fp8Weights`` on the composed route, the CLI's refusal."""
import pytest
import torch


def _tie_row():
    from fault_tolerant_llm_training_amd.utils import fp8

    v = fp8.decode_table()[:127]
    mids = torch.cat([torch.tensor([448.0]), (v[:-1] + v[1:]) / 2])  # amax, then every e4m3 midpoint
    return (mids * 2.0 ** -8 * torch.tensor([1.0, -1.0]).repeat(64)[:127]).float()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_definition_codes_are_torchs_e4m3_conversion(dtype):
    from fault_tolerant_llm_training_amd.utils import fp8

    w = (0.02 * torch.randn(9, 127, generator=torch.Generator().manual_seed(1))).to(dtype)
    w[1] = _tie_row().to(dtype)
    w[2] = 0.0
    w[2, 5] = -0.0
    w[3, 7] = 4096 * w[3].abs().max()
    w[4, 0] = float("inf")
    codes, scale = fp8.quantize_rows(w)
    f = w.float()
    amax = f.abs().amax(dim=1)
    assert torch.equal(scale[[0, 1, 3]], amax[[0, 1, 3]] / 448) and scale[2] == 1 and torch.isnan(scale[4])
    inv = torch.where(amax == 0, torch.ones_like(amax), torch.full_like(amax, 448.0) / amax)  # one IEEE division
    want = (f * inv[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    keep = torch.arange(9) != 4  # the non-finite row: zero codes by definition
    assert torch.equal(codes[keep], want[keep]) and int(codes[4].sum()) == 0
    assert codes[2].tolist() == [0] * 5 + [0x80] + [0] * 121
    # decode inverts encode on every finite code, and dequant is code * scale in float64
    table = fp8.decode_table()
    finite = torch.arange(256)[~torch.isnan(table)]
    assert torch.equal(fp8.e4m3_rne(table[finite].float()), finite.to(torch.uint8))
    assert torch.equal(table[finite], finite.to(torch.uint8).view(torch.float8_e4m3fn).double())
    assert torch.equal(fp8.dequant(codes[:4], scale[:4]), table[codes[:4].long()] * scale[:4].double()[:, None])


def test_generate_with_fp8_weights_equals_a_forward_on_the_dequantized_weights():
    from fault_tolerant_llm_training_amd.generation import (Fp8Weights, KVCache, decode_step, generate, generate_batch,
                                                            prefill)
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for
    from fault_tolerant_llm_training_amd.utils import fp8

    margs = model_args_for("tiny", vocab_size=264, seq_len=32)
    model, deq = (build_model(margs, "cpu", torch.float64, seed=7) for _ in range(2))
    w8 = Fp8Weights(model)
    with torch.no_grad():
        for layer, qs in zip(deq.layers.values(), w8.layers):
            at, ff = layer.attention, layer.feed_forward
            for dst, (c, s) in zip((at.wqkv, at.wo.weight, ff.w13, ff.w2.weight), qs):
                dst.copy_(fp8.dequant(c, s))
        deq.output.weight.copy_(fp8.dequant(*w8.head))
    prompt = [5, 9, 100, 3]
    ca, cb = (KVCache(margs, 12, "cpu", torch.float64) for _ in range(2))
    la, lb = prefill(model, prompt, ca), prefill(model, prompt, cb)  # the prompt: the unquantized weights
    ids = []
    for _ in range(8):
        ids.append(int(la.argmax()))
        la, lb = decode_step(model, ids[-1], ca, w8), decode_step(deq, ids[-1], cb)
        assert float((la - lb).norm() / lb.norm()) < 1e-10
    assert generate(model, prompt, 9, weights=w8)[:8] == ids
    assert generate_batch(model, [prompt, [7]], 9, weights=w8)[0][:8] == ids
    with pytest.raises(ValueError):
        Fp8Weights(build_model(margs, "cpu", torch.float32, seed=7))
    with pytest.raises(ValueError):
        generate(deq, prompt, 2, weights=w8)  # another model's weights


def test_cli_refuses_fp8_weights_with_fp32(capsys):
    from fault_tolerant_llm_training_amd.generate import main

    rc = main(["--checkpoint", "none.ckpt", "--model", "tiny", "--vocab-size", "256", "--model-dtype", "fp32",
               "--device", "cpu", "--prompt-ids", "1,2", "--weight-dtype", "fp8"])
    err = capsys.readouterr().err
    assert rc == 2 and err.startswith("generate: error: --weight-dtype fp8")
