"""FP8 KV cache on the CPU: the composed route of the ``_kv8`` ops (``utils.fp8.quantize_rows`` behind
the append, ``utils.fp8.dequant`` in front of ``attn``) through ``generation``, in float64."""
import pytest
import torch

PROMPTS = [[5, 9, 100, 3], [7], [5, 9, 100, 3], [200, 1, 1, 30, 8, 8]]


@pytest.fixture(scope="module")
def tiny():
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    margs = model_args_for("tiny", vocab_size=264, seq_len=32)
    return margs, build_model(margs, "cpu", torch.float64, seed=7)


def _deq(rows):
    from fault_tolerant_llm_training_amd.utils import fp8

    return fp8.dequant(*fp8.quantize_rows(rows.reshape(-1, rows.shape[-1]))).view(rows.shape)


def fp8_values(codes, scale):
    from fault_tolerant_llm_training_amd.utils import fp8

    return fp8.dequant(codes.reshape(-1, codes.shape[-1]), scale.reshape(-1)).view(codes.shape)


def test_kv8_ops_are_the_model_dtype_ops_on_the_dequantized_rows():
    """Append then attend on an FP8 cache against ``qkv_append_`` / ``attn`` on a float64 cache whose rows
    are replaced by dequant(quantize_rows(.)): 1e-10, the bound of the composed paths in
    test_generate_cpu.py. The rows forms are loops over the one-row forms."""
    from fault_tolerant_llm_training_amd.ops import decode as D

    hq, hkv, d, smax = 4, 2, 16, 6
    gen = torch.Generator().manual_seed(3)
    ang = torch.rand(smax, d // 2, generator=gen, dtype=torch.float64) * 6
    cos, sin = ang.cos().float(), ang.sin().float()
    km, vm = (torch.zeros(hkv, smax, d, dtype=torch.float64) for _ in range(2))
    kc, vc = (torch.zeros(hkv, smax, d, dtype=torch.uint8) for _ in range(2))
    ks, vs = (torch.zeros(hkv, smax) for _ in range(2))
    for pos in range(smax):
        qkv = torch.randn((hq + 2 * hkv) * d, generator=gen, dtype=torch.float64) * 2.0 ** (pos - 3)
        qa, qb = qkv.clone(), qkv.clone()
        D.qkv_append_kv8_(qa, cos, sin, pos, kc, vc, ks, vs)
        D.qkv_append_(qb, cos, sin, pos, km, vm)
        km[:, pos], vm[:, pos] = _deq(km[:, pos]), _deq(vm[:, pos])
        assert torch.equal(qa, qb)
        got, want = D.attn_kv8(qa[: hq * d], kc, vc, ks, vs, pos + 1), D.attn(qb[: hq * d], km, vm, pos + 1)
        assert float((got - want).norm() / want.norm()) < 1e-10
    for bad in (-1, smax):
        with pytest.raises(ValueError):
            D.qkv_append_kv8_(qa, cos, sin, bad, kc, vc, ks, vs)
    for bad in (0, smax + 1):
        with pytest.raises(ValueError):
            D.attn_kv8(qa[: hq * d], kc, vc, ks, vs, bad)


def test_generate_is_prefill_and_decode_steps_on_an_fp8_cache(tiny):
    from fault_tolerant_llm_training_amd.generation import KVCache, decode_step, generate, prefill

    margs, model = tiny
    prompt = PROMPTS[0]
    cq, cm = KVCache(margs, 12, "cpu", torch.float64, kv_dtype="fp8"), KVCache(margs, 12, "cpu", torch.float64)
    assert cq.kv_dtype == "fp8" and cq.k.dtype == torch.uint8 and cq.k_scale.shape == cq.k.shape[:-1]
    assert cm.kv_dtype == "model" and cm.k_scale is None
    assert cq.nbytes == 2 * cq.k.numel() + 8 * cq.k_scale.numel() and cm.nbytes == 16 * cm.k.numel()
    lq, lm = prefill(model, prompt, cq), prefill(model, prompt, cm)
    assert torch.equal(lq, lm)  # the prompt's logits come from the unquantized K / V
    for codes, scale, rows in ((cq.k, cq.k_scale, cm.k), (cq.v, cq.v_scale, cm.v)):  # and its rows are the definition's
        P = len(prompt)
        assert torch.equal(fp8_values(codes[:, :, :P], scale[:, :, :P]), _deq(rows[:, :, :P]))
    ids = []
    for _ in range(7):
        ids.append(int(lq.argmax()))
        lq = decode_step(model, ids[-1], cq)
    assert generate(model, prompt, 8, kv_dtype="fp8")[:7] == ids


def test_batch_rows_equal_single_runs_and_model_is_the_default(tiny):
    from fault_tolerant_llm_training_amd.generation import generate, generate_batch

    _, model = tiny
    one = [generate(model, p, 6, kv_dtype="fp8") for p in PROMPTS]
    assert generate_batch(model, PROMPTS, 6, kv_dtype="fp8") == one  # rows 0 and 2: copy_row with scales
    assert generate(model, PROMPTS[0], 6, kv_dtype="model") == generate(model, PROMPTS[0], 6)
    assert generate_batch(model, PROMPTS, 6, kv_dtype="model") == generate_batch(model, PROMPTS, 6)
    for call in (lambda: generate(model, PROMPTS[0], 2, kv_dtype="fp4"),
                 lambda: generate_batch(model, PROMPTS, 2, kv_dtype="bf16")):
        with pytest.raises(ValueError, match="'model' or 'fp8'"):
            call()


def test_cli_takes_kv_dtype_on_the_cpu_and_refuses_fp32_on_the_gpu(capsys):
    from fault_tolerant_llm_training_amd.generate import main

    common = ["--checkpoint", "none.ckpt", "--model", "tiny", "--vocab-size", "256", "--model-dtype", "fp32",
              "--prompt-ids", "1,2", "--kv-dtype", "fp8"]
    assert main(common + ["--device", "cpu"]) == 2  # accepted: the first complaint is the missing file
    assert capsys.readouterr().err.startswith("generate: error: cannot read none.ckpt")
    assert main(common + ["--device", "cuda"]) == 2
    assert capsys.readouterr().err.startswith("generate: error: --kv-dtype fp8")
