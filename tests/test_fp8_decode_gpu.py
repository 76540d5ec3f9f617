"""Weight-only FP8 decode on the GPU (csrc/kernels/decode_w8.hip): the quantizer against its
definition (utils/fp8.py), the gemv kernels against float64, and generation with ``Fp8Weights``."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
MANT = {torch.bfloat16: 7, torch.float16: 10}
EMIN = {torch.bfloat16: -126, torch.float16: -14}
NS, KS = [1, 5, 257], [16, 1040, 4096, 5136]  # K: one lane, a partial step, one unrolled sweep, sweep + tail


@pytest.fixture(scope="module")
def K():
    from fault_tolerant_llm_training_amd._native import kernels

    return kernels()


def ulp_at(ref, dtype):
    _, e = torch.frexp(ref.abs().clamp(min=2.0 ** -300))
    return torch.ldexp(torch.ones_like(ref), (e - 1).clamp(min=EMIN[dtype]) - MANT[dtype])


def rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen, device="cuda")


def _operands(N, Kd, dtype, gen):
    """Random x, the definition's codes and scale of a random weight, a residual, and float64 W."""
    from fault_tolerant_llm_training_amd.utils import fp8

    x = torch.randn(Kd, generator=gen, device="cuda").to(dtype)
    w = (torch.randn(N, Kd, generator=gen, device="cuda") / math.sqrt(Kd)).to(dtype)
    codes, scale = (t.cuda() for t in fp8.quantize_rows(w.cpu()))
    return x, codes, scale, torch.randn(N, generator=gen, device="cuda").to(dtype), fp8.dequant(codes, scale)


@pytest.mark.parametrize("Kd", [16, 1040, 4096])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_quantizer_equals_the_definition_bit_for_bit(K, dt, N, Kd):
    from fault_tolerant_llm_training_amd.utils import fp8

    dtype = DTYPES[dt]
    gen = torch.Generator().manual_seed(21)
    w = (0.02 * torch.randn(N, Kd, generator=gen)).to(dtype)
    if N >= 5:
        w[1] = 0.0
        w[1, Kd // 2] = -0.0
        w[2, 3] = 4096 * w[2].abs().max()  # the rest of the row: subnormal codes or zero
        v = fp8.decode_table()[:127]
        mids = torch.cat([torch.tensor([448.0]), (v[:-1] + v[1:]) / 2])  # amax, then every e4m3 midpoint
        row = (mids * 2.0 ** -8 * torch.tensor([1.0, -1.0]).repeat(64)[:127]).repeat(Kd // 127 + 1)[:Kd]
        w[3] = row.to(dtype)
        assert torch.equal(w[3].double(), row)  # inv = 2^8 exactly: w * inv are the ties themselves
    want_c, want_s = fp8.quantize_rows(w)
    codes, scale = K.quantize_rows_e4m3(w.cuda())
    assert codes.dtype == torch.uint8 and scale.dtype == torch.float32
    bad = (codes.cpu() != want_c).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), codes.cpu()[tuple(bad[0])], want_c[tuple(bad[0])])
    assert torch.equal(scale.cpu().view(torch.int32), want_s.view(torch.int32))
    again = K.quantize_rows_e4m3(w.cuda())
    assert torch.equal(again[0], codes) and torch.equal(again[1], scale)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_gemv_w8_is_exact_on_small_integers(K, dt):
    """Integer codes and activations, power-of-two scales: every product and partial sum is exact in
    fp32, so the result is the float64 product rounded once to the dtype."""
    from fault_tolerant_llm_training_amd.utils import fp8

    dtype = DTYPES[dt]
    gen = torch.Generator(device="cuda").manual_seed(22)
    for N in NS:
        for Kd in KS:
            x = _ints((Kd,), -4, 4, gen).to(dtype)
            codes = fp8.e4m3_rne(_ints((N, Kd), -4, 4, gen).float())
            scale = torch.ldexp(torch.ones(N, device="cuda"), torch.arange(N, device="cuda") % 5 - 2)
            res = _ints((N,), -64, 64, gen).to(dtype)
            ref = torch.mv(fp8.dequant(codes, scale), x.double())
            y = K.gemv_w8(x, codes, scale, None)
            assert y.dtype == dtype and y.shape == (N,)
            assert torch.equal(y, ref.to(dtype)), (N, Kd)
            assert torch.equal(K.gemv_w8(x, codes, scale, res), (ref + res.double()).to(dtype)), (N, Kd)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_gemv_w8_random_operands_within_one_rounding_plus_fp32_accumulation(K, dt):
    """The bound of the 16-bit gemv test plus one fp32 rounding for the scale multiply."""
    dtype = DTYPES[dt]
    gen = torch.Generator(device="cuda").manual_seed(23)
    for N in NS:
        for Kd in KS:
            x, codes, scale, res, W = _operands(N, Kd, dtype, gen)
            for r in (None, res):
                ref, mag = torch.mv(W, x.double()), torch.mv(W.abs(), x.double().abs())
                if r is not None:
                    ref, mag = ref + r.double(), mag + r.double().abs()
                y = K.gemv_w8(x, codes, scale, r)
                bound = 0.5 * ulp_at(ref, dtype) + (Kd + 1) * 2.0 ** -23 * mag
                worst = float(((y.double() - ref).abs() / bound).max())
                print(f"gemv_w8 {dt} N={N} K={Kd} residual={r is not None}: max err / bound = {worst:.3f}")
                assert worst <= 1.0, (N, Kd)
                assert torch.equal(K.gemv_w8(x, codes, scale, r), y)


@pytest.mark.parametrize("Kd", [16, 4096])
@pytest.mark.parametrize("H", [1, 5, 256])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_gemv_swiglu_w8_equals_the_composed_ops_bit_for_bit(K, dt, H, Kd):
    from fault_tolerant_llm_training_amd.ops.functional import swiglu_reference

    x, codes, scale, _, _ = _operands(2 * H, Kd, DTYPES[dt], torch.Generator(device="cuda").manual_seed(24))
    scale = scale * 2  # pre-activations of order 2, where silu is not linear
    a = K.gemv_swiglu_w8(x, codes, scale)
    assert a.shape == (H,) and torch.equal(a, swiglu_reference(K.gemv_w8(x, codes, scale, None)))


@pytest.mark.parametrize("Kd", [1040, 4096, 5136, 8208])
@pytest.mark.parametrize("R", [1, 2, 3, 8, 9, 17])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_rows_forms_return_the_one_row_bits(K, dt, R, Kd):
    """K = 5136 and 8208 take the staged kernels (R > 1) through a second and a third chunk of
    activations in LDS: a tail in a later chunk, and two full sweeps plus one."""
    dtype, N = DTYPES[dt], 257
    gen = torch.Generator(device="cuda").manual_seed(25)
    _, codes, scale, _, _ = _operands(N, Kd, dtype, gen)
    x = torch.randn(R, Kd, generator=gen, device="cuda").to(dtype)
    res = torch.randn(R, N, generator=gen, device="cuda").to(dtype)
    y, yr = K.gemv_rows_w8(x, codes, scale, None), K.gemv_rows_w8(x, codes, scale, res)
    a = K.gemv_swiglu_rows_w8(x, codes[:256], scale[:256])
    assert y.shape == (R, N) and a.shape == (R, 128)
    for r in range(R):
        assert torch.equal(y[r], K.gemv_w8(x[r], codes, scale, None)), r
        assert torch.equal(yr[r], K.gemv_w8(x[r], codes, scale, res[r])), r
        assert torch.equal(a[r], K.gemv_swiglu_w8(x[r], codes[:256], scale[:256])), r


# ------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def tiny():
    from fault_tolerant_llm_training_amd.generation import Fp8Weights
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    margs = model_args_for("tiny", vocab_size=512, seq_len=64)
    model = build_model(margs, "cuda", torch.bfloat16, seed=3)
    return margs, model, Fp8Weights(model)


def test_fp8_decode_logits_are_as_close_to_float64_as_the_bf16_decode(tiny):
    """A 9-token prompt, then 8 teacher-forced decode steps. e_fp8: the logits with ``weights`` against
    a float64 CPU decode whose five products use dequant(codes, scale); e_bf16: the logits without
    ``weights`` against the float64 decode of the model's own weights. Both GPU paths round the same
    activations to bf16 and accumulate in fp32, so e_fp8 <= 1.5 e_bf16."""
    from fault_tolerant_llm_training_amd.generation import KVCache, decode_step, prefill
    from fault_tolerant_llm_training_amd.models.llama import build_model
    from fault_tolerant_llm_training_amd.utils import fp8

    margs, model, w8 = tiny
    tokens = torch.randint(0, 512, (17,), generator=torch.Generator().manual_seed(9))
    ref, refq = (build_model(margs, "cpu", torch.float64, seed=3) for _ in range(2))
    with torch.no_grad():
        for m in (ref, refq):
            m.flat.params.copy_(model.flat.params.double().cpu())
        for layer, qs in zip(refq.layers.values(), w8.layers):
            at, ff = layer.attention, layer.feed_forward
            for dst, (c, s) in zip((at.wqkv, at.wo.weight, ff.w13, ff.w2.weight), qs):
                dst.copy_(fp8.dequant(c.cpu(), s.cpu()))
        refq.output.weight.copy_(fp8.dequant(w8.head[0].cpu(), w8.head[1].cpu()))

    def run(pre, dec, dtype, device, weights=None):
        cache = KVCache(margs, 17, device, dtype)
        prefill(pre, tokens[:9], cache)
        return torch.stack([decode_step(dec, int(t), cache, weights) for t in tokens[9:]]).cpu()

    got = run(model, model, torch.bfloat16, "cuda", w8)
    e_fp8 = rel(got, run(ref, refq, torch.float64, "cpu"))
    e_bf16 = rel(run(model, model, torch.bfloat16, "cuda"), run(ref, ref, torch.float64, "cpu"))
    print(f"tiny: e_fp8 {e_fp8:.3e} e_bf16 {e_bf16:.3e} ratio {e_fp8 / e_bf16:.3f}")
    assert e_fp8 <= 1.5 * e_bf16
    assert torch.equal(run(model, model, torch.bfloat16, "cuda", w8), got)


PROMPTS = [[1, 5, 9, 200, 3, 77, 410, 8, 2], [7, 7, 300], [511, 0, 42, 42, 19]]


def test_generate_with_fp8_weights_batch_graph_and_default(tiny):
    from fault_tolerant_llm_training_amd.generation import (BatchKVCache, DecodeGraph, decode_step_rows, generate,
                                                            generate_batch, prefill)
    from fault_tolerant_llm_training_amd.ops import decode as D

    margs, model, w8 = tiny
    one = [generate(model, p, 8, weights=w8) for p in PROMPTS]
    assert generate_batch(model, PROMPTS, 8, weights=w8) == one
    assert generate_batch(model, PROMPTS, 8, weights=w8, graph=True) == one
    assert [generate(model, p, 8, weights=w8, graph=True) for p in PROMPTS] == one
    # the graph's logits after every replay are the eager loop's
    g = DecodeGraph(model, 3, 17, w8)
    g.begin(PROMPTS, 8)
    cache = BatchKVCache(margs, 3, 17, "cuda", torch.bfloat16)
    logits = torch.stack([prefill(model, p, cache.row(b)) for b, p in enumerate(PROMPTS)])
    for t in range(7):
        g.replay()
        logits = decode_step_rows(model, D.sample(logits, 0.0, 0, 0, 0), cache, t, w8)
        assert torch.equal(g.logits, logits), t
    # weights=None is the path without the argument
    assert [generate(model, p, 8, weights=None) for p in PROMPTS] == [generate(model, p, 8) for p in PROMPTS]
    assert generate(model, PROMPTS[0], 8, weights=None, graph=True) == generate(model, PROMPTS[0], 8, graph=True)
