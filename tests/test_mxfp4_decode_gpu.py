"""Weight-only MXFP4 decode on the GPU (csrc/kernels/decode_mx4.hip): the quantizer against its
definition (utils/mxfp4.py), the gemv kernels against float64, and generation with ``Mxfp4Weights``."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
MANT = {torch.bfloat16: 7, torch.float16: 10}
EMIN = {torch.bfloat16: -126, torch.float16: -14}
# A lane takes 128 elements, 32 lanes a row: a chunk is 4096. K: one block; part of a chunk with whole
# units (scale dwords) and with a partial unit (scale bytes); one chunk; a chunk and one unit
NS, KS = [1, 5, 257], [32, 1152, 2080, 4096, 4224]


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


def _operands(N, Kd, dtype, gen, gain=1.0):
    """Random x, the definition's codes and scales of a random weight, a residual, and float64 W."""
    from fault_tolerant_llm_training_amd.utils import mxfp4

    x = torch.randn(Kd, generator=gen, device="cuda").to(dtype)
    w = (gain * torch.randn(N, Kd, generator=gen, device="cuda") / math.sqrt(Kd)).to(dtype)
    codes, scales = (t.cuda() for t in mxfp4.quantize_rows(w.cpu()))
    return x, codes, scales, torch.randn(N, generator=gen, device="cuda").to(dtype), mxfp4.dequant(codes, scales)


@pytest.mark.parametrize("Kd", [32, 2080, 4096])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_quantizer_equals_the_definition_bit_for_bit(K, dt, N, Kd):
    from fault_tolerant_llm_training_amd.utils import mxfp4

    dtype = DTYPES[dt]
    gen = torch.Generator().manual_seed(21)
    w = (0.02 * torch.randn(N, Kd, generator=gen)).to(dtype)
    if N >= 5:
        w[1] = 0.0
        w[1, Kd // 2] = -0.0
        w[2, 3] = 4096 * w[2].abs().max()  # the rest of its block: zero codes
        ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
        row = (torch.cat([torch.tensor([6.0]), ties, -ties, torch.zeros(17)]) / 8).repeat(Kd // 32)
        w[3] = row.to(dtype)  # amax = 6 * 2^-3 exactly: w / 2^-3 are the ties themselves
        assert torch.equal(w[3].float(), row)
    want_c, want_s = mxfp4.quantize_rows(w)
    codes, scales = K.quantize_rows_mxfp4(w.cuda())
    assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8
    bad = (codes.cpu() != want_c).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), codes.cpu()[tuple(bad[0])], want_c[tuple(bad[0])])
    assert torch.equal(scales.cpu(), want_s)
    again = K.quantize_rows_mxfp4(w.cuda())
    assert torch.equal(again[0], codes) and torch.equal(again[1], scales)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_gemv_mx4_is_exact_on_small_integers(K, dt):
    """Every product and partial sum is exact in fp32: the float64 product rounded once. The random codes are not
    symmetric in a byte's nibbles, so a swapped nibble or byte order would not survive."""
    from fault_tolerant_llm_training_amd.utils import mxfp4

    dtype = DTYPES[dt]
    gen = torch.Generator(device="cuda").manual_seed(22)
    whole = torch.tensor([0, 2, 4, 5, 6, 7], device="cuda")  # the codes of 0, 1, 2, 3, 4, 6
    for N in NS:
        for Kd in KS:
            x = _ints((Kd,), -4, 4, gen).to(dtype)
            c = whole[_ints((N, Kd // 2, 2), 0, 5, gen)] + 8 * _ints((N, Kd // 2, 2), 0, 1, gen)
            codes = (c[:, :, 0] | (c[:, :, 1] << 4)).to(torch.uint8)
            scales = (127 + (torch.arange(N * (Kd // 32), device="cuda") % 5 - 2)).to(torch.uint8).view(N, -1)
            res = _ints((N,), -64, 64, gen).to(dtype)
            ref = torch.mv(mxfp4.dequant(codes, scales), x.double())
            y = K.gemv_mx4(x, codes, scales, None)
            assert y.dtype == dtype and y.shape == (N,)
            assert torch.equal(y, ref.to(dtype)), (N, Kd)
            assert torch.equal(K.gemv_mx4(x, codes, scales, res), (ref + res.double()).to(dtype)), (N, Kd)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_gemv_mx4_random_operands_within_one_rounding_plus_fp32_accumulation(K, dt):
    """The bound of the FP8 test: one rounding to the dtype and one fp32 rounding per accumulation step."""
    dtype = DTYPES[dt]
    gen = torch.Generator(device="cuda").manual_seed(23)
    for N in NS:
        for Kd in KS:
            x, codes, scales, res, W = _operands(N, Kd, dtype, gen)
            for r in (None, res):
                ref, mag = torch.mv(W, x.double()), torch.mv(W.abs(), x.double().abs())
                if r is not None:
                    ref, mag = ref + r.double(), mag + r.double().abs()
                y = K.gemv_mx4(x, codes, scales, r)
                bound = 0.5 * ulp_at(ref, dtype) + (Kd + 1) * 2.0 ** -23 * mag
                worst = float(((y.double() - ref).abs() / bound).max())
                print(f"gemv_mx4 {dt} N={N} K={Kd} residual={r is not None}: max err / bound = {worst:.3f}")
                assert worst <= 1.0, (N, Kd)
                assert torch.equal(K.gemv_mx4(x, codes, scales, r), y)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_a_0xff_scale_byte_poisons_its_row_and_no_other(K, dt):
    x, codes, scales, _, _ = _operands(5, 4224, DTYPES[dt], torch.Generator(device="cuda").manual_seed(26))
    clean = K.gemv_mx4(x, codes, scales, None)
    scales[1, 130] = scales[3, 0] = 255
    y = K.gemv_mx4(x, codes, scales, None)
    assert torch.isnan(y).tolist() == [False, True, False, True, False] and torch.equal(y[[0, 2, 4]], clean[[0, 2, 4]])


@pytest.mark.parametrize("Kd", [32, 4096])
@pytest.mark.parametrize("H", [1, 5, 256])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_gemv_swiglu_mx4_equals_the_composed_ops_bit_for_bit(K, dt, H, Kd):
    from fault_tolerant_llm_training_amd.ops.functional import swiglu_reference

    # gain 2: pre-activations of order 2, where silu is not linear
    x, codes, scales, _, _ = _operands(2 * H, Kd, DTYPES[dt], torch.Generator(device="cuda").manual_seed(24), gain=2.0)
    a = K.gemv_swiglu_mx4(x, codes, scales)
    assert a.shape == (H,) and torch.equal(a, swiglu_reference(K.gemv_mx4(x, codes, scales, None)))


@pytest.mark.parametrize("Kd", [2080, 4096, 4224, 8224, 8320])
@pytest.mark.parametrize("R", [1, 2, 3, 8, 9, 17])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_rows_forms_return_the_one_row_bits(K, dt, R, Kd):
    """K = 4224 reaches a second staged chunk of activations; 8224 (scale bytes) and 8320 (scale dwords) a third."""
    dtype, N = DTYPES[dt], 257
    gen = torch.Generator(device="cuda").manual_seed(25)
    _, codes, scales, _, _ = _operands(N, Kd, dtype, gen)
    x = torch.randn(R, Kd, generator=gen, device="cuda").to(dtype)
    res = torch.randn(R, N, generator=gen, device="cuda").to(dtype)
    y, yr = K.gemv_rows_mx4(x, codes, scales, None), K.gemv_rows_mx4(x, codes, scales, res)
    a = K.gemv_swiglu_rows_mx4(x, codes[:256], scales[:256])
    assert y.shape == (R, N) and a.shape == (R, 128)
    for r in range(R):
        assert torch.equal(y[r], K.gemv_mx4(x[r], codes, scales, None)), r
        assert torch.equal(yr[r], K.gemv_mx4(x[r], codes, scales, res[r])), r
        assert torch.equal(a[r], K.gemv_swiglu_mx4(x[r], codes[:256], scales[:256])), r


def test_host_checks_refuse_what_the_kernels_cannot_take(K):
    x, codes, scales, _, _ = _operands(5, 64, torch.bfloat16, torch.Generator(device="cuda").manual_seed(27))
    c32, s32 = codes[:, :16].contiguous(), scales[:, :1].contiguous()  # the K = 32 weight
    assert K.gemv_mx4(x[:32], c32, s32, None).shape == (5,)
    # dtype; not contiguous; K = 48; scales' dtype and shape; x is not [K]; x 8 bytes off a 16-byte boundary
    for bad in ((x.float(), codes, scales), (x, codes.t().contiguous().t(), scales),
                (x, codes[:, :24].contiguous(), scales), (x, codes, scales.int()), (x, codes, s32),
                (x[:32], codes, scales), (x[4:36], c32, s32)):
        with pytest.raises(RuntimeError):
            K.gemv_mx4(*bad, None)
    with pytest.raises(RuntimeError):
        K.quantize_rows_mxfp4(torch.zeros(4, 48, device="cuda", dtype=torch.bfloat16))


# ------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def tiny():
    from fault_tolerant_llm_training_amd.generation import Mxfp4Weights
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    margs = model_args_for("tiny", vocab_size=512, seq_len=64)
    model = build_model(margs, "cuda", torch.bfloat16, seed=3)
    return margs, model, Mxfp4Weights(model)


def test_mxfp4_decode_logits_are_as_close_to_float64_as_the_bf16_decode(tiny):
    """The construction and the factor of the FP8 test: 9 prompt tokens, 8 teacher-forced steps; the MXFP4 logits
    against a float64 decode of dequant(codes, scales), the bf16 logits against float64 of the model's weights."""
    from fault_tolerant_llm_training_amd.generation import KVCache, decode_step, prefill
    from fault_tolerant_llm_training_amd.models.llama import build_model
    from fault_tolerant_llm_training_amd.utils import mxfp4

    margs, model, w4 = tiny
    tokens = torch.randint(0, 512, (17,), generator=torch.Generator().manual_seed(9))
    ref, refq = (build_model(margs, "cpu", torch.float64, seed=3) for _ in range(2))
    with torch.no_grad():
        for m in (ref, refq):
            m.flat.params.copy_(model.flat.params.double().cpu())
        for layer, qs in zip(refq.layers.values(), w4.layers):
            at, ff = layer.attention, layer.feed_forward
            for dst, (c, s) in zip((at.wqkv, at.wo.weight, ff.w13, ff.w2.weight), qs):
                dst.copy_(mxfp4.dequant(c.cpu(), s.cpu()))
        refq.output.weight.copy_(mxfp4.dequant(w4.head[0].cpu(), w4.head[1].cpu()))

    def run(pre, dec, dtype, device, weights=None):
        cache = KVCache(margs, 17, device, dtype)
        prefill(pre, tokens[:9], cache)
        return torch.stack([decode_step(dec, int(t), cache, weights) for t in tokens[9:]]).cpu()

    got = run(model, model, torch.bfloat16, "cuda", w4)
    e_mx4 = rel(got, run(ref, refq, torch.float64, "cpu"))
    e_bf16 = rel(run(model, model, torch.bfloat16, "cuda"), run(ref, ref, torch.float64, "cpu"))
    print(f"tiny: e_mx4 {e_mx4:.3e} e_bf16 {e_bf16:.3e} ratio {e_mx4 / e_bf16:.3f}")
    assert e_mx4 <= 1.5 * e_bf16
    assert torch.equal(run(model, model, torch.bfloat16, "cuda", w4), got)


PROMPTS = [[1, 5, 9, 200, 3, 77, 410, 8, 2], [7, 7, 300], [511, 0, 42, 42, 19]]


def test_generate_with_mxfp4_weights_batch_graph_and_default(tiny):
    from fault_tolerant_llm_training_amd.generation import (BatchKVCache, DecodeGraph, decode_step_rows, generate,
                                                            generate_batch, prefill)
    from fault_tolerant_llm_training_amd.ops import decode as D

    margs, model, w4 = tiny
    one = [generate(model, p, 8, weights=w4) for p in PROMPTS]
    assert generate_batch(model, PROMPTS, 8, weights=w4) == one
    assert generate_batch(model, PROMPTS, 8, weights=w4, graph=True) == one
    assert [generate(model, p, 8, weights=w4, graph=True) for p in PROMPTS] == one
    g = DecodeGraph(model, 3, 17, w4)
    g.begin(PROMPTS, 8)
    cache = BatchKVCache(margs, 3, 17, "cuda", torch.bfloat16)
    logits = torch.stack([prefill(model, p, cache.row(b)) for b, p in enumerate(PROMPTS)])
    for t in range(7):
        g.replay()
        logits = decode_step_rows(model, D.sample(logits, 0.0, 0, 0, 0), cache, t, w4)
        assert torch.equal(g.logits, logits), t
    with pytest.raises(ValueError):
        DecodeGraph(model, 3, 17, w4, mma=True)
    assert [generate(model, p, 8, weights=None) for p in PROMPTS] == [generate(model, p, 8) for p in PROMPTS]
    assert generate(model, PROMPTS[0], 8, weights=None, graph=True) == generate(model, PROMPTS[0], 8, graph=True)
