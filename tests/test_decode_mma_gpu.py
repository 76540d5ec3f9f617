"""Matrix-core batched decode on the GPU (csrc/kernels/decode_mma.hip): the four skinny GEMM ops against
float64, their batch invariance, and generation with ``mma=True``."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
MANT = {torch.bfloat16: 7, torch.float16: 10}
EMIN = {torch.bfloat16: -126, torch.float16: -14}
RS = [1, 5, 16, 17, 33, 64]  # one row, a partial column tile, one tile, one more, into the third, the cap
NS = [5, 80, 257]            # less than a fragment, past one workgroup tile of 64, a ragged last tile
# K: less than one MFMA step; 9 chunks of 128, the smallest K whose split engages with unequal slices (4 + 5;
# 16-bit weights only, codes need K % 16); a partial step after whole ones; whole chunks; a tail after them
KS = [16, 1032, 1040, 4096, 5136]


@pytest.fixture(scope="module")
def D():
    from fault_tolerant_llm_training_amd._native import kernels
    from fault_tolerant_llm_training_amd.ops import decode

    kernels()
    return decode


def plain(D, x, w, res=None):
    return D.gemm_rows_mma(x, w, res) if torch.is_tensor(w) else D.gemm_rows_mma_w8(x, w[0], w[1], res)


def fused(D, x, w):
    return D.gemm_swiglu_rows_mma(x, w) if torch.is_tensor(w) else D.gemm_swiglu_rows_mma_w8(x, w[0], w[1])


def head(w, n):
    """The first n rows of a weight (a tensor, or a (codes, scale) pair)."""
    return w[:n] if torch.is_tensor(w) else (w[0][:n], w[1][:n])


def ulp_at(ref, dtype):
    _, e = torch.frexp(ref.abs().clamp(min=2.0 ** -300))
    return torch.ldexp(torch.ones_like(ref), (e - 1).clamp(min=EMIN[dtype]) - MANT[dtype])


def rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def random_weight(rows, Kd, dtype, gen, w8, gain=1.0):
    """A random weight [rows, K] for the ops (w8: the definition's codes and scale) and its float64 values."""
    from fault_tolerant_llm_training_amd.utils import fp8

    w = (gain * torch.randn(rows, Kd, generator=gen, device="cuda") / math.sqrt(Kd)).to(dtype)
    if not w8:
        return w, w.double()
    codes, scale = (t.cuda() for t in fp8.quantize_rows(w.cpu()))
    return (codes, scale), fp8.dequant(codes, scale)


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("w8", [False, True], ids=["w16", "w8"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_exact_on_small_integers(D, dt, w8, R):
    """Integers in [-4, 4], power-of-two scales, an integer residual: every product and partial sum is exact
    in fp32, so each op returns the float64 product rounded once (SwiGLU: the composed ops on that)."""
    from fault_tolerant_llm_training_amd.ops.functional import swiglu_reference
    from fault_tolerant_llm_training_amd.utils import fp8

    dtype = DTYPES[dt]
    gen = torch.Generator(device="cuda").manual_seed(31)
    for N in NS:
        for Kd in KS:
            if w8 and Kd % 16:
                continue
            x = torch.randint(-4, 5, (R, Kd), generator=gen, device="cuda").to(dtype)
            wi = torch.randint(-4, 5, (2 * N, Kd), generator=gen, device="cuda")
            scale = torch.ldexp(torch.ones(2 * N, device="cuda"), torch.arange(2 * N, device="cuda") % 5 - 2)
            res = torch.randint(-64, 65, (R, N), generator=gen, device="cuda").to(dtype)
            w = (fp8.e4m3_rne(wi.float()), scale) if w8 else wi.to(dtype)
            ref = x.double() @ (wi.double() * (scale.double()[:, None] if w8 else 1.0)).T
            y = plain(D, x, head(w, N))
            assert y.dtype == dtype and y.shape == (R, N)
            assert torch.equal(y, ref[:, :N].to(dtype)), (N, Kd)
            assert torch.equal(plain(D, x, head(w, N), res), (ref[:, :N] + res.double()).to(dtype)), (N, Kd)
            assert torch.equal(fused(D, x, w), swiglu_reference(ref.to(dtype))), (N, Kd)


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("w8", [False, True], ids=["w16", "w8"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_random_operands_within_one_rounding_plus_fp32_accumulation(D, dt, w8, R):
    """|y - ref| <= 0.5 ulp(ref) + (K + 1) 2^-23 (|W| |x| + |res|): 16-bit products are exact in fp32 and
    2^-23 per accumulation covers any order, truncation included; + 1 for the scale multiply of the w8 forms."""
    dtype = DTYPES[dt]
    gen = torch.Generator(device="cuda").manual_seed(32)
    for N in NS:
        for Kd in KS:
            if w8 and Kd % 16:
                continue
            w, W = random_weight(N, Kd, dtype, gen, w8)
            x = torch.randn(R, Kd, generator=gen, device="cuda").to(dtype)
            res = torch.randn(R, N, generator=gen, device="cuda").to(dtype)
            for r in (None, res):
                ref, mag = x.double() @ W.T, x.double().abs() @ W.abs().T
                if r is not None:
                    ref, mag = ref + r.double(), mag + r.double().abs()
                y = plain(D, x, w, r)
                bound = 0.5 * ulp_at(ref, dtype) + (Kd + 1) * 2.0 ** -23 * mag
                worst = float(((y.double() - ref).abs() / bound).max())
                print(f"gemm_rows_mma{'_w8' if w8 else ''} {dt} R={R} N={N} K={Kd} residual={r is not None}: "
                      f"max err / bound = {worst:.3f}")
                assert worst <= 1.0, (N, Kd)


@pytest.mark.parametrize("Kd", [1040, 5136])
@pytest.mark.parametrize("R", [2, 17, 64])
@pytest.mark.parametrize("w8", [False, True], ids=["w16", "w8"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_batch_invariance_bitwise(D, dt, w8, R, Kd):
    """Row r of the R-row call has the bits of the one-row call on x[r]; a permuted batch gives the permuted
    rows; two calls give equal bits. All four ops (N = 257, H = 128)."""
    dtype, N = DTYPES[dt], 257
    gen = torch.Generator(device="cuda").manual_seed(33)
    w, _ = random_weight(N, Kd, dtype, gen, w8, gain=2.0)
    x = torch.randn(R, Kd, generator=gen, device="cuda").to(dtype)
    res = torch.randn(R, N, generator=gen, device="cuda").to(dtype)
    perm = torch.randperm(R, generator=gen, device="cuda")
    y, yr, a = plain(D, x, w), plain(D, x, w, res), fused(D, x, head(w, 256))
    assert torch.equal(plain(D, x, w), y) and torch.equal(plain(D, x, w, res), yr)
    assert torch.equal(fused(D, x, head(w, 256)), a)
    xp = x[perm].contiguous()
    assert torch.equal(plain(D, xp, w), y[perm]) and torch.equal(plain(D, xp, w, res[perm].contiguous()), yr[perm])
    assert torch.equal(fused(D, xp, head(w, 256)), a[perm])
    for r in range(R):
        x1 = x[r : r + 1].clone()  # its own allocation: a row view of x need not be 16-byte aligned
        assert torch.equal(plain(D, x1, w)[0], y[r]), r
        assert torch.equal(plain(D, x1, w, res[r : r + 1].clone())[0], yr[r]), r
        assert torch.equal(fused(D, x1, head(w, 256))[0], a[r]), r


@pytest.mark.parametrize("Kd", [16, 4096])
@pytest.mark.parametrize("H", [1, 5, 256])
@pytest.mark.parametrize("w8", [False, True], ids=["w16", "w8"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_swiglu_forms_equal_the_composed_ops_bit_for_bit(D, dt, w8, H, Kd):
    from fault_tolerant_llm_training_amd.ops.functional import swiglu_reference

    gen = torch.Generator(device="cuda").manual_seed(34)
    w, _ = random_weight(2 * H, Kd, DTYPES[dt], gen, w8, gain=2.0)  # pre-activations of order 2: silu not linear
    for R in (5, 33):
        x = torch.randn(R, Kd, generator=gen, device="cuda").to(DTYPES[dt])
        a = fused(D, x, w)
        assert a.shape == (R, H) and torch.equal(a, swiglu_reference(plain(D, x, w)))


def test_fp32_on_the_gpu_is_refused(D):
    x, w = torch.zeros(2, 16, device="cuda"), torch.zeros(8, 16, device="cuda")
    with pytest.raises(ValueError, match="bf16 or fp16"):
        D.gemm_rows_mma(x, w)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        D.gemm_rows_mma(x.bfloat16()[:, :12].contiguous(), w.bfloat16()[:, :12].contiguous())
    with pytest.raises(RuntimeError, match="1 <= R <= 64"):
        D.gemm_rows_mma(torch.zeros(65, 16, device="cuda").bfloat16(), w.bfloat16())


# ------------------------------------------------------------------------------- model level
PROMPTS = [[1, 5, 9, 200, 3, 77, 410, 8, 2], [7, 7, 300], [511, 0, 42, 42, 19]]


@pytest.fixture(scope="module")
def tiny():
    from fault_tolerant_llm_training_amd.generation import Fp8Weights
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    margs = model_args_for("tiny", vocab_size=512, seq_len=64)
    model = build_model(margs, "cuda", torch.bfloat16, seed=3)
    return margs, model, Fp8Weights(model)


@pytest.mark.parametrize("fp8w", [False, True], ids=["w16", "w8"])
def test_generate_batch_mma_graph_and_batch_invariance(tiny, fp8w):
    from fault_tolerant_llm_training_amd.generation import (BatchKVCache, DecodeGraph, decode_step_rows,
                                                            generate_batch, prefill)
    from fault_tolerant_llm_training_amd.ops import decode as D

    margs, model, w8 = tiny
    w = w8 if fp8w else None
    rows = generate_batch(model, PROMPTS, 8, weights=w, mma=True)
    assert generate_batch(model, PROMPTS, 8, weights=w, mma=True, graph=True) == rows
    assert [generate_batch(model, [p], 8, weights=w, mma=True)[0] for p in PROMPTS] == rows
    # the graph's logits after every replay are the eager loop's
    g = DecodeGraph(model, 3, 17, w, mma=True)
    g.begin(PROMPTS, 8)
    cache = BatchKVCache(margs, 3, 17, "cuda", torch.bfloat16)
    logits = torch.stack([prefill(model, p, cache.row(b)) for b, p in enumerate(PROMPTS)])
    for t in range(7):
        g.replay()
        logits = decode_step_rows(model, D.sample(logits, 0.0, 0, 0, 0), cache, t, w, mma=True)
        assert torch.equal(g.logits, logits), t


def test_mma_logits_are_as_close_to_float64_as_the_default_decode(tiny):
    """A 9-token prompt, then 8 teacher-forced decode steps against a float64 CPU decode: both GPU paths
    round the same activations to bf16 and accumulate in fp32, so e_mma <= 1.5 e_default."""
    from fault_tolerant_llm_training_amd.generation import BatchKVCache, KVCache, decode_step, decode_step_rows, prefill
    from fault_tolerant_llm_training_amd.models.llama import build_model

    margs, model, _ = tiny
    tokens = torch.randint(0, 512, (17,), generator=torch.Generator().manual_seed(9))
    ref = build_model(margs, "cpu", torch.float64, seed=3)
    with torch.no_grad():
        ref.flat.params.copy_(model.flat.params.double().cpu())
    cache = KVCache(margs, 17, "cpu", torch.float64)
    prefill(ref, tokens[:9], cache)
    want = torch.stack([decode_step(ref, int(t), cache) for t in tokens[9:]])

    def run(mma):
        cache = BatchKVCache(margs, 1, 17, "cuda", torch.bfloat16)
        prefill(model, tokens[:9], cache.row(0))
        return torch.cat([decode_step_rows(model, [int(t)], cache, i, mma=mma) for i, t in enumerate(tokens[9:])]).cpu()

    e_mma, e_def = rel(run(True), want), rel(run(False), want)
    print(f"tiny: e_mma {e_mma:.3e} e_default {e_def:.3e} ratio {e_mma / e_def:.3f}")
    assert e_mma <= 1.5 * e_def
