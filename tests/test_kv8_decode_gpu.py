"""FP8 KV cache on the GPU (csrc/kernels/decode_kv8.hip): the quantizing append and the prefill quantizer
bit for bit against the definition (utils/fp8.py) on what the model-dtype ops store, the attention
kernels against float64 on the dequantized cache, the rows / device-step forms against the one-row
ops, and generation with ``kv_dtype="fp8"``."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
SHAPES = [(4, 2, 64), (4, 1, 128)]


@pytest.fixture(scope="module")
def K():
    from fault_tolerant_llm_training_amd._native import kernels

    return kernels()


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-300)).item()


def quantized(rows):
    """The definition on head rows [..., D] (any device): codes [..., D], scale [...], on the GPU."""
    from fault_tolerant_llm_training_amd.utils import fp8

    c, s = fp8.quantize_rows(rows.reshape(-1, rows.shape[-1]).cpu())
    return c.view(rows.shape).cuda(), s.view(rows.shape[:-1]).cuda()


def same(codes, scale, want):
    return torch.equal(codes, want[0]) and torch.equal(scale.view(torch.int32), want[1].view(torch.int32))


def fp8_cache(shape, gen):
    """A cache of random head rows whose magnitudes spread over 2^10: (codes, scale) and its float64 values."""
    from fault_tolerant_llm_training_amd.utils import fp8

    rows = torch.randn(shape, generator=gen) * torch.exp2(10 * torch.rand(shape[:-1], generator=gen) - 5)[..., None]
    c, s = quantized(rows.bfloat16())
    return c, s, fp8.dequant(c.view(-1, shape[-1]).cpu(), s.view(-1).cpu()).view(shape)


def ref_attn(q, kd, vd, n):
    """float64 softmax attention of q [Hq D] over keys 0 .. n-1 of the float64 caches [Hkv, Smax, D]."""
    hkv, _, d = kd.shape
    hq = q.numel() // d
    k, v = (t[:, :n].repeat_interleave(hq // hkv, dim=0) for t in (kd, vd))
    s = torch.einsum("hd,hnd->hn", q.double().cpu().view(hq, d), k) / math.sqrt(d)
    return torch.einsum("hn,hnd->hd", torch.softmax(s, dim=-1), v).reshape(-1)


def empty_kv8(*lead, hkv, smax, d):
    """Caches filled with a pattern no append writes by accident (code 0x55, scale -3)."""
    return (torch.full((*lead, hkv, smax, d), 0x55, dtype=torch.uint8, device="cuda"),
            torch.full((*lead, hkv, smax, d), 0x55, dtype=torch.uint8, device="cuda"),
            torch.full((*lead, hkv, smax), -3.0, device="cuda"), torch.full((*lead, hkv, smax), -3.0, device="cuda"))


# ------------------------------------------------------------------------------- append, prefill
@pytest.mark.parametrize("hq,hkv,d", SHAPES)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_append_stores_the_definition_of_the_model_dtype_rows(K, hq, hkv, d, dt):
    from fault_tolerant_llm_training_amd.models.llama import rope_tables

    dtype, smax = DTYPES[dt], 24
    cos, sin = (t.cuda() for t in rope_tables(d, smax, 500000.0))
    gen = torch.Generator().manual_seed(31)
    k_at, v_at = hq * d, (hq + hkv) * d  # head 0 of K and of V inside qkv
    for pos in (0, smax - 1):
        for edge in ("none", "zeros", "largest", "nan"):
            qkv = torch.randn((hq + 2 * hkv) * d, generator=gen).to(dtype)
            for at in (k_at, v_at):
                if edge == "zeros":
                    qkv[at : at + d] = 0.0
                    qkv[at + 1 : at + d : 2] = -0.0
                elif edge == "largest":
                    qkv[at : at + d] = 0.0
                    qkv[at + 5] = torch.finfo(dtype).max
                elif edge == "nan":
                    qkv[at + 7] = float("nan")
            qa, qb = qkv.cuda(), qkv.cuda()
            km, vm = (torch.zeros(hkv, smax, d, dtype=dtype, device="cuda") for _ in range(2))
            kc, vc, ks, vs = empty_kv8(hkv=hkv, smax=smax, d=d)
            before = [t.clone() for t in (kc, vc, ks, vs)]
            K.decode_qkv_append_(qb, cos, sin, pos, km, vm)
            K.decode_qkv_append_kv8_(qa, cos, sin, pos, kc, vc, ks, vs)
            assert torch.equal(qa.view(torch.int16), qb.view(torch.int16)), (pos, edge)
            assert same(kc[:, pos], ks[:, pos], quantized(km[:, pos])), (pos, edge)
            assert same(vc[:, pos], vs[:, pos], quantized(vm[:, pos])), (pos, edge)
            if edge == "zeros":
                assert float(vs[0, pos]) == 1.0 and vc[0, pos].tolist() == [0x00, 0x80] * (d // 2)
            others = [i for i in range(smax) if i != pos]
            for t, t0 in zip((kc, vc, ks, vs), before):
                assert torch.equal(t[:, others], t0[:, others]), (pos, edge)
    for bad in (-1, smax):
        with pytest.raises(RuntimeError):
            K.decode_qkv_append_kv8_(qa, cos, sin, bad, kc, vc, ks, vs)


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("hq,hkv,d", SHAPES)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_prefill_quantizer_is_the_definition_on_the_transposed_rows(K, hq, hkv, d, dt, P):
    smax = 8
    gen = torch.Generator().manual_seed(32)
    w = hkv * d  # k and v as prefill passes them: column slices of a wider buffer
    buf = (torch.randn(P, 2 * w + 8, generator=gen) * 8.0).to(DTYPES[dt]).cuda()
    k, v = buf[:, 8 : 8 + w], buf[:, 8 + w :]
    kc, vc, ks, vs = empty_kv8(hkv=hkv, smax=smax, d=d)
    before = [t.clone() for t in (kc, vc, ks, vs)]
    K.kv_quantize_prefill_(k, v, kc, vc, ks, vs)
    assert same(kc[:, :P], ks[:, :P], quantized(k.view(P, hkv, d).transpose(0, 1)))
    assert same(vc[:, :P], vs[:, :P], quantized(v.view(P, hkv, d).transpose(0, 1)))
    for t, t0 in zip((kc, vc, ks, vs), before):
        assert torch.equal(t[:, P:], t0[:, P:])


# ------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("hq,hkv,d", SHAPES + [(16, 1, 64)])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_attention_against_float64_on_the_dequantized_cache(K, hq, hkv, d, dt):
    """The bound of test_generate_gpu.py::test_decode_attn: the codes decode exactly, and what follows is
    the same fp32 arithmetic and the same output rounding."""
    C = int(K.decode_attn_chunk())
    smax = 2 * C + 8
    gen = torch.Generator().manual_seed(33)
    kc, ks, kd = fp8_cache((hkv, smax, d), gen)
    vc, vs, vd = fp8_cache((hkv, smax, d), gen)
    for n in (1, C - 1, C, C + 1, 2 * C + 3):
        q = torch.randn(hq * d, generator=gen).to(DTYPES[dt]).cuda()
        o = K.decode_attn_kv8(q, kc, vc, ks, vs, n)
        e = rel(o.cpu(), ref_attn(q, kd, vd, n))
        print(f"decode_attn_kv8 {dt} Hq={hq} Hkv={hkv} D={d} n_keys={n}: rel {e:.2e}")
        assert e < 1e-2, n
        assert torch.equal(K.decode_attn_kv8(q, kc, vc, ks, vs, n), o)
        kn, vn, ksn, vsn = kc.clone(), vc.clone(), ks.clone(), vs.clone()
        kn[:, n:], vn[:, n:], ksn[:, n:], vsn[:, n:] = 0x7F, 0x7F, float("nan"), float("nan")
        assert torch.equal(K.decode_attn_kv8(q, kn, vn, ksn, vsn, n), o)  # nothing at or beyond n_keys is read
    for bad in (0, smax + 1):
        with pytest.raises(RuntimeError):
            K.decode_attn_kv8(q, kc, vc, ks, vs, bad)


@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("hq,hkv,d", SHAPES)
def test_rows_and_device_step_forms_return_the_one_row_bits(K, hq, hkv, d, t):
    from fault_tolerant_llm_training_amd.models.llama import rope_tables
    from fault_tolerant_llm_training_amd.ops import decode as D

    C = int(K.decode_attn_chunk())
    B, smax, lengths = 3, C + 4, [0, C - 1, C + 2]
    pos0 = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    cos, sin = (x.cuda() for x in rope_tables(d, smax, 500000.0))
    gen = torch.Generator().manual_seed(34)
    qkv = torch.randn(B, (hq + 2 * hkv) * d, generator=gen).bfloat16().cuda()
    kc, ks, _ = fp8_cache((B, hkv, smax, d), gen)
    vc, vs, _ = fp8_cache((B, hkv, smax, d), gen)
    ctl = D.new_ctl("cuda")
    D.write_ctl(ctl, t, 0.0, 0, 0, 0)
    # append: one row at a time, all rows, all rows with t from the control block
    one, rows, dev = ([x.clone() for x in (qkv, kc, vc, ks, vs)] for _ in range(3))
    for b in range(B):
        K.decode_qkv_append_kv8_(one[0][b], cos, sin, lengths[b] + t, *(x[b] for x in one[1:]))
    K.decode_qkv_append_rows_kv8_(rows[0], cos, sin, pos0, t, max(lengths) + t, *rows[1:])
    K.decode_qkv_append_rows_dev_kv8_(dev[0], cos, sin, pos0, ctl, *dev[1:])
    for a, b, c in zip(one, rows, dev):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and torch.equal(a.view(torch.uint8),
                                                                                      c.view(torch.uint8))
    # attention over the appended caches; q is the column slice of qkv, as in a decode pass
    q, cache = rows[0][:, : hq * d], rows[1:]
    o = K.decode_attn_rows_kv8(q, *cache, pos0, t, max(lengths) + t + 1)
    for b in range(B):
        assert torch.equal(o[b], K.decode_attn_kv8(q[b].contiguous(), *(x[b] for x in cache), lengths[b] + t + 1)), b
    part, od = D.attn_part(B, hq, smax, d, "cuda"), torch.empty_like(o)
    K.decode_attn_rows_dev_kv8(q, *cache, pos0, ctl, part, od)
    assert torch.equal(od, o)
    # a position beyond the capacity writes nothing (and leaves the row's Q unrotated)
    far = torch.tensor([0, smax - t, 5], dtype=torch.int32, device="cuda")
    skip = [x.clone() for x in (qkv, kc, vc, ks, vs)]
    K.decode_qkv_append_rows_dev_kv8_(skip[0], cos, sin, far, ctl, *skip[1:])
    for x, x0 in zip(skip, (qkv, kc, vc, ks, vs)):
        assert torch.equal(x[1].view(torch.uint8), x0[1].view(torch.uint8))
    assert not torch.equal(skip[1][2], kc[2])


# ------------------------------------------------------------------------------- model level
PROMPTS = [[1, 5, 9, 200, 3, 77, 410, 8, 2], [7, 7, 300], [511, 0, 42, 42, 19], [7, 7, 300]]


@pytest.fixture(scope="module")
def tiny():
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    margs = model_args_for("tiny", vocab_size=512, seq_len=64)
    return margs, build_model(margs, "cuda", torch.bfloat16, seed=3)


def test_generate_with_an_fp8_cache_batch_graph_weights_and_mma(tiny):
    from fault_tolerant_llm_training_amd.generation import (BatchKVCache, DecodeGraph, Fp8Weights, decode_step_rows,
                                                            generate, generate_batch, prefill)
    from fault_tolerant_llm_training_amd.models.llama import build_model
    from fault_tolerant_llm_training_amd.ops import decode as D

    margs, model = tiny
    one = [generate(model, p, 8, kv_dtype="fp8") for p in PROMPTS]
    assert generate_batch(model, PROMPTS, 8, kv_dtype="fp8") == one
    assert generate_batch(model, PROMPTS, 8, kv_dtype="fp8", graph=True) == one
    assert generate(model, PROMPTS[0], 8, kv_dtype="fp8", graph=True) == one[0]
    # the graph's logits after every replay are the eager loop's
    g = DecodeGraph(model, 4, 17, kv_dtype="fp8")
    g.begin(PROMPTS, 8)
    cache = BatchKVCache(margs, 4, 17, "cuda", torch.bfloat16, kv_dtype="fp8")
    logits = torch.stack([prefill(model, p, cache.row(b)) for b, p in enumerate(PROMPTS)])
    for t in range(7):
        g.replay()
        logits = decode_step_rows(model, D.sample(logits, 0.0, 0, 0, 0), cache, t)
        assert torch.equal(g.logits, logits), t
    w8 = Fp8Weights(model)
    for kw in ({"weights": w8}, {"mma": True}, {"weights": w8, "mma": True, "graph": True}):
        ids = generate_batch(model, PROMPTS, 8, kv_dtype="fp8", **kw)
        assert [len(r) for r in ids] == [8] * 4 and generate_batch(model, PROMPTS, 8, kv_dtype="fp8", **kw) == ids
    assert generate(model, PROMPTS[0], 8, kv_dtype="model") == generate(model, PROMPTS[0], 8)
    with pytest.raises(ValueError):
        generate(build_model(margs, "cuda", torch.float32, seed=3), PROMPTS[0], 2, kv_dtype="fp8")


def test_fp8_cache_logits_are_as_close_to_float64_as_the_bf16_cache(tiny):
    """The form and margin of test_fp8_decode_gpu.py's closeness test: a 9-token prompt, then 8
    teacher-forced decode steps. e_kv8: the logits with ``kv_dtype="fp8"`` against a float64 CPU run of
    the same definition; e_bf16: the logits of the bf16 cache against a float64 run with a float64
    cache. e_kv8 <= 1.5 e_bf16."""
    from fault_tolerant_llm_training_amd.generation import KVCache, decode_step, prefill
    from fault_tolerant_llm_training_amd.models.llama import build_model

    margs, model = tiny
    tokens = torch.randint(0, 512, (17,), generator=torch.Generator().manual_seed(9))
    ref = build_model(margs, "cpu", torch.float64, seed=3)
    with torch.no_grad():
        ref.flat.params.copy_(model.flat.params.double().cpu())

    def run(m, dtype, device, kv_dtype):
        cache = KVCache(margs, 17, device, dtype, kv_dtype=kv_dtype)
        prefill(m, tokens[:9], cache)
        return torch.stack([decode_step(m, int(t), cache) for t in tokens[9:]]).cpu()

    got = run(model, torch.bfloat16, "cuda", "fp8")
    e_kv8 = rel(got, run(ref, torch.float64, "cpu", "fp8"))
    e_bf16 = rel(run(model, torch.bfloat16, "cuda", "model"), run(ref, torch.float64, "cpu", "model"))
    print(f"tiny: e_kv8 {e_kv8:.3e} e_bf16 {e_bf16:.3e} ratio {e_kv8 / e_bf16:.3f}")
    assert e_kv8 <= 1.5 * e_bf16
    assert torch.equal(run(model, torch.bfloat16, "cuda", "fp8"), got)
