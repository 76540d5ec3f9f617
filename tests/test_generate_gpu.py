"""Text generation on the GPU: the decode kernels (csrc/kernels/decode.hip) against their
definitions, the decode path of a model against its full forward, and --sample-every runs of
train.py (eager and --hip-graph) against runs without it.
"""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
MANT = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}
EMIN = {torch.bfloat16: -126, torch.float16: -14, torch.float32: -126}


@pytest.fixture(scope="module")
def K():
    from fault_tolerant_llm_training_amd._native import kernels

    return kernels()


def rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def ulp_at(ref: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of ``dtype`` at the float64 values ``ref``."""
    _, e = torch.frexp(ref.abs().clamp(min=2.0 ** -300))  # |ref| = m 2^e, m in [0.5, 1)
    e = (e - 1).clamp(min=EMIN[dtype])
    return torch.ldexp(torch.ones_like(ref), e - MANT[dtype])


# ------------------------------------------------------------------------------- gemv / gemv_swiglu
NS, KS = [1, 5, 257, 4096], [8, 264, 4096]


def _ints(shape, lo, hi, dtype, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen, device="cuda").to(dtype)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_gemv_small_integers_are_exact(K, dt):
    """Small-integer operands: every product and partial sum is exact in fp32, so the result is the
    float64 product rounded once to the output dtype, bit for bit; with and without residual."""
    dtype = DTYPES[dt]
    gen = torch.Generator(device="cuda").manual_seed(11)
    for N in NS:
        for Kd in KS:
            x, w = _ints((Kd,), -4, 4, dtype, gen), _ints((N, Kd), -4, 4, dtype, gen)
            res = _ints((N,), -64, 64, dtype, gen)
            ref = torch.mv(w.double(), x.double())
            assert abs(ref).max() < 2 ** 24
            y = K.gemv(x, w, None)
            assert y.dtype == dtype and y.shape == (N,)
            assert torch.equal(y, ref.to(dtype)), (N, Kd)
            assert torch.equal(K.gemv(x, w, res), (ref + res.double()).to(dtype)), (N, Kd)
            assert torch.equal(K.gemv(x, w, None), y)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_gemv_random_operands_within_one_rounding_plus_fp32_accumulation(K, dt):
    dtype = DTYPES[dt]
    gen = torch.Generator(device="cuda").manual_seed(12)
    for N in NS:
        for Kd in KS:
            x = torch.randn(Kd, generator=gen, device="cuda").to(dtype)
            w = (torch.randn(N, Kd, generator=gen, device="cuda") / math.sqrt(Kd)).to(dtype)
            res = torch.randn(N, generator=gen, device="cuda").to(dtype)
            for r in (None, res):
                ref = torch.mv(w.double(), x.double())
                mag = torch.mv(w.double().abs(), x.double().abs())
                if r is not None:
                    ref, mag = ref + r.double(), mag + r.double().abs()
                y = K.gemv(x, w, r)
                err = (y.double() - ref).abs()
                bound = 0.5 * ulp_at(ref, dtype) + Kd * 2.0 ** -23 * mag
                worst = float((err / bound).max())
                print(f"gemv {dt} N={N} K={Kd} residual={r is not None}: max err / bound = {worst:.3f}")
                assert worst <= 1.0, (N, Kd)
                assert torch.equal(K.gemv(x, w, r), y)  # bit-reproducible


@pytest.mark.parametrize("dt", list(DTYPES))
def test_gemv_swiglu_equals_the_composed_ops_bit_for_bit(K, dt):
    from fault_tolerant_llm_training_amd.ops.functional import swiglu_reference

    dtype = DTYPES[dt]
    gen = torch.Generator(device="cuda").manual_seed(13)
    for H in NS:
        for Kd in KS:
            x = torch.randn(Kd, generator=gen, device="cuda").to(dtype)
            w13 = (2 * torch.randn(2 * H, Kd, generator=gen, device="cuda") / math.sqrt(Kd)).to(dtype)
            a = K.gemv_swiglu(x, w13)
            want = swiglu_reference(K.gemv(x, w13, None))
            assert a.shape == (H,) and a.dtype == dtype
            diff = int((a.view(torch.int16 if dtype != torch.float32 else torch.int32)
                        != want.view(torch.int16 if dtype != torch.float32 else torch.int32)).sum())
            print(f"gemv_swiglu {dt} H={H} K={Kd}: {diff} of {H} outputs differ")
            assert torch.equal(a, want), (H, Kd, diff)
            assert torch.equal(K.gemv_swiglu(x, w13), a)


def test_gemv_refuses_what_it_cannot_vectorise_and_the_wrapper_falls_back(K):
    from fault_tolerant_llm_training_amd.ops.decode import gemv

    x, w = torch.randn(12, device="cuda").bfloat16(), torch.randn(3, 12, device="cuda").bfloat16()
    with pytest.raises(RuntimeError):
        K.gemv(x, w, None)  # K % 8
    assert torch.equal(gemv(x, w), torch.mv(w, x))
    x, w = torch.randn(17, device="cuda").bfloat16()[1:], torch.randn(3, 16, device="cuda").bfloat16()
    with pytest.raises(RuntimeError):
        K.gemv(x, w, None)  # x not 16-byte aligned
    assert torch.equal(gemv(x, w), torch.mv(w, x))
    x32, w32 = torch.randn(12, device="cuda"), torch.randn(5, 12, device="cuda")
    ref = torch.mv(w32.double(), x32.double())
    assert (K.gemv(x32, w32, None).double() - ref).abs().max() < 1e-5  # fp32: K % 4 is enough


# ------------------------------------------------------------------------------- decode_qkv_append_
@pytest.mark.parametrize("hq,hkv,d", [(4, 2, 64), (4, 1, 128)])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_qkv_append(K, hq, hkv, d, dt):
    from fault_tolerant_llm_training_amd.models.llama import rope_tables
    from fault_tolerant_llm_training_amd.ops.functional import rope_reference

    dtype, smax = DTYPES[dt], 24
    cos, sin = (t.cuda() for t in rope_tables(d, smax, 500000.0))
    torch.manual_seed(5)
    for pos in (0, 1, smax - 1):
        qkv = torch.randn((hq + 2 * hkv) * d, device="cuda").to(dtype)
        kc, vc = (torch.randn(hkv, smax, d, device="cuda").to(dtype) for _ in range(2))
        q0, k0, v0 = qkv.clone(), kc.clone(), vc.clone()
        K.decode_qkv_append_(qkv, cos, sin, pos, kc, vc)
        qk = rope_reference(q0[: (hq + hkv) * d].float().view(1, 1, hq + hkv, d), cos[pos : pos + 1],
                            sin[pos : pos + 1]).view(hq + hkv, d)
        assert rel(qkv[: hq * d], qk[:hq].reshape(-1)) < 1e-2  # the tolerance of test_kernels_gpu.py::test_rope
        assert rel(kc[:, pos], qk[hq:]) < 1e-2
        assert torch.equal(qkv[hq * d :], q0[hq * d :])  # K and V of qkv itself stay
        assert torch.equal(vc[:, pos], q0[(hq + hkv) * d :].view(hkv, d))
        others = [i for i in range(smax) if i != pos]
        assert torch.equal(kc[:, others], k0[:, others]) and torch.equal(vc[:, others], v0[:, others])
    with pytest.raises(RuntimeError):
        K.decode_qkv_append_(qkv, cos, sin, smax, kc, vc)
    with pytest.raises(RuntimeError):
        K.decode_qkv_append_(qkv, cos, sin, -1, kc, vc)


# ------------------------------------------------------------------------------- decode_attn
@pytest.mark.parametrize("hq,hkv,d", [(4, 2, 64), (4, 1, 128), (4, 4, 64)])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_decode_attn(K, hq, hkv, d, dt):
    from test_flash_attn_gpu import ref_attn

    dtype = DTYPES[dt]
    C = int(K.decode_attn_chunk())
    smax = 2 * C + 8
    torch.manual_seed(6)
    for n in (1, C - 1, C, C + 1, 2 * C + 3):
        kc, vc = (torch.randn(hkv, smax, d, device="cuda").to(dtype) for _ in range(2))
        q = torch.randn(hq * d, device="cuda").to(dtype)
        o = K.decode_attn(q, kc, vc, n)
        qa = torch.zeros(1, n, hq, d, device="cuda")
        qa[0, -1] = q.float().view(hq, d)
        ref = ref_attn(qa, kc[:, :n].float().transpose(0, 1)[None], vc[:, :n].float().transpose(0, 1)[None])[0, -1]
        e = rel(o.view(hq, d), ref)
        print(f"decode_attn {dt} Hq={hq} Hkv={hkv} D={d} n_keys={n}: rel {e:.2e}")
        assert e < 1e-2, n
        assert torch.equal(K.decode_attn(q, kc, vc, n), o)
        kn, vn = kc.clone(), vc.clone()
        kn[:, n:] = float("nan")
        vn[:, n:] = float("nan")
        assert torch.equal(K.decode_attn(q, kn, vn, n), o)  # rows at and beyond n_keys are never read
    with pytest.raises(RuntimeError):
        K.decode_attn(q, kc, vc, smax + 1)
    with pytest.raises(RuntimeError):
        K.decode_attn(q, kc, vc, 0)


# ------------------------------------------------------------------------------- sample_
@pytest.mark.parametrize("V", [50304, 131072])
def test_greedy_is_exact_on_planted_ties(K, V):
    from fault_tolerant_llm_training_amd.utils.sampling import sample_reference

    torch.manual_seed(7)
    x = torch.randn(8, V, device="cuda").bfloat16()
    plants = [(V - 1, 7, 2048), (2047, 2048), (V - 8, V - 1), (0, V - 1), (12345, 12346, 40000), (8, 9), (4095, 511),
              (V // 2,)]
    for r, cols in enumerate(plants):
        x[r, list(cols)] = 50.0
    x[7, 3] = float("nan")  # not ordered: never the maximum
    out = torch.empty(8, dtype=torch.int64, device="cuda")
    K.sample_(x, out, 0.0, 0, 99, 0)
    assert out.tolist() == [min(c) for c in plants]
    assert torch.equal(out.cpu(), sample_reference(x, 0.0, 0, 99, 0))
    K.sample_(x, out, 0.9, 1, 99, 3)  # top_k = 1 is greedy at any temperature
    assert out.tolist() == [min(c) for c in plants]


MARGIN = 1e-5  # rows whose u * total lies this close (relative) to a cumulative boundary may be left out


@pytest.fixture(scope="module")
def sample_case():
    from fault_tolerant_llm_training_amd.utils.sampling import sample_reference

    torch.manual_seed(8)
    x = (2.5 * torch.randn(4096, 50304, device="cuda")).bfloat16()
    tok, margin = sample_reference(x, 0.8, 40, key=0x5EED5EED, step=21, return_margin=True)
    return x, tok, margin


def test_sampler_matches_the_float64_oracle(K, sample_case):
    from fault_tolerant_llm_training_amd.utils.sampling import sample_reference

    x, tok, margin = sample_case
    out = torch.empty(4096, dtype=torch.int64, device="cuda")
    K.sample_(x, out, 0.8, 40, 0x5EED5EED, 21)
    again = torch.empty_like(out)
    K.sample_(x, again, 0.8, 40, 0x5EED5EED, 21)
    assert torch.equal(out, again)
    close = margin < MARGIN
    wrong = (out.cpu() != tok).numpy()
    print(f"sample_: {int(wrong.sum())} of 4096 rows differ from the oracle, {int(close.sum())} rows within "
          f"{MARGIN} of a boundary, distinct tokens {len(set(tok.tolist()))}")
    assert close.sum() <= 0.01 * 4096
    assert not (wrong & ~close).any()
    # the oracle against itself in fp32 stays within the same cap for this seed (CPU only)
    tok32 = sample_reference(x[:1024], 0.8, 40, key=0x5EED5EED, step=21, dtype=np.float32)
    wrong32 = (tok32 != tok[:1024]).numpy()
    assert not (wrong32 & ~close[:1024]).any() and wrong32.sum() <= 0.01 * 1024
    # a row alone at its row index draws the same token: the draw depends on the row index only
    K.sample_(x[:3], again[:3], 0.8, 40, 0x5EED5EED, 21)
    assert torch.equal(again[:3], out[:3])
    K.sample_(x, again, 0.8, 40, 0x5EED5EED, 22)
    assert not torch.equal(again, out)


def test_sampler_top_k_0_and_ties_at_the_kth_value(K, sample_case):
    from fault_tolerant_llm_training_amd.utils.sampling import sample_reference

    # The share of rows within MARGIN of a boundary grows with the number of candidates: about
    # 2 * MARGIN per candidate that carries weight. With all 50304 columns as candidates that is no
    # longer a small share (a fifth of the rows), so there the rows away from a boundary must match and
    # must be the majority; the 1 % cap is asserted where few candidates make it meaningful: V = 64
    # (expected share 64 * 2e-5) and top_k = 7.
    x = sample_case[0][:512]
    for xs, temperature, top_k, cap in ((x, 1.0, 0, 0.5), (x, 0.8, 50304, 0.5), (x, 1.3, 7, 0.01),
                                        (sample_case[0][:, :64].contiguous(), 1.0, 0, 0.01)):
        R = xs.shape[0]
        tok, margin = sample_reference(xs, temperature, top_k, key=123, step=4, return_margin=True)
        out = torch.empty(R, dtype=torch.int64, device="cuda")
        K.sample_(xs, out, temperature, top_k, 123, 4)
        close = margin < MARGIN
        wrong = (out.cpu() != tok).numpy()
        print(f"sample_ V={xs.shape[1]} T={temperature} top_k={top_k}: {int(wrong.sum())} of {R} rows differ, "
              f"{int(close.sum())} within {MARGIN} of a boundary")
        assert close.sum() <= cap * R
        assert not (wrong & ~close).any(), (temperature, top_k)
    # a flat row: every value ties at the k-th one, so the candidates are the k lowest columns
    flat = torch.zeros(64, 4096, device="cuda").bfloat16()
    out = torch.empty(64, dtype=torch.int64, device="cuda")
    K.sample_(flat, out, 1.0, 5, 77, 0)
    assert int(out.max()) < 5 and len(set(out.tolist())) > 1
    assert torch.equal(out.cpu(), sample_reference(flat, 1.0, 5, 77, 0))
    with pytest.raises(RuntimeError):
        K.sample_(flat[:, :4092], out, 1.0, 5, 77, 0)


# ------------------------------------------------------------------------------- model level
def _model_pair(margs):
    from fault_tolerant_llm_training_amd.models.llama import build_model

    gpu = build_model(margs, "cuda", torch.bfloat16, seed=3)
    cpu = build_model(margs, "cpu", torch.float32, seed=3)
    with torch.no_grad():
        cpu.flat.params.copy_(gpu.flat.params.float().cpu())
    return gpu, cpu


@pytest.mark.parametrize("name", ["tiny", "dim512"])
def test_decode_logits_are_as_close_to_fp32_as_the_full_forward(name):
    """e_full: the existing forward's logits against the fp32 CPU model of the same weights; e_dec:
    the teacher-forced decode logits. The decode path rounds at the same places and sums in another
    order, so e_dec <= 2 e_full; likewise prefill + decode."""
    from fault_tolerant_llm_training_amd.generation import KVCache, decode_step, prefill
    from fault_tolerant_llm_training_amd.models.llama import TransformerModelArgs, model_args_for

    if name == "tiny":
        margs = model_args_for("tiny", vocab_size=512, seq_len=64)
    else:
        margs = TransformerModelArgs(dim=512, n_layers=2, n_heads=4, n_kv_heads=2, multiple_of=64, vocab_size=512,
                                     seq_len=64)
    gpu, cpu = _model_pair(margs)
    torch.manual_seed(9)
    P = 40
    tokens = torch.randint(0, 512, (P,))
    with torch.no_grad():
        ref = cpu(tokens.view(1, -1))[0]
        full = gpu(tokens.view(1, -1).cuda())[0]
    e_full = rel(full.cpu(), ref)

    def run(prefix):
        cache = KVCache(margs, P, "cuda", torch.bfloat16)
        rows = [prefill(gpu, tokens[:prefix], cache)] if prefix else []
        rows += [decode_step(gpu, int(tokens[t]), cache) for t in range(prefix, P)]
        return torch.stack(rows).cpu()

    dec = run(0)
    e_dec = rel(dec, ref)
    pre = run(17)
    e_pre = rel(pre, ref[16:])
    print(f"model {name}: e_full {e_full:.3e} e_dec {e_dec:.3e} e_prefill+decode {e_pre:.3e}")
    assert e_dec <= 2 * e_full
    assert e_pre <= 2 * e_full
    assert torch.equal(run(0), dec)  # bit-reproducible end to end


def test_generate_on_the_gpu_is_greedy_consistent_and_reproducible():
    from fault_tolerant_llm_training_amd.generation import generate
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    model = build_model(model_args_for("tiny", vocab_size=512, seq_len=64), "cuda", torch.bfloat16, seed=3)
    a = generate(model, [1, 5, 9], 12, temperature=0.9, top_k=30, key=42, step=7)
    assert a == generate(model, [1, 5, 9], 12, temperature=0.9, top_k=30, key=42, step=7)
    assert a != generate(model, [1, 5, 9], 12, temperature=0.9, top_k=30, key=42, step=8)
    assert len(a) == 12 and all(0 <= t < 512 for t in a)
    g = generate(model, [1, 5, 9], 12)
    assert g == generate(model, [1, 5, 9], 12, temperature=0.5, top_k=1)


# ------------------------------------------------------------------------------- train.py
GPU = ["--device", "cuda", "--model", "tiny", "--synthetic-data", "--vocab-size", "1024", "--sequence-length", "128",
       "--batch-size", "2", "--training-steps", "6", "--logging-frequency", "1", "--state-digest", "--prefetch", "1"]
MODES = {"eager": [], "graph": ["--hip-graph"]}
SAMPLE = ["--sample-every", "2", "--sample-tokens", "16", "--sample-temperature", "0.8", "--sample-top-k", "40"]


@pytest.fixture(scope="module")
def train_runs(tmp_path_factory):
    from helpers import run_train

    cache = {}

    def get(mode, on):
        if (mode, on) not in cache:
            d = str(tmp_path_factory.mktemp(f"{mode}{int(on)}"))
            rc, out = run_train(d, "1", GPU + MODES[mode] + (SAMPLE if on else []) +
                                ["--metrics-file", "m.jsonl", "--checkpoint-path", os.path.join(d, "ck")], timeout=240)
            assert rc == 0, out
            recs = [json.loads(ln) for ln in open(os.path.join(d, "m.jsonl")).read().splitlines() if ln.strip()]
            cache[(mode, on)] = (out, [r for r in recs if "sample_step" in r])
        return cache[(mode, on)]

    return get


def _losses(out):
    return re.findall(r"Training step: (\d+) \| Loss: ([-\d.naninf]+) .*?grad_norm: ([-\d.naninf]+)", out)


def _digest(out):
    m = re.search(r"State digest at step 6: (params=\w+ exp_avg=\w+ exp_avg_sq=\w+ optimizer_step=\d+ data_loader=.*)",
                  out)
    assert m, out
    return m.group(1)


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_training_is_unchanged_by_sampling(train_runs, mode):
    off, none = train_runs(mode, False)
    on, recs = train_runs(mode, True)
    assert none == [] and "Sample at step" not in off
    assert len(_losses(off)) == 6 and _losses(off) == _losses(on)
    assert _digest(off) == _digest(on)
    assert [r["sample_step"] for r in recs] == [2, 4, 6]
    for r in recs:
        assert len(r["sample_ids"]) == 16 and all(0 <= t < 1024 for t in r["sample_ids"])
        assert f"Sample at step {r['sample_step']} | {r['sample_text']!r} | 16 tokens | " in on


def test_eager_and_graph_runs_log_the_same_sample(train_runs):
    a, b = train_runs("eager", True)[1], train_runs("graph", True)[1]
    assert [(r["sample_step"], r["sample_ids"]) for r in a] == [(r["sample_step"], r["sample_ids"]) for r in b]
