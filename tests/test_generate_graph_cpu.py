"""Graph-replayed decoding on the CPU path: ``graph=True`` runs the eager loop there and returns the
same ids; the composed device-step ops (step state read from the control block) equal the host-``t``
definitions; the control block round-trips; the command-line flags exist.
"""
import pytest
import torch

PROMPTS = [[7], [3, 250], list(range(20, 37)), [3, 250]]
KEYS = [0, (1 << 63) - 1, 0x8000000000000001 & ((1 << 63) - 1), 0x243F6A8885A308D3 & ((1 << 63) - 1)]


@pytest.fixture(scope="module")
def tiny64():
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    return build_model(model_args_for("tiny", vocab_size=264, seq_len=32), "cpu", torch.float64, seed=7)


@pytest.mark.parametrize("kw", [dict(), dict(temperature=0.8, top_k=40, key=0x5EED, step=3)], ids=["greedy", "sampled"])
def test_graph_flag_on_cpu_returns_the_eager_ids(tiny64, kw):
    from fault_tolerant_llm_training_amd.generation import generate, generate_batch

    want = generate_batch(tiny64, PROMPTS, 10, **kw)
    assert generate_batch(tiny64, PROMPTS, 10, graph=True, **kw) == want
    assert generate_batch(tiny64, PROMPTS, 10, graph=False, **kw) == want
    assert generate(tiny64, PROMPTS[2], 10, graph=True, **kw) == generate(tiny64, PROMPTS[2], 10, **kw)
    assert generate(tiny64, PROMPTS[0], 10, graph=True, **kw) == want[0]  # row 0 is the sampler's row 0
    eos = want[1][4]
    assert generate_batch(tiny64, PROMPTS, 10, eos_id=eos, graph=True, **kw) == \
        generate_batch(tiny64, PROMPTS, 10, eos_id=eos, **kw)


def test_decode_graph_refuses_a_cpu_model(tiny64):
    from fault_tolerant_llm_training_amd.generation import DecodeGraph, graph_supported

    assert not graph_supported(tiny64)
    with pytest.raises(ValueError):
        DecodeGraph(tiny64, 2, 16)


def test_control_block_round_trips():
    from fault_tolerant_llm_training_amd.ops import decode as D

    ctl = D.new_ctl("cpu")
    assert ctl.dtype == torch.int32 and ctl.numel() == D.CTL_WORDS
    for key in KEYS:
        for t, temp, top_k, step in ((0, 0.0, 0, 0), (1000, 0.8, 40, (1 << 32) - 1), (7, 1.5, 1 << 40, 12)):
            D.write_ctl(ctl, t, temp, top_k, key, step)
            got = D.read_ctl(ctl)
            assert got[0] == t and got[3] == key and got[4] == step
            assert got[1] == torch.tensor(temp, dtype=torch.float32).item()  # the float32 the kernel takes
            assert got[2] == min(top_k, (1 << 31) - 1)
    D.write_ctl(ctl, 5, 0.0, 0, 0, 0)
    D.ctl_advance_(ctl)
    D.ctl_advance_(ctl)
    assert D.read_ctl(ctl)[0] == 7
    for bad in (dict(temperature=-1.0), dict(temperature=float("inf")), dict(top_k=-1), dict(t=-1)):
        args = dict(t=0, temperature=0.0, top_k=0, key=0, step=0)
        args.update(bad)
        with pytest.raises(ValueError):
            D.write_ctl(ctl, **args)


def test_composed_dev_cache_ops_equal_the_host_t_definitions():
    from fault_tolerant_llm_training_amd.models.llama import rope_tables
    from fault_tolerant_llm_training_amd.ops import decode as D

    torch.manual_seed(1)
    hq, hkv, d, smax, B = 4, 2, 8, 12, 3
    cos, sin = (x.double() for x in rope_tables(d, smax, 500000.0))
    positions = [0, 5, smax - 3]
    pos0 = torch.tensor(positions, dtype=torch.int32)
    ctl = D.new_ctl("cpu")
    part = D.attn_part(B, hq, smax, d, "cpu")
    kc, vc = torch.randn(B, hkv, smax, d).double(), torch.randn(B, hkv, smax, d).double()
    k1, v1 = kc.clone(), vc.clone()
    for t in (0, 2, 1):  # written between the calls: t is read when the op runs
        D.write_ctl(ctl, t, 0.0, 0, 0, 0)
        qkv = torch.randn(B, (hq + 2 * hkv) * d).double()
        q1 = qkv.clone()
        D.qkv_append_rows_dev_(qkv, cos, sin, pos0, ctl, kc, vc)
        D.qkv_append_rows_(q1, cos, sin, pos0, t, k1, v1, positions)
        assert torch.equal(qkv, q1) and torch.equal(kc, k1) and torch.equal(vc, v1)
        o = torch.full((B, hq * d), float("nan")).double()
        assert D.attn_rows_dev(qkv[:, : hq * d], kc, vc, pos0, ctl, part, o) is o
        assert torch.equal(o, D.attn_rows(q1[:, : hq * d], k1, v1, pos0, t, positions))
    # a row whose position is outside the cache writes nothing; the rows inside are written
    D.write_ctl(ctl, 3, 0.0, 0, 0, 0)
    qkv = torch.randn(B, (hq + 2 * hkv) * d).double()
    before_k, before_v = kc.clone(), vc.clone()
    D.qkv_append_rows_dev_(qkv, cos, sin, pos0, ctl, kc, vc)
    assert torch.equal(kc[2], before_k[2]) and torch.equal(vc[2], before_v[2])
    assert not torch.equal(kc[1], before_k[1])


@pytest.mark.parametrize("temperature,top_k", [(0.0, 0), (0.8, 0), (0.8, 1), (0.8, 40)])
def test_composed_sample_dev_equals_sample_with_the_token_key(temperature, top_k):
    from fault_tolerant_llm_training_amd.generation import token_key
    from fault_tolerant_llm_training_amd.ops import decode as D

    torch.manual_seed(2)
    R, V, n_cap = 5, 64, 1001
    logits = torch.randn(R, V).double()
    ctl = D.new_ctl("cpu")
    for key in KEYS:
        for t in (0, 1, 1000):
            tok = torch.full((R, 1), -1, dtype=torch.int64)
            out = torch.full((R, n_cap), -1, dtype=torch.int64)
            D.write_ctl(ctl, t, temperature, top_k, key, 9)
            D.sample_dev_(logits, ctl, tok, out)
            want = D.sample(logits, temperature, top_k, token_key(key, t), 9)
            assert torch.equal(tok.view(-1), want) and torch.equal(out[:, t], want)
            out[:, t] = -1
            assert (out == -1).all()  # nothing outside column t


def test_token_key_is_one_function():
    from fault_tolerant_llm_training_amd import generation
    from fault_tolerant_llm_training_amd.utils import sampling

    assert generation.token_key is sampling.token_key
    assert generation.token_key(0, 0) == 0x9E3779B97F4A7C15 & ((1 << 63) - 1)
    assert generation.token_key((1 << 63) - 1, 1000) == ((1 << 63) - 1 + 1001 * 0x9E3779B97F4A7C15) & ((1 << 63) - 1)


def test_the_flags_exist():
    from fault_tolerant_llm_training_amd.generate import build_parser
    from fault_tolerant_llm_training_amd.utils.config import get_args

    assert build_parser().parse_args(["--checkpoint", "x", "--decode-graph"]).decode_graph is True
    assert build_parser().parse_args(["--checkpoint", "x"]).decode_graph is False
    assert get_args([]).sample_graph is False
    assert get_args(["--sample-every", "10", "--sample-graph"]).sample_graph is True
    with pytest.raises(SystemExit):
        get_args(["--sample-graph"])  # needs --sample-every
