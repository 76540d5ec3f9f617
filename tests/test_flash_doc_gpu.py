"""Document-masked attention for packed sequences on the MI355X: the DOC instantiations of the
flash kernels (flash_doc_fwd / flash_doc_bwd, flash_f32_doc_*), the boundary scan (doc_bounds) and
the model / training-step level (Transformer.set_document_mask).

Query i sees key j iff doc_start[i] <= j <= i. The attention tests pass the boundaries as host-built
tensors, so they do not depend on the scan kernel. Reference: the fp32 ``ref_attn`` of
test_flash_attn_gpu.py with the document mask added; tolerances are that file's (rel 1e-2 forward,
2e-2 for each of dQ / dK / dV), applied to the whole tensor AND to the rows of every document of at
least 32 tokens (a whole-tensor norm hides one wrong document), plus isfinite everywhere."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def bounds(starts, S):
    """starts: per batch row, the sorted document start positions (the first is 0) -> int32
    (doc_start, doc_end) [B, S] on the GPU."""
    ds = torch.zeros(len(starts), S, dtype=torch.int32)
    de = torch.full((len(starts), S), S, dtype=torch.int32)
    for b, st in enumerate(starts):
        st = sorted(st)
        assert st[0] == 0
        for a, e in zip(st, st[1:] + [S]):
            ds[b, a:e] = a
            de[b, a:e] = e
    return ds.cuda(), de.cuda()


def ref_attn(q, k, v, doc_start):
    """q [B,S,Hq,D], k/v [B,S,Hkv,D] -> o [B,S,Hq,D]; doc_start [B,S]."""
    B, S, Hq, D = q.shape
    rep = Hq // k.shape[2]
    k = k.repeat_interleave(rep, 2)
    v = v.repeat_interleave(rep, 2)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) / D**0.5
    pos = torch.arange(S, device=q.device)
    mask = (pos.view(1, 1, S) > pos.view(1, S, 1)) | (pos.view(1, 1, S) < doc_start.view(B, S, 1).long())
    s = s.masked_fill(mask.view(B, 1, S, S), float("-inf"))
    p = s.softmax(-1)
    return torch.einsum("bhqk,bkhd->bqhd", p, v)


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-12)).item()


def check(name, got, ref, tol, starts, S):
    """got / ref [B, S, H, D]: isfinite, whole-tensor tolerance, and per document of >= 32 tokens."""
    assert torch.isfinite(got).all(), name
    r = rel(got, ref)
    print(f"{name}: whole {r:.3e}")
    assert r < tol, (name, r)
    for b, st in enumerate(starts):
        st = sorted(st)
        for a, e in zip(st, st[1:] + [S]):
            if e - a >= 32:
                r = rel(got[b, a:e], ref[b, a:e])
                assert r < tol, (name, b, a, e, r)


def random_starts(S, seed, max_len):
    g = torch.Generator().manual_seed(seed)
    st, p = [0], 0
    while True:
        p += int(torch.randint(1, max_len, (1,), generator=g))
        if p >= S:
            return st
        st.append(p)


CASES = {
    # a boundary inside a 32-row wave slice and past the first key tile: rows that are still empty
    # while their wave-mates' running max moves (the -inf trap of the forward)
    "inslice": ((1, 256, 2, 1, 128), [[0, 70, 200]]),
    # tile-aligned boundaries (tiles skipped, nothing masked at a boundary) | one-token documents
    # and a last row that is its own document
    "aligned_tiny": ((2, 320, 8, 2, 64), [[0, 64, 128, 192, 256], [0, 1, 2, 319]]),
    "ragged": ((1, 1000, 4, 2, 128), [[0, 333, 334, 901]]),
    "small": ((3, 100, 4, 4, 64), [[0, 99], [0], [0, 31, 32, 33]]),
    "random_2wave": ((1, 2048, 4, 4, 64), [random_starts(2048, 5, 300)]),
    "layer8b": ((1, 2048, 32, 8, 128), [list(range(0, 2048, 256))]),
    # head_dim 64 with 4-wave blocks (4 tiles x 8 x 16 = 512 blocks, the smallest grid that selects
    # them), GQA: the slice-pair dK/dV kernel <64, 4> that only the doc path launches. Boundaries
    # inside a 32-row slice (70, 300, 33, 511), tile-aligned (128, 256, 384) and none
    "wave4_gqa": ((8, 512, 16, 4, 64), [[0, 70, 256, 300], [0, 128, 384], [0, 33, 256, 511], [0],
                                        [0, 70, 256, 300], [0, 1, 2, 129], [0, 255, 256, 257], [0, 300]]),
}


def make(shape, dt=torch.bfloat16, seed=0):
    B, S, Hq, Hkv, D = shape
    torch.manual_seed(seed)
    T = B * S
    qkv = torch.randn(T, (Hq + 2 * Hkv) * D, device="cuda").to(dt)
    qk = torch.randn(T, (Hq + Hkv) * D, device="cuda").to(dt)
    do = torch.randn(T, Hq * D, device="cuda").to(dt)
    return qk, qkv, do


def leaves(qk, qkv, shape, ft=torch.float32):
    B, S, Hq, Hkv, D = shape
    q = qk[:, : Hq * D].to(ft).view(B, S, Hq, D).requires_grad_(True)
    k = qk[:, Hq * D :].to(ft).view(B, S, Hkv, D).requires_grad_(True)
    v = qkv[:, (Hq + Hkv) * D :].to(ft).view(B, S, Hkv, D).requires_grad_(True)
    return q, k, v


def run_case(shape, starts, dt, fwd, bwd, tol_f, tol_b, ft=torch.float32):
    B, S, Hq, Hkv, D = shape
    ds, de = bounds(starts, S)
    qk, qkv, do = make(shape, dt)
    o, lse = fwd(qk, qkv, ds, de)
    q, k, v = leaves(qk, qkv, shape, ft)
    ref = ref_attn(q, k, v, ds)
    check("o", o.view(B, S, Hq, D), ref, tol_f, starts, S)
    dqkv = bwd(do, qk, qkv, o, lse, ds, de)
    gq, gk, gv = torch.autograd.grad(ref, (q, k, v), do.to(ft).view(B, S, Hq, D))
    check("dq", dqkv[:, : Hq * D].view(B, S, Hq, D), gq, tol_b, starts, S)
    check("dk", dqkv[:, Hq * D : (Hq + Hkv) * D].view(B, S, Hkv, D), gk, tol_b, starts, S)
    check("dv", dqkv[:, (Hq + Hkv) * D :].view(B, S, Hkv, D), gv, tol_b, starts, S)


@pytest.fixture(scope="module")
def K():
    from fault_tolerant_llm_training_amd._native import kernels

    return kernels()


@pytest.mark.parametrize("case", list(CASES))
def test_flash_doc_fwd_bwd(K, case):
    shape, starts = CASES[case]
    _, S, Hq, Hkv, D = shape
    run_case(shape, starts, torch.bfloat16,
             lambda qk, qkv, ds, de: K.flash_doc_fwd(qk, qkv, ds, de, S, Hq, Hkv, D),
             lambda do, qk, qkv, o, lse, ds, de: K.flash_doc_bwd(do, qk, qkv, o, lse, ds, de, S, Hq, Hkv, D),
             1e-2, 2e-2)


def test_flash_doc_fp16(K):
    shape, starts = CASES["aligned_tiny"]
    _, S, Hq, Hkv, D = shape
    run_case(shape, starts, torch.float16,
             lambda qk, qkv, ds, de: K.flash_doc_fwd(qk, qkv, ds, de, S, Hq, Hkv, D),
             lambda do, qk, qkv, o, lse, ds, de: K.flash_doc_bwd(do, qk, qkv, o, lse, ds, de, S, Hq, Hkv, D),
             1e-2, 2e-2)


@pytest.mark.parametrize("case", ["inslice", "aligned_tiny"])
def test_flash_doc_leak_amplification(K, case):
    """One forward per document index t: V of every document EXCEPT the t-th of each row is offset
    by 100, and the rows of the t-th documents are compared on their own. Their reference values
    are O(1) (softmax averages of unit normals), so a probability of 1e-3 leaked from any other
    document moves an output element by 0.1: a relative error of 0.1 or more, ten times the 1e-2
    tolerance. (Offsetting the document under test itself would hide the leak twice: relative to
    an offset of 100 j a leak of 1e-3 is 1e-3 / j, and the bf16 output has a spacing of 0.5-2
    there.) Every document is checked, one-token documents included. Forward only: the offset
    does not enter dV, and dQ / dK would measure the bf16 rounding of O times the offset."""
    shape, starts = CASES[case]
    B, S, Hq, Hkv, D = shape
    ds, de = bounds(starts, S)
    qk, qkv0, _ = make(shape)
    vcol = (Hq + Hkv) * D
    docs = [list(zip(sorted(st), sorted(st)[1:] + [S])) for st in starts]
    for t in range(max(len(d) for d in docs)):
        qkv = qkv0.clone()
        for b, d in enumerate(docs):
            for j, (a, e) in enumerate(d):
                if j != t:
                    qkv[b * S + a : b * S + e, vcol:] += 100.0
        o, _ = K.flash_doc_fwd(qk, qkv, ds, de, S, Hq, Hkv, D)
        assert torch.isfinite(o).all()
        q, k, v = leaves(qk, qkv, shape)
        ref = ref_attn(q, k, v, ds)
        for b, d in enumerate(docs):
            if t < len(d):
                a, e = d[t]
                assert ref[b, a:e].abs().max().item() < 10  # the document under test holds no offset
                r = rel(o.view(B, S, Hq, D)[b, a:e], ref[b, a:e])
                assert r < 1e-2, (t, b, a, e, r)


@pytest.mark.parametrize("shape,starts", [((1, 512, 12, 12, 64), [[0, 100, 101, 300]]),
                                          ((1, 1024, 8, 8, 128), [[0, 257, 700]])])
def test_flash_doc_bwd_with_rope_backward(K, shape, starts):
    """No GQA: the direct dK/dV store with the in-kernel RoPE backward == flash_doc_bwd without
    tables followed by rope_bwd_, within the 4e-3 of test_flash_bwd_with_rope_backward."""
    from fault_tolerant_llm_training_amd.models.llama import rope_tables

    B, S, Hq, Hkv, D = shape
    ds, de = bounds(starts, S)
    qk, qkv, do = make(shape, seed=2)
    cos, sin = (t.cuda() for t in rope_tables(D, S, 500000.0))
    o, lse = K.flash_doc_fwd(qk, qkv, ds, de, S, Hq, Hkv, D)
    ref = K.flash_doc_bwd(do, qk, qkv, o, lse, ds, de, S, Hq, Hkv, D)
    K.rope_bwd_(ref, cos, sin, S, Hq, Hkv, D)
    got = K.flash_doc_bwd(do, qk, qkv, o, lse, ds, de, S, Hq, Hkv, D, cos, sin)
    assert torch.isfinite(got).all()
    for lo, hi in ((0, Hq * D), (Hq * D, (Hq + Hkv) * D), ((Hq + Hkv) * D, (Hq + 2 * Hkv) * D)):
        assert rel(got[:, lo:hi], ref[:, lo:hi]) < 4e-3, (lo, hi)
    # and the masked result itself is right (rotated frame, no tables)
    run_case(shape, starts, torch.bfloat16,
             lambda qk, qkv, ds, de: K.flash_doc_fwd(qk, qkv, ds, de, S, Hq, Hkv, D),
             lambda do, qk, qkv, o, lse, ds, de: K.flash_doc_bwd(do, qk, qkv, o, lse, ds, de, S, Hq, Hkv, D),
             1e-2, 2e-2)


@pytest.mark.parametrize("shape", [(1, 1024, 32, 8, 128), (1, 512, 12, 12, 64), (8, 512, 16, 16, 64)])
def test_one_document_is_bitwise_the_plain_unsplit_kernels(K, shape):
    """doc_start = 0, doc_end = S: flash_doc_fwd == flash_fwd with the key split and the pipelined
    kernel off, flash_doc_bwd == flash_bwd(mode 1) with the dQ and dK/dV splits off (at these shapes
    the plain path then selects the dQ and dK/dV kernels the doc path extends), bit for bit.

    (8, 512, 16, 16, 64) is head_dim 64 with 4-wave blocks (512 blocks): there the two paths differ
    on purpose. The plain path runs the one-slice flash_bwd_kernel<64, 1> for dK / dV (faster than
    the slice pair at that geometry) and no switch selects the slice pair for it; the doc path runs
    the slice-pair kernel <64, 4>, the only dK/dV kernel with the mask. The forward and the dQ
    columns (the unsplit dQ kernel on both sides) are still bit-identical; dK / dV come from two
    different kernels and agree within the backward tolerance of this file (2e-2)."""
    B, S, Hq, Hkv, D = shape
    same_dkdv_kernel = not (D == 64 and -(-S // 128) * B * Hq >= 512)
    ds, de = bounds([[0]] * B, S)
    qk, qkv, do = make(shape, seed=4)
    try:
        K.flash_set_fwd_split(0)
        K.flash_set_fwd_pipe(0)
        K.flash_set_dq_split(0)
        K.flash_set_kv_split(0)
        o, lse = K.flash_fwd(qk, qkv, S, Hq, Hkv, D)
        dqkv = K.flash_bwd(do, qk, qkv, o, lse, S, Hq, Hkv, D, 1)
    finally:
        K.flash_set_fwd_split(-1)
        K.flash_set_fwd_pipe(1)
        K.flash_set_dq_split(-1)
        K.flash_set_kv_split(-1)
    o2, lse2 = K.flash_doc_fwd(qk, qkv, ds, de, S, Hq, Hkv, D)
    assert torch.equal(o, o2)
    assert torch.equal(lse[..., :S], lse2[..., :S])
    dqkv2 = K.flash_doc_bwd(do, qk, qkv, o, lse, ds, de, S, Hq, Hkv, D)
    if same_dkdv_kernel:
        assert torch.equal(dqkv, dqkv2)
        return
    assert torch.isfinite(dqkv2).all()
    assert torch.equal(dqkv[:, : Hq * D], dqkv2[:, : Hq * D])
    for name, lo, hi in (("dk", Hq * D, (Hq + Hkv) * D), ("dv", (Hq + Hkv) * D, (Hq + 2 * Hkv) * D)):
        r = rel(dqkv2[:, lo:hi], dqkv[:, lo:hi])
        print(f"{name}: slice pair vs one slice {r:.3e}")
        assert r < 2e-2, (name, r)


def test_flash_doc_bwd_is_bitwise_reproducible(K):
    shape, starts = CASES["layer8b"]
    _, S, Hq, Hkv, D = shape
    ds, de = bounds(starts, S)
    qk, qkv, do = make(shape, seed=1)
    o, lse = K.flash_doc_fwd(qk, qkv, ds, de, S, Hq, Hkv, D)
    a = K.flash_doc_bwd(do, qk, qkv, o, lse, ds, de, S, Hq, Hkv, D)
    b = K.flash_doc_bwd(do, qk, qkv, o, lse, ds, de, S, Hq, Hkv, D)
    assert torch.equal(a, b)


def test_flash_doc_rejects_bad_boundaries(K):
    shape, starts = CASES["inslice"]
    _, S, Hq, Hkv, D = shape
    ds, de = bounds(starts, S)
    qk, qkv, _ = make(shape)
    for bad_s, bad_e in ((ds.long(), de), (ds, de[:, :-1].contiguous()), (ds.cpu(), de), (ds.view(-1), de)):
        with pytest.raises(RuntimeError):
            K.flash_doc_fwd(qk, qkv, bad_s, bad_e, S, Hq, Hkv, D)


def _layouts(S):
    """Token layouts of tests/test_doc_mask_cpu.py (BOS = 1): none, at 0, consecutive, at S - 1,
    and two different rows."""
    def row(pos):
        t = torch.randint(2, 50, (S,), generator=torch.Generator().manual_seed(S + len(pos)))
        for p in pos:
            t[p] = 1
        return t

    rows = [row([]), row([0]), row([0, 1, 2]) if S > 3 else row([0]), row([S - 1]),
            row([0, S // 3, S // 3 + 1, S - 2]), row([5 % S, S // 2])]
    return torch.stack(rows)


@pytest.mark.parametrize("S", [33, 2048, 65536])
def test_doc_bounds_kernel_matches_cpu_composition(S):
    from fault_tolerant_llm_training_amd.ops.attention import doc_bounds

    tok = _layouts(S)
    cs, ce = doc_bounds(tok, 1)
    gs, ge = doc_bounds(tok.cuda(), 1)
    assert gs.dtype == ge.dtype == torch.int32 and gs.is_cuda
    assert torch.equal(gs.cpu(), cs) and torch.equal(ge.cpu(), ce)


@pytest.mark.parametrize("case", ["inslice", "aligned_tiny", "ragged", "small"])
def test_flash_f32_doc(case):
    """The fp32 kernels against a float64 reference, at the fp32 attention tolerances of
    tests/test_dtypes_gpu.py (2e-5 forward, 3x that for the gradients)."""
    from fault_tolerant_llm_training_amd.ops.attention import flash_attn_bwd, flash_attn_fwd

    shape, starts = CASES[case]
    _, S, Hq, Hkv, D = shape
    run_case(shape, starts, torch.float32,
             lambda qk, qkv, ds, de: flash_attn_fwd(qk, qkv, S, Hq, Hkv, D, (ds, de)),
             lambda do, qk, qkv, o, lse, ds, de: flash_attn_bwd(do, qk, qkv, o, lse, S, Hq, Hkv, D, doc=(ds, de)),
             2e-5, 6e-5, ft=torch.float64)


# ------------------------------------------------------------------ model level
def _packed_tokens(B, S, V, seed):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(2, V, (B, S), generator=g)
    lab = torch.randint(2, V, (B, S), generator=g)
    for b in range(B):
        tok[b, 0] = 1
        for p in torch.randint(1, S, (3,), generator=g).tolist():
            tok[b, p] = 1
    return tok, lab


def test_tiny_model_with_document_mask_gpu_vs_cpu():
    """The tiny preset in bf16 on the HIP path with the mask vs the CPU path with the mask: the
    tolerances of test_kernels_gpu.py::test_tiny_model_gpu_vs_cpu; and the mask changes the loss."""
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    def rel_(a, b):
        return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()

    a = model_args_for("tiny", vocab_size=512, seq_len=64)
    mg = build_model(a, "cuda", torch.bfloat16, seed=7)
    mc = build_model(a, "cpu", torch.bfloat16, seed=7)
    mc.load_state_dict({k: v.cpu() for k, v in mg.state_dict().items()})
    tok, lab = _packed_tokens(2, 64, 512, 0)
    with torch.no_grad():
        plain = mg(tok.cuda(), lab.cuda()).item()
    mg.set_document_mask(1)
    mc.set_document_mask(1)
    lg = mg(tok.cuda(), lab.cuda())
    lc = mc(tok, lab)
    lg.backward()
    lc.backward()
    assert abs(lg.item() - lc.item()) < 2e-2
    assert rel_(mg.flat.grads.cpu(), mc.flat.grads) < 3e-2
    assert lg.item() != plain


@pytest.mark.parametrize("recompute_attention", [False, True])
def test_document_mask_activation_checkpointing_is_bit_identical(recompute_attention):
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    a = model_args_for("tiny", vocab_size=512, seq_len=128)
    tok, lab = _packed_tokens(2, 128, 512, 1)
    out = []
    for ck in (0, -1):
        m = build_model(a, "cuda", torch.bfloat16, seed=5)
        m.set_document_mask(1)
        if ck:
            m.set_activation_checkpointing(ck, recompute_attention=recompute_attention)
        loss = m(tok.cuda(), lab.cuda())
        loss.backward()
        torch.cuda.synchronize()
        out.append((loss.item(), m.flat.grads.clone()))
    assert out[0][0] == out[1][0]
    assert torch.equal(out[0][1], out[1][1])


def test_graphed_steps_with_document_mask_bitwise_equal_eager():
    """Whole-step HIP-graph replay with the mask (doc_bounds is captured: it reads the staged token
    buffer) == eager over 3 replayed steps, in the manner of tests/test_graphs_gpu.py."""
    from fault_tolerant_llm_training_amd.graphs import GraphedStep
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for
    from fault_tolerant_llm_training_amd.optim.adamw import FlatAdamW
    from fault_tolerant_llm_training_amd.parallel.ddp import GradReducer
    from fault_tolerant_llm_training_amd.utils.lr import build_lr_scheduler

    V, S = 1024, 256

    def setup():
        a = model_args_for("tiny", vocab_size=V, seq_len=S)
        m = build_model(a, "cuda", torch.bfloat16, seed=3)
        m.set_document_mask(1)
        red = GradReducer(m.flat, m.sinks_in_backward_order(), bucket_mb=1.0)
        opt = FlatAdamW(m.parameters(), m.flat, lr=3e-3, max_grad_norm=1.0, reducer=red)
        m.gate = opt.gate
        return m, red, opt, build_lr_scheduler(opt, 4)

    inv = torch.full((1,), 1.0 / (2 * S), device="cuda")
    batches = [_packed_tokens(2, S, V, 20 + i) for i in range(6)]  # different layouts every step

    m, red, opt, sched = setup()
    losses_e = []
    for tok, lab in batches:
        loss = m(tok.cuda(), lab.cuda(), inv)
        loss.backward()
        red.finish()
        opt.step()
        sched.step()
        losses_e.append(loss.item())
    pe = m.flat.params.clone()

    m2, red2, opt2, sched2 = setup()

    def fwd_bwd(tok, lab):
        loss = m2(tok, lab, inv)
        loss.backward()
        red2.finish()
        return loss

    gs = GraphedStep(m2, red2, opt2, sched2, fwd_bwd)
    losses_g = []
    for tok, lab in batches[:2]:  # eager warmup steps
        loss = fwd_bwd(tok.cuda(), lab.cuda())
        opt2.step()
        sched2.step()
        losses_g.append(loss.item())
    losses_g.append(gs.prime(*batches[2]).item())
    for tok, lab in batches[3:]:
        losses_g.append(gs.step(tok, lab).item())
    gs.finish()
    torch.cuda.synchronize()
    assert losses_g == losses_e
    assert torch.equal(m2.flat.params, pe)
