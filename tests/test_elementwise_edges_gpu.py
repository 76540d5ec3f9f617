"""The streaming HIP kernels (norm, SwiGLU, RoPE, cross-entropy, gradient norm, AdamW) held element by
element to fp64 references at their dispatch and value edges (criterion and references:
tests/elementwise_oracle.py; its CPU proof: tests/test_elementwise_oracle_cpu.py).

Figures measured on an MI355X (largest share of non-RNE elements against the 2 % cap, largest error in
units of the bound) are printed by test_zz_figures and recorded here:

    kernel          non-RNE share   error / bound
    adamw           0.0000 %        0.872
    colsum          0.0000 %        0.500
    grad_norm       -               0.016
    norm_bwd        0.0000 %        0.937
    norm_bwd_part   -               0.101
    norm_finish     -               0.087
    norm_fwd        0.1221 %        0.500
    rope_fwd / bwd  0.0000 %        0.612 / 0.639
    sumsq_into      -               0.039
    swiglu_fwd/bwd  0.0031 %        0.846
    xent_fwd        -               0.215
    xent_bwd        0.0000 %        0.868

(0.500 for a 16-bit output without slack is an exact RNE result: half a storage ulp.) Every case
passed on its first run on the device. One defect was found by reading and fixed before that run: a
cross-entropy row whose first 8-column group of a thread is -inf left the per-thread running maximum at
-inf, so x - max was -inf - (-inf) = NaN in xent_fwd and xent_eval_; their loops now skip such a group,
as the wave merge below them already did (the rows of test_xent with -inf groups cover it). A second
came from test_grad_norm_adamw (test_dtypes_gpu.py) at training-scale inputs: adamw_ formed 1 - beta and
the bias corrections in fp32; they are now formed in double and rounded once, and the AdamW reference
here uses plain double scalars.
"""
import math

import pytest
import torch

import elementwise_oracle as O
from elementwise_oracle import BF16, DTYPES, F16, F32, accept, bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from fault_tolerant_llm_training_amd._native import kernels

    return kernels()


def dev(t):
    return None if t is None else t.cuda()


dtp = pytest.mark.parametrize("dt", DTYPES, ids=O.tag)
lnp = pytest.mark.parametrize("ln", [False, True], ids=["rms", "ln"])


# ---------------------------------------------------------------- norm
@dtp
@lnp
@pytest.mark.parametrize("add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("N", O.NORM_FWD_N)
def test_norm_fwd(K, N, add, ln, dt):
    for M in O.NORM_FWD_M:
        x, d, w = O.norm_fwd_inputs(M, N, dt, ln, add)
        if add:
            y, rstd, mean, h = K.add_norm_fwd(dev(x), dev(d), dev(w), O.NORM_EPS, ln)
            hr = (x.float() + d.float()).to(dt)
            assert bits_equal(h, hr), f"h is not the {O.tag(dt)} add (M={M})"
        else:
            y, rstd, mean = K.norm_fwd(dev(x), dev(w), O.NORM_EPS, ln)
            y2, rstd2, _, h2 = K.add_norm_fwd(dev(x), None, dev(w), O.NORM_EPS, ln)
            assert bits_equal(y, y2) and bits_equal(rstd, rstd2) and h2.numel() == 0
            hr = x
        ref = O.norm_fwd_ref(hr, w, dt, ln)
        note = f"M={M} N={N} ln={ln} add={add}"
        accept("norm_fwd.y", y, ref["y"][0], dt, ref["y"][1], ref["y"][2], note)
        accept("norm_fwd.rstd", rstd, ref["rstd"][0], F32, ref["rstd"][1], note=note)
        if ln:
            accept("norm_fwd.mean", mean, ref["mean"][0], F32, ref["mean"][1], note=note)
        else:
            assert mean.numel() == 0
        if M > 1:  # the all-zero row: rstd = eps^-1/2
            assert abs(rstd[1].item() - O.NORM_EPS ** -0.5) <= 4 * O.EPS32 * O.NORM_EPS ** -0.5


def run_norm_bwd(K, M, N, dt, ln):
    inp = O.norm_bwd_inputs(M, N, dt, ln)
    dx64, dxs, dw64, dws = O.norm_bwd_ref(inp, dt, ln)
    c = {k: dev(v) for k, v in inp.items()}
    nsq = (N + 31) // 32
    note = f"M={M} N={N} ln={ln}"
    for dres in (False, True):
        for acc in (False, True):
            outs = []
            for _ in range(2):  # the second run: bit-equal repeatability
                dw = c["dw0"].clone()
                sq = torch.full((nsq,), 7.0, device="cuda")  # stale contents must be overwritten
                dx = K.norm_bwd(c["dy"], c["x"], c["w"], c["rstd"], c["mean"], dw, c["dres"] if dres else None, acc, sq)
                outs.append((dx, dw, sq))
            assert all(bits_equal(a, b) for a, b in zip(*outs)), f"not repeatable: {note}"
            dx, dw, sq = outs[0]
            a = inp["dres"].double() if dres else 0.0
            b = inp["dw0"].double() if acc else 0.0
            n2 = f"{note} dres={dres} acc={acc}"
            accept("norm_bwd.dx", dx, dx64 + a, dt, dxs + O.EPS32 * (inp["dres"].double().abs() if dres else 0.0), note=n2)
            accept("norm_bwd.dw", dw, dw64 + b, dt, dws + O.EPS32 * (inp["dw0"].double().abs() if acc else 0.0), note=n2)
            # sq[i]: the sum of squares of the 32 stored dw of block i: square, 5 shuffle levels
            d2 = torch.zeros(nsq * 32, dtype=torch.float64)
            d2[:N] = dw.cpu().double().pow(2)
            accept("colsum.sq", sq, d2.view(nsq, 32).sum(-1), F32, 7 * O.EPS32 * d2.view(nsq, 32).sum(-1), note=n2)
    # the two halves on their own give the fused op's bits; the partial rows sum to dw
    dxp, part = K.norm_bwd_part(c["dy"], c["x"], c["w"], c["rstd"], c["mean"], None)
    dw = torch.empty_like(c["dw0"])
    K.colsum_(part, dw, False, None)
    dw2 = torch.empty_like(c["dw0"])
    dx2 = K.norm_bwd(c["dy"], c["x"], c["w"], c["rstd"], c["mean"], dw2, None, False, None)
    assert bits_equal(dxp, dx2) and bits_equal(dw, dw2) and part.shape[1] == N and part.dtype == F32
    accept("norm_bwd_part.part", part.double().sum(0).float(), dw64, F32, dws + part.shape[0] * O.EPS32 * dw64.abs(), note=note)


@dtp
@lnp
@pytest.mark.parametrize("M,N", O.NORM_BWD_ONEWAVE)
def test_norm_bwd_one_wave(K, M, N, ln, dt):
    run_norm_bwd(K, M, N, dt, ln)


@dtp
@lnp
@pytest.mark.parametrize("M,N", O.NORM_BWD_SPLIT)
def test_norm_bwd_split(K, M, N, ln, dt):
    run_norm_bwd(K, M, N, dt, ln)


@dtp
@lnp
@pytest.mark.parametrize("M,N", O.NORM_BWD_FALLBACK)
def test_norm_bwd_split_disabled(K, M, N, ln, dt, monkeypatch):
    monkeypatch.setenv("FT_NORM_BWD_SPLIT", "0")  # read on every call
    run_norm_bwd(K, M, N, dt, ln)


@dtp
@pytest.mark.parametrize("N", [8, 40, 4096])
@pytest.mark.parametrize("P", [1, 9])
def test_colsum(K, P, N, dt):
    g = O.gen(9, P, N)
    part = torch.randn(P, N, generator=g)
    dw0 = torch.randn(N, generator=g).to(dt)
    nsq = (N + 31) // 32
    for acc in (False, True):
        dw = dw0.cuda()
        sq = torch.full((nsq,), 7.0, device="cuda")
        K.colsum_(part.cuda(), dw, acc, sq)
        ref = part.double().sum(0) + (dw0.double() if acc else 0.0)
        # 8 row groups of ceil(P / 8) rows, then 8 partials and the old value: ceil(P / 8) + 9 additions
        sl = ((P + 7) // 8 + 9) * O.EPS32 * (part.double().abs().sum(0) + dw0.double().abs())
        accept("colsum.dw", dw, ref, dt, sl, note=f"P={P} N={N} acc={acc}")
        d2 = torch.zeros(nsq * 32, dtype=torch.float64)
        d2[:N] = dw.cpu().double().pow(2)
        accept("colsum.sq", sq, d2.view(nsq, 32).sum(-1), F32, 7 * O.EPS32 * d2.view(nsq, 32).sum(-1))


# ---------------------------------------------------------------- SwiGLU
def run_swiglu(K, gu, da, dt, what):
    ref = O.swiglu_ref(gu, da, dt)
    try:
        for exact in (False, True):
            K.set_exact_math(exact)
            a = K.swiglu_fwd(gu.cuda())
            dgu = K.swiglu_bwd(da.cuda(), gu.cuda())
            accept("swiglu_fwd", a, ref["a"][0], dt, ref["a"][1], note=f"{what} exact={exact}")
            accept("swiglu_bwd", dgu, ref["dgu"][0], dt, ref["dgu"][1], note=f"{what} exact={exact}")
    finally:
        K.set_exact_math(False)


@dtp
@pytest.mark.parametrize("random_u", [False, True], ids=["u1", "urand"])
def test_swiglu_every_gate(K, dt, random_u):
    gu, da = O.swiglu_inputs(dt, random_u)
    run_swiglu(K, gu, da, dt, "gate sweep")


def test_swiglu_grid_stride(K):
    gu, da = O.swiglu_stride_inputs()
    run_swiglu(K, gu, da, BF16, "T=1040 F=8192")


# ---------------------------------------------------------------- RoPE
@dtp
@pytest.mark.parametrize("B,S,hq,hkv,d", O.ROPE_CASES)
def test_rope(K, B, S, hq, hkv, d, dt):
    qkv, cos, sin = O.rope_inputs(B, S, hq, hkv, d, dt)
    assert cos.shape[0] > S
    qk = K.rope_fwd(qkv.cuda(), cos.cuda(), sin.cuda(), S, hq, hkv, d)
    ref, sl = O.rope_ref(qkv, cos, sin, S, hq, hkv, d)
    accept("rope_fwd", qk, ref, dt, sl, note=f"S={S} d={d}")
    dq = qkv.cuda()
    K.rope_bwd_(dq, cos.cuda(), sin.cuda(), S, hq, hkv, d)
    ref, sl = O.rope_ref(qkv, cos, sin, S, hq, hkv, d, bwd=True)
    width = (hq + hkv) * d
    accept("rope_bwd", dq[:, :width], ref, dt, sl, note=f"S={S} d={d}")
    assert bits_equal(dq[:, width:], qkv[:, width:]), "rope_bwd_ touched the V columns"


# ---------------------------------------------------------------- cross-entropy, scale_by_
@dtp
@pytest.mark.parametrize("T,V", [(5, V) for V in O.XENT_V] + [(32769, 8)])
def test_xent(K, T, V, dt):
    x, labs = O.xent_inputs(T, V, dt)
    for i, lab in enumerate(labs):
        note = f"T={T} V={V} labels {i}"
        loss, lse = K.xent_fwd(x.cuda(), lab.cuda(), O.IGNORE)
        lse64, lses, loss64, losss = O.xent_ref(x, lab)
        accept("xent_fwd.lse", lse, lse64, F32, lses, note=note)
        accept("xent_fwd.loss", loss, loss64, F32, losss, note=note)
        # the evaluation kernel repeats this arithmetic (tests/test_eval_gpu.py): the same fixed-point sum,
        # no row left out as non-finite, on the -inf groups too
        live = lab != O.IGNORE
        acc = torch.zeros(4, dtype=torch.int64, device="cuda")
        K.xent_eval_(x.cuda(), lab.cuda(), acc, O.IGNORE)
        want = torch.round(loss.cpu() * float(2 ** 24)).to(torch.int64)[live].sum().item()
        assert acc[0].item() == want and acc[1].item() == int(live.sum()) and acc[3].item() == 0, note
        grad = torch.tensor([2.0])
        inv = torch.tensor([1.0 / max(1, int((lab != O.IGNORE).sum()))])
        l32 = lse64.float()
        g = x.cuda()
        K.xent_bwd_(g, lab.cuda(), l32.cuda(), grad.cuda(), inv.cuda(), O.IGNORE)
        g64, gs = O.xent_bwd_ref(x, lab, l32, grad[0], inv[0])
        accept("xent_bwd", g, g64, dt, gs, note=note)


@dtp
@pytest.mark.parametrize("n", [8 * 1000, 8 * (2048 * 256 + 300)], ids=["small", "past-grid-cap"])
def test_scale_by(K, n, dt):
    x = (3 * torch.randn(n, generator=O.gen(10, n))).to(dt)
    x[:4] = torch.tensor([0.0, -0.0, math.inf, -math.inf]).to(dt)
    for s in (1.0, 0.5, 1.0 / 3.0):
        g = torch.tensor([s], dtype=F32)
        y = x.cuda()
        K.scale_by_(y, g.cuda())
        assert bits_equal(y, x if s == 1.0 else (x.float() * g).to(dt)), f"scale_by_ g={s}"


# ---------------------------------------------------------------- gradient norm
@dtp
def test_sumsq_into(K, dt):
    x = torch.randn(8000, generator=O.gen(8)).to(dt)
    for nb in (1, 3, 4096):
        part = torch.full((nb,), 7.0, device="cuda")  # blocks with no work must write 0 over this
        K.sumsq_into_(x.cuda(), part)
        p2 = torch.full((nb,), -3.0, device="cuda")
        K.sumsq_into_(x.cuda(), p2)
        assert bits_equal(part, p2), "sumsq_into_ is not order-fixed"
        ref, sl = O.sumsq_ref(x, nb)
        accept("sumsq_into", part, ref, F32, sl, note=f"nb={nb}")
        if nb == 4096:
            assert torch.count_nonzero(part[4:]).item() == 0


@pytest.mark.parametrize("view", ["aligned", "offset"])
@pytest.mark.parametrize("np_", [1, 3, 4, 5, 1023, 4097])
def test_norm_finish(K, np_, view):
    p = torch.rand(np_ + 1, generator=O.gen(11, np_)) + 0.01
    pc = p.cuda()
    part, pr = (pc[1:], p[1:]) if view == "offset" else (pc[:-1], p[:-1])  # [1:]: not 16-byte aligned, the scalar path
    for max_norm in (0.0, 1.0, 1e6):
        stats = torch.zeros(3, device="cuda")
        K.norm_finish_(part, stats, max_norm)
        norm, sl, _ = O.finish_ref(pr, max_norm)
        accept("norm_finish", stats[:1], norm.reshape(1), F32, sl.reshape(1), note=f"np={np_} {view}")
        got = stats.cpu().double()
        # the clip coefficient from the norm the kernel stored: add, divide, min
        coef = min(1.0, max_norm / (got[0].item() + 1e-6)) if max_norm > 0 else 1.0
        assert abs(got[1].item() - coef) <= 3 * O.EPS32 * coef and got[2].item() == 0.0
        if max_norm == 0.0:
            assert got[1].item() == 1.0


@dtp
def test_grad_norm_and_flags(K, dt):
    n = 8 * (2048 * 256 + 300)  # past the 2048-block cap of the reduction
    x = (1e-3 * torch.randn(n, generator=O.gen(12))).to(dt)
    xc = x.cuda()
    stats = torch.zeros(3, device="cuda")
    K.grad_norm_(xc, stats, 1.0)
    s2 = torch.zeros(3, device="cuda")
    K.grad_norm_(xc, s2, 1.0)
    assert bits_equal(stats, s2)
    ref = x.double().pow(2).sum().sqrt()
    # per thread 2 * 8 * ceil(n8 / (2048 * 256)) operations, 6 + 4 in the block, then norm_finish_'s 2 + 6 + 16, sqrt
    k = 2 * 8 * 2 + 10 + 24 + 2
    accept("grad_norm", stats[:1], ref.reshape(1), F32, (k * O.EPS32 * ref).reshape(1))
    assert abs(stats[1].item() - min(1.0, 1.0 / (stats[0].item() + 1e-6))) <= 3 * O.EPS32
    assert stats[2].item() == 0.0
    for bad in (math.inf, math.nan):
        y = xc.clone()
        y[12345] = bad
        st = torch.zeros(3, device="cuda")
        K.grad_norm_(y, st, 1.0)
        assert st[2].item() == 1.0 and st[1].item() == 1.0
        K.grad_norm_(xc, st, 1.0)  # sticky: a later finite call leaves the flag set
        assert st[2].item() == 1.0 and st[0].item() == stats[0].item()
        st[2] = 0.0
        K.grad_norm_(xc, st, 1.0)
        assert st[2].item() == 0.0
    p, g, m, v = (t.cuda() for t in O.adamw_inputs(8 * 255, dt, F32))
    p0 = p.clone()
    K.adamw_(p, g, m, v, torch.tensor([1.0, 1.0, 1.0], device="cuda"), 1e-2, 0.9, 0.999, 1e-8, 0.1, 3)
    assert bits_equal(p, p0), "a set non-finite flag must skip the update"


# ---------------------------------------------------------------- AdamW
@pytest.mark.parametrize("n,max_blocks", O.ADAMW_SIZES)
@pytest.mark.parametrize("pdt,sdt", O.ADAMW_PAIRS, ids=lambda d: O.tag(d))
def test_adamw(K, pdt, sdt, n, max_blocks):
    p, g, m, v = O.adamw_inputs(n, pdt, sdt)
    hp = O.ADAMW_HP
    try:
        for step in O.ADAMW_STEPS:
            for wd in (0.0, 0.1):
                for coef in (1.0, 0.37):
                    ref = O.adamw_ref(p, g, m, v, coef, step, wd, **hp)
                    stats = torch.tensor([1.0, coef, 0.0], device="cuda")
                    for exact in (False, True):
                        K.set_exact_math(exact)
                        note = f"n={n} step={step} wd={wd} coef={coef} exact={exact}"
                        pc, mc, vc = p.cuda(), m.cuda(), v.cuda()
                        K.adamw_(pc, g.cuda(), mc, vc, stats, hp["lr"], hp["b1"], hp["b2"], hp["eps"], wd, step, max_blocks)
                        accept("adamw.p", pc, ref["p"][0], pdt, ref["p"][1], note=note)
                        accept("adamw.m", mc, ref["m"][0], sdt, ref["m"][1], note=note)
                        accept("adamw.v", vc, ref["v"][0], sdt, ref["v"][1], note=note)
                        assert torch.isfinite(pc.float()).all()
                        # the device hyper tensor [lr, 1/bc1, 1/sqrt(bc2)]: the bits of the host-argument call
                        hy = torch.from_numpy(O.adamw_hyper(hp["lr"], hp["b1"], hp["b2"], step)).cuda()
                        p2, m2, v2 = p.cuda(), m.cuda(), v.cuda()
                        K.adamw_(p2, g.cuda(), m2, v2, stats, 123.0, hp["b1"], hp["b2"], hp["eps"], wd, 7, max_blocks, hy)
                        assert bits_equal(p2, pc) and bits_equal(m2, mc) and bits_equal(v2, vc), f"hyper: {note}"
    finally:
        K.set_exact_math(False)


def test_zz_figures():
    """Prints what the criterion left unused, per kernel (run with -s)."""
    for name, (flips, worst) in sorted(O.FIGURES.items()):
        print(f"FIGURE {name:16s} non-RNE share {flips:.4%} (cap 2 %)   largest error / bound {worst:.3f}")
