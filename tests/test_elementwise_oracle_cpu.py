"""The element-wise acceptance criterion (tests/elementwise_oracle.py), proved on the CPU.

(a) The same formulas evaluated in torch fp32 and rounded to the storage dtype are accepted against the
    fp64 references on exactly the inputs tests/test_elementwise_edges_gpu.py feeds the kernels: the
    inputs and every operation count k leave room for an honest fp32 kernel.
(b) A table of wrong evaluations, each of which the whole-tensor `rel` bounds of test_kernels_gpu.py /
    test_dtypes_gpu.py accept, is rejected on those inputs.
"""
import math

import numpy as np
import pytest
import torch

import elementwise_oracle as O
from elementwise_oracle import BF16, DTYPES, F16, F32, judge

f32 = np.float32


# ---------------------------------------------------------------- fp32 evaluations (mut: a wrong variant)
def norm_fwd_f32(x, d, w, dt, ln, mut=None):
    h = (x.float() + d.float()).to(dt) if d is not None else x
    xf, wf = h.float(), w.float()
    mu = xf.mean(-1, keepdim=True) if ln else torch.zeros(xf.shape[0], 1)
    xc = xf - mu
    var = xc.pow(2).mean(-1, keepdim=True)
    if mut == "var":
        var = xf.pow(2).mean(-1, keepdim=True) - mu * mu
    r = torch.rsqrt(var + (0.0 if mut == "eps" else O.NORM_EPS))
    y = (xc * r * wf).to(dt) if mut == "wfirst" else ((xc * r).to(dt).float() * wf).to(dt)
    if mut == "zero":
        y[-1] = 0
    if mut == "neighbour":
        y[-1] = y[-2]
    return h, dict(y=y, rstd=r.squeeze(-1), mean=mu.squeeze(-1))


def norm_verdicts(M, N, dt, ln, add, mut=None):
    x, d, w = O.norm_fwd_inputs(M, N, dt, ln, add)
    h, got = norm_fwd_f32(x, d, w, dt, ln, mut)
    ref = O.norm_fwd_ref(h, w, dt, ln)
    return {k: judge(got[k], ref[k][0], dt if k == "y" else F32, ref[k][1], ref[k][2])
            for k in (("y", "rstd", "mean") if ln else ("y", "rstd"))}


def norm_bwd_f32(inp, dt, ln, dres, acc):
    x, g, w = inp["x"].float(), inp["dy"].float(), inp["w"].float()
    r = inp["rstd"].unsqueeze(-1)
    mu = inp["mean"].unsqueeze(-1) if ln else 0.0
    n = (x - mu) * r
    dn = g * w
    dx = r * (dn - (dn.mean(-1, keepdim=True) if ln else 0.0) - n * (dn * n).mean(-1, keepdim=True))
    if dres:
        dx = dx + inp["dres"].float()
    dw = (g * n).sum(0) + (inp["dw0"].float() if acc else 0.0)
    return dx.to(dt), dw.to(dt)


def swiglu_f32(gu, da, dt, swap=False):
    F_ = gu.shape[-1] // 2
    g, u = gu[..., :F_].float(), gu[..., F_:].float()
    if swap:
        g, u = u, g
    s = 1.0 / (1.0 + torch.exp(-g))
    silu = g * s
    d = da.float()
    return (silu * u).to(dt), torch.cat([d * u * (s + silu * (1 - s)), d * silu], -1).to(dt)


def rope_f32(qkv, cos, sin, S, hq, hkv, d, neg=False):
    T, width = qkv.shape[0], (hq + hkv) * d
    x = qkv[:, :width].float().reshape(T, -1, d // 2, 2)
    pos = torch.arange(T) % S
    c, s = cos[pos].unsqueeze(1), sin[pos].unsqueeze(1) * (-1.0 if neg else 1.0)
    a, b = x[..., 0], x[..., 1]
    return torch.stack((a * c - b * s, a * s + b * c), -1).reshape(T, width).to(qkv.dtype)


def xent_f32(x, lab, drop=0):
    xf = x.float()
    lse = torch.logsumexp(xf[:, : xf.shape[1] - drop], -1)
    xy = xf.gather(1, lab.clamp(min=0).unsqueeze(1)).squeeze(1)
    return lse, torch.where(lab == O.IGNORE, torch.zeros_like(lse), lse - xy)


def xent_bwd_f32(x, lab, lse32, grad32, inv32):
    p = torch.exp(x.float() - lse32.unsqueeze(1))
    live = lab != O.IGNORE
    p[live, lab[live]] -= 1.0
    return (p * (grad32 * inv32) * live.unsqueeze(1)).to(x.dtype)


def adamw_f32(p, g, m, v, coef, step, wd, lr, b1, b2, eps, mut=None):
    if mut == "step":
        step += 1
    if mut == "lr":
        lr *= 2
    if mut == "wd":
        wd = 0.0
    if mut == "eps":
        eps = 1e-3
    h = O.adamw_hyper(lr, b1, b2, step)
    t = lambda s: torch.tensor(f32(s))
    gj = g.float() * t(1.0 if mut == "clip" else coef)
    pf = p.float() * (t(1.0) - t(h[0]) * t(wd))
    mf = m.float() + (gj - m.float()) * t(1.0 - b1)
    vf = v.float() * t(b2) + t(1.0 - b2) * gj * gj
    pf = pf - (t(h[0]) * t(h[1])) * mf / (vf.sqrt() * t(h[2]) + t(eps))
    return dict(p=p if mut == "p" else pf.to(p.dtype), m=mf.to(m.dtype), v=v if mut == "v" else vf.to(v.dtype))


def adamw_verdicts(n, pdt, sdt, step, wd, coef, mut=None):
    p, g, m, v = O.adamw_inputs(n, pdt, sdt)
    got = adamw_f32(p, g, m, v, coef, step, wd, mut=mut, **O.ADAMW_HP)
    ref = O.adamw_ref(p, g, m, v, coef, step, wd, **O.ADAMW_HP)
    return {k: judge(got[k], ref[k][0], pdt if k == "p" else sdt, ref[k][1]) for k in ("p", "m", "v")}


def ok(vs):
    bad = {k: v.why for k, v in vs.items() if not v.ok}
    assert not bad, bad


def rejected(vs):
    assert any(not v.ok for v in vs.values()), {k: (v.flips, v.worst) for k, v in vs.items()}


# ---------------------------------------------------------------- the criterion itself
def test_ulp_and_neighbours():
    x = torch.tensor([1.0, 1.5, 2.0 ** -126, 2.0 ** -133, 0.0, 3e38, 1.0 + 2.0 ** -8], dtype=torch.float64)
    assert O.ulp(x, BF16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -133, 2.0 ** -133, 2.0 ** -133, 2.0 ** 120, 2.0 ** -7]
    assert O.ulp(torch.tensor([1.0, 1e-7, 7e4], dtype=torch.float64), F16).tolist() == [2.0 ** -10, 2.0 ** -24, 2.0 ** 5]
    y = torch.tensor([1.001, -1.001, 1.0, 0.999, 1e-45, -1e-45], dtype=torch.float64)
    assert O.other_neighbour(y, BF16).double().tolist() == [1.0 + 2.0 ** -7, -1.0 - 2.0 ** -7, 1.0, 1.0 - 2.0 ** -8,
                                                         2.0 ** -133, -(2.0 ** -133)]


def test_judge_rules():
    r = torch.linspace(0.5, 2.0, 1000, dtype=torch.float64)
    exact = O.rne(r, BF16)
    assert judge(exact, r, BF16).ok and judge(exact, r, BF16).flips == 0
    one_off = exact.clone()
    one_off[:15] = O.other_neighbour(r, BF16)[:15]  # 1.5 %: neighbours, below the cap
    assert judge(one_off, r, BF16).ok
    one_off[:30] = O.other_neighbour(r, BF16)[:30]  # 3 %
    assert not judge(one_off, r, BF16).ok
    two = exact.clone()
    two[7] = two[7].double() + 3 * O.ulp(r, BF16)[7]
    assert not judge(two, r, BF16).ok
    assert judge(two, r, BF16, slack=3 * O.ulp(r, BF16)).ok  # a cancellation bound admits it
    nan = exact.clone()
    nan[3] = math.nan
    assert not judge(nan, r, BF16).ok
    inf = exact.clone()
    inf[3] = -math.inf
    assert not judge(inf, r, BF16).ok
    big = torch.tensor([7e4, -7e4], dtype=torch.float64)
    assert judge(torch.tensor([math.inf, -math.inf]).half(), big, F16).ok
    assert not judge(torch.tensor([-math.inf, math.inf]).half(), big, F16).ok
    tiny = torch.tensor([1e-39, 0.0], dtype=torch.float64)
    assert judge(torch.zeros(2), tiny, F32).ok  # below 2^-126: not part of the contract
    assert not judge(torch.tensor([1.0 + 2.0 ** -20]), torch.ones(1, dtype=torch.float64), F32,
                     slack=torch.full((1,), 4 * O.EPS32)).ok


# ---------------------------------------------------------------- (a) fp32 is accepted
@pytest.mark.parametrize("dt", DTYPES, ids=O.tag)
@pytest.mark.parametrize("ln", [False, True])
def test_fp32_norm_fwd_accepted(dt, ln):
    for N in O.NORM_FWD_N:
        for M in O.NORM_FWD_M:
            for add in (False, True):
                ok(norm_verdicts(M, N, dt, ln, add))


@pytest.mark.parametrize("dt", DTYPES, ids=O.tag)
@pytest.mark.parametrize("ln", [False, True])
def test_fp32_norm_bwd_accepted(dt, ln):
    for M, N in sorted(set(O.NORM_BWD_ONEWAVE + O.NORM_BWD_SPLIT + O.NORM_BWD_FALLBACK)):
        inp = O.norm_bwd_inputs(M, N, dt, ln)
        dx64, dxs, dw64, dws = O.norm_bwd_ref(inp, dt, ln)
        for dres in (False, True):
            for acc in (False, True):
                dx, dw = norm_bwd_f32(inp, dt, ln, dres, acc)
                a = inp["dres"].double() if dres else 0.0
                b = inp["dw0"].double() if acc else 0.0
                ok(dict(dx=judge(dx, dx64 + a, dt, dxs + O.EPS32 * (inp["dres"].double().abs() if dres else 0.0)),
                        dw=judge(dw, dw64 + b, dt, dws + O.EPS32 * (inp["dw0"].double().abs() if acc else 0.0))))


@pytest.mark.parametrize("dt", DTYPES, ids=O.tag)
def test_fp32_swiglu_accepted(dt):
    cases = [O.swiglu_inputs(dt, False), O.swiglu_inputs(dt, True)] + ([O.swiglu_stride_inputs()] if dt == BF16 else [])
    for gu, da in cases:
        a, dgu = swiglu_f32(gu, da, dt)
        ref = O.swiglu_ref(gu, da, dt)
        ok(dict(a=judge(a, ref["a"][0], dt, ref["a"][1]), dgu=judge(dgu, ref["dgu"][0], dt, ref["dgu"][1])))


@pytest.mark.parametrize("dt", DTYPES, ids=O.tag)
def test_fp32_rope_accepted(dt):
    for B, S, hq, hkv, d in O.ROPE_CASES:
        qkv, cos, sin = O.rope_inputs(B, S, hq, hkv, d, dt)
        for bwd in (False, True):
            ref, sl = O.rope_ref(qkv, cos, sin, S, hq, hkv, d, bwd)
            ok(dict(qk=judge(rope_f32(qkv, cos, sin, S, hq, hkv, d, neg=bwd), ref, dt, sl)))


@pytest.mark.parametrize("dt", DTYPES, ids=O.tag)
def test_fp32_xent_accepted(dt):
    for T, V in [(5, V) for V in O.XENT_V] + [(32769, 8)]:
        x, labs = O.xent_inputs(T, V, dt)
        for lab in labs:
            lse64, lses, loss64, losss = O.xent_ref(x, lab)
            lse, loss = xent_f32(x, lab)
            grad, inv = torch.tensor(2.0), torch.tensor(1.0 / max(1, int((lab != O.IGNORE).sum())))
            l32 = lse64.float()
            g64, gs = O.xent_bwd_ref(x, lab, l32, grad, inv)
            ok(dict(lse=judge(lse, lse64, F32, lses), loss=judge(loss, loss64, F32, losss),
                    grad=judge(xent_bwd_f32(x, lab, l32, grad, inv), g64, dt, gs)))


@pytest.mark.parametrize("pdt,sdt", O.ADAMW_PAIRS, ids=lambda d: O.tag(d))
def test_fp32_adamw_accepted(pdt, sdt):
    for n, _ in O.ADAMW_SIZES:
        for step in O.ADAMW_STEPS:
            for wd in (0.0, 0.1):
                for coef in (1.0, 0.37):
                    ok(adamw_verdicts(n, pdt, sdt, step, wd, coef))


@pytest.mark.parametrize("dt", DTYPES, ids=O.tag)
def test_fp32_sumsq_accepted(dt):
    x = torch.randn(8000, generator=O.gen(8)).to(dt)
    for nb in (1, 3, 4096):
        part, sl = O.sumsq_ref(x, nb)
        blk = (torch.arange(1000) % (nb * 256)) // 256
        got = torch.zeros(nb).index_add_(0, blk, x.float().reshape(-1, 8).pow(2).sum(-1))
        ok(dict(partial=judge(got, part, F32, sl)))
        norm, nsl, _ = O.finish_ref(got, 1.0)
        ok(dict(norm=judge(got.sum().sqrt().reshape(1), norm.reshape(1), F32, nsl.reshape(1))))


# ---------------------------------------------------------------- (b) the mutation table
@pytest.mark.parametrize("mut", ["p", "v", "wd", "step", "eps", "lr", "clip"])
@pytest.mark.parametrize("pdt,sdt", [(BF16, BF16), (F32, F32)], ids=lambda d: O.tag(d))
def test_adamw_mutation_rejected(mut, pdt, sdt):
    """bf16 / bf16 is the storage with the most room; step 3, wd 0.1, clip coefficient 0.37."""
    ok(adamw_verdicts(8 * 257, pdt, sdt, 3, 0.1, 0.37))
    rejected(adamw_verdicts(8 * 257, pdt, sdt, 3, 0.1, 0.37, mut))


NORM_MUTS = [("zero", False), ("neighbour", False), ("eps", False), ("zero", True), ("eps", True), ("var", True)]


# weight before the rounding: 16-bit only (fp32 has no intermediate rounding to reorder)
@pytest.mark.parametrize("mut,ln,dt", [(m, ln, dt) for m, ln in NORM_MUTS for dt in (BF16, F32)]
                         + [("wfirst", False, BF16), ("wfirst", False, F16), ("wfirst", True, BF16)],
                         ids=lambda a: O.tag(a) if isinstance(a, torch.dtype) else str(a))
def test_norm_mutation_rejected(mut, ln, dt):
    ok(norm_verdicts(9, 4104, dt, ln, False))
    rejected(norm_verdicts(9, 4104, dt, ln, False, mut))


def test_norm_one_lost_row_of_many_rejected():
    """The case the issue measured: one zeroed dx row of M = 2049 (rel 1.6e-2 under the old 2e-2 bound)."""
    inp = O.norm_bwd_inputs(2049, 1544, BF16, False)
    dx64, dxs, _, _ = O.norm_bwd_ref(inp, BF16, False)
    dx, _ = norm_bwd_f32(inp, BF16, False, False, False)
    assert judge(dx, dx64, BF16, dxs).ok
    dx[-1] = 0
    assert not judge(dx, dx64, BF16, dxs).ok


@pytest.mark.parametrize("dt", DTYPES, ids=O.tag)
def test_xent_mutation_rejected(dt):
    for V in (2056, 16392):
        x, labs = O.xent_inputs(5, V, dt)
        lse64, lses, loss64, losss = O.xent_ref(x, labs[0])
        lse, loss = xent_f32(x, labs[0], drop=8)
        assert not judge(lse, lse64, F32, lses).ok and not judge(loss, loss64, F32, losss).ok


@pytest.mark.parametrize("dt", DTYPES, ids=O.tag)
def test_swiglu_and_rope_mutations_rejected(dt):
    gu, da = O.swiglu_inputs(dt, True)
    ref = O.swiglu_ref(gu, da, dt)
    a, dgu = swiglu_f32(gu, da, dt, swap=True)
    assert not judge(a, ref["a"][0], dt, ref["a"][1]).ok and not judge(dgu, ref["dgu"][0], dt, ref["dgu"][1]).ok
    B, S, hq, hkv, d = O.ROPE_CASES[3]
    qkv, cos, sin = O.rope_inputs(B, S, hq, hkv, d, dt)
    r64, sl = O.rope_ref(qkv, cos, sin, S, hq, hkv, d)
    assert not judge(rope_f32(qkv, cos, sin, S, hq, hkv, d, neg=True), r64, dt, sl).ok
