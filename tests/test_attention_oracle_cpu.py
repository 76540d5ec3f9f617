"""The attention acceptance criterion (tests/attention_oracle.py), proved on the CPU.

(a) An honest torch-fp32 emulation of the kernels' scheme -- 64-key tiles with an online softmax, the
    rescale deferred until a row of the 32-row wave grows by more than 8 log2 units, P and dS rounded to the
    storage type, delta from the rounded o, 16-bit GQA partials, the backward fed the emulated forward's own
    o and lse -- is accepted against the fp64 reference on every input family at every shape of
    tests/test_flash_edges_gpu.py, in two summation orders (order 1: the key split's even / odd tile
    halves merged at the end, 16-key chunks in reverse, dQ per 128-key tile in reverse as the mode-0 atomics
    may land, dK / dV per 32-query slice in reverse, RoPE after the rounding instead of before it). The
    largest error / bound per output is kept in FIGURES and printed by test_zz_figures.
(b) Every wrong variant of MUTATIONS is rejected on the case named next to it.
The criterion is not measured on the code under test: nothing here runs a kernel.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import attention_oracle as A
from attention_oracle import BF16, F16, F32, LN2, LOG2E, judge, tag

FIGURES = {}  # (family of kernels, output) -> largest error / bound of the honest emulation


def rd(x, dt):
    return x if dt == F32 else x.to(dt).float()


def wave_any(need):
    """need [B,H,S] bool -> true for every row of a 32-row wave slice in which some row is true."""
    B, H, S = need.shape
    Sp = (S + 31) // 32 * 32
    w = F.pad(need, (0, Sp - S)).view(B, H, Sp // 32, 32).any(-1, keepdim=True)
    return w.expand(B, H, Sp // 32, 32).reshape(B, H, Sp)[..., :S]


def heads(q, k, v, mut=None):
    Hq, Hkv = q.shape[2], k.shape[2]
    G = Hq // Hkv
    idx = torch.arange(Hq) % Hkv if mut == "kv_mod" else torch.arange(Hq) // G
    return q.float().permute(0, 2, 1, 3), k.float().permute(0, 2, 1, 3)[:, idx], v.float().permute(0, 2, 1, 3)[:, idx]


def visible(B, S, ds, mut=None):
    pos = torch.arange(S)
    ds = torch.zeros(B, S, dtype=torch.long) if ds is None else ds.long()
    if mut == "ds+1":
        ds = torch.minimum(ds + 1, pos.view(1, S))
    if mut == "ds-1":
        ds = (ds - 1).clamp(min=0)
    i, j = pos.view(1, S, 1), pos.view(1, 1, S)
    causal = j <= i + 1 if mut == "causal+1" else (j < i if mut == "causal-1" else j <= i)
    vis = causal & (j >= ds.view(B, S, 1))
    if mut == "drop_last":
        vis[:, :, S - 1] = False
    return vis.view(B, 1, S, S)


def emu_fwd(q, k, v, dt, ds=None, order=0, mut=None):
    """-> o [B,S,Hq,D] in dt, lse [B,Hq,S] fp32 (log2 domain; natural for dt = fp32)."""
    B, S, Hq, D = q.shape
    f32k = dt == F32
    qh, kh, vh = heads(q, k, v, mut)
    cs = torch.tensor((1.0 if f32k else LOG2E) / (D if mut == "scale" else math.sqrt(D)), dtype=torch.float32)
    ex = torch.exp if f32k else torch.exp2
    thr = 0.0 if f32k else A.RESCALE_LOG2
    x = qh @ kh.transpose(-1, -2)
    vis = visible(B, S, ds, mut).expand(B, Hq, S, S)
    if mut in ("pad_key", "batch_leak"):
        # one more key column behind the ragged end, seen by the last two rows: the clamped copy of key
        # S - 1, or key 0 of the next batch row
        src = S - 1 if mut == "pad_key" else 0
        kx = (kh if mut == "pad_key" else kh.roll(-1, 0))[:, :, src:src + 1]
        vx = (vh if mut == "pad_key" else vh.roll(-1, 0))[:, :, src:src + 1]
        x = torch.cat([x, qh @ kx.transpose(-1, -2)], -1)
        vh = torch.cat([vh, vx], 2)
        extra = torch.zeros(B, Hq, S, 1, dtype=torch.bool)
        extra[:, :, max(S - 2, 0):] = True
        vis = torch.cat([vis, extra], -1)
    nk = x.shape[-1]
    ntile = (nk + 63) // 64

    def sweep(tiles):
        m = torch.full((B, Hq, S), -math.inf)
        l = torch.zeros(B, Hq, S)
        o = torch.zeros(B, Hq, S, D)
        skipped = False
        for t in tiles:
            k0, k1 = t * 64, min(t * 64 + 64, nk)
            vt = vis[..., k0:k1]
            st = x[..., k0:k1].masked_fill(~vt, -math.inf)
            cand = st.max(-1).values * cs
            need = wave_any(cand > m + thr) if not f32k else torch.ones_like(m, dtype=torch.bool)
            mn = torch.maximum(m, cand)
            alpha = torch.where(mn == -math.inf, torch.ones_like(m), ex(m - mn))
            alpha = torch.where(need, alpha, torch.ones_like(m))
            jump = bool((need & (m > -math.inf) & (alpha < 1)).any())
            m = torch.where(need, mn, m)
            l = l * alpha
            if mut == "skip_rescale" and jump and not skipped:
                skipped = True  # O keeps the old scale on this one tile
            else:
                o = o * alpha.unsqueeze(-1)
            if f32k:  # the score is scaled (and rounded) first, then m is subtracted
                p = ex(st * cs - m.unsqueeze(-1))
            else:  # one rounding: the fma
                p = ex((st.double() * cs.double() - m.unsqueeze(-1).double()).float())
            p = torch.where(vt & (m.unsqueeze(-1) > -math.inf), p, torch.zeros_like(p))
            pb = rd(p, dt)
            if order == 0:
                l = l + p.sum(-1)
                o = o + pb @ vh[:, :, k0:k1]
            else:
                l = l + p.flip(-1).sum(-1)
                for c0 in reversed(range(0, k1 - k0, 16)):
                    o = o + pb[..., c0:c0 + 16] @ vh[:, :, k0 + c0:min(k0 + c0 + 16, k1)]
        return m, l, o

    if order == 0:
        m, l, o = sweep(range(ntile))
    else:  # the key split: even and odd tiles with their own (m, l, O), merged at the common max
        m0, l0, o0 = sweep(range(0, ntile, 2))
        m1, l1, o1 = sweep(range(1, ntile, 2))
        m = torch.maximum(m0, m1)
        a0 = torch.where(m0 == -math.inf, torch.zeros_like(m), ex(m0 - m))
        a1 = torch.where(m1 == -math.inf, torch.zeros_like(m), ex(m1 - m))
        l = l0 * a0 + l1 * a1
        o = o0 * a0.unsqueeze(-1) + o1 * a1.unsqueeze(-1)
    out = rd(o * (1.0 / l).unsqueeze(-1), dt).to(dt).permute(0, 2, 1, 3).contiguous()
    lse = m + (torch.log(l) if f32k else torch.log2(l))
    if mut == "lse_nat":
        lse = lse * LN2
    if mut == "lse_no_l":
        lse = m
    return out, lse


def rope_back(x, cos, sin):
    B, S, H, D = x.shape
    c, s = cos[:S].view(1, S, 1, D // 2), sin[:S].view(1, S, 1, D // 2)
    a, b = x.view(B, S, H, D // 2, 2).unbind(-1)
    return torch.stack((a * c + b * s, -a * s + b * c), -1).reshape(B, S, H, D)


def emu_bwd(q, k, v, do, o, lse, dt, ds=None, de=None, order=0, mut=None, cos=None, sin=None):
    """-> dq [B,S,Hq,D], dk, dv [B,S,Hkv,D] in dt."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    G = Hq // Hkv
    f32k = dt == F32
    qh, kh, vh = heads(q, k, v)
    dh, oh = do.float().permute(0, 2, 1, 3), o.float().permute(0, 2, 1, 3)
    cs = torch.tensor((1.0 if f32k else LOG2E) / math.sqrt(D), dtype=torch.float32)
    scale = torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32)
    ex = torch.exp if f32k else torch.exp2
    vis = visible(B, S, ds, mut).expand(B, Hq, S, S)
    x = qh @ kh.transpose(-1, -2)
    if f32k:
        p = ex(x * cs - lse.unsqueeze(-1))
    else:
        p = ex((x.double() * cs.double() - lse.unsqueeze(-1).double()).float())
    p = torch.where(vis, p, torch.zeros_like(p))
    dP = dh @ vh.transpose(-1, -2)
    delta = (dh * oh).sum(-1, keepdim=True)
    if mut == "delta_nb":
        delta = delta.roll(1, 2)
    dS = p * (dP - delta)
    pb, dsb = rd(p, dt), rd(dS, dt)
    pos = torch.arange(S)
    # dQ
    dsq = dsb
    if mut == "dq_last_tile":
        dsq = dsb.masked_fill((pos >= 64 * ((S - 1) // 64)).view(1, 1, 1, S), 0.0)
    if order == 0:
        dq = (dsq @ kh) * scale
    else:
        dq = torch.zeros(B, Hq, S, D)
        for k0 in reversed(range(0, S, 128)):
            dq = dq + (dsq[..., k0:k0 + 128] @ kh[:, :, k0:k0 + 128]) * scale
    # dK / dV per q-head
    pk, dk_ = pb, dsb
    if mut == "dkdv_diag":
        same = (pos.view(S, 1) // 32 == pos.view(1, S) // 32).view(1, 1, S, S)
        pk, dk_ = pb.masked_fill(same, 0.0), dsb.masked_fill(same, 0.0)
    if mut == "de-1":  # the key-major sweep of key j ends one row early: query doc_end[j] - 1 is lost
        lost = (pos.view(1, S, 1) >= (de.long() - 1).view(B, 1, S)).view(B, 1, S, S)
        pk, dk_ = pb.masked_fill(lost, 0.0), dsb.masked_fill(lost, 0.0)
    if order == 0:
        dv_h, dk_h = pk.transpose(-1, -2) @ dh, dk_.transpose(-1, -2) @ qh
    else:
        dv_h, dk_h = torch.zeros(B, Hq, S, D), torch.zeros(B, Hq, S, D)
        for q0 in reversed(range(0, S, 32)):
            dv_h = dv_h + pk[:, :, q0:q0 + 32].transpose(-1, -2) @ dh[:, :, q0:q0 + 32]
            dk_h = dk_h + dk_[:, :, q0:q0 + 32].transpose(-1, -2) @ qh[:, :, q0:q0 + 32]
    if mut != "dk_noscale":
        dk_h = dk_h * scale

    def fold(xh):
        xs = xh.view(B, Hkv, G, S, D)
        if G > 1:
            xs = rd(xs, dt)  # the 16-bit partials
        if mut == "fold_drop" and G > 1:
            xs = xs[:, :, : G - 1]
        acc = torch.zeros(B, Hkv, S, D)
        for g_ in range(xs.shape[2]):
            acc = acc + xs[:, :, g_]
        return acc.permute(0, 2, 1, 3)

    dq, dk, dv = dq.permute(0, 2, 1, 3), fold(dk_h), fold(dv_h)
    if cos is not None:
        sn = -sin if mut == "rope_sin" else sin
        if order == 0:
            dq, dk = rope_back(dq.contiguous(), cos, sn), rope_back(dk.contiguous(), cos, sn)
        else:
            dq, dk = rope_back(rd(dq, dt).contiguous(), cos, sn), rope_back(rd(dk, dt).contiguous(), cos, sn)
    return tuple(rd(t, dt).to(dt).contiguous() for t in (dq, dk, dv))


# ---------------------------------------------------------------- (a) the honest emulation is accepted
def run_honest(fam, shape, dt, starts=None, rope=False, backward=True):
    B, S, Hq, Hkv, D = shape
    q, k, v, do = A.inputs(fam, shape, dt)
    ds, de = A.doc_bounds(starts, S) if starts is not None else (None, None)
    cos, sin = A.rope_tables(D, S) if rope else (None, None)
    ref = A.reference(q, k, v, do, dt, ds, cos, sin, backward)
    if dt == F16:  # the fp64 result itself stays inside fp16
        for name in ("o", "dq", "dk", "dv") if backward else ("o",):
            assert torch.isfinite(A.rne(ref[name][0], F16)).all(), (fam, shape, name)
    fk = "fp32" if dt == F32 else "16-bit"
    for order in (0, 1):
        o, lse = emu_fwd(q, k, v, dt, ds, order)
        got = {"o": o, "lse": lse}
        if backward:
            got["dq"], got["dk"], got["dv"] = emu_bwd(q, k, v, do, o, lse, dt, ds, de, order, None, cos, sin)
        for name, g in got.items():
            ver = judge(g, ref[name][0], F32 if name == "lse" else dt, ref[name][1])
            assert ver.ok, f"honest emulation (order {order}) rejected: {name} [{tag(dt)}] {fam} {shape}: {ver.why}"
            FIGURES[(fk, name)] = max(FIGURES.get((fk, name), 0.0), ver.worst)
        A.check_single_key_rows("emulation", o, lse, v, ref, dt, f"{fam} {shape}")


DT16 = (BF16, F16)
dt16 = pytest.mark.parametrize("dt", DT16, ids=tag)


@dt16
@pytest.mark.parametrize("shape", A.SEQ_SHAPES + A.HEAD_SHAPES + A.WAVE4_SHAPES, ids=str)
def test_honest_shapes(shape, dt):
    run_honest("randn", shape, dt, rope=shape[1] in (33, 129))


@dt16
@pytest.mark.parametrize("shape", A.FAMILY_SHAPES, ids=str)
def test_honest_families(shape, dt):
    for fam in A.families(dt):
        run_honest(fam, shape, dt)


@dt16
@pytest.mark.parametrize("case", list(A.DOC_CASES))
def test_honest_doc(case, dt):
    shape, starts = A.DOC_CASES[case]
    run_honest("randn", shape, dt, starts)
    if case.startswith("edges"):
        run_honest("kvoffset", shape, dt, starts, rope=True)


@pytest.mark.parametrize("shape", [s for s in A.SEQ_SHAPES + A.HEAD_SHAPES if s[1] <= 129], ids=str)
def test_honest_f32_shapes(shape):
    run_honest("randn", shape, F32)


@pytest.mark.parametrize("shape", [s for s in A.FAMILY_SHAPES if s[1] <= 129], ids=str)
def test_honest_f32_families(shape):
    for fam in A.FAMILIES:
        run_honest(fam, shape, F32)


@pytest.mark.parametrize("case", [c for c, (s, _) in A.DOC_CASES.items() if s[1] <= 129 and s[0] <= 3])
def test_honest_f32_doc(case):
    shape, starts = A.DOC_CASES[case]
    run_honest("randn", shape, F32, starts)


# ---------------------------------------------------------------- (b) mutations are rejected
EDGE_STARTS = A.DOC_CASES["edges64"][1]
# mutation -> (family, shape, document starts or None, RoPE, the outputs of which at least one must be rejected)
MUTATIONS = {
    "causal+1": ("randn", (3, 65, 4, 2, 64), None, False, ("o",)),           # key <= i + 1
    "causal-1": ("randn", (3, 65, 4, 2, 64), None, False, ("o",)),           # key < i
    "drop_last": ("randn", (3, 257, 4, 2, 64), None, False, ("o",)),         # last key of a ragged S dropped
    "pad_key": ("randn", (3, 257, 4, 2, 64), None, False, ("o",)),           # the padding key at index S included
    "batch_leak": ("kvoffset", (3, 129, 4, 2, 128), None, False, ("o",)),    # keys of batch row b + 1
    "kv_mod": ("kvoffset", (1, 33, 4, 2, 64), None, False, ("o",)),          # h % Hkv instead of h / rep
    "skip_rescale": ("late_peak", (1, 257, 4, 2, 128), None, False, ("o",)), # one tile's rescale skipped
    "lse_nat": ("randn", (3, 33, 4, 2, 64), None, False, ("lse",)),
    "lse_no_l": ("uniform", (2, 65, 4, 2, 64), None, False, ("lse",)),
    "scale": ("randn", (3, 129, 4, 2, 128), None, False, ("o",)),            # 1 / D
    "dk_noscale": ("randn", (3, 33, 4, 2, 64), None, False, ("dk",)),
    "dq_last_tile": ("randn", (3, 129, 4, 2, 64), None, False, ("dq",)),
    "dkdv_diag": ("randn", (3, 65, 4, 2, 128), None, False, ("dk", "dv")),
    "fold_drop": ("randn", (1, 33, 8, 1, 64), None, False, ("dk", "dv")),
    "delta_nb": ("randn", (3, 64, 4, 2, 64), None, False, ("dq", "dk")),
    "ds+1": ("randn", (3, 129, 4, 2, 64), EDGE_STARTS, False, ("o",)),
    "ds-1": ("kvoffset", (3, 129, 4, 2, 64), EDGE_STARTS, False, ("o",)),
    "de-1": ("randn", (3, 129, 4, 2, 64), EDGE_STARTS, False, ("dk", "dv")),
    "rope_sin": ("randn", (3, 33, 4, 2, 64), None, True, ("dq", "dk")),
}
FWD_MUT = {"causal+1", "causal-1", "drop_last", "pad_key", "batch_leak", "kv_mod", "skip_rescale", "lse_nat",
           "lse_no_l", "scale", "ds+1", "ds-1"}


# (the fp32 kernels rescale on every tile: nothing is deferred, so skip_rescale has no fp32 form)
@pytest.mark.parametrize("mut,dt", [(m, d) for m in MUTATIONS for d in (BF16, F16, F32)
                                    if not (d == F32 and m == "skip_rescale")],
                         ids=lambda x: x if isinstance(x, str) else tag(x))
def test_mutation_rejected(mut, dt):
    fam, shape, starts, rope, outs = MUTATIONS[mut]
    B, S, Hq, Hkv, D = shape
    q, k, v, do = A.inputs(fam, shape, dt)
    ds, de = A.doc_bounds(starts, S) if starts is not None else (None, None)
    cos, sin = A.rope_tables(D, S) if rope else (None, None)
    ref = A.reference(q, k, v, do, dt, ds, cos, sin)
    fwd = mut in FWD_MUT
    o, lse = emu_fwd(q, k, v, dt, ds, 0, mut if fwd else None)
    got = {"o": o, "lse": lse}
    if not fwd:
        got["dq"], got["dk"], got["dv"] = emu_bwd(q, k, v, do, o, lse, dt, ds, de, 0, mut, cos, sin)
    ver = {n: judge(got[n], ref[n][0], F32 if n == "lse" else dt, ref[n][1]) for n in outs}
    print(f"{mut} [{tag(dt)}] on {fam} {shape}" + (f" docs {starts}" if starts else "") + ": "
          + "; ".join(f"{n} error/bound {x.worst:.3g}" + ("" if x.ok else " REJECTED") for n, x in ver.items()))
    assert any(not x.ok for x in ver.values()), f"{mut} is accepted on {fam} {shape}"


def test_zz_figures():
    """Largest error / bound of the honest emulation per output (run after the tests above)."""
    for (fk, name), w in sorted(FIGURES.items()):
        print(f"emulation {fk:7s} {name:4s} {w:.3f}")
    assert all(w <= 1.0 for w in FIGURES.values())
