"""The flash attention kernels (csrc/kernels/flash_attn.hip, flash_f32.hip) held element by element to
fp64 references at their tile, mask and value edges (criterion, references and input families:
tests/attention_oracle.py; its CPU proof: tests/test_attention_oracle_cpu.py).

Every case builds its inputs and one fp64 reference (torch fp64 on the device), then runs every path:
  forward   key-split, pipelined, plain, flash_doc_fwd with one document (bitwise the plain kernel);
            each held to the oracle for o and lse2, rows that see one key bitwise v / the fp32 score,
            a second launch bitwise equal.
  backward  fed the kernel's own o and lse: mode 0, mode 1 with dq_split 0 / 1, kv_split 0 / 1 (head
            dim 64, 2-wave blocks), dkdv2 on / off (head dim 128), with RoPE tables (in-kernel and with
            flash_set_direct_rope(False)), flash_doc_bwd; dQ, dK, dV held to the fp64 gradient, a second
            launch bitwise equal wherever the path is deterministic.

Largest error / bound measured on an MI355X (printed by test_zz_figures), next to the same figure of the
CPU emulation of tests/test_attention_oracle_cpu.py; 332 cases, 9.2 s, every case passed on its first run
and no defect was found:

    output          MI355X   CPU emulation
    o  (forward)    0.806    0.806
    lse2            0.080    0.096
    dQ              0.555    0.555
    dK              0.587    0.543
    dV              0.948    0.948
    fp32 o / lse    0.072 / 0.175    0.179 / 0.300
    fp32 dQ/dK/dV   0.017 / 0.011 / 0.079    0.015 / 0.017 / 0.198

(Three figures are equal to three digits. Supposed, not verified: their worst element's error is one storage
rounding of P or dS on the same seeded inputs, which the emulation reproduces exactly.)
"""
from contextlib import contextmanager

import pytest
import torch

import attention_oracle as A
from attention_oracle import BF16, F16, F32, accept, bits_equal, tag

pytestmark = pytest.mark.gpu

DEFAULTS = dict(fwd_split=-1, fwd_pipe=1, dq_split=-1, kv_split=-1, dkdv2=True, direct_rope=True)


@pytest.fixture(scope="module")
def K():
    from fault_tolerant_llm_training_amd._native import kernels

    return kernels()


@contextmanager
def knobs(K, **kw):
    try:
        for name, val in kw.items():
            getattr(K, "flash_set_" + name)(val)
        yield
    finally:
        for name, val in DEFAULTS.items():
            getattr(K, "flash_set_" + name)(val)


def cuda(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


def cols(dqkv, shape):
    B, S, Hq, Hkv, D = shape
    a, b = Hq * D, (Hq + Hkv) * D
    return dqkv[:, :a].view(B, S, Hq, D), dqkv[:, a:b].view(B, S, Hkv, D), dqkv[:, b:].view(B, S, Hkv, D)


def hold_fwd(name, o, lse, v, ref, shape, dt, note):
    B, S, Hq, Hkv, D = shape
    accept(("f32_o." if dt == F32 else "o.") + name, o.view(B, S, Hq, D), ref["o"], dt, note)
    accept(("f32_lse." if dt == F32 else "lse2.") + name, lse[..., :S], ref["lse"], F32, note)
    A.check_single_key_rows(name, o.view(B, S, Hq, D), lse, v, ref, dt, note)


def hold_bwd(name, dqkv, ref, shape, dt, note):
    for key, got in zip(("dq", "dk", "dv"), cols(dqkv, shape)):
        accept(("f32_" if dt == F32 else "") + f"{key}.{name}", got, ref[key], dt, note)


def run16(K, fam, shape, dt, wide, starts=None, rope=True):
    """One case of the 16-bit kernels: every forward and backward path against one reference."""
    B, S, Hq, Hkv, D = shape
    note = f"{fam} {shape} {'wide' if wide else 'narrow'} qk" + (f" docs {starts}" if starts else "")
    q, k, v, do = cuda(*A.inputs(fam, shape, dt))
    qk, qkv, dout = A.pack(q.cpu(), k.cpu(), v.cpu(), do.cpu(), wide)
    qk, qkv, dout = (qkv.cuda(),) * 2 + (dout.cuda(),) if wide else cuda(qk, qkv, dout)
    doc = starts is not None
    ds, de = cuda(*A.doc_bounds(starts if doc else [[0]] * B, S))
    cos, sin = cuda(*A.rope_tables(D, S))
    ref = A.reference(q, k, v, do, dt, ds if doc else None)
    rref = dict(ref)
    rref["dq"] = A.rotate_back(*(t.contiguous() for t in ref["dq"]), cos, sin, A.U[dt])
    rref["dk"] = A.rotate_back(*(t.contiguous() for t in ref["dk"]), cos, sin, A.U[dt])
    if dt == F16:
        for n in ("o", "dq", "dk", "dv"):
            assert torch.isfinite(A.rne(ref[n][0], F16)).all(), (note, n)

    # ---- forward
    fwd = {}
    if not doc:
        for name, kn in (("split", dict(fwd_split=1)), ("pipe", dict(fwd_split=0, fwd_pipe=1)),
                         ("plain", dict(fwd_split=0, fwd_pipe=0))):
            with knobs(K, **kn):
                fwd[name] = K.flash_fwd(qk, qkv, S, Hq, Hkv, D)
                again = K.flash_fwd(qk, qkv, S, Hq, Hkv, D)
            assert bits_equal(fwd[name][0], again[0]) and bits_equal(fwd[name][1][..., :S], again[1][..., :S]), name
        o, lse = K.flash_fwd(qk, qkv, S, Hq, Hkv, D)  # the default route: what training feeds the backward
    fwd["doc"] = K.flash_doc_fwd(qk, qkv, ds, de, S, Hq, Hkv, D)
    again = K.flash_doc_fwd(qk, qkv, ds, de, S, Hq, Hkv, D)
    assert bits_equal(fwd["doc"][0], again[0]) and bits_equal(fwd["doc"][1][..., :S], again[1][..., :S])
    if doc:
        o, lse = fwd["doc"]
    else:  # one document: bitwise the plain unsplit, unpipelined kernel
        assert bits_equal(fwd["doc"][0], fwd["plain"][0]), note
        assert bits_equal(fwd["doc"][1][..., :S], fwd["plain"][1][..., :S]), note
    for name, (oo, ll) in fwd.items():
        hold_fwd(name, oo, ll, v, ref, shape, dt, note)

    # ---- backward, from the kernel's own o and lse
    def bwd(mode, cs=(None, None)):
        if doc or mode == "doc":
            return K.flash_doc_bwd(dout, qk, qkv, o, lse, ds, de, S, Hq, Hkv, D, *cs)
        return K.flash_bwd(dout, qk, qkv, o, lse, S, Hq, Hkv, D, mode, *cs)

    tabs = (cos, sin)
    paths = [("doc", "doc", {}, False)]
    if rope:
        paths.append(("doc_rope", "doc", {}, True))
    if not doc:
        nw2 = D == 64 and -(-S // 128) * B * Hq < 512
        paths += [("mode0", 0, {}, False), ("det", 1, {}, False), ("dq0", 1, dict(dq_split=0), False),
                  ("dq1", 1, dict(dq_split=1), False)]
        if nw2:
            paths += [("kv0", 1, dict(kv_split=0), False), ("kv1", 1, dict(kv_split=1), False)]
        if D == 128:
            paths.append(("dkdv2_off", 1, dict(dkdv2=False), False))
        if rope:
            paths += [("mode0_rope", 0, {}, True), ("det_rope", 1, {}, True),
                      ("rope_sep", 1, dict(direct_rope=False), True)]
            if D == 128:
                paths.append(("dkdv2_off_rope", 1, dict(dkdv2=False), True))
    nq = Hq * D
    for name, mode, kn, rot in paths:
        with knobs(K, **kn):
            g = bwd(mode, tabs if rot else (None, None))
            again = bwd(mode, tabs if rot else (None, None))
        hold_bwd(name, g, rref if rot else ref, shape, dt, note)
        if mode == 0:  # dQ by atomics: dK / dV are still reproducible
            assert bits_equal(g[:, nq:], again[:, nq:]), (name, note)
        else:
            assert bits_equal(g, again), (name, note)


dt16 = pytest.mark.parametrize("dt", (BF16, F16), ids=tag)


@dt16
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("shape", A.SEQ_SHAPES, ids=str)
def test_seq(K, shape, wide, dt):
    run16(K, "randn", shape, dt, wide, rope=shape[1] in (33, 65, 129))


@dt16
@pytest.mark.parametrize("i", range(len(A.HEAD_SHAPES)), ids=lambda i: str(A.HEAD_SHAPES[i]))
def test_heads(K, i, dt):
    run16(K, "kvoffset", A.HEAD_SHAPES[i], dt, wide=i % 2 == 1)


@pytest.mark.parametrize("shape", A.FAMILY_SHAPES, ids=str)
@pytest.mark.parametrize("fam,dt", [(f, d) for d in (BF16, F16) for f in A.families(d)],
                         ids=lambda x: x if isinstance(x, str) else tag(x))
def test_families(K, fam, dt, shape):
    run16(K, fam, shape, dt, wide=shape[4] == 128, rope=fam in ("randn", "hot_diag", "pm80"))


@dt16
@pytest.mark.parametrize("shape", A.WAVE4_SHAPES, ids=str)
def test_wave4(K, shape, dt):
    run16(K, "randn", shape, dt, wide=False)


@dt16
@pytest.mark.parametrize("case", list(A.DOC_CASES))
def test_doc(K, case, dt):
    shape, starts = A.DOC_CASES[case]
    run16(K, "kvoffset" if case.startswith("edges") else "randn", shape, dt, wide=case in ("small", "edges64"),
          starts=starts)


# ---------------------------------------------------------------- fp32 kernels
def run32(K, fam, shape, wide, starts=None):
    B, S, Hq, Hkv, D = shape
    note = f"{fam} {shape}" + (f" docs {starts}" if starts else "")
    q, k, v, do = cuda(*A.inputs(fam, shape, F32))
    qk, qkv, dout = A.pack(q.cpu(), k.cpu(), v.cpu(), do.cpu(), wide)
    qk, qkv, dout = (qkv.cuda(),) * 2 + (dout.cuda(),) if wide else cuda(qk, qkv, dout)
    doc = starts is not None
    ds, de = cuda(*A.doc_bounds(starts if doc else [[0]] * B, S))
    ref = A.reference(q, k, v, do, F32, ds if doc else None)
    runs = [("f32doc", lambda: K.flash_f32_doc_fwd(qk, qkv, ds, de, S, Hq, Hkv, D),
             lambda o, l: K.flash_f32_doc_bwd(dout, qk, qkv, o, l, ds, de, S, Hq, Hkv, D))]
    if not doc:
        runs.append(("f32", lambda: K.flash_f32_fwd(qk, qkv, S, Hq, Hkv, D),
                     lambda o, l: K.flash_f32_bwd(dout, qk, qkv, o, l, S, Hq, Hkv, D)))
    for name, f, b in runs:
        o, lse = f()
        o2, lse2 = f()
        assert bits_equal(o, o2) and bits_equal(lse, lse2), (name, note)
        hold_fwd(name, o, lse, v, ref, shape, F32, note)
        g = b(o, lse)
        assert bits_equal(g, b(o, lse)), (name, note)
        hold_bwd(name, g, ref, shape, F32, note)


@pytest.mark.parametrize("i", [i for i, s in enumerate(A.SEQ_SHAPES + A.HEAD_SHAPES) if s[1] <= 129],
                         ids=lambda i: str((A.SEQ_SHAPES + A.HEAD_SHAPES)[i]))
def test_f32_shapes(K, i):
    run32(K, "kvoffset", (A.SEQ_SHAPES + A.HEAD_SHAPES)[i], wide=i % 2 == 1)


@pytest.mark.parametrize("shape", [s for s in A.FAMILY_SHAPES if s[1] <= 129], ids=str)
@pytest.mark.parametrize("fam", A.FAMILIES)
def test_f32_families(K, fam, shape):
    run32(K, fam, shape, wide=False)


@pytest.mark.parametrize("case", [c for c, (s, _) in A.DOC_CASES.items() if s[1] <= 129 and s[0] <= 3])
def test_f32_doc(K, case):
    shape, starts = A.DOC_CASES[case]
    run32(K, "randn", shape, wide=False, starts=starts)


def test_zz_figures():
    """Largest accepted error / bound per output and path (run after the tests above)."""
    fam = {}
    for key, w in sorted(A.FIGURES.items()):
        print(f"{key:6s} {w:.3f}")
        fam[key] = w
    assert all(w <= 1.0 for w in fam.values())
