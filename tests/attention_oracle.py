"""fp64 references, seeded inputs and the per-element acceptance criterion of the attention kernel tests.

A plain module shared by tests/test_attention_oracle_cpu.py (which proves on the CPU that the criterion
accepts an honest fp32 emulation of the kernels' scheme and rejects a table of wrong ones) and
tests/test_flash_edges_gpu.py (which holds csrc/kernels/flash_attn.hip and flash_f32.hip to it). Every
reference is the formula in fp64 on the stored inputs, with explicit gradient formulas (no autograd); none
calls the project's CPU paths. All functions work on whatever device their inputs are on.

Query i of a sequence sees key j iff doc_start[i] <= j <= i (doc_start = 0 without a document mask):
    s = q k^T / sqrt(D),  w = softmax_j(s),  o = w v,  lse = log sum_j exp(s)   (lse2 = lse * log2 e)
    dP = dO v^T,  delta = rowsum(dO * o),  dS = w (dP - delta)
    dQ = dS k / sqrt(D),  dK = sum_group dS^T q / sqrt(D),  dV = sum_group w^T dO
and, with RoPE tables, dQ / dK rotated back (pair (a, b) -> (a c + b s, -a s + b c)).

The criterion (`judge`): per element, nothing left out,
    16-bit output:  |got - ref64| <= ulp_dt(ref64) + slack        fp32 output:  |got - ref64| <= slack
NaN sets equal, every output finite where the reference is; differences below 2^-126 are ignored (fp32
denormal handling is not part of the contract). There is no flip share and no excluded element.

The slack is derived term by term from what the kernels round (`reference`, each term stated next to its
use). Constants, and where they come from:
    u            2^-8 (bf16) / 2^-11 (fp16) / 0 (fp32): one rounding to the storage type -- `cvt8` of P in
                 the forward, of P and dS in the three backward kernels, `cvt1` of the GQA partials.
    2^-25        fp16 only: an fp16 P or dS below 2^-14 is rounded to a subnormal, an absolute error of
                 half the subnormal spacing 2^-24 (the P of a row are >= 1 at the row maximum, so l >= 1).
    kD           terms of a score / dP dot product: D for the MFMA kernels (fp32 accumulation of D exact
                 products, order unknown), D/4 + 4 for the fp32 kernels (dot_part: D/4 fmas per lane,
                 quad_sum: 2 adds, the scale product, one spare).
    3 |x|        the softmax scale is LOG2E_F / sqrt((float)D) (run_fwd / run_bwd): the constant, the
                 square root and the quotient are one rounding each (fp32 kernels: 1 / sqrtf, and the product).
    2 (m - x)    fmaf(s, sl2, -m) rounds once at |x - m|; the factors exp2(m_old - m_new) of the later
                 rescales multiply O and l alike, so they act as one more relative error of the weight: their
                 exponents add up to at most m - x.
    RESCALE_LOG2 = 8: the deferred rescale leaves the running max up to 8 log2 units stale, so the exponent
                 that is rounded can be 8 larger (twice: the fma and the rescale factors); 0 for fp32.
    2 + 3 (nt+1) exp2 / expf itself (1 ulp = 2 half-ulps), and per key tile after the key's own (nt of
                 them, + 1 for the key-split merge) the rescale's exp2 (2) and product (1).
    acc(n)       n + 2 ceil(n / 64) + 8: fp32 accumulation of n summands (MFMA / fma chains, n roundings at
                 most), one rescale product and one row-sum add per tile, and 8 for the lane-half / split
                 merges, 1 / l, the final product and the scale. Used for O, l, dQ (also the mode-0 atomics:
                 at most 2 per 128-key tile, each one rounding of the running sum), dK and dV.
    D/2 + 4      delta: a lane adds D/2 products in sequence, one shuffle add (flash_bwd_dq_kernel; the
                 pre-kernel's chain of D/16 + 4 is shorter).
    lse2         (sum_j w_j eps_ij + acc(n) 2^-24) / ln 2   [the relative error of l through log2]
                 + 2^-24 (|lse2| + 2 (log2 n + RESCALE_LOG2 + 2))   [the final add; log2f at 1 ulp of its
                 result, which is at most log2 n + 8]. This is the kernel's chain, not k (|m| + log2 n + 1).
"""
import math
from dataclasses import dataclass

import torch

from elementwise_oracle import BF16, DTYPES, EPS32, F16, F32, TINY, gen, rne, tag, ulp  # noqa: F401

LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
RESCALE_LOG2 = 8.0
BN = 64  # key tile of the forward and dQ kernels
U = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 0.0}
SUB = {BF16: 0.0, F16: 2.0 ** -25, F32: 0.0}
F64 = torch.float64


# ---------------------------------------------------------------- shapes (B, S, Hq, Hkv, D)
SEQS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 257)
HEADS = ((2, 2), (4, 2), (4, 1), (8, 1))  # GQA groups of 1, 2, 4, 8
DIMS = (64, 128)
# every S at one head configuration per D; B = 3: a ragged last tile meets the next batch row
SEQ_SHAPES = [(3, S, 4, 2, D) for D in DIMS for S in SEQS]
# every head configuration at S in {33, 129}; B alternates 1 / 3
HEAD_SHAPES = [((1, 3)[(i + (S > 33)) % 2], S, hq, hkv, D) for D in DIMS for S in (33, 129)
               for i, (hq, hkv) in enumerate(HEADS)]
# every input family at S in {65, 257}
FAMILY_SHAPES = [(2, 65, 4, 2, D) for D in DIMS] + [(1, 257, 4, 2, D) for D in DIMS]
# the smallest grids with tiles * B * Hq >= 512: the 4-wave head-dim-64 backward kernels
WAVE4_SHAPES = [(16, 129, 16, 4, 64), (16, 129, 16, 16, 64)]

FAMILIES = ("randn", "hot_first", "hot_diag", "hot_tile_last", "hot_tile_next", "uniform", "late_peak",
            "early_peak", "ramp", "qzero", "pm80", "kvoffset")
# fp16: v and dO scaled by 2^+-12 (both up leaves fp16: dQ ~ 2^24)
FAMILIES_F16 = ("v_up", "v_down", "vdo_down")


def families(dt):
    return FAMILIES + (FAMILIES_F16 if dt == F16 else ())


def late_peak_at(S):
    return 64 if S <= 129 else 192


def inputs(fam, shape, dt):
    """Seeded (q [B,S,Hq,D], k, v [B,S,Hkv,D], do [B,S,Hq,D]) in dt, on the CPU.

    Scores are steered through a common direction: q += a in every column and k += b / sqrt(D) in
    every column give q . k / sqrt(D) += a b (natural units; 1.44 a b in log2 units)."""
    B, S, Hq, Hkv, D = shape
    g = gen(11, (FAMILIES + FAMILIES_F16).index(fam), B, S, Hq, Hkv, D, DTYPES.index(dt))
    q = torch.randn(B, S, Hq, D, generator=g)
    k = torch.randn(B, S, Hkv, D, generator=g)
    v = torch.randn(B, S, Hkv, D, generator=g)
    do = torch.randn(B, S, Hq, D, generator=g)
    pos = torch.arange(S, dtype=torch.float32).view(1, S, 1, 1)
    rd = math.sqrt(D)
    if fam.startswith("hot_"):
        # one key outscores the rest by 40 natural (57 log2) units
        q = 1.0 + 0.1 * q
        if fam == "hot_diag":
            k = (4.0 * pos).expand(B, S, Hkv, D).clone()  # exact in bf16 up to S = 257; 4 sqrt(D) per key
        else:
            j = {"hot_first": 0, "hot_tile_last": min(63, S - 1), "hot_tile_next": min(64, S - 1)}[fam]
            k = 0.1 * k
            k[:, j] += 40.0 / rd
    elif fam == "uniform":
        k = k[:, :1].expand(B, S, Hkv, D).clone()  # all scores of a row equal: o is the running mean of v
    elif fam == "late_peak":
        # low for one or three tiles, then 30 natural (43 log2) units up: far past RESCALE_LOG2
        q = 1.0 + 0.1 * q
        k = 0.1 * k + (pos >= late_peak_at(S)) * (30.0 / rd)
    elif fam == "early_peak":
        # the first 4 keys 150 natural (216 log2) units up: later keys underflow to 0 against the max
        q = 1.0 + 0.1 * q
        k = 0.1 * k + (pos < 4) * (150.0 / rd)
    elif fam == "ramp":
        # test_flash_fwd_growing_scores, slope 0.3: the running max moves by about RESCALE_LOG2 per tile
        u = torch.nn.functional.normalize(torch.randn(D, generator=g), dim=0)
        q = q + 4.0 * u
        k = 0.5 * k + 0.3 * pos * u
    elif fam == "qzero":
        q[:, ::3] = 0.0
    elif fam == "pm80":
        # scores near +-80 natural units, the sign by (row, key)
        a = math.sqrt(80.0)
        sq = torch.randint(0, 2, (B, S, Hq, 1), generator=g) * 2.0 - 1.0
        sk = torch.randint(0, 2, (B, S, Hkv, 1), generator=g) * 2.0 - 1.0
        q = 0.1 * q + a * sq
        k = 0.1 * k + a * sk / rd
    elif fam == "kvoffset":
        v = v + torch.arange(Hkv, dtype=torch.float32).view(1, 1, Hkv, 1)
    elif fam == "v_up":
        v, do = v * 2.0 ** 12, do * 2.0 ** -12
    elif fam == "v_down":
        v, do = v * 2.0 ** -12, do * 2.0 ** 12
    elif fam == "vdo_down":
        v, do = v * 2.0 ** -12, do * 2.0 ** -12
    else:
        assert fam == "randn", fam
    return q.to(dt), k.to(dt), v.to(dt), do.to(dt)


def pack(q, k, v, do, wide):
    """-> qk, qkv [T, .], do [T, Hq D]. wide: qk is the qkv buffer itself (Q / K rotated in place by the QKV
    projection's epilogue); narrow: qk is a buffer of its own and qkv's Q / K columns hold other values."""
    B, S, Hq, D = q.shape
    T = B * S
    qk = torch.cat([q.reshape(T, -1), k.reshape(T, -1)], 1).contiguous()
    if wide:
        qkv = torch.cat([qk, v.reshape(T, -1)], 1).contiguous()
        return qkv, qkv, do.reshape(T, -1).contiguous()
    junk = torch.randn(qk.shape, generator=gen(12, T, qk.shape[1])).to(qk.dtype)
    return qk, torch.cat([junk, v.reshape(T, -1)], 1).contiguous(), do.reshape(T, -1).contiguous()


def doc_bounds(starts, S):
    """starts: per batch row the sorted document starts (the first is 0) -> int32 (doc_start, doc_end) [B, S]."""
    ds = torch.zeros(len(starts), S, dtype=torch.int32)
    de = torch.full((len(starts), S), S, dtype=torch.int32)
    for b, st in enumerate(starts):
        st = sorted(st)
        assert st[0] == 0 and st[-1] < S
        for a, e in zip(st, st[1:] + [S]):
            ds[b, a:e] = a
            de[b, a:e] = e
    return ds, de


def _random_starts(S, seed, max_len):
    g = torch.Generator().manual_seed(seed)
    st, p = [0], 0
    while True:
        p += int(torch.randint(1, max_len, (1,), generator=g))
        if p >= S:
            return st
        st.append(p)


# The boundary placements of CASES in tests/test_flash_doc_gpu.py cut down to S <= 257, and: a boundary at
# every one of rows 31, 32, 33, 63, 64, 65; a one-token document at the very end; one at row 0.
DOC_CASES = {
    "inslice": ((1, 256, 2, 1, 128), [[0, 70, 200]]),
    "aligned_tiny": ((2, 257, 8, 2, 64), [[0, 64, 128, 192, 256], [0, 1, 2, 256]]),
    "ragged": ((1, 250, 4, 2, 128), [[0, 83, 84, 225]]),
    "small": ((3, 100, 4, 4, 64), [[0, 99], [0], [0, 31, 32, 33]]),
    "random_2wave": ((1, 257, 4, 4, 64), [_random_starts(257, 5, 40)]),
    "layer": ((1, 256, 8, 2, 128), [list(range(0, 256, 64))]),
    "wave4_gqa": ((16, 129, 16, 4, 64), [[0, 70, 128], [0, 64], [0, 33, 127], [0], [0, 70, 100], [0, 1, 2, 128],
                                         [0, 63, 64, 65], [0, 100]] * 2),
    "edges64": ((3, 129, 4, 2, 64), [[0, 31, 32, 33, 63, 64, 65], [0, 128], [0, 1]]),
    "edges128": ((3, 129, 2, 2, 128), [[0, 31, 32, 33, 63, 64, 65], [0, 128], [0, 1]]),
}


# ---------------------------------------------------------------- fp64 reference and slack
def rope_tables(D, S, theta=500000.0):
    """fp32 [S, D/2] cos / sin from the formula (angles in fp64, rounded once)."""
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=F64) / D))
    ang = torch.arange(S, dtype=F64).view(S, 1) * inv.view(1, -1)
    return ang.cos().to(F32).contiguous(), ang.sin().to(F32).contiguous()


def rotate_back(x, e, cos, sin, u):
    """x, e [B, S, H, D] fp64 (value, error bound) -> the RoPE backward of x and its bound. The direct
    dK store and the separate rope_bwd_ pass rotate the stored 16-bit value: one rounding (u) in front;
    then two products and one add (3 half-ulps over |a c| + |b s|)."""
    B, S, H, D = x.shape
    c = cos[:S].to(device=x.device, dtype=F64).view(1, S, 1, D // 2)
    s = sin[:S].to(device=x.device, dtype=F64).view(1, S, 1, D // 2)
    xa, xb = x.view(B, S, H, D // 2, 2).unbind(-1)
    e = e + u * (x.abs() + e)
    ea, eb = e.view(B, S, H, D // 2, 2).unbind(-1)
    out = torch.stack((xa * c + xb * s, -xa * s + xb * c), -1).reshape(B, S, H, D)
    mag = torch.stack(((xa * c).abs() + (xb * s).abs(), (xa * s).abs() + (xb * c).abs()), -1)
    err = torch.stack((ea * c.abs() + eb * s.abs(), ea * s.abs() + eb * c.abs()), -1) + 3 * EPS32 * mag
    return out, err.reshape(B, S, H, D)


def acc(n):
    return n + 2 * torch.ceil(n / BN) + 8


def reference(q, k, v, do, dt, doc_start=None, cos=None, sin=None, backward=True):
    """q, do [B,S,Hq,D], k, v [B,S,Hkv,D] (any float dtype: the stored inputs). dt: the kernels' storage
    type (F32: the flash_f32 kernels, natural-log lse). Returns {name: (ref64, slack)} for o, dq [B,S,Hq,D],
    dk, dv [B,S,Hkv,D], lse [B,Hq,S] (log2 domain for 16-bit dt), and 'score': the scaled score of each
    row's diagonal key in the lse's unit with the slack of the dot product and the scale alone (what lse is
    for a row that sees one key), 'one': bool [B,S], the rows that see exactly one key."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    G = Hq // Hkv
    dev = q.device
    f32k = dt == F32
    u, sub = U[dt], SUB[dt]
    c = 1.0 if f32k else LOG2E          # natural units -> the kernel's exponent unit
    nat = 1.0 if f32k else LN2          # an error of the exponent (kernel unit) -> relative error
    kD = D / 4 + 4 if f32k else D
    R = 0.0 if f32k else RESCALE_LOG2
    scale = 1.0 / math.sqrt(D)

    qh = q.to(F64).permute(0, 2, 1, 3)
    kh = k.to(F64).permute(0, 2, 1, 3).repeat_interleave(G, 1)
    vh = v.to(F64).permute(0, 2, 1, 3).repeat_interleave(G, 1)
    pos = torch.arange(S, device=dev)
    ds = torch.zeros(B, S, dtype=torch.long, device=dev) if doc_start is None else doc_start.to(dev).long()
    vis = ((pos.view(1, 1, S) <= pos.view(1, S, 1)) & (pos.view(1, 1, S) >= ds.view(B, S, 1))).view(B, 1, S, S)
    visf = vis.to(F64)
    n = visf.sum(-1)                                       # [B,1,S] visible keys
    nt = torch.ceil((pos.view(1, 1, S) + 1) / BN)          # key tiles up to the diagonal

    s = (qh @ kh.transpose(-1, -2)) * scale                # natural units
    A = (qh.abs() @ kh.abs().transpose(-1, -2)) * scale    # sum |q_d k_d| / sqrt(D)
    sm = s.masked_fill(~vis, -math.inf)
    m = sm.max(-1, keepdim=True).values
    p = torch.exp(sm - m)
    l = p.sum(-1, keepdim=True)
    w = p / l
    lse = (m + l.log()).squeeze(-1)                        # natural
    o = w @ vh
    x, mx, L = s * c, m * c, lse * c                       # kernel units

    # relative error of one softmax weight (before its rounding to the storage type); see the module docstring
    arg = EPS32 * (kD * c * A + 3 * x.abs() + 2 * (mx - x).clamp(min=0) + 2 * R)
    eps = (nat * arg + EPS32 * (2 + 3 * (nt.unsqueeze(-1) + 1))) * visf
    we = w * eps
    wes = we.sum(-1, keepdim=True)
    wv = w @ vh.abs()
    an = acc(n).unsqueeze(-1)
    o_slack = (u * wv                                      # P rounded to the storage type before the PV product
               + we @ vh.abs() + o.abs() * wes             # the weights' fp32 error, in the numerator and in l
               + 2 * an * EPS32 * wv                       # fp32 accumulation of O and of l
               + 4 * EPS32 * o.abs()                       # 1 / l and the final product
               + sub * (visf @ vh.abs()))                  # fp16: subnormal P
    ln_n = torch.log2(n) if not f32k else torch.log(n)
    lse_slack = ((wes.squeeze(-1) + acc(n) * EPS32) / nat + EPS32 * (L.abs() + 2 * (ln_n + R + 2)))
    diag = torch.arange(S, device=dev)
    score = x[:, :, diag, diag]
    score_slack = EPS32 * (kD * c * A[:, :, diag, diag] + 5 * score.abs())  # dot product; scale (3), product, m
    out = {"o": (o.permute(0, 2, 1, 3), o_slack.permute(0, 2, 1, 3)), "lse": (L, lse_slack),
           "score": (score, score_slack), "one": (ds == pos.view(1, S))}
    if not backward:
        return out

    dh = do.to(F64).permute(0, 2, 1, 3)
    # delta from the stored o: the forward's own bound on it, through sum_d |dO_d|; then its fp32 chain
    e_o = o_slack + (ulp(o, dt) if not f32k else 0.0)
    delta = (dh * o).sum(-1, keepdim=True)
    d_delta = (dh.abs() * e_o).sum(-1, keepdim=True) + (D / 2 + 4) * EPS32 * (dh * o).abs().sum(-1, keepdim=True)
    dP = dh @ vh.transpose(-1, -2)
    AdP = dh.abs() @ vh.abs().transpose(-1, -2)
    # P = exp2(x - lse2) from the kernel's own lse2 (within lse_slack): relative error of the fp32 P
    etaP = nat * (lse_slack.unsqueeze(-1) + EPS32 * (kD * c * A + 3 * x.abs() + (x - L.unsqueeze(-1)).abs())) + 2 * EPS32
    dS = w * (dP - delta)
    # dS = P (dP - delta) in fp32: P's error, dP's accumulation, delta's error, the subtraction and product
    e_dS = w * (etaP * (dP - delta).abs() + kD * EPS32 * AdP + d_delta + 2 * EPS32 * (dP.abs() + delta.abs()))
    e_dS = e_dS + u * (dS.abs() + e_dS) + sub * visf       # dS rounded before the dK and dQ products
    e_P = w * etaP
    e_P = e_P + u * (w + e_P) + sub * visf                 # P rounded before the dV product
    del etaP, AdP, arg, eps, we

    dq = (dS @ kh) * scale
    dq_slack = scale * (e_dS @ kh.abs() + an * EPS32 * (dS.abs() @ kh.abs())) + 2 * EPS32 * dq.abs()
    nq = (S - pos).to(F64).view(1, 1, S, 1)                # queries at or behind the key
    aq = acc(nq)
    wT, dST = w.transpose(-1, -2), dS.transpose(-1, -2)
    dv_h = wT @ dh
    dv_hs = e_P.transpose(-1, -2) @ dh.abs() + aq * EPS32 * (wT @ dh.abs())
    dk_h = (dST @ qh) * scale
    dk_hs = scale * (e_dS.transpose(-1, -2) @ qh.abs() + aq * EPS32 * (dST.abs() @ qh.abs())) + 2 * EPS32 * dk_h.abs()

    def fold(x_h, e_h):
        xs = x_h.view(B, Hkv, G, S, D)
        es = e_h.view(B, Hkv, G, S, D)
        e = es.sum(2)
        if G > 1:  # per-q-head partials rounded to 16 bits, then G fp32 adds in the finalize pass
            e = e + u * (xs.abs() + es).sum(2) + G * EPS32 * xs.abs().sum(2)
        return xs.sum(2).permute(0, 2, 1, 3), e.permute(0, 2, 1, 3)

    dk, dk_slack = fold(dk_h, dk_hs)
    dv, dv_slack = fold(dv_h, dv_hs)
    dq, dq_slack = dq.permute(0, 2, 1, 3), dq_slack.permute(0, 2, 1, 3)
    if cos is not None:
        dq, dq_slack = rotate_back(dq.contiguous(), dq_slack.contiguous(), cos, sin, u)
        dk, dk_slack = rotate_back(dk.contiguous(), dk_slack.contiguous(), cos, sin, u)
    out.update(dq=(dq, dq_slack), dk=(dk, dk_slack), dv=(dv, dv_slack))
    return out


# ---------------------------------------------------------------- the criterion
@dataclass
class Verdict:
    ok: bool
    why: str
    worst: float  # largest error in units of the bound


FIGURES = {}  # output name -> largest accepted error / bound; filled by accept()


def judge(got, ref64, dt, slack):
    g = got.detach().to(device=ref64.device, dtype=F64).reshape(-1)
    r = ref64.reshape(-1)
    assert g.numel() == r.numel(), (got.shape, ref64.shape)
    sl = slack.expand_as(ref64).reshape(-1)
    why = []
    if not torch.equal(g.isnan(), r.isnan()):
        why.append(f"NaN sets differ ({int(g.isnan().sum())} got, {int(r.isnan().sum())} expected)")
    fin = torch.isfinite(r)
    if not bool(torch.isfinite(g[fin]).all()):
        why.append(f"{int((~torch.isfinite(g[fin])).sum())} elements not finite where the reference is")
    both = fin & torch.isfinite(g)
    z = torch.zeros_like(r)
    err = torch.where(both, (g - r).abs(), z)
    bound = torch.where(both, sl, z) + (ulp(torch.where(both, r, z), dt) if dt != F32 else 0.0)
    ratio = torch.where(err < TINY, z, err / bound.clamp(min=1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        i = int(ratio.argmax())
        why.append(f"{int((ratio > 1).sum())} of {g.numel()} elements beyond the bound; worst at flat index {i}: "
                   f"got {g[i].item():.9g}, fp64 {r[i].item():.9g}, error/bound {worst:.3g}")
    return Verdict(not why, "; ".join(why), worst)


def accept(name, got, ref, dt, note=""):
    """ref: (ref64, slack). Records the figure under the part of `name` before the first dot."""
    v = judge(got, ref[0], dt, ref[1])
    key = name.split(".")[0]
    if v.worst <= 1.0:
        FIGURES[key] = max(FIGURES.get(key, 0.0), v.worst)
    assert v.ok, f"{name} [{tag(dt)}] {note}: {v.why}"
    return v


def bits_equal(a, b):
    a, b = a.detach().contiguous(), b.detach().to(a.device).contiguous()
    it = torch.int32 if a.dtype == F32 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it))


def check_single_key_rows(name, o, lse, v, ref, dt, note=""):
    """Rows that see exactly one key (row 0 of every sequence and document, one-token documents):
    o[i] == v[i] bitwise (P is 1 after its rounding, l is within 2^-17 of 1, and v (1 +- 2^-17) rounds
    back to v), and lse is the fp32 score: the dot product's and the scale's roundings, nothing else.
    o [B,S,Hq,D], lse [B,Hq,>=S], v [B,S,Hkv,D]."""
    one = ref["one"].to(o.device)
    B, S, Hq, D = o.shape
    G = Hq // v.shape[2]
    vq = v.to(o.device).repeat_interleave(G, 2)
    assert bits_equal(o[one], vq[one]), f"{name} [{tag(dt)}] {note}: a row that sees one key is not that key's v"
    sc, ss = ref["score"]
    oh = one.view(B, 1, S).expand(B, Hq, S).to(sc.device)
    err = (lse[..., :S].to(device=sc.device, dtype=F64) - sc).abs()[oh]
    bad = err > ss[oh]
    assert not bool(bad.any()), (f"{name} [{tag(dt)}] {note}: lse of {int(bad.sum())} one-key rows is not the fp32 "
                                 f"score (worst error / bound {float((err / ss[oh].clamp(min=1e-300)).max()):.3g})")
