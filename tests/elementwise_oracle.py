"""fp64 references, seeded inputs and the acceptance criterion of the element-wise kernel tests.

A plain module shared by tests/test_elementwise_oracle_cpu.py (which proves on the CPU that the
criterion accepts an honest fp32 evaluation and rejects a table of wrong ones) and
tests/test_elementwise_edges_gpu.py (which holds the HIP kernels to it). Every reference is the
operation's formula in fp64 on the stored inputs; none calls the project's CPU paths.

The criterion (`judge`):
  * 16-bit outputs: every finite element within one storage ulp of the fp64 result, at most 2 % of
    the elements different from RNE_dt(fp64 result) (the flip rate test_exact_math_switch accepts: a
    cap, not a measurement), NaN sets equal, infinities equal in sign.
  * cancellation outputs: the bound gains `slack` = k * 2^-24 * sum|summands| (evaluated in fp64), k
    the kernel's operation count along its longest chain; each k is derived next to its use below.
    An element whose fp64 result is within that slack of a rounding tie is not counted as a flip.
  * fp32 outputs: the slack alone.
  * differences below 2^-126 are ignored (fp32 denormal handling is not part of the contract).
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

EPS32 = 2.0 ** -24  # half an fp32 ulp, relative: the error of one correctly rounded fp32 operation
TINY = 2.0 ** -126
FLIP_CAP = 0.02
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = (BF16, F16, F32)
_FMT = {BF16: (7, -126, 127), F16: (10, -14, 15)}  # mantissa bits, min / max normal exponent


def tag(dt):
    return {BF16: "bf16", F16: "fp16", F32: "fp32"}[dt]


def gen(*seed):
    return torch.Generator().manual_seed(hash(tuple(int(s) for s in seed)) & 0x7FFFFFFF)


def rne(x64, dt):
    """fp64 -> dt by round-to-nearest-even (through fp32: a second rounding only moves values within
    2^-29 of a tie, which at worst counts one element towards the flip share)."""
    return x64.to(F32).to(dt)


def ulp(x64, dt):
    """Spacing of dt at |x64|, floored at the spacing of the smallest normal."""
    mant, emin, emax = _FMT[dt]
    a = torch.nan_to_num(x64.abs(), nan=0.0, posinf=0.0)
    _, e = torch.frexp(a)
    e = torch.where(a == 0, torch.full_like(e, emin), e - 1).clamp(emin, emax)
    return torch.exp2(e.to(torch.float64) - mant)


def other_neighbour(x64, dt):
    """The dt value bracketing x64 on the other side of rne(x64, dt) (rne itself where exact)."""
    r = rne(x64, dt)
    r64 = r.to(torch.float64)
    bits = r.view(torch.int16).to(torch.int32)
    mag = bits & 0x7FFF
    neg = (bits & 0x8000) != 0
    away = (x64.abs() > r64.abs()) | ((r64 == 0) & (x64 != 0))
    mag2 = torch.where(away, mag + 1, (mag - 1).clamp(min=0))
    # stepping off zero takes the sign of x64
    neg = torch.where(r64 == 0, x64 < 0, neg)
    out = mag2 | (neg.to(torch.int32) << 15)
    out = torch.where(out >= 0x8000, out - 0x10000, out).to(torch.int16).view(dt)
    return torch.where(x64 == r64, r, out)


@dataclass
class Verdict:
    ok: bool
    why: str
    flips: float  # share of finite elements that differ from RNE_dt(ref64)
    worst: float  # largest error in units of the bound


FIGURES = {}  # kernel name -> [largest flip share, largest error / bound]; filled by accept()


def judge(got, ref64, dt, slack=None, alts=()):
    """`ref64`: the fp64 result (the one RNE is taken of); `alts`: further fp64 results an element may
    be a neighbour of instead (the norm's two-step rounding). `slack`: fp64 tensor or None."""
    g = got.detach().cpu().to(torch.float64).reshape(-1)
    refs = [r.reshape(-1).to(torch.float64) for r in (ref64,) + tuple(alts)]
    r0 = refs[0]
    assert g.numel() == r0.numel(), (g.shape, r0.shape)
    sl = torch.zeros_like(r0) if slack is None else slack.to(torch.float64).expand_as(ref64).reshape(-1)
    target = rne(r0, dt).to(torch.float64)
    why = []
    if not torch.equal(g.isnan(), r0.isnan()):
        why.append(f"NaN sets differ ({int(g.isnan().sum())} got, {int(r0.isnan().sum())} expected)")
    if not (torch.equal(g == math.inf, target == math.inf) and torch.equal(g == -math.inf, target == -math.inf)):
        why.append("infinities differ")
    fin = torch.isfinite(g) & torch.isfinite(target)
    if not bool(fin.any()):
        return Verdict(not why, "; ".join(why), 0.0, 0.0)
    ratio = None
    for r in refs:
        r = torch.where(fin, r, torch.zeros_like(r))
        err = (torch.where(fin, g, torch.zeros_like(g)) - r).abs()
        bound = torch.where(fin, sl, torch.zeros_like(sl)) + (ulp(r, dt) if dt in _FMT else 0.0)
        q = torch.where(err < TINY, torch.zeros_like(err), err / bound.clamp(min=1e-300))
        ratio = q if ratio is None else torch.minimum(ratio, q)
    ratio = torch.where(fin, ratio, torch.zeros_like(ratio))
    worst = float(ratio.max())
    if worst > 1.0:
        i = int(ratio.argmax())
        why.append(f"{int((ratio > 1).sum())} of {g.numel()} elements beyond the bound; worst at flat index {i}: "
                   f"got {g[i].item():.9g}, fp64 {r0[i].item():.9g}, error/bound {worst:.3g}")
    flips = 0.0
    if dt in _FMT:
        # an element whose fp64 result lies within its cancellation slack of a rounding tie has no
        # determined RNE at fp32 accuracy: it is held to the bound above, not counted as a flip
        t = torch.where(fin, target, torch.zeros_like(target))
        to_tie = 0.5 * ulp(t, dt) - (torch.where(fin, r0, torch.zeros_like(r0)) - t).abs()
        diff = fin & (g != target) & ((g - target).abs() >= TINY) & (to_tie > sl)
        flips = float(diff.sum()) / float(fin.sum())
        if flips > FLIP_CAP:
            why.append(f"{flips:.2%} of the elements differ from RNE (cap {FLIP_CAP:.0%})")
    return Verdict(not why, "; ".join(why), flips, worst)


def accept(name, got, ref64, dt, slack=None, alts=(), note=""):
    v = judge(got, ref64, dt, slack, alts)
    f = FIGURES.setdefault(name.split(".")[0], [0.0, 0.0])
    f[0], f[1] = max(f[0], v.flips), max(f[1], v.worst if v.worst <= 1.0 else f[1])
    assert v.ok, f"{name} [{tag(dt)}] {note}: {v.why}"
    return v


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    it = torch.int32 if a.dtype == F32 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it))


# ---------------------------------------------------------------- norm
NORM_EPS = 1e-5
NORM_FWD_N = (8, 512, 520, 1032, 2048, 2056, 4096, 4104, 8192)
NORM_FWD_M = (1, 4, 5, 9)
NORM_BWD_ONEWAVE = [(M, N) for N in (8, 520, 1032, 4104, 8192) for M in (1, 9, 17)]
NORM_BWD_SPLIT = [(M, N) for N in (1544, 2048, 2056, 3592, 4096) for M in (1, 5)] + [(1025, 1544), (2049, 1544)]
NORM_BWD_FALLBACK = [(M, N) for N in (1544, 2048, 2056, 3592, 4096) for M in (5, 17)]


def norm_k(N):
    """Row reduction: a lane adds 8 * CH values in sequence (CH = the kernel's chunk-count
    instantiation, 512 columns each), then 6 shuffle levels, then divide, add eps, rsqrt, multiply."""
    ch = next(c for c in (1, 2, 4, 8, 16) if c >= (N + 511) // 512)
    return 8 * ch + 6 + 4


def big_scale(dt):
    # 2^+-30 where the format holds it; fp16 (max 65504, smallest subnormal 2^-24) takes 2^+-12
    return 12 if dt == F16 else 30


def norm_rows(M, N, dt, g, ln):
    """Value rows by row index: 0 plain, 1 all zero, 2 / 3 scaled by 2^+-30, 4 mean 100 with unit spread,
    5 one huge element; with a single row, plain."""
    x = torch.randn(M, N, generator=g)
    d = 0.5 * torch.randn(M, N, generator=g)
    for r in range(M):
        k = r % 6
        if k == 1:
            x[r], d[r] = 0.0, 0.0
        elif k in (2, 3):
            s = 2.0 ** (big_scale(dt) if k == 2 else -big_scale(dt))
            x[r] *= s
            d[r] *= s
        elif k == 4:
            x[r] += 100.0
        elif k == 5:
            x[r, (7 * r) % N] = 1e4
    return x.to(dt), d.to(dt)


def norm_fwd_inputs(M, N, dt, ln, add):
    g = gen(1, M, N, DTYPES.index(dt), ln, add)
    x, d = norm_rows(M, N, dt, g, ln)
    w = (1 + 0.1 * torch.randn(N, generator=g)).to(dt)
    return x, (d if add else None), w


def norm_fwd_ref(h, w, dt, ln, eps=NORM_EPS):
    """h: the (added) input in dt. Returns {name: (ref64, slack, alts)} for y, rstd, mean."""
    N = h.shape[-1]
    K = norm_k(N)
    x = h.to(torch.float64)
    w64 = w.to(torch.float64)
    mu = x.mean(-1, keepdim=True) if ln else torch.zeros(x.shape[0], 1, dtype=torch.float64)
    # the mean is a K-operation sum of N terms divided by N: |error| <= K 2^-24 mean|x|
    dmu = K * EPS32 * x.abs().mean(-1, keepdim=True) if ln else torch.zeros_like(mu)
    xc = x - mu
    rstd = (xc.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    # sum of squares: K operations plus the subtraction and the square per term, halved by the
    # square root, plus rsqrt itself: (K + 4) 2^-24 relative. An error dmu of the mean adds N dmu^2
    # to the sum of squares (the first-order term sums to zero): 0.5 rstd^3 dmu^2.
    rstd_slack = rstd * (K + 4) * EPS32 + 0.5 * rstd.pow(3) * dmu.pow(2)
    n = xc * rstd
    # (x - mu) * rstd: the error of mu enters in full (a cancellation for LayerNorm), the rest is relative
    n_slack = rstd * dmu + n.abs() * (K + 6) * EPS32
    out = {"rstd": (rstd.squeeze(-1), rstd_slack.squeeze(-1), ()), "mean": (mu.squeeze(-1), dmu.squeeze(-1), ())}
    if dt in _FMT:
        # documented order: round the normalised value to dt, then multiply by the weight. The fp32
        # value being rounded may sit on the other side of a tie: its other neighbour is accepted
        # (and counts towards the flip share); the product of two dt values is exact in fp32.
        y0 = rne(n, dt).to(torch.float64) * w64
        y1 = other_neighbour(n, dt).to(torch.float64) * w64
        out["y"] = (y0, (w64.abs() * rstd * dmu) if ln else None, (y1,))
    else:
        out["y"] = (n * w64, w64.abs() * n_slack, ())
    return out


def norm_bwd_inputs(M, N, dt, ln):
    g = gen(2, M, N, DTYPES.index(dt), ln)
    x = torch.randn(M, N, generator=g)
    if ln:
        x[2::5] += 100.0
    x = x.to(dt)
    dy = torch.randn(M, N, generator=g).to(dt)
    dres = torch.randn(M, N, generator=g).to(dt)
    w = (1 + 0.1 * torch.randn(N, generator=g)).to(dt)
    dw0 = torch.randn(N, generator=g).to(dt)
    x64 = x.to(torch.float64)
    mu = x64.mean(-1, keepdim=True) if ln else torch.zeros(M, 1, dtype=torch.float64)
    rstd = ((x64 - mu).pow(2).mean(-1) + NORM_EPS).rsqrt().to(F32)
    mean = mu.squeeze(-1).to(F32) if ln else None
    return dict(x=x, dy=dy, dres=dres, w=w, dw0=dw0, rstd=rstd, mean=mean)


def norm_bwd_ref(inp, dt, ln):
    """dx (without dres), its slack, dw (without dw0), its slack; rstd / mean are fp32 inputs."""
    x, g, w = (inp[k].to(torch.float64) for k in ("x", "dy", "w"))
    M, N = x.shape
    r = inp["rstd"].to(torch.float64).unsqueeze(-1)
    mu = inp["mean"].to(torch.float64).unsqueeze(-1) if ln else 0.0
    n = (x - mu) * r
    dn = g * w
    sdnn = (dn * n).mean(-1, keepdim=True)
    sdn = dn.mean(-1, keepdim=True) if ln else 0.0
    dx = r * (dn - sdn - n * sdnn)
    # the two row means are norm_k-operation sums (the split kernel adds 4 cross-wave terms); then
    # subtract twice, multiply twice: k = norm_k + 4 + 4 over the summands of dx
    K = norm_k(N) + 8
    S = r * (dn.abs() + (dn.abs().mean(-1, keepdim=True) if ln else 0.0) + n.abs() * (dn * n).abs().mean(-1, keepdim=True))
    # dw: a column's rows are added along one chain of at most M + 4 (waves) + 8 + 8 (colsum) terms
    dw = (g * n).sum(0)
    dw_slack = (M + 24) * EPS32 * (g * n).abs().sum(0)
    return dx, K * EPS32 * S, dw, dw_slack


# ---------------------------------------------------------------- SwiGLU
def swiglu_gate(dt):
    """16-bit: every finite bit pattern; fp32: 4096 log-spaced magnitudes over [2^-126, 2^127], both signs, zeros."""
    if dt in _FMT:
        g = torch.arange(65536, dtype=torch.int32)
        g = torch.where(g >= 32768, g - 65536, g).to(torch.int16).view(dt)
        return torch.where(torch.isfinite(g), g, torch.zeros_like(g))
    mag = torch.exp2(torch.linspace(-126, 127, 4096, dtype=torch.float64)).to(F32)
    return torch.cat([mag, -mag, torch.zeros(1024)])


def swiglu_inputs(dt, random_u):
    gate = swiglu_gate(dt).reshape(-1, 1024)
    g = gen(3, DTYPES.index(dt), random_u)
    u = torch.randn(gate.shape, generator=g).to(dt) if random_u else torch.ones_like(gate)
    da = torch.randn(gate.shape, generator=g).to(dt)
    return torch.cat([gate, u], -1).contiguous(), da


def swiglu_stride_inputs():
    g = gen(4)
    T, F_ = 1040, 8192  # 1040 * 1024 vectors: just past the 4096-block x 256-thread grid cap
    return torch.randn(T, 2 * F_, generator=g).to(BF16), torch.randn(T, F_, generator=g).to(BF16)


def swiglu_ref(gu, da, dt):
    F_ = gu.shape[-1] // 2
    g, u = gu[..., :F_].to(torch.float64), gu[..., F_:].to(torch.float64)
    d = da.to(torch.float64)
    s = 1.0 / (1.0 + torch.exp(-g))
    silu = g * s
    a = silu * u
    t1, t2 = s, silu * (1.0 - s)
    dg = d * u * (t1 + t2)
    du = d * silu
    # exp(-g) is exp2(-g * log2 e): rounding the product moves the exponent by |g| log2(e) 2^-24,
    # i.e. the value by ~|g| 2^-24 relative, plus the product's constant and exp2 (1 ulp): (2|g| + 4)
    # half-ulps, weighted by exp(-g) / (1 + exp(-g)) = 1 - s in the denominator; then the add, the
    # reciprocal (1 ulp) and two multiplies: 6.
    k = 6 + (1.0 - s) * (2 * g.abs() + 4)
    sl_a = k * EPS32 * a.abs()
    sl_du = (k + 1) * EPS32 * du.abs()
    # s + silu (1 - s) cancels near g = -1.28; 1 - s carries the rounding of s (1 ulp of ~1) in full
    # where s -> 1, times silu: 3 half-ulps of |silu|
    sl_dg = EPS32 * (d * u).abs() * ((k + 4) * (t1.abs() + t2.abs()) + 3 * silu.abs())
    if dt in _FMT:  # storage rounding dominates where nothing cancels
        sl_a, sl_du = torch.zeros_like(a), torch.zeros_like(a)
    # below g ~ -87.3 the sigmoid itself is under 2^-126 (exp(-g) overflows fp32 at -88.7) while
    # g * s is not yet: fp32 denormal handling of s is not part of the contract, so s may be off by 2^-126
    low = ((g < -87.0) & (g > -200.0)).to(torch.float64) * TINY
    sl_a = sl_a + (g * u).abs() * low
    sl_du = sl_du + (d * g).abs() * low
    sl_dg = sl_dg + (d * u).abs() * (1 + g.abs()) * low
    return dict(a=(a, sl_a), dgu=(torch.cat([dg, du], -1), torch.cat([sl_dg, sl_du], -1)))


# ---------------------------------------------------------------- RoPE
ROPE_CASES = [(5, S, 2, 1, d) for d in (8, 64, 128) for S in (3, 64)] + [(1, 8192, 1, 1, 8)]  # B, S, hq, hkv, d
ROPE_THETA = 500000.0


def rope_inputs(B, S, hq, hkv, d, dt):
    from fault_tolerant_llm_training_amd.models.llama import rope_tables

    cos, sin = rope_tables(d, S + 5, ROPE_THETA)  # tables longer than S
    g = gen(5, B, S, d, DTYPES.index(dt))
    qkv = torch.randn(B * S, (hq + 2 * hkv) * d, generator=g).to(dt)
    return qkv, cos.to(F32).contiguous(), sin.to(F32).contiguous()


def rope_ref(qkv, cos, sin, S, hq, hkv, d, bwd=False):
    """Rotated [T, (hq+hkv)*d] columns in fp64 from the fp32 tables, and the slack: two products and
    one add per output (k = 3) over |a cos| + |b sin|."""
    T = qkv.shape[0]
    width = (hq + hkv) * d
    x = qkv[:, :width].to(torch.float64).reshape(T, -1, d // 2, 2)
    pos = torch.arange(T) % S
    c = cos.to(torch.float64)[pos].unsqueeze(1)
    s = sin.to(torch.float64)[pos].unsqueeze(1) * (-1.0 if bwd else 1.0)
    a, b = x[..., 0], x[..., 1]
    out = torch.stack((a * c - b * s, a * s + b * c), -1).reshape(T, width)
    mag = torch.stack(((a * c).abs() + (b * s).abs(), (a * s).abs() + (b * c).abs()), -1).reshape(T, width)
    return out, 3 * EPS32 * mag


# ---------------------------------------------------------------- cross-entropy
XENT_V = (8, 2048, 2056, 16384, 16392)
IGNORE = -100


def xent_inputs(T, V, dt):
    g = gen(6, T, V, DTYPES.index(dt))
    x = 3 * torch.randn(T, V, generator=g)
    lab = torch.randint(0, V, (T,), generator=g)
    if T == 5:
        x[1] = 2.5  # all logits equal
        x[2, V // 2] = 40.0  # one dominant logit
        x[3] += 3e4 if dt == F16 else 300.0
        if V > 8:  # some aligned 8-column groups -inf, the row's first among them
            x[4].view(-1, 8)[0::3] = -math.inf
        labs = [torch.tensor([0, V - 1, V // 2, int(lab[3]), 9 if V > 8 else 1]),
                torch.tensor([IGNORE, 0, V - 1, V - 1, IGNORE])]
    else:
        lab[::7] = IGNORE
        lab[1], lab[2] = 0, V - 1
        labs = [lab]
    return x.to(dt), labs


def xent_ref(x, lab):
    x64 = x.to(torch.float64)
    T, V = x64.shape
    lse = torch.logsumexp(x64, -1)
    mx = x64.max(-1).values
    ign = lab == IGNORE
    xy = x64.gather(1, lab.clamp(min=0).unsqueeze(1)).squeeze(1)
    loss = torch.where(ign, torch.zeros_like(lse), lse - xy)
    # a thread adds 8 ceil(V / 2048) exponentials in sequence, each rescale of the running sum is one
    # more product; 6 shuffle levels, 4 waves. An exponential's argument (x - m) log2(e) is rounded
    # before exp2: relative error (2 |x - m| + 4) 2^-24 each, and their softmax-weighted mean of |x - m|
    # is at most ln V. log turns the relative error of the sum into an absolute one; M + log S adds
    # 4 half-ulps of |lse| + |M|.
    k = 2 * 8 * ((V + 2047) // 2048) + 6 + 4 + 2 * math.log(V) + 4
    lse_slack = EPS32 * (k + 4 * (lse.abs() + mx.abs()))
    loss_slack = torch.where(ign, torch.zeros_like(lse), lse_slack + EPS32 * (lse.abs() + xy.abs()))
    return lse, lse_slack, loss, loss_slack


def xent_bwd_ref(x, lab, lse32, grad32, inv32):
    """(exp(x - lse) - onehot) * grad * inv_count with the fp32 lse / grad / inv_count the kernel is given."""
    x64 = x.to(torch.float64)
    l = lse32.to(torch.float64).unsqueeze(1)
    scale = float(grad32) * float(inv32)
    p = torch.exp(x64 - l)
    oh = torch.zeros_like(p)
    live = lab != IGNORE
    oh[live, lab[live]] = 1.0
    out = (p - oh) * scale * live.unsqueeze(1)
    # x - lse, times log2(e), exp2: (2 |x - lse| + 4) half-ulps on p; the subtraction and the two
    # products of the scale: 3 over |p| + onehot
    dif = torch.nan_to_num((x64 - l).abs(), posinf=0.0)
    slack = abs(scale) * EPS32 * (p * (2 * dif + 4) + 3 * (p + oh))
    return out, slack


# ---------------------------------------------------------------- gradient norm
def sumsq_ref(x, nb):
    """Block b of an nb-block launch sums the 8-element vectors i with (i % (nb * 256)) // 256 == b."""
    x64 = x.to(torch.float64).reshape(-1, 8)
    n8 = x64.shape[0]
    blk = (torch.arange(n8) % (nb * 256)) // 256
    part = torch.zeros(nb, dtype=torch.float64).index_add_(0, blk, x64.pow(2).sum(-1))
    # a thread squares and adds 8 values per vector it owns, then 6 shuffle levels and 4 waves
    k = 2 * 8 * ((n8 + nb * 256 - 1) // (nb * 256)) + 6 + 4
    return part, k * EPS32 * part


def finish_ref(partial, max_norm):
    s = partial.to(torch.float64).sum()
    norm = s.sqrt()
    # 1024 threads: each adds ceil(np / 1024) values (4 per vector load), 6 shuffle levels, 16 waves, sqrt
    k = (partial.numel() + 1023) // 1024 + 6 + 16 + 2
    coef = min(1.0, max_norm / (float(norm) + 1e-6)) if max_norm > 0 and math.isfinite(float(norm)) else 1.0
    return norm, k * EPS32 * partial.to(torch.float64).abs().sum() / (2 * norm.clamp(min=1e-300)) + 2 * EPS32 * norm, coef


# ---------------------------------------------------------------- AdamW
ADAMW_PAIRS = ((BF16, BF16), (BF16, F32), (F16, F16), (F16, F32), (F32, F32))
ADAMW_SIZES = ((8, 0), (8 * 255, 0), (8 * 257, 0), (8 * 1000, 2))  # (n, max_blocks)
ADAMW_STEPS = (1, 3, 100000)
# lr 1e-2: the decoupled decay lr * wd = 1e-3 then moves a bf16 parameter across a rounding boundary
# in ~18 % of the elements; at lr 1e-3 a dropped decay would flip 1.8 %, below the cap
ADAMW_HP = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8)


def adamw_scale_inputs(n, pdt, sdt, g=None):
    """Training scale: every term of the update moves the stored value."""
    g = g or gen(7, n, DTYPES.index(pdt), DTYPES.index(sdt))
    p = (0.02 * torch.randn(n, generator=g)).to(pdt)
    gr = (1e-3 * torch.randn(n, generator=g)).to(pdt)
    m = (1e-3 * torch.randn(n, generator=g)).to(sdt)
    v = (1e-6 * torch.rand(n, generator=g)).to(sdt)
    return p, gr, m, v


def adamw_inputs(n, pdt, sdt):
    p, gr, m, v = adamw_scale_inputs(n, pdt, sdt)
    gr[3::8], m[3::8], v[3::8] = 0, 0, 0  # p only decays; the result stays finite
    v[5::8] = 1e-7 if sdt == F16 else 1e-40  # subnormal in the state dtype
    return p, gr, m, v


def adamw_hyper(lr, b1, b2, step):
    """[lr, 1/bc1, 1/sqrt(bc2)], bc = 1 - beta^step: formed in double, each rounded to fp32 once."""
    return np.array([lr, 1.0 / (1.0 - b1 ** step), 1.0 / math.sqrt(1.0 - b2 ** step)], dtype=np.float32)


def adamw_ref(p, g, m, v, coef, step, wd, lr, b1, b2, eps):
    """torch AdamW's formula in fp64 with double scalars (the kernel's fp32 scalars, each rounded once,
    are within the operation counts below). Returns {name: (ref64, slack)}."""
    h = [lr, 1.0 / (1.0 - b1 ** step), 1.0 / math.sqrt(1.0 - b2 ** step)]
    f = float
    b1f, b2f = b1, b2
    p64, g64, m64, v64 = (t.to(torch.float64) for t in (p, g, m, v))
    gj = g64 * float(np.float32(coef))  # stats[1] is an fp32 input
    pd = p64 * (1.0 - h[0] * f(wd))
    dm = (gj - m64) * (1.0 - b1f)
    m2 = m64 + dm
    va, vb = v64 * b2f, (1.0 - b2f) * gj * gj
    v2 = va + vb
    upd = (h[0] * h[1]) * m2 / (v2.sqrt() * h[2] + f(eps))
    # m: clip product, subtract, multiply, add: 4 over |m| + |dm|. v: clip, square, two products, add: 5.
    m_slack = 4 * EPS32 * (m64.abs() + dm.abs())
    v_slack = 5 * EPS32 * v2
    # update: the longer operand chain is v's (5), then sqrt (1 ulp = 2), * 1/sqrt(bc2), + eps, the
    # reciprocal (1 ulp = 2), lr / bc1, two products: 14; the decay (1 - lr wd, product) and the final
    # subtraction: 3 on |p|. One k = 16 over both summands.
    p_slack = 16 * EPS32 * (pd.abs() + upd.abs())
    return dict(p=(pd - upd, p_slack), m=(m2, m_slack), v=(v2, v_slack))
