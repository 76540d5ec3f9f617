"""GEMM routing table (docs / tests): the kernel every GEMM of a step takes, asked of the same
choosers the autograd functions in ops/functional.py and ops/attention.py switch on
(``fwd_kernel`` / ``dx_kernel`` / ``dw_kernel`` and the fused-node gates), for a preset and dtype, on
shape / dtype specs (nothing is allocated; no GPU needed). This module only formats the answers.
tests/test_routing_cpu.py pins the table per preset.
"""
from . import attention as A
from . import functional as Fx


class _Spec:
    """The routing-relevant attributes of a tensor (shape, dtype, device) without storage."""

    def __init__(self, *shape, dtype, cuda=True):
        self.shape, self.dtype, self.is_cuda = tuple(shape), dtype, cuda

    def is_contiguous(self):
        return True


def _name(kernel, M, N, K, a_t, b_t):
    """The table's name of a chooser's answer for C[M, N] over K; a w4 product with its plan."""
    if kernel != "w4":
        return {"f32": "f32 mfma", "blas": "hipBLASLt"}[kernel]
    nj, sp = Fx._w4_plan(M, N, K, a_t, b_t)
    return f"w4 {32 * nj}" + (f" x{sp}" if sp > 1 else "")


def routing_table(margs, dtype, tokens: int = 2048, cuda: bool = True) -> dict:
    """{product: kernel} for one transformer layer and the LM head of ``margs`` at ``tokens`` rows:
    "w4 <tile width>[ xS]" (S = K slices), "w4 qkv+rope", "w4 swiglu", "w4 swiglu-bwd",
    "f32 mfma" (fp32 models: csrc/kernels/gemm_f32.hip), or "hipBLASLt"."""
    T, D, V = tokens, margs.dim, margs.vocab_size
    hd, Hq, Hkv, Fh = margs.head_dim, margs.n_heads, margs.kv_heads, margs.ffn_hidden
    W = (Hq + 2 * Hkv) * hd
    sp = lambda *s: _Spec(*s, dtype=dtype, cuda=cuda)  # noqa: E731
    x, wqkv, wo, w13, w2, head = sp(T, D), sp(W, D), sp(D, Hq * hd), sp(2 * Fh, D), sp(D, Fh), sp(V, D)

    def fwd(xx, w):  # y[Tn, N] = xx[Tn, K] w[N, K]^T
        return _name(Fx.fwd_kernel(xx, w), xx.shape[0], w.shape[0], xx.shape[1], False, False)

    def dx(Tn, w):  # dX[Tn, K] = dY[Tn, N] w[N, K]
        N, K = w.shape
        return _name(Fx.dx_kernel(sp(Tn, N), w), Tn, K, N, False, True)

    def dw(Tn, w):  # dW[N, K] = dY[Tn, N]^T X[Tn, K]
        N, K = w.shape
        return _name(Fx.dw_kernel(sp(Tn, N), sp(Tn, K)), N, K, Tn, True, True)

    t = {}
    t["qkv fwd"] = "w4 qkv+rope" if A._qkv_rope_ok(x, wqkv, hd) else fwd(x, wqkv)
    t["qkv dX"], t["qkv dW"] = dx(T, wqkv), dw(T, wqkv)
    t["wo fwd"], t["wo dX"], t["wo dW"] = fwd(sp(T, Hq * hd), wo), dx(T, wo), dw(T, wo)
    if cuda and Fx._ffn_w4t_ok(x, w13, w2):
        t["w13 fwd"], t["w2 dX"] = "w4 swiglu", "w4 swiglu-bwd"
    else:
        t["w13 fwd"], t["w2 dX"] = fwd(x, w13), dx(T, w2)
    t["w13 dX"], t["w13 dW"] = dx(T, w13), dw(T, w13)
    t["w2 fwd"], t["w2 dW"] = fwd(sp(T, Fh), w2), dw(T, w2)
    rows = Fx._head_rows(T, V)
    t["head fwd"], t["head dX"], t["head dW"] = fwd(sp(rows, D), head), dx(rows, head), dw(rows, head)
    return t
