"""Per-parameter statistics of the flat training state (``--tensor-stats-every``).

For every parameter tensor, four numbers of each of the four flat buffers (parameters, gradients,
``exp_avg``, ``exp_avg_sq``), over the tensor's elements ``x``:

========== =====================================================================
sumsq      sum of ``x^2`` over the finite elements
absmax     max ``|x|`` over the finite elements (0 if there are none)
nonfinite  number of NaN or +-Inf elements
zeros      number of elements equal to +-0 (subnormals are not zeros)
========== =====================================================================

Every tensor is a contiguous range of its buffer (``models/flat.py``), so one buffer is one
streaming pass with a segment table: ``csrc/kernels/tensor_stats.hip`` on GPU tensors of a kernel
dtype. :func:`segment_stats_reference`, a float64 PyTorch composition of the definition, is the CPU
path (``--device cpu``, fp64 models) and the oracle of the tests. Squares are formed and summed in
float64, where they are exact for bf16 / fp16 / fp32: a sum over ``n`` elements errs by at most
``(n-1) * 2^-53`` relative, on either path. The passes write nothing but their own outputs.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch

FIELDS = ("sumsq", "absmax", "nonfinite", "zeros")
BUFFERS = ("params", "grads", "exp_avg", "exp_avg_sq")
# dtypes the gfx950 kernel covers; others take the composition
_KERNEL_DTYPES = (torch.bfloat16, torch.float16, torch.float32)
_REF_CHUNK = 1 << 24  # elements widened to float64 at a time by the composition


def chunk() -> int:
    """Elements per work item of the kernel: a segment longer than this is cut into items of this
    size, whose partial results a second kernel folds in a fixed order."""
    from .._native import kernels

    return int(kernels().segment_stats_chunk())


def _check_table(offsets: Sequence[int], numels: Sequence[int]) -> int:
    """Segments sorted by offset, disjoint, gaps allowed. Returns the end of the last one."""
    if len(offsets) != len(numels):
        raise ValueError(f"segment table: {len(offsets)} offsets, {len(numels)} lengths")
    end = 0
    for s, (o, n) in enumerate(zip(offsets, numels)):
        if o < 0 or n < 0:
            raise ValueError(f"segment {s} has a negative offset or length ({o}, {n})")
        if o < end:
            raise ValueError(f"segment {s} at {o} starts before the end of the segments ahead of it ({end}): "
                             "the table must be sorted by offset and disjoint")
        end = o + n
    return end


def segment_stats_reference(buf: torch.Tensor, offsets: Sequence[int], numels: Sequence[int]) -> torch.Tensor:
    """The definition: float64 ``[nseg, 4]`` (``FIELDS``) on the CPU, for a contiguous 1-D ``buf``
    of any floating dtype on any device."""
    offsets, numels = [int(o) for o in offsets], [int(n) for n in numels]
    flat = buf.detach()
    if flat.dim() != 1 or not flat.is_contiguous():
        raise ValueError("segment statistics need a contiguous 1-D buffer")
    if _check_table(offsets, numels) > flat.numel():
        raise ValueError(f"the segments end past the end of the buffer ({flat.numel()} elements)")
    out = torch.zeros(len(offsets), 4, dtype=torch.float64)
    for s, (o, n) in enumerate(zip(offsets, numels)):
        sumsq, absmax, bad, zeros = 0.0, 0.0, 0, 0
        for lo in range(o, o + n, _REF_CHUNK):
            x = flat[lo : min(lo + _REF_CHUNK, o + n)].to(torch.float64)
            fin = torch.isfinite(x)
            xf = torch.where(fin, x, torch.zeros_like(x))
            sumsq += float((xf * xf).sum())
            absmax = max(absmax, float(xf.abs().max()))
            bad += int(x.numel() - int(fin.sum()))
            zeros += int((x == 0).sum())
        out[s] = torch.tensor([sumsq, absmax, float(bad), float(zeros)], dtype=torch.float64)
    return out


class SegmentStatsPlan:
    """A segment table ``(offsets, numels)`` planned once. With a GPU ``device`` the kernel's work
    table is built and copied here; :meth:`run` on a buffer of that device is then enqueue-only on
    the current stream (two launches, no host sync, no H2D copy), so it may sit between HIP-graph
    replays. Buffers elsewhere, or of a dtype the kernel does not cover, take the composition.

    ``chunk``: elements per work item (0 = the built-in size); ``sumsq`` is bit-reproducible for
    a given (table, chunk, 16-byte phase of the buffer's address)."""

    def __init__(self, offsets: Sequence[int], numels: Sequence[int], device=None, chunk: int = 0):
        self.offsets = [int(o) for o in offsets]
        self.numels = [int(n) for n in numels]
        self.nseg = len(self.offsets)
        self.extent = _check_table(self.offsets, self.numels)
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.items = self.seg_first = self.partial = None
        if self.device is not None and self.device.type == "cuda":
            from .._native import kernels

            items, first, extent = kernels().segment_stats_plan(
                torch.tensor(self.offsets, dtype=torch.int64), torch.tensor(self.numels, dtype=torch.int64), int(chunk))
            assert int(extent) == self.extent
            self.items = items.to(self.device)
            self.seg_first = first.to(self.device)
            self.partial = torch.empty(items.shape[0], 4, dtype=torch.float64, device=self.device)

    def run(self, buf: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """float64 ``[nseg, 4]`` of ``buf``: on its GPU (asynchronously) from the kernel, on the
        CPU from the composition."""
        t = buf.detach()
        if self.items is not None and t.is_cuda and t.device == self.device and t.dtype in _KERNEL_DTYPES:
            from .._native import kernels

            if out is None:
                out = torch.empty(self.nseg, 4, dtype=torch.float64, device=self.device)
            kernels().segment_stats_(t, self.items, self.seg_first, self.extent, self.partial, out)
            return out
        if t.is_cuda and t.dtype in _KERNEL_DTYPES:
            raise ValueError(f"this plan was built for {self.device}, the buffer is on {t.device}")
        res = segment_stats_reference(t, self.offsets, self.numels)
        if out is not None:
            out.copy_(res)
            return out
        return res


class StateStats:
    """The four buffers of a model / optimizer pair, planned once.

    One process (or ``--dp-mode allreduce``, where the state is replicated): rank 0 runs four
    passes over the slot table. ZeRO-1: the parameters are replicated, rank 0 reads them alone;
    gradients and moments are sharded, so every rank runs the same pass over its own pieces -- the
    slot ranges clipped to ``optimizer.shard_pieces()``, which is also where the reduced gradient
    lives (``reducer.grad_shard``; the replicated sparse-embedding gradient is read as the same
    slice), with moment offsets translated into the compact state layout -- and the per-rank
    ``[P, 4]`` tables are combined over the control group in rank order: sum for ``sumsq`` /
    ``nonfinite`` / ``zeros``, max for ``absmax``. The alignment gaps of the flat layout belong to
    no segment."""

    def __init__(self, model, optimizer, rank: int = 0, world: int = 1, group=None):
        flat = model.flat
        self.model, self.optimizer = model, optimizer
        self.rank, self.world, self.group = int(rank), int(world), group
        slots = sorted(flat.slots.values(), key=lambda s: s.offset)
        self.names: List[str] = [s.name for s in slots]
        self.numel: Dict[str, int] = {s.name: int(s.numel) for s in slots}
        self.sharded = bool(getattr(optimizer, "zero1", False))
        dev = flat.device
        P = len(slots)
        self._plans = {}  # buffer -> (plan, row of every segment)
        whole = ([s.offset for s in slots], [s.numel for s in slots], list(range(P)))
        if self.rank == 0:
            self._plans["params"] = (SegmentStatsPlan(whole[0], whole[1], dev), whole[2])
        if self.sharded:
            g_off, s_off, lens, rows = [], [], [], []
            for flo, slo, n in sorted(optimizer.shard_pieces()):
                for row, s in enumerate(slots):
                    lo, hi = max(s.offset, flo), min(s.offset + s.numel, flo + n)
                    if lo < hi:
                        g_off.append(lo)
                        s_off.append(slo + lo - flo)
                        lens.append(hi - lo)
                        rows.append(row)
            self._plans["grads"] = (SegmentStatsPlan(g_off, lens, dev), rows)
            moments = SegmentStatsPlan(s_off, lens, dev)
            self._plans["exp_avg"] = self._plans["exp_avg_sq"] = (moments, rows)
        elif self.rank == 0:
            plan = SegmentStatsPlan(whole[0], whole[1], dev)
            for b in ("grads", "exp_avg", "exp_avg_sq"):
                self._plans[b] = (plan, whole[2])

    def _buffer(self, name: str) -> torch.Tensor:
        if name == "params":
            return self.model.flat.params
        if name == "grads":
            return self.model.flat.grads
        return getattr(self.optimizer, name)

    def tables(self, buffers: Sequence[str] = BUFFERS) -> Optional[Dict[str, torch.Tensor]]:
        """float64 ``[P, 4]`` per buffer on rank 0, None elsewhere. Every rank calls it (ZeRO-1
        combines over the control group). The passes are enqueued on the current stream behind the
        optimizer's pending updates (``gate.wait_all()``: stream waits, no device-wide sync); the
        host then waits for the results alone."""
        self.optimizer.gate.wait_all()
        raw = {b: self._plans[b][0].run(self._buffer(b)) for b in buffers if b in self._plans}
        P = len(self.names)
        local = {}
        for b in buffers:
            t = torch.zeros(P, 4, dtype=torch.float64)
            if b in raw:
                r = raw[b].cpu()
                _fold_into(t, self._plans[b][1], r)
            local[b] = t
        shared = [b for b in buffers if b != "params"]
        if self.sharded and self.world > 1 and shared:
            import torch.distributed as dist

            mine = torch.stack([local[b] for b in shared])
            parts = [torch.empty_like(mine) for _ in range(self.world)]
            dist.all_gather(parts, mine, group=self.group)
            total = torch.zeros_like(mine)
            for p in parts:  # rank order
                total[..., 0] += p[..., 0]
                total[..., 1] = torch.maximum(total[..., 1], p[..., 1])
                total[..., 2:] += p[..., 2:]
            for i, b in enumerate(shared):
                local[b] = total[i]
        return local if self.rank == 0 else None

    def collect(self, buffers: Sequence[str] = BUFFERS) -> Optional[dict]:
        """``{"numel": {name: int}, buffer: {name: [sumsq, absmax, nonfinite, zeros]}}`` on rank 0."""
        tabs = self.tables(buffers)
        if tabs is None:
            return None
        rec: dict = {"numel": dict(self.numel)}
        for b in buffers:
            rec[b] = {n: _row(tabs[b][i]) for i, n in enumerate(self.names)}
        return rec


def _fold_into(table: torch.Tensor, rows: Sequence[int], r: torch.Tensor) -> None:
    """Rows of ``r`` (CPU, one per segment) into their parameter's row of ``table``, in segment order."""
    for row, v in zip(rows, r.tolist()):
        t = table[row]
        t[0] += v[0]
        t[1] = max(float(t[1]), v[1])
        t[2] += v[2]
        t[3] += v[3]


def _row(t: torch.Tensor) -> list:
    v = t.tolist()
    return [v[0], v[1], int(v[2]), int(v[3])]


def collect(model, optimizer) -> dict:
    """The statistics of all four buffers of a single-process model / optimizer pair."""
    return StateStats(model, optimizer).collect()


def should_record(step: int, every: int, first_step: int) -> bool:
    """A record at step boundary ``step``: every ``every`` steps, never at step 0 and never at the
    first boundary of a process (``first_step``), where no backward has run yet and the gradient
    buffer means nothing."""
    return every > 0 and step > 0 and step != first_step and step % every == 0


def metrics_record(step: int, rec: dict) -> dict:
    out = {"tensor_stats_step": int(step), "fields": list(FIELDS), "numel": rec["numel"]}
    for b in BUFFERS:
        out[b] = rec[b]
    return out


def log_line(step: int, rec: dict) -> str:
    numel = rec["numel"]
    bad = {b: sum(v[2] for v in rec[b].values()) for b in BUFFERS}
    rms = {n: math.sqrt(v[0] / max(1, numel[n])) for n, v in rec["grads"].items()}
    g = max(rms, key=rms.get)
    p = max(rec["params"], key=lambda n: rec["params"][n][1])
    return (f"Tensor stats at step {step}: {len(numel)} parameters | non-finite: "
            + " ".join(f"{b}={bad[b]}" for b in BUFFERS)
            + f" | largest gradient RMS: {g} {rms[g]:.3e} | largest parameter absmax: {p} {rec['params'][p][1]:.3e}")


def nonfinite_line(step: int, rec: dict, limit: int = 8) -> str:
    """The parameters whose gradient holds NaN / Inf, in layout order (``rec``: a ``grads`` record)."""
    numel = rec["numel"]
    bad = [(n, v[2]) for n, v in rec["grads"].items() if v[2]]
    names = ", ".join(f"{n} ({c}/{numel[n]})" for n, c in bad[:limit])
    more = f", ... ({len(bad) - limit} more)" if len(bad) > limit else ""
    return (f"Non-finite gradients in {len(bad)} of {len(numel)} parameters (gradient buffer of step {step}, the "
            f"last backward that ran: up to two steps after the first bad one, on the same parameters because the "
            f"guard skipped every update since): {names}{more}")
