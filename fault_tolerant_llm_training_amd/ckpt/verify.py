"""Checkpoint state digests: the record a save puts into the file, and the checks against it.

Every checkpoint the engine writes carries a ``state_digest`` record beside ``data.pkl``: for each
flat state buffer (parameters, ``exp_avg``, ``exp_avg_sq`` and, under ``--ema-decay``, ``ema``) the
position-weighted exact digest of
:mod:`..utils.digest`, formed on the device from the snapshot the file was written from. A resume
digests the buffers where they live after the restore and refuses to train on a mismatch
(:func:`verify_restored`, :class:`CheckpointCorrupt`): a flipped bit, a short or misdirected write
or a stale page anywhere between HBM at save and HBM at resume changes the digest.
``python -m fault_tolerant_llm_training_amd.ckpt verify FILE...`` makes the same check offline, on
the CPU, from the file alone (:func:`verify_file`).

Record layout (little-endian, fixed size, readable with ``zipfile`` + ``struct``)::

    header   8s magic "FTDIGEST" | u32 version (1) | u32 count
    entry    32s buffer name | 64s archive record holding it ("data/<key>") | 16s dtype
             | u64 element count | u64 digest                       (strings NUL-padded)

``torch.load`` never looks at the record, so the files load as before.
"""
from __future__ import annotations

import mmap
import struct
import warnings
import zipfile
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from ..utils.digest import MASK64, digest_int

RECORD_NAME = "state_digest"
MAGIC = b"FTDIGEST"
VERSION = 1
_HEADER = struct.Struct("<8sII")
_ENTRY = struct.Struct("<32s64s16sQQ")
VALUE_OFFSET = _ENTRY.size - 8  # of the digest inside an entry

_DTYPES = {str(d).replace("torch.", ""): d for d in
           (torch.bfloat16, torch.float16, torch.float32, torch.float64)}


def dtype_name(dtype: torch.dtype) -> str:
    return str(dtype).replace("torch.", "")


@dataclass
class DigestEntry:
    name: str      # the engine's buffer name ("params", "exp_avg", "exp_avg_sq")
    record: str    # archive record that holds the buffer ("data/<key>")
    dtype: str     # "bfloat16", ...
    numel: int
    digest: int    # in [0, 2^64)


class CheckpointCorrupt(RuntimeError):
    """The state restored from ``path`` is not the state its writer saved."""

    def __init__(self, path: str, buffer: str, want: int, got: int):
        self.path, self.buffer, self.want, self.got = path, buffer, want, got
        super().__init__(f"checkpoint {path} is corrupt: buffer {buffer} has digest {got:016x}, "
                         f"the file records {want:016x}")


def record_size(count: int) -> int:
    return _HEADER.size + count * _ENTRY.size


def value_offset(index: int) -> int:
    """Byte offset of entry ``index``'s digest inside the record."""
    return _HEADER.size + index * _ENTRY.size + VALUE_OFFSET


def pack_record(entries: Sequence[DigestEntry]) -> bytes:
    out = [_HEADER.pack(MAGIC, VERSION, len(entries))]
    for e in entries:
        name, rec, dt = e.name.encode(), e.record.encode(), e.dtype.encode()
        if len(name) > 32 or len(rec) > 64 or len(dt) > 16:
            raise ValueError(f"digest record: field too long in {e}")
        out.append(_ENTRY.pack(name, rec, dt, int(e.numel), int(e.digest) & MASK64))
    return b"".join(out)


def parse_record(raw: bytes) -> List[DigestEntry]:
    if len(raw) < _HEADER.size:
        raise ValueError("digest record: truncated header")
    magic, version, count = _HEADER.unpack_from(raw, 0)
    if magic != MAGIC:
        raise ValueError(f"digest record: bad magic {magic!r}")
    if version != VERSION:
        raise ValueError(f"digest record: unknown version {version}")
    if len(raw) != record_size(count):
        raise ValueError(f"digest record: {len(raw)} bytes for {count} entries")
    entries = []
    for i in range(count):
        name, rec, dt, numel, dg = _ENTRY.unpack_from(raw, _HEADER.size + i * _ENTRY.size)
        entries.append(DigestEntry(name.rstrip(b"\0").decode(), rec.rstrip(b"\0").decode(),
                                   dt.rstrip(b"\0").decode(), numel, dg))
    return entries


def _find(zf: zipfile.ZipFile, tail: str) -> Optional[zipfile.ZipInfo]:
    """The archive member ``<archive name>/<tail>``."""
    for zi in zf.infolist():
        if zi.filename.split("/", 1)[-1] == tail:
            return zi
    return None


def read_digest_record(path: str) -> Optional[List[DigestEntry]]:
    """The parsed ``state_digest`` record of a checkpoint, or None if the file has none (a
    reference ``torch.save`` file, or one written without the native runtime)."""
    try:
        with zipfile.ZipFile(path) as zf:
            zi = _find(zf, RECORD_NAME)
            if zi is None:
                return None
            return parse_record(zf.read(zi))
    except zipfile.BadZipFile:
        return None


Pieces = Union[torch.Tensor, Sequence[Tuple[torch.Tensor, int]]]


def _partial(buf: Pieces) -> int:
    if isinstance(buf, torch.Tensor):
        return digest_int(buf, 0)
    total = 0
    for t, first_pos in buf:
        total += digest_int(t, first_pos)
    return total & MASK64


def _dtype_numel(buf: Pieces) -> Tuple[Optional[str], Optional[int]]:
    """dtype name and, for a whole tensor, the element count (pieces: the count is the caller's
    sum over ranks, not known here)."""
    if isinstance(buf, torch.Tensor):
        return dtype_name(buf.dtype), buf.numel()
    for t, _ in buf:
        return dtype_name(t.dtype), None
    return None, None


def verify_restored(record: Optional[Sequence[DigestEntry]], buffers: Dict[str, Pieces], group=None,
                    path: str = "", numels: Optional[Dict[str, int]] = None, log=None) -> Dict[str, str]:
    """Compare live buffers with a checkpoint's digest record.

    ``buffers``: name → the whole tensor, or this rank's list of ``(piece, first_pos)`` of it
    (ZeRO-1 shards); with pieces the ranks of ``group`` (gloo) each digest their own and the
    partial digests are added mod 2^64 as Python ints, so every rank sees the same value and
    raises together. ``numels`` gives the full element count of buffers passed as pieces.

    A buffer is compared only if the record has an entry of its name with the same dtype and
    element count; every other one is skipped with one ``log`` line (moment dtype converted on
    load, reference-style per-tensor file, no record). Returns name → 16-hex digest of the
    compared buffers; raises :class:`CheckpointCorrupt` on the first mismatch.
    """
    by_name = {e.name: e for e in record} if record else {}
    todo = []
    for name, buf in buffers.items():
        e = by_name.get(name)
        dt, n = _dtype_numel(buf)
        if n is None:
            n = (numels or {}).get(name)
        if e is None:
            why = "the file has no digest record" if not record else "no digest entry in the file"
        elif dt is not None and e.dtype != dt:
            why = f"saved as {e.dtype}, restored as {dt}"
        elif n is not None and e.numel != n:
            why = f"saved with {e.numel} elements, restored with {n}"
        else:
            todo.append((name, e, buf))
            continue
        if log is not None:
            log(f"Checkpoint digest of {name} not verified: {why}")
    got = [_partial(buf) for _name, _e, buf in todo]
    if group is not None and todo:
        import torch.distributed as dist

        every = [None] * dist.get_world_size(group)
        dist.all_gather_object(every, got, group=group)
        got = [sum(g[i] for g in every) & MASK64 for i in range(len(todo))]
    out = {}
    for (name, e, _buf), g in zip(todo, got):
        if g != e.digest:
            raise CheckpointCorrupt(path, name, e.digest, g)
        out[name] = f"{g:016x}"
    return out


# ---------------------------------------------------------------------------- offline check
_CHUNK_BYTES = 64 << 20


def verify_file(path: str, out=print) -> int:
    """Digest the storages of ``path`` on the CPU and compare them with its record.
    0: all match; 1: a mismatch; 2: no record."""
    record = read_digest_record(path)
    if record is None:
        out(f"{path}: no digest record")
        return 2
    status = 0
    with zipfile.ZipFile(path) as zf, open(path, "rb") as f:
        for e in record:
            zi = _find(zf, e.record)
            dtype = _DTYPES.get(e.dtype)
            if zi is None or dtype is None or zi.compress_type != zipfile.ZIP_STORED:
                out(f"{path}: {e.name}: MISMATCH (record {e.record!r} of dtype {e.dtype} not readable)")
                status = 1
                continue
            es = torch.empty((), dtype=dtype).element_size()
            if zi.file_size < e.numel * es:
                out(f"{path}: {e.name}: MISMATCH ({e.record} holds {zi.file_size} bytes, "
                    f"{e.numel * es} expected)")
                status = 1
                continue
            # stored, so the bytes follow the local header: 30 + name + extra (64-B alignment pad)
            f.seek(zi.header_offset)
            hdr = f.read(30)
            nlen, xlen = struct.unpack_from("<HH", hdr, 26)
            data_off = zi.header_offset + 30 + nlen + xlen
            got = 0
            if e.numel:
                gran = mmap.ALLOCATIONGRANULARITY
                lo = data_off // gran * gran
                with mmap.mmap(f.fileno(), data_off - lo + e.numel * es, access=mmap.ACCESS_READ,
                               offset=lo) as mm:
                    step = _CHUNK_BYTES // es
                    for pos in range(0, e.numel, step):
                        n = min(step, e.numel - pos)
                        with warnings.catch_warnings():  # a read-only mapping, only read here
                            warnings.simplefilter("ignore", UserWarning)
                            t = torch.frombuffer(mm, dtype=dtype, count=n, offset=data_off - lo + pos * es)
                        got += digest_int(t, pos)
                        del t
            got &= MASK64
            ok = got == e.digest
            out(f"{path}: {e.name}: {'ok' if ok else 'MISMATCH'} digest={got:016x} "
                f"recorded={e.digest:016x} ({e.numel} x {e.dtype}, {e.record})")
            if not ok:
                status = 1
    return status
