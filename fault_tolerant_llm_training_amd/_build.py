"""In-tree build of the native components with explicit ``hipcc`` (gfx950 only).

Two shared objects are produced next to this file:

* ``_kernels.so`` — the hand-written CDNA4 HIP kernels (``csrc/kernels/*.hip``),
  registered as ``torch.ops.ftamd.*`` through ``TORCH_LIBRARY_FRAGMENT``.
* ``_runtime.so`` — the C++ runtime (``csrc/runtime/*.cpp``): async-signal-safe
  signal flags, the pinned-host checkpoint snapshot engine and the checkpoint
  writer thread, exposed through pybind11.

No hipify, no ``torch.utils.cpp_extension`` JIT: sources are compiled directly
with ``hipcc --offload-arch=gfx950`` and linked against the HIP runtime that
ships inside the installed PyTorch wheel (both carry SONAME
``libamdhip64.so.7``, so one runtime is loaded per process).

Usage: ``python -m fault_tolerant_llm_training_amd._build [-j N] [--force]``.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import os
import subprocess
import sys
import sysconfig
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = ROOT / "csrc"
BUILD = ROOT / "build"
ARCH = "gfx950"  # MI355X (CDNA4) only

KERNELS_SO = PKG / "_kernels.so"
RUNTIME_SO = PKG / "_runtime.so"


def _torch_paths():
    import torch

    tdir = Path(torch.__file__).resolve().parent
    return tdir / "include", tdir / "lib", int(torch._C._GLIBCXX_USE_CXX11_ABI)


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def _common_flags(ext_name: str):
    inc, _lib, abi = _torch_paths()
    import pybind11

    return [
        "-O3",
        "-std=c++17",
        "-fPIC",
        f"-D_GLIBCXX_USE_CXX11_ABI={abi}",
        "-D__HIP_PLATFORM_AMD__=1",
        "-DUSE_ROCM=1",
        "-DHIPBLAS_V2",
        "-D__HIP_NO_HALF_OPERATORS__=1",
        "-D__HIP_NO_HALF_CONVERSIONS__=1",
        "-DTORCH_API_INCLUDE_EXTENSION_H",
        f"-DTORCH_EXTENSION_NAME={ext_name}",
        "-I",
        str(inc),
        "-I",
        str(inc / "torch" / "csrc" / "api" / "include"),
        "-I",
        sysconfig.get_paths()["include"],
        "-I",
        pybind11.get_include(),
        "-I",
        str(CSRC / "kernels"),
        "-I",
        str(CSRC / "runtime"),
        "-Wno-unused-result",
        "-Wno-ignored-attributes",
        "-Wno-deprecated-declarations",
    ]


def _includes(src: Path, dirs, seen=None):
    """Local headers ``src`` includes (``#include "x.h"``), transitively."""
    seen = set() if seen is None else seen
    for line in src.read_text(errors="replace").splitlines():
        line = line.strip()
        if not line.startswith("#include \""):
            continue
        name = line.split('"')[1]
        for d in dirs:
            h = d / name
            if h.exists() and h not in seen:
                seen.add(h)
                _includes(h, dirs, seen)
                break
    return seen


def _needs(obj: Path, src: Path, headers) -> bool:
    if not obj.exists():
        return True
    t = obj.stat().st_mtime
    if src.stat().st_mtime > t:
        return True
    return any(h.stat().st_mtime > t for h in headers)


# The w4 GEMM translation units: their device assembly is kept (-save-temps=obj, the exact code
# that is assembled and linked) and checked by _w4check before _kernels.so may be linked.
W4_CHECKED = ("gemm_w4_fwd", "gemm_w4_dx", "gemm_w4_dw")


# Translation units compiled without the packed fp32 instructions (v_pk_fma_f32, v_pk_mul_f32,
# v_pk_add_f32). The results are the same either way (the packed forms round each element as the
# scalar ones do); the reason is registers. With them the compiler pairs the accumulators of the
# decode_w8 kernels across activation rows (about 2270 v_pk_fma_f32) and the pairing costs VGPRs:
# 74 -> 114 for the one-row gemv, 127 -> 242 for the 8-row tile, and the 4-row SwiGLU tile reaches
# 256 with spills to scratch. Without them every kernel of the unit stays at or under 128 VGPRs with
# no scratch, which the 512-thread workgroups of the multi-row forms need to fit twice per CU. The
# two builds were compared by their register counts only, not timed against each other. The other
# units keep the flags they were tuned with. decode_mx4 is not in the list: its products are dot2
# instructions, the only fp32 the compiler packs is the block sums' add and scale fma across the rows of a
# tile (8 rows: 16 v_pk_add_f32, 16 v_pk_fma_f32), and with that every kernel of the unit is without scratch (plain forms 75-102
# VGPRs, SwiGLU 113-148).
NO_PACKED_FP32 = ("decode_w8",)
NO_PACKED_FP32_FLAGS = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]


def _asm_of(src: Path, obj: Path) -> Path:
    return obj.parent / f"{src.stem}-hip-amdgcn-amd-amdhsa-{ARCH}.s"


def _compile(src: Path, obj: Path, flags, device: bool):
    cmd = [_hipcc()] + flags
    if device:
        cmd += [f"--offload-arch={ARCH}", "-x", "hip"]
        if src.stem in W4_CHECKED:
            cmd += ["-save-temps=obj"]
        if src.stem in NO_PACKED_FP32:
            cmd += NO_PACKED_FP32_FLAGS
    cmd += ["-c", str(src), "-o", str(obj)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(obj.parent))
    if r.returncode != 0:
        raise RuntimeError(f"compile failed: {src}\n{' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    if device and src.stem in W4_CHECKED:
        check_w4_asm(_asm_of(src, obj), obj)
    return obj


def check_w4_asm(asm: Path, obj: Path = None) -> int:
    """The w4 static check (_w4check) on one TU's kept assembly; on an unsafe placement the object
    is deleted (so the next build recompiles it) and the build fails. Returns the kernel count."""
    from . import _w4check

    n, bad = _w4check.check_asm(str(asm))
    if bad or n == 0:
        if obj is not None and obj.exists():
            obj.unlink()
        raise RuntimeError(f"w4 static check failed for {Path(asm).name} (_kernels.so not linked):\n"
                           + _w4check.report(n, bad))
    return n


def _link(objs, out: Path, device: bool, extra=()):
    _inc, lib, _ = _torch_paths()
    cmd = [_hipcc(), "-shared", "-fPIC"]
    if device:
        cmd += [f"--offload-arch={ARCH}"]
    cmd += [str(o) for o in objs]
    cmd += [
        "-L",
        str(lib),
        "-lc10",
        "-lc10_hip",
        "-ltorch",
        "-ltorch_cpu",
        "-ltorch_hip",
        "-lamdhip64",
        f"-Wl,-rpath,{lib}",
        *extra,
        "-o",
        str(out) + ".tmp",
    ]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed: {out}\n{' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    os.replace(str(out) + ".tmp", out)


def build(jobs: int = 0, force: bool = False, verbose: bool = True) -> None:
    BUILD.mkdir(exist_ok=True)
    jobs = jobs or min(8, os.cpu_count() or 4)
    targets = [
        (KERNELS_SO, sorted((CSRC / "kernels").glob("*.hip")), CSRC / "kernels", "_kernels", True, ()),
        (RUNTIME_SO, sorted((CSRC / "runtime").glob("*.cpp")), CSRC / "runtime", "_runtime", False, ("-lz", "-ltorch_python")),
    ]
    for out, srcs, hdr_dir, name, device, extra in targets:
        dirs = [hdr_dir, CSRC / "kernels"]
        flags = _common_flags(name)
        objs, work = [], []
        for s in srcs:
            o = BUILD / f"{name}_{s.stem}.o"
            objs.append(o)
            if force or _needs(o, s, _includes(s, dirs)):
                work.append((s, o))
        if work:
            with cf.ThreadPoolExecutor(max_workers=jobs) as ex:
                futs = [ex.submit(_compile, s, o, flags, device) for s, o in work]
                for f in futs:
                    o = f.result()
                    if verbose:
                        print(f"[build] compiled {o.name}", flush=True)
        if work or force or not out.exists() or any(o.stat().st_mtime > out.stat().st_mtime for o in objs):
            _link(objs, out, device, extra)
            if verbose:
                print(f"[build] linked {out.relative_to(ROOT)}", flush=True)


SANITIZERS = {"asan": ["address", "undefined"], "tsan": ["thread"]}
SELFTEST_SRCS = ("signals.cpp", "zip_writer.cpp", "file_reader.cpp")


def build_selftest(kind: str, out_dir: Path = None, verbose: bool = False) -> Path:
    """Host-only build of csrc/tests/runtime_selftest.cpp + the runtime's host sources under
    ASan+UBSan (``asan``) or ThreadSanitizer (``tsan``) — SURVEY.md §5.2. Each ``-fsanitize=``
    follows ``-Xarch_host`` so only host code is instrumented (no GPU sanitizer on this pool);
    the sources are compiled as plain C++ (no device code in them)."""
    out_dir = Path(out_dir or (BUILD / f"selftest_{kind}"))
    out_dir.mkdir(parents=True, exist_ok=True)
    san = []
    for name in SANITIZERS[kind]:
        san += ["-Xarch_host", f"-fsanitize={name}"]
    flags = ["-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__=1",
             "-I", str(CSRC / "runtime"), *san]
    if kind == "asan":
        flags += ["-Xarch_host", "-fno-sanitize-recover=undefined"]
    srcs = [CSRC / "runtime" / f for f in SELFTEST_SRCS] + [CSRC / "tests" / "runtime_selftest.cpp"]
    exe = out_dir / "runtime_selftest"
    cmd = [_hipcc(), *flags, *map(str, srcs), "-L/opt/rocm/lib", "-lamdhip64", "-lz", "-lpthread",
           "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"selftest build failed ({kind})\n{' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    if verbose:
        print(f"[build] {exe}", flush=True)
    return exe


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", "--jobs", type=int, default=0)
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--selftest", choices=sorted(SANITIZERS), help="build the sanitized runtime self-test")
    a = ap.parse_args(argv)
    if a.selftest:
        build_selftest(a.selftest, verbose=True)
        return 0
    build(a.jobs, a.force)


if __name__ == "__main__":
    sys.exit(main())
