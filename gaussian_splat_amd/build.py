"""Build libgsplat.so in-tree (hipcc, gfx950) and the oracle (gcc).

The product library is compiled ahead of time for gfx950 only; the .so lives
next to this file so it travels with the repo snapshot to the GPU box.
Every translation unit is built with -ffp-contract=off: the pipeline's
floating-point contract spells out every fused op explicitly.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"
BUILD = ROOT / "build" / "gsplat"
LIB = PKG / "libgsplat.so"
ARCH = os.environ.get("GSPLAT_ARCH", "gfx950")

HIP_SOURCES = sorted((CSRC / "kernels").glob("*.hip")) + [CSRC / "host" / "renderer.cpp", CSRC / "host" / "group.cpp"]
CXX_SOURCES = [CSRC / "host" / "ply_loader.cpp", CSRC / "host" / "scene_io.cpp", CSRC / "host" / "camera.cpp",
               CSRC / "host" / "instanced_splat_renderer.cpp", CSRC / "host" / "renderable.cpp"]

COMMON = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
          f"-I{ROOT / 'include'}", f"-I{CSRC}"]
# No SLP vectorisation on the device: it packs the composite's colour fmas
# into v_pk_fma_f32, whose operand pairs cost extra v_movs per record (the
# composite ran 5 % faster without it; other kernels unchanged).
HIP_ONLY = ["-fno-slp-vectorize"]


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found")


def _run(cmd: list[str]) -> None:
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"build failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")


def _stale(out: Path, deps: list[Path]) -> bool:
    if not out.exists():
        return True
    t = out.stat().st_mtime
    return any(d.stat().st_mtime > t for d in deps if d.exists())


def _headers() -> list[Path]:
    return (list((ROOT / "include").rglob("*.h")) + list(CSRC.rglob("*.h")))


def build_lib(verbose: bool = False, extra: list[str] | None = None, build_dir: Path = BUILD,
              lib: Path = LIB) -> Path:
    """Compile and link libgsplat.so.  `extra` flags / `build_dir` / `lib`
    build a variant (tools/build_variant.py: A/B timing, debug counters)."""
    extra = list(extra or [])
    build_dir.mkdir(parents=True, exist_ok=True)
    hipcc = _hipcc()
    hdrs = _headers()
    jobs = []
    objs = []
    for src in HIP_SOURCES:
        obj = build_dir / (src.name + ".o")
        objs.append(obj)
        if _stale(obj, [src, *hdrs]):
            jobs.append([hipcc, "-x", "hip", f"--offload-arch={ARCH}", *COMMON, *HIP_ONLY, *extra, "-c", str(src),
                         "-o", str(obj)])
    for src in CXX_SOURCES:
        if not src.exists():
            continue
        obj = build_dir / (src.name + ".o")
        objs.append(obj)
        if _stale(obj, [src, *hdrs]):
            jobs.append(["g++", *COMMON, *extra, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-c", str(src),
                         "-o", str(obj)])
    workers = min(len(jobs), int(os.environ.get("MAX_JOBS", "8")) or 1) if jobs else 1
    with ThreadPoolExecutor(max_workers=workers) as ex:
        for cmd in jobs:
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
        list(ex.map(_run, jobs))
    if jobs or _stale(lib, objs):
        lib.parent.mkdir(parents=True, exist_ok=True)
        _run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", str(lib), *map(str, objs),
              "-lpthread", "-ldl"])
    return lib


DROPIN_SRC = ROOT / "tests" / "cpp" / "dropin_app.cpp"
DROPIN_BIN = ROOT / "tests" / "cpp" / "dropin_app"


def build_dropin_app(lib: Path = LIB) -> Path:
    """The reference's call sites (main.mm) as a plain C++ program against the
    drop-in headers and libgsplat.so; run by the GPU tests."""
    deps = [DROPIN_SRC, lib, *_headers()]
    if _stale(DROPIN_BIN, deps):
        _run([_hipcc(), "-O2", "-std=c++17", f"-I{ROOT / 'include'}", str(DROPIN_SRC), f"-L{lib.parent}", "-lgsplat",
              "-Wl,-rpath,$ORIGIN/../../gaussian_splat_amd", "-o", str(DROPIN_BIN)])
    return DROPIN_BIN


RCCL_STUB_SRC = ROOT / "tests" / "cpp" / "rccl_stub.hip"
# (beside libgsplat.so, not in tests/: the test tree holds sources only, so a suite run from another
# copy of tests/ against this build still finds it; loaded only through GS_RCCL_LIB)
RCCL_STUB = PKG / "librccl_stub.so"


def build_rccl_stub() -> Path:
    """Test infrastructure: the RCCL entry points as stream-ordered peer copies
    (tests/cpp/rccl_stub.hip), loaded only through GS_RCCL_LIB by the GPU
    tests, so the group's RCCL transport runs on a one-GPU box."""
    if _stale(RCCL_STUB, [RCCL_STUB_SRC]):
        _run([_hipcc(), "-x", "hip", f"--offload-arch={ARCH}", "-O2", "-std=c++17", "-fPIC", "-shared",
              str(RCCL_STUB_SRC), "-o", str(RCCL_STUB)])
    return RCCL_STUB


def build_oracle() -> None:
    """Test infrastructure: the C oracle and, when /root/reference exists, oracle/_ref."""
    _run(["make", "-s", "-C", str(ROOT / "oracle"), "-j4"])


def build_all(verbose: bool = False) -> Path:
    lib = build_lib(verbose)
    build_dropin_app(lib)
    build_rccl_stub()
    build_oracle()
    return lib


if __name__ == "__main__":
    print(build_all(verbose="-v" in sys.argv))
