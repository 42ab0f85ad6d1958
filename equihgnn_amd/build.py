"""Build libequihgnn_hip.so (gfx950) in-tree with hipcc.

    python -m equihgnn_amd.build          # incremental
    python -m equihgnn_amd.build --force

The .so is git-ignored but travels with the gpurun snapshot; nothing is JIT-compiled at run time.
"""
from __future__ import annotations

import glob
import os
from concurrent.futures import ThreadPoolExecutor
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(ROOT, "include")
LIB = os.path.join(PKG, "libequihgnn_hip.so")
# measurement build of the panel kernels (-DPN_STAMPS: per-wavefront s_memtime stamps around the phases of a panel's life);
# bench.py loads it BESIDE the product library to time the aggregation prologues that have no launch of their own
STAMPS_LIB = os.path.join(PKG, "libequihgnn_panel_stamps.so")
# the row-panel family (csrc/panel.h) and what its libraries need beside it: the sources of STAMPS_LIB and of the tools'
# diagnostic variants of the panel kernels
PANEL_SOURCES = ["panel.hip", "api.hip"]
ARCH = "gfx950"
MAX_COMPILES = 16           # hipcc processes in flight: more than the CPUs a build is given only slows it down
# every compile of the sources, the product library's objects and the diagnostic variants alike
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-I", INCLUDE, "-I", CSRC,
         "-ffp-contract=off",  # a*b+c stays two roundings unless written fmaf(): the kNN
                               # distances must match the reference's fp32 CPU arithmetic
         "-Wall", "-Wno-unused-function"]


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (ROCm toolchain required to build libequihgnn_hip.so)")


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def needs_build() -> bool:
    if not os.path.exists(LIB) or not os.path.exists(STAMPS_LIB):
        return True
    t = min(os.path.getmtime(LIB), os.path.getmtime(STAMPS_LIB))
    deps = sources() + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(INCLUDE, "*.h"))
    return any(os.path.getmtime(d) > t for d in deps)


def compile_variant(srcs, defines, out: str, verbose: bool = True) -> str:
    """A diagnostic build: the csrc files `srcs` (e.g. PANEL_SOURCES) with the extra macros `defines`
    (e.g. ["PN_STAMPS"], ["INC_ABLATE=1"]) compiled into the shared library `out`, with the product's flags."""
    cmd = [_hipcc(), *FLAGS, "-shared", *(f"-D{d}" for d in defines), *(os.path.join(CSRC, s) for s in srcs), "-o", out]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return out


def build(force: bool = False, verbose: bool = True) -> str:
    if not force and not needs_build():
        return LIB
    bdir = os.path.join(PKG, "build")
    os.makedirs(bdir, exist_ok=True)
    hipcc = _hipcc()
    headers = glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(INCLUDE, "*.h"))
    # one batch: the product's objects and, under names of their own, the -DPN_STAMPS objects of the stamps library
    units = [(src, ".o", []) for src in sources()]
    units += [(os.path.join(CSRC, s), ".stamps.o", ["-DPN_STAMPS"]) for s in PANEL_SOURCES]
    objs = {".o": [], ".stamps.o": []}
    jobs = []                   # (source, command) of every stale object
    for src, ext, defines in units:
        obj = os.path.join(bdir, os.path.basename(src).replace(".hip", ext))
        objs[ext].append(obj)
        if not force and os.path.exists(obj) and all(os.path.getmtime(obj) > os.path.getmtime(d) for d in [src, *headers]):
            continue
        jobs.append((src, [hipcc, *FLAGS, *defines, "-c", src, "-o", obj]))
    jobs.sort(key=lambda j: -os.path.getsize(j[0]))        # the longest compiles first: the big sources bound the build
    if verbose:
        for _, cmd in jobs:
            print(" ".join(cmd), flush=True)
    with ThreadPoolExecutor(min(MAX_COMPILES, os.cpu_count() or 1)) as pool:
        for (src, _), rc in zip(jobs, list(pool.map(subprocess.call, [cmd for _, cmd in jobs]))):
            if rc != 0:
                raise RuntimeError(f"hipcc failed on {src}")
    for lib, ext in ((LIB, ".o"), (STAMPS_LIB, ".stamps.o")):
        cmd = [hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", lib, *objs[ext]]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
