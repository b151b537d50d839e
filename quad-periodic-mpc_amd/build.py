"""Build the HIP extension in-tree: libcmpc_hip.so (kernels + C ABI) for gfx950.

Plain ``hipcc`` (no torch extension machinery): the library exposes only the C ABI of
``include/cmpc_solver.h`` and is loaded with ctypes. Each translation unit is compiled in
parallel into ``build/obj`` and recompiled only when it or a header it includes changed (the
fully unrolled register kernels take minutes per TU).
"""
from __future__ import annotations

import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libcmpc_hip.so")
OBJ = os.path.join(ROOT, "build", "obj")


def wide_builds() -> list:
    """The rows (NV, PERSIST, REFINE, LIT) of kWideBuild in csrc/cmpc_wide_builds.h, the one statement of
    which builds of the wide kernel template exist."""
    text = open(os.path.join(CSRC, "cmpc_wide_builds.h")).read()
    body = re.search(r"kWideBuild\[\]\s*=\s*\{(.*?)\n\};", text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    rows = [tuple(map(int, r)) for r in re.findall(r"\{(\d+),\s*([01]),\s*([01]),\s*([01])\}", body)]
    if not rows or len(set(rows)) != len(rows):
        raise RuntimeError("cmpc_wide_builds.h: no rows, or a row twice, in kWideBuild")
    return rows


def wide_unit(row: tuple) -> tuple:
    return ("cmpc_wide_unit.hip", ("CMPC_UNIT_WIDE=%d,%d,%d,%d" % row,))


# The translation units as (source, defines): one unit per kernel family, and one per build of the
# wide template (compiled side by side the kernels spilled), so the large unrolled kernels compile
# in parallel. The widest first: they take longest.
UNITS = ([("cmpc_tail.hip", ()), ("cmpc_class1.hip", ())] +
         [wide_unit(r) for r in sorted(wide_builds(), key=lambda r: -r[0])] +
         [("cmpc_condense.hip", ()), ("cmpc_launch.hip", ()), ("cmpc_inst_table.hip", ()),
          ("cmpc_estimator.hip", ()), ("cmpc_assemble.hip", ()), ("cmpc_admm.hip", ()), ("cmpc_quadprog.hip", ()),
          ("cmpc_evaluate.hip", ()), ("cmpc_sensitivity.hip", ()), ("cmpc_gain.hip", ()),
          # the per-instance builds of the hooks, each kernel in a unit of its own
          ("cmpc_condense.hip", ("CMPC_CONDENSE_INST=1",)), ("cmpc_evaluate.hip", ("CMPC_EVALUATE_INST=1",)),
          ("cmpc_sensitivity.hip", ("CMPC_SENSITIVITY_INST=1",)), ("cmpc_gain.hip", ("CMPC_GAIN_INST=1",)),
          ("cmpc_abi.cpp", ())])
ARCH = os.environ.get("CMPC_OFFLOAD_ARCH", "gfx950")
# -fno-slp-vectorize: the SLP pass packs adjacent row updates into v_pk_fma_f32, which ties
# slot registers into 64-bit pairs and made the register-resident rows spill
# -ffp-contract=on: multiply-adds fuse only inside one source expression (clang's front end emits
# llvm.fmuladd), never across statements in the back end, so a kernel body rounds the same in
# every launch form it is inlined into (the one-per-entry and persistent wide builds, the
# single-instance path); with `fast` the back end fused differently per form and the same record
# could get different forces in batches of different sizes
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-result", "-fno-slp-vectorize", "-ffp-contract=on"]


def _deps(path: str, seen=None) -> set:
    """The file plus every quoted #include it pulls in, recursively."""
    seen = set() if seen is None else seen
    path = os.path.normpath(path)
    if path in seen or not os.path.exists(path):
        return seen
    seen.add(path)
    for inc in re.findall(r'#include\s+"([^"]+)"', open(path).read()):
        _deps(os.path.join(os.path.dirname(path), inc), seen)
    return seen


def _obj(src: str, defines: tuple) -> str:
    tag = ("_" + "_".join(d.replace("=", "-") for d in defines)) if defines else ""
    return os.path.join(OBJ, f"{src}{tag}.o")


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False, out: str | None = None,
          defines: tuple = ()) -> str:
    lib = out or LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OBJ, exist_ok=True)

    def compile_one(unit: tuple) -> str:
        src, unit_defines = unit
        path = os.path.join(CSRC, src)
        obj = _obj(src, unit_defines + tuple(defines))
        if not force and not _stale(obj, _deps(path)):
            return obj
        cmd = [hipcc, f"--offload-arch={ARCH}", *FLAGS, *[f"-D{d}" for d in unit_defines + tuple(defines)], "-c",
               path, "-o", obj + ".tmp"]
        if src.endswith(".cpp"):
            cmd[1:1] = ["-x", "hip"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        os.replace(obj + ".tmp", obj)
        return obj

    jobs = max(1, min(len(UNITS), int(os.environ.get("MAX_JOBS", os.cpu_count() or 1))))
    with ThreadPoolExecutor(jobs) as ex:
        objs = list(ex.map(compile_one, UNITS))
    if not force and not _stale(lib, objs):
        return lib
    tmp = lib + ".tmp"
    subprocess.run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", tmp] + objs,
                   check=True)
    os.replace(tmp, lib)
    if out is None:
        build_tools(lib)
        build_multi(lib)
    return lib


MULTI_LIB = os.path.join(PKG, "libcmpc_multi.so")


def build_multi(lib: str = LIB) -> str:
    """libcmpc_multi.so (include/cmpc_multi.h): the config-4 sharding over RCCL as a C ABI, linked
    against libcmpc_hip.so and librccl; plus its C++ test caller cmpc_multi_test."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(CSRC, "cmpc_multi.cpp")
    hdrs = [os.path.join(ROOT, "include", h) for h in ("cmpc_multi.h", "cmpc_solver.h")]
    if _stale(MULTI_LIB, [src, lib] + hdrs):
        subprocess.run([hipcc, "-x", "hip", "--offload-arch=" + ARCH, "-O2", "-std=c++17", "-fPIC",
                        "-Wall", "-shared", "-o", MULTI_LIB + ".tmp", src, f"-L{PKG}", "-lcmpc_hip",
                        "-L/opt/rocm/lib", "-lrccl", "-Wl,-rpath,$ORIGIN", f"-Wl,-rpath,{PKG}",
                        "-Wl,-rpath,/opt/rocm/lib"], check=True)
        os.replace(MULTI_LIB + ".tmp", MULTI_LIB)
    exe = os.path.join(PKG, "cmpc_multi_test")
    tsrc = os.path.join(CSRC, "tools", "cmpc_multi_test.cpp")
    if _stale(exe, [tsrc, MULTI_LIB] + hdrs):
        subprocess.run([hipcc, "-x", "hip", "--offload-arch=" + ARCH, "-O2", "-std=c++17", "-o", exe + ".tmp",
                        tsrc, f"-L{PKG}", "-lcmpc_multi", "-lcmpc_hip", "-Wl,-rpath,$ORIGIN",
                        f"-Wl,-rpath,{PKG}"], check=True)
        os.replace(exe + ".tmp", exe)
    # the same kind of caller for cmpc_multi_set_model
    exe = os.path.join(PKG, "cmpc_multi_model_test")
    tsrc = os.path.join(CSRC, "tools", "cmpc_multi_model_test.cpp")
    if _stale(exe, [tsrc, MULTI_LIB] + hdrs):
        subprocess.run([hipcc, "-x", "hip", "--offload-arch=" + ARCH, "-O2", "-std=c++17", "-o", exe + ".tmp",
                        tsrc, f"-L{PKG}", "-lcmpc_multi", "-lcmpc_hip", "-Wl,-rpath,$ORIGIN",
                        f"-Wl,-rpath,{PKG}"], check=True)
        os.replace(exe + ".tmp", exe)
    return MULTI_LIB


def build_tools(lib: str = LIB) -> str:
    """cmpc_abi_latency: a plain C++ caller of the reference ABI, linked against the library
    the way the be2r controller links it (only include/cmpc_solver.h)."""
    exe = os.path.join(PKG, "cmpc_abi_latency")
    src = os.path.join(CSRC, "tools", "cmpc_abi_latency.cpp")
    if _stale(exe, [src, lib]):
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe + ".tmp", src, f"-L{PKG}", "-lcmpc_hip",
                        f"-Wl,-rpath,$ORIGIN", f"-Wl,-rpath,{PKG}"], check=True)
        os.replace(exe + ".tmp", exe)
    build_mfma_probe()
    build_plan_dump()
    return exe


def build_plan_dump() -> str:
    """cmpc_plan_dump: prints the launch plan of a batched solve (csrc/cmpc_plan.h). Compiled by the
    host compiler alone, which keeps that header free of HIP; tests/test_launch_plan.py runs it."""
    exe = os.path.join(PKG, "cmpc_plan_dump")
    src = os.path.join(CSRC, "tools", "cmpc_plan_dump.cpp")
    if _stale(exe, _deps(src)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe + ".tmp", src], check=True)
        os.replace(exe + ".tmp", exe)
    return exe


def build_mfma_probe() -> str:
    """cmpc_mfma_probe: a stand-alone one-wave check of the broadcast 4x4x1 MFMA's register layout
    and rounding, which the class-1 and tail-class row sweeps (mfma_chunk in cmpc_common.h) rely on."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = os.path.join(PKG, "cmpc_mfma_probe")
    src = os.path.join(CSRC, "tools", "cmpc_mfma_probe.cpp")
    if _stale(exe, [src]):
        subprocess.run([hipcc, "-x", "hip", "--offload-arch=" + ARCH, "-O2", "-std=c++17", "-o",
                        exe + ".tmp", src], check=True)
        os.replace(exe + ".tmp", exe)
    return exe


if __name__ == "__main__":
    import sys
    print(build(force="--force" in sys.argv, verbose=True))
