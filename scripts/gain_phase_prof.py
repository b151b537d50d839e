"""Phase-level cycle breakdown of the gain kernel (diagnostic, not part of the product path).

Build (no GPU needed):  python scripts/gain_phase_prof.py --build
Run (GPU):              python scripts/gain_phase_prof.py

The diagnostic library is the product's objects with the shared unit of csrc/cmpc_gain.hip compiled
again under -DCMPC_GAIN_PHASE_PROF: lane 0 of every instance adds the clock64() cycles of each phase to
a device counter. A lone wave (batch 1) gives the phases' latencies; a full batch gives per-wave
latencies with the waves of a SIMD interleaved, which rank the phases only.
"""
import argparse
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PROF_LIB = os.path.join(ROOT, "quad-periodic-mpc_amd", "libcmpc_gain_prof.so")
PHASES = ["set-up (staging, frame, Bdt, the face)", "S1 G, Pn Adt", "S2 T = G'Pn", "S3 R", "S4 Cholesky, Y = L^-1 M",
          "S5 P_k", "step 0: K_0, G"]


def build():
    b = importlib.import_module("quad-periodic-mpc_amd.build")
    b.build()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj = os.path.join(b.OBJ, "cmpc_gain.hip_prof.o")
    subprocess.run([hipcc, f"--offload-arch={b.ARCH}", *b.FLAGS, "-DCMPC_GAIN_PHASE_PROF", "-c",
                    os.path.join(b.CSRC, "cmpc_gain.hip"), "-o", obj], check=True)
    objs = [obj if u == ("cmpc_gain.hip", ()) else b._obj(*u) for u in b.UNITS]
    subprocess.run([hipcc, f"--offload-arch={b.ARCH}", "-shared", "-fPIC", "-o", PROF_LIB] + objs, check=True)
    print(PROF_LIB)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--batch", type=int, default=65536)
    a = ap.parse_args()
    if a.build:
        return build()
    os.environ["CMPC_LIB"] = PROF_LIB
    import torch
    cm = importlib.import_module("quad-periodic-mpc_amd")
    sm = importlib.import_module("quad-periodic-mpc_amd.solver")
    lib = sm.load_library()
    lib.cmpc_gain_phase_read.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    dev = torch.device("cuda:0")
    for N in (10, 20):
        prm = cm.make_params(N)
        B = a.batch
        recs = torch.from_numpy(cm.make_instances(B, N, seed=9100 + N)).to(dev)
        forces = torch.zeros((B, 12 * N), dtype=torch.float32, device=dev)
        status = torch.zeros(B, dtype=torch.uint8, device=dev)
        gain = torch.zeros((B, sm.GAIN_WORDS), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        s = sm.BatchSolver(prm, max_batch=B)
        s.solve(recs, forces, status)
        s.gain(recs, forces, gain)
        torch.cuda.synchronize()
        out = (ctypes.c_ulonglong * 8)()
        for label, batch in (("a lone wave", 1), (f"per wave of {B}", B)):
            lib.cmpc_gain_phase_read(out, 1)
            s.gain(recs, forces, gain, batch=batch)
            torch.cuda.synchronize()
            lib.cmpc_gain_phase_read(out, 0)
            c = np.array(list(out)[:7], np.float64) / batch
            free = gain[:batch, sm.GAIN_FREE].mean().item()
            print(f"N={N} {label}: {c.sum():.0f} cycles, face dimension {free:.1f}; " +
                  ", ".join(f"{p} {v:.0f} ({100 * v / c.sum():.0f} %)" for p, v in zip(PHASES, c)), flush=True)
        s.close()


if __name__ == "__main__":
    main()
