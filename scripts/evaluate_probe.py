"""Time BatchSolver.evaluate (cmpc_batch_evaluate) beside the same handle's solve on the same
records: HIP events on the handle's stream after warm-up, N = 10 and N = 20 at 65536 instances.
One line per shape: evaluate ms, solve ms, ratio (medians over --reps timed calls each)."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(stream, reps, fn):
    import torch
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    cm = importlib.import_module("quad-periodic-mpc_amd")
    sm = importlib.import_module("quad-periodic-mpc_amd.solver")
    dev = torch.device("cuda:0")
    B = args.batch
    for N in (10, 20):
        prm = cm.make_params(N)
        recs = torch.from_numpy(cm.make_instances(B, N, seed=9100 + N)).to(dev)
        forces = torch.zeros((B, 12 * N), dtype=torch.float32, device=dev)
        status = torch.zeros(B, dtype=torch.uint8, device=dev)
        x_pred = torch.zeros((B, 12 * N), dtype=torch.float32, device=dev)
        cert = torch.zeros((B, sm.CERT_WORDS), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        s = sm.BatchSolver(prm, max_batch=B)
        stream = torch.cuda.ExternalStream(s.stream_handle)
        for _ in range(args.warmup):
            s.solve(recs, forces, status)
            s.evaluate(recs, forces, x_pred, cert)
        stream.synchronize()
        t_solve = timed(stream, args.reps, lambda: s.solve(recs, forces, status))
        t_eval = timed(stream, args.reps, lambda: s.evaluate(recs, forces, x_pred, cert))
        t_cert = timed(stream, args.reps, lambda: s.evaluate(recs, forces, None, cert))
        c = cert.cpu().numpy()
        ok = status.cpu().numpy() == 0
        s.close()
        r = c[ok, sm.CERT_GAP] / np.maximum(1.0, c[ok, sm.CERT_COST0])
        print(f"N={N} batch={B}: evaluate {t_eval:.3f} ms (cert only {t_cert:.3f} ms), solve {t_solve:.3f} ms, "
              f"ratio {t_eval / t_solve:.3f}; solved {int(ok.sum())}, gap/max(1,cost0) median {np.median(r):.2e} "
              f"max {r.max():.2e}, viol max {c[ok, sm.CERT_VIOL].max():.2e}", flush=True)


if __name__ == "__main__":
    main()
