"""Time BatchSolver.sensitivity (cmpc_batch_sensitivity) beside the same handle's solve and evaluate
on the same records: HIP events on the handle's stream after warm-up, N = 10 and N = 20 at 65536
instances. One line per shape: the three times and the ratios (medians over --reps timed calls each),
the mean dimension of the face and the smallest inactive slack over the solved instances."""
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
        grad = torch.randn((B, 12 * N), dtype=torch.float32, device=dev)
        status = torch.zeros(B, dtype=torch.uint8, device=dev)
        cert = torch.zeros((B, sm.CERT_WORDS), dtype=torch.float64, device=dev)
        sens = torch.zeros((B, sm.SENS_WORDS), dtype=torch.float64, device=dev)
        dtraj = torch.zeros((B, 12 * N), dtype=torch.float64, device=dev)
        dg = torch.zeros((B, 12 * N), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        s = sm.BatchSolver(prm, max_batch=B)
        stream = torch.cuda.ExternalStream(s.stream_handle)
        for _ in range(args.warmup):
            s.solve(recs, forces, status)
            s.evaluate(recs, forces, None, cert)
            s.sensitivity(recs, forces, grad, sens, dtraj=dtraj, dg=dg)
        stream.synchronize()
        t_solve = timed(stream, args.reps, lambda: s.solve(recs, forces, status))
        t_eval = timed(stream, args.reps, lambda: s.evaluate(recs, forces, None, cert))
        t_sens = timed(stream, args.reps, lambda: s.sensitivity(recs, forces, grad, sens, dtraj=dtraj, dg=dg))
        t_bwd = timed(stream, args.reps, lambda: s.sensitivity(recs, forces, grad, sens, dtraj=dtraj))
        c = sens.cpu().numpy()
        ok = status.cpu().numpy() == 0
        s.close()
        print(f"N={N} batch={B}: sensitivity {t_sens:.3f} ms (without dg {t_bwd:.3f} ms), solve {t_solve:.3f} ms, "
              f"evaluate {t_eval:.3f} ms; sensitivity / solve {t_sens / t_solve:.3f}, / evaluate "
              f"{t_sens / t_eval:.2f}; solved {int(ok.sum())}, face dimension mean {c[ok, sm.SENS_FREE].mean():.1f}, "
              f"smallest inactive slack {c[ok, sm.SENS_SLACK].min():.2e} N, finite {bool(np.isfinite(c[ok, :27]).all())}",
              flush=True)


if __name__ == "__main__":
    main()
