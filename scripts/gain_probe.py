"""Time BatchSolver.gain (cmpc_batch_gain) and BatchSolver.feedback (cmpc_batch_feedback) beside the same
handle's solve and sensitivity on the same records: HIP events on the handle's stream after warm-up,
N = 10 and N = 20 at 65536 instances. One line per shape: the four times and the ratios (medians over
--reps timed calls each), the mean dimension of the face over all steps and of step 0."""
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
        host = cm.make_instances(B, N, seed=9100 + N)
        recs = torch.from_numpy(host).to(dev)
        forces = torch.zeros((B, 12 * N), dtype=torch.float32, device=dev)
        grad = torch.randn((B, 12 * N), dtype=torch.float32, device=dev)
        status = torch.zeros(B, dtype=torch.uint8, device=dev)
        sens = torch.zeros((B, sm.SENS_WORDS), dtype=torch.float64, device=dev)
        dtraj = torch.zeros((B, 12 * N), dtype=torch.float64, device=dev)
        gain = torch.zeros((B, sm.GAIN_WORDS), dtype=torch.float64, device=dev)
        # the present state: x_0's p, w, v words moved a little (the rpy words of the record are not x_0's)
        x = np.zeros((B, 12), np.float32)
        x[:, 3:6], x[:, 6:9], x[:, 9:12] = host[:, 0:3], host[:, 10:13], host[:, 3:6]
        x[:, 3:] += np.float32(1e-3)
        states = torch.from_numpy(x).to(dev)
        u = torch.zeros((B, 12), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        s = sm.BatchSolver(prm, max_batch=B)
        stream = torch.cuda.ExternalStream(s.stream_handle)
        for _ in range(args.warmup):
            s.solve(recs, forces, status)
            s.sensitivity(recs, forces, grad, sens, dtraj=dtraj)
            s.gain(recs, forces, gain)
            s.feedback(recs, forces, gain, states, u)
        stream.synchronize()
        t_solve = timed(stream, args.reps, lambda: s.solve(recs, forces, status))
        t_sens = timed(stream, args.reps, lambda: s.sensitivity(recs, forces, grad, sens, dtraj=dtraj))
        t_gain = timed(stream, args.reps, lambda: s.gain(recs, forces, gain))
        t_fb = timed(stream, args.reps, lambda: s.feedback(recs, forces, gain, states, u))
        c = gain.cpu().numpy()
        ok = status.cpu().numpy() == 0
        s.close()
        print(f"N={N} batch={B}: gain {t_gain:.3f} ms, feedback {t_fb:.3f} ms, solve {t_solve:.3f} ms, sensitivity "
              f"(without dg) {t_sens:.3f} ms; gain / solve {t_gain / t_solve:.3f}, gain / sensitivity "
              f"{t_gain / t_sens:.3f}; solved {int(ok.sum())}, face dimension mean {c[ok, sm.GAIN_FREE].mean():.1f}, "
              f"of step 0 {c[ok, sm.GAIN_FREE0].mean():.2f}, finite {bool(np.isfinite(c[ok, :144]).all())}", flush=True)


if __name__ == "__main__":
    main()
