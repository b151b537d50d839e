"""Due-masked solve against the unmasked solve: one handle, HIP events after
warm-up, every form in the same run on the same records.

  N = 10, batch 65536, config-3 instances: every 13th instance due (5042), all due, unmasked
  N = 16, batch 65536:                      every 13th instance due, unmasked

Per form: the mean solve time over back-to-back solves, then the two spans of
cmpc_batch_read_timing (class 1's launch; from its end until the side streams have joined) of
solves run one at a time.

  python scripts/due_probe.py [--batch 65536] [--reps 50]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(s, recs, f, st, it, due, reps, rounds=5):
    """-> (median over rounds of the mean ms per solve, [class-1 span, join span] medians)."""
    for _ in range(5):
        s.solve(recs, f, st, it, due=due)
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            s.solve(recs, f, st, it, due=due)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    s.enable_timing(8)
    for _ in range(8):
        s.solve(recs, f, st, it, due=due)
        torch.cuda.synchronize()
    spans, _ = s.read_timing()
    s.enable_timing(0)
    return float(np.median(ms)), [round(float(x), 4) for x in np.median(spans, axis=0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    cm = importlib.import_module("quad-periodic-mpc_amd")
    sm = importlib.import_module("quad-periodic-mpc_amd.solver")
    torch.cuda.set_stream(torch.cuda.Stream())
    B = args.batch
    out = {}
    for N, forms in ((10, ("unmasked", "due_1_13", "due_all", "unmasked")), (16, ("unmasked", "due_1_13", "unmasked"))):
        prm = cm.make_params(N)
        recs = torch.from_numpy(cm.make_instances(B, N)).cuda()
        f = torch.empty((B, 12 * N), device="cuda")
        st = torch.empty(B, dtype=torch.uint8, device="cuda")
        it = torch.empty(B, dtype=torch.int32, device="cuda")
        masks = {"unmasked": None,
                 "due_1_13": (torch.arange(B, device="cuda") % 13 == 0).to(torch.uint8),
                 "due_all": torch.ones(B, dtype=torch.uint8, device="cuda")}
        s = sm.BatchSolver(prm, max_batch=B, stream=torch.cuda.current_stream())
        res = {}
        for k, form in enumerate(forms):   # the unmasked solve first and last: the drift of the run
            ms, spans = timed(s, recs, f, st, it, masks[form], args.reps)
            name = form if form not in res else form + "_again"
            res[name] = {"ms": round(ms, 4), "class1_ms": spans[0], "join_ms": spans[1],
                         "solved": B if masks[form] is None else int(masks[form].sum())}
            print(f"N={N} B={B} {name}: {ms:.4f} ms/solve, class-1 span {spans[0]:.4f} ms, "
                  f"until joined {spans[1]:.4f} ms, {res[name]['solved']} instances solved", flush=True)
        s.close()
        full = res["unmasked"]["ms"]
        for name in res:
            res[name]["ratio_to_unmasked"] = round(res[name]["ms"] / full, 4)
        out[f"N{N}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
