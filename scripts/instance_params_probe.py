"""What the per-instance tables cost: one handle, HIP events around
back-to-back solves after warm-up, the same records solved in several forms in one run:

  shared   the handle's shared model, mu, f_max, weights and alpha (the default robot: the literal
           builds where there is one);
  table    a parameter table (cmpc_batch_set_instance_params) of identical default rows, one per
           instance: the per-instance builds, which load each instance's entry, on a problem whose
           every value is the shared one's;
  costs    a cost table (cmpc_batch_set_instance_costs) of identical default rows alone;
  both     both tables.

Workloads: config 3 (N = 10, bench.py's instance mix), N = 16 trot and N = 20 (config 5's records,
the solve alone). The shared form runs first and last (the drift of the run); forces must agree bit
for bit between the forms.

  python scripts/instance_params_probe.py [--batch 65536] [--reps 50] [--forms shared,table,shared_again]

(--forms picks the forms and their order; a library named by CMPC_LIB must export every symbol the
binding declares, as every library this tree builds does)
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


def timed(s, recs, f, st, it, reps, rounds=5):
    """-> median over rounds of the mean ms per solve."""
    for _ in range(5):
        s.solve(recs, f, st, it)
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            s.solve(recs, f, st, it)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--forms", default="shared,table,costs,both,shared_again")
    args = ap.parse_args()
    cm = importlib.import_module("quad-periodic-mpc_amd")
    sm = importlib.import_module("quad-periodic-mpc_amd.solver")
    torch.cuda.set_stream(torch.cuda.Stream())
    B = args.batch
    table = torch.from_numpy(np.repeat(cm.make_instance_params(), B, axis=0)).cuda()
    costs = torch.from_numpy(np.repeat(cm.make_instance_costs(), B, axis=0)).cuda()
    forms = args.forms.split(",")
    with_costs = "costs" in forms or "both" in forms
    out = {}
    for name, N, kw in (("config3", 10, {}), ("n16_trot", 16, dict(random_contact_frac=0.0)), ("n20", 20, {})):
        prm = cm.make_params(N)
        recs = torch.from_numpy(cm.make_instances(B, N, **kw)).cuda()
        f = torch.empty((B, 12 * N), device="cuda")
        st = torch.empty(B, dtype=torch.uint8, device="cuda")
        it = torch.empty(B, dtype=torch.int32, device="cuda")
        s = sm.BatchSolver(prm, max_batch=B, stream=torch.cuda.current_stream())
        res, digest = {}, {}
        for form in forms:
            s.set_instance_params(table if form in ("table", "both") else None)
            if with_costs:
                s.set_instance_costs(costs if form in ("costs", "both") else None)
            res[form] = round(timed(s, recs, f, st, it, args.reps), 4)
            digest[form] = (f.cpu().numpy().tobytes(), st.cpu().numpy().tobytes())
            print(f"{name} B={B} {form}: {res[form]:.4f} ms/solve", flush=True)
        s.close()
        tabled = [form for form in ("table", "costs", "both") if form in res]
        for form in tabled:
            res[f"ratio_{form}_to_shared"] = round(res[form] / res["shared"], 4)
        res["same_bits"] = all(digest[form] == digest["shared"] for form in digest)
        print(f"{name}: {' / '.join(tabled)} over shared = "
              f"{' / '.join('%.4f' % res[f'ratio_{form}_to_shared'] for form in tabled)}, same bits: {res['same_bits']}",
              flush=True)
        out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
