"""How far the refined wide-class solution is from the fp64 optimum, and why (GPU; test
infrastructure: uses oracle/ and tests/param_sets.py). Per instance of the default, f_max 30 and
mu 0.2 sets at N = 16 / 20 trot: the distance with and without the refinement, the rows active at
ours and at the fp64 optimum, the exact fp64 minimiser on OUR active set (numpy, null-space method)
against that optimum, the reduced Hessian's condition number on the face, and evaluate's gap at
ours / at fp32(x64) / at the reference's forces. profiles/r10_params/refine_face_{parent,new}.log."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import evaluate_ref as er  # noqa: E402
import param_sets as ps  # noqa: E402
from oracle import oracle as orc  # noqa: E402

cm = importlib.import_module("quad-periodic-mpc_amd")
sm = importlib.import_module("quad-periodic-mpc_amd.solver")
sm.load_library()


def face(rec, prm, x, tol):
    """Active rows of the six per stance foot-step at x (slack <= tol) -> (C [m, 12N], b [m])."""
    N = prm.horizon
    ub, stance, mui = er._consts(rec, prm)
    rows, rhs = [], []
    f = x.reshape(4 * N, 3)
    for s in np.flatnonzero(stance):
        cand = [((mui, 0, 1), 0.0), ((-mui, 0, 1), 0.0), ((0, mui, 1), 0.0), ((0, -mui, 1), 0.0),
                ((0, 0, 1), 0.0), ((0, 0, -1), -ub[s])]
        for c, b in cand:
            if np.dot(c, f[s]) - b <= tol:
                r = np.zeros(12 * N)
                r[3 * s:3 * s + 3] = c
                rows.append(r)
                rhs.append(b)
    return np.array(rows).reshape(-1, 12 * N), np.array(rhs)


def face_minimiser(rec, prm, C, b):
    N = prm.horizon
    ub, stance, _ = er._consts(rec, prm)
    keep = np.repeat(stance, 3)
    H, g = orc.fp64_condense(rec, prm)
    H, g, C = H[np.ix_(keep, keep)], g[keep], C[:, keep]
    # independent rows only
    q, r = np.linalg.qr(C.T, mode="complete")
    rank = int((np.abs(np.diag(r[:min(r.shape)])) > 1e-9).sum()) if C.size else 0
    Z = q[:, rank:]
    x0 = np.linalg.lstsq(C, b, rcond=None)[0] if C.size else np.zeros(keep.sum())
    Hz = Z.T @ H @ Z
    y = np.linalg.solve(Hz, -Z.T @ (H @ x0 + g)) if Z.shape[1] else np.zeros(0)
    out = np.zeros(12 * N)
    out[keep] = x0 + Z @ y
    ev = np.linalg.eigvalsh(Hz) if Z.shape[1] else np.array([1.0])
    return out, C.shape[0], rank, Z.shape[1], ev.max() / ev.min()


for set_name in ("default", "fmax30", "mu0.2"):
    for case in ("n16_trot", "n20_trot"):
        d = ps.cpu_data(set_name, case)
        prm, recs, x64 = d["prm"], d["recs"], d["x64"]
        s = sm.BatchSolver(prm, max_batch=len(recs))
        try:
            f_on, st_on, it_on = s.solve_host(recs)
            _, c_on = s.evaluate_host(recs, f_on)
            _, c_64 = s.evaluate_host(recs, x64.astype(np.float32))
            _, c_rf = s.evaluate_host(recs, d["q"].astype(np.float32))
            s.set_refine(False)
            f_off, st_off, _ = s.solve_host(recs)
        finally:
            s.close()
        e_on, e_off = ps.rel_dist(f_on, x64), ps.rel_dist(f_off, x64)
        for i in range(len(recs)):
            sc = max(np.abs(x64[i]).max(), 1.0)
            C, b = face(recs[i], prm, f_on[i].astype(np.float64), 1e-5 * sc)
            C64, _ = face(recs[i], prm, x64[i], 1e-7 * sc)
            xf, m, rank, nz, kappa = face_minimiser(recs[i], prm, C, b)
            j = int(np.abs(f_on[i] - x64[i]).argmax())
            n = int(3 * (cm.unpack_gait(recs[i:i + 1], prm.horizon) != 0).sum())
            g0 = np.maximum(1.0, c_on[i, er.COST0])
            print(f"{set_name} {case} #{i}: n {n} |x64| {sc:.1f} ours {e_on[i]:.1e} (abs {e_on[i] * sc:.1e} N, comp {j % 3} "
                  f"step {j // 12}) unrefined {e_off[i]:.1e} trips {it_on[i]} | active rows ours {m} (rank {rank}) fp64 "
                  f"{C64.shape[0]}; free dims {nz} kappa(Z'HZ) {kappa:.1e}; exact-on-our-face vs x64 "
                  f"{np.abs(xf - x64[i]).max() / sc:.1e}, ours vs exact-on-our-face {np.abs(f_on[i] - xf).max() / sc:.1e} | "
                  f"gap/cost0 ours {c_on[i, er.GAP] / g0:.1e} fp32(x64) {c_64[i, er.GAP] / g0:.1e} reference "
                  f"{c_rf[i, er.GAP] / g0:.1e} cost0 {g0:.1e}", flush=True)
