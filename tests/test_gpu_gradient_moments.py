"""The gradient qg from suffix moments (cmpc_common.h moment_recur / grad_from_moments): with
we_i = w .* e_i the weighted state error of step i and b a column of Bdt entering at step k,

    g = 2 (b . M0_k + u1 . M1_k + u2 . M2_k),   u1 = N1 b, u2 = N1 u1,
    M0_k = sum_{i>=k} we_i,  M1_k = sum_{i>=k} (i - k) we_i,  M2_k = sum_{i>=k} C(i - k, 2) we_i,

in place of every lane running ze_i = we_i + Adt' ze_{i+1} and a 13-term dot product with ze_k.

* the parity hook (cmpc_condense.hip, the same helper) against the float64 condensation at N = 1
  (one step: M1 = M2 = 0), 2, 3, 10 and 20, plain and stress instances, half of them with the
  record's history flag and a non-zero f_est(3), so the Q_qp f term is part of e_i;
* every solver kernel family against the reference pipeline run live: the N = 10 batch that fills
  class 1 (both builds), the tail class and the wide 80 / 96 / 120 classes, class 1 with padding
  lanes (N = 3), and the refining wide builds (N = 12 all-stance: 144; N = 16 trot: 96; N = 20
  trot: 120).
"""

import numpy as np
import pytest

from support import COND_BOUND, gpu_solve, hook_records, solver_mod  # noqa: F401
from test_gpu_parity import assert_failed_reference, assert_parity

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N", [1, 2, 3, 10, 20])
def test_hook_gradient_matches_fp64_condensation(cm, orc, solver_mod, N):
    """qg and qH of BatchSolver.condense against oracle.fp64_condense, normwise (max |difference| /
    max |qg|, qH likewise), within COND_BOUND[N] (2e-6 below N = 10). A CPU model of the two forms
    in fp32 gives qg 1.2e-7 .. 2.8e-7 for the moments and 1.2e-7 .. 3.2e-7 for the recursion."""
    import torch
    prm = cm.make_params(N)
    recs, flag = hook_records(cm, N)
    k = recs.shape[0]
    H = torch.zeros((k, 12 * N, 12 * N), dtype=torch.float32, device="cuda")
    g = torch.zeros((k, 12 * N), dtype=torch.float32, device="cuda")
    s = solver_mod.BatchSolver(prm, max_batch=k)
    try:
        s.condense(torch.from_numpy(recs).cuda(), H, g)
        torch.cuda.synchronize()
    finally:
        s.close()
    H = H.cpu().numpy(); g = g.cpu().numpy()
    bound = COND_BOUND[N] if N >= 10 else 2e-6
    worst_h = worst_g = 0.0
    moved = 0.0  # how far the Q_qp f term moves qg (it must be part of what is compared)
    for i in range(k):
        H64, g64 = orc.fp64_condense(recs[i], prm)
        worst_h = max(worst_h, np.abs(H[i] - H64).max() / np.abs(H64).max())
        worst_g = max(worst_g, np.abs(g[i] - g64).max() / np.abs(g64).max())
        if flag[i]:
            r0 = recs[i].copy()
            r0.view(np.uint32)[30] = 0
            moved = max(moved, np.abs(orc.fp64_condense(r0, prm)[1] - g64).max() / np.abs(g64).max())
    print(f"[gradient-moments] N={N}: qg vs fp64 {worst_g:.2e}, qH vs fp64 {worst_h:.2e} "
          f"(bound {bound:.0e}); f_est moves qg by {moved:.1e}")
    assert moved > 100 * bound, moved
    assert worst_g <= bound, worst_g
    assert worst_h <= bound, worst_h


def _live(cm, orc, solver_mod, recs, N, label, gait="trotting"):
    prm = cm.make_params(N)
    q, st_ref, _ = orc.ref_solve_batch(recs, prm, nthreads=16)
    f, st, _ = gpu_solve(solver_mod, prm, recs)
    ok = st_ref == 0
    assert (st[ok] == 0).all(), np.bincount(st[ok])
    assert_parity(orc, recs, prm, f, q, ok, label=label, gait=gait)
    assert_failed_reference(orc, recs, prm, f, st, st_ref, label=f"{label} N={N}")


# reduced sizes n of the kernel families at N <= 10: class 1's 60- and 64-wide builds, the tail
# class, wide 80 / 96 / 120
FAMILY_EDGES = [0, 60, 64, 72, 80, 96, 120]


def test_every_kernel_family_live(cm, orc, solver_mod):
    """N = 10, 256 random-contact instances (seed chosen so that no family is empty), every
    instance within 1e-4 of the reference pipeline."""
    if not orc.ref_available():
        pytest.skip("oracle/_ref not present")
    N = 10
    recs = cm.make_instances(256, N, seed=9330, random_contact_frac=1.0)
    n = 3 * (cm.unpack_gait(recs, N) != 0).sum(1)
    counts = [int(((n > lo) & (n <= hi)).sum()) for lo, hi in zip(FAMILY_EDGES[:-1], FAMILY_EDGES[1:])]
    print(f"[gradient-moments] N={N}: instances per family (c1-60, c1-64, tail, w80, w96, w120) {counts}")
    assert min(counts) > 0, counts
    _live(cm, orc, solver_mod, recs, N, "gradient moments, every family")


def test_class1_padding_lanes_live(cm, orc, solver_mod):
    """N = 3 (n <= 36): class 1 with most of its lanes padding."""
    if not orc.ref_available():
        pytest.skip("oracle/_ref not present")
    recs = cm.make_instances(64, 3, seed=9303, random_contact_frac=1.0)
    _live(cm, orc, solver_mod, recs, 3, "gradient moments, padding lanes")


@pytest.mark.parametrize("N,B,gait,n_lo,n_hi", [(12, 16, "standing", 144, 144), (16, 64, "trotting", 81, 96),
                                               (20, 32, "trotting", 97, 120)])
def test_refining_wide_builds_live(cm, orc, solver_mod, N, B, gait, n_lo, n_hi):
    """The refining wide builds: N = 12 all-stance (n = 144), N = 16 trot (n = 96: wide 96), N = 20
    trot (n = 120: wide 120)."""
    if not orc.ref_available():
        pytest.skip("oracle/_ref not present")
    recs = cm.make_instances(B, N, seed=9300 + N, random_contact_frac=0.0, gait=gait)
    n = 3 * (cm.unpack_gait(recs, N) != 0).sum(1)
    assert n.min() >= n_lo and n.max() <= n_hi, (n.min(), n.max())
    _live(cm, orc, solver_mod, recs, N, f"gradient moments, wide {n_hi} refining", gait=gait)
