"""The H entries built from Bdt's structure (cmpc_common.h step_proj / foot_entries: one projection
per horizon step and two FMAs per entry instead of a 13-term dot product with a Bdt column):

* the parity hook (cmpc_condense.hip, the same helpers) against the float64 condensation at the
  smallest horizons, where the block bookkeeping can go wrong (N = 1: a single step with no
  successor; N = 2, 3), and at N = 10; wide roll / pitch (stress) and x_drag in +-0.5 so the drag
  rows of Bdt carry weight;
* every solver kernel family that builds H this way against the reference pipeline run live: one
  N = 10 batch whose random contact tables put instances into class 1 (n <= 60 and 61..64), the
  tail class (65..72) and the wide 80 / 96 / 120 classes, and one N = 3 batch where class 1 runs
  with mostly padding lanes;
* one refining wide build (N = 12 all-stance, n = 144).
"""

import numpy as np
import pytest

from support import COND_BOUND, gpu_solve, solver_mod  # noqa: F401
from test_gpu_parity import assert_failed_reference, assert_parity

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N", [1, 2, 3, 10])
def test_hook_matches_fp64_condensation(cm, orc, solver_mod, N):
    """qH / qg of BatchSolver.condense against oracle.fp64_condense, normwise (max |difference| /
    max |qH|, qg likewise), within COND_BOUND (2e-6 up to N = 12; the 13-term form measures
    1.5e-7 .. 4.5e-7 on these)."""
    import torch
    prm = cm.make_params(N)
    recs = np.concatenate([
        cm.make_instances(4, N, seed=4100 + N, random_contact_frac=1.0),
        cm.make_instances(4, N, seed=4200 + N, random_contact_frac=1.0, stress=True)])
    k = recs.shape[0]
    H = torch.zeros((k, 12 * N, 12 * N), dtype=torch.float32, device="cuda")
    g = torch.zeros((k, 12 * N), dtype=torch.float32, device="cuda")
    s = solver_mod.BatchSolver(prm, max_batch=k)
    try:
        s.condense(torch.from_numpy(np.ascontiguousarray(recs)).cuda(), H, g)
        torch.cuda.synchronize()
    finally:
        s.close()
    H = H.cpu().numpy(); g = g.cpu().numpy()
    bound = COND_BOUND[10]
    worst_h = worst_g = 0.0
    for i in range(k):
        H64, g64 = orc.fp64_condense(recs[i], prm)
        worst_h = max(worst_h, np.abs(H[i] - H64).max() / np.abs(H64).max())
        worst_g = max(worst_g, np.abs(g[i] - g64).max() / np.abs(g64).max())
        assert np.array_equal(H[i], H[i].T)
    print(f"[condense-structure] N={N}: qH vs fp64 {worst_h:.2e}, qg vs fp64 {worst_g:.2e} "
          f"(bound {bound:.0e})")
    assert max(worst_h, worst_g) <= bound, (worst_h, worst_g)


# reduced sizes n of the kernel families at N <= 10: class 1's 60- and 64-wide builds, the tail
# class, wide 80 / 96 / 120
FAMILY_EDGES = [0, 60, 64, 72, 80, 96, 120]


def test_every_kernel_family_live(cm, orc, solver_mod):
    """N = 10, 256 random-contact instances (seed chosen so that no family is empty), every
    instance within 1e-4 of the reference pipeline."""
    if not orc.ref_available():
        pytest.skip("oracle/_ref not present")
    N, B = 10, 256
    prm = cm.make_params(N)
    recs = cm.make_instances(B, N, seed=3460, random_contact_frac=1.0)
    n = 3 * (cm.unpack_gait(recs, N) != 0).sum(1)
    counts = [int(((n > lo) & (n <= hi)).sum()) for lo, hi in zip(FAMILY_EDGES[:-1], FAMILY_EDGES[1:])]
    print(f"[condense-structure] N={N}: instances per family (c1-60, c1-64, tail, w80, w96, w120) {counts}")
    assert min(counts) > 0, counts
    q, st_ref, _ = orc.ref_solve_batch(recs, prm, nthreads=16)
    f, st, _ = gpu_solve(solver_mod, prm, recs)
    ok = st_ref == 0
    assert (st[ok] == 0).all(), np.bincount(st[ok])
    assert_parity(orc, recs, prm, f, q, ok, label="condense structure, every family")
    assert_failed_reference(orc, recs, prm, f, st, st_ref, label="condense structure N=10")


def test_class1_padding_lanes_live(cm, orc, solver_mod):
    """N = 3 (n <= 36): class 1 with most of its lanes padding."""
    if not orc.ref_available():
        pytest.skip("oracle/_ref not present")
    N, B = 3, 64
    prm = cm.make_params(N)
    recs = cm.make_instances(B, N, seed=3463, random_contact_frac=1.0)
    q, st_ref, _ = orc.ref_solve_batch(recs, prm, nthreads=16)
    f, st, _ = gpu_solve(solver_mod, prm, recs)
    ok = st_ref == 0
    assert (st[ok] == 0).all(), np.bincount(st[ok])
    assert_parity(orc, recs, prm, f, q, ok, label="condense structure, padding lanes")
    assert_failed_reference(orc, recs, prm, f, st, st_ref, label="condense structure N=3")


def test_refining_wide_build_live(cm, orc, solver_mod):
    """N = 12 all-stance (n = 144: the refining 144-column build), held as the N >= 11 live cases."""
    if not orc.ref_available():
        pytest.skip("oracle/_ref not present")
    N, B = 12, 8
    prm = cm.make_params(N)
    recs = cm.make_instances(B, N, seed=3472, random_contact_frac=0.0, gait="standing")
    assert (3 * (cm.unpack_gait(recs, N) != 0).sum(1) == 144).all()
    q, st_ref, _ = orc.ref_solve_batch(recs, prm, nthreads=16)
    f, st, _ = gpu_solve(solver_mod, prm, recs)
    ok = st_ref == 0
    assert (st[ok] == 0).all(), np.bincount(st[ok])
    assert_parity(orc, recs, prm, f, q, ok, label="condense structure, wide 144 refining", gait="standing")
    assert_failed_reference(orc, recs, prm, f, st, st_ref, label="condense structure N=12")
