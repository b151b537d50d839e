"""Class 1's factorisation panels (cmpc_class1.hip, solve_c1): four pivots per step, the second pair
of a panel (columns k+2, k+3 and rows k+2, k+3 of J) only where k + 2 < n. The shapes are the
smallest at which a panel can go wrong, not the workload's own.

* every residue of n mod 4 and the half-panel guard, live against the reference pipeline: N = 1 with
  0 .. 4 stance feet (n = 0, 3, 6, 9, 12: first panels that end after their first pair among them),
  random tables at N = 2 and 3 (n up to 36), tables constructed to n = 57 and 60 (the last panels of
  the 60-wide build) and to n = 63 (the 64-wide build alone) at N = 10;
* one record in every build, bit for bit: the 60-wide build, the 64-wide build, the single-instance
  path and the per-instance kernels under a table of default rows. At N <= 5 the launch plan gives
  every batch the 60-wide build (12 N <= 64), so besides N = 3 the records of one case are at N = 6,
  where pieces of 4096 do take the 64-wide build;
* a failing pivot at any place in a panel: alpha on a ladder of negative values (the handle's shared
  alpha: the cost table refuses a row with alpha <= 0), the expected status from the smallest
  eigenvalue of the condensation hook's H in float64.
"""

import numpy as np
import pytest

from status_cases import NOT_PD, OK
from support import bits, gpu_solve, package, reduced_sizes, set_tables, solver_mod  # noqa: F401
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

B_LIVE = 192


def count_tables(rng, N, counts):
    """Stance tables [B, N, 4] with counts[b] stance foot-steps each, placed at random."""
    tab = np.zeros((len(counts), 4 * N), np.uint8)
    for b, c in enumerate(counts):
        tab[b, rng.choice(4 * N, int(c), replace=False)] = 1
    return tab.reshape(len(counts), N, 4)


def counted_records(N, B, seed, counts):
    recs = package().make_instances(B, N, seed=seed, random_contact_frac=0.0)
    recs = set_tables(recs, N, count_tables(np.random.default_rng(seed), N, counts))
    assert (reduced_sizes(recs, N) == 3 * np.asarray(counts)).all()
    return recs


# ---- 1. every residue of n mod 4, the half-panel guard --------------------------------------------
# (name, N, stance foot-steps per record: a number, or None for the generator's random tables)
LIVE = [("n0", 1, 0), ("n3", 1, 1), ("n6", 1, 2), ("n9", 1, 3), ("n12", 1, 4),
        ("random_N2", 2, None), ("random_N3", 3, None),
        ("n57", 10, 19), ("n60", 10, 20), ("n63", 10, 21)]


def live_records(N, fs, seed):
    if fs is None:
        return package().make_instances(B_LIVE, N, seed=seed, random_contact_frac=1.0)
    return counted_records(N, B_LIVE, seed, np.full(B_LIVE, fs))


@pytest.mark.parametrize("name,N,fs", LIVE, ids=[c[0] for c in LIVE])
def test_live_parity_every_residue(cm, orc, solver_mod, name, N, fs):
    """192 instances per case: status 0, swing forces exactly 0, forces within 1e-4 of the reference
    pipeline (assert_parity). An n = 0 instance has no QP: CMPC_OK with zero forces."""
    if not orc.ref_available():
        pytest.skip("oracle/_ref not present")
    prm = cm.make_params(N)
    recs = live_records(N, fs, 7500 + 16 * N + (fs or 0))
    n = reduced_sizes(recs, N)
    if fs is None:   # the random tables reach every residue, and a lone first pair (n - 4 m = 1 or 2)
        assert set(n[n > 0] % 4) == {0, 1, 2, 3} and (n % 4 == 1).any() and (n % 4 == 2).any(), np.bincount(n)
    f, st, it = gpu_solve(solver_mod, prm, recs)
    assert (st == OK).all(), np.bincount(st)
    swing = np.repeat(cm.unpack_gait(recs, N) == 0, 3, axis=1)
    assert (bits(f[swing]) == 0).all()
    assert (bits(f[n == 0]) == 0).all() and (it[n == 0] == 0).all()
    live = n > 0
    if not live.any():
        return
    q, st_ref, _ = orc.ref_solve_batch(recs[live], prm, nthreads=16)
    assert (st_ref == 0).all(), np.bincount(st_ref)
    assert_parity(orc, recs[live], prm, f[live], q, label=f"c1 panel, {name}")


# ---- 2. one record, every build -------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 6])
def test_one_record_every_build(cm, solver_mod, N):
    """16384 records with 0 .. 20 stance foot-steps (n = 0 .. 60, every residue) solved whole (the
    60-wide build), in pieces of 4096 (at N = 6 the 64-wide build), for a dozen one at a time (the
    single-instance path) and whole under a cost table of default rows (the per-instance kernels):
    forces, status and trip counts agree bit for bit."""
    B = 16384
    rng = np.random.default_rng(7600 + N)
    recs = counted_records(N, B, 7600 + N, rng.integers(0, min(4 * N, 20) + 1, size=B))
    prm = cm.make_params(N)
    f_all, st_all, it_all = gpu_solve(solver_mod, prm, recs)
    assert (st_all == OK).all(), np.bincount(st_all)
    s = solver_mod.BatchSolver(prm, max_batch=4096)
    try:
        parts = [s.solve_host(recs[a:a + 4096]) for a in range(0, B, 4096)]
    finally:
        s.close()
    for j, whole in enumerate((f_all, st_all, it_all)):
        np.testing.assert_array_equal(bits(np.concatenate([p[j] for p in parts])), bits(whole))
    s1 = solver_mod.BatchSolver(prm, max_batch=1)
    try:
        for i in rng.choice(B, 12, replace=False):
            f1, st1, it1 = s1.solve_host(recs[i:i + 1])
            assert st1[0] == st_all[i] and it1[0] == it_all[i], i
            np.testing.assert_array_equal(bits(f1[0]), bits(f_all[i]), err_msg=f"instance {i}")
    finally:
        s1.close()
    s = solver_mod.BatchSolver(prm, max_batch=B)
    try:
        s.set_instance_costs(np.repeat(cm.make_instance_costs(), B, axis=0))
        f_i, st_i, it_i = s.solve_host(recs)
    finally:
        s.close()
    np.testing.assert_array_equal(bits(f_i), bits(f_all))
    np.testing.assert_array_equal(st_i, st_all)
    np.testing.assert_array_equal(it_i, it_all)


# ---- 3. a failing pivot at any place in a panel -----------------------------------------------------
# The cost table refuses a row with alpha <= 0 (cmpc_batch_set_instance_costs), so the ladder goes
# through the handle's shared alpha, which is not validated: one solve of the batch per alpha, and
# the records whose H stays positive definite under it are the clean ones beside the failing ones.
# Under the default weights the x / y force entries of B'SB are a thousandth of the z entries and the
# first or second pivot fails under any alpha that decides the sign. These weights balance a foot's
# block (angular rates 1, velocities 600: (dt / m)^2 against (dt r / I)^2), so the ladder's alphas
# fail pivots from 0 to beyond 4, in three or all four places of a panel (float64 Cholesky of the
# oracle's condensation on the same records: none of the live instances falls between the thresholds
# at N = 1 and 2, 13 of 336 at N = 3, where none stays positive definite).
PIVOT_WEIGHTS = (1, 1, 1, 10, 10, 10, 1, 1, 1, 600, 600, 600)
ALPHA_LADDER = (-2e-4, -5e-4, -1e-3, -2e-3, -5e-3, -1e-2, -3e-2)
EIG_BAND = 1e-3


def first_failing_pivot(H):
    A = H.copy()
    for k in range(len(A)):
        if A[k, k] <= 0:
            return k
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k]) / A[k, k]
    return -1


@pytest.mark.parametrize("N", [1, 2, 3])
def test_failing_pivot_anywhere_in_a_panel(cm, solver_mod, N):
    """Smallest eigenvalue of the hook's H (float64, stance variables) below -1e-3 |H|: CMPC_NOT_PD
    and zero forces; above +1e-3 |H|: CMPC_OK; in between not asserted (at most a fifth of the
    instances). A record that solves keeps the bits it has in a batch of solving records alone."""
    import torch
    B = 48
    recs = cm.make_instances(B, N, seed=7700 + N, random_contact_frac=1.0)
    stance = np.repeat(cm.unpack_gait(recs, N) != 0, 3, axis=1)
    d_recs = torch.from_numpy(np.ascontiguousarray(recs)).cuda()
    H = torch.zeros((B, 12 * N, 12 * N), dtype=torch.float32, device="cuda")
    g = torch.zeros((B, 12 * N), dtype=torch.float32, device="cuda")
    live = between = 0
    places, counts = set(), np.zeros(5, int)
    s = solver_mod.BatchSolver(cm.make_params(N), max_batch=B)
    try:
        for alpha in ALPHA_LADDER:
            s.set_params(cm.make_params(N, alpha=alpha, weights=PIVOT_WEIGHTS))
            s.condense(d_recs, H, g)
            torch.cuda.synchronize()
            f, st, it = s.solve_host(recs)
            counts += np.bincount(st, minlength=5)[:5]
            H64 = H.cpu().numpy().astype(np.float64)
            for i in range(B):
                if not stance[i].any():   # no QP
                    assert st[i] == OK and (bits(f[i]) == 0).all(), (alpha, i)
                    continue
                live += 1
                Hr = H64[i][np.ix_(stance[i], stance[i])]
                w = np.linalg.eigvalsh(Hr)
                r = w[0] / np.abs(w).max()
                if r < -EIG_BAND:
                    assert st[i] == NOT_PD and (bits(f[i]) == 0).all() and it[i] == 0, (alpha, i, r, st[i])
                    places.add(first_failing_pivot(Hr) % 4)
                elif r > EIG_BAND:
                    assert st[i] == OK, (alpha, i, r, st[i])
                else:
                    between += 1
            ok = st == OK
            if ok.any() and not ok.all():   # the clean records beside the failing ones keep their bits
                f_c, st_c, it_c = s.solve_host(recs[ok])
                assert (st_c == OK).all()
                np.testing.assert_array_equal(bits(f_c), bits(f[ok]))
                np.testing.assert_array_equal(it_c, it[ok])
    finally:
        s.close()
    print(f"[c1-panel] failing pivots N={N}: {counts} by status over the ladder, {between} of {live} between "
          f"the thresholds, failing places mod 4 {sorted(places)}")
    assert counts[NOT_PD] > 0 and (N == 3 or counts[OK] > 0)   # (at N = 3 no record stays positive definite)
    assert between * 5 <= live, (between, live)
    assert len(places) >= 3, places   # the ladder does spread the failures over a panel's places
