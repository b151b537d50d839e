"""Class 1's two-stance rows (cmpc_class1.hip, the st2 path of solve_c1): a table with exactly two
stance feet at every step (and 6 N <= the build's row width) is condensed straight into the row registers, lane
v computing its whole row, the entries below the diagonal from its own recursion continued below its
step. Every other table takes the exchange through the LDS.

* the hook's row-owner mode (BatchSolver.condense(rows=True)): the continued recursion against the
  float64 condensation, both triangles, on test_gpu_condense_structure's hook instances;
* live parity against the reference pipeline at N = 1, 2, 3, 10: trot (at N = 10 every one of its
  phase tables), tables of random foot pairs, and near-misses of those (n = 6 N, but one step with
  three stance feet and one with a single foot: the general path);
* one record in every build: the 60-wide build (a whole batch of 16384), the 64-wide build (pieces
  of 4096) and the single-instance path agree bit for bit;
* the trot batch under non-default parameters and a non-default robot model, held as
  tests/test_gpu_params.py and tests/test_gpu_model.py hold theirs.
"""
import functools

import numpy as np
import pytest

import model_ref as mr
import param_sets as ps
from conftest import rel_force_err
from support import (COND_BOUND, REF_TOL, assert_swing_zero, closing, gpu_solve, package, set_tables,  # noqa: F401
                     solver_mod)
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

HORIZONS = [1, 2, 3, 10]
B_LIVE = 192
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def pair_tables(rng, B, N):
    tab = np.zeros((B, N, 4), np.uint8)
    pick = rng.integers(0, len(PAIRS), size=(B, N))
    for b in range(B):
        for i in range(N):
            tab[b, i, list(PAIRS[pick[b, i]])] = 1
    return tab


def near_miss_tables(rng, B, N):
    """Pair tables with one stance foot moved to another step: 2 N stance foot-steps as before, one
    step with three and one with a single foot."""
    tab = pair_tables(rng, B, N)
    for b in range(B):
        i1, i2 = rng.choice(N, 2, replace=False)
        while (tab[b, i1] == tab[b, i2]).all():   # the same pair: nothing to move, draw step i2 again
            tab[b, i2] = 0
            tab[b, i2, list(PAIRS[rng.integers(0, len(PAIRS))])] = 1
        f = rng.choice(np.nonzero((tab[b, i1] == 1) & (tab[b, i2] == 0))[0])
        tab[b, i1, f] = 0
        tab[b, i2, f] = 1
    return tab


@functools.lru_cache(maxsize=None)
def live_records(kind, N):
    cm = package()
    if kind == "trot":
        recs = cm.make_instances(B_LIVE, N, seed=7000 + N, random_contact_frac=0.0)
    elif kind == "pairs":
        recs = cm.make_instances(B_LIVE, N, seed=7100 + N, random_contact_frac=0.0)
        recs = set_tables(recs, N, pair_tables(np.random.default_rng(7100 + N), B_LIVE, N))
    else:
        recs = cm.make_instances(B_LIVE, N, seed=7200 + N, random_contact_frac=0.0)
        recs = set_tables(recs, N, near_miss_tables(np.random.default_rng(7200 + N), B_LIVE, N))
    recs.setflags(write=False)
    return recs


def stance_counts(recs, N):
    return (package().unpack_gait(recs, N) != 0).reshape(len(recs), N, 4).sum(2)


# ---- 1. the hook in row-owner mode ---------------------------------------------------------------
@pytest.mark.parametrize("N", HORIZONS)
def test_hook_row_owner_matches_fp64_condensation(cm, orc, solver_mod, N):
    """Every row's own entries on both sides of the diagonal against oracle.fp64_condense, each
    triangle normwise (max |difference| / max |qH|) within COND_BOUND[10], qg likewise; the default
    mode's upper triangle and qg are reproduced bit for bit (the same chain down to the row's step)."""
    import torch
    prm = cm.make_params(N)
    recs = np.concatenate([
        cm.make_instances(4, N, seed=4100 + N, random_contact_frac=1.0),
        cm.make_instances(4, N, seed=4200 + N, random_contact_frac=1.0, stress=True)])
    k = recs.shape[0]
    d_recs = torch.from_numpy(np.ascontiguousarray(recs)).cuda()
    H = torch.zeros((k, 12 * N, 12 * N), dtype=torch.float32, device="cuda")
    g = torch.zeros((k, 12 * N), dtype=torch.float32, device="cuda")
    H0, g0 = torch.zeros_like(H), torch.zeros_like(g)
    s = solver_mod.BatchSolver(prm, max_batch=k)
    try:
        s.condense(d_recs, H, g, rows=True)
        s.condense(d_recs, H0, g0)
        torch.cuda.synchronize()
    finally:
        s.close()
    H = H.cpu().numpy(); g = g.cpu().numpy(); H0 = H0.cpu().numpy(); g0 = g0.cpu().numpy()
    bound = COND_BOUND[10]
    up = np.triu(np.ones((12 * N, 12 * N), bool))
    worst_u = worst_l = worst_g = asym = 0.0
    for i in range(k):
        H64, g64 = orc.fp64_condense(recs[i], prm)
        d = np.abs(H[i] - H64) / np.abs(H64).max()
        worst_u = max(worst_u, d[up].max())
        worst_l = max(worst_l, d[~up].max())
        worst_g = max(worst_g, np.abs(g[i] - g64).max() / np.abs(g64).max())
        asym = max(asym, np.abs(H[i] - H[i].T).max() / np.abs(H[i]).max())
        assert np.array_equal(H[i][up], H0[i][up]) and np.array_equal(g[i], g0[i])
    print(f"[c1-static-rows] hook rows N={N}: upper vs fp64 {worst_u:.2e}, lower {worst_l:.2e}, qg "
          f"{worst_g:.2e} (bound {bound:.0e}); max|H - H'| / max|H| {asym:.2e}")
    assert max(worst_u, worst_l, worst_g) <= bound, (worst_u, worst_l, worst_g)


# ---- 2. live parity ------------------------------------------------------------------------------
LIVE = [(kind, N) for kind in ("trot", "pairs", "near_miss") for N in HORIZONS
        if not (kind == "near_miss" and N < 2)]   # (a near-miss needs two steps)


@pytest.mark.parametrize("kind,N", LIVE)
def test_live_parity(cm, orc, solver_mod, kind, N):
    if not orc.ref_available():
        pytest.skip("oracle/_ref not present")
    prm = cm.make_params(N)
    recs = live_records(kind, N)
    cnt = stance_counts(recs, N)
    assert (cnt.sum(1) == 2 * N).all()
    if kind == "near_miss":   # one step with three feet and one with one
        assert ((cnt == 3).sum(1) == 1).all() and ((cnt == 1).sum(1) == 1).all()
    else:
        assert (cnt == 2).all()
    if kind == "trot" and N == 10:
        tables = {t.tobytes() for t in cm.unpack_gait(recs, N)}
        assert len(tables) == 18, len(tables)   # every phase of the deployed trot
    q, st_ref, _ = orc.ref_solve_batch(recs, prm, nthreads=16)
    assert (st_ref == 0).all(), np.bincount(st_ref)
    f, st, _ = gpu_solve(solver_mod, prm, recs)
    assert (st == 0).all(), np.bincount(st)
    assert_parity(orc, recs, prm, f, q, label=f"two-stance rows, {kind}")


# ---- 3. one record, every build ------------------------------------------------------------------
def test_one_record_every_build(cm, solver_mod):
    """16384 trot instances at N = 10 solved whole (class 1's 60-wide build), in four pieces of 4096
    (the 64-wide build) and, for a dozen, one at a time (the single-instance path): forces, status
    and trip counts agree bit for bit."""
    N, B = 10, 16384
    prm = cm.make_params(N)
    recs = cm.make_instances(B, N, seed=7300, random_contact_frac=0.0)
    assert (stance_counts(recs, N) == 2).all()
    f_all, st_all, it_all = gpu_solve(solver_mod, prm, recs)
    assert (st_all == 0).all(), np.bincount(st_all)
    s = solver_mod.BatchSolver(prm, max_batch=4096)
    try:
        parts = [s.solve_host(recs[a:a + 4096]) for a in range(0, B, 4096)]
    finally:
        s.close()
    np.testing.assert_array_equal(np.concatenate([p[0] for p in parts]), f_all)
    np.testing.assert_array_equal(np.concatenate([p[1] for p in parts]), st_all)
    np.testing.assert_array_equal(np.concatenate([p[2] for p in parts]), it_all)
    s1 = solver_mod.BatchSolver(prm, max_batch=1)
    try:
        for i in np.random.default_rng(7300).choice(B, 12, replace=False):
            f1, st1, it1 = s1.solve_host(recs[i:i + 1])
            assert st1[0] == st_all[i] and it1[0] == it_all[i], i
            np.testing.assert_array_equal(f1[0], f_all[i], err_msg=f"instance {i}")
    finally:
        s1.close()


# ---- 4. non-default parameters and model ---------------------------------------------------------
@pytest.mark.parametrize("set_name", ps.NON_DEFAULT)
def test_trot_under_set(cm, orc, solver_mod, set_name):
    """The N = 10 trot batch of test_live_parity (192 instances, every phase table; trajectories
    built with the set's dt) under each set of tests/param_sets.py, with gate (a) of
    tests/test_gpu_params.py on every instance: status 0, swing legs zero, within 1e-4 of the
    reference pipeline and within 1e-4 of the fp64 optimum.
    The reference's own distance from that optimum is printed, not asserted: test_gpu_params.py
    asserts it <= 5e-5 on its batches (so that a miss cannot be the reference's drift), and on this
    batch it is 3.1e-6 .. 3.7e-5 for eight sets but 5.06e-5 on one instance under alpha 1e-5 (CPU
    figures, independent of the kernels). No instance is left out for it: both gates hold where the
    reference drifts as well."""
    if not orc.ref_available():
        pytest.skip("oracle/_ref not present")
    N = 10
    prm = ps.set_params(set_name, N)
    recs = cm.make_instances(B_LIVE, N, seed=7000 + N, dt=ps.SETS[set_name].get("dt", 0.026),
                             random_contact_frac=0.0)
    assert (stance_counts(recs, N) == 2).all()
    assert len({t.tobytes() for t in cm.unpack_gait(recs, N)}) == 18   # every phase of the deployed trot
    q, st_ref, _ = orc.ref_solve_batch(recs, prm, nthreads=16)
    x64, ri64 = ps.fp64_batch(orc, recs, prm)
    assert (ri64 == 0).all() and (st_ref == 0).all()
    ref64 = ps.rel_dist(q, x64)
    f, st, _ = gpu_solve(solver_mod, prm, recs)
    e_ref, e64 = rel_force_err(f, q), ps.rel_dist(f, x64)
    print(f"[c1-static-rows] params {set_name}: ours within {e64.max():.1e} of the fp64 optimum, the "
          f"reference within {ref64.max():.1e}; ours vs the reference {e_ref.max():.1e}")
    assert_swing_zero(cm, recs, N, f)
    assert (st == 0).all(), np.bincount(st)
    assert e_ref.max() <= REF_TOL, (e_ref.max(), int(e_ref.argmax()))
    assert e64.max() <= REF_TOL, (e64.max(), int(e64.argmax()))


def test_trot_under_model(cm, orc, solver_mod):
    """The N = 10 trot batch of test_live_parity (192 instances, every phase table) under the
    "heavy" model of tests/model_ref.py: status 0, swing legs zero, within 1e-4 of the fp64 optimum
    under that model (tests/test_gpu_model.py's gate at N <= 10)."""
    if not orc.ref_available():
        pytest.skip("oracle/_ref not present")
    N = 10
    prm = cm.make_params(N)
    mdl = mr.model("heavy")
    recs = live_records("trot", N)
    assert len({t.tobytes() for t in cm.unpack_gait(recs, N)}) == 18
    x64, ri64 = mr.fp64_batch(recs, prm, mdl)
    assert (ri64 == 0).all()
    with closing(solver_mod.BatchSolver(prm, max_batch=len(recs), model=mdl)) as s:
        f, st, _ = s.solve_host(recs)
    e64 = ps.rel_dist(f, x64)
    print(f"[c1-static-rows] model heavy: ours within {e64.max():.1e} of the fp64 optimum")
    assert_swing_zero(cm, recs, N, f)
    assert (st == 0).all(), np.bincount(st)
    assert e64.max() <= REF_TOL, (e64.max(), int(e64.argmax()))
