"""Class 1's active-set selection (cmpc_class1.hip, solve_c1): foot-step s is scored in lane 3 s + 2,
which holds fz and takes fy and fx from the two lanes below by wave shifts, and the foot-step's
upper bound and active flags are registers of that lane.

* the six constraint kinds of a foot-step (+-mu on x, +-mu on y, fz >= 0, fz <= f_max), each as the
  first pick, at foot-steps whose three lanes straddle a DPP row (5: lanes 15-17) or the wave's
  halves (10: lanes 30-32) and at ones that do not (0, 15, and the last one, 19): the records of
  tests/golden/c1_select_kinds.npz (scripts/make_c1_select_cases.py), whose first pick is checked
  here on the CPU before they are solved;
* a record symmetric in two feet, whose two most violated constraints tie;
* drop trips (the flag cleared and set again), the iteration cap and an infeasible bound;
* per-instance mu and f_max that differ from the handle's;
* n = 3, 12, 30, 57 and 60 in the 60-wide build (N = 1 and 5, where every batch gets it), n = 60 and
  63 in the 64-wide build (N = 10, where a batch below 16384 gets it for every n <= 64); trot tables
  (the two-stance condensation) and others (the exchange through the LDS).

Every batch is checked against the reference pipeline at REF_TOL with its status codes, and bit for
bit (forces, status, trip counts) between the batched launch, the per-instance kernels under a table
of the handle's own values and the single-instance path. Batches of at most 256, except the one that
takes the fixture through the 60-wide build at N = 10, which needs 16384.

At N = 10 a small batch gets the 64-wide build and a single instance of n <= 60 the 60-wide one. The
two builds keep R^-1 beside R up to 42 and 45 active positions (SharedC1::QI, what fits their LDS) and
back-substitute beyond, so they agree bit for bit on a record only while its active set stays within
42 positions, which a solve of at most 42 trips does. A longer solve is held to the same status and
trip count and to forces within REF_TOL across the builds.
"""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel_force_err
from status_cases import INFEASIBLE, MAX_ITER, OK, check_invariants, status_counts
from support import (REF_TOL, active_counts, assert_same, bits, closing, gpu_solve, needs_ref,  # noqa: F401
                     package, records, reduced_sizes, set_tables, solver_mod)

gpu = pytest.mark.gpu

LEAD = 1e-3   # the fixture's margin: violation and lead over the runner-up, over max(1, |x|_max)
FOOT_STEPS = (0, 5, 10, 15, 19)
RINV_BOTH = 42   # active positions up to which both class-1 builds keep R^-1 (SharedC1<60>::QI)


# ---- helpers -----------------------------------------------------------------------------------------
def first_pick(orc, cm, rec, prm):
    """The dual active set's first pick in float64: the most violated constraint 6 s + t at the
    unconstrained optimum x = -H^-1 g of the oracle's fp32 condensation, with the kernel's slack
    expressions -> (constraint, its slack, the lead over the runner-up), both over max(1, |x|_max)."""
    c = orc.condense(rec, prm, full=True)
    red = orc.reduce(rec, prm, c["qH"], c["qg"])
    x = -np.linalg.solve(red["H"], red["g"])
    gait = cm.unpack_gait(rec[None], prm.horizon)[0]
    ub = gait[gait != 0].astype(np.float64) * prm.f_max
    fx, fy, fz = x.reshape(-1, 3).T
    mui = 1.0 / prm.mu
    fn = 1.0 / np.sqrt(mui * mui + 1.0)
    sl = np.stack([(mui * fx + fz) * fn, (-mui * fx + fz) * fn, (mui * fy + fz) * fn, (-mui * fy + fz) * fn,
                   fz, ub - fz], -1).reshape(-1)
    o = np.argsort(sl, kind="stable")
    scale = max(1.0, np.abs(x).max())
    return int(o[0]), sl[o[0]] / scale, (sl[o[1]] - sl[o[0]]) / scale


def default_rows(cm, prm, B):
    """The per-instance table whose every row is the handle's own mu and f_max on the default robot."""
    return np.repeat(cm.make_instance_params(mu=prm.mu, f_max=prm.f_max), B, axis=0)


def assert_same_across_builds(got, ref, label):
    """Two solves of the same records by the 60-wide and the 64-wide build: status and trip counts
    equal, forces bit for bit for the records of at most RINV_BOTH trips and within REF_TOL otherwise."""
    short = ref[2] <= RINV_BOTH
    assert_same(got, ref, short, label=label)
    assert_same((ref[0], got[1], got[2]), ref, label=label)
    assert (rel_force_err(got[0], ref[0].astype(np.float64)) <= REF_TOL).all(), label


def every_path(solver_mod, cm, prm, recs, singles=None):
    """The batched solve -> (forces, status, iters), after checking that the per-instance kernels under
    default_rows and the single-instance path (records ``singles``; None: all) give the same bits
    (at N > 5, where the single instance gets the other build: assert_same_across_builds)."""
    B = len(recs)
    out = gpu_solve(solver_mod, prm, recs)
    with closing(solver_mod.BatchSolver(prm, max_batch=B)) as s:
        s.set_instance_params(default_rows(cm, prm, B))
        assert_same(s.solve_host(recs), out, label="per-instance kernels, the handle's own rows")
    same = assert_same if prm.horizon <= 5 else assert_same_across_builds
    with closing(solver_mod.BatchSolver(prm, max_batch=1)) as s1:
        for i in (range(B) if singles is None else singles):
            same(s1.solve_host(recs[i:i + 1]), tuple(a[i:i + 1] for a in out), label=f"single-instance path, record {i}")
    return out


def assert_reference(orc, recs, prm, out, label):
    """Status CMPC_OK where the reference solves (it must solve every record), forces within REF_TOL."""
    f, st, _ = out
    q, st_ref, _ = orc.ref_solve_batch(recs, prm, nthreads=16)
    assert (st_ref == 0).all(), f"{label}: the reference fails on records {np.nonzero(st_ref)[0][:8]}"
    assert (st == OK).all(), f"{label}: {status_counts(st)}"
    err = rel_force_err(f, q)
    print(f"[c1-select] {label}: {len(err)} instances, max err vs the reference {err.max():.2e}")
    assert err.max() <= REF_TOL, f"{label}: {err.max():.3e} at record {int(np.argmax(err))}"


def count_tables(rng, N, counts):
    tab = np.zeros((len(counts), 4 * N), np.uint8)
    for b, c in enumerate(counts):
        tab[b, rng.choice(4 * N, int(c), replace=False)] = 1
    return tab.reshape(len(counts), N, 4)


def sizes_of(recs, N):
    return reduced_sizes(recs, N)


# ---- 1. the six kinds as the first pick --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kinds():
    d = np.load(os.path.join(GOLDEN, "c1_select_kinds.npz"), allow_pickle=False)
    out = {k: d[k] for k in d.files}
    for a in out.values():
        a.setflags(write=False)
    return out


def kind_group(f_max):
    k = kinds()
    m = k["f_max"] == f_max
    return np.ascontiguousarray(k["records"][m]), k["foot_step"][m], k["kind"][m]


def test_kind_records_pick_what_they_claim(cm, orc):
    """Every cell (foot-step, kind) of the fixture once, every record a trot record of n = 60, and on
    the CPU its first pick is that constraint, violated by more than LEAD and as far ahead of the
    runner-up."""
    k = kinds()
    N = int(k["horizon"])
    cells = sorted(zip(k["foot_step"].tolist(), k["kind"].tolist()))
    assert cells == [(s, t) for s in FOOT_STEPS for t in range(6)]
    assert (sizes_of(k["records"], N) == 60).all()
    assert (cm.unpack_gait(k["records"], N).reshape(-1, N, 4).sum(2) == 2).all()   # two stance feet per step
    for rec, s, t, f_max in zip(k["records"], k["foot_step"], k["kind"], k["f_max"]):
        p, viol, lead = first_pick(orc, cm, rec, cm.make_params(N, f_max=float(f_max)))
        assert p == 6 * s + t and viol < -LEAD and lead > LEAD, (s, t, p, viol, lead)


@gpu
@pytest.mark.parametrize("f_max", [120.0, 40.0])
def test_kinds_every_path(cm, orc, solver_mod, needs_ref, f_max):
    """The fixture's records under their f_max (the 64-wide build, the two-stance condensation):
    the reference's forces, every path the same bits, at least one trip each."""
    recs, s, t = kind_group(f_max)
    prm = cm.make_params(10, f_max=f_max)
    out = every_path(solver_mod, cm, prm, recs)
    assert_reference(orc, recs, prm, out, f"kinds f_max={f_max:g}")
    assert (out[2] >= 1).all(), out[2]


@gpu
@pytest.mark.parametrize("f_max", [120.0, 40.0])
def test_kinds_in_the_60_wide_build(cm, solver_mod, f_max):
    """The same records repeated to a batch of 16384, which the launch plan gives the 60-wide build:
    every copy agrees with the small batch's solve by the 64-wide build (assert_same_across_builds),
    and the copies of a record with each other."""
    recs, _, _ = kind_group(f_max)
    prm = cm.make_params(10, f_max=f_max)
    small = gpu_solve(solver_mod, prm, recs)
    B = 16384
    idx = np.arange(B) % len(recs)
    big = gpu_solve(solver_mod, prm, np.ascontiguousarray(recs[idx]))
    assert_same_across_builds(big, tuple(a[idx] for a in small), "60-wide build against the 64-wide build")
    assert_same(big, tuple(a[idx] for a in tuple(b[:len(recs)] for b in big)), label="copies of one record")
    print(f"[c1-select] f_max={f_max:g}: {int((small[2] <= RINV_BOTH).sum())} of {len(recs)} records within "
          f"{RINV_BOTH} trips (trips {small[2].tolist()})")
    assert (small[2] <= RINV_BOTH).any()


# ---- 2. a tie ----------------------------------------------------------------------------------------
def mirrored_record(cm, vdes_x):
    """N = 1, the two front feet in stance, everything mirrored in the x-z plane (no roll, no yaw, no
    lateral motion, the feet at y = -+0.13): the two feet's forces mirror each other, so constraint t
    of foot-step 0 and of foot-step 1 are violated alike for t = 0, 1, 4, 5. The desired forward
    speed asks for more fx than the cone allows."""
    R = records()
    p = np.array([[0.0, 0.0, 0.29]])
    r = np.zeros((1, 12))
    r[0, 0:4] = (0.18, 0.18, -0.18, -0.18)
    r[0, 4:8] = (-0.13, 0.13, -0.13, 0.13)
    r[0, 8:12] = -0.29
    traj = np.zeros((1, 12))
    traj[0, 5] = 0.29
    traj[0, 9] = vdes_x
    rec = R.pack_records(p, np.zeros((1, 3)), np.array([[1.0, 0, 0, 0]]), np.zeros((1, 3)), r, traj,
                         np.array([[1, 1, 0, 0]]), x_drag=np.zeros(1))
    return rec


def test_mirrored_record_ties_on_the_cpu(cm, orc):
    """In float64 the first pick of the mirrored record is constraint 1 (-mu on x of foot-step 0), and
    constraint 7, the same kind of foot-step 1, is violated alike to rounding."""
    prm = cm.make_params(1)
    rec = mirrored_record(cm, 3.0)[0]
    p, viol, lead = first_pick(orc, cm, rec, prm)
    assert p in (1, 7) and viol < -LEAD and abs(lead) < 1e-9, (p, viol, lead)


@gpu
def test_tie_between_two_feet(cm, orc, solver_mod, needs_ref):
    """The mirrored record at a ladder of desired speeds: the reference's forces, every path the same
    bits and trip counts whichever of the tied constraints goes first, and forces that mirror each
    other as far as REF_TOL tells."""
    prm = cm.make_params(1)
    recs = np.concatenate([mirrored_record(cm, vx) for vx in (1.0, 2.0, 3.0, -3.0)])
    out = every_path(solver_mod, cm, prm, recs)
    assert_reference(orc, recs, prm, out, "mirrored feet")
    f = out[0].astype(np.float64)
    a, b = f[:, 0:3], f[:, 3:6] * np.array([1.0, -1.0, 1.0])
    scale = np.maximum(np.abs(f).max(axis=1), 1.0)[:, None]
    assert (np.abs(a - b) <= 2 * REF_TOL * scale).all(), (a, b)
    assert (out[2] >= 2).all(), out[2]   # both tied constraints end up active


# ---- 3. sizes and builds, drop trips ---------------------------------------------------------------------
# (name, N, stance foot-steps per record; "trot": the generator's trot tables; a pair: random counts)
SIZES = [("n3", 1, 1), ("n12", 1, 4), ("n30_trot", 5, "trot"), ("n57", 5, 19), ("n60", 5, 20),
         ("n63_wide", 10, 21), ("mixed_N10", 10, (1, 21))]
B_SIZES = 128


def size_records(name, N, fs):
    cm = package()
    seed = 9400 + 32 * N + sum(map(ord, name)) % 32
    recs = cm.make_instances(B_SIZES, N, seed=seed, random_contact_frac=0.0, stress=True)
    if fs == "trot":
        return recs
    rng = np.random.default_rng(seed)
    counts = np.full(B_SIZES, fs) if isinstance(fs, int) else rng.integers(fs[0], fs[1] + 1, size=B_SIZES)
    return set_tables(recs, N, count_tables(rng, N, counts))


@gpu
@pytest.mark.parametrize("name,N,fs", SIZES, ids=[c[0] for c in SIZES])
def test_sizes_and_builds(cm, orc, solver_mod, needs_ref, name, N, fs):
    """128 stress records per size: the reference's forces and status, every path the same bits."""
    recs = size_records(name, N, fs)
    n = sizes_of(recs, N)
    if isinstance(fs, int):
        assert (n == 3 * fs).all()
    elif fs == "trot":
        assert (n == 6 * N).all()
    prm = cm.make_params(N)
    out = every_path(solver_mod, cm, prm, recs, singles=range(0, B_SIZES, 8))
    assert_reference(orc, recs, prm, out, name)


@gpu
def test_drop_trips(cm, orc, solver_mod, needs_ref):
    """Stress records at N = 10 with 1 .. 21 stance foot-steps placed at random: a solve that took
    more trips than it can have constraints active at its forces (support.active_counts' upper
    count) has dropped one, so its flag was cleared, and a constraint re-added after a drop finds the
    flag as the drop left it. Several such instances, each at the reference's forces."""
    N = 10
    recs = size_records("mixed_N10", N, (1, 21))
    prm = cm.make_params(N)
    f, st, it = gpu_solve(solver_mod, prm, recs)
    assert (st == OK).all(), status_counts(st)
    _, hi, _ = active_counts(cm, prm, recs, f)
    dropped = it > hi
    print(f"[c1-select] drop trips: {int(dropped.sum())} of {len(recs)} instances took more trips than active "
          f"constraints (up to {int((it - hi).max())} more)")
    assert dropped.sum() >= 4, int(dropped.sum())
    q, st_ref, _ = orc.ref_solve_batch(recs[dropped], prm, nthreads=16)
    assert (st_ref == 0).all()
    assert rel_force_err(f[dropped], q).max() <= REF_TOL


# ---- 4. the failure contract -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N", [1, 5, 10])
def test_negative_f_max_is_infeasible(cm, solver_mod, N):
    """f_max = -120: fz >= 0 and fz <= ub < 0 exclude each other, with ub read from the lane's register.
    CMPC_INFEASIBLE and zero forces for every record with a stance foot, on every path."""
    recs = size_records("mixed", N, (0, min(4 * N, 21)))
    prm = cm.make_params(N, f_max=-120.0)
    out = every_path(solver_mod, cm, prm, recs, singles=range(0, B_SIZES, 8))
    f, st, it = out
    n = sizes_of(recs, N)
    check_invariants(recs, prm, f, st, it, label=f"f_max=-120 N={N}")
    assert (st[n > 0] == INFEASIBLE).all() and (st[n == 0] == OK).all(), status_counts(st)


def sinking_records(cm, N, B, seed, counts_hi):
    """Stress records whose trajectory sinks fast (status_cases.all_zero_force_records' lever: z 0.3 m
    lower per step, v_z -6 m/s), with 1 .. counts_hi stance foot-steps: the optimum pins most feet at
    zero force by three pyramid rows each, reached through many drops."""
    R = records()
    recs = cm.make_instances(B, N, seed=seed, random_contact_frac=0.0, stress=True)
    rng = np.random.default_rng(seed)
    recs = set_tables(recs, N, count_tables(rng, N, rng.integers(1, counts_hi + 1, size=B)))
    traj = recs[:, R.REC_HDR:R.REC_HDR + 12 * N].reshape(B, N, 12)
    for k in range(N):
        traj[:, k, 5] = recs[:, R.REC_P + 2] - 0.3 * (k + 1)
        traj[:, k, 11] = -6.0
    return recs


@gpu
def test_iteration_cap(cm, solver_mod):
    """max_iter = 1 allows 1 + 2 n trips. Sinking records at N = 10 take up to a few more than 2 n (an
    add and a drop per variable): every status is CMPC_OK or CMPC_MAX_ITER and at least one instance
    ends at the cap, with zero forces and 2 n + 2 counted trips, on every path; one within the cap has
    the bits of the max_iter = 100 solve."""
    N = 10
    recs = sinking_records(cm, N, 256, 9300 + N, min(4 * N, 21))
    n = sizes_of(recs, N)
    full = gpu_solve(solver_mod, cm.make_params(N), recs)
    prm1 = cm.make_params(N, max_iter=1)
    capped = np.nonzero(full[2] > 2 * n + 1)[0]
    out = every_path(solver_mod, cm, prm1, recs, singles=sorted(set(range(0, 256, 16)) | set(capped.tolist())))
    f, st, it = out
    print(f"[c1-select] max_iter=1 N={N}: {status_counts(st)}, most trips beyond 2 n: {int((full[2] - 2 * n).max())}")
    assert (full[1] == OK).all() and np.isin(st, (OK, MAX_ITER)).all(), status_counts(st)
    check_invariants(recs, prm1, f, st, it, label=f"max_iter=1 N={N}")
    assert_same(out, full, st == OK, label="instances within the cap vs max_iter = 100")
    assert (bits(f[st == MAX_ITER]) == 0).all() and (it[st == MAX_ITER] == 2 * n[st == MAX_ITER] + 2).all()
    assert ((st == MAX_ITER) == (full[2] > 2 * n + 1)).all()
    assert (st == MAX_ITER).any(), status_counts(st)


# ---- 5. per-instance mu and f_max ----------------------------------------------------------------------
MU_FMAX = [(0.4, 120.0), (0.6, 150.0), (0.2, 35.0), (0.8, 60.0)]


@gpu
@pytest.mark.parametrize("N", [5, 10])
def test_per_instance_mu_and_f_max(cm, solver_mod, N):
    """A table whose row i carries combination i % 4 of (mu, f_max), on a handle with the defaults:
    row i has the bits of the shared handle of its combination, and the combinations do differ (35 N
    and 60 N bind in trot, so the bound in the lane's register is the row's, not the handle's)."""
    B = 128
    recs = package().make_instances(B, N, seed=9500 + N, random_contact_frac=0.25, stress=True)
    if N == 10:   # keep every record in class 1
        rng = np.random.default_rng(9500)
        heavy = sizes_of(recs, N) > 63
        recs[heavy] = set_tables(recs[heavy], N, count_tables(rng, N, np.full(int(heavy.sum()), 21)))
    assert (sizes_of(recs, N) <= 63).all()
    ids = np.arange(B) % len(MU_FMAX)
    outs = [gpu_solve(solver_mod, cm.make_params(N, mu=mu, f_max=fm), recs) for mu, fm in MU_FMAX]
    want = tuple(np.stack([outs[k][j][i] for i, k in enumerate(ids)]) for j in range(3))
    with closing(solver_mod.BatchSolver(cm.make_params(N), max_batch=B)) as s:
        s.set_instance_params(cm.make_instance_params(mu=np.array([c[0] for c in MU_FMAX])[ids],
                                                      f_max=np.array([c[1] for c in MU_FMAX])[ids]))
        got = s.solve_host(recs)
    assert (want[1] == OK).all(), status_counts(want[1])
    assert_same(got, want, label="table rows against their shared handles")
    for k in range(1, len(MU_FMAX)):
        m = ids == k
        assert (bits(outs[k][0][m]) != bits(outs[0][0][m])).any(axis=1).mean() > 0.5, k
    fz = got[0].reshape(B, -1, 3)[:, :, 2]
    for k in (2, 3):   # the bound binds, and at the row's value
        m = ids == k
        top = fz[m].max(axis=1)
        assert (top <= MU_FMAX[k][1] * (1 + 1e-4)).all() and (top >= MU_FMAX[k][1] * (1 - 1e-4)).mean() > 0.5, k
