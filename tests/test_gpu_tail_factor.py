"""The tail class's factorisation (cmpc_tail.hip, solve_t; n = 66, 69, 72 at N <= 10, unrefined): the
main pivots' trailing sweep and the J pass run their main columns as MFMA outer products, the looping
per-instance build keeps the broadcast reads. The shapes are the smallest at which this kernel can go
wrong, not the workload's own: the class exists only for 22, 23 and 24 stance foot-steps, and N = 6 is
the smallest horizon that reaches all three (24 foot-steps, 2 / 1 / 0 of them swing).

* live parity for every n at N = 6 and N = 10, normal and stress states, against the reference pipeline;
  the stress states put constraints of the foot-steps 21 .. 23 (the tail rows and the seam at 63 / 64 /
  65) into the active set and produce drop trips;
* one set of records through every build and launch form, bit for bit: the one-per-entry kernel, the
  looping rest kernel behind a stale grid hint, the single-instance path, and both per-instance kernels
  under a table of default rows; the records in two orders, so that a looping workgroup solves a record
  behind different predecessors;
* a failing pivot: the handle's shared alpha on a ladder of negative values, the expected status from the
  smallest eigenvalue of the condensation hook's H in float64. Where the pivot fails is bounded by the
  problem, not by the ladder: the forces of one horizon step reach the state through a wrench of six
  components (five for two stance feet, whose forces have no moment about the line through them), so
  2 B'SB of the stance variables has rank <= 6 N = 60 < n and a null direction is complete inside the
  first step that holds two stance feet. Under any alpha that decides the sign the pivot that fails is
  among the first dozen (float64 Cholesky of the oracle's condensation on these records and on tables
  built with two stance feet in every leading step: pivots 0 .. 8; of the hook's H on the GPU: 2 .. 9);
  pivots 62 / 63 and the tail pivots 64 .. 71 are out of an alpha ladder's reach on a physical record.
  Tables with one stance foot in every leading step and a gentle first rung push the failure to
  pivots 15 .. 22, and the test asserts that spread. For the same reason no tail-class record solves
  under a negative shared alpha (and the cost table refuses a row with alpha <= 0), so the solving
  records beside the failing ones are class-1 records with a lone stance foot, whose 3 x 3 H stays
  positive definite down to alpha = -2e-2: they must keep the bits of their solve alone on every rung,
  and in a batch of 16384 whose failing tail-class records go through the looping rest kernel.
"""

import numpy as np
import pytest

from status_cases import NOT_PD, OK
from support import (ACT_LO, active_counts, assert_same, assert_swing_zero, bits, closing, gpu_solve,  # noqa: F401
                     needs_ref, package, reduced_sizes, set_tables, solver_mod)
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

B_LIVE = 192
TAIL_SIZES = (66, 69, 72)


def count_tables(rng, N, counts):
    """Stance tables [B, N, 4] with counts[b] stance foot-steps each, placed at random."""
    tab = np.zeros((len(counts), 4 * N), np.uint8)
    for b, c in enumerate(counts):
        tab[b, rng.choice(4 * N, int(c), replace=False)] = 1
    return tab.reshape(len(counts), N, 4)


def tail_records(N, B, seed, stress):
    """B records at horizon N with 22, 23, 24, 22, ... stance foot-steps (n = 66, 69, 72 in turn)."""
    counts = 22 + np.arange(B) % 3
    recs = package().make_instances(B, N, seed=seed, random_contact_frac=0.0, stress=stress)
    recs = set_tables(recs, N, count_tables(np.random.default_rng(seed), N, counts))
    n = reduced_sizes(recs, N)
    assert (n == 3 * counts).all() and set(n) == set(TAIL_SIZES), np.bincount(n)
    return recs


def late_active(cm, prm, recs, f):
    """Per instance: whether a constraint of the stance foot-steps 21 .. 23 (in stance order: the
    variables 63 .. 71) is active at forces f (slack <= ACT_LO max(1, |f|_max), as active_counts)."""
    N = prm.horizon
    stance = cm.unpack_gait(recs, N) != 0
    f3 = np.asarray(f, np.float64).reshape(len(f), 4 * N, 3)
    fx, fy, fz = f3[..., 0], f3[..., 1], f3[..., 2]
    mui = 1.0 / prm.mu
    fn = 1.0 / np.sqrt(mui * mui + 1.0)
    slack = np.stack([(mui * fx + fz) * fn, (-mui * fx + fz) * fn, (mui * fy + fz) * fn,
                      (-mui * fy + fz) * fn, fz, prm.f_max - fz], -1)
    scale = np.maximum(1.0, np.abs(f3).max(axis=(1, 2)))[:, None, None]
    order = np.cumsum(stance, axis=1) - 1
    late = stance & (order >= 21)
    return ((slack <= ACT_LO * scale) & late[..., None]).any(axis=(1, 2))


# ---- 1. live parity for every n ---------------------------------------------------------------------
# (the reference's qpOASES solves every record of these seeds: checked on the CPU, st_ref == 0 for all
# 192 of each case, nWSR <= 57)
LIVE = [(6, False, 2206), (6, True, 2206), (10, False, 2210), (10, True, 2210)]


@pytest.mark.parametrize("N,stress,seed", LIVE, ids=[f"N{c[0]}_{'stress' if c[1] else 'normal'}" for c in LIVE])
def test_live_parity_every_tail_size(cm, orc, solver_mod, needs_ref, N, stress, seed):
    """192 records, 64 of each n: status 0, swing forces exactly 0 (the padding rows of n = 66 and 69
    among them), forces within 1e-4 of the reference pipeline on every instance (assert_parity)."""
    prm = cm.make_params(N)
    recs = tail_records(N, B_LIVE, seed, stress)
    f, st, it = gpu_solve(solver_mod, prm, recs)
    _, hi, _ = active_counts(cm, prm, recs, f)
    late = late_active(cm, prm, recs, f)
    print(f"[tail-factor] live N={N} stress={stress}: trips {it.min()}..{it.max()}, {(it > hi).sum()} instances "
          f"with more trips than possibly active constraints (drop trips), {late.sum()} with an active "
          f"constraint in the foot-steps 21..23, status {np.bincount(st)}")
    assert (st == OK).all(), np.bincount(st)
    assert_swing_zero(cm, recs, N, f)
    if stress:
        assert late.sum() >= B_LIVE // 4, late.sum()   # the tail rows and the seam take part in the active set
        assert (it > hi).any()                         # and some instance dropped a constraint on the way
    q, st_ref, _ = orc.ref_solve_batch(recs, prm, nthreads=16)
    assert (st_ref == 0).all(), np.bincount(st_ref)
    assert_parity(orc, recs, prm, f, q, label=f"tail factor, stress={stress}")


# ---- 2. every build and launch form, bit for bit ---------------------------------------------------
B_HINT = 16384   # the smallest batch whose grids are sized from an earlier solve's class counts


def form_records():
    """96 normal and 96 stress records at N = 10 (32 of each n in either half)."""
    return np.concatenate([tail_records(10, 96, 2310, False), tail_records(10, 96, 2311, True)])


def stale_hint_solves(solver_mod, prm, trot, batches, costs=None):
    """A handle that solved trot-only batches (no instance above class 1: the hinted tail grid is its
    floor of 64 workgroups) gets each of ``batches`` in turn, re-staled before every one: the entries
    past the hinted grid go to the looping rest kernel -> the outputs of ``batches``."""
    out = []
    with closing(solver_mod.BatchSolver(prm, max_batch=len(trot))) as s:
        if costs is not None:
            s.set_instance_costs(costs)
        for b in batches:
            for _ in range(3):
                s.solve_host(trot)
            out.append(s.solve_host(b))
    return out


def test_every_build_and_launch_form_agrees(cm, solver_mod):
    """The one-per-entry kernel (a fresh handle, the batch alone) is the comparator; the rest kernel
    (stale hint at 16384 instances: 192 tail-class records among trot records, 64 of them inside the
    hinted grid, 128 over the rest kernel's 32 looping workgroups), the same with the records in the
    opposite order (other predecessors in every looping workgroup), the single-instance path, and the
    per-instance builds of both kernels under a table of default rows."""
    N = 10
    prm = cm.make_params(N)
    recs = form_records()
    T = len(recs)
    base = gpu_solve(solver_mod, prm, recs)
    assert (base[1] == OK).all(), np.bincount(base[1])
    # the single-instance path: four records of each n, normal and stress
    with closing(solver_mod.BatchSolver(prm, max_batch=1)) as s1:
        for i in list(range(6)) + list(range(96, 102)):
            f1, st1, it1 = s1.solve_host(recs[i:i + 1])
            assert st1[0] == base[1][i] and it1[0] == base[2][i], i
            np.testing.assert_array_equal(bits(f1[0]), bits(base[0][i]), err_msg=f"single-instance path, record {i}")
    # the per-instance one-per-entry kernel
    with closing(solver_mod.BatchSolver(prm, max_batch=T)) as s:
        s.set_instance_costs(np.repeat(cm.make_instance_costs(), T, axis=0))
        assert_same(s.solve_host(recs), base, label="per-instance kernel, default rows")
    # the looping kernels behind a stale hint
    trot = cm.make_instances(B_HINT, N, seed=2320, random_contact_frac=0.0)
    idx = 7 + 85 * np.arange(T)
    fwd, rev = trot.copy(), trot.copy()
    fwd[idx] = recs
    rev[idx] = recs[::-1]
    alone = gpu_solve(solver_mod, prm, fwd)   # a fresh handle: no hint, one workgroup per entry
    assert_same(tuple(a[idx] for a in alone), base, label="batch of 16384, fresh handle")
    got_f, got_r = stale_hint_solves(solver_mod, prm, trot, [fwd, rev])
    assert_same(got_f, alone, label="stale hint (rest kernel)")
    assert_same(tuple(a[idx][::-1] for a in got_r), base, label="stale hint, records in the opposite order")
    got_i, = stale_hint_solves(solver_mod, prm, trot, [fwd], costs=np.repeat(cm.make_instance_costs(), B_HINT, axis=0))
    assert_same(got_i, alone, label="stale hint, per-instance kernels")


# ---- 3. a failing pivot -----------------------------------------------------------------------------
# (the weights of tests/test_gpu_c1_panel.py: they balance a foot's block, so that the failing pivot is
# not always the first or second)
PIVOT_WEIGHTS = (1, 1, 1, 10, 10, 10, 1, 1, 1, 600, 600, 600)
# The first rung is gentle: 2 alpha is 1e-4 .. 2e-4 of |H|, inside the band in which the status is not
# asserted, but three orders above the fp32 factorisation's own error (72 pivots x 6e-8), and under it
# the leading one-foot steps of LATE_STEPS keep their pivots, so the failure falls as late as the
# tables allow. The other rungs decide the sign (|smallest eigenvalue| > 1e-3 |H|).
ALPHA_LADDER = (-2e-4, -2e-3, -3e-3, -5e-3, -1e-2, -2e-2, -3e-2)
EIG_BAND = 1e-3
# stance feet per horizon step: one foot (3 variables, rank 3) in every leading step, the steps with
# four feet last; 22, 23 and 24 stance foot-steps. Float64 Cholesky of the oracle's condensation under
# alpha = -2e-4: the first failing pivot is 15 .. 22, where the random tables give 2 .. 9.
LATE_STEPS = {22: [1] * 6 + [4] * 4, 23: [1] * 5 + [2] + [4] * 4, 24: [1] * 4 + [2] * 2 + [4] * 4}


def late_tail_records(N, B, seed):
    """Tail-class records whose tables follow LATE_STEPS (feet chosen at random)."""
    rng = np.random.default_rng(seed)
    tab = np.zeros((B, N, 4), np.uint8)
    for b in range(B):
        for i, c in enumerate(LATE_STEPS[22 + b % 3]):
            tab[b, i, rng.choice(4, c, replace=False)] = 1
    recs = set_tables(package().make_instances(B, N, seed=seed, random_contact_frac=0.0), N, tab)
    assert set(reduced_sizes(recs, N)) == set(TAIL_SIZES)
    return recs


def lone_foot_records(N, B, seed, stress=False):
    """Class-1 records with one stance foot in step 0 and none after (n = 3). Their H is 3 x 3 with
    eigenvalues of the order of |H| (the foot's force moves every later state), so it stays positive
    definite down to alpha = -2e-2 under PIVOT_WEIGHTS (float64: smallest eigenvalue 0.04 .. 0.18 |H|
    from -2e-4 to -2e-2) and fails at -3e-2: the solving records beside the failing tail-class ones."""
    rng = np.random.default_rng(seed)
    tab = np.zeros((B, N, 4), np.uint8)
    tab[np.arange(B), 0, rng.integers(0, 4, size=B)] = 1
    return set_tables(package().make_instances(B, N, seed=seed, random_contact_frac=0.0, stress=stress), N, tab)


def first_failing_pivot(H):
    A = H.copy()
    for k in range(len(A)):
        if A[k, k] <= 0:
            return k
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k]) / A[k, k]
    return -1


def test_failing_pivot_raises_not_pd(cm, solver_mod):
    """24 tail-class records of random tables, 24 of LATE_STEPS tables and 16 lone-foot class-1 records.
    Smallest eigenvalue of the hook's H (float64, stance variables) below -1e-3 |H|: CMPC_NOT_PD, zero
    forces, no trips; above +1e-3 |H|: CMPC_OK; in between not asserted (the gentle first rung, and at
    most a fifth of the tail-class records over the deciding rungs). On every rung where records solve
    beside failing ones they keep the bits they have in a batch of solving records alone. The failing
    pivots (float64 elimination of the hook's H of the records that came back CMPC_NOT_PD) must spread
    from the first panel's to beyond pivot 14."""
    import torch
    N, BT, BC = 10, 48, 16
    recs = np.concatenate([tail_records(N, BT // 4, 2330, False), tail_records(N, BT // 4, 2331, True),
                           late_tail_records(N, BT // 2, 2333), lone_foot_records(N, BC, 2332)])
    B = len(recs)
    tail = np.arange(B) < BT
    stance = np.repeat(cm.unpack_gait(recs, N) != 0, 3, axis=1)
    d_recs = torch.from_numpy(np.ascontiguousarray(recs)).cuda()
    H = torch.zeros((B, 12 * N, 12 * N), dtype=torch.float32, device="cuda")
    g = torch.zeros((B, 12 * N), dtype=torch.float32, device="cuda")
    between = isolated = mixed_rungs = 0
    places, counts = set(), np.zeros(5, int)
    with closing(solver_mod.BatchSolver(cm.make_params(N), max_batch=B)) as s:
        for alpha in ALPHA_LADDER:
            s.set_params(cm.make_params(N, alpha=alpha, weights=PIVOT_WEIGHTS))
            s.condense(d_recs, H, g)
            torch.cuda.synchronize()
            f, st, it = s.solve_host(recs)
            counts += np.bincount(st[tail], minlength=5)[:5]
            H64 = H.cpu().numpy().astype(np.float64)
            for i in range(B):
                Hr = H64[i][np.ix_(stance[i], stance[i])]
                w = np.linalg.eigvalsh(Hr)
                r = w[0] / np.abs(w).max()
                if r < -EIG_BAND:
                    assert st[i] == NOT_PD and (bits(f[i]) == 0).all() and it[i] == 0, (alpha, i, r, st[i])
                elif r > EIG_BAND:
                    assert st[i] == OK, (alpha, i, r, st[i])
                elif alpha != ALPHA_LADDER[0]:
                    between += tail[i]
                if tail[i] and st[i] == NOT_PD:
                    assert (bits(f[i]) == 0).all() and it[i] == 0, (alpha, i)
                    places.add(first_failing_pivot(Hr))
            ok = st == OK
            if ok.any() and (st[tail] == NOT_PD).any():   # the clean records beside the failing ones keep their bits
                f_c, st_c, it_c = s.solve_host(recs[ok])
                assert (st_c == OK).all()
                np.testing.assert_array_equal(bits(f_c), bits(f[ok]))
                np.testing.assert_array_equal(it_c, it[ok])
                isolated += int(ok.sum())
                mixed_rungs += 1
    print(f"[tail-factor] failing pivots: tail-class records by status over the ladder {counts}, {between} of "
          f"{BT * (len(ALPHA_LADDER) - 1)} between the thresholds on the deciding rungs, failing pivots (float64) "
          f"{sorted(places)}; {isolated} solving records on {mixed_rungs} rungs compared with their solve alone")
    assert counts[NOT_PD] > 0 and counts[OK] == 0   # (2 B'SB of a tail-class record is singular: module doc)
    assert between * 5 <= BT * (len(ALPHA_LADDER) - 1), between
    assert mixed_rungs >= 5 and isolated >= 5 * BC, (mixed_rungs, isolated)   # lone_foot_records: -2e-3 .. -2e-2 at least
    assert min(places) <= 3 and max(places) >= 15, sorted(places)


def test_failing_records_in_the_looping_kernel_leave_the_rest(cm, solver_mod):
    """Under a shared alpha no tail-class record solves (module doc), so a clean record cannot follow a
    failed one inside the tail class's looping workgroups. What can be held: 192 failing tail-class
    records among 16384 lone-foot records behind a stale hint (128 of them through the rest kernel's 32
    looping workgroups, failed record after failed record in one LDS) all come back CMPC_NOT_PD with
    zero forces and no trips, and every solving record keeps the bits of the batch without them."""
    N = 10
    prm = cm.make_params(N, alpha=-5e-3, weights=PIVOT_WEIGHTS)
    comp = lone_foot_records(N, B_HINT, 2340)
    recs = form_records()
    idx = 7 + 85 * np.arange(len(recs))
    mixed = comp.copy()
    mixed[idx] = recs
    with closing(solver_mod.BatchSolver(cm.make_params(N), max_batch=B_HINT)) as s:
        s.set_params(prm)
        for _ in range(3):
            want = s.solve_host(comp)
        f, st, it = s.solve_host(mixed)
    assert (want[1] == OK).all(), np.bincount(want[1])
    assert (st[idx] == NOT_PD).all() and (bits(f[idx]) == 0).all() and (it[idx] == 0).all(), np.bincount(st[idx])
    rest = np.ones(B_HINT, bool)
    rest[idx] = False
    assert_same((f, st, it), want, rows=rest, label="solving records beside 192 failing tail-class records")
