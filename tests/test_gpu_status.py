"""GPU tests of the solve's failure contract (include/cmpc_solver.h CMPC_OK .. CMPC_BAD_INPUT,
INTEGRATION.md §4): a failed QP returns all-zero forces and a documented status byte, an instance
that reports CMPC_OK has finite, feasible forces, and a failed instance changes nothing of any
other, in the same launch or in a later one on the same handle.

The levers and the invariants are tests/status_cases.py's (alpha = -1: CMPC_NOT_PD; f_max = -120:
CMPC_INFEASIBLE; one record word NaN / +-Inf / 3e38: CMPC_BAD_INPUT, or CMPC_NOT_PD where the word
reaches qH; max_iter = 1: CMPC_MAX_ITER). Every comparison between two solves is on bit patterns;
every output buffer is pre-filled with sentinels, so a row the kernels leave alone shows.

The shapes are the smallest at which each build and launch form runs: random contact tables at
N = 10 / 16 / 20 in batches of 16384 (the sparse wide classes as persistent workgroups, class 1
split into its 60- and 64-wide builds) and 512 (one workgroup per entry, the single 64-wide class-1
build); eight n = 72 records for the tail class's one-workgroup hand-off launch; max_batch = 1
handles for the single-instance fast path and the reference ABI.

Kernel safety with non-finite input, from the code: every loop of classify, class 1, the tail class
and the wide classes is bounded by integers (the active set by max_iter + 2n trips, the refinement
by its constant cap of passes, the lists by their counts), and no address, lane index or trip count is
computed from a float (a NaN only ever loses a comparison: `sl < best`, `r > 0`, `zn > 1e-9 dn`,
`d > 0` all take their "no" side)."""
import ctypes

import numpy as np
import pytest

import status_cases as sc
from status_cases import BAD_INPUT, INFEASIBLE, MAX_ITER, NOT_PD, OK
from conftest import golden_params, load_golden, rel_force_err
from support import Dev, abi_floats, assert_due_result, assert_same, bits, records, solver_mod  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [(10, 512), (16, 512), (20, 512), (10, 16384), (16, 16384), (20, 16384)]


def poisoned(N, B):
    recs = sc.clean_batch(N, B)
    bad, cases = sc.poison_batch(recs, N, f_est=(N == 20))
    return recs, bad, cases


def test_gradient_only_nan_is_refused(cm, solver_mod):
    """A NaN in a word that reaches only the gradient (qH stays finite, every pivot passes): the
    instance must come back CMPC_BAD_INPUT with all-zero forces, never CMPC_OK with NaN forces."""
    N, B = 10, 64
    recs = sc.clean_batch(N, B)
    words = [l for l in sc.levers(N) if l[1] == "g"]
    bad = np.array(recs)
    for i in range(B):
        bad[i], _ = sc.poison(recs[i], words[i % len(words)][2], np.float32(np.nan))
    prm = cm.make_params(N)
    d = Dev(solver_mod, prm, B)
    try:
        f, st, it = d.run(bad)
    finally:
        d.close()
    nan_ok = int(((st == OK) & ~np.isfinite(f).all(axis=1)).sum())
    print(f"[status] g-only NaN, {B} records at N={N}: status {sc.status_counts(st)}, "
          f"{nan_ok} with status ok and non-finite forces")
    sc.check_invariants(bad, prm, f, st, it, label="g-only NaN")
    assert (st == BAD_INPUT).all(), sc.status_counts(st)


@pytest.mark.parametrize("N,B", SHAPES)
def test_poisoned_batch_statuses_and_isolation(cm, solver_mod, N, B):
    """Invariants 1-4 on the random-contact batches: clean solve, every 7th record poisoned
    (rotating through the levers' words and values, gait bytes kept), clean solve again, all on one
    handle. Every size class the batch holds has a poisoned record ahead of a clean one."""
    recs, bad, cases = poisoned(N, B)
    prm = cm.make_params(N)
    rows = sc.class_report(recs, N, cases)
    print(f"[status classes] N={N} B={B} (instances/poisoned): {sc.format_report(rows)}")
    assert [(lo, hi) for lo, hi, cnt, nb, pair in rows] == [(lo + 1, hi) for lo, hi, n in sc.expected_classes(N)]
    assert all(pair for lo, hi, cnt, nb, pair in rows), sc.format_report(rows)
    d = Dev(solver_mod, prm, B)
    try:
        clean = d.run(recs)
        got = d.run(bad)
        again = d.run(recs)
    finally:
        d.close()
    assert (clean[1] == OK).all(), sc.status_counts(clean[1])
    sc.check_invariants(recs, prm, *clean, label=f"clean N={N} B={B}")
    f, st, it = got
    print(f"[status] N={N} B={B}: {len(cases)} poisoned -> {sc.status_counts(st)}")
    sc.check_invariants(bad, prm, f, st, it, label=f"poisoned N={N} B={B}")
    sc.check_poisoned(cases, st, label=f"N={N} B={B}")
    touched = np.zeros(B, bool)
    touched[list(cases)] = True
    assert_same(got, clean, ~touched, label="untouched rows of the poisoned solve vs the clean solve")
    unused = np.zeros(B, bool)
    unused[[i for i, c in cases.items() if c[1] == "unused"]] = True
    assert_same(got, clean, unused, label="rows poisoned in a word the solve does not read")
    assert_same(again, clean, label="clean solve after the poisoned one")


@pytest.mark.parametrize("N", [10, 16, 20])
def test_due_output_steps_and_instance_builds_on_poisoned_batch(cm, solver_mod, N):
    """The status byte and the zero forces through the other ways out of the library, on the
    512-record poisoned batch: the due-masked solve (due rows as the unmasked solve, a poisoned row
    that is not due keeps its sentinels), set_output_steps(1) (a failed row is 12 zeros, status and
    iters unchanged) and the per-instance builds with a table of default rows (bit for bit the
    shared builds)."""
    B = 512
    recs, bad, cases = poisoned(N, B)
    prm = cm.make_params(N)
    d = Dev(solver_mod, prm, B)
    try:
        ref = d.run(bad)
        due = (np.arange(B) % 3 != 1).astype(np.uint8)
        due[sorted(cases)[::2]] = 0          # half of the poisoned rows are not due
        assert due[sorted(cases)].any() and not due[sorted(cases)].all()
        assert_due_result(d.run(bad, due), ref, due, d.cols)
        d.s.set_instance_params(records().make_instance_params(mass=np.full(B, 12.0)))
        assert d.s.instance_count == B
        assert_same(d.run(bad), ref, label="per-instance builds, default rows")
        assert_due_result(d.run(bad, due), ref, due, d.cols)
        d.s.set_instance_params(None)
        assert_same(d.run(bad), ref, label="shared builds after the table was cleared")
    finally:
        d.close()
    d1 = Dev(solver_mod, prm, B, out_steps=1)
    try:
        f1, st1, it1 = d1.run(bad)
    finally:
        d1.close()
    assert f1.shape == (B, 12)
    np.testing.assert_array_equal(st1, ref[1])
    np.testing.assert_array_equal(it1, ref[2])
    np.testing.assert_array_equal(bits(f1), bits(ref[0][:, :12]))
    assert (bits(f1[st1 != OK]) == 0).all()
    sc.check_invariants(bad, prm, f1, st1, it1, label=f"one output step N={N}")


def test_tail_handoff_workgroup_isolation(cm, solver_mod):
    """The eight n = 72 records whose active set outgrows the tail class's 64 lanes and which the
    single hand-off workgroup solves one after another. Records 1 and 4 poisoned (a gradient-only
    NaN, a NaN foot offset): the other six equal the clean run bit for bit. A poisoned record fails
    in the tail class itself (on its first trip, or at a pivot) and is never handed off, so the
    hand-off workgroup cannot see a failed instance ahead of a clean one: what this shows is that
    the tail class's failures leave the hand-off list and its six solves as they were."""
    N, B = 10, 8
    R = records()
    prm = cm.make_params(N)
    recs = sc.all_zero_force_records(cm, B, N)
    assert (sc.reduced_sizes(recs, N) == 72).all()
    bad = np.array(recs)
    bad[1, R.REC_V + 2] = np.nan
    bad[4, R.REC_R + 4 * 2 + 0] = np.nan   # r_z of leg 0 (in stance at steps 0-5)
    d = Dev(solver_mod, prm, B)
    try:
        clean = d.run(recs)
        got = d.run(bad)
        again = d.run(recs)
    finally:
        d.close()
    assert (clean[1] == OK).all() and (clean[2] > 64).all(), (clean[1], clean[2])   # every record is handed off
    f, st, it = got
    print(f"[status] tail hand-off: status {st.tolist()}, iters {it.tolist()}")
    sc.check_invariants(bad, prm, f, st, it, label="tail hand-off")
    assert st[1] == BAD_INPUT and st[4] in (BAD_INPUT, NOT_PD), st
    keep = np.ones(B, bool)
    keep[[1, 4]] = False
    assert_same(got, clean, keep, label="hand-off rows 0, 2, 3, 5, 6, 7")
    assert_same(again, clean, label="clean hand-off batch after the poisoned one")


@pytest.mark.parametrize("N", [10, 16, 20])
def test_single_instance_path_alternating(cm, solver_mod, N):
    """Up to six poisoned and six clean records per size class, one at a time on a max_batch = 1
    handle, poisoned and clean alternating: status, forces and iters equal the batched result, and
    a clean solve behind a failed one equals the same solve on a handle that never saw a failure."""
    B = 16384
    recs, bad, cases = poisoned(N, B)
    prm = cm.make_params(N)
    n = sc.reduced_sizes(recs, N)
    order, seen = [], []
    for lo, hi in zip(sc.CLASS_EDGES[:-1], sc.CLASS_EDGES[1:]):
        idx = np.nonzero((n > lo) & (n <= hi))[0]
        p = [int(i) for i in idx if int(i) in cases and cases[int(i)][1] != "unused"][:6]
        c = [int(i) for i in idx if int(i) not in cases][:6]
        if not idx.size:
            continue
        assert p and c, (lo, hi)
        seen.append(f"{lo + 1}-{hi}:{len(p)}p/{len(c)}c")
        for k in range(max(len(p), len(c))):   # poisoned, clean, poisoned, clean, ...
            order += [i for i in (p[k:k + 1] + c[k:k + 1])]
    print(f"[status] single-instance path N={N}: " + " ".join(seen))
    assert len(seen) == len(sc.expected_classes(N))
    sel = np.array(order)
    d = Dev(solver_mod, prm, len(sel))
    try:
        f_b, st_b, it_b = d.run(bad[sel])
    finally:
        d.close()
    sc.check_invariants(bad[sel], prm, f_b, st_b, it_b, label="batched comparator")
    s = solver_mod.BatchSolver(prm, max_batch=1)
    fresh = solver_mod.BatchSolver(prm, max_batch=1)
    try:
        for k, i in enumerate(sel):
            f1, st1, it1 = s.solve_host(bad[i:i + 1])
            assert st1[0] == st_b[k] and it1[0] == it_b[k], (i, cases.get(int(i)), st1[0], st_b[k], it1[0], it_b[k])
            assert np.array_equal(bits(f1[0]), bits(f_b[k])), (i, cases.get(int(i)))
            if int(i) in cases:
                assert st1[0] != OK and (bits(f1) == 0).all(), (i, cases[int(i)], st1[0])
            else:
                f2, st2, it2 = fresh.solve_host(bad[i:i + 1])
                assert st2[0] == st1[0] == OK and it2[0] == it1[0] and np.array_equal(bits(f2), bits(f1)), i
    finally:
        s.close()
        fresh.close()


@pytest.mark.parametrize("N", [10, 16, 20])
def test_alpha_minus_one_is_not_pd(cm, solver_mod, N):
    """qH = 2 (B'SB - I) is negative definite on every stance variable (tests/test_status_cases.py
    holds diag(B'SB) < 0.5 for these records): the first pivot fails in every build, the refining
    ones included. An all-swing instance has no QP and stays CMPC_OK with zero forces. The same
    handle then solves with the default alpha as a fresh handle does."""
    B = 512
    recs = sc.clean_batch(N, B)
    prm = cm.make_params(N, alpha=-1.0)
    n = sc.reduced_sizes(recs, N)
    d = Dev(solver_mod, prm, B)
    try:
        f, st, it = d.run(recs)
        d.s.set_params(cm.make_params(N))
        after = d.run(recs)
    finally:
        d.close()
    print(f"[status] alpha=-1 N={N}: {sc.status_counts(st)}")
    sc.check_invariants(recs, prm, f, st, it, label=f"alpha=-1 N={N}")
    assert (st[n > 0] == NOT_PD).all() and (st[n == 0] == OK).all(), sc.status_counts(st)
    assert (it == 0).all()
    d = Dev(solver_mod, cm.make_params(N), B)
    try:
        assert_same(after, d.run(recs), label="default alpha after alpha = -1 on one handle")
    finally:
        d.close()


@pytest.mark.parametrize("N", [10, 16, 20])
def test_negative_f_max_is_infeasible(cm, solver_mod, N):
    """f_max = -120 (the shared parameters are not validated): a stance foot-step has
    ub = gait * f_max < 0, and fz >= 0 excludes fz <= ub. Every instance with a stance foot-step is
    CMPC_INFEASIBLE with zero forces."""
    B = 512
    recs = sc.clean_batch(N, B)
    prm = cm.make_params(N, f_max=-120.0)
    n = sc.reduced_sizes(recs, N)
    d = Dev(solver_mod, prm, B)
    try:
        f, st, it = d.run(recs)
    finally:
        d.close()
    print(f"[status] f_max=-120 N={N}: {sc.status_counts(st)}, iters {int(it.min())}..{int(it.max())}")
    sc.check_invariants(recs, prm, f, st, it, label=f"f_max=-120 N={N}")
    assert (st[n > 0] == INFEASIBLE).all() and (st[n == 0] == OK).all(), sc.status_counts(st)


@pytest.mark.parametrize("N", [10, 16, 20])
def test_iteration_cap(cm, solver_mod, N):
    """max_iter = 1: the kernels allow max_iter + 2n trips, so every status is CMPC_OK or
    CMPC_MAX_ITER and iters <= 1 + 2n + 1; an instance that still ends CMPC_OK equals the
    max_iter = 100 result bit for bit, one that hits the cap has all-zero forces."""
    B = 512
    recs = sc.clean_batch(N, B)
    n = sc.reduced_sizes(recs, N)
    d = Dev(solver_mod, cm.make_params(N), B)
    try:
        full = d.run(recs)
        prm1 = cm.make_params(N, max_iter=1)
        d.s.set_params(prm1)
        f, st, it = d.run(recs)
    finally:
        d.close()
    print(f"[status] max_iter=1 N={N}: {sc.status_counts(st)} ({int((st == MAX_ITER).sum())} of {B} hit the cap)")
    assert np.isin(st, (OK, MAX_ITER)).all(), sc.status_counts(st)
    assert (it <= 1 + 2 * n + 1).all()
    sc.check_invariants(recs, prm1, f, st, it, label=f"max_iter=1 N={N}")
    assert (full[1] == OK).all()
    assert_same((f, st, it), full, st == OK, label="instances within the cap vs max_iter = 100")
    assert (bits(f[st == MAX_ITER]) == 0).all()


def test_reference_abi_failed_solve(cm, solver_mod, capfd):
    """The reference ABI: after a good solve, a call with a NaN in p prints the reference's
    `failed to solve!` and get_solution returns 0.0 for every force; a valid call afterwards matches
    the golden forces again."""
    N = 10
    g = load_golden("n10_mixed")
    prm = golden_params(cm, g)

    def call(rec):
        solver_mod.setup_problem(prm.dt, N, prm.mu, prm.f_max)
        solver_mod.update_x_drag(float(rec[28]))
        solver_mod.update_solver_settings(100, 1e-7, 1e-8, 1.5, 1e-5, 0)
        abi_floats(solver_mod, cm, rec, N, prm)
        return np.array([solver_mod.get_solution(j) for j in range(12 * N)])

    ok_rows = [i for i in range(len(g["status"])) if g["status"][i] == 0][:3]
    first = call(g["records"][ok_rows[0]])
    assert rel_force_err(first[None], g["q_ref"][ok_rows[0]][None]).max() <= 1e-4
    assert np.abs(first).max() > 1.0
    capfd.readouterr()
    bad = np.array(g["records"][ok_rows[1]])
    bad[records().REC_P + 1] = np.nan
    sol = call(bad)
    ctypes.CDLL(None).fflush(None)   # the library prints through C stdio, block-buffered into a capture file
    out = capfd.readouterr().out
    assert "failed to solve!" in out, out
    assert (sol == 0.0).all() and not np.signbit(sol).any()
    for i in ok_rows[1:]:
        sol = call(g["records"][i])
        assert rel_force_err(sol[None], g["q_ref"][i][None]).max() <= 1e-4
    ctypes.CDLL(None).fflush(None)
    assert "failed to solve!" not in capfd.readouterr().out
