"""The per-instance table (cmpc_batch_set_instance_params): mass, inertia, mu and f_max per instance.

Every other GPU test solves a batch of one robot on one ground. Here instance i takes row i of a table,
under the mix of tests/instance_mix.py (four combos of model, mu and f_max, rotated over the batch so
that every instance of every kernel family meets every combo), over param_sets.CASES, the smallest
batches that reach every kernel family. The comparisons are of bits unless stated otherwise:

 1. a table whose rows are all one combo is the shared handle of that combo (full and half due);
 2. under the mixed table, row i is row i of the shared handle of its combo solving the whole batch
    (every case, every rotation; with a due mask at N = 10 and N = 16);
 3. the mixed solve against the fp64 optimum of each row's own model and parameters
    (cost_mix.cpu_data with mix="model"; tests/test_instance_params_ref.py is its CPU side), at the project's
    gates: 1e-4 at N <= 10, 1e-5 from N = 11, status 0, swing legs exactly zero;
 4. one 16384-instance batch against four pieces of 4096 (the 60 / 64 split, the persistent builds);
 5. the life cycle: clear, set_params, set_model, batch > count, bad rows, an eliminating f_max;
 6. evaluate, condense (both modes), rollout, the config-5 residual and ADMM, row by row against the
    shared handles.
"""
import functools
import importlib

import numpy as np
import pytest

import cost_mix as cx
import instance_mix as im
import model_ref as mr
import param_sets as ps
import support
from support import (FP64_TOL, IT_FILL, REF_TOL, ST_FILL, TIGHT, assert_same_bits, bits, closing, half_due,  # noqa: F401
                     nan_where_not_due, package, row_by_row, sentinel_forces, sentinel_solve, solver,
                     solver_mod)

pytestmark = pytest.mark.gpu

NC = im.NC
shared = functools.partial(support.shared_handle, im)   # (k, N, B): a fresh shared handle of combo k
shared_solve = functools.partial(support.shared_solve, im)   # (k, case): its solve of the whole batch, cached
rowwise = functools.partial(support.rowwise, im)   # (case, ids): row i of the shared handle of combo ids[i]


def table_handle(N, B, tab):
    """A default handle (default model, mu 0.4, f_max 120) with the table set."""
    return solver().BatchSolver(package().make_params(N), max_batch=B, instance_params=tab)


# ---- 1: a uniform table is the shared handle ---------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["full", "due"])
@pytest.mark.parametrize("case", ["n10_families", "n16_trot", "n20_standing"])
def test_uniform_table_is_the_shared_handle(cm, solver_mod, case, masked):
    N = ps.CASES[case][0]
    recs = ps.case_records("default", case)
    B = len(recs)
    due = half_due(B) if masked else None
    rin = nan_where_not_due(recs, due) if masked else recs
    with closing(shared(1, N, B)) as s:
        want = sentinel_solve(s, rin, due)
        assert s.instance_count == 0
    m = np.ones(B, bool) if due is None else due != 0
    assert (want[1][m] == 0).mean() > 0.9 and (want[1][~m] == ST_FILL).all()
    np.testing.assert_array_equal(bits(want[0][~m]), bits(sentinel_forces(B, 12 * N)[~m]))
    with closing(table_handle(N, B, im.combo_rows(np.full(B, 1)))) as s:
        assert s.instance_count == B
        assert_same_bits(sentinel_solve(s, rin, due), want, "uniform table of combo 1")
    with closing(solver_mod.BatchSolver(cm.make_params(N), max_batch=B)) as s:
        assert not np.array_equal(bits(sentinel_solve(s, rin, due)[0])[m], bits(want[0])[m])   # combo 1 is not the default


# ---- 2: the mixed table, row by row -----------------------------------------------------------------
@pytest.mark.parametrize("s_rot", range(NC))
@pytest.mark.parametrize("case", list(ps.CASES))
def test_mixed_table_row_by_row(cm, solver_mod, case, s_rot):
    N = ps.CASES[case][0]
    recs = ps.case_records("default", case)
    B = len(recs)
    ids = im.combo_ids(B, s_rot)
    if case == "n10_families":
        counts = ps.family_counts(recs)
        assert min(counts) > 0, counts   # c1-60, c1-64, tail, w80, w96, w120
    want = rowwise(case, ids)
    with closing(table_handle(N, B, im.table(B, s_rot))) as s:
        got = sentinel_solve(s, recs)
    assert_same_bits(got, want, f"{case} rotation {s_rot}")
    assert (got[1] == 0).mean() > 0.9
    dflt = shared_solve(0, case)
    differ = (bits(got[0]) != bits(dflt[0])).any(1)
    assert differ[(ids != 0) & (got[1] == 0) & (np.abs(dflt[0]).max(1) > 0)].all()


@pytest.mark.parametrize("s_rot", [0, 3])
@pytest.mark.parametrize("case", ["n10_families", "n16_trot"])
def test_mixed_table_under_a_due_mask(cm, solver_mod, case, s_rot):
    N = ps.CASES[case][0]
    recs = ps.case_records("default", case)
    B = len(recs)
    ids = im.combo_ids(B, s_rot)
    due = half_due(B, seed=7 + s_rot)
    m = due != 0
    want = rowwise(case, ids)
    with closing(table_handle(N, B, im.table(B, s_rot))) as s:
        got = sentinel_solve(s, nan_where_not_due(recs, due), due)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(bits(g[m]), bits(w[m]))   # row i is row i of the table, mask or not
    np.testing.assert_array_equal(bits(got[0][~m]), bits(sentinel_forces(B, 12 * N)[~m]))
    assert (got[1][~m] == ST_FILL).all() and (got[2][~m] == IT_FILL).all()


# ---- 3: against the fp64 optimum of each row ---------------------------------------------------------
@pytest.mark.parametrize("case", list(ps.CASES))
def test_mixed_table_against_the_fp64_optimum(cm, orc, solver_mod, case):
    """Measured on an MI355X when this test was written: see DESIGN.md §3.3."""
    if not orc.ref_available():
        pytest.skip("oracle/_ref not present")
    d = cx.cpu_data(case, 0, mix="model")
    N, recs, ids, x64 = d["N"], d["recs"], d["ids"], d["x64"]
    assert (d["ri64"] == 0).all(), d["ri64"]
    with closing(table_handle(N, len(recs), im.table(len(recs), 0))) as s:
        f, st, it = sentinel_solve(s, recs)
    e64 = ps.rel_dist(f, x64)
    per = [float(e64[ids == k].max()) for k in range(NC)]
    print(f"[inst] {case}: {len(recs)} instances under the mix, ours within {e64.max():.1e} of the fp64 optimum "
          f"(per combo {', '.join(f'{v:.1e}' for v in per)}; mean iters {it.mean():.1f})")
    swing = np.repeat(cm.unpack_gait(recs, N) == 0, 3, axis=1)
    assert np.all(f[swing] == 0.0)
    assert (st == 0).all(), np.bincount(st)
    gate = REF_TOL if N <= 10 else FP64_TOL
    assert e64.max() <= gate, (float(e64.max()), int(e64.argmax()), int(ids[e64.argmax()]))


# ---- 4: launch forms ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [10, 16])
def test_launch_forms_agree_under_the_mix(cm, solver_mod, N):
    """test_gpu_model.test_launch_forms_agree_under_model under the rotated mix: one 16384-instance
    random-contact batch (at N = 10 the 60 / 64 split of class 1, the persistent sparse wide classes)
    against the same records and rows in four pieces of 4096 (one workgroup per entry)."""
    B, P = 16384, 4096
    prm = cm.make_params(N)
    recs = cm.make_instances(B, N, seed=8400 + N, random_contact_frac=1.0)
    tab = im.table(B, 1)
    with closing(solver_mod.BatchSolver(prm, max_batch=B, instance_params=tab)) as s:
        f_all, st_all, it_all = s.solve_host(recs)
    parts = []
    with closing(solver_mod.BatchSolver(prm, max_batch=P)) as s:
        for a in range(0, B, P):
            s.set_instance_params(tab[a:a + P])
            parts.append(s.solve_host(recs[a:a + P]))
    f_p, st_p, it_p = (np.concatenate([p[j] for p in parts]) for j in range(3))
    diff = np.nonzero((bits(f_p) != bits(f_all)).any(1) | (st_p != st_all) | (it_p != it_all))[0]
    assert diff.size == 0, (diff.size, diff[:8])
    assert (st_all == 0).mean() > 0.99
    with closing(solver_mod.BatchSolver(prm, max_batch=P)) as s:
        f_def = s.solve_host(recs[:P])[0]
    ids = im.combo_ids(P, 1)
    same = (bits(f_def) == bits(f_all[:P])).all(1)
    assert same[ids == 0].all()                       # combo 0 is the default handle
    assert not same[(ids != 0) & (np.abs(f_def).max(1) > 0)].any()


# ---- 5: life cycle -----------------------------------------------------------------------------------
def test_clear_and_survive(cm, solver_mod):
    recs10 = ps.case_records("default", "n10_families")
    recs16 = ps.case_records("default", "n16_trot")
    B = len(recs10)
    p10, p16 = cm.make_params(10), cm.make_params(16)
    tab = im.table(B, 2)
    want10 = rowwise("n10_families", im.combo_ids(B, 2))
    want16 = rowwise("n16_trot", im.combo_ids(len(recs16), 2))
    with closing(solver_mod.BatchSolver(p10, max_batch=B)) as s:
        fresh = sentinel_solve(s, recs10)
        s.set_instance_params(tab)
        assert s.instance_count == B
        assert_same_bits(sentinel_solve(s, recs10), want10, "table set")
        s.set_params(p16)                                  # the table survives set_params ...
        assert s.instance_count == B
        assert_same_bits(sentinel_solve(s, recs16), want16, "N = 16 under the same table")
        s.set_params(p10)
        assert_same_bits(sentinel_solve(s, recs10), want10, "back at N = 10")
        s.set_model(mr.model("x2"))                        # ... and set_model, which stays hidden
        assert s.model.mass == 24.0
        assert_same_bits(sentinel_solve(s, recs10), want10, "set_model under a table")
        s.set_model(None)
        s.set_instance_params(None)                        # clear: a fresh handle's bits
        assert s.instance_count == 0
        assert_same_bits(sentinel_solve(s, recs10), fresh, "cleared")
        s.set_model(mr.model("heavy"))
        s.set_params(im.combo_params(1, 10))
        s.set_instance_params(tab)
        s.set_instance_params(None)                        # what was set under the table shows again
        assert_same_bits(sentinel_solve(s, recs10), shared_solve(1, "n10_families"), "shared values after a clear")


def test_batch_beyond_the_table_is_refused(cm, solver_mod):
    import torch
    recs = ps.case_records("default", "n3_padding")
    B = len(recs)
    with closing(solver_mod.BatchSolver(cm.make_params(3), max_batch=B)) as s:
        s.set_instance_params(im.table(B - 8, 0))
        assert s.instance_count == B - 8
        r = torch.from_numpy(np.array(recs)).cuda()
        f = torch.from_numpy(sentinel_forces(B, 36)).cuda()
        st = torch.full((B,), ST_FILL, dtype=torch.uint8, device="cuda")
        it = torch.full((B,), IT_FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(solver_mod.CmpcError, match=r"\(-1\)"):
            s.solve(r, f, st, it)
        with pytest.raises(solver_mod.CmpcError, match=r"\(-1\)"):
            s.solve(r, f, st, it, due=torch.ones(B, dtype=torch.uint8, device="cuda"))
        with pytest.raises(solver_mod.CmpcError):
            s.solve_host(recs)
        with pytest.raises(solver_mod.CmpcError):
            s.evaluate_host(recs, np.zeros((B, 36), np.float32))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bits(f.cpu().numpy()), bits(sentinel_forces(B, 36)))
        assert (st.cpu().numpy() == ST_FILL).all() and (it.cpu().numpy() == IT_FILL).all()
        got = s.solve_host(recs[:B - 8])                   # within the table: solved
        assert (got[1] == 0).mean() > 0.9
        with pytest.raises(solver_mod.CmpcError, match=r"\(-1\)"):
            s.set_instance_params(im.table(B + 1, 0))       # count > max_batch
        assert s.instance_count == B - 8


def test_bad_rows_are_rejected(cm, solver_mod):
    """Every bad model of test_gpu_model.test_bad_models_are_rejected, plus mu <= 0, a NaN f_max and a
    non-finite mu, at a middle row: -2, and the previous table (or none) stays in force."""
    recs = ps.case_records("default", "n3_padding")
    B = len(recs)
    good = im.table(B, 1)
    nan, inf = float("nan"), float("inf")
    D = list(mr.DEFAULT[1])
    bad_rows = [[0.0] + D + [0.4, 120.0], [-1.0] + D + [0.4, 120.0], [12.0, 0.07, -0.26, 0.242, 0.4, 120.0],
                [nan] + D + [0.4, 120.0], [12.0, 0.07, 0.26, nan, 0.4, 120.0], [inf] + D + [0.4, 120.0],
                [12.0, 0.0, 0.26, 0.242, 0.4, 120.0],
                # positive and finite, but 1.f / (float) mass and 1.0 / inertia overflow
                [1e-39] + D + [0.4, 120.0], [12.0, 1e-310, 0.26, 0.242, 0.4, 120.0],
                [12.0] + D + [0.0, 120.0], [12.0] + D + [-0.4, 120.0], [12.0] + D + [0.4, nan],
                [12.0] + D + [nan, 120.0], [12.0] + D + [0.4, inf], [12.0] + D + [1e-50, 120.0]]
    with closing(solver_mod.BatchSolver(cm.make_params(3), max_batch=B)) as s:
        fresh = sentinel_solve(s, recs)
        for row in bad_rows[:3]:                            # no table yet: none afterwards
            t = good.copy()
            t[B // 2] = row
            with pytest.raises(solver_mod.CmpcError, match=r"\(-2\)"):
                s.set_instance_params(t)
            assert s.instance_count == 0
        assert_same_bits(sentinel_solve(s, recs), fresh, "a rejected first table")
        s.set_instance_params(good)
        want = sentinel_solve(s, recs)
        assert not np.array_equal(bits(want[0]), bits(fresh[0]))
        for row in bad_rows:
            t = im.table(B, 2)
            t[B // 2] = row
            with pytest.raises(solver_mod.CmpcError, match=r"\(-2\)"):
                s.set_instance_params(t)
            assert s.instance_count == B
        assert_same_bits(sentinel_solve(s, recs), want, "after rejected tables")
    with pytest.raises(solver_mod.CmpcError):
        bad = good.copy()
        bad[0, 0] = -1.0
        solver_mod.BatchSolver(cm.make_params(3), max_batch=B, instance_params=bad)


def test_an_eliminating_f_max_is_that_instance_alone(cm, solver_mod):
    """A row with f_max = 0.005 (|gait x f_max| < 0.01: every foot-step eliminated) gives zero forces
    and status 0 for that instance; every other row keeps its bits."""
    case = "n10_families"
    recs = ps.case_records("default", case)
    B = len(recs)
    ids = im.combo_ids(B, 0)
    want = rowwise(case, ids)
    tab = im.table(B, 0)
    hit = [3, B // 2, B - 1]
    tab[hit, cm.INST_FMAX] = 0.005
    with closing(table_handle(10, B, tab)) as s:
        f, st, it = sentinel_solve(s, recs)
    keep = np.ones(B, bool)
    keep[hit] = False
    assert (f[hit] == 0.0).all() and (st[hit] == 0).all()
    for g, w in zip((f, st, it), want):
        np.testing.assert_array_equal(bits(g[keep]), bits(w[keep]))


# ---- 6: the other entry points, row by row against the shared handles --------------------------------
@pytest.mark.parametrize("case,k", [("n10_families", 32), ("n20_standing", 4)])
def test_evaluate_row_by_row(cm, solver_mod, case, k):
    N = ps.CASES[case][0]
    recs = ps.case_records("default", case)[:k]
    ids = im.combo_ids(k, 1)
    f = rowwise(case, im.combo_ids(len(ps.case_records("default", case)), 1))[0][:k]
    got, want, outs = row_by_row(lambda s: s.evaluate_host(recs, f), lambda c: shared(c, N, k),
                                 lambda: table_handle(N, k, im.table(k, 1)), ids, NC)
    np.testing.assert_array_equal(bits(got[0]), bits(want[0]))                       # x_pred
    np.testing.assert_array_equal(got[1].view(np.uint64), want[1].view(np.uint64))   # all eight words
    assert not np.array_equal(got[1][ids != 0], outs[0][1][ids != 0])


@pytest.mark.parametrize("rows", [False, True], ids=["mirrored", "rows"])
@pytest.mark.parametrize("N", [3, 10])
def test_condense_row_by_row(cm, solver_mod, N, rows):
    import torch
    B = 8
    recs_np = cm.make_instances(B, N, seed=9500 + N, random_contact_frac=1.0)
    recs = torch.from_numpy(recs_np).cuda()
    ids = im.combo_ids(B, 3)

    def hook(s):
        H = torch.zeros((B, 12 * N, 12 * N), dtype=torch.float32, device="cuda")
        g = torch.zeros((B, 12 * N), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        s.condense(recs, H, g, rows=rows)
        torch.cuda.synchronize()
        return H.cpu().numpy(), g.cpu().numpy()

    got, want, outs = row_by_row(hook, lambda c: shared(c, N, B),
                                 lambda: table_handle(N, B, im.table(B, 3)), ids, NC)
    assert_same_bits(got, want, "condense")
    assert not np.array_equal(got[0][ids != 0], outs[0][0][ids != 0])


def test_rollout_row_by_row(cm, solver_mod):
    import torch
    inst = importlib.import_module("quad-periodic-mpc_amd.instances")
    N, B = 10, 96
    recs = cm.make_instances(B, N, seed=9577)
    g = np.random.Generator(np.random.Philox(12))
    u = np.zeros((B, 12 * N), np.float32)
    u[:, :12] = g.normal(0, 20, (B, 12))
    xi = g.normal(0, 2, (B, 6)).astype(np.float32)
    due = np.zeros(B, np.uint8)
    due[g.choice(B, 64, replace=False)] = 1
    loco = inst.make_loco_states(B, seed=10)
    ids = im.combo_ids(B, 2)
    d_rec, d_u, d_xi, d_due = (torch.from_numpy(a).cuda() for a in (recs, u, xi, due))

    def step(s):
        d_loco = torch.from_numpy(loco.copy()).cuda()
        torch.cuda.synchronize()
        s.rollout(d_loco, d_rec, d_u, xi6=d_xi, due=d_due)
        torch.cuda.synchronize()
        return d_loco.cpu().numpy()

    got, want, outs = row_by_row(step, lambda c: shared(c, N, B),
                                 lambda: table_handle(N, B, im.table(B, 2)), ids, NC)
    np.testing.assert_array_equal(bits(got), bits(want))
    np.testing.assert_array_equal(bits(got[due == 0]), bits(loco[due == 0]))
    m = (due != 0) & (ids != 0)
    assert (bits(got[m]) != bits(outs[0][m])).any(1).all()


def test_residual_row_by_row(cm, solver_mod):
    import torch
    N, B = 20, 64
    recs = cm.make_instances(B, N, seed=9588)
    logs = cm.make_logs(recs, seed=9589)
    ids = im.combo_ids(B, 1)
    due = half_due(B, seed=3)

    def resid(s, masked):
        d_rec = torch.from_numpy(np.array(recs, np.float32)).cuda()
        d_log = torch.from_numpy(np.ascontiguousarray(logs)).cuda()
        est = torch.zeros((B, 816), dtype=torch.float32, device="cuda")
        fext6 = torch.full((B, 6), np.nan, dtype=torch.float32, device="cuda")
        dd = torch.from_numpy(due).cuda() if masked else None
        torch.cuda.synchronize()
        s.estimate(est, d_rec, logs=d_log, sim_time=1.0, fext6=fext6, due=dd)
        torch.cuda.synchronize()
        return fext6.cpu().numpy()

    # (every handle runs both forms, the masked one behind the full one; the shared handles' masked output is not used)
    got, want, outs = row_by_row(lambda s: (resid(s, False), resid(s, True)), lambda c: shared(c, N, B),
                                 lambda: table_handle(N, B, im.table(B, 1)), ids, NC)
    (got, got_due), want, outs = got, want[0], [o[0] for o in outs]
    np.testing.assert_array_equal(bits(got), bits(want))
    np.testing.assert_array_equal(bits(got_due[due != 0]), bits(want[due != 0]))
    assert np.isnan(got_due[due == 0]).all()
    # the mass and inertia reach the residual (mu and f_max do not enter it)
    assert (bits(got[ids != 0]) != bits(outs[0][ids != 0])).any(1).all()


def test_admm_row_by_row(cm, solver_mod):
    import torch
    N, B = 3, 16
    recs_np = cm.make_instances(B, N, seed=9599)
    recs = torch.from_numpy(np.ascontiguousarray(recs_np)).cuda()
    ids = im.combo_ids(B, 0)

    def admm(s):
        H = torch.empty((B, 12 * N, 12 * N), dtype=torch.float32, device="cuda")
        gv = torch.empty((B, 12 * N), dtype=torch.float32, device="cuda")
        f = torch.empty((B, 12 * N), dtype=torch.float32, device="cuda")
        status = torch.empty(B, dtype=torch.uint8, device="cuda")
        iters = torch.empty(B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s.condense(recs, H, gv)
        s.admm(recs, H, gv, f, status, iters, settings=solver_mod.admm_settings(**TIGHT))
        torch.cuda.synchronize()
        return f.cpu().numpy(), status.cpu().numpy(), iters.cpu().numpy()

    got, want, outs = row_by_row(admm, lambda c: shared(c, N, B),
                                 lambda: table_handle(N, B, im.table(B, 0)), ids, NC)
    assert_same_bits(got, want, "admm")
    assert (bits(got[0][ids != 0]) != bits(outs[0][0][ids != 0])).any(1).all()
