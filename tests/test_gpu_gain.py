"""BatchSolver.gain (cmpc_batch_gain) and BatchSolver.feedback (cmpc_batch_feedback): the fp64 Riccati
gain against the numpy reference of tests/gain_ref.py at the same forces, its invariances, the
per-instance tables, the contract, solve -> gain end to end, and the feedback law against its numpy
restatement and against a second solve at the moved state.

The parity bar (gain_cases.bar(N)): per instance |G - ref|_inf <= bar max(|ref|_inf, tiny) over the 144
words of G; FREE and FREE0 exact; SLACK bit for bit (the slack's products are exact in fp64 and its
square root and division correctly rounded on both sides). bar(N) = 300 x the largest disagreement of
the reference's own two paths (dense KKT against Riccati) at horizon N: 4.2e-13 at N = 1, 3.3e-13 at 2,
5.7e-12 at 10, 3.9e-12 at 11, 4.5e-11 at 16, 6.6e-9 at 20. The reference is the Riccati path.
"""
import functools

import numpy as np
import pytest

import cost_mix as cx
import gain_cases as gc
import gain_ref as gr
import instance_mix as im
import sensitivity_ref as sr
from conftest import golden_params, load_golden
from support import closing, needs_ref, row_by_row, solver_mod  # noqa: F401

pytestmark = pytest.mark.gpu

BATCHES = [1, 3, 130]
FILL = -1.0


def run(s, recs, U, act_tol=gc.ACT_TOL):
    """One device call into a sentinel-filled output -> gain [B, GAIN_WORDS] as numpy."""
    import torch
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) for a in (recs, U)]
    o = torch.full((recs.shape[0], gr.WORDS), FILL, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()   # the fill is done before the handle's own stream writes
    s.gain(t[0], t[1], o, act_tol=act_tol)
    torch.cuda.synchronize()
    return o.cpu().numpy()


def fresh(solver_mod, prm, recs, U, max_batch=None, **kw):
    with closing(solver_mod.BatchSolver(prm, max_batch=max_batch or len(recs))) as s:
        return run(s, recs, U, **kw)


def same_bits(a, b, label=""):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64),
                                  err_msg=label)


def assert_parity(got, ref, N, label):
    """-> the worst ratio to the bar."""
    assert np.isfinite(got[:, :144]).all() and (got[:, 147] == 0).all(), label
    np.testing.assert_array_equal(got[:, gr.FREE], ref[:, gr.FREE], err_msg=label)
    np.testing.assert_array_equal(got[:, gr.FREE0], ref[:, gr.FREE0], err_msg=label)
    same_bits(got[:, gr.SLACK], ref[:, gr.SLACK], label + " slack")
    zero = ref[:, :144] == 0
    assert (got[:, :144][zero] == 0).all(), label
    r = np.array([gc.rel(g, w) for g, w in zip(got, ref)]) / gc.bar(N)
    print(f"[gain] {label}: worst ratio to the bar {r.max():.2e} (N = {N}, instance {int(r.argmax())})")
    assert r.max() <= 1.0, (label, int(r.argmax()), float(r.max()))
    return float(r.max())


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", gc.CASES)
def test_parity_with_reference(cm, orc, solver_mod, case, B):
    p = gc.pool(cm, orc, case)
    K = len(p["recs"])
    # the batch of 130 wraps the pool; the batch of 3 starts at the hand-built faces
    idx = (np.arange(B) + (min(p["m_faces"]) if B == 3 else 0)) % K
    got = fresh(solver_mod, p["prm"], p["recs"][idx], p["U"][idx])
    assert_parity(got, p["gric"][idx], p["prm"].horizon, f"{case} B={B}")
    for j, i in enumerate(idx):
        if int(i) in p["m_faces"]:   # the structure of every face type, on the kernel's own output
            assert got[j, gr.FREE] == p["m_faces"][int(i)], (case, j)
            gc.structure(cm, p, int(i), got[j])


@pytest.mark.parametrize("case", ["n10_edge", "n20_mixed"])
def test_invariance_bitwise(cm, orc, solver_mod, case):
    p = gc.pool(cm, orc, case)
    prm = p["prm"]
    N = prm.horizon
    idx = np.arange(130) % len(p["recs"])
    recs, U = p["recs"][idx], p["U"][idx]
    # the words G does not depend on: trajectory, p, v, w, f_est(3), the flag word
    dirty = recs.copy()
    dirty[:, 32:32 + 12 * N] = np.nan
    dirty[:, 0:6] = np.nan
    dirty[:, 10:13] = np.nan
    dirty[:, 29:31] = np.nan
    with closing(solver_mod.BatchSolver(prm, max_batch=130)) as s:
        a = run(s, recs, U)
        same_bits(a, run(s, recs, U), "the same call twice")
        same_bits(a, s.gain_host(recs, U), "host form")
        same_bits(a, run(s, dirty, U), "NaN in the words G does not read")
        s.set_instance_params(im.combo_rows(np.zeros(130, int)))
        s.set_instance_costs(cx.combo_rows(np.zeros(130, int)))
        same_bits(a, run(s, recs, U), "tables of default rows")
    assert np.abs(a[:, :144]).max() > 0
    # an instance alone against the same instance inside the batch (a larger handle, too)
    for i in (0, 77, 129):
        same_bits(a[i:i + 1], fresh(solver_mod, prm, recs[i:i + 1], U[i:i + 1], max_batch=64), f"instance {i} alone")


def test_gain_last_matches_batched(cm, solver_mod):
    """cmpc_gain_last after the single-instance protocol, bit for bit the batched call on the same
    record and the forces get_solution returns."""
    N = 10
    prm = cm.make_params(N)
    rec = load_golden("n10_mixed")["records"][1].copy()
    solver_mod.setup_problem(0.026, N, 0.4, 120)
    solver_mod.update_x_drag(float(rec[28]))
    solver_mod.update_solver_settings(100, 1e-7, 1e-8, 1.5, 1e-5, 0)
    gait = cm.unpack_gait(rec[None], N)[0].astype(np.int32)
    solver_mod.update_problem_data_floats(rec[0:3], rec[3:6], rec[6:10], rec[10:13], rec[13:25],
                                          rec[25], rec[26], rec[27], np.array(prm.weights),
                                          rec[32:32 + 12 * N], prm.alpha, gait)
    sol = np.array([solver_mod.get_solution(j) for j in range(12 * N)]).astype(np.float32)
    gain = solver_mod.gain_last()
    with closing(solver_mod.BatchSolver(prm, max_batch=1)) as s:
        gb = s.gain_host(rec[None], sol[None])
    assert gain.shape == (gr.WORDS,) and gain[gr.FREE0] > 0 and np.abs(gain[:144]).max() > 0
    same_bits(gain, gb[0])


def test_both_tables_row_by_row(cm, orc, solver_mod):
    """Both per-instance tables set (the 16 pairs of cost_mix.pair_ids): instance i equals, bit for
    bit, the shared handle that holds row i's values."""
    p = gc.pool(cm, orc, "n10_edge")
    N, B = 10, 32
    idx = np.arange(B) % len(p["recs"])
    recs, U = p["recs"][idx], p["U"][idx]
    mids, cids = cx.pair_ids(B)

    def table():
        s = solver_mod.BatchSolver(cm.make_params(N), max_batch=B)
        s.set_instance_params(im.combo_rows(mids))
        s.set_instance_costs(cx.combo_rows(cids))
        return s

    def shared(k):
        km, kc = k % im.NC, k // im.NC
        return solver_mod.BatchSolver(cx.pair_params(km, kc, N), max_batch=B, model=im.combo_model(km))

    got, want, outs = row_by_row(functools.partial(run, recs=recs, U=U), shared, table, mids + im.NC * cids,
                                 im.NC * cx.NC)
    same_bits(got, want, "tables against shared handles")
    # the same record under two pairs gives two answers: the tables are read
    K = len(p["recs"])
    assert K < B and any((want[i, :144] != want[i + K, :144]).any() for i in range(B - K))


def test_contract(cm, orc, solver_mod):
    """Every error return with d_gain untouched; NaN forces; all-zero forces."""
    import torch
    p = gc.pool(cm, orc, "n10_edge")
    dev = torch.device("cuda:0")
    d_rec, d_u = (torch.from_numpy(a[:4].copy()).to(dev) for a in (p["recs"], p["U"]))
    d_g = torch.full((4, gr.WORDS), FILL, dtype=torch.float64, device=dev)
    d_x = torch.zeros((4, 12), dtype=torch.float32, device=dev)
    d_o = torch.full((4, 12), FILL, dtype=torch.float32, device=dev)
    call = lambda s, batch, tol, gain, rec=d_rec.data_ptr(), u=d_u.data_ptr(): s.lib.cmpc_batch_gain(   # noqa: E731
        s._h, rec, u, batch, tol, gain)
    fb = lambda s, batch, rec, u, g, x, o: s.lib.cmpc_batch_feedback(s._h, rec, u, g, x, None, batch, o)  # noqa: E731
    with closing(solver_mod.BatchSolver(p["prm"], max_batch=4)) as s:
        torch.cuda.synchronize()
        g = d_g.data_ptr()
        assert call(s, 5, 1e-3, g) < 0                       # batch > max_batch
        assert call(s, -1, 1e-3, g) < 0
        assert call(s, 4, 1e-3, None) < 0                    # a NULL argument
        assert call(s, 4, 1e-3, g, rec=None) < 0
        assert call(s, 4, 1e-3, g, u=None) < 0
        assert call(s, 4, -1.0, g) == -2
        assert call(s, 4, float("nan"), g) == -2
        assert call(s, 4, float("inf"), g) == -2
        with pytest.raises(solver_mod.CmpcError):
            s.gain(d_rec, d_u, d_g, act_tol=-1e-3)
        with pytest.raises(solver_mod.CmpcError):
            s.gain(d_rec, d_u, d_g, batch=5)
        ptrs = [t.data_ptr() for t in (d_rec, d_u, d_g, d_x, d_o)]
        assert fb(s, 5, *ptrs) < 0 and fb(s, -1, *ptrs) < 0
        for j in range(5):
            assert fb(s, 4, *[None if i == j else q for i, q in enumerate(ptrs)]) < 0, j
        assert fb(s, 3, ptrs[0], ptrs[1], ptrs[2] + 8, ptrs[3], ptrs[4]) < 0   # d_gain off its 16-byte alignment
        s.set_output_steps(1)                                # no full solution
        assert call(s, 4, 1e-3, g) == -3
        with pytest.raises(solver_mod.CmpcError):
            s.gain_host(p["recs"][:4], p["U"][:4])
        s.set_output_steps(0)
        s.set_instance_costs(cx.combo_rows(np.zeros(2, int)))  # a table of two rows
        assert call(s, 4, 1e-3, g) < 0
        assert fb(s, 4, *ptrs) < 0
        torch.cuda.synchronize()
        assert (d_g == FILL).all() and (d_o == FILL).all()   # nothing was launched
        assert call(s, 2, 0.0, g) == 0                       # act_tol = 0 is allowed
        torch.cuda.synchronize()
        assert (d_g[:2, gr.FREE] >= 0).all() and (d_g[2:] == FILL).all()
    recs, U = p["recs"][:6].copy(), p["U"][:6].copy()
    clean = fresh(solver_mod, p["prm"], recs, U)
    U[1, 7] = np.nan
    U[3, 12 * 6 + 2] = np.inf    # a force of a later step
    U[4] = 0.0
    got = fresh(solver_mod, p["prm"], recs, U)
    for i in (1, 3):
        assert np.isnan(got[i, :144]).all() and np.isnan(got[i, gr.SLACK]), i
        assert 0 <= got[i, gr.FREE0] <= 12 and got[i, gr.FREE0] <= got[i, gr.FREE] <= 120 and got[i, 147] == 0, i
    assert not got[4, :144].any() and not np.signbit(got[4, :144]).any() and got[4, gr.FREE] == 0
    for i in (0, 2, 5):
        same_bits(clean[i], got[i], f"instance {i}")


@pytest.mark.parametrize("name", gc.E2E_SETS)
def test_solve_then_gain(cm, orc, solver_mod, needs_ref, name):
    """The handle's own forces go in, on six golden instances: FREE is the dimension of the fp64
    optimum's face (at 1e-6 N), and G meets the parity bar against the reference evaluated at the
    solver's forces."""
    g = load_golden(name)
    prm = golden_params(cm, g)
    recs = g["records"][:6]
    with closing(solver_mod.BatchSolver(prm, max_batch=6)) as s:
        f, st, _ = s.solve_host(recs)
        assert (st == 0).all()
        got = run(s, recs, f, act_tol=1e-3)
    for i in range(6):
        x64, _ = orc.fp64_solve(recs[i], prm)
        _, d64, _ = sr.face(recs[i], prm, x64, 1e-6)
        assert got[i, gr.FREE] == d64.sum() and got[i, gr.FREE0] == d64[:4].sum(), (name, i)
    ref = np.array([gr.riccati(orc, r, prm, u, 1e-3) for r, u in zip(recs, f)])
    assert_parity(got, ref, prm.horizon, f"{name} solve -> gain")


# ---- feedback ---------------------------------------------------------------------------------------
def run_feedback(s, recs, forces, gain, states, due=None):
    """One device call into a sentinel-filled output -> u [B, 12] float32 as numpy."""
    import torch
    dev = torch.device("cuda:0")
    B = recs.shape[0]
    t = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) for a in (recs, forces, states)]
    d_g = torch.from_numpy(np.ascontiguousarray(gain, np.float64)).to(dev)
    d_due = None if due is None else torch.from_numpy(np.ascontiguousarray(due, np.uint8)).to(dev)
    o = torch.full((B, 12), FILL, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    s.feedback(t[0], t[1], d_g, t[2], o, due=d_due)
    torch.cuda.synchronize()
    return o.cpu().numpy()


def assert_one_ulp(got, ref, label):
    """Each word within one fp32 ulp of the reference (fp64 sums in another order, rounded once)."""
    ulp = np.spacing(np.maximum(np.abs(ref), np.abs(got)).astype(np.float32))
    bad = np.abs(got.astype(np.float64) - ref.astype(np.float64)) > ulp
    assert not bad.any(), (label, np.argwhere(bad)[:8].tolist(), got[bad][:8], ref[bad][:8])


def test_feedback_against_reference(cm, orc, solver_mod):
    """cmpc_batch_feedback against gain_ref.feedback over 130 instances of the pool: a small random
    delta; a yaw difference across +-pi; a delta large enough for the guard to clamp fz at 0 and at ub;
    swing feet exactly +0.0; due instances keep their sentinel; NULL due writes every instance."""
    p = gc.pool(cm, orc, "n10_edge")
    prm = p["prm"]
    N, B = prm.horizon, 130
    rng = np.random.default_rng(615)
    idx = np.arange(B) % len(p["recs"])
    recs, U = p["recs"][idx].copy(), p["U"][idx]
    # instances 40..59: the record's yaw just below +pi, the state's just above -pi
    psi = np.pi - 0.005
    recs[40:60, 6:10] = np.array([np.cos(psi / 2), 0.0, 0.0, np.sin(psi / 2)], np.float32)
    x0 = np.array([gr.x0(orc, r, prm) for r in recs])
    delta = 1e-2 * rng.standard_normal((B, 12))
    delta[60:80] = 0.0
    delta[60:80, 5] = np.where(np.arange(20) % 2, 1.0, -1.0)    # p_z by +-1 m
    delta[60:80, 11] = np.where(np.arange(20) % 2, 2.0, -2.0)   # v_z by +-2 m/s
    states = (x0 + delta).astype(np.float32)
    states[40:60, 2] = np.float32(-np.pi + 0.005)
    due = (rng.random(B) < 0.3).astype(np.uint8)
    due[[40, 41, 60, 61]] = 0
    with closing(solver_mod.BatchSolver(prm, max_batch=B)) as s:
        gain = run(s, recs, U)
        got = run_feedback(s, recs, U, gain, states, due)
        every = run_feedback(s, recs, U, gain, states)
        s.set_output_steps(1)   # the forces at the handle's output stride: step 0 alone
        step0 = run_feedback(s, recs, U[:, :12], gain, states, due)
    ref = np.array([gr.feedback(orc, r, prm, u[:12], g, x) for r, u, g, x in zip(recs, U, gain, states)])
    live = due == 0
    assert live.sum() > 60 and (~live).sum() > 20
    assert (got[~live] == FILL).all()
    assert_one_ulp(got[live], ref[live], "masked")
    assert_one_ulp(every, ref, "NULL due")
    np.testing.assert_array_equal(got.view(np.uint32), step0.view(np.uint32))
    np.testing.assert_array_equal(got[live].view(np.uint32), every[live].view(np.uint32))
    swing = np.repeat(cm.unpack_gait(recs, N)[:, :4] == 0, 3, axis=1)
    assert swing.any() and (every[swing] == 0).all() and not np.signbit(every[swing]).any()
    # the cases are what they claim to be
    raw = states[40:60, 2].astype(np.float64) - x0[40:60, 2]
    assert (np.abs(raw) > 6.0).all() and np.abs(gain[40:60, :144]).max() > 0
    ub = float(np.float32(prm.f_max))
    rawf = U[60:80, :12].astype(np.float64) + np.einsum("bij,bj->bi", gain[60:80, :144].reshape(-1, 12, 12),
                                                        states[60:80].astype(np.float64) - x0[60:80])
    st = ~swing[60:80, 2::3]
    assert (rawf[:, 2::3][st] < 0).any() and (rawf[:, 2::3][st] > ub).any()
    assert (every[60:80, 2::3] >= 0).all() and (every[60:80, 2::3] <= ub).all()


def test_feedback_parameter_table_row_by_row(cm, orc, solver_mod):
    """With the per-instance parameter table set (instance_mix: mu 0.4 / 0.6 / 0.2 / 0.8, f_max 120 / 150 /
    120 / 60), instance i's guard uses row i's mu and f_max: bit for bit the shared handle of row i's
    combo, on one gain and on deltas half of which drive the guard into its clamps."""
    p = gc.pool(cm, orc, "n10_edge")
    N, B = 10, 64
    idx = np.arange(B) % len(p["recs"])
    recs, U = p["recs"][idx], p["U"][idx]
    x0 = np.array([gr.x0(orc, r, p["prm"]) for r in recs])
    delta = 1e-2 * np.random.default_rng(77).standard_normal((B, 12))
    delta[::2, 5] = np.where(np.arange(B // 2) % 4 < 2, 1.0, -1.0)   # p_z by +-1 m: fz past 0 and past ub
    delta[::2, 9] = 0.5                                              # v_x: fx past mu fz
    states = (x0 + delta).astype(np.float32)
    gain = fresh(solver_mod, p["prm"], recs, U)
    ids = im.combo_ids(B, 1)

    def table():
        s = solver_mod.BatchSolver(cm.make_params(N), max_batch=B)
        s.set_instance_params(im.combo_rows(ids))
        return s

    got, want, outs = row_by_row(functools.partial(run_feedback, recs=recs, forces=U, gain=gain, states=states),
                                 lambda k: solver_mod.BatchSolver(im.combo_params(k, N), max_batch=B,
                                                                  model=im.combo_model(k)), table, ids, im.NC)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    # each combo's mu and f_max show: every pair of shared handles differs somewhere
    for a in range(im.NC):
        for b in range(a + 1, im.NC):
            assert (outs[a] != outs[b]).any(), (a, b)
    assert (got[:, 2::3].max(1) == np.array([im.COMBOS[k][2] for k in ids], np.float32)).any()   # fz at row i's ub


@pytest.mark.parametrize("name", list(gc.FD_INSTANCES))
def test_feedback_end_to_end(cm, orc, solver_mod, needs_ref, name):
    """feedback(solve(rec), gain, x_0 + delta) against the step-0 forces of solve(rec + delta), delta =
    (j % 5 - 2) 2^-12 in the j-th of the p, w, v words: within 2e-4 max(|f|_inf, 1 N). Both solves are
    within the project's REF_TOL = 1e-4 (norm-wise) of their optima, and the optimum is affine on the
    face; the test first checks on the CPU that the fp64 optimum's face is the same at both points."""
    g = load_golden(name)
    prm = golden_params(cm, g)
    ids = list(gc.FD_INSTANCES[name])
    recs = g["records"][ids].copy()
    moved = recs.copy()
    for j, c in enumerate(sorted(gc.X0_WORD)):
        moved[:, gc.X0_WORD[c]] += np.float32((j % 5 - 2) * 2.0 ** -12)
    assert (moved != recs).any()
    for r, m in zip(recs, moved):
        a = sr.slacks(r, prm, orc.fp64_solve(r, prm)[0])[0] <= 1e-6
        b = sr.slacks(m, prm, orc.fp64_solve(m, prm)[0])[0] <= 1e-6
        assert (a == b).all(), name
    states = np.array([gr.x0(orc, m, prm) for m in moved]).astype(np.float32)
    with closing(solver_mod.BatchSolver(prm, max_batch=len(ids))) as s:
        f, st, _ = s.solve_host(recs)
        f2, st2, _ = s.solve_host(moved)
        assert (st == 0).all() and (st2 == 0).all()
        gain = run(s, recs, f, act_tol=1e-3)
        u = run_feedback(s, recs, f, gain, states)
    err = np.abs(u.astype(np.float64) - f2[:, :12]).max(1) / np.maximum(np.abs(f2).max(1), 1.0)
    held = np.abs(f[:, :12].astype(np.float64) - f2[:, :12]).max(1) / np.maximum(np.abs(f2).max(1), 1.0)
    print(f"[gain] {name}: feedback against the second solve {err.max():.2e} (the held forces alone {held.max():.2e})")
    assert err.max() <= 2e-4, (name, err)
