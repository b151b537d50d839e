"""What the test modules share that is neither a test nor data (a helper module, no tests in it):
the package accessors, the ``solver_mod`` and ``needs_ref`` fixtures (a test module imports a fixture
by name), the gates, the sentinel-filled solve and the handles around it, the bitwise comparers, and
the row-by-row scaffold of the per-instance table tests.

Test modules import from here and from the data modules (param_sets, status_cases, model_ref,
evaluate_ref, instance_mix, cost_mix), never from each other. The one exception is the parity gate
itself, assert_parity / assert_failed_reference / tol_for, which stays in tests/test_gpu_parity.py:
pytest rewrites ``assert`` in test modules only, and that gate's failure messages matter. For the
same reason every assert in this module carries its own message.

Importing this module needs neither torch nor a GPU; torch is imported inside the functions that
use it.
"""
import contextlib
import functools
import importlib

import numpy as np
import pytest

# ---- gates: each defined here and nowhere else ------------------------------------------------------
# Ours against the reference pipeline and against the fp64 optimum at N <= 10, where the kernels solve
# in fp32: the north-star 1e-4, norm-wise per instance (conftest.rel_force_err, param_sets.rel_dist).
REF_TOL = 1e-4
# Ours against the fp64 optimum from N = 11, where the wide classes refine against the exact QP
# (measured <= 4e-6 under the default parameters).
FP64_TOL = 1e-5
# The condition on the inputs before a kernel is judged at REF_TOL: the reference pipeline itself is
# within half that bar of the fp64 optimum, so a miss cannot be the reference's drift.
REF_COND = 5e-5
# qH / qg of the structured condensation (cmpc_condense.hip) against the reference's dense fp32 GEMMs
# (the golden qH / qg, SolverMPC.cpp:806-814) and against the float64 condensation
# (oracle.fp64_condense), normwise: max |difference| / max |qH| (qg likewise), per horizon. The
# reference's own fp32 qH is 2.2e-7 .. 5.5e-7 from the fp64 one on the golden fixtures (N = 10 .. 20),
# so the force differences of up to ~1e-4 at N >= 16 come from the conditioning of the QP, not from a
# drift of the condensed matrices.
COND_BOUND = {10: 2e-6, 12: 2e-6, 16: 3e-6, 20: 4e-6}
# ADMM settings tight enough to reach qpOASES's vertex (tests/test_gpu_admm.py)
TIGHT = dict(max_iter=10000, rho=1e-3, sigma=1e-8, alpha=1.5, terminate=1e-4)

# what a solve's status and iteration outputs are pre-filled with
ST_FILL, IT_FILL = 0xAB, -7


# ---- the package -------------------------------------------------------------------------------------
def package():
    return importlib.import_module("quad-periodic-mpc_amd")


def records():
    return importlib.import_module("quad-periodic-mpc_amd.records")


def solver():
    return importlib.import_module("quad-periodic-mpc_amd.solver")


@pytest.fixture(scope="module")
def solver_mod():
    mod = solver()
    mod.load_library()
    return mod


@pytest.fixture
def needs_ref(orc):
    if not orc.ref_available():
        pytest.skip("oracle/_ref not present")


# ---- small things ------------------------------------------------------------------------------------
@contextlib.contextmanager
def closing(s):
    try:
        yield s
    finally:
        s.close()


def free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def sentinel_forces(B, cols):
    """A distinct finite float per word (2^23 + index), so a stray write shows wherever it lands."""
    return (np.uint32(0x4B000000) + np.arange(B * cols, dtype=np.uint32)).view(np.float32).reshape(B, cols)


def reduced_sizes(recs, N):
    """n = 3 x stance foot-steps per record (gait byte x f_max = 120 N: any nonzero byte)."""
    return 3 * (records().unpack_gait(recs, N) != 0).sum(1)


def half_due(B, seed=5):
    due = np.zeros(B, np.uint8)
    due[np.random.default_rng(seed).choice(B, B // 2, replace=False)] = 1
    return due


def nan_where_not_due(recs, due):
    """The records with every word of the instances that are not due set to NaN."""
    out = np.array(recs, np.float32)
    out[due == 0] = np.nan
    return out


def set_tables(recs, N, tab):
    """Write the stance tables tab [B, N, 4] (0 / 1) into the records' gait words."""
    off = records().gait_offset(N)
    recs = np.ascontiguousarray(recs).copy()
    recs[:, off:off + N].view(np.uint8)[:, :] = tab.reshape(len(recs), 4 * N).astype(np.uint8)
    return recs


def hook_records(cm, N):
    """4 plain + 4 stress random-contact instances for the condensation hook; every other one carries
    the history flag and f_est(3) of the size the config-5 disturbance gives (tens of newtons, both
    signs). -> (records, flag)"""
    R = records()
    recs = np.concatenate([
        cm.make_instances(4, N, seed=4100 + N, random_contact_frac=1.0),
        cm.make_instances(4, N, seed=4100 + N, random_contact_frac=1.0, stress=True)])
    fest = np.array([-23.5, 0, 17.25, 0, 9.0, 0, -31.0, 0], np.float32)
    flag = (fest != 0).astype(np.uint32)
    recs[:, R.REC_FEST3] = fest
    recs[:, R.REC_FLAGS] = flag.view(np.float32)
    return np.ascontiguousarray(recs), flag


ACT_HI = 1e-3   # slack <= ACT_HI max(1, |f|_max): counted as possibly active (upper count)
ACT_LO = 2e-5   # slack <= ACT_LO max(1, |f|_max): counted as active (lower count)


def active_counts(cm, prm, recs, f):
    """Per instance: n, and the upper / lower counts of active constraints at forces f."""
    N = prm.horizon
    stance = cm.unpack_gait(recs, N) != 0                      # [B, 4N] per foot-step
    f3 = np.asarray(f, np.float64).reshape(len(f), 4 * N, 3)
    fx, fy, fz = f3[..., 0], f3[..., 1], f3[..., 2]
    mui = 1.0 / prm.mu
    fn = 1.0 / np.sqrt(mui * mui + 1.0)
    slack = np.stack([(mui * fx + fz) * fn, (-mui * fx + fz) * fn, (mui * fy + fz) * fn,
                      (-mui * fy + fz) * fn, fz, prm.f_max - fz], -1)      # [B, 4N, 6]
    scale = np.maximum(1.0, np.abs(f3).max(axis=(1, 2)))[:, None, None]
    live = stance[..., None]
    hi = ((slack <= ACT_HI * scale) & live).sum(axis=(1, 2))
    lo = ((slack <= ACT_LO * scale) & live).sum(axis=(1, 2))
    return 3 * stance.sum(1), hi, lo


# ---- solves ------------------------------------------------------------------------------------------
def gpu_solve(solver_mod, prm, recs):
    """solve_host of the records on a fresh handle -> (forces, status, iters)."""
    with closing(solver_mod.BatchSolver(prm, max_batch=max(1, recs.shape[0]))) as s:
        return s.solve_host(recs)


def sentinel_solve(s, recs, due=None, full_horizon=False):
    """One device solve into sentinel-filled buffers -> (forces, status, iters) as numpy; the call
    synchronises on both sides (the handle runs on its own stream, the uploads on torch's).
    ``full_horizon``: the force buffer is sized for the full horizon whatever the handle's output
    steps -> (forces [B, out_cols], status, iters, the force words past B x out_cols)."""
    import torch
    B, oc = recs.shape[0], s.out_cols
    r = torch.from_numpy(np.array(recs, np.float32)).cuda()
    f = torch.from_numpy(sentinel_forces(B, 12 * s.horizon if full_horizon else oc)).cuda()
    st = torch.full((B,), ST_FILL, dtype=torch.uint8, device="cuda")
    it = torch.full((B,), IT_FILL, dtype=torch.int32, device="cuda")
    dd = None if due is None else torch.from_numpy(np.array(due, np.uint8)).cuda()
    torch.cuda.synchronize()
    s.solve(r, f, st, it, due=dd)
    torch.cuda.synchronize()  # returns: the handle's stream drained
    if not full_horizon:
        return f.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()
    flat = f.cpu().numpy().reshape(-1)
    return flat[:B * oc].reshape(B, oc).copy(), st.cpu().numpy(), it.cpu().numpy(), flat[B * oc:].copy()


class Dev:
    """One handle sized for a batch of B, with the refine and output-step settings applied."""

    def __init__(self, solver_mod, prm, B, refine=True, out_steps=0):
        self.B = B
        self.s = solver_mod.BatchSolver(prm, max_batch=B)
        if not refine:
            self.s.set_refine(False)
        if out_steps:
            self.s.set_output_steps(out_steps)
        self.cols = self.s.out_cols

    def close(self):
        self.s.close()

    def run(self, recs, due=None):
        """sentinel_solve of a whole batch of B."""
        if len(recs) != self.B:
            raise ValueError(f"Dev sized for {self.B} records, got {len(recs)}")
        return sentinel_solve(self.s, recs, due)


def full_solve(solver_mod, prm, recs, **kw):
    with closing(Dev(solver_mod, prm, recs.shape[0], **kw)) as d:
        return d.run(recs)


def _abi_gait_traj(cm, rec, N, gait, traj):
    gait = cm.unpack_gait(rec[None], N)[0].astype(np.int32) if gait is None else gait
    return gait, (rec[32:32 + 12 * N] if traj is None else traj)


def abi_floats(solver_mod, cm, rec, N, prm, gait=None, traj=None):
    """update_problem_data_floats of one record (the gait table and trajectory its own unless given)."""
    gait, traj = _abi_gait_traj(cm, rec, N, gait, traj)
    solver_mod.update_problem_data_floats(rec[0:3], rec[3:6], rec[6:10], rec[10:13], rec[13:25],
                                          rec[25], rec[26], rec[27], np.array(prm.weights),
                                          traj, prm.alpha, gait)


def abi_doubles(solver_mod, cm, rec, N, prm, gait=None, traj=None):
    """update_problem_data, the double-precision entry point (roll / pitch not passed)."""
    gait, traj = _abi_gait_traj(cm, rec, N, gait, traj)
    solver_mod.update_problem_data(*(np.asarray(rec[a:b], np.float64) for a, b in
                                     ((0, 3), (3, 6), (6, 10), (10, 13), (13, 25))),
                                   float(rec[27]), np.array(prm.weights, np.float64),
                                   np.asarray(traj, np.float64), float(prm.alpha), gait)


def abi_solve(solver_mod, cm, rec, prm):
    """setup_problem -> update_x_drag -> update_solver_settings -> update_problem_data_floats ->
    get_solution through the reference ABI -> forces [12N] float64."""
    N = prm.horizon
    solver_mod.setup_problem(prm.dt, N, prm.mu, prm.f_max)
    solver_mod.update_x_drag(float(rec[28]))
    solver_mod.update_solver_settings(100, 1e-7, 1e-8, 1.5, 1e-5, 0)
    abi_floats(solver_mod, cm, rec, N, prm)
    return np.array([solver_mod.get_solution(j) for j in range(12 * N)])


# ---- comparers ---------------------------------------------------------------------------------------
def assert_same_bits(got, want, msg=""):
    """Every array of two tuples bit for bit."""
    for a, b in zip(got, want):
        np.testing.assert_array_equal(bits(a), bits(b), err_msg=msg)


def assert_same(got, ref, rows=None, label=""):
    """(forces, status, iters) of two solves bit for bit, over ``rows`` (a mask; None: all)."""
    rows = slice(None) if rows is None else rows
    for name, a, b in zip(("forces", "status", "iters"), got, ref):
        a, b = bits(a)[rows], bits(b)[rows]
        if not np.array_equal(a, b):
            bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
            raise AssertionError(f"{label}: {name} differ in {bad.size} rows (first of the selection: {bad[:8]})")


def assert_swing_zero(cm, recs, N, f):
    """Every force component of a swing foot-step is exactly zero."""
    swing = np.repeat(cm.unpack_gait(recs, N) == 0, 3, axis=1)
    assert np.all(f[swing] == 0.0), \
        (f"{int((f[swing] != 0.0).sum())} nonzero force words on swing legs, forces {np.shape(f)}; first "
         f"(instance, column): {np.argwhere(swing & (np.asarray(f) != 0.0))[:8].tolist()}")


def assert_due_result(got, ref, due, cols):
    """Due rows carry the unmasked solve's bits, the others their sentinels."""
    f, st, it = got
    f_ref, st_ref, it_ref = ref
    m = np.asarray(due) != 0
    sent = sentinel_forces(len(m), cols)
    assert (st_ref <= 4).all() and (it_ref >= 0).all(), \
        ("the comparator did not write every row: first rows with status > 4 "
         f"{np.nonzero(st_ref > 4)[0][:8]}, with iters < 0 {np.nonzero(it_ref < 0)[0][:8]}")
    np.testing.assert_array_equal(bits(f)[m], bits(f_ref)[m])
    np.testing.assert_array_equal(st[m], st_ref[m])
    np.testing.assert_array_equal(it[m], it_ref[m])
    np.testing.assert_array_equal(bits(f)[~m], bits(sent)[~m])
    assert (st[~m] == ST_FILL).all() and (it[~m] == IT_FILL).all(), \
        (f"rows that are not due lost their sentinels: status at rows {np.nonzero(~m & (st != ST_FILL))[0][:8]} "
         f"({st[~m & (st != ST_FILL)][:8]}), iters at rows {np.nonzero(~m & (it != IT_FILL))[0][:8]} "
         f"({it[~m & (it != IT_FILL)][:8]})")


# ---- the per-instance tables: row i against the shared handle of row i's combo -----------------------
# A mix is tests/instance_mix.py or tests/cost_mix.py (the module): NC combos, combo_params(k, N) and
# combo_model(k) of the shared handle of combo k.
def rows_of(outs, ids):
    """outs[k]: an array (or tuple of arrays) of combo k's shared handle -> row i from combo ids[i]."""
    if isinstance(outs[0], tuple):
        return tuple(rows_of([o[j] for o in outs], ids) for j in range(len(outs[0])))
    if any(len(o) != len(ids) for o in outs):
        raise AssertionError(f"rows_of: {len(ids)} ids for outputs of {[len(o) for o in outs]} rows")
    return np.stack([outs[k][i] for i, k in enumerate(ids)])


def row_by_row(op, shared, table, ids, n_combos):
    """The scaffold of a row-by-row test: ``op(handle)`` on ``shared(k)``, a fresh shared handle of
    every combo k < n_combos, and on ``table()``, a fresh handle with the table set -> (got, want, outs): the
    table handle's output, row i of combo ids[i]'s shared output, and the shared outputs per combo.
    Every handle is closed. The comparison, and the check that the rows really differ, are the
    caller's."""
    outs = []
    for k in range(n_combos):
        with closing(shared(k)) as s:
            outs.append(op(s))
    want = rows_of(outs, ids)
    with closing(table()) as s:
        got = op(s)
    return got, want, outs


def shared_handle(mix, k, N, B):
    """A fresh shared handle of the mix's combo k."""
    return solver().BatchSolver(mix.combo_params(k, N), max_batch=B, model=mix.combo_model(k))


@functools.lru_cache(maxsize=None)
def shared_solve(mix, k, case):
    """(forces, status, iters) of the param_sets case's whole batch on the shared handle of the mix's
    combo k; once per (mix, combo, case) per process, read-only."""
    import param_sets as ps
    N = ps.CASES[case][0]
    recs = ps.case_records("default", case)
    with closing(shared_handle(mix, k, N, len(recs))) as s:
        out = sentinel_solve(s, recs)
    for a in out:
        a.setflags(write=False)
    return out


def rowwise(mix, case, ids):
    """Row i of the case's whole-batch solve on the shared handle of combo ids[i]."""
    return rows_of([shared_solve(mix, k, case) for k in range(mix.NC)], ids)
