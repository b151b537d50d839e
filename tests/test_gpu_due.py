"""GPU tests of the due-masked solve and estimate (cmpc_batch_solve_due / cmpc_batch_estimate_due;
BatchSolver.solve(due=...) / .estimate(due=...)): batches whose robots have their MPC steps on
different control ticks.

The comparator throughout is the unmasked solve / estimate of the same build on the same records
(unchanged code, held to qpOASES by tests/test_gpu_parity.py and tests/test_gpu_estimator.py). No
tolerance is involved: every comparison is on bit patterns (floats viewed as uint32). A due
instance must get exactly what the unmasked call writes for its record; of an instance that is not
due the record is never read and the outputs keep the sentinels they were pre-filled with."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

from support import (ST_FILL, Dev, assert_due_result, bits, full_solve, package, records, reduced_sizes,  # noqa: F401
                     sentinel_forces, solver, solver_mod)

pytestmark = pytest.mark.gpu

# reduced sizes on both sides of every class edge (tests/test_gpu_parity.py CLASS_EDGES: 60, 64, 80,
# 96, 120, 128, 144, 192) and of the tail class's 72
TARGETS = [3, 57, 60, 63, 66, 72, 75, 81, 96, 99, 120, 123, 129, 144, 147, 192, 195, 240]
EDGES = [0, 60, 64, 72, 80, 96, 120, 128, 144, 192, 256]


@functools.lru_cache(maxsize=None)
def class_batch(N):
    """Four instances per reduced size of TARGETS (two of them due) + 12 random ones, the last of
    the batch due -> (records, due)."""
    cm = package()
    R = records()
    targets = [t for t in TARGETS if t <= 12 * N]
    B = 4 * len(targets) + 12
    B += B % 64 == 0                              # (N = 11: 52 + 12) never a multiple of the wavefront
    recs = cm.make_instances(B, N, seed=4100 + N, random_contact_frac=1.0)
    rng = np.random.default_rng(900 + N)
    go = R.gait_offset(N)
    gait = recs[:, go:go + N].view(np.uint8)      # [B, 4N] step-major, leg-minor (a view)
    due = np.zeros(B, np.uint8)
    for k, n in enumerate(targets):
        for j in range(4):
            row = np.zeros(4 * N, np.uint8)
            row[rng.choice(4 * N, n // 3, replace=False)] = 1
            gait[4 * k + j] = row
        due[4 * k + rng.choice(4, 2, replace=False)] = 1
    due[4 * len(targets):] = rng.integers(0, 2, B - 4 * len(targets))
    due[B - 1] = 1
    assert B % 64 != 0
    got_n = reduced_sizes(recs, N)[:4 * len(targets)].reshape(-1, 4)
    assert (got_n == np.array(targets)[:, None]).all()
    recs.setflags(write=False)
    due.setflags(write=False)
    return recs, due


CASES = [(3, True, 0), (10, True, 0), (11, True, 0), (16, True, 0), (20, True, 0), (16, False, 0), (10, True, 1)]


@functools.lru_cache(maxsize=None)
def class_batch_reference(N, refine, out_steps):
    recs, _ = class_batch(N)
    return full_solve(solver(), package().make_params(N), recs, refine=refine, out_steps=out_steps)


@pytest.mark.parametrize("N,refine,out_steps", CASES)
def test_every_class_small_batch(cm, solver_mod, N, refine, out_steps):
    """Every size class at every horizon family (N = 3: no classify pass in the unmasked solve;
    10: tail class; 11: class 1 listed; 16, 20: the wide classes carry the batch), without the
    refinement at N = 16 and with one output step at N = 10."""
    recs, due = class_batch(N)
    ref = class_batch_reference(N, refine, out_steps)
    d = Dev(solver_mod, cm.make_params(N), recs.shape[0], refine=refine, out_steps=out_steps)
    try:
        got = d.run(recs, due)
        cols = d.cols
    finally:
        d.close()
    assert cols == 12 * (out_steps or N)
    assert_due_result(got, ref, due, cols)


@pytest.mark.parametrize("N", [10, 20])
def test_not_due_records_are_never_read(cm, solver_mod, N):
    """Every word of the records that are not due is a NaN pattern and their gait bytes 0xFF (a
    reduced size of 12 N if it were counted): the outputs are bit-identical to the clean batch's."""
    recs, due = class_batch(N)
    R = records()
    bad = recs.copy()
    nd = due == 0
    bad.view(np.uint32)[nd] = 0x7FC00000
    go = R.gait_offset(N)
    bad[:, go:go + N].view(np.uint8)[nd] = 0xFF
    d = Dev(solver_mod, cm.make_params(N), recs.shape[0])
    try:
        clean = d.run(recs, due)
        got = d.run(bad, due)
    finally:
        d.close()
    assert_due_result(clean, class_batch_reference(N, True, 0), due, 12 * N)
    for a, b in zip(got, clean):
        np.testing.assert_array_equal(bits(a), bits(b))


@pytest.mark.parametrize("N", [10, 16])
def test_degenerate_masks(cm, solver_mod, N):
    B = 130
    prm = cm.make_params(N)
    recs = cm.make_instances(B, N, seed=5200 + N, random_contact_frac=1.0)
    ref = full_solve(solver_mod, prm, recs)
    n = reduced_sizes(recs, N)
    cls = np.searchsorted(EDGES, n, side="left")   # EDGES[c - 1] < n <= EDGES[c]
    singles = [0, B - 1] + [int(np.nonzero(cls == c)[0][0]) for c in np.unique(cls)]
    assert len(np.unique(cls)) >= 3
    d = Dev(solver_mod, prm, B)
    try:
        ones = np.ones(B, np.uint8)
        got = d.run(recs, ones)                              # all due: the unmasked solve everywhere
        for a, b in zip(got, ref):
            np.testing.assert_array_equal(bits(a), bits(b))
        assert_due_result(d.run(recs, np.zeros(B, np.uint8)), ref, np.zeros(B, np.uint8), 12 * N)  # none
        for i in singles:                                    # exactly one
            m = np.zeros(B, np.uint8)
            m[i] = 1
            assert_due_result(d.run(recs, m), ref, m, 12 * N)
        m = np.zeros(B, np.uint8)                            # any nonzero byte counts as due
        m[::3], m[1::7], m[5::11] = 1, 2, 255
        assert {1, 2, 255} <= set(m.tolist()) and (m == 0).any()
        assert_due_result(d.run(recs, m), ref, m, 12 * N)
        # the timing hooks record a due solve; the overflow count is of due instances only (below
        # 16384 instances class 1 takes every n <= 64)
        d.s.enable_timing(1)
        d.run(recs, m)
        ms, ovf = d.s.read_timing()
        assert ms.shape == (1, 2) and (ms >= 0).all()
        assert ovf == int(((m != 0) & (n > 64)).sum())
    finally:
        d.close()


@functools.lru_cache(maxsize=None)
def large_batch(N):
    cm = package()
    B = 16384
    recs = cm.make_instances(B, N, seed=6300 + N, random_contact_frac=1.0)
    recs.setflags(write=False)
    return recs, full_solve(solver(), cm.make_params(N), recs)


@pytest.mark.parametrize("pre_trot", [False, True])
@pytest.mark.parametrize("N", [10, 20])
def test_large_batch_forms_and_hint(cm, solver_mod, N, pre_trot):
    """16384 instances (the 60 / 64 class-1 split, persistent sparse classes, hinted grids with
    their rest launches), every 13th due, interleaved with unmasked solves on one handle: a due
    solve leaves a hint the next solve of either form scales, and takes one from either form.
    Every call gives a fresh handle's bits. pre_trot: the handle has seen only trot batches before
    (hint ~ 0 for the wide classes), as tests/test_gpu_parity.py's stale-hint test."""
    recs, ref = large_batch(N)
    B = recs.shape[0]
    due = (np.arange(B) % 13 == 5).astype(np.uint8)
    d = Dev(solver_mod, cm.make_params(N), B)
    try:
        if pre_trot:
            trot = cm.make_instances(B, N, seed=6400 + N, random_contact_frac=0.0)
            for _ in range(3):
                d.run(trot)
        for form in ("full", "full", "due", "due", "full", "due"):
            if form == "full":
                for a, b in zip(d.run(recs), ref):
                    np.testing.assert_array_equal(bits(a), bits(b))
            else:
                assert_due_result(d.run(recs, due), ref, due, 12 * N)
    finally:
        d.close()


@pytest.mark.parametrize("source", ["logs", "fext3"])
def test_estimator_due(cm, solver_mod, source):
    """Sample counts 399, 400, 450, 500, 501 and 0 (the first estimation, re-estimations, the last
    one, past the stop, an empty history), masks (1,0,1,0,1,0) then its inverse on the same state:
    after the first call the due instances equal the unmasked step of a copy and the others their
    state before it; after the second every instance equals the unmasked step."""
    import torch
    R = records()
    N, B = 20, 6
    counts = [399, 400, 450, 500, 501, 0]
    prm = cm.make_params(N)
    recs_np = cm.make_instances(B, N, seed=7700)
    f3, tt = cm.make_disturbance(B, R.EST_WINDOW)
    est_np = np.zeros((B, R.EST_WORDS), np.float32)
    for i, c in enumerate(counts):   # primed as tests/test_gpu_estimator.py primes them
        k = min(c, R.EST_WINDOW)
        est_np[i, R.EST_F:R.EST_F + k] = f3[i, :k]
        est_np[i, R.EST_T:R.EST_T + k] = tt[:k]
        est_np.view(np.int32)[i, R.EST_COUNT] = c
        est_np.view(np.int32)[i, R.EST_HEAD] = c % R.EST_WINDOW
        if c > R.EST_WINDOW:         # a fit of an earlier step: stat, amp, freq, phase
            est_np[i, 804:812] = np.array([-10.0, 15.0, 0.33, 0.4]).view(np.float32)
            est_np[i, 802] = 3.5
    logs_np = cm.make_logs(recs_np)
    fx_np = np.linspace(-20, 5, B).astype(np.float32)
    fx6_fill = sentinel_forces(B, 6)
    s = solver_mod.BatchSolver(prm, max_batch=B)

    def state():
        return (torch.from_numpy(est_np.copy()).cuda(), torch.from_numpy(recs_np.copy()).cuda(),
                torch.from_numpy(fx6_fill.copy()).cuda())

    def step(est, recs, fx6, due):
        kw = dict(logs=torch.from_numpy(logs_np).cuda(), fext6=fx6) if source == "logs" else \
            dict(fext3=torch.from_numpy(fx_np).cuda())
        d = None if due is None else torch.from_numpy(np.asarray(due, np.uint8)).cuda()
        torch.cuda.synchronize()
        s.estimate(est, recs, sim_time=10.4, due=d, **kw)
        torch.cuda.synchronize()
        return [bits(t.cpu().numpy()) for t in (est, recs, fx6)]

    try:
        before = [bits(a) for a in (est_np, recs_np, fx6_fill)]
        full = step(*state(), None)
        mask = np.array([1, 0, 1, 0, 1, 0], np.uint8)
        st = state()
        first = step(*st, mask)
        second = step(*st, 1 - mask)
    finally:
        s.close()
    m = mask != 0
    assert not np.array_equal(full[0], before[0]) and not np.array_equal(full[1], before[1])
    for got, ref, pre in zip(first, full, before):
        np.testing.assert_array_equal(got[m], ref[m])
        np.testing.assert_array_equal(got[~m], pre[~m])
    for got, ref in zip(second, full):
        np.testing.assert_array_equal(got, ref)
    if source == "logs":
        assert not np.array_equal(full[2], before[2])


def test_staggered_closed_loop(cm, solver_mod):
    """256 trotting robots whose iterationCounters are the generator's random values (not snapped
    to a multiple of iters_between_mpc), 3 x 13 + 2 control ticks. Loop A: assemble ->
    solve(due) -> rollout(due). Loop B: assemble -> unmasked solve into scratch -> the due rows
    merged into the held forces and status -> rollout(due). Controller state, held forces and
    status are bit-identical after every tick."""
    import torch
    R = records()
    inst = importlib.import_module("quad-periodic-mpc_amd.instances")
    N, B, ITERS, DT = 10, 256, 13, 0.002
    ticks = 3 * ITERS + 2
    prm = cm.make_params(N)
    loco = inst.make_loco_states(B, seed=31, gaits=("trotting",), omni_frac=1.0, first_run_frac=1.0)
    loco[:, R.LOCO_CMD + 2] = 0.0
    recs0 = cm.make_instances(B, N, seed=8800)
    lp = R.make_loco_params(DT, ITERS, 0.0)

    class Loop:
        def __init__(self):
            self.loco = torch.from_numpy(loco.copy()).cuda()
            self.rec = torch.from_numpy(recs0.copy()).cuda()
            self.due = torch.zeros(B, dtype=torch.uint8, device="cuda")
            self.f = torch.from_numpy(sentinel_forces(B, 12 * N)).cuda()
            self.st = torch.full((B,), ST_FILL, dtype=torch.uint8, device="cuda")
            self.s = solver_mod.BatchSolver(prm, max_batch=B)

    a, b = Loop(), Loop()
    f_tmp = torch.zeros((B, 12 * N), dtype=torch.float32, device="cuda")
    st_tmp = torch.zeros(B, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dues = []
    try:
        for t in range(ticks):
            a.s.assemble(a.loco, lp, a.rec, a.due)
            a.s.solve(a.rec, a.f, a.st, due=a.due)
            a.s.rollout(a.loco, a.rec, a.f, due=a.due)
            b.s.assemble(b.loco, lp, b.rec, b.due)
            b.s.solve(b.rec, f_tmp, st_tmp)
            torch.cuda.synchronize()
            m = b.due != 0
            b.f = torch.where(m[:, None], f_tmp, b.f)
            b.st = torch.where(m, st_tmp, b.st)
            torch.cuda.synchronize()
            b.s.rollout(b.loco, b.rec, b.f, due=b.due)
            torch.cuda.synchronize()
            due = a.due.cpu().numpy()
            np.testing.assert_array_equal(due, b.due.cpu().numpy())
            for x, y in ((a.loco, b.loco), (a.f, b.f), (a.rec, b.rec)):
                np.testing.assert_array_equal(bits(x.cpu().numpy()), bits(y.cpu().numpy()), err_msg=f"tick {t}")
            st = a.st.cpu().numpy()
            np.testing.assert_array_equal(st, b.st.cpu().numpy())
            assert (st[due != 0] == 0).all(), (t, np.bincount(st[due != 0]))  # every solved QP
            dues.append(due != 0)
    finally:
        a.s.close()
        b.s.close()
    dues = np.array(dues)                                    # [ticks, B]
    assert not dues.all(axis=1).any()                        # never in lockstep
    for t0 in range(ticks - ITERS + 1):                      # once per 13 consecutive ticks
        assert (dues[t0:t0 + ITERS].sum(0) == 1).all()
    assert (a.st.cpu().numpy() == 0).all()                   # every robot has solved by now


def test_argument_checks(cm, solver_mod):
    """Python refuses a due mask of the wrong dtype, length or device; the C entry points return
    what the unmasked ones return for a batch above max_batch and for NULL outputs."""
    import torch
    N, B = 10, 8
    s = solver_mod.BatchSolver(cm.make_params(N), max_batch=B)
    try:
        recs = torch.zeros((B, s.record_words), dtype=torch.float32, device="cuda")
        f = torch.zeros((B, 12 * N), dtype=torch.float32, device="cuda")
        st = torch.zeros(B, dtype=torch.uint8, device="cuda")
        est = torch.zeros((B, 816), dtype=torch.float32, device="cuda")
        fx = torch.zeros(B, dtype=torch.float32, device="cuda")
        for bad in (torch.ones(B, dtype=torch.int32, device="cuda"),
                    torch.ones(B, dtype=torch.bool, device="cuda"),
                    torch.ones(B - 1, dtype=torch.uint8, device="cuda"),
                    torch.ones(B, dtype=torch.uint8),
                    np.ones(B, np.uint8)):
            with pytest.raises(solver_mod.CmpcError):
                s.solve(recs, f, st, due=bad)
            with pytest.raises(solver_mod.CmpcError):
                s.estimate(est, recs, fext3=fx, due=bad)
        lib, h = s.lib, s._h
        due = torch.ones(B + 1, dtype=torch.uint8, device="cuda")
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        for args in ((p(recs), B + 1, p(f), p(st), None),     # batch > max_batch
                     (p(recs), B, None, p(st), None),         # NULL forces
                     (p(recs), B, p(f), None, None),          # NULL status
                     (None, B, p(f), p(st), None)):           # NULL records
            rc = lib.cmpc_batch_solve(h, *args)
            assert rc < 0
            assert lib.cmpc_batch_solve_due(h, args[0], p(due), *args[1:]) == rc
            assert lib.cmpc_batch_solve_due(h, args[0], None, *args[1:]) == rc
        rc = lib.cmpc_batch_estimate(h, p(est), None, p(fx), None, 0.0, p(recs), None, B + 1)
        assert rc < 0
        assert lib.cmpc_batch_estimate_due(h, p(est), None, p(fx), None, 0.0, p(recs), None, p(due), B + 1) == rc
        assert lib.cmpc_batch_estimate_due(h, p(est), None, None, None, 0.0, p(recs), None, p(due), B) == \
            lib.cmpc_batch_estimate(h, p(est), None, None, None, 0.0, p(recs), None, B) < 0
    finally:
        s.close()
