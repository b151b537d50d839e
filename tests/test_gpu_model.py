"""The robot model (cmpc_model: body mass and principal inertia) through every kernel.

Every other GPU test runs the one robot the reference knows, m = 12 and I_body = diag(.07, .26, .242),
so a kernel family that used Ib1 for Ib2, or kept a stray 1/12, passes all of them. Here the model
sets of tests/model_ref.py run over param_sets.CASES (the smallest batches that reach every kernel
family) against the float64 optimum with the model as an argument (model_ref.fp64_solve, tied to
oracle.fp64_solve by tests/test_model_ref.py, which also shows that every tamper of the model moves
that optimum by more than ten gates).

Gates, the project's own: status 0; swing legs exactly zero; N <= 10 within 1e-4 of the fp64 optimum;
N >= 11 (refined) within FP64_TOL = 1e-5 of it. "mini" (a Mini-Cheetah-sized body) is past what an
fp32 condensation can do (test_model_ref.test_fp32_condensation_condition), so it is held to status,
swing and feasibility only, and its distance is reported in the ledger.

Then: the default model is bitwise the solver without a model (a handle that set the default, one that
went to "heavy" and back, one given NULL; with due masks; interleaved with set_params); the
condensation hook, cmpc_batch_evaluate, the rollout, the config-5 residual and ADMM under "heavy";
the reference surface (cmpc_set_model); rejected values leave the handle as it was;
parallel.RootPipeline(model=...) at world 1 and, over gloo, at world 2 (the peer's rows carry the
model's bits); cmpc_multi_set_model (world 1 and the loopback world 2).

Measured on an MI355X (DESIGN.md §3.2 has the table per model and case): N <= 10 ours within 9.4e-6 of
the fp64 optimum ("payload"), N >= 11 within 1.4e-6 ("iperm", N = 20 standing); "mini" 1.3e-4 at
N = 10, 1.2e-6 at N = 16 trot and 1.3e-5 at N = 20 standing.
"""
import functools
import importlib

import numpy as np
import pytest

import evaluate_ref as er
import model_ref as mr
import param_sets as ps
from conftest import PARITY_LEDGER, rel_force_err
from support import (COND_BOUND, FP64_TOL, REF_TOL, ST_FILL, TIGHT, abi_solve, assert_same_bits,  # noqa: F401
                     assert_swing_zero, bits, closing, hook_records, sentinel_solve, solver, solver_mod)

pytestmark = pytest.mark.gpu

VIOL_BAR = 2e-5    # test_gpu_evaluate.test_solve_then_evaluate: no row violated by more than this x max(1, |f|)
SHORT_CASES = ["n10_families", "n16_trot", "n20_standing"]
PARITY = ([(m, c) for m in ("heavy", "payload") for c in ps.CASES] +
          [(m, c) for m in ("x2", "massonly", "iperm") for c in SHORT_CASES])


@pytest.fixture
def x64_ref(orc):
    """For the tests that need the fp64 optimum (qpOASES on the float64 QP)."""
    if not orc.ref_available():
        pytest.skip("oracle/_ref not present")


def model_solve(solver_mod, prm, recs, mdl):
    with closing(solver_mod.BatchSolver(prm, max_batch=max(1, recs.shape[0]), model=mdl)) as s:
        return s.solve_host(recs)


@functools.lru_cache(maxsize=None)
def own_solve(model_name, case):
    """This solver's (forces, status, iters) of a (model set, case), solved once per process."""
    d = mr.cpu_data(model_name, case)
    out = model_solve(solver(), d["prm"], d["recs"], mr.model(model_name))
    for a in out:
        a.setflags(write=False)
    return out


# ---- parity against the fp64 optimum under the model ----------------------------------------------
@pytest.mark.parametrize("model_name,case", PARITY)
def test_parity_under_model(cm, x64_ref, solver_mod, model_name, case):
    d = mr.cpu_data(model_name, case)
    prm, recs, x64 = d["prm"], d["recs"], d["x64"]
    N = prm.horizon
    assert (d["ri64"] == 0).all(), d["ri64"]
    if case == "n10_families":
        counts = ps.family_counts(recs)
        assert min(counts) > 0, counts   # c1-60, c1-64, tail, w80, w96, w120
    f, st, it = own_solve(model_name, case)
    e64 = ps.rel_dist(f, x64)
    at_fmax = int((np.abs(x64.reshape(len(recs), -1, 3)[:, :, 2] - prm.f_max) < 1e-6).sum(1).max())
    line = (f"model {model_name} {case}: {len(recs)} instances, ours within {e64.max():.1e} of the fp64 "
            f"optimum (mean iters {it.mean():.1f}; at most {at_fmax} fz rows at f_max)")
    print("[model] " + line)
    PARITY_LEDGER.append(line)
    assert_swing_zero(cm, recs, N, f)
    assert (st == 0).all(), np.bincount(st)
    gate = REF_TOL if N <= 10 else FP64_TOL
    assert e64.max() <= gate, (e64.max(), int(e64.argmax()))


@pytest.mark.parametrize("case", SHORT_CASES)
def test_mini_is_feasible_and_reported(cm, x64_ref, solver_mod, case):
    """ "mini": status 0, swing legs zero, feasible by cmpc_batch_evaluate under the same model within
    test_gpu_evaluate's bar for our own solves; the distance from the fp64 optimum and the evaluate
    gap go to the ledger, not to an assertion."""
    d = mr.cpu_data("mini", case)
    prm, recs, x64 = d["prm"], d["recs"], d["x64"]
    f, st, it = own_solve("mini", case)
    with closing(solver_mod.BatchSolver(prm, max_batch=len(recs), model=mr.model("mini"))) as s:
        _, c = s.evaluate_host(recs, f)
    e64 = ps.rel_dist(f, x64)
    r = c[:, er.GAP] / np.maximum(1.0, c[:, er.COST0])
    line = (f"model mini {case}: {len(recs)} instances, ours within {e64.max():.1e} of the fp64 optimum "
            f"(reported, not gated; fp64 qpOASES failures {int((d['ri64'] != 0).sum())}); evaluate gap / "
            f"max(1, cost0) median {np.median(r):.1e} max {r.max():.1e}")
    print("[model] " + line)
    PARITY_LEDGER.append(line)
    assert (st == 0).all(), np.bincount(st)
    assert_swing_zero(cm, recs, prm.horizon, f)
    fmax = np.maximum(1.0, np.abs(f).max(axis=1))
    assert (c[:, er.SWING] == 0).all()
    assert (c[:, er.VIOL] <= VIOL_BAR * fmax).all(), float((c[:, er.VIOL] / fmax).max())


# ---- the default model is the solver without a model, bit for bit ----------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["full", "due"])
@pytest.mark.parametrize("case", ["n10_families", "n16_trot"])
def test_default_model_is_bitwise(cm, solver_mod, case, masked):
    N = ps.CASES[case][0]
    prm = cm.make_params(N)
    recs = ps.case_records("default", case)
    B = len(recs)
    due = None
    if masked:
        due = np.zeros(B, np.uint8)
        due[np.random.default_rng(5).choice(B, B // 2, replace=False)] = 1
    heavy = mr.model("heavy")
    with closing(solver_mod.BatchSolver(prm, max_batch=B)) as fresh:
        want = sentinel_solve(fresh, recs, due)
        m0 = fresh.model
        assert (m0.mass, tuple(m0.inertia)) == mr.DEFAULT
    m = np.ones(B, bool) if due is None else due != 0
    assert (want[1][m] == 0).mean() > 0.9 and (want[1][~m] == ST_FILL).all()
    with closing(solver_mod.BatchSolver(prm, max_batch=B, model=cm.make_model())) as s:
        assert_same_bits(sentinel_solve(s, recs, due), want, "set_model(make_model())")
    with closing(solver_mod.BatchSolver(prm, max_batch=B)) as s:
        s.set_model(heavy)
        got_heavy = sentinel_solve(s, recs, due)
        assert not np.array_equal(bits(got_heavy[0])[m], bits(want[0])[m])
        s.set_model(cm.make_model())
        assert_same_bits(sentinel_solve(s, recs, due), want, "heavy and back")
        s.set_model(heavy)
        s.set_model(None)
        assert_same_bits(sentinel_solve(s, recs, due), want, "heavy, then NULL")
        assert (s.model.mass, tuple(s.model.inertia)) == mr.DEFAULT
    with closing(solver_mod.BatchSolver(prm, max_batch=B, model=heavy)) as s:
        assert_same_bits(sentinel_solve(s, recs, due), got_heavy, "a handle created with the model")


@pytest.mark.parametrize("N", [16, 20])
def test_launch_forms_agree_under_model(cm, solver_mod, N):
    """tests/test_gpu_parity.py::test_batch_size_invariance under "heavy": one 16384-instance
    random-contact batch (every size class; the sparse wide classes persistent) against the same
    records in four pieces of 4096 (one workgroup per entry): forces, status and iteration counts agree
    bit for bit. The small parity batches above take the one-per-entry builds; here the persistent
    model-reading builds run too (under the default model the launcher takes the persistent refining
    96- and 120-column builds with the model as literals, which the existing test covers)."""
    prm = cm.make_params(N)
    heavy = mr.model("heavy")
    B = 16384
    recs = cm.make_instances(B, N, seed=8300 + N, random_contact_frac=1.0)
    f_all, st_all, it_all = model_solve(solver_mod, prm, recs, heavy)
    with closing(solver_mod.BatchSolver(prm, max_batch=4096, model=heavy)) as s:
        parts = [s.solve_host(recs[a:a + 4096]) for a in range(0, B, 4096)]
    f_p = np.concatenate([p[0] for p in parts])
    st_p = np.concatenate([p[1] for p in parts])
    it_p = np.concatenate([p[2] for p in parts])
    diff = np.nonzero((f_p != f_all).any(1) | (st_p != st_all) | (it_p != it_all))[0]
    assert diff.size == 0, (diff.size, diff[:8])
    assert (st_all == 0).mean() > 0.99
    f_def, _, _ = model_solve(solver_mod, prm, recs[:4096], None)
    assert not np.array_equal(f_def, f_all[:4096])


def test_model_persists_across_set_params(cm, solver_mod):
    """The model is handle state of its own: set_model then set_params, and set_params then set_model,
    both solve as a fresh handle created with those parameters and that model; set_params does not
    reset it, set_model does not touch the parameters."""
    recs10 = ps.case_records("default", "n10_families")
    recs16 = ps.case_records("default", "n16_trot")
    heavy, payload = mr.model("heavy"), mr.model("payload")
    p10, p10w, p16 = cm.make_params(10), ps.set_params("W1", 10), cm.make_params(16)

    def fresh(prm, mdl, recs):
        with closing(solver_mod.BatchSolver(prm, max_batch=len(recs), model=mdl)) as s:
            return sentinel_solve(s, recs)

    with closing(solver_mod.BatchSolver(p10, max_batch=len(recs10))) as s:
        s.set_model(heavy)
        s.set_params(p10w)                       # model first, then parameters
        assert s.model.mass == 20.0
        assert_same_bits(sentinel_solve(s, recs10), fresh(p10w, heavy, recs10), "set_model, set_params")
        s.set_params(p16)                        # another horizon: the refining wide classes
        assert_same_bits(sentinel_solve(s, recs16), fresh(p16, heavy, recs16), "set_params to N = 16")
        s.set_params(p10)
        s.set_model(payload)                     # parameters first, then model
        assert_same_bits(sentinel_solve(s, recs10), fresh(p10, payload, recs10), "set_params, set_model")
        s.set_params(p10w)
        s.set_model(None)
        assert_same_bits(sentinel_solve(s, recs10), fresh(p10w, None, recs10), "back to the default model")
    assert not np.array_equal(fresh(p10, heavy, recs10)[0], fresh(p10, payload, recs10)[0])


# ---- errors ------------------------------------------------------------------------------------------
def test_bad_models_are_rejected(cm, solver_mod):
    recs = ps.case_records("default", "n3_padding")
    prm = cm.make_params(3)
    heavy = mr.model("heavy")
    bad = [cm.make_model(0.0), cm.make_model(-1.0), cm.make_model(12.0, (0.07, -0.26, 0.242)),
           cm.make_model(float("nan")), cm.make_model(12.0, (0.07, 0.26, float("nan"))),
           cm.make_model(float("inf")), cm.make_model(12.0, (0.0, 0.26, 0.242)),
           # positive and finite, but 1.f / (float) mass and 1.0 / inertia overflow
           cm.make_model(1e-39), cm.make_model(12.0, (1e-310, 0.26, 0.242))]
    with closing(solver_mod.BatchSolver(prm, max_batch=len(recs), model=heavy)) as s:
        want = sentinel_solve(s, recs)
        for b in bad:
            with pytest.raises(solver_mod.CmpcError, match=r"\(-2\)"):
                s.set_model(b)
            assert (s.model.mass, tuple(s.model.inertia)) == mr.MODELS["heavy"]
            assert_same_bits(sentinel_solve(s, recs), want, "after a rejected model")
    for b in bad[:2]:
        with pytest.raises(solver_mod.CmpcError):
            solver_mod.set_model(b)
        with pytest.raises(solver_mod.CmpcError):
            solver_mod.BatchSolver(prm, max_batch=4, model=b)


# ---- the condensation hook and cmpc_batch_evaluate ---------------------------------------------------
@pytest.mark.parametrize("N", [1, 3, 10, 20])
@pytest.mark.parametrize("model_name", ["heavy", "payload"])
def test_hook_matches_fp64_condensation_under_model(cm, solver_mod, model_name, N):
    """BatchSolver.condense against model_ref.fp64_condense on support.hook_records' eight
    records, normwise, within COND_BOUND[N] (2e-6 below N = 10)."""
    import torch
    prm = cm.make_params(N)
    mdl = mr.model(model_name)
    recs, _ = hook_records(cm, N)
    k = recs.shape[0]
    H = torch.zeros((k, 12 * N, 12 * N), dtype=torch.float32, device="cuda")
    g = torch.zeros((k, 12 * N), dtype=torch.float32, device="cuda")
    with closing(solver_mod.BatchSolver(prm, max_batch=k, model=mdl)) as s:
        s.condense(torch.from_numpy(recs).cuda(), H, g)
        torch.cuda.synchronize()
    H = H.cpu().numpy(); g = g.cpu().numpy()
    bound = COND_BOUND[N] if N >= 10 else 2e-6
    worst_h = worst_g = 0.0
    for i in range(k):
        H64, g64 = mr.fp64_condense(recs[i], prm, mdl)
        worst_h = max(worst_h, np.abs(H[i] - H64).max() / np.abs(H64).max())
        worst_g = max(worst_g, np.abs(g[i] - g64).max() / np.abs(g64).max())
    print(f"[model] hook {model_name} N={N}: qg vs fp64 {worst_g:.2e}, qH vs fp64 {worst_h:.2e} (bound {bound:.0e})")
    assert worst_g <= bound, worst_g
    assert worst_h <= bound, worst_h


EVAL_K = 8   # leading instances of a case held against the test-side fp64 evaluation


@pytest.mark.parametrize("case", SHORT_CASES)
@pytest.mark.parametrize("model_name", ["heavy", "payload"])
def test_evaluate_own_solves_under_model(cm, x64_ref, solver_mod, model_name, case):
    """cmpc_batch_evaluate of test_parity_under_model's own solves, on a handle with the same model:
    x_pred, cost, cost0 and the gradient words against evaluate_ref's two fp64 paths with the model
    (model_ref.evaluate) at test_gpu_evaluate's 1e-12 bars, on the leading EVAL_K instances; on every
    instance feasible by the certificate, and the gap within what the distance gate implies
    (gap_bound at dist = gate x max(|U*|, 1), plus 1e-9 max(1, cost0))."""
    d = mr.cpu_data(model_name, case)
    prm, recs, x64 = d["prm"], d["recs"], d["x64"]
    mdl = mr.model(model_name)
    f, st, _ = own_solve(model_name, case)
    with closing(solver_mod.BatchSolver(prm, max_batch=len(recs), model=mdl)) as s:
        x, c = s.evaluate_host(recs, f)
    with closing(solver_mod.BatchSolver(prm, max_batch=len(recs))) as s:
        _, c_default = s.evaluate_host(recs, f)
    assert (st == 0).all()
    assert not np.array_equal(c[:, er.COST], c_default[:, er.COST])   # the model reaches the kernel
    k = min(EVAL_K, len(recs))
    ref = [mr.evaluate(recs[i], prm, mdl, f[i]) for i in range(k)]
    x_ref, c_ref = np.array([a for a, _ in ref]), np.array([b for _, b in ref])
    s_cost = 1e-12 * np.maximum(1.0, c_ref[:, er.COST0])
    s_f = 1e-12 * max(1.0, prm.f_max)
    ratios = {}
    for name, w, bar in (("cost", er.COST, s_cost), ("cost0", er.COST0, s_cost), ("gap", er.GAP, s_cost),
                         ("viol", er.VIOL, s_f), ("swing", er.SWING, s_f), ("gradmax", er.GRADMAX, s_f)):
        ratios[name] = np.abs(c[:k, w] - c_ref[:, w]) / bar
    x32 = x_ref.astype(np.float32)
    ratios["x_pred"] = (np.abs(x[:k].astype(np.float64) - x32.astype(np.float64)) /
                        np.spacing(np.abs(x32)).astype(np.float64)).reshape(k, -1).max(1)
    fmax = np.maximum(1.0, np.abs(f).max(axis=1))
    tol = REF_TOL if prm.horizon <= 10 else FP64_TOL
    worst = 0.0
    bounds = np.zeros(len(recs))
    for i in range(len(recs)):
        dist = tol * max(np.abs(x64[i]).max(), 1.0)
        Hg = mr.fp64_condense(recs[i], prm, mdl)
        bounds[i] = er.gap_bound(Hg, recs[i], prm, f[i], x64[i], dist) + 1e-9 * max(1.0, c[i, er.COST0])
        worst = max(worst, c[i, er.GAP] / bounds[i])
    print(f"[model] evaluate {model_name} {case}: worst ratio to the 1e-12 bars " +
          ", ".join(f"{n} {v.max():.2e}" for n, v in ratios.items()) +
          f"; gap / its bound max {worst:.2e}; viol / (1e-5 max(1,|f|)) max {(c[:, er.VIOL] / (1e-5 * fmax)).max():.3f}")
    for name, v in ratios.items():
        assert v.max() <= 1.0, (model_name, case, name, int(v.argmax()), float(v.max()))
    assert (c[:, er.SWING] == 0).all()
    assert (c[:, er.VIOL] <= VIOL_BAR * fmax).all(), float((c[:, er.VIOL] / fmax).max())
    assert (c[:, er.GAP] <= bounds).all(), (int((c[:, er.GAP] / bounds).argmax()), worst)


# ---- rollout -----------------------------------------------------------------------------------------
def test_rollout_under_model(cm, solver_mod):
    """cmpc_batch_rollout of 64 due instances (of 96) at N = 10 under "heavy" with random xi6 against
    model_ref.step64, within the 2e-5 of tests/test_assemble.py's rollout parity; the instances that
    are not due keep their state."""
    import torch
    R = importlib.import_module("quad-periodic-mpc_amd.records")
    inst = importlib.import_module("quad-periodic-mpc_amd.instances")
    N, B = 10, 96
    prm = cm.make_params(N)
    mdl = mr.model("heavy")
    recs = cm.make_instances(B, N, seed=9377)
    g = np.random.Generator(np.random.Philox(11))
    u = np.zeros((B, 12 * N), np.float32)
    u[:, :12] = g.normal(0, 20, (B, 12))
    xi = g.normal(0, 2, (B, 6)).astype(np.float32)
    due = np.zeros(B, np.uint8)
    due[g.choice(B, 64, replace=False)] = 1
    loco = inst.make_loco_states(B, seed=9)
    d_loco = torch.from_numpy(loco.copy()).cuda()
    d_rec, d_u, d_xi, d_due = (torch.from_numpy(a).cuda() for a in (recs, u, xi, due))
    torch.cuda.synchronize()
    with closing(solver_mod.BatchSolver(prm, max_batch=B, model=mdl)) as s:
        s.rollout(d_loco, d_rec, d_u, xi6=d_xi, due=d_due)
        torch.cuda.synchronize()
    got = d_loco.cpu().numpy()
    np.testing.assert_array_equal(bits(got[due == 0]), bits(loco[due == 0]))
    moved = 0.0
    for b in np.nonzero(due)[0]:
        x1 = mr.step64(recs[b], u[b, :12], xi[b], prm, mdl)
        x1_default = mr.step64(recs[b], u[b, :12], xi[b], prm, mr.model("default"))
        gx = np.concatenate([got[b, R.LOCO_RPY:R.LOCO_RPY + 3], got[b, R.LOCO_POS:R.LOCO_POS + 3],
                             got[b, R.LOCO_WW:R.LOCO_WW + 3], got[b, R.LOCO_VW:R.LOCO_VW + 3]])
        np.testing.assert_allclose(gx, x1, rtol=2e-5, atol=2e-5 * np.abs(x1).max())
        moved = max(moved, np.abs(x1 - x1_default).max() / np.abs(x1).max())
    assert moved > 1e-3, moved   # the default model's step is far outside the tolerance


# ---- the config-5 residual ---------------------------------------------------------------------------
def _residual_run(solver_mod, prm, recs, logs, mdl):
    import torch
    B = len(recs)
    d_rec = torch.from_numpy(np.array(recs, np.float32)).cuda()
    d_log = torch.from_numpy(np.ascontiguousarray(logs)).cuda()
    est = torch.zeros((B, 816), dtype=torch.float32, device="cuda")
    fext6 = torch.full((B, 6), np.nan, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with closing(solver_mod.BatchSolver(prm, max_batch=B)) as s:
        if mdl != "never":
            s.set_model(mdl)
        s.estimate(est, d_rec, logs=d_log, sim_time=1.0, fext6=fext6)
        torch.cuda.synchronize()
    return fext6.cpu().numpy()


def test_residual_under_model(cm, orc, solver_mod):
    """estimate(logs=...) under "heavy" on 64 instances: d_fext6 against model_ref.residual64.

    The bar is the fp32 rounding scale of this residual, measured on the same logs: the maximum
    distance of oracle.residual (the restated fp32 residual, default model) from residual64 at the
    default model, normalised by max(|f_ext|_inf, 1); the gate is 4 x that maximum, because another
    model changes the magnitudes by at most 2-3 x in these sets. Measured on an MI355X: scale 1.44e-6
    (gate 5.8e-6); the kernel is 6.5e-7 from residual64 at the default model and 5.0e-7 under "heavy",
    whose residuals differ from the default model's by 0.58. At the default model the kernel's output is
    bit-identical to a handle that never set a model."""
    N, B = 20, 64
    prm = cm.make_params(N)
    recs = cm.make_instances(B, N, seed=9388)
    logs = cm.make_logs(recs, seed=9389)
    heavy, dflt = mr.model("heavy"), mr.model("default")

    def ndist(a, ref):
        return np.abs(a - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1.0)

    ref_d = np.array([mr.residual64(logs[i], recs[i], dflt) for i in range(B)])
    ref_h = np.array([mr.residual64(logs[i], recs[i], heavy) for i in range(B)])
    scale = ndist(np.array([orc.residual(logs[i], recs[i]) for i in range(B)], np.float64), ref_d).max()
    never = _residual_run(solver_mod, prm, recs, logs, "never")
    got_d = _residual_run(solver_mod, prm, recs, logs, cm.make_model())
    got_h = _residual_run(solver_mod, prm, recs, logs, heavy)
    e_d, e_h = ndist(got_d.astype(np.float64), ref_d).max(), ndist(got_h.astype(np.float64), ref_h).max()
    print(f"[model] residual: fp32 rounding scale {scale:.2e} (oracle.residual vs residual64, default model); "
          f"kernel vs residual64: default {e_d:.2e}, heavy {e_h:.2e}; gate {4 * scale:.2e}; "
          f"heavy vs default references differ by {ndist(ref_h, ref_d).max():.2e}")
    np.testing.assert_array_equal(bits(got_d), bits(never))
    assert 0 < scale < 1e-4, scale     # an fp32 rounding scale, not a modelling difference
    assert e_h <= 4 * scale, (e_h, scale)
    assert ndist(ref_h, ref_d).min() > 100 * scale   # the model moves the residual far beyond the gate


# ---- ADMM --------------------------------------------------------------------------------------------
def test_admm_follows_the_hook_under_model(cm, orc, solver_mod):
    """N = 3, 16 instances, "heavy": BatchSolver.admm on the hook's H and g against oracle.jcqp_admm on
    the same H and g, at test_gpu_admm.test_admm_short_horizons_match_oracle's tolerances (1e-6 where
    the termination iteration agrees, 1e-3 otherwise). cmpc_batch_admm recomputes nothing from the
    model: it follows through H and g."""
    import torch
    N, B = 3, 16
    prm = cm.make_params(N)
    recs_np = cm.make_instances(B, N, seed=9399)
    recs = torch.from_numpy(np.ascontiguousarray(recs_np)).cuda()
    H = torch.empty((B, 12 * N, 12 * N), dtype=torch.float32, device="cuda")
    gv = torch.empty((B, 12 * N), dtype=torch.float32, device="cuda")
    f = torch.empty((B, 12 * N), dtype=torch.float32, device="cuda")
    status = torch.empty(B, dtype=torch.uint8, device="cuda")
    iters = torch.empty(B, dtype=torch.int32, device="cuda")
    H0 = torch.empty_like(H)
    g0 = torch.empty_like(gv)
    torch.cuda.synchronize()
    with closing(solver_mod.BatchSolver(prm, max_batch=B)) as s:
        s.condense(recs, H0, g0)
        s.set_model(mr.model("heavy"))
        s.condense(recs, H, gv)
        s.admm(recs, H, gv, f, status, iters, settings=solver_mod.admm_settings(**TIGHT))
        torch.cuda.synchronize()
    assert not torch.equal(H0, H)
    H, gv, f, iters = H.cpu().numpy(), gv.cpu().numpy(), f.cpu().numpy(), iters.cpu().numpy()
    for i in range(B):
        A, u = orc.fmat_ub(recs_np[i], prm)
        x, it, ok = orc.jcqp_admm(H[i], gv[i], A, u, **TIGHT)
        tol = 1e-6 if iters[i] == it else 1e-3
        assert rel_force_err(f[i:i + 1], x[None])[0] <= tol, (i, it, iters[i])


# ---- the reference surface ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["n10_families", "n16_trot"])
def test_reference_surface_follows_the_model(cm, solver_mod, case):
    """In one process: set_model(heavy) -> update_problem_data_floats equals BatchSolver(model=heavy)
    bit for bit on the same record; set_model(None) -> the default's bits again; cmpc_evaluate_last
    evaluates under the model of the solve (its cost is the heavy handle's, not the default's)."""
    N = ps.CASES[case][0]
    prm = cm.make_params(N)
    recs = ps.case_records("default", case)[:3]
    heavy = mr.model("heavy")
    try:
        for rec in recs:
            for mdl in (heavy, None, heavy):
                solver_mod.set_model(mdl)
                sol = abi_solve(solver_mod, cm, rec, prm)
                f, st, _ = model_solve(solver_mod, prm, rec[None], mdl)
                assert st[0] == 0
                np.testing.assert_array_equal(sol, f[0].astype(np.float64))
                _, cert = solver_mod.evaluate_last()
                with closing(solver_mod.BatchSolver(prm, max_batch=1, model=mdl)) as s:
                    _, c = s.evaluate_host(rec[None], f)
                np.testing.assert_array_equal(cert, c[0])
            f_def, _, _ = model_solve(solver_mod, prm, rec[None], None)
            assert not np.array_equal(f_def[0], f[0])
    finally:
        solver_mod.set_model(None)


# ---- parallel.RootPipeline ---------------------------------------------------------------------------
def test_root_pipeline_passes_the_model_to_its_lanes(cm, solver_mod):
    """A world-1 RootPipeline(model=heavy) over two lanes and three pieces gives the single-handle
    "heavy" forces bit for bit: every lane's handle got the model, none kept the default."""
    import torch
    par = importlib.import_module("quad-periodic-mpc_amd.parallel")
    prm = cm.make_params(10)
    recs = ps.case_records("default", "n10_families")
    heavy = mr.model("heavy")
    f, st, _ = model_solve(solver_mod, prm, recs, heavy)
    f_def, _, _ = model_solve(solver_mod, prm, recs, None)
    assert not np.array_equal(f, f_def)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        pipe = par.RootPipeline(prm, len(recs), chunks=3, device="cuda", model=heavy)
        try:
            assert len(pipe._solvers) == 2 and all(sv.model.mass == 20.0 for sv in pipe._solvers)
            pipe.step(torch.from_numpy(np.array(recs)).cuda())
            torch.cuda.synchronize()
            np.testing.assert_array_equal(bits(pipe.forces.cpu().numpy()), bits(f))
            np.testing.assert_array_equal(pipe.local_status.cpu().numpy(), st)
        finally:
            pipe.close()
    with pytest.raises(ValueError):
        par.RootPipeline(prm, 8, solve_fn=lambda r, f, s: None, model=mr.model("heavy"))


def _gloo_worker(rank, world, port, q):
    try:
        import os
        import sys
        from conftest import ROOT
        sys.path.insert(0, ROOT)
        import torch
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        cm = importlib.import_module("quad-periodic-mpc_amd")
        par = importlib.import_module("quad-periodic-mpc_amd.parallel")
        solver_mod = importlib.import_module("quad-periodic-mpc_amd.solver")
        solver_mod.load_library()
        N, B = 10, 96
        prm = cm.make_params(N)
        recs = cm.make_instances(B, N, seed=9331, random_contact_frac=1.0)   # every rank regenerates the batch
        heavy = mr.model("heavy")
        f_heavy, st_heavy, _ = model_solve(solver_mod, prm, recs, heavy)     # one handle, the whole batch
        f_def, _, _ = model_solve(solver_mod, prm, recs, None)
        # host rows over gloo, each rank's own lanes on the GPU behind them
        pipe = par.RootPipeline(prm, B, chunks=2, model=heavy, lane_device="cuda")
        try:
            assert len(pipe._solvers) == 2 and all(sv.model.mass == 20.0 for sv in pipe._solvers)
            for _ in range(2):
                pipe.step(torch.from_numpy(recs) if rank == 0 else None)
            a, b = pipe.start, pipe.stop
            assert b > a
            mine = pipe.local_forces.numpy()
            np.testing.assert_array_equal(bits(mine), bits(f_heavy[a:b]))
            np.testing.assert_array_equal(pipe.local_status.numpy(), st_heavy[a:b])
            assert not np.array_equal(mine, f_def[a:b])
            if rank == 0:
                np.testing.assert_array_equal(bits(pipe.forces.numpy()), bits(f_heavy))
        finally:
            pipe.close()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, ("ok", (a, b))))
    except Exception as e:  # report to the parent instead of hanging it
        import traceback
        q.put((rank, (repr(e) + traceback.format_exc()[-1500:], None)))


def test_root_pipeline_world2_gloo_under_model():
    """World 2 over gloo in the style of tests/test_parallel.py, with the real solver as
    tests/test_gpu_config4.py runs it on one GPU: RootPipeline(model=heavy, lane_device="cuda") moves
    host rows between the ranks and solves each rank's rows on its own lanes. Every rank's rows, the
    peer's too, carry the single-handle "heavy" bits and differ from the default model's; root's
    gathered forces are the whole single-handle solve."""
    import socket
    import torch.multiprocessing as mp
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        results = dict(q.get(timeout=240) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(v[0] == "ok" for v in results.values()), results
    (a0, b0), (a1, b1) = results[0][1], results[1][1]
    assert a0 == 0 and b0 == a1 and b1 == 96 and b1 > a1   # the peer solved rows of its own


def test_multi_c_abi_forwards_the_model(cm, tmp_path):
    """cmpc_multi_set_model through a plain C++ caller of its own (csrc/tools/cmpc_multi_model_test.cpp,
    in the style of tests/test_gpu_multi.py's): at world 1 and in the loopback world 2 (the automatic
    and an even root share) every multi solve under "heavy" equals the single handle's
    "heavy" solve bit for bit, and that solve differs from the default model's: the peer's handle got
    the model."""
    import json
    import os
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "quad-periodic-mpc_amd", "cmpc_multi_model_test")
    if not os.path.exists(exe):
        pytest.fail("cmpc_multi_model_test not built (quad-periodic-mpc_amd/build.py build_multi)")
    N, B = 10, 4000
    recs = cm.make_instances(B, N, seed=7711, random_contact_frac=0.5)
    f = tmp_path / "recs.f32"
    np.ascontiguousarray(recs, np.float32).tofile(f)
    m, I = mr.MODELS["heavy"]
    r = subprocess.run([exe, str(f), str(B), str(N), repr(m)] + [repr(x) for x in I],
                       capture_output=True, text=True, timeout=240)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["model_moves"] and d["all_bitwise"] and len(d["cases"]) == 3
    assert all(c["rows"][1] > 0 for c in d["cases"] if c["loopback"])

