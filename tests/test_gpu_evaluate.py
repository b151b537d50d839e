"""BatchSolver.evaluate (cmpc_batch_evaluate): the fp64 prediction, cost and optimality gap of given
forces against the numpy reference of tests/evaluate_ref.py, its invariances, its argument checks,
and solve -> evaluate end to end.

Bars of the parity test (set with the feature, from the reference's own noise: its two fp64 paths
differ by at most 3.2e-15 of the scale below; the factor ~300 allows for the kernel's summation
order and FMA contraction):
  cost, cost0, gap     within 1e-12 max(1, cost0)
  viol, swing, gradmax within 1e-12 max(1, f_max)
  x_pred               within 1 fp32 ulp of float32(reference)
Worst ratio to each bar over every case and batch, measured on an MI355X: cost 2.1e-3,
cost0 1.6e-3, gap 7.4e-3, viol 0, swing 0, gradmax 1.9e-5, x_pred 0 ulp.
"""
import numpy as np
import pytest

import evaluate_ref as er
import param_sets
from conftest import golden_params, load_golden
from support import solver_mod  # noqa: F401

pytestmark = pytest.mark.gpu

BATCHES = [1, 3, 130]
# N = 1: the recursions end at once; 2; 10 from the edge set (all-swing, one foot, all-stance,
# first-step-only, x_drag = +-0.5); 11; 20: 240 columns, several per lane
CASES = ["n1", "n2", "n10_edge", "n11", "n20_mixed", "n20_standing"]
# "<case>@<set>": the same records and forces under a non-default parameter set of
# tests/param_sets.py (twelve distinct non-zero weights; mu, f_max, alpha and dt all moved), so a
# wrong weight index or coefficient in the kernel's closed forms shows; the bars are the same
CASES += [f"{c}@{s}" for s in ("W1", "all") for c in ("n2", "n10_edge", "n20_mixed")]


def _stance(cm, prm, rec):
    return cm.unpack_gait(rec[None], prm.horizon)[0] != 0


def _random_forces(cm, prm, rec, rng, feasible):
    """A feasible vector (inside every stance pyramid, 0 on swing legs), or one with fz < 0 on one
    stance foot-step, |fx| > mu fz on another and a non-zero force on a swing leg."""
    N = prm.horizon
    st = _stance(cm, prm, rec)
    f = np.zeros((4 * N, 3))
    fz = rng.uniform(0.0, 0.5 * prm.f_max, 4 * N)
    f[:, 2] = fz
    f[:, 0] = rng.uniform(-1, 1, 4 * N) * prm.mu * fz * 0.99
    f[:, 1] = rng.uniform(-1, 1, 4 * N) * prm.mu * fz * 0.99
    f[~st] = 0.0
    if not feasible:
        on, off = np.flatnonzero(st), np.flatnonzero(~st)
        if len(on) >= 1:
            f[on[0], 2] = -3.0
        if len(on) >= 2:
            f[on[-1], 0] = 2.0 * prm.mu * f[on[-1], 2] + 1.0
        if len(off) >= 1:
            f[off[0]] = (0.5, -0.25, 2.0)
    return f.reshape(-1).astype(np.float32)


_POOLS = {}


def pool(cm, orc, case):
    """(prm, records [K, words], forces [K, 12N], reference x_pred [K, N, 12], cert [K, 8]) of a
    case, computed once."""
    if case in _POOLS:
        return _POOLS[case]
    rng = np.random.default_rng(20240 + len(case))
    full_name = case
    case, _, set_name = case.partition("@")
    over = param_sets.SETS[set_name or "default"]
    if case.startswith("n") and case[1:].isdigit():
        N = int(case[1:])
        prm = cm.make_params(N, **over)
        base = cm.make_instances(4, N, seed=811 + N, random_contact_frac=1.0)
        recs, forces = [], []
        for r in base:
            for feasible in (True, False):
                recs.append(r)
                forces.append(_random_forces(cm, prm, r, rng, feasible))
    else:
        g = load_golden(case)
        prm = golden_params(cm, g)
        N = prm.horizon
        if set_name:
            prm = cm.make_params(N, **over)
        k = min(6, len(g["records"]))
        recs = [r for r in g["records"][:k]]
        forces = [q.astype(np.float32) for q in g["q_ref"][:k]]
        # the Qdt f term live: a copy of each record with flag bit 0 set and f_est(3) = 7.5
        for r, q in zip(g["records"][:k], g["q_ref"][:k]):
            r2 = r.copy()
            r2[29] = 7.5
            r2[30:31] = np.array([1], np.uint32).view(np.float32)
            recs.append(r2)
            forces.append(q.astype(np.float32))
        for r in g["records"][:2]:
            for feasible in (True, False):
                recs.append(r)
                forces.append(_random_forces(cm, prm, r, rng, feasible))
    recs, forces = np.array(recs, np.float32), np.array(forces, np.float32)
    ref = [er.evaluate(orc, r, prm, u) for r, u in zip(recs, forces)]
    _POOLS[full_name] = (prm, recs, forces, np.array([x for x, _ in ref]), np.array([c for _, c in ref]))
    return _POOLS[full_name]


def device_evaluate(solver_mod, prm, recs, forces, max_batch=None):
    import torch
    B = recs.shape[0]
    s = solver_mod.BatchSolver(prm, max_batch=max_batch or B)
    try:
        dev = torch.device("cuda:0")
        d_rec = torch.from_numpy(np.ascontiguousarray(recs)).to(dev)
        d_f = torch.from_numpy(np.ascontiguousarray(forces)).to(dev)
        d_x = torch.zeros((B, prm.horizon, 12), dtype=torch.float32, device=dev)
        d_c = torch.full((B, solver_mod.CERT_WORDS), -1.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()   # the fills above are done before the handle's own stream writes
        s.evaluate(d_rec, d_f, d_x, d_c)
        torch.cuda.synchronize()
        return d_x.cpu().numpy(), d_c.cpu().numpy()
    finally:
        s.close()


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", CASES)
def test_parity_with_reference(cm, orc, solver_mod, case, B):
    prm, recs, forces, x_ref, c_ref = pool(cm, orc, case)
    idx = np.arange(B) % len(recs)
    x, c = device_evaluate(solver_mod, prm, recs[idx], forces[idx])
    x_ref, c_ref = x_ref[idx], c_ref[idx]
    s_cost = 1e-12 * np.maximum(1.0, c_ref[:, er.COST0])
    s_f = 1e-12 * max(1.0, prm.f_max)
    ratios = {}
    for name, w, bar in (("cost", er.COST, s_cost), ("cost0", er.COST0, s_cost), ("gap", er.GAP, s_cost),
                         ("viol", er.VIOL, s_f), ("swing", er.SWING, s_f), ("gradmax", er.GRADMAX, s_f)):
        ratios[name] = np.abs(c[:, w] - c_ref[:, w]) / bar
    x32 = x_ref.astype(np.float32)
    ratios["x_pred"] = (np.abs(x.astype(np.float64) - x32.astype(np.float64)) /
                        np.spacing(np.abs(x32)).astype(np.float64)).reshape(B, -1).max(1)
    print(f"[evaluate] {case} B={B}: worst ratio to the bar " +
          ", ".join(f"{k} {v.max():.2e}" for k, v in ratios.items()))
    assert np.isfinite(c).all()
    assert (c[:, 6:] == 0).all()
    for name, v in ratios.items():
        assert v.max() <= 1.0, (case, B, name, int(v.argmax()), float(v.max()))
    if case.partition("@")[0] == "n10_edge":
        # the all-swing instance (its golden forces are 0): gap = viol = 0, cost = cost0 exactly
        allswing = [i for i in range(B) if not _stance(cm, prm, recs[idx][i]).any() and not forces[idx][i].any()]
        assert B < 6 or allswing
        for i in allswing:
            assert c[i, er.GAP] == 0 and c[i, er.VIOL] == 0 and c[i, er.COST] == c[i, er.COST0]


@pytest.mark.parametrize("case", ["n10_edge", "n20_mixed"])
def test_invariance_bitwise(cm, orc, solver_mod, case):
    prm, recs, forces, _, _ = pool(cm, orc, case)
    idx = np.arange(130) % len(recs)
    x, c = device_evaluate(solver_mod, prm, recs[idx], forces[idx])
    x2, c2 = device_evaluate(solver_mod, prm, recs[idx], forces[idx])
    assert (x.view(np.uint32) == x2.view(np.uint32)).all() and (c.view(np.uint64) == c2.view(np.uint64)).all()
    # an instance alone against the same instance inside the batch (a larger handle, too)
    for i in (0, 77, 129):
        x1, c1 = device_evaluate(solver_mod, prm, recs[idx][i:i + 1], forces[idx][i:i + 1], max_batch=64)
        assert (x1[0].view(np.uint32) == x[i].view(np.uint32)).all()
        assert (c1[0].view(np.uint64) == c[i].view(np.uint64)).all()
    # host buffers against the device call
    s = solver_mod.BatchSolver(prm, max_batch=130)
    try:
        xh, ch = s.evaluate_host(recs[idx], forces[idx])
    finally:
        s.close()
    assert (xh.view(np.uint32) == x.view(np.uint32)).all() and (ch.view(np.uint64) == c.view(np.uint64)).all()


def test_evaluate_last_matches_batched(cm, solver_mod):
    """cmpc_evaluate_last after the single-instance protocol, bit for bit the batched call on the
    same record and the forces get_solution returns."""
    N = 10
    prm = cm.make_params(N)
    g = load_golden("n10_mixed")
    rec = g["records"][1].copy()
    solver_mod.setup_problem(0.026, N, 0.4, 120)
    solver_mod.update_x_drag(float(rec[28]))
    solver_mod.update_solver_settings(100, 1e-7, 1e-8, 1.5, 1e-5, 0)
    gait = cm.unpack_gait(rec[None], N)[0].astype(np.int32)
    solver_mod.update_problem_data_floats(rec[0:3], rec[3:6], rec[6:10], rec[10:13], rec[13:25],
                                          rec[25], rec[26], rec[27], np.array(prm.weights),
                                          rec[32:32 + 12 * N], prm.alpha, gait)
    sol = np.array([solver_mod.get_solution(j) for j in range(12 * N)]).astype(np.float32)
    x_last, c_last = solver_mod.evaluate_last()
    # the estimator step wrote f_est(3) into the solved record; its flag stays clear while this
    # process has pushed at most 500 samples (f_est(3) is then not read)
    rec[29] = solver_mod.get_f_est()[3]
    s = solver_mod.BatchSolver(prm, max_batch=1)
    try:
        xb, cb = s.evaluate_host(rec[None], sol[None])
    finally:
        s.close()
    assert x_last.shape == (N, 12)
    assert (x_last.view(np.uint32) == xb[0].view(np.uint32)).all()
    assert (c_last.view(np.uint64) == cb[0].view(np.uint64)).all()
    assert c_last[er.COST] < c_last[er.COST0] and c_last[er.SWING] == 0


def test_arguments(cm, orc, solver_mod):
    import torch
    prm, recs, forces, _, c_ref = pool(cm, orc, "n10_edge")
    dev = torch.device("cuda:0")
    d_rec = torch.from_numpy(recs[:4]).to(dev)
    d_f = torch.from_numpy(forces[:4]).to(dev)
    d_c = torch.zeros((4, solver_mod.CERT_WORDS), dtype=torch.float64, device=dev)
    s = solver_mod.BatchSolver(prm, max_batch=4)
    torch.cuda.synchronize()
    try:
        with pytest.raises(solver_mod.CmpcError):       # both outputs NULL
            s.evaluate(d_rec, d_f, None, None)
        # batch > max_batch: the entry point itself refuses (the wrapper would raise first)
        assert s.lib.cmpc_batch_evaluate(s._h, d_rec.data_ptr(), d_f.data_ptr(), 5, None, d_c.data_ptr()) < 0
        with pytest.raises(solver_mod.CmpcError):
            s.evaluate(d_rec, d_f, None, d_c, batch=5)
        assert s.lib.cmpc_batch_evaluate(s._h, d_rec.data_ptr(), d_f.data_ptr(), -1, None, d_c.data_ptr()) < 0
        # a handle that keeps one output step holds no full solution
        s.set_output_steps(1)
        with pytest.raises(solver_mod.CmpcError):
            s.evaluate(d_rec, d_f, None, d_c)
        with pytest.raises(solver_mod.CmpcError):
            s.evaluate_host(recs[:4], forces[:4])
        s.set_output_steps(0)
        torch.cuda.synchronize()
        assert (d_c == 0).all()                          # nothing was launched
        # NaN forces: a NaN cost, a clean return, and the other instances untouched by it
        bad = forces[:4].copy()
        bad[2, 5] = np.nan
        x, c = s.evaluate_host(recs[:4], bad)
        assert np.isnan(c[2, er.COST]) and np.isnan(x[2]).any()
        ok = [0, 1, 3]
        assert (np.abs(c[ok, er.COST] - c_ref[ok, er.COST]) <= 1e-12 * np.maximum(1, c_ref[ok, er.COST0])).all()
        # x_pred alone, cert alone
        s.evaluate(d_rec, d_f, None, d_c)
        torch.cuda.synchronize()
        assert (np.abs(d_c.cpu().numpy()[:, er.COST] - c_ref[:4, er.COST])
                <= 1e-12 * np.maximum(1, c_ref[:4, er.COST0])).all()
    finally:
        s.close()


@pytest.mark.parametrize("N,B,kw", [(10, 512, dict(random_contact_frac=1.0)), (16, 256, dict(gait="trotting"))],
                         ids=["n10-random-contacts", "n16-trot"])
def test_solve_then_evaluate(cm, solver_mod, N, B, kw):
    """Every solved instance is feasible by the certificate: no force on a swing leg, and no row
    violated by more than twice the solver's own add threshold 1e-5 max(1, |x|_max). The kernels
    test the same six rows with the same normalisation (the four friction rows times
    rsqrt(1/mu^2 + 1), fz and ub - fz as they are: cmpc_class1.hip, cmpc_tail.hip, cmpc_wide.h
    `fnorm`), so the bar is the one tests/test_gpu_active_set_paths.py uses."""
    prm = cm.make_params(N)
    recs = cm.make_instances(B, N, seed=4242 + N, **kw)
    s = solver_mod.BatchSolver(prm, max_batch=B)
    try:
        f, st, _ = s.solve_host(recs)
        _, c = s.evaluate_host(recs, f)
    finally:
        s.close()
    ok = st == 0
    assert ok.any()
    fmax = np.maximum(1.0, np.abs(f).max(axis=1))
    print(f"[evaluate] N={N}: {ok.sum()}/{B} solved; viol / (1e-5 max(1,|f|)) max "
          f"{(c[ok, er.VIOL] / (1e-5 * fmax[ok])).max():.3f}; gap/max(1,cost0) median "
          f"{np.median(c[ok, er.GAP] / np.maximum(1, c[ok, er.COST0])):.2e} max "
          f"{(c[ok, er.GAP] / np.maximum(1, c[ok, er.COST0])).max():.2e}")
    assert (c[ok, er.SWING] == 0).all()
    assert (c[ok, er.VIOL] <= 2e-5 * fmax[ok]).all(), float((c[ok, er.VIOL] / fmax[ok]).max())


@pytest.mark.parametrize("name", ["n10_mixed", "n20_standing"])
def test_gap_of_golden_and_own_solutions(cm, solver_mod, name):
    """The oracle-free quality figure: gap / max(1, cost0) at the golden qpOASES forces and at this
    solver's, printed per set. Nothing is asserted of the distribution."""
    g = load_golden(name)
    prm = golden_params(cm, g)
    recs = g["records"]
    s = solver_mod.BatchSolver(prm, max_batch=len(recs))
    try:
        f, st, _ = s.solve_host(recs)
        _, c_own = s.evaluate_host(recs, f)
        _, c_ref = s.evaluate_host(recs, g["q_ref"].astype(np.float32))
    finally:
        s.close()
    for who, c in (("own", c_own), ("qpOASES golden", c_ref)):
        r = c[:, er.GAP] / np.maximum(1.0, c[:, er.COST0])
        print(f"[evaluate] {name} {who}: gap/max(1,cost0) median {np.median(r):.2e} max {r.max():.2e}; "
              f"viol max {c[:, er.VIOL].max():.2e}")
    assert np.isfinite(c_own).all() and np.isfinite(c_ref).all()
