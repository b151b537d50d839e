"""The pool of the sensitivity tests (tests/test_sensitivity_ref.py, tests/test_gpu_sensitivity.py): a
helper module, no tests in it. Shapes are those of tests/test_gpu_evaluate.py; per case the records,
forces U and upstream gradients V, with both numpy references of tests/sensitivity_ref.py computed
once per process.

Inputs per case: the golden qpOASES forces (or seeded random ones where there is no golden file),
the same with the Qdt f term live, seeded feasible and infeasible forces, and hand-built forces that
put one stance foot-step on each face type of include/cmpc_solver.h (interior, one side, an edge, the
cap, cap and one side, cap and two sides, the apex). V is seeded normal.
"""
import numpy as np

import param_sets
import sensitivity_ref as sr
from conftest import golden_params, load_golden

ACT_TOL = 1e-3
# N = 1: the recursions end at once; 2; 10 from the edge set (all-swing, one foot, all-stance,
# first-step-only, x_drag = +-0.5); 11; 20: up to 240 free dimensions
CASES = ["n1", "n2", "n10_edge", "n11", "n20_mixed", "n20_standing"]
# "<case>@<set>": the same under a non-default parameter set of tests/param_sets.py
CASES += [f"{c}@{s}" for s in ("W1", "all") for c in ("n2", "n10_edge", "n20_mixed")]

# The parity bar of the GPU tests, per output block norm-wise and per horizon: 300 x the largest
# disagreement of the two numpy paths at that horizon, over this pool and over the golden sets of the
# end-to-end test (tests/test_sensitivity_ref.py measures and prints both; the factor is the one
# tests/test_gpu_evaluate.py uses for the kernel's summation order and contraction). Measured: N = 1
# 4.8e-15 (n1), 2 4.0e-14 (n2@W1), 10 1.5e-13 (n10_edge@all), 11 2.4e-13 (n11), 16 5.9e-13 (n16_trot),
# 20 1.1e-10 (n20_standing): the disagreement grows with the conditioning of Z'HZ, so one bar for
# every horizon would be 1e5 too wide at the short ones.
REF_NOISE = {1: 4.8e-15, 2: 4.0e-14, 10: 1.5e-13, 11: 2.4e-13, 16: 5.9e-13, 20: 1.1e-10}
E2E_SETS = ["n10_mixed", "n16_trot", "n20_standing"]


def bar(N):
    return 300 * REF_NOISE[N]


def e2e_inputs(cm, name):
    """The end-to-end test's six golden records of a set, its upstream gradients and the golden
    forces -> (prm, recs, V, q_ref)."""
    g = load_golden(name)
    prm = golden_params(cm, g)
    V = np.random.default_rng(40 + prm.horizon).standard_normal((6, 12 * prm.horizon)).astype(np.float32)
    return prm, g["records"][:6], V, g["q_ref"][:6].astype(np.float32)


FACES = ("interior", "side", "edge", "cap", "cap+side", "cap+2sides", "apex")
FACE_DIM = dict(zip(FACES, (3, 2, 1, 2, 1, 0, 0)))


def stance(cm, prm, rec):
    return cm.unpack_gait(rec[None], prm.horizon)[0] != 0


def random_forces(cm, prm, rec, rng, feasible):
    """Inside every stance pyramid and 0 on swing legs, or with fz < 0 on one stance foot-step,
    |fx| > mu fz on another and a force on a swing leg."""
    N = prm.horizon
    st = stance(cm, prm, rec)
    f = np.zeros((4 * N, 3))
    fz = rng.uniform(0.05 * prm.f_max, 0.5 * prm.f_max, 4 * N)
    f[:, 2] = fz
    f[:, 0] = rng.uniform(-1, 1, 4 * N) * prm.mu * fz * 0.9
    f[:, 1] = rng.uniform(-1, 1, 4 * N) * prm.mu * fz * 0.9
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


def face_forces(cm, prm, rec, rng):
    """Feasible forces whose stance foot-steps cycle through FACES -> (forces [12N] float32, the
    face's dimension m they must give at ACT_TOL)."""
    N = prm.horizon
    st = stance(cm, prm, rec)
    f = random_forces(cm, prm, rec, rng, True).astype(np.float64).reshape(4 * N, 3)
    mu = 1.0 / np.float64(np.float32(1.0) / np.float32(prm.mu))   # the kernel's mu (1/mu is fmat's fp32)
    ub = float(np.float32(prm.f_max))
    m = 0
    for n, t in enumerate(np.flatnonzero(st)):
        kind = FACES[n % len(FACES)]
        fz = ub if kind.startswith("cap") else 0.0 if kind == "apex" else f[t, 2]
        fx, fy = (0.3 * mu * fz, -0.2 * mu * fz) if fz else (0.0, 0.0)
        if kind == "side":
            fx = mu * fz
        elif kind == "edge":
            fx, fy = -mu * fz, mu * fz
        elif kind == "cap+side":
            fy = -mu * fz
        elif kind == "cap+2sides":
            fx, fy = mu * fz, mu * fz
        f[t] = (fx, fy, fz)
        m += FACE_DIM[kind]
    return f.reshape(-1).astype(np.float32), m


_POOLS = {}


def pool(cm, orc, case):
    """-> dict(prm, recs [K, words], U [K, 12N], V [K, 12N], m_faces {index: m}, ric, den): the two
    references as lists of (sens, dtraj, dg) per instance. Computed once; leave it unchanged."""
    if case in _POOLS:
        return _POOLS[case]
    rng = np.random.default_rng(31700 + len(case))
    name, _, set_name = case.partition("@")
    over = param_sets.SETS[set_name or "default"]
    recs, U, m_faces = [], [], {}
    if name[1:].isdigit():
        N = int(name[1:])
        prm = cm.make_params(N, **over)
        base = list(cm.make_instances(4, N, seed=811 + N, random_contact_frac=1.0))
        for r in base:
            for feasible in (True, False):
                recs.append(r)
                U.append(random_forces(cm, prm, r, rng, feasible))
        live = base[:2]
    else:
        g = load_golden(name)
        prm = golden_params(cm, g)
        N = prm.horizon
        if set_name:
            prm = cm.make_params(N, **over)
        k = min(6, len(g["records"]))
        for r, q in zip(g["records"][:k], g["q_ref"][:k]):
            recs.append(r)
            U.append(q.astype(np.float32))
        for r, q in zip(g["records"][:k], g["q_ref"][:k]):   # the Qdt f term live
            r2 = r.copy()
            r2[29] = 7.5
            r2[30:31] = np.array([1], np.uint32).view(np.float32)
            recs.append(r2)
            U.append(q.astype(np.float32))
        for r in g["records"][:2]:
            for feasible in (True, False):
                recs.append(r)
                U.append(random_forces(cm, prm, r, rng, feasible))
        live = [recs[k], recs[k + 1]]
        base = list(g["records"][:k])
    # the face types, on the two records with the most stance foot-steps and on one more (in the golden
    # cases one with Qdt f live)
    order = np.argsort([-stance(cm, prm, r).sum() for r in base], kind="stable")
    for r in [base[order[0]], base[order[min(1, len(base) - 1)]], live[0]]:
        u, m = face_forces(cm, prm, r, rng)
        m_faces[len(recs)] = m
        recs.append(r)
        U.append(u)
    recs, U = np.array(recs, np.float32), np.array(U, np.float32)
    V = rng.standard_normal(U.shape).astype(np.float32)
    out = dict(prm=prm, recs=recs, U=U, V=V, m_faces=m_faces,
               ric=[sr.riccati(orc, r, prm, u, v, ACT_TOL) for r, u, v in zip(recs, U, V)],
               den=[sr.dense(orc, r, prm, u, v, ACT_TOL) for r, u, v in zip(recs, U, V)])
    _POOLS[case] = out
    return out


def stacked(refs):
    """A list of (sens, dtraj, dg) -> (sens [K, 32], dtraj [K, 12N], dg [K, 12N])."""
    return tuple(np.array([r[j] for r in refs]) for j in range(3))
