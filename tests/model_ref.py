"""float64 references with the robot model as an argument (a helper module, no tests in it).

oracle.py states the reference pipeline in float64 for the one robot the reference knows, m = 12 and
I_body = diag(.07, .26, .242) (RobotState.h:25-26). Here the same three functions take the model
(``ct_mats64``, ``fp64_condense``, ``fp64_solve``: oracle.py's own code with m and I_body passed in;
x0, the swing elimination and qpOASES through oracle.condense / oracle.reduce / oracle.qpoases as the
oracle calls them), plus the config-5 residual (``residual64``), one single-rigid-body step
(``step64``) and evaluate_ref's two paths under a model. tests/test_model_ref.py ties them to the
oracle: equal at the default model, and the scaling identity under (c m, c I).

A model is a ``cmpc_model`` (``make_model``); MODELS holds the sets of tests/test_gpu_model.py.
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import evaluate_ref as er
import param_sets as ps
from support import package

# name -> (mass, inertia); "mini" (a Mini-Cheetah-sized body) is reported, not gated: condensing in
# fp32 alone moves its optimum by 1.4e-4 at N = 10 (test_model_ref.test_fp32_condensation_condition)
MODELS = {
    "heavy": (20.0, (0.15, 0.60, 0.55)),
    "payload": (17.0, (0.12, 0.33, 0.25)),
    "x2": (24.0, (0.14, 0.52, 0.484)),
    "massonly": (18.0, (0.07, 0.26, 0.242)),
    "iperm": (12.0, (0.26, 0.07, 0.242)),
    "mini": (9.0, (0.011253, 0.036203, 0.042673)),
}
GATED = ["heavy", "payload", "x2", "massonly", "iperm"]
DEFAULT = (12.0, (0.07, 0.26, 0.242))


def model(name):
    """The named set (or "default") as a cmpc_model."""
    m, I = DEFAULT if name == "default" else MODELS[name]
    return package().make_model(m, I)


def mass_inertia(mdl):
    return float(mdl.mass), np.array([mdl.inertia[0], mdl.inertia[1], mdl.inertia[2]], np.float64)


def _rot64(q):
    w_, x, y, z = np.asarray(q, np.float64)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w_ * z), 2 * (x * z + w_ * y)],
                     [2 * (x * y + w_ * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w_ * x)],
                     [2 * (x * z - w_ * y), 2 * (y * z + w_ * x), 1 - 2 * (x * x + y * y)]])


def _skew(r):
    return np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])


def ct_mats64(rec, mdl):
    """oracle.ct_mats64 (ct_ss_mats, SolverMPC.cpp:260-279) with the model's m and I_body."""
    m, Ib = mass_inertia(mdl)
    R = _rot64(rec[6:10])
    Iw = R @ np.diag(Ib) @ R.T
    Ii = np.linalg.inv(Iw)
    r = rec[13:25].reshape(3, 4).astype(np.float64)
    A = np.zeros((13, 13)); B = np.zeros((13, 12))
    A[3, 9] = A[4, 10] = A[5, 11] = A[11, 12] = 1.0
    A[11, 9] = rec[28]
    A[0:3, 6:9] = R.T
    for b in range(4):
        B[6:9, 3 * b:3 * b + 3] = Ii @ _skew(r[:, b])
        B[9:12, 3 * b:3 * b + 3] = np.eye(3) / m
    Q = np.zeros((13, 6)); Q[6:12] = np.eye(6)
    return A, B, Q


def discretise(rec, prm, mdl, dtype=np.float64):
    """(Adt, Bdt, Qdt) = blocks of expm(dt [A B Q; 0]); ``dtype`` float32 rounds the three blocks."""
    from scipy.linalg import expm
    A, B, Q = ct_mats64(rec, mdl)
    M = np.zeros((31, 31))
    M[:13, :13] = A; M[:13, 13:25] = B; M[:13, 25:31] = Q
    E = expm(prm.dt * M)
    return E[:13, :13].astype(dtype), E[:13, 13:25].astype(dtype), E[:13, 25:31].astype(dtype)


def fp64_condense(rec, prm, mdl, dtype=np.float64):
    """oracle.fp64_condense with the model. ``dtype`` float32: the discretised matrices rounded to
    fp32 and every product of the condensation in fp32 (numpy's summation order), the figure the
    fp32 horizons' condition is stated in; the result is widened again."""
    from oracle import oracle as orc
    N = prm.horizon
    c = orc.condense(rec, prm, full=False)
    Ad, Bd, Qd = discretise(rec, prm, mdl, dtype)
    x0 = c["x0"].astype(dtype)
    nx, nu = 13 * N, 12 * N
    Bqp = np.zeros((nx, nu), dtype); Aqp = np.zeros((nx, 13), dtype); Qqp = np.zeros((nx, 6), dtype)
    P = [np.eye(13, dtype=dtype)]
    for _ in range(N):
        P.append(Ad @ P[-1])
    for r in range(N):
        Aqp[13 * r:13 * r + 13] = P[r + 1]
        for cc in range(r + 1):
            Bqp[13 * r:13 * r + 13, 12 * cc:12 * cc + 12] = P[r - cc] @ Bd
            Qqp[13 * r:13 * r + 13] += P[r - cc] @ Qd
    w = np.tile(np.array(list(prm.weights) + [0.0], dtype), N)
    Xd = np.zeros(nx, dtype)
    Xd.reshape(N, 13)[:, :12] = rec[32:32 + 12 * N].reshape(N, 12)
    f = np.zeros(6, dtype)
    if int(np.ascontiguousarray(rec[30:31], np.float32).view(np.uint32)[0]) & 1:
        f[3] = rec[29]
    qH = dtype(2) * (Bqp.T @ (w[:, None] * Bqp) + dtype(prm.alpha) * np.eye(nu, dtype=dtype))
    qg = dtype(2) * Bqp.T @ (w * (Aqp @ x0 + Qqp @ f - Xd))
    return qH.astype(np.float64), qg.astype(np.float64)


def fp64_solve(rec, prm, mdl, dtype=np.float64):
    """oracle.fp64_solve with the model -> (q_soln [12N], qpOASES return value)."""
    from oracle import oracle as orc
    nu = 12 * prm.horizon
    qH, qg = fp64_condense(rec, prm, mdl, dtype)
    red = orc.reduce(rec, prm, qH.astype(np.float32), qg.astype(np.float32))
    keep = ~red["var_elim"]
    x, _, ri, _ = orc.qpoases(qH[np.ix_(keep, keep)], qg[keep], red["A"], red["lb"], red["ub"],
                              nwsr_max=1000)
    out = np.zeros(nu)
    out[keep] = x
    return out, ri


def fp64_batch(recs, prm, mdl, dtype=np.float64):
    """fp64_solve of every record -> (x64 [B, 12N], qpOASES return values [B])."""
    with ThreadPoolExecutor(8) as ex:
        out = list(ex.map(lambda r: fp64_solve(r, prm, mdl, dtype), recs))
    return np.array([x for x, _ in out]), np.array([ri for _, ri in out])


@functools.lru_cache(maxsize=None)
def cpu_data(model_name, case):
    """-> dict(prm, recs, x64, ri64) of a (model set, param_sets case) under the default cmpc_params,
    computed once per process and read-only."""
    N = ps.CASES[case][0]
    prm = ps.set_params("default", N)
    recs = ps.case_records("default", case)
    x64, ri64 = fp64_batch(recs, prm, model(model_name))
    for a in (recs, x64, ri64):
        a.setflags(write=False)
    return dict(prm=prm, recs=recs, x64=x64, ri64=ri64)


def residual64(log, rec, mdl):
    """f_ext[6] of ConvexMPCLocomotion.cpp:639-771 in float64 from the fp32 words of a LogData
    record and the current record: e = x_k - A_prev x_prev - B_prev u_prev with the ct_ss_mats
    structure (I_world = R diag(I_body) R' from the logged rotation, u_prev = minus the logged
    forces, x(12) = -9.81), f_ext = (-e6, -e7, e8, e9, e10, e11)."""
    m, Ib = mass_inertia(mdl)
    log = np.asarray(log, np.float64)
    rec = np.asarray(rec, np.float64)
    R = log[37:46].reshape(3, 3)
    Ii = np.linalg.inv(R @ np.diag(Ib) @ R.T)
    r = log[25:37].reshape(3, 4)
    u = -log[12:24].reshape(4, 3)
    tq = sum(Ii @ _skew(r[:, b]) @ u[b] for b in range(4))
    fs = u.sum(0) / m
    e = np.zeros(12)
    e[6:9] = rec[10:13] - tq
    e[9:12] = rec[3:6] - fs
    e[11] -= log[24] * log[9] + (-9.81)
    return np.array([-e[6], -e[7], e[8], e[9], e[10], e[11]])


def step64(rec, u0, xi, prm, mdl):
    """x+ = Adt x0 + Bdt u0 + Qdt xi in float64 (expm of the 31 x 31 generator) -> x+[:12]; x0 the
    restated pipeline's (oracle.condense: rpy of quat_to_rpy in fp32, x0[12] = -9.8)."""
    from oracle import oracle as orc
    Ad, Bd, Qd = discretise(rec, prm, mdl)
    x0 = orc.condense(rec, prm, full=False)["x0"].astype(np.float64)
    x1 = Ad @ x0 + Bd @ np.asarray(u0, np.float64) + Qd @ np.asarray(xi, np.float64)
    return x1[:12]


# ---- evaluate_ref's two paths under a model ---------------------------------------------------------
class _ModelOracle:
    """The three oracle functions evaluate_ref calls, with the model bound."""

    def __init__(self, mdl):
        from oracle import oracle as orc
        self._orc, self._mdl = orc, mdl

    def ct_mats64(self, rec):
        return ct_mats64(rec, self._mdl)

    def fp64_condense(self, rec, prm):
        return fp64_condense(rec, prm, self._mdl)

    def condense(self, rec, prm, full=True):
        return self._orc.condense(rec, prm, full=full)   # x0 only: it holds no model


def evaluate(rec, prm, mdl, U):
    """evaluate_ref.evaluate under the model: x_pred, cost, cost0 from the trajectory path, the
    gradient words from the dense path -> (x_pred [N, 12] float64, cert [8])."""
    return er.evaluate(_ModelOracle(mdl), rec, prm, U)


def trajectory(rec, prm, mdl, U):
    return er.trajectory(_ModelOracle(mdl), rec, prm, U)
