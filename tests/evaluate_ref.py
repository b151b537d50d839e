"""numpy fp64 reference of BatchSolver.evaluate (cmpc_batch_evaluate), two independent paths.

* dense: qH, qg from ``oracle.fp64_condense`` -> J = 1/2 U'HU + g'U, grad = HU + g, and the gap /
  viol / swing / gradmax formulas of include/cmpc_solver.h on that gradient;
* trajectory: x_pred, cost, cost0 (and a numpy adjoint gradient) from ``oracle.ct_mats64``,
  ``scipy.linalg.expm(dt M)`` and a plain loop over the steps.

The product imports neither. Conventions both paths and the kernel share, all taken from how the
reference pipeline holds the numbers in fp32:
  * x_0 = the restated pipeline's x0 (``oracle.condense``: rpy of quat_to_rpy rounded to fp32);
  * dt, alpha, weights, f_max: the fp32 values of the parameter block, widened;
  * 1/mu = fp32(1 / fp32(mu)) as fmat holds it (SolverMPC.cpp:657), mu = 1 / that;
  * ub = fp32(gait x f_max) per foot-step; swing (eliminated) iff |ub| < 0.01 (SolverMPC.cpp:869-894).
"""
import numpy as np

COST, COST0, GAP, VIOL, SWING, GRADMAX = range(6)


def _consts(rec, prm):
    N = prm.horizon
    off = 32 + 12 * N
    gait = np.ascontiguousarray(rec[off:off + N], np.float32).view(np.uint8)[:4 * N]
    ub = (gait.astype(np.float32) * np.float32(prm.f_max)).astype(np.float64)   # [4N]
    stance = ~(np.abs(ub) < np.float64(np.float32(0.01)))
    mui = np.float64(np.float32(1.0) / np.float32(prm.mu))
    return ub, stance, mui


def certificate(rec, prm, U, grad, cost, cost0):
    """The cert words from a gradient (either path's) at forces U."""
    N = prm.horizon
    ub, stance, mui = _consts(rec, prm)
    mu = 1.0 / mui
    f = np.asarray(U, np.float64).reshape(4 * N, 3)
    g = np.asarray(grad, np.float64).reshape(4 * N, 3)
    vmin = ub * (g[:, 2] - mu * np.abs(g[:, 0]) - mu * np.abs(g[:, 1]))
    terms = (g * f).sum(1) - np.minimum(0.0, vmin)
    fn = 1.0 / np.sqrt(mui * mui + 1.0)
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    slack = np.stack([(mui * fx + fz) * fn, (-mui * fx + fz) * fn, (mui * fy + fz) * fn,
                      (-mui * fy + fz) * fn, fz, ub - fz], -1)
    cert = np.zeros(8)
    cert[COST], cert[COST0] = cost, cost0
    cert[GAP] = terms[stance].sum()
    cert[VIOL] = max(0.0, (-slack[stance]).max()) if stance.any() else 0.0
    cert[SWING] = np.abs(f[~stance]).max() if (~stance).any() else 0.0
    cert[GRADMAX] = np.abs(g[stance]).max() if stance.any() else 0.0
    return cert


def dense(orc, rec, prm, U):
    """-> (J, grad) from the dense fp64 condensation."""
    qH, qg = orc.fp64_condense(rec, prm)
    U = np.asarray(U, np.float64)
    return 0.5 * U @ qH @ U + qg @ U, qH @ U + qg


def trajectory(orc, rec, prm, U):
    """-> (x_pred [N, 12], cost, cost0, grad [12N]) by simulating the discretised model."""
    from scipy.linalg import expm
    N = prm.horizon
    A, B, Q = orc.ct_mats64(rec)
    M = np.zeros((31, 31))
    M[:13, :13] = A; M[:13, 13:25] = B; M[:13, 25:31] = Q
    E = expm(prm.dt * M)
    Ad, Bd, Qd = E[:13, :13], E[:13, 13:25], E[:13, 25:31]
    x0 = orc.condense(rec, prm, full=False)["x0"].astype(np.float64)
    f = np.zeros(6)
    if int(np.ascontiguousarray(rec[30:31], np.float32).view(np.uint32)[0]) & 1:
        f[3] = rec[29]
    W = np.array(list(prm.weights) + [0.0])
    xd = np.zeros((N, 13))
    xd[:, :12] = rec[32:32 + 12 * N].reshape(N, 12)
    u = np.asarray(U, np.float64).reshape(N, 12)
    alpha = float(prm.alpha)

    def run(uu):
        x, xs, c = x0, [], 0.0
        for k in range(N):
            x = Ad @ x + Bd @ uu[k] + Qd @ f
            xs.append(x)
            c += (W * (x - xd[k])) @ (x - xd[k])
        return np.array(xs), c + alpha * (uu * uu).sum()

    xs, cost = run(u)
    _, cost0 = run(np.zeros_like(u))
    lam = np.zeros(13)
    grad = np.zeros((N, 12))
    for k in range(N - 1, -1, -1):
        lam = Ad.T @ lam + 2.0 * W * (xs[k] - xd[k])
        grad[k] = Bd.T @ lam + 2.0 * alpha * u[k]
    return xs[:, :12], cost, cost0, grad.reshape(-1)


def evaluate(orc, rec, prm, U):
    """The reference the GPU tests compare with: x_pred, cost, cost0 from the trajectory path, the
    gradient words from the dense path -> (x_pred [N, 12] float64, cert [8])."""
    xs, cost, cost0, _ = trajectory(orc, rec, prm, U)
    _, grad = dense(orc, rec, prm, U)
    return xs, certificate(rec, prm, U, grad, cost, cost0)


def gap_bound(Hg, rec, prm, U, x64, dist):
    """An upper bound of the Frank-Wolfe gap of a feasible U that is within ``dist`` (inf-norm, in
    newtons) of the optimum U* = x64. With d = U - U* and y the gap's maximiser at U,
      gap(U) = grad(U).(U - y) = grad(U*).(U* - y) + grad(U*).d + d'H(U - y)
             <= 0 + |d|_inf (|grad(U*)|_1 + |H (U - y)|_1),
    the first term by U*'s optimality. ``Hg``: the caller's fp64 condensation (qH, qg) of the record,
    under its own robot model; the stance columns only are used."""
    N = prm.horizon
    ub, stance, mui = _consts(rec, prm)
    keep = np.repeat(stance, 3)
    H, g = Hg
    U = np.asarray(U, np.float64)
    grad = (H @ U + g).reshape(4 * N, 3)
    mu = 1.0 / mui
    y = np.zeros((4 * N, 3))
    lift = stance & (ub * (grad[:, 2] - mu * np.abs(grad[:, 0]) - mu * np.abs(grad[:, 1])) < 0)
    y[lift, 0] = -np.sign(grad[lift, 0]) * mu * ub[lift]
    y[lift, 1] = -np.sign(grad[lift, 1]) * mu * ub[lift]
    y[lift, 2] = ub[lift]
    g_opt = (H @ x64 + g)[keep]
    return dist * (np.abs(g_opt).sum() + np.abs((H @ (U - y.reshape(-1)))[keep]).sum())
