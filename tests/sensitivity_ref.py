"""numpy fp64 reference of BatchSolver.sensitivity (cmpc_batch_sensitivity), two independent paths
(a helper module, no tests in it; the product imports neither).

* dense: qH from ``oracle.fp64_condense``, Z from the SVD null space of each foot-step's active
  rows, ``np.linalg.solve`` on Z'HZ, and the gradients through the dense prediction matrices
  (Aqp, Bqp, Qqp built from powers of Adt);
* riccati: the backward Riccati recursion of include/cmpc_solver.h over the 12 dynamic states on
  the ``scipy.linalg.expm`` discretisation, a forward rollout and the adjoint sweep, plain loops.

Both take the face from ``face`` and x_k(U) from ``evaluate_ref.trajectory``. The conventions are
those of tests/evaluate_ref.py. A foot-step whose fz row is active, or both sides of one axis, is at
the apex: all of it is pinned (on the feasible set fz = 0 forces fx = fy = 0).
"""
import numpy as np

import evaluate_ref as er

X0, WEIGHTS, ALPHA, FEST3, FREE, SLACK, WORDS = 0, 12, 24, 25, 26, 27, 32


def slacks(rec, prm, U):
    """-> (normalised slack [4N, 6] in the order of CMPC_CERT_VIOL's rows, stance [4N], 1/mu)."""
    N = prm.horizon
    ub, stance, mui = er._consts(rec, prm)
    f = np.asarray(U, np.float64).reshape(4 * N, 3)
    fn = 1.0 / np.sqrt(mui * mui + 1.0)
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    s = np.stack([(mui * fx + fz) * fn, (-mui * fx + fz) * fn, (mui * fy + fz) * fn,
                  (-mui * fy + fz) * fn, fz, ub - fz], -1)
    return s, stance, mui


def face(rec, prm, U, act_tol):
    """-> (Z [12N, m] block diagonal over foot-steps, d [4N] free dimension per foot-step, the
    smallest slack of an inactive row of a stance foot-step)."""
    N = prm.horizon
    s, stance, mui = slacks(rec, prm, U)
    act = s <= act_tol
    normals = np.array([[mui, 0, 1], [-mui, 0, 1], [0, mui, 1], [0, -mui, 1], [0, 0, 1], [0, 0, 1.0]])
    blocks, d = [], np.zeros(4 * N, int)
    for t in range(4 * N):
        a = act[t]
        if not stance[t] or a[4] or (a[0] and a[1]) or (a[2] and a[3]):
            Zs = np.zeros((3, 0))
        elif not a.any():
            Zs = np.eye(3)
        else:
            _, sv, vt = np.linalg.svd(normals[a])
            Zs = vt[int((sv > 1e-9 * sv[0]).sum()):].T
        blocks.append(Zs)
        d[t] = Zs.shape[1]
    Z = np.zeros((12 * N, int(d.sum())))
    c = 0
    for t, Zs in enumerate(blocks):
        Z[3 * t:3 * t + 3, c:c + d[t]] = Zs
        c += d[t]
    free = s[stance][~act[stance]]
    return Z, d, (free.min() if free.size else np.inf)


def _model(orc, rec, prm):
    from scipy.linalg import expm
    A, B, Q = orc.ct_mats64(rec)
    M = np.zeros((31, 31))
    M[:13, :13] = A; M[:13, 13:25] = B; M[:13, 25:31] = Q
    E = expm(prm.dt * M)
    return E[:13, :13], E[:13, 13:25], E[:13, 25:31]


def _pack(N, dx0, dW, dalpha, dfest, m, slack, dtraj, w, rec):
    sens = np.zeros(WORDS)
    sens[X0:X0 + 12] = dx0
    sens[WEIGHTS:WEIGHTS + 12] = dW
    sens[ALPHA] = dalpha
    flag = int(np.ascontiguousarray(rec[30:31], np.float32).view(np.uint32)[0]) & 1
    sens[FEST3] = dfest if flag else 0.0
    sens[FREE], sens[SLACK] = m, slack
    return sens, np.asarray(dtraj).reshape(-1), np.asarray(w).reshape(-1)


def dense(orc, rec, prm, U, V, act_tol):
    """-> (sens [32], dtraj [12N], dg [12N])."""
    N = prm.horizon
    U, V = np.asarray(U, np.float64), np.asarray(V, np.float64)
    Z, d, slack = face(rec, prm, U, act_tol)
    qH, _ = orc.fp64_condense(rec, prm)
    w = -Z @ np.linalg.solve(Z.T @ qH @ Z, Z.T @ V) if Z.shape[1] else np.zeros(12 * N)
    Ad, Bd, Qd = _model(orc, rec, prm)
    P = [np.eye(13)]
    for _ in range(N):
        P.append(Ad @ P[-1])
    Bqp = np.zeros((13 * N, 12 * N)); Aqp = np.zeros((13 * N, 13)); Qqp = np.zeros((13 * N, 6))
    for r in range(N):
        Aqp[13 * r:13 * r + 13] = P[r + 1]
        for c in range(r + 1):
            Bqp[13 * r:13 * r + 13, 12 * c:12 * c + 12] = P[r - c] @ Bd
            Qqp[13 * r:13 * r + 13] += P[r - c] @ Qd
    W = np.array(list(prm.weights) + [0.0])
    S = np.tile(W, N)
    dX = Bqp @ w
    xs = er.trajectory(orc, rec, prm, U)[0]
    e = xs - rec[32:32 + 12 * N].reshape(N, 12).astype(np.float64)
    dXk = dX.reshape(N, 13)[:, :12]
    return _pack(N, (2 * Aqp.T @ (S * dX))[:12], 2 * (dXk * e).sum(0), 2 * w @ U,
                 2 * (S * dX) @ Qqp[:, 3], d.sum(), slack, -2 * W[:12] * dXk, w, rec)


def riccati(orc, rec, prm, U, V, act_tol):
    """-> (sens [32], dtraj [12N], dg [12N])."""
    N = prm.horizon
    U, V = np.asarray(U, np.float64), np.asarray(V, np.float64)
    Z, d, slack = face(rec, prm, U, act_tol)
    Ad, Bd, Qd = _model(orc, rec, prm)
    A, B, q3 = Ad[:12, :12], Bd[:12], Qd[:12, 3]
    W = np.diag(np.array(prm.weights, np.float64))
    alpha = float(prm.alpha)
    dk = d.reshape(N, 4).sum(1)
    col = np.concatenate([[0], np.cumsum(dk)])
    Zk = [Z[12 * k:12 * k + 12, col[k]:col[k + 1]] for k in range(N)]
    P, p = np.zeros((12, 12)), np.zeros(12)
    K, kap = [None] * N, [None] * N
    for k in range(N - 1, -1, -1):
        Pn, G = P + W, B @ Zk[k]
        R = alpha * Zk[k].T @ Zk[k] + G.T @ Pn @ G
        M = G.T @ Pn @ A
        K[k] = np.linalg.solve(R, M) if dk[k] else np.zeros((0, 12))
        kap[k] = np.linalg.solve(R, G.T @ p + 0.5 * Zk[k].T @ V[12 * k:12 * k + 12]) if dk[k] else np.zeros(0)
        P = A.T @ Pn @ A - M.T @ K[k]
        p = A.T @ p - M.T @ kap[k]
    dx = np.zeros((N + 1, 12))
    w = np.zeros((N, 12))
    for k in range(N):
        w[k] = Zk[k] @ (-K[k] @ dx[k] - kap[k])
        dx[k + 1] = A @ dx[k] + B @ w[k]
    lam, dfest = np.zeros(12), 0.0
    for k in range(N, 0, -1):
        lam = A.T @ lam + 2 * W @ dx[k]
        dfest += lam @ q3
    xs = er.trajectory(orc, rec, prm, U)[0]
    e = xs - rec[32:32 + 12 * N].reshape(N, 12).astype(np.float64)
    return _pack(N, A.T @ lam, 2 * (dx[1:] * e).sum(0), 2 * w.reshape(-1) @ U, dfest, d.sum(), slack,
                 -2 * np.diag(W) * dx[1:], w, rec)


BLOCKS = ("x0", "weights", "alpha", "fest3", "dtraj", "dg")


def blocks(out):
    """The output blocks the parity bars are taken over, by name."""
    sens, dtraj, dg = out
    return dict(x0=sens[X0:X0 + 12], weights=sens[WEIGHTS:WEIGHTS + 12], alpha=sens[ALPHA:ALPHA + 1],
                fest3=sens[FEST3:FEST3 + 1], dtraj=dtraj, dg=dg)


def rel(got, ref, tiny=1e-300):
    """|got - ref|_inf / max(|ref|_inf, tiny)."""
    return float(np.abs(np.asarray(got) - np.asarray(ref)).max() / max(np.abs(ref).max(), tiny))
