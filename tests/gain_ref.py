"""numpy fp64 reference of BatchSolver.gain (cmpc_batch_gain) and BatchSolver.feedback
(cmpc_batch_feedback): a helper module, no tests in it; the product imports neither.

The gain G = d u_0* / d x_0 of the minimiser over the face U lies on, by two independent paths that
share only ``sensitivity_ref.face`` and ``sensitivity_ref._model``:

* riccati: the backward recursion of include/cmpc_solver.h over the 12 dynamic states, from P = 0
  with Pn = P + W and G_k = Bdt Z_k: R = alpha Z_k'Z_k + G_k'Pn G_k, P_k = Adt'Pn Adt -
  (Adt'Pn G_k) R^-1 (G_k'Pn Adt), and at k = 0 K_0 = R^-1 G_0'Pn Adt, G = -Z_0 K_0;
* dense: rows 0..11 of -Z (Z'HZ)^-1 Z' 2 B_qp'S A_qp[:, :12] with ``oracle.fp64_condense``'s H (qg =
  2 B_qp'S (A_qp x_0 - xd), so 2 B_qp'S A_qp is d qg / d x_0).

Both return the CMPC_GAIN_WORDS doubles of one instance. ``feedback`` is cmpc_batch_feedback's
arithmetic in numpy: the wrapped difference, u_0 + G delta, the guard, one rounding to fp32.
"""
import numpy as np

import evaluate_ref as er
import sensitivity_ref as sr

K, FREE, FREE0, SLACK, WORDS = 0, 144, 145, 146, 148


def _pack(G, d, slack):
    out = np.zeros(WORDS)
    out[K:K + 144] = np.asarray(G).reshape(-1)
    out[FREE], out[FREE0], out[SLACK] = d.sum(), d[:4].sum(), slack
    return out


def riccati(orc, rec, prm, U, act_tol):
    N = prm.horizon
    Z, d, slack = sr.face(rec, prm, np.asarray(U, np.float64), act_tol)
    Ad, Bd, _ = sr._model(orc, rec, prm)
    A, B = Ad[:12, :12], Bd[:12]
    W = np.diag(np.array(prm.weights, np.float64))
    alpha = float(prm.alpha)
    dk = d.reshape(N, 4).sum(1)
    col = np.concatenate([[0], np.cumsum(dk)])
    P = np.zeros((12, 12))
    G = np.zeros((12, 12))
    for k in range(N - 1, -1, -1):
        Zk = Z[12 * k:12 * k + 12, col[k]:col[k + 1]]
        Pn, Gk = P + W, B @ Zk
        M = Gk.T @ Pn @ A
        if dk[k]:
            Kk = np.linalg.solve(alpha * Zk.T @ Zk + Gk.T @ Pn @ Gk, M)
            P = A.T @ Pn @ A - M.T @ Kk
            if k == 0:
                G = -(Zk @ Kk) + 0.0   # pinned rows +0.0, not -0.0
        else:
            P = A.T @ Pn @ A
    return _pack(G, d, slack)


def dense(orc, rec, prm, U, act_tol):
    N = prm.horizon
    Z, d, slack = sr.face(rec, prm, np.asarray(U, np.float64), act_tol)
    if d[:4].sum() == 0:
        return _pack(np.zeros((12, 12)), d, slack)
    qH, _ = orc.fp64_condense(rec, prm)
    Ad, Bd, _ = sr._model(orc, rec, prm)
    pw = [np.eye(13)]
    for _ in range(N):
        pw.append(Ad @ pw[-1])
    Bqp = np.zeros((13 * N, 12 * N))
    Aqp = np.zeros((13 * N, 13))
    for r in range(N):
        Aqp[13 * r:13 * r + 13] = pw[r + 1]
        for c in range(r + 1):
            Bqp[13 * r:13 * r + 13, 12 * c:12 * c + 12] = pw[r - c] @ Bd
    S = np.tile(np.array(list(prm.weights) + [0.0]), N)
    dg = 2.0 * Bqp.T @ (S[:, None] * Aqp[:, :12])
    full = -Z @ np.linalg.solve(Z.T @ qH @ Z, Z.T @ dg)
    return _pack(full[:12] + 0.0, d, slack)


def x0(orc, rec, prm):
    """x_0 in the order of the traj rows, as the kernels form it (rpy of quat_to_rpy rounded to fp32)."""
    return orc.condense(rec, prm, full=False)["x0"].astype(np.float64)[:12]


def feedback(orc, rec, prm, u0, gain, state):
    """-> the 12 corrected step-0 forces, float32. ``u0`` the held step-0 forces [12] float32, ``gain``
    the instance's CMPC_GAIN_WORDS doubles, ``state`` the present state [12] float32 in traj-row order."""
    ub, stance, mui = er._consts(rec, prm)
    mu = 1.0 / mui
    delta = np.asarray(state, np.float32).astype(np.float64) - x0(orc, rec, prm)
    delta[:3] -= 2.0 * np.pi * np.rint(delta[:3] / (2.0 * np.pi))
    u = np.asarray(u0, np.float32).astype(np.float64) + np.asarray(gain[K:K + 144]).reshape(12, 12) @ delta
    out = np.zeros(12, np.float32)
    for f in range(4):
        if not stance[f]:
            continue
        fz = min(max(u[3 * f + 2], 0.0), ub[f])
        out[3 * f + 2] = fz
        out[3 * f] = min(max(u[3 * f], -mu * fz), mu * fz)
        out[3 * f + 1] = min(max(u[3 * f + 1], -mu * fz), mu * fz)
    return out
