"""Inputs that make the convex-MPC solve fail, and the invariants every solve result must keep,
shared by tests/test_gpu_status.py and tests/test_status_cases.py (a helper module, no tests in it).

The levers (all deterministic, no API beyond make_params and the record words):

* alpha = -1: qH = 2 (B'SB + alpha I) with diag(B'SB) far below 1 (``btsb_diag_max``), so the first
  Cholesky pivot of every instance with a stance foot is negative: CMPC_NOT_PD.
* f_max = -120: a stance foot-step has ub = gait * f_max < 0, so fz >= 0 and fz <= ub exclude each
  other: CMPC_INFEASIBLE.
* one record word set to NaN, +Inf, -Inf or 3e38 (= kBigF of cmpc_common.h, the solver's "not a
  number any more" threshold). The words fall in three groups, read off the condensation
  (cmpc_common.h make_model / make_bdt / make_cond_geo / state_error, which cmpc_condense.hip and
  every solve kernel share) and confirmed against oracle.fp64_condense by tests/test_status_cases.py:

  - "g": p, v, omega, a trajectory entry at or behind the first step with a stance foot (row i
    reaches the stance foot-steps up to step i only), and f_est(3) when the record's flag bit is
    set. They enter x0, X_d or Q_qp f only: qg = 2 B_qp' S (A_qp x0 + Q_qp f - X_d). qH stays finite, every pivot
    passes, and without a check of the result the solve would end "optimal" with NaN forces.
    Expected status: CMPC_BAD_INPUT.
  - "H": a quaternion component (the rotation in B_c and A_c), a foot offset r of a leg that is in
    stance somewhere (the [r]x block of B_c) and x_drag (A_c[11][9], which the discretisation
    carries into Bdt rows 5 and 11). They reach qH, where the NaN meets a pivot first.
    Expected status: CMPC_BAD_INPUT or CMPC_NOT_PD.
  - "unused": the stored roll / pitch / yaw (the solve recomputes rpy from q) and f_est(3) while the
    flag bit is clear. The solve never reads them: status, forces and iters equal the clean record's.

The gait bytes are never touched, so a poisoned record stays in its size class and list.
"""
import functools

import numpy as np

from support import bits, package, records, reduced_sizes

OK, MAX_ITER, INFEASIBLE, NOT_PD, BAD_INPUT = 0, 1, 2, 3, 4
HANDOFF = 0xFE   # kHandoffStatus of cmpc_kernels.h: internal to the tail class, never a result

VALUES = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(3e38))
VALUE_NAMES = ("nan", "+inf", "-inf", "3e38")

# class 1 (60- / 64-wide builds), 65-72 (the tail class at N <= 10, the 80-column class above), wide 80 .. 256
CLASS_EDGES = [0, 60, 64, 72, 80, 96, 120, 128, 144, 192, 256]
CLASS_COPIES = 4   # constructed records per class at the end of clean_batch


def expected_classes(N):
    """The size classes a horizon-N record can fall in -> list of (lo, hi, n) with n the largest
    reduced size (a multiple of 3, at most 12 N) inside (lo, hi]."""
    out = []
    for lo, hi in zip(CLASS_EDGES[:-1], CLASS_EDGES[1:]):
        n = 3 * (min(hi, 12 * N) // 3)
        if n > lo:
            out.append((lo, hi, n))
    return out

# statuses a poisoned word of each group may end with
EXPECT = {"g": (BAD_INPUT,), "H": (BAD_INPUT, NOT_PD), "unused": (OK,)}


def status_counts(st):
    """np.bincount of a status array by name, for assertion messages."""
    names = records().STATUS_NAMES
    st = np.asarray(st).astype(np.int64).ravel()
    return {names.get(int(c), hex(int(c))): int((st == c).sum()) for c in np.unique(st)}


# ---- the words ----------------------------------------------------------------------------------
def levers(N, f_est=False):
    """-> list of (name, group, word) with word = index into the record, or a callable
    (record) -> index for the words that depend on the record's gait. ``f_est``: the records have
    their use-f_est flag set (clean_batch does it at N = 20), so word 29 reaches qg."""
    R = records()

    def stance_r(axis):
        def pick(rec):
            g = R.unpack_gait(rec[None], N)[0].reshape(N, 4)
            legs = np.nonzero(g.any(axis=0))[0]
            return None if legs.size == 0 else R.REC_R + 4 * axis + int(legs[0])
        return pick

    def traj_word(step, comp):
        # row i of the trajectory enters the error e_i, which reaches the gradient entries of the
        # stance foot-steps at or before step i only: the row is taken at or behind the record's
        # first stance step (a row ahead of it is a word the solve reads without effect)
        def pick(rec):
            g = R.unpack_gait(rec[None], N)[0].reshape(N, 4)
            steps = np.nonzero(g.any(axis=1))[0]
            return None if steps.size == 0 else R.REC_HDR + 12 * max(step, int(steps[0])) + comp
        return pick

    out = [("p_x", "g", R.REC_P), ("p_z", "g", R.REC_P + 2), ("v_y", "g", R.REC_V + 1),
           ("w_x", "g", R.REC_W), ("w_z", "g", R.REC_W + 2),
           ("traj[first stance][2]", "g", traj_word(0, 2)),   # yaw_des at the first step with a stance foot
           (f"traj[{N - 1}][5]", "g", R.REC_HDR + 12 * (N - 1) + 5),  # z_des of the last step
           (f"traj[>={N // 2}][7]", "g", traj_word(N // 2, 7)),       # a zero-weight component
           ("q_w", "H", R.REC_Q), ("q_y", "H", R.REC_Q + 2),
           ("r_x", "H", stance_r(0)), ("r_z", "H", stance_r(2)),
           ("x_drag", "H", R.REC_XDRAG),
           ("yaw", "unused", R.REC_RPY + 2)]
    out.append(("f_est", "g" if f_est else "unused", R.REC_FEST3))
    return out


def lever_cases(N, f_est=False):
    """Every (lever, value) pair -> list of (name, group, word, value, value name)."""
    return [(nm, grp, w, v, vn) for nm, grp, w in levers(N, f_est) for v, vn in zip(VALUES, VALUE_NAMES)]


def poison(rec, word, value):
    """A copy of one record with ``word`` (index or callable) set to ``value`` -> (record, index);
    (None, None) when the record has no such word (an all-swing record has no stance leg)."""
    w = word(rec) if callable(word) else int(word)
    if w is None:
        return None, None
    out = np.array(rec, np.float32)
    out[w] = value
    return out, w


# ---- batches ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clean_batch(N, B):
    """B records of the random-contact batch of tests/test_gpu_parity.py's
    test_large_batch_every_size_class_live (seed 8100 + N, every record with Bernoulli contacts).
    The random tables do not reach every size class (none above 96 at N = 10, none above 192 and
    one record in class 1 at N = 20), so the last CLASS_COPIES x classes records get constructed
    tables: for every class of expected_classes(N), CLASS_COPIES records with that class's reduced
    size, the stance foot-steps placed at random. At N = 20 every record has the use-f_est flag set
    and f_est(3) within +-10 N, so f_est reaches qg. Read-only."""
    R = records()
    recs = package().make_instances(B, N, seed=8100 + N, random_contact_frac=1.0)
    classes = expected_classes(N)
    rng = np.random.default_rng(7300 + N)
    go = R.gait_offset(N)
    gait = recs[:, go:go + N].view(np.uint8)   # [B, 4N] (a view)
    first = B - CLASS_COPIES * len(classes)
    for k, (lo, hi, n) in enumerate(classes):
        for j in range(CLASS_COPIES):
            row = np.zeros(4 * N, np.uint8)
            row[rng.choice(4 * N, n // 3, replace=False)] = 1
            gait[first + CLASS_COPIES * k + j] = row
    if N == 20:
        recs[:, R.REC_FEST3] = (10.0 * np.sin(np.arange(B, dtype=np.float64))).astype(np.float32)
        recs[:, R.REC_FLAGS] = np.ones(B, np.uint32).view(np.float32)
    recs.setflags(write=False)
    return recs


def all_zero_force_records(cm, B, N=10, seed=5):
    """n = 72 records (steps 0-5 all stance, 6-9 swing: the tail class) whose trajectory sinks
    fast (z 0.3 m lower per step, v_z -6 m/s): the optimum is zero force on every foot, pinned by
    three independent pyramid rows per stance foot-step, so the dual active set grows to 72
    positions, past the tail class's 64 lanes."""
    R = records()
    recs = cm.make_instances(B, N, seed=seed, random_contact_frac=0.0, gait="standing")
    g = np.zeros((B, 4 * N), np.uint8)
    g[:, :24] = 1
    recs[:, R.gait_offset(N):R.gait_offset(N) + N].view(np.uint8)[:, :] = g
    traj = recs[:, R.REC_HDR:R.REC_HDR + 12 * N].reshape(B, N, 12)
    for k in range(N):
        traj[:, k, 5] = recs[:, R.REC_P + 2] - 0.3 * (k + 1)
        traj[:, k, 11] = -6.0
    recs[:, R.REC_HDR:R.REC_HDR + 12 * N] = traj.reshape(B, -1)
    return recs


def poison_batch(recs, N, every=7, first=3, f_est=False, cover_classes=True):
    """Poison every ``every``-th record from ``first`` on, rotating through lever_cases, and (with
    ``cover_classes``) the first record of every size class that would otherwise have no poisoned
    record ahead of a clean one. -> (records, cases) with cases = {index: (name, group, word index,
    value name)}. Records without the lever's word (all swing) stay clean."""
    cases_all = lever_cases(N, f_est)
    out = np.array(recs, np.float32)
    cases = {}
    k = 0

    def hit(i, failing=False):
        nonlocal k
        for _ in range(len(cases_all)):
            nm, grp, word, val, vn = cases_all[k % len(cases_all)]
            k += 1
            if failing and grp == "unused":
                continue
            rec, w = poison(out[i], word, val)
            if rec is not None:
                out[i] = rec
                cases[int(i)] = (nm, grp, int(w), vn)
                return
    n = reduced_sizes(recs, N)
    for i in range(first, len(out), every):
        if n[i] > 0:
            hit(i)
    if cover_classes:
        for lo, hi in zip(CLASS_EDGES[:-1], CLASS_EDGES[1:]):
            idx = np.nonzero((n > lo) & (n <= hi))[0]
            if idx.size >= 2 and not _has_pair(idx, cases):
                if int(idx[0]) not in cases or cases[int(idx[0])][1] == "unused":
                    out[idx[0]] = recs[idx[0]]
                    hit(idx[0], failing=True)
                if int(idx[-1]) in cases:   # (a clean record behind it)
                    del cases[int(idx[-1])]
                    out[idx[-1]] = recs[idx[-1]]
    return out, cases


def _has_pair(idx, cases):
    """Does the class (record indices ``idx``, ascending) hold a record poisoned in a word the
    solve reads with a clean one behind it?"""
    clean = np.array([int(i) not in cases for i in idx])
    bad = np.array([int(i) in cases and cases[int(i)][1] != "unused" for i in idx])
    if not bad.any():
        return False
    return bool(clean[np.argmax(bad):].any())


def class_report(recs, N, cases):
    """Per size class: (lo, hi, instances, poisoned, has a poisoned record ahead of a clean one)."""
    n = reduced_sizes(recs, N)
    rows = []
    for lo, hi in zip(CLASS_EDGES[:-1], CLASS_EDGES[1:]):
        idx = np.nonzero((n > lo) & (n <= hi))[0]
        if idx.size:
            rows.append((lo + 1, hi, int(idx.size), sum(int(i) in cases for i in idx), _has_pair(idx, cases)))
    return rows


def format_report(rows):
    return " ".join(f"{lo}-{hi}:{cnt}/{bad}p{'' if pair else '(no pair)'}" for lo, hi, cnt, bad, pair in rows)


# ---- invariants ---------------------------------------------------------------------------------
def check_invariants(recs, prm, f, st, it, label="", f_max=None, mu=None):
    """Invariants 1 and 2 over a whole batch; raises AssertionError naming the first offender.

    1. status == 0: every force finite, swing legs exactly 0, friction pyramid to 1e-4 f_max.
    2. status != 0: every force word is +0.0 (bit pattern 0), iters within the cap
       max_iter + 2n + 1, status one of the four documented codes.
    ``f`` may hold the leading steps only (set_output_steps)."""
    N = prm.horizon
    f_max = abs(prm.f_max) if f_max is None else f_max
    mu = prm.mu if mu is None else mu
    B = recs.shape[0]
    st = np.asarray(st)
    it = np.asarray(it)
    f = np.asarray(f, np.float32).reshape(B, -1)
    steps = f.shape[1] // 12
    n = reduced_sizes(recs, N)
    known = np.isin(st, (OK, MAX_ITER, INFEASIBLE, NOT_PD, BAD_INPUT))
    assert known.all(), f"{label}: undocumented status {status_counts(st[~known])} at {np.nonzero(~known)[0][:8]}"
    cap = prm.max_iter + 2 * n + 1
    assert ((it >= 0) & (it <= cap)).all(), \
        f"{label}: iters outside 0..max_iter+2n+1 at {np.nonzero((it < 0) | (it > cap))[0][:8]}"
    ok = st == OK
    fb = bits(f)
    nz = (fb[~ok] != 0).any(axis=1)
    assert not nz.any(), (f"{label}: {int(nz.sum())} failed instances with a force word that is not +0.0 "
                          f"(first: {np.nonzero(~ok)[0][nz][:8]}, status {status_counts(st[~ok][nz])})")
    fo = f[ok]
    fin = np.isfinite(fo).all(axis=1)
    assert fin.all(), (f"{label}: {int((~fin).sum())} instances with status ok and a non-finite force "
                       f"(first: {np.nonzero(ok)[0][~fin][:8]})")
    gait = records().unpack_gait(recs, N).reshape(B, N, 4)[:, :steps][ok]
    F = fo.reshape(-1, steps, 4, 3)
    swing = gait == 0
    assert (bits(np.ascontiguousarray(F[swing])) == 0).all(), f"{label}: a swing leg's force is not +0.0"
    F = F.astype(np.float64)
    fx, fy, fz = F[..., 0], F[..., 1], F[..., 2]
    tol = 1e-4 * f_max
    assert (fz >= -tol).all() and (fz <= f_max + tol).all(), f"{label}: fz outside [0, f_max]"
    assert (np.abs(fx) <= mu * fz + tol).all() and (np.abs(fy) <= mu * fz + tol).all(), \
        f"{label}: friction pyramid violated"


def check_poisoned(cases, st, label=""):
    """Invariant 3: the status of every poisoned record is one its word's group allows."""
    wrong = [(i, c, int(st[i])) for i, c in cases.items() if int(st[i]) not in EXPECT[c[1]]]
    names = records().STATUS_NAMES
    assert not wrong, (f"{label}: {len(wrong)} of {len(cases)} poisoned records with a status their word does not "
                       f"allow, first: " + "; ".join(f"#{i} {c[0]}={c[3]} ({c[1]}) -> {names.get(s, hex(s))}"
                                                     for i, c, s in wrong[:6]))


# ---- CPU references -----------------------------------------------------------------------------
def btsb_diag_max(recs, prm, fp64=True):
    """max diag(B'SB) per record over the stance variables (qH = 2 (B'SB + alpha I)), from
    oracle.fp64_condense, or (``fp64`` False) from the oracle's fp32 restatement of the reference's
    condensation, which is some hundred times faster; 0 for an all-swing record."""
    from oracle import oracle as orc
    N = prm.horizon
    gait = records().unpack_gait(recs, N)
    out = np.zeros(len(recs))
    for i in range(len(recs)):
        qH = orc.fp64_condense(recs[i], prm)[0] if fp64 else orc.condense(recs[i], prm, full=True)["qH"]
        d = np.diag(qH).astype(np.float64) / 2 - prm.alpha
        keep = np.repeat(gait[i] != 0, 3)
        out[i] = d[keep].max() if keep.any() else 0.0
    return out
