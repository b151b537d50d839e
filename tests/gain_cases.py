"""The data of the gain tests (tests/test_gain_ref.py, tests/test_gpu_gain.py): a helper module, no
tests in it. The records and forces are the pool of tests/sensitivity_cases.py (its upstream gradients
are not used); per case both numpy references of tests/gain_ref.py, computed once per process.
"""
import numpy as np

import gain_ref as gr
import sensitivity_cases as sc
import sensitivity_ref as sr
from sensitivity_cases import ACT_TOL, CASES, E2E_SETS  # noqa: F401

# The parity bar of the GPU tests, norm-wise per instance and per horizon: 300 x the largest
# disagreement of the two numpy paths at that horizon, relative to |G|_inf of the Riccati path, over the
# pool of sensitivity_cases.CASES (N = 1, 2, 10, 11, 20) and over the six golden instances of each
# end-to-end set (which adds N = 16). tests/test_gain_ref.py measures and prints them; the factor is
# the one tests/test_gpu_evaluate.py and tests/test_gpu_sensitivity.py use for a kernel's summation
# order and contraction. Measured: N = 1 1.4e-15 (n1), 2 1.1e-15 (n2@W1), 10 1.9e-14 (n10_edge@W1), 11 1.3e-14
# (n11), 16 1.5e-13 (n16_trot), 20 2.2e-11 (n20_standing): the disagreement grows with the conditioning of
# Z'HZ, as sensitivity's does.
REF_NOISE = {1: 1.4e-15, 2: 1.1e-15, 10: 1.9e-14, 11: 1.3e-14, 16: 1.5e-13, 20: 2.2e-11}

# The instances of the finite-difference test and of the end-to-end feedback test: those of the first
# six of each golden set whose fp64 optimum keeps its face inside +-2^-10 of every p, w, v word
# (n16_trot[4], n16_trot[5] and n20_standing[1] change face there).
FD_INSTANCES = {"n10_mixed": (0, 1, 2), "n16_trot": (0, 1, 2), "n20_standing": (0, 2, 3)}
# record word of column c of G for c = 3..11: p, w, v (the rpy columns have no record word: the
# quaternion also forms R)
X0_WORD = {3: 0, 4: 1, 5: 2, 6: 10, 7: 11, 8: 12, 9: 3, 10: 4, 11: 5}


def bar(N):
    return 300 * REF_NOISE[N]


def rel(got, ref, tiny=1e-300):
    """|got - ref|_inf / max(|ref|_inf, tiny) over the 144 words of G."""
    g, r = np.asarray(got)[..., :144], np.asarray(ref)[..., :144]
    return float(np.abs(g - r).max() / max(np.abs(r).max(), tiny))


_POOLS = {}


def pool(cm, orc, case):
    """sensitivity_cases.pool(case) with ``gric`` and ``gden`` added: [K, CMPC_GAIN_WORDS] of either
    path. Computed once; leave it unchanged."""
    if case not in _POOLS:
        p = dict(sc.pool(cm, orc, case))
        for key, fn in (("gric", gr.riccati), ("gden", gr.dense)):
            p[key] = np.array([fn(orc, r, p["prm"], u, ACT_TOL) for r, u in zip(p["recs"], p["U"])])
            p[key].setflags(write=False)
        _POOLS[case] = p
    return _POOLS[case]


def structure(cm, p, i, out):
    """What include/cmpc_solver.h states of G's rows, on instance i of a pool whose forces were built by
    sensitivity_cases.face_forces: swing and pinned rows exactly 0, the rows of a foot-step orthogonal
    to its active normals, FREE0 as counted by face type."""
    prm, rec, U = p["prm"], p["recs"][i], p["U"][i]
    G = out[:144].reshape(12, 12)
    gmax = np.abs(G).max()
    st = sc.stance(cm, prm, rec)
    s, _, mui = sr.slacks(rec, prm, U)
    normals = np.array([[mui, 0, 1], [-mui, 0, 1], [0, mui, 1], [0, -mui, 1], [0, 0, 1], [0, 0, 1.0]])
    kinds = {t: sc.FACES[n % len(sc.FACES)] for n, t in enumerate(np.flatnonzero(st))}
    free0 = 0
    for t in range(4):
        rows = G[3 * t:3 * t + 3]
        dim = sc.FACE_DIM[kinds[t]] if st[t] else 0
        free0 += dim
        if dim == 0:
            assert not rows.any() and not np.signbit(rows).any(), (i, t)
            continue
        for a in np.flatnonzero(s[t] <= ACT_TOL):
            assert np.abs(normals[a] @ rows).max() <= 1e-12 * gmax, (i, t, int(a))
    assert out[gr.FREE0] == free0, (i, out[gr.FREE0], free0)
    return free0
