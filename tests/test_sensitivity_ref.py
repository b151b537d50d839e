"""The numpy reference of cmpc_batch_sensitivity (tests/sensitivity_ref.py) against itself and against
the solve: its two paths agree over the GPU tests' pool, and what it returns is the derivative of
``oracle.fp64_solve`` (central differences). CPU only.
"""
import numpy as np
import pytest

import sensitivity_cases as sc
import sensitivity_ref as sr
from conftest import golden_params, load_golden
from support import needs_ref  # noqa: F401


def _disagreement(a, b):
    A, B = sr.blocks(a), sr.blocks(b)
    return {k: sr.rel(B[k], A[k]) for k in sr.BLOCKS}


def test_two_paths_agree(cm, orc):
    """Dense KKT against Riccati, per output block norm-wise, over the whole pool and the end-to-end
    sets, per horizon: the reference's own noise, from which the GPU bars (sensitivity_cases.bar(N) =
    300 x REF_NOISE[N]) are taken. Measured: the table of sensitivity_cases.REF_NOISE. Asserted within
    10 x REF_NOISE only: another BLAS rounds differently, a broken path misses by orders of
    magnitude."""
    worst = {}
    for case in sc.CASES:
        p = sc.pool(cm, orc, case)
        N = p["prm"].horizon
        for i, (a, b) in enumerate(zip(p["den"], p["ric"])):
            assert a[0][sr.FREE] == b[0][sr.FREE] and a[0][sr.SLACK] == b[0][sr.SLACK]
            for k, r in _disagreement(a, b).items():
                if r > worst.get(N, (0.0, ""))[0]:
                    worst[N] = (r, f"{k} of {case}[{i}]")
    for name in sc.E2E_SETS:
        prm, recs, V, q = sc.e2e_inputs(cm, name)
        N = prm.horizon
        for i, (r, u, v) in enumerate(zip(recs, q, V)):
            d = _disagreement(sr.dense(orc, r, prm, u, v, sc.ACT_TOL), sr.riccati(orc, r, prm, u, v, sc.ACT_TOL))
            k = max(d, key=d.get)
            if d[k] > worst.get(N, (0.0, ""))[0]:
                worst[N] = (d[k], f"{k} of {name}[{i}]")
    print("[sensitivity_ref] dense against Riccati, worst per horizon: " +
          ", ".join(f"N={N} {v[0]:.1e} ({v[1]})" for N, v in sorted(worst.items())))
    assert sorted(worst) == sorted(sc.REF_NOISE)
    for N, v in worst.items():
        assert v[0] <= 10 * sc.REF_NOISE[N], (N, v)


def test_face_types(cm, orc):
    """The hand-built forces land on the faces they were built for: m as counted by type."""
    seen = 0
    for case in sc.CASES:
        p = sc.pool(cm, orc, case)
        for i, m in p["m_faces"].items():
            assert p["ric"][i][0][sr.FREE] == m, (case, i)
            seen += m > 0
    assert seen >= len(sc.CASES)


FD_SETS = sc.E2E_SETS


@pytest.mark.parametrize("name", FD_SETS)
def test_derivative_of_the_solve(cm, orc, needs_ref, name):
    """L = V.U*(theta) with U* = oracle.fp64_solve: the analytic gradient at U* (face at 1e-6 N)
    against central differences, for three instances per set. p_z and a trajectory word (steps of
    2^-10, exact in fp32; the map is linear on the face): 1e-8 relative. Three weights (relative step
    1e-4 of an fp32 parameter): 1e-3 relative, the step's own error."""
    g = load_golden(name)
    prm = golden_params(cm, g)
    N = prm.horizon
    rng = np.random.default_rng(977 + N)
    h = 2.0 ** -10
    for i in range(3):
        rec = g["records"][i]
        V = rng.standard_normal(12 * N)
        U, _ = orc.fp64_solve(rec, prm)
        sens, dtraj, _ = sr.riccati(orc, rec, prm, U, V, 1e-6)
        assert sens[sr.SLACK] > 1e-2, (name, i, sens[sr.SLACK])
        assert sens[sr.FREE] > 0

        def loss(r, p=prm):
            return V @ orc.fp64_solve(r, p)[0]

        k, j = N // 3, 5                       # the desired height of step k
        for word, want in ((2, sens[sr.X0 + 5]), (32 + 12 * k + j, dtraj[12 * k + j])):
            rp, rm = rec.copy(), rec.copy()
            rp[word] += np.float32(h)
            rm[word] -= np.float32(h)
            assert float(rp[word]) - float(rm[word]) == 2 * h
            fd = (loss(rp) - loss(rm)) / (2 * h)
            print(f"[sensitivity_ref] {name}[{i}] word {word}: analytic {want:.12e} fd {fd:.12e}")
            assert abs(fd - want) <= 1e-8 * abs(want), (name, i, word, fd, want)
        base = [float(x) for x in prm.weights]
        for jw in (2, 5, 11):                  # yaw, height, v_z: non-zero in the golden sets
            assert base[jw] > 0
            out = []
            for sgn in (1, -1):
                w = list(base)
                w[jw] = base[jw] * (1 + sgn * 1e-4)
                pw = cm.make_params(N, dt=float(prm.dt), mu=float(prm.mu), f_max=float(prm.f_max),
                                    weights=tuple(w), alpha=float(prm.alpha))
                out.append((float(pw.weights[jw]), loss(rec, pw)))
            fd = (out[0][1] - out[1][1]) / (out[0][0] - out[1][0])
            want = sens[sr.WEIGHTS + jw]
            print(f"[sensitivity_ref] {name}[{i}] weight {jw}: analytic {want:.9e} fd {fd:.9e}")
            assert abs(fd - want) <= 1e-3 * abs(want), (name, i, jw, fd, want)
