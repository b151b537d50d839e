"""The numpy reference of cmpc_batch_gain (tests/gain_ref.py) against itself and against the solve: its
two paths agree over the GPU tests' pool, what it returns is the derivative of ``oracle.fp64_solve``'s
step-0 forces (central differences), and it has the structure include/cmpc_solver.h states. CPU only.
"""
import numpy as np
import pytest

import gain_cases as gc
import gain_ref as gr
import sensitivity_cases as sc
import sensitivity_ref as sr
from conftest import golden_params, load_golden
from support import needs_ref  # noqa: F401


def test_two_paths_agree(cm, orc):
    """Dense KKT against Riccati, norm-wise per instance relative to |G|_inf of the Riccati path, over
    the whole pool and the end-to-end sets, per horizon: the reference's own noise, from which the GPU
    bars (gain_cases.bar(N) = 300 x REF_NOISE[N]) are taken. Where step 0 has no free direction both
    paths give exactly 0. Measured: the table of gain_cases.REF_NOISE. Asserted within 10 x REF_NOISE
    only: another BLAS rounds differently, a broken path misses by orders of magnitude."""
    worst, total, empty = {}, 0, 0
    for case in gc.CASES:
        p = gc.pool(cm, orc, case)
        N = p["prm"].horizon
        for i, (a, b) in enumerate(zip(p["gden"], p["gric"])):
            assert (a[144:] == b[144:]).all() and b[147] == 0, (case, i)
            total += 1
            if b[gr.FREE0] == 0:
                empty += 1
                assert not a[:144].any() and not b[:144].any(), (case, i)
                continue
            assert np.abs(b[:144]).max() > 0, (case, i)
            r = gc.rel(a, b)
            if r > worst.get(N, (0.0, ""))[0]:
                worst[N] = (r, f"{case}[{i}]")
    for name in gc.E2E_SETS:
        prm, recs, _, q = sc.e2e_inputs(cm, name)
        N = prm.horizon
        for i, (r, u) in enumerate(zip(recs, q)):
            e = gc.rel(gr.dense(orc, r, prm, u, gc.ACT_TOL), gr.riccati(orc, r, prm, u, gc.ACT_TOL))
            if e > worst.get(N, (0.0, ""))[0]:
                worst[N] = (e, f"{name}[{i}]")
    print(f"[gain_ref] step 0 without a free direction: {empty} of {total} instances")
    print("[gain_ref] dense against Riccati, worst per horizon: " +
          ", ".join(f"N={N} {v[0]:.1e} ({v[1]})" for N, v in sorted(worst.items())))
    assert (empty, total) == (31, 188)
    assert sorted(worst) == sorted(gc.REF_NOISE)
    for N, v in worst.items():
        assert v[0] <= 10 * gc.REF_NOISE[N], (N, v)


@pytest.mark.parametrize("name", list(gc.FD_INSTANCES))
def test_derivative_of_the_solve(cm, orc, needs_ref, name):
    """Columns 3..11 of G at U* = oracle.fp64_solve (face at 1e-6 N) against central differences of
    U*'s step-0 forces in the record's p, w and v words (steps of 2^-10, exact in fp32; the optimum is
    affine on the face): 1e-9 |G|_inf. Measured: <= 3.2e-11."""
    g = load_golden(name)
    prm = golden_params(cm, g)
    h = 2.0 ** -10
    for i in gc.FD_INSTANCES[name]:
        rec = g["records"][i]
        U, _ = orc.fp64_solve(rec, prm)
        out = gr.riccati(orc, rec, prm, U, 1e-6)
        assert out[gr.SLACK] > 1e-2, (name, i, out[gr.SLACK])
        assert out[gr.FREE0] > 0
        G = out[:144].reshape(12, 12)
        fd = np.zeros((12, 12))
        for c, word in gc.X0_WORD.items():
            rp, rm = rec.copy(), rec.copy()
            rp[word] += np.float32(h)
            rm[word] -= np.float32(h)
            assert float(rp[word]) - float(rm[word]) == 2 * h
            fd[:, c] = (orc.fp64_solve(rp, prm)[0][:12] - orc.fp64_solve(rm, prm)[0][:12]) / (2 * h)
        err = np.abs(fd[:, 3:] - G[:, 3:]).max() / np.abs(G).max()
        print(f"[gain_ref] {name}[{i}]: |G|_inf {np.abs(G).max():.3e}, central differences off by {err:.1e} of it")
        assert err <= 1e-9, (name, i, err)


def test_structure(cm, orc):
    seen = 0
    for case in gc.CASES:
        p = gc.pool(cm, orc, case)
        for i in p["m_faces"]:
            for key in ("gric", "gden"):
                seen += gc.structure(cm, p, i, p[key][i]) > 0
            assert p["gric"][i][gr.FREE] == p["m_faces"][i]
    assert seen >= len(gc.CASES)
