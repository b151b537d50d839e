"""Pins the numpy reference of BatchSolver.evaluate (tests/evaluate_ref.py) on the CPU: its two
independent paths (dense fp64 condensation / simulated trajectory with a numpy adjoint) agree to
rounding, and the Frank-Wolfe gap bounds the cost distance to the fp64 optimum.

Measured when this test was written (18 instances): cost - cost0 vs J at most 1.8e-15 relative,
the two gradients at most 4.8e-15 apart; the bars below leave a factor of ~50 / ~20.
"""
import numpy as np
import pytest

import evaluate_ref as er
from conftest import golden_params, load_golden

SETS = ["n10_mixed", "n16_trot", "n20_standing"]
PER_SET = 6


def instances(cm):
    for name in SETS:
        g = load_golden(name)
        prm = golden_params(cm, g)
        for i in range(PER_SET):
            yield name, i, prm, g["records"][i], g["q_ref"][i]


def test_dense_and_trajectory_paths_agree(cm, orc):
    worst_j, worst_g = 0.0, 0.0
    for name, i, prm, rec, q in instances(cm):
        J, gd = er.dense(orc, rec, prm, q)
        _, cost, cost0, gt = er.trajectory(orc, rec, prm, q)
        rj = abs((cost - cost0) - J) / abs(J)
        rg = np.abs(gd - gt).max()
        worst_j, worst_g = max(worst_j, rj), max(worst_g, rg)
        assert rj <= 1e-13, (name, i, rj)
        assert rg <= 1e-13, (name, i, rg)
    print(f"[evaluate_ref] cost - cost0 vs J: {worst_j:.2e} relative; gradients: {worst_g:.2e} absolute")


def test_x0_is_the_pipelines(cm, orc):
    """x_0's rpy: fp32 arguments with every operation rounded, fp64 atan2 / asin, rounded to fp32
    (what the evaluate kernel restates) is bit for bit the restated pipeline's x0."""
    f32 = np.float32
    for name, i, prm, rec, _ in instances(cm):
        w, x, y, z = [f32(v) for v in rec[6:10]]
        asd = min(-2.0 * float(f32(f32(x * z) - f32(w * y))), 0.99999)
        ww, xx, yy, zz = f32(w * w), f32(x * x), f32(y * y), f32(z * z)
        rpy = [f32(np.arctan2(float(f32(2) * f32(f32(y * z) + f32(w * x))), float(f32(f32(f32(ww - xx) - yy) + zz)))),
               f32(np.arcsin(float(f32(asd)))),
               f32(np.arctan2(float(f32(2) * f32(f32(x * y) + f32(w * z))), float(f32(f32(f32(ww + xx) - yy) - zz))))]
        x0 = orc.condense(rec, prm, full=False)["x0"]
        assert [float(v) for v in rpy] == [float(v) for v in x0[:3]], (name, i, rpy, x0[:3])
        assert float(x0[12]) == float(f32(-9.8))


def test_gap_bounds_the_distance_to_the_optimum(cm, orc):
    if not orc.ref_available():
        pytest.skip("oracle/_ref not present")
    for name, i, prm, rec, q in instances(cm):
        x64, _ = orc.fp64_solve(rec, prm)
        cert_q = er.evaluate(orc, rec, prm, q)[1]
        cert_x = er.evaluate(orc, rec, prm, x64)[1]
        tol = 1e-12 * max(1.0, cert_q[er.COST0])
        assert cert_q[er.GAP] >= cert_q[er.COST] - cert_x[er.COST] - tol, (name, i)
        assert cert_x[er.GAP] >= -tol, (name, i, cert_x[er.GAP])
