"""The float64 yardstick with the robot model as an argument (tests/model_ref.py), on the CPU.

tests/test_gpu_model.py holds the kernels to model_ref.fp64_solve under five models. That is worth
what the helper is worth, so here it is tied to oracle.py, which knows only m = 12 and
I_body = diag(.07, .26, .242):

 1. at the default model it is oracle.fp64_solve (measured distance 0.0);
 2. the scaling identity: the model (c m, c I) under (alpha, f_max) has c x the optimum of the default
    model under (c^2 alpha, f_max / c): B -> B / c, the friction cone is homogeneous, only the fz bound
    and the regulariser rescale. For c = 2 ("x2") both sides agree within 9e-14;
 3. the optimum moves by more than ten gates under every tamper a kernel could commit (two inertia
    entries swapped, the mass or the inertia left at the default), on every instance used: measured
    minimum 4.1e-3 ("heavy", entries 1 <-> 2, N = 10);
 4. the fp32 horizons' condition on the inputs: condensing in fp32 (the discretised matrices rounded
    to fp32, the products in fp32) moves the optimum of every gated model by at most REF_COND = 5e-5,
    half the N <= 10 gate (measured <= 1e-5; 1.4e-4 for "mini", which is why that model is reported
    and not gated).

Skipped without oracle/_ref (qpOASES), as the other tests of the float64 optimum are.
"""
import functools

import numpy as np
import pytest

import model_ref as mr
import param_sets as ps
from support import FP64_TOL, REF_COND, REF_TOL, needs_ref, package  # noqa: F401

pytestmark = pytest.mark.usefixtures("needs_ref")

# case -> leading instances used
DEFAULT_INPUTS = {"n10_families": 32, "n16_trot": 6, "n20_standing": 2}


@functools.lru_cache(maxsize=None)
def _x64(model_key, case, k):
    """fp64 optimum of the case's first k records under a model given as (mass, inertia) or a name."""
    cm = package()
    mdl = mr.model(model_key) if isinstance(model_key, str) else cm.make_model(*model_key)
    N = ps.CASES[case][0]
    x, ri = mr.fp64_batch(ps.case_records("default", case)[:k], ps.set_params("default", N), mdl)
    assert (ri == 0).all(), ri
    return x


@pytest.mark.parametrize("case", list(DEFAULT_INPUTS))
def test_default_model_is_the_oracle(orc, case):
    k = DEFAULT_INPUTS[case]
    N = ps.CASES[case][0]
    prm = ps.set_params("default", N)
    recs = ps.case_records("default", case)[:k]
    want, ri = ps.fp64_batch(orc, recs, prm)
    assert (ri == 0).all()
    dist = ps.rel_dist(_x64("default", case, k), want)
    print(f"[model] default model vs oracle.fp64_solve, {case}: {dist.max():.1e}")
    assert dist.max() <= 1e-12
    # and the matrices themselves
    A, B, Q = mr.ct_mats64(recs[0], mr.model("default"))
    A0, B0, Q0 = orc.ct_mats64(recs[0])
    assert np.array_equal(A, A0) and np.array_equal(Q, Q0) and np.abs(B - B0).max() <= 1e-12 * np.abs(B0).max()


@pytest.mark.parametrize("case", list(DEFAULT_INPUTS))
def test_scaling_identity(cm, orc, case):
    k = DEFAULT_INPUTS[case]
    N = ps.CASES[case][0]
    p0 = cm.make_params(N)
    recs = ps.case_records("default", case)[:k]
    scaled, ri = ps.fp64_batch(orc, recs, cm.make_params(N, alpha=4 * p0.alpha, f_max=p0.f_max / 2))
    assert (ri == 0).all()
    dist = ps.rel_dist(_x64("x2", case, k), 2 * scaled)
    print(f"[model] x2 vs 2 x oracle(4 alpha, f_max / 2), {case}: {dist.max():.1e}")
    assert dist.max() <= 1e-10


def _tampers(name):
    m, I = mr.MODELS[name]
    out = {}
    for i, j in ((0, 1), (1, 2), (0, 2)):
        J = list(I)
        J[i], J[j] = J[j], J[i]
        out[f"swap{i}-{j}"] = (m, tuple(J))
    out["mass12"] = (mr.DEFAULT[0], I)
    out["inertia-default"] = (m, mr.DEFAULT[1])
    return out


SENS_INPUTS = {10: ("n10_families", 32), 16: ("n16_trot", 6)}


@pytest.mark.parametrize("N", [10, 16])
@pytest.mark.parametrize("tamper", ["swap0-1", "swap1-2", "swap0-2", "mass12", "inertia-default"])
@pytest.mark.parametrize("name", ["heavy", "payload"])
def test_optimum_sees_tampered_model(name, tamper, N):
    """The analogue of test_gpu_params.test_optimum_sees_tampered_weights: the fp64 optimum under the
    model against the optimum under the tampered model differs by more than 10 x the horizon's gate
    on every instance used, so a kernel family that used Ib1 for Ib2, or kept a stray 1/12, misses
    the gate of tests/test_gpu_model.py."""
    case, k = SENS_INPUTS[N]
    x = _x64(name, case, k)
    xt = _x64(_tampers(name)[tamper], case, k)
    dist = ps.rel_dist(xt, x)
    bar = 10 * (REF_TOL if N <= 10 else FP64_TOL)
    print(f"[model] {name} {tamper} N={N}: optimum moves by {dist.min():.1e} (min) .. {dist.max():.1e} "
          f"over {len(dist)} instances; bar {bar:.0e}")
    assert dist.min() > bar, (name, tamper, N, dist.min())


@pytest.mark.parametrize("case", ["n10_families", "n3_padding"])
@pytest.mark.parametrize("name", mr.GATED)
def test_fp32_condensation_condition(name, case):
    """Every gated model's fp32-condensed optimum is within REF_COND of its fp64 optimum on the fp32
    horizons' cases, so a miss of the N <= 10 gate cannot be the precision of the condensation."""
    d = mr.cpu_data(name, case)
    assert (d["ri64"] == 0).all(), d["ri64"]
    x32, ri = mr.fp64_batch(d["recs"], d["prm"], mr.model(name), dtype=np.float32)
    assert (ri == 0).all(), ri
    dist = ps.rel_dist(x32, d["x64"])
    print(f"[model] {name} {case}: fp32 condensation moves the optimum by {dist.max():.1e} (bar {REF_COND:.0e})")
    assert dist.max() <= REF_COND, (name, case, dist.max())
