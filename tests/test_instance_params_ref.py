"""The yardstick of the per-instance table (tests/instance_mix.py), on the CPU.

tests/test_gpu_instance_params.py holds a solve under a mixed table to model_ref.fp64_solve with each
row's own model, mu and f_max. Here, at rotation 0 and over every case of param_sets.CASES:

 1. qpOASES returns 0 on every instance of the mix;
 2. condensing in fp32 alone (the discretised matrices rounded to fp32, the products in fp32) moves the
    optimum of every instance of the fp32 horizons' cases by at most REF_COND = 5e-5, half the N <= 10
    gate, so a miss of that gate cannot be the precision of the condensation (measured when the mix was
    chosen: 2.13e-5 at n10_families, 1.3e-6 at n3_padding);
 3. giving an instance its neighbour's combo moves its fp64 optimum by more than 10 x the horizon's
    gate on every instance (measured minimum 9.8e-2, medians 0.38-0.56): a kernel that reads the wrong
    row, or a shared value, cannot pass.

Also: make_instance_params' layout and broadcasting. Skipped without oracle/_ref (qpOASES), as the
other tests of the float64 optimum are.
"""
import numpy as np
import pytest

import cost_mix as cx
import instance_mix as im
import param_sets as ps
from support import FP64_TOL, REF_COND, REF_TOL, needs_ref  # noqa: F401


def test_make_instance_params_layout(cm):
    t = cm.make_instance_params()
    assert t.shape == (1, 6) and t.dtype == np.float64
    np.testing.assert_array_equal(t[0], [12.0, 0.07, 0.26, 0.242, 0.4, 120.0])
    t = cm.make_instance_params(mass=[12.0, 20.0, 17.0], mu=0.6)
    assert t.shape == (3, 6)
    np.testing.assert_array_equal(t[:, cm.INST_MASS], [12.0, 20.0, 17.0])
    np.testing.assert_array_equal(t[:, cm.INST_MU], [0.6] * 3)
    np.testing.assert_array_equal(t[:, cm.INST_INERTIA:cm.INST_INERTIA + 3], [[0.07, 0.26, 0.242]] * 3)
    t = cm.make_instance_params(inertia=[[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]], f_max=[60.0, 150.0])
    np.testing.assert_array_equal(t[1], [12.0, 0.4, 0.5, 0.6, 0.4, 150.0])
    assert (cm.INST_MASS, cm.INST_INERTIA, cm.INST_MU, cm.INST_FMAX, cm.INST_WORDS) == (0, 1, 4, 5, 6)
    with pytest.raises(ValueError):
        cm.make_instance_params(inertia=[0.1, 0.2])
    with pytest.raises(ValueError):
        cm.make_instance_params(mass=[1.0, 2.0], mu=[0.4, 0.5, 0.6])
    # the mix's own table
    t = im.table(6, 1)
    np.testing.assert_array_equal(t[0], [20.0, 0.15, 0.60, 0.55, 0.6, 150.0])
    np.testing.assert_array_equal(t[3], [12.0, 0.07, 0.26, 0.242, 0.4, 120.0])
    np.testing.assert_array_equal(t[4], t[0])


@pytest.mark.parametrize("case", list(ps.CASES))
def test_mix_is_solvable_and_rows_are_told_apart(needs_ref, case):
    d = cx.cpu_data(case, 0, mix="model")
    N, recs, ids, x64 = d["N"], d["recs"], d["ids"], d["x64"]
    assert (d["ri64"] == 0).all(), d["ri64"]
    # the neighbour's combo
    xn, rin = cx.fp64_rows(recs, N, model_ids=(ids + 1) % len(im.COMBOS))
    assert (rin == 0).all(), rin
    move = ps.rel_dist(xn, x64)
    bar = 10 * (REF_TOL if N <= 10 else FP64_TOL)
    print(f"[inst] {case}: the neighbour's combo moves the fp64 optimum by {move.min():.1e} (min), "
          f"{np.median(move):.2f} (median) over {len(move)} instances; bar {bar:.0e}")
    assert move.min() > bar, (case, int(move.argmin()), float(move.min()))


@pytest.mark.parametrize("case", ["n10_families", "n3_padding"])
def test_mix_fp32_condensation_condition(needs_ref, case):
    d = cx.cpu_data(case, 0, mix="model")
    x32, ri = cx.fp64_rows(d["recs"], d["N"], model_ids=d["ids"], dtype=np.float32)
    assert (ri == 0).all(), ri
    dist = ps.rel_dist(x32, d["x64"])
    per = [float(dist[d["ids"] == k].max()) for k in range(len(im.COMBOS))]
    print(f"[inst] {case}: fp32 condensation moves the optimum by {dist.max():.2e} "
          f"(per combo {', '.join(f'{v:.1e}' for v in per)}; bar {REF_COND:.0e})")
    assert dist.max() <= REF_COND, (case, float(dist.max()))
