"""The yardstick of the per-instance cost table (tests/cost_mix.py), on the CPU.

tests/test_gpu_instance_costs.py holds a solve under a mixed cost table to model_ref.fp64_solve with
each row's own weights and alpha. Here, over every case of param_sets.CASES:

 1. qpOASES returns 0 on every instance of the mix at rotation 0 and under the neighbour's combo;
 2. condensing in fp32 alone (the discretised matrices rounded to fp32, the products in fp32) moves the
    optimum of every instance of the fp32 horizons' cases by at most REF_COND = 5e-5, half the N <= 10
    gate, with the cost table alone and with both tables (measured when the mix was chosen: 3.05e-5
    at n10_families, 2.6e-6 at n3_padding; 4.2e-5 and 2.9e-6 with both tables);
 3. giving an instance its neighbour's cost combo moves its fp64 optimum by more than 10 x the
    horizon's gate on every instance (measured minimum 3.0e-2, at n20_trot);
 4. alpha alone (combo 0 against combo 2: the same weights) moves it by more than that bar too
    (measured minimum 1.2e-1): a kernel that reads the wrong row, a shared weight or the shared alpha
    cannot pass.

Also: make_instance_costs' layout and broadcasting. Skipped without oracle/_ref (qpOASES), as the
other tests of the float64 optimum are.
"""
import numpy as np
import pytest

import cost_mix as cx
import param_sets as ps
from support import FP64_TOL, REF_COND, REF_TOL, needs_ref  # noqa: F401


def test_make_instance_costs_layout(cm):
    t = cm.make_instance_costs()
    assert t.shape == (1, 16) and t.dtype == np.float32
    np.testing.assert_array_equal(t[0, :12], np.array(cm.DEFAULT_WEIGHTS, np.float32))
    assert t[0, 12] == np.float32(4e-5) and (t[0, 13:] == 0).all()
    assert (cm.COST_WEIGHTS, cm.COST_ALPHA, cm.COST_WORDS) == (0, 12, 16)
    t = cm.make_instance_costs(alpha=[4e-5, 1e-5, 1e-4])
    assert t.shape == (3, 16)
    np.testing.assert_array_equal(t[:, cm.COST_ALPHA], np.array([4e-5, 1e-5, 1e-4], np.float32))
    np.testing.assert_array_equal(t[:, :12], np.tile(np.array(cm.DEFAULT_WEIGHTS, np.float32), (3, 1)))
    t = cm.make_instance_costs(weights=[ps.W1, cx.W2], alpha=2e-5)
    assert t.shape == (2, 16)
    np.testing.assert_array_equal(t[1, :12], np.array(cx.W2, np.float32))
    np.testing.assert_array_equal(t[:, 12], np.float32([2e-5, 2e-5]))
    t = cm.make_instance_costs(weights=ps.W1, alpha=[1e-5, 1e-4])
    np.testing.assert_array_equal(t[:, :12], np.tile(np.array(ps.W1, np.float32), (2, 1)))
    with pytest.raises(ValueError):
        cm.make_instance_costs(weights=[1.0, 2.0])
    with pytest.raises(ValueError):
        cm.make_instance_costs(weights=[ps.W1, cx.W2], alpha=[1e-5, 2e-5, 3e-5])
    with pytest.raises(ValueError):
        cm.make_instance_costs(alpha=[[1e-5]])
    # the mix's own table
    t = cx.table(6, 1)
    np.testing.assert_array_equal(t[0, :13], np.float32(list(ps.W1) + [4e-5]))
    np.testing.assert_array_equal(t[2, :13], np.float32(list(cx.W2) + [1e-4]))
    np.testing.assert_array_equal(t[3, :13], np.float32(list(cm.DEFAULT_WEIGHTS) + [4e-5]))
    np.testing.assert_array_equal(t[4], t[0])


@pytest.mark.parametrize("case", list(ps.CASES))
def test_mix_is_solvable_and_rows_are_told_apart(needs_ref, case):
    d = cx.cpu_data(case, 0)
    N, recs, ids, x64 = d["N"], d["recs"], d["ids"], d["x64"]
    assert (d["ri64"] == 0).all(), d["ri64"]
    xn, rin = cx.fp64_rows(recs, N, (ids + 1) % cx.NC)   # the neighbour's combo
    assert (rin == 0).all(), rin
    move = ps.rel_dist(xn, x64)
    bar = 10 * (REF_TOL if N <= 10 else FP64_TOL)
    print(f"[cost] {case}: the neighbour's combo moves the fp64 optimum by {move.min():.1e} (min), "
          f"{np.median(move):.2f} (median) over {len(move)} instances; bar {bar:.0e}")
    assert move.min() > bar, (case, int(move.argmin()), float(move.min()))


@pytest.mark.parametrize("case", list(ps.CASES))
def test_alpha_alone_is_told_apart(needs_ref, case):
    N = ps.CASES[case][0]
    recs = ps.case_records("default", case)
    x0, r0 = cx.fp64_rows(recs, N, np.zeros(len(recs), int))
    x2, r2 = cx.fp64_rows(recs, N, np.full(len(recs), 2))
    assert (r0 == 0).all() and (r2 == 0).all()
    move = ps.rel_dist(x2, x0)
    bar = 10 * (REF_TOL if N <= 10 else FP64_TOL)
    print(f"[cost] {case}: alpha 1e-5 against 4e-5 moves the fp64 optimum by {move.min():.1e} (min); bar {bar:.0e}")
    assert move.min() > bar, (case, int(move.argmin()), float(move.min()))


@pytest.mark.parametrize("case", ["n10_families", "n3_padding"])
def test_mix_fp32_condensation_condition(needs_ref, case):
    d = cx.cpu_data(case, 0)
    x32, ri = cx.fp64_rows(d["recs"], d["N"], d["ids"], dtype=np.float32)
    assert (ri == 0).all(), ri
    dist = ps.rel_dist(x32, d["x64"])
    per = [float(dist[d["ids"] == k].max()) for k in range(cx.NC)]
    print(f"[cost] {case}: fp32 condensation moves the optimum by {dist.max():.2e} "
          f"(per combo {', '.join(f'{v:.1e}' for v in per)}; bar {REF_COND:.0e})")
    assert dist.max() <= REF_COND, (case, float(dist.max()))


@pytest.mark.parametrize("case", ["n10_families", "n3_padding"])
def test_pairs_fp32_condensation_condition(needs_ref, case):
    d = cx.cpu_data_pairs(case)
    assert (d["ri64"] == 0).all(), d["ri64"]
    x32, ri = cx.fp64_rows(d["recs"], d["N"], d["cids"], d["mids"], dtype=np.float32)
    assert (ri == 0).all(), ri
    dist = ps.rel_dist(x32, d["x64"])
    print(f"[cost] {case}, both tables: fp32 condensation moves the optimum by {dist.max():.2e} (bar {REF_COND:.0e})")
    assert dist.max() <= REF_COND, (case, float(dist.max()))
