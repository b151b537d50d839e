"""The paths of one active-set trip, held to the live reference (tests/test_gpu_parity.py's rule).

The Goldfarb-Idnani loop forms the reflection's tw = J_v . w from the trip's z and one column of J,
and takes |d2|^2 by a lane reduction. A batch exercises every path of a trip only if it holds
instances that take no trip at all, instances that stop right after an add, and instances that
drop a constraint; at N = 10 also a class-1 instance whose active set grows past QI positions, so
that r = R^-1 d1 runs both as the matvec over the kept inverse and as the back substitution. The
test asserts those conditions per kernel family before it compares forces, so a change of the
instance generator that empties one of them fails here instead of passing vacuously.

What can be read from the outputs (forces, status, iters), per instance:
  * trips = iters. Every trip is an add or a drop, and the positions at the end are adds - drops, so
    drops = (iters - positions) / 2. The positions are at most the constraints whose slack at the
    returned forces is within support.ACT_HI of zero (a loose count that can only be too large), hence
    iters > that count proves a drop.
  * a solved instance with iters >= 1 ended right after an add (the loop leaves only from the
    selection, which follows an add).
  * the positions are at least the constraints whose slack is within support.ACT_LO of zero: an active
    constraint sits on its plane up to fp32 rounding, and the solver itself only adds a constraint
    violated by more than 1e-5 max(1, |x|_max), so twice that counts none that was merely close
    except in a band of 3e-5 max(1, |x|_max) above zero.

Families by the reduced size n = 3 x stance foot-steps: class 1 (n <= 64: the 60- and 64-wide
builds), the tail class (n 65..72; an instance it hands on after 64 active positions is left out of
its counts), the wide classes (n > 72; at N = 12 their refining builds).
"""
import numpy as np
import pytest

from support import active_counts, gpu_solve, solver_mod  # noqa: F401
from test_gpu_parity import assert_failed_reference, assert_parity

pytestmark = pytest.mark.gpu

QI = {60: 42, 64: 45}   # positions up to which class 1 keeps R^-1 (SharedC1<NV>::QI)

# (N, stress, batch, seed, size bins (lo, hi] that must be populated, class-1 instance past QI):
# N = 10 with every contact random covers class 1 at 60 and 64 wide, the tail class and the 80 / 96 /
# 120 classes; N = 12 the refining wide builds. Seeds from a search over 7300..7315 per batch:
#   * n > 96 at N = 10 needs 33 of 40 Bernoulli(0.5) contacts: only seed 7300 has such an instance
#     (one), and without stress its wide instances drop nothing, so the unstressed batch takes a
#     seed whose three families all drop (7304: 4 / 3 / 1 instances) and leaves the 120 class to
#     the stressed one;
#   * without stress no class-1 active set comes near QI (at most 36 positions over the 16 seeds),
#     so that condition is the stressed batch's.
C1_BINS = ((0, 60), (60, 64))
N10_BINS = C1_BINS + ((64, 72), (72, 80), (80, 96))
BATCHES = [(10, False, 2048, 7304, N10_BINS, False),
           (10, True, 2048, 7300, N10_BINS + ((96, 120),), True),
           (12, False, 1024, 7300, ((72, 80), (80, 96), (96, 120)), False)]


def family_masks(n, hi):
    return {"class 1": n <= 64,
            "tail": (n > 64) & (n <= 72) & (hi < 64),
            "wide": n > 72}


def path_counts(n, hi, lo, st, it):
    """{family: (instances, zero trips, stopped after an add, with a drop)} and the class-1
    instances whose active set passed QI."""
    out = {}
    ok = st == 0
    for name, m in family_masks(n, hi).items():
        m = m & ok
        out[name] = (int(m.sum()), int((m & (it == 0)).sum()), int((m & (it >= 1)).sum()),
                     int((m & (it > hi)).sum()))
    past = ok & (((n <= 60) & (lo > QI[60])) | ((n > 60) & (n <= 64) & (lo > QI[64])))
    return out, int(past.sum())


@pytest.mark.parametrize("N,stress,B,seed,bins,past", BATCHES, ids=["n10", "n10-stress", "n12"])
def test_active_set_paths_match_reference_live(cm, orc, solver_mod, N, stress, B, seed, bins, past):
    prm = cm.make_params(N)
    recs = cm.make_instances(B, N, seed=seed, stress=stress, random_contact_frac=1.0)
    f, st, it = gpu_solve(solver_mod, prm, recs)
    n, hi, lo = active_counts(cm, prm, recs, f)
    counts, past_qi = path_counts(n, hi, lo, st, it)
    for name, c in counts.items():
        print(f"[paths] N={N} stress={stress} {name}: {c[0]} solved, {c[1]} with no trip, {c[2]} "
              f"stopped after an add, {c[3]} with a drop")
    print(f"[paths] N={N} stress={stress}: {past_qi} class-1 instances past QI; trips mean "
          f"{it.mean():.2f} max {it.max()}")
    families = ("wide",) if N >= 11 else ("class 1", "tail", "wide")
    for name in families:
        inst, zero, after_add, drop = counts[name]
        assert zero >= 1, (name, "no instance without a trip")
        assert after_add >= 1, (name, "no instance that stops after an add")
        assert drop >= 1, (name, "no instance with a drop")
    if past:
        assert past_qi >= 1, "no class-1 instance whose active set passes QI"
    for lo_n, hi_n in bins:
        assert ((n > lo_n) & (n <= hi_n)).any(), ("no instance with n in", lo_n, hi_n)
    if not orc.ref_available():
        pytest.skip("oracle/_ref not present")
    q, st_ref, _ = orc.ref_solve_batch(recs, prm, nthreads=16)
    ok = st_ref == 0
    assert (st[ok] == 0).all(), np.bincount(st[ok])
    label = f"paths stress={stress} frac=1.0"
    assert_parity(orc, recs, prm, f, q, ok, label=label)
    assert_failed_reference(orc, recs, prm, f, st, st_ref, label=f"paths N={N}")
