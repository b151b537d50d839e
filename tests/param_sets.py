"""Non-default parameter sets and the small batches that reach every kernel family, shared by
tests/test_gpu_params.py and tests/test_gpu_evaluate.py (a helper module, no tests in it).

Every existing fixture and seeded batch was made with make_params(N): dt 0.026, mu 0.4, f_max 120,
alpha 4e-5 and DEFAULT_WEIGHTS, whose pairs (0,1), (2,3), (6,7), (9,10) are equal and whose omega_x /
omega_y weights are zero. W1 has twelve distinct non-zero weights; the other sets move one scalar
each, and "all" moves everything at once.

CPU data of a (set, case) is computed once per process (inputs, the restated reference pipeline in
its default summation order, the float64 optimum of every instance) and returned read-only.
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from support import package, reduced_sizes

W1 = (0.4, 0.25, 8, 10, 2, 50, 0.03, 0.01, 0.3, 0.2, 0.32, 0.1)

SETS = {
    "default": {},
    "W1": dict(weights=W1),
    "mu0.2": dict(mu=0.2),
    "mu0.8": dict(mu=0.8),
    "fmax30": dict(f_max=30.0),
    "alpha4e-4": dict(alpha=4e-4),
    "alpha1e-5": dict(alpha=1e-5),
    "dt0.013": dict(dt=0.013),
    "dt0.04": dict(dt=0.04),
    "all": dict(mu=0.6, f_max=80.0, alpha=1e-4, dt=0.02, weights=W1),
}
NON_DEFAULT = [s for s in SETS if s != "default"]

# name -> (N, batch, make_instances keywords, reduced sizes n the batch must have (lo, hi) or None)
CASES = {
    "n10_families": (10, 128, dict(seed=9330, random_contact_frac=1.0), None),
    "n3_padding": (3, 32, dict(seed=9303, random_contact_frac=1.0), (0, 36)),
    "n12_standing": (12, 8, dict(seed=9312, random_contact_frac=0.0, gait="standing"), (144, 144)),
    "n16_trot": (16, 16, dict(seed=9316, random_contact_frac=0.0), (81, 96)),
    "n16_walking": (16, 4, dict(seed=9316, random_contact_frac=0.0, gait="walking"), (129, 144)),
    "n16_standing": (16, 4, dict(seed=9316, random_contact_frac=0.0, gait="standing"), (192, 192)),
    "n20_trot": (20, 8, dict(seed=9320, random_contact_frac=0.0), (97, 120)),
    "n20_standing": (20, 4, dict(seed=9320, random_contact_frac=0.0, gait="standing"), (240, 240)),
}

# reduced sizes n of the kernel families at N <= 10: class 1's 60- and 64-wide builds, the tail
# class, wide 80 / 96 / 120
FAMILY_EDGES = [0, 60, 64, 72, 80, 96, 120]


def set_params(name, N, **over):
    """make_params(N) with the named set's values (``over``: further keywords on top)."""
    return package().make_params(N, **{**SETS[name], **over})


def case_records(set_name, case):
    """The case's records, their trajectories built with the set's dt."""
    cm = package()
    N, B, kw, span = CASES[case]
    recs = cm.make_instances(B, N, dt=SETS[set_name].get("dt", 0.026), **kw)
    n = reduced_sizes(recs, N)
    if span is not None:
        assert n.min() >= span[0] and n.max() <= span[1], (case, int(n.min()), int(n.max()))
    return recs


def family_counts(recs, N=10):
    n = reduced_sizes(recs, N)
    return [int(((n > lo) & (n <= hi)).sum()) for lo, hi in zip(FAMILY_EDGES[:-1], FAMILY_EDGES[1:])]


def fp64_batch(orc, recs, prm):
    """oracle.fp64_solve of every record -> (x64 [B, 12N], qpOASES return values [B])."""
    with ThreadPoolExecutor(8) as ex:   # (numpy / scipy / the qpOASES call release the GIL)
        out = list(ex.map(lambda r: orc.fp64_solve(r, prm), recs))
    return np.array([x for x, _ in out]), np.array([ri for _, ri in out])


def rel_dist(f, x64):
    """|f - x64|_inf / max(|x64|_inf, 1) per instance (conftest.rel_force_err's norm)."""
    f = np.asarray(f, np.float64).reshape(x64.shape)
    return np.abs(f - x64).max(axis=1) / np.maximum(np.abs(x64).max(axis=1), 1.0)


@functools.lru_cache(maxsize=None)
def cpu_data(set_name, case):
    """-> dict(prm, recs, q (reference pipeline, default order), st_ref, x64, ri64, ref64: the
    reference's distance from the fp64 optimum per instance, inf where its qpOASES fails)."""
    from oracle import oracle as orc
    N = CASES[case][0]
    prm = set_params(set_name, N)
    recs = case_records(set_name, case)
    q, st_ref, _ = orc.ref_solve_batch(recs, prm, nthreads=16)
    x64, ri64 = fp64_batch(orc, recs, prm)
    ref64 = np.where(st_ref == 0, rel_dist(q, x64), np.inf)
    for a in (recs, q, st_ref, x64, ri64, ref64):
        a.setflags(write=False)
    return dict(prm=prm, recs=recs, q=q, st_ref=st_ref, x64=x64, ri64=ri64, ref64=ref64)
