"""The per-instance mix of tests/test_instance_params_ref.py and tests/test_gpu_instance_params.py (a
helper module, no tests in it).

Four combos of a robot model (tests/model_ref.py), a friction coefficient and a force limit:

    0  default     mu 0.4  f_max 120     2  "payload"   mu 0.2  f_max 120
    1  "heavy"     mu 0.6  f_max 150     3  "massonly"  mu 0.8  f_max  60   (18 kg on 60 N feet: the
                                                                             limit binds in trot)

Instance i of a batch takes combo (i + s) % 4 for a rotation s, so over s = 0..3 every instance of
every kernel family meets every combo. The records are those of param_sets.CASES.

CPU data of a (case, rotation) is computed once per process and returned read-only.
"""
import functools

import numpy as np

import model_ref as mr
import param_sets as ps

# combo -> (model name, mu, f_max)
COMBOS = [("default", 0.4, 120.0), ("heavy", 0.6, 150.0), ("payload", 0.2, 120.0), ("massonly", 0.8, 60.0)]


def combo_ids(B, s):
    """Combo of each of B instances under rotation s."""
    return (np.arange(B) + s) % len(COMBOS)


def combo_model(k):
    return mr.model(COMBOS[k][0])


def combo_params(k, N):
    """cmpc_params of horizon N with the combo's mu and f_max (everything else the default)."""
    return mr._cm().make_params(N, mu=COMBOS[k][1], f_max=COMBOS[k][2])


def combo_rows(ids):
    """The [B, 6] float64 table whose row i is combo ids[i] (make_instance_params' layout)."""
    cm = mr._cm()
    mass = np.array([mr.mass_inertia(combo_model(k))[0] for k in range(len(COMBOS))])
    inertia = np.array([mr.mass_inertia(combo_model(k))[1] for k in range(len(COMBOS))])
    mu = np.array([c[1] for c in COMBOS])
    f_max = np.array([c[2] for c in COMBOS])
    ids = np.asarray(ids)
    return cm.make_instance_params(mass[ids], inertia[ids], mu[ids], f_max[ids])


def table(B, s):
    """The rotated mix for a batch of B."""
    return combo_rows(combo_ids(B, s))


def fp64_rows(recs, N, ids, dtype=np.float64):
    """model_ref.fp64_solve of every record under its own combo -> (x64 [B, 12N], qpOASES returns [B])."""
    from concurrent.futures import ThreadPoolExecutor
    prms = [combo_params(k, N) for k in range(len(COMBOS))]
    mdls = [combo_model(k) for k in range(len(COMBOS))]
    with ThreadPoolExecutor(8) as ex:
        out = list(ex.map(lambda a: mr.fp64_solve(a[0], prms[a[1]], mdls[a[1]], dtype), zip(recs, ids)))
    return np.array([x for x, _ in out]), np.array([ri for _, ri in out])


@functools.lru_cache(maxsize=None)
def cpu_data(case, s=0):
    """-> dict(N, recs, ids, x64, ri64) of a case under rotation s: the fp64 optimum of every
    instance with its own row's model, mu and f_max."""
    N = ps.CASES[case][0]
    recs = ps.case_records("default", case)
    ids = combo_ids(len(recs), s)
    x64, ri64 = fp64_rows(recs, N, ids)
    for a in (recs, ids, x64, ri64):
        a.setflags(write=False)
    return dict(N=N, recs=recs, ids=ids, x64=x64, ri64=ri64)
