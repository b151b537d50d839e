"""The per-instance cost mix of tests/test_instance_costs_ref.py and tests/test_gpu_instance_costs.py, and
what needs both this table and tests/instance_mix.py's: the 16 pairs and the float64 optimum of every
row of either mix (a helper module, no tests in it).

Four combos of state weights and force regularisation alpha:

    0  default weights  alpha 4e-5        2  default weights  alpha 1e-5  (the reference's own fallback)
    1  param_sets.W1    alpha 4e-5        3  W2 (below)       alpha 1e-4

Instance i of a batch takes combo (i + s) % 4 for a rotation s, so over s = 0..3 every instance of
every kernel family meets every combo. The records are those of param_sets.CASES. For the tests with
both tables set, instance i takes model / mu / f_max combo i % 4 of instance_mix and cost combo
(i // 4) % 4: the 16 pairs.

CPU data of a (case, rotation, mix) is computed once per process and returned read-only.
"""
import functools

import numpy as np

import instance_mix as im
import model_ref as mr
import param_sets as ps
from instance_mix import NC, combo_ids  # noqa: F401  (cx.combo_ids, cx.NC: the same rotation over as many combos)
from support import package

W2 = (1.0, 0.6, 12, 20, 14, 40, 0.05, 0.02, 0.4, 0.5, 0.35, 0.15)

# combo -> (weights or None for the default, alpha)
COMBOS = [(None, 4e-5), (ps.W1, 4e-5), (None, 1e-5), (W2, 1e-4)]
assert len(COMBOS) == NC


def combo_weights(k):
    w = COMBOS[k][0]
    return tuple(package().DEFAULT_WEIGHTS) if w is None else tuple(w)


def combo_kw(k):
    """make_params keywords of cost combo k."""
    return dict(weights=combo_weights(k), alpha=COMBOS[k][1])


def combo_params(k, N, **over):
    """cmpc_params of horizon N with the combo's weights and alpha (everything else the default, or ``over``)."""
    return package().make_params(N, **{**combo_kw(k), **over})


def combo_model(k):
    """Every cost combo runs the default robot."""
    return None


def combo_rows(ids):
    """The [B, 16] float32 table whose row i is cost combo ids[i] (make_instance_costs' layout)."""
    w = np.array([combo_weights(k) for k in range(NC)], np.float32)
    a = np.array([c[1] for c in COMBOS], np.float32)
    ids = np.asarray(ids)
    return package().make_instance_costs(w[ids], a[ids])


def table(B, s):
    """The rotated mix for a batch of B."""
    return combo_rows(combo_ids(B, s))


# ---- both tables: model / mu / f_max combo i % 4 of instance_mix, cost combo (i // 4) % 4 -------------
def pair_ids(B):
    i = np.arange(B)
    return i % im.NC, (i // 4) % NC


def pair_params(km, kc, N):
    """cmpc_params of the shared handle of the pair (instance_mix combo km, cost combo kc)."""
    return combo_params(kc, N, mu=im.COMBOS[km][1], f_max=im.COMBOS[km][2])


def fp64_rows(recs, N, cost_ids=None, model_ids=None, dtype=np.float64):
    """model_ref.fp64_solve of every record under its own cost combo and its own instance_mix combo
    (None: combo 0, the defaults, for every record) -> (x64 [B, 12N], qpOASES returns [B])."""
    from concurrent.futures import ThreadPoolExecutor
    cost_ids = np.zeros(len(recs), int) if cost_ids is None else cost_ids
    model_ids = np.zeros(len(recs), int) if model_ids is None else model_ids
    prms = {(km, kc): pair_params(km, kc, N) for km in set(map(int, model_ids)) for kc in set(map(int, cost_ids))}
    mdls = [im.combo_model(k) for k in range(im.NC)]
    with ThreadPoolExecutor(8) as ex:
        out = list(ex.map(lambda a: mr.fp64_solve(a[0], prms[(int(a[1]), int(a[2]))], mdls[int(a[1])], dtype),
                          zip(recs, model_ids, cost_ids)))
    return np.array([x for x, _ in out]), np.array([ri for _, ri in out])


def _cpu_data(case, cost_ids=None, model_ids=None, **ids):
    """-> the read-only dict(N, recs, **ids, x64, ri64) of a case: the fp64 optimum of every instance
    under its own row of either table."""
    N = ps.CASES[case][0]
    recs = ps.case_records("default", case)
    x64, ri64 = fp64_rows(recs, N, cost_ids, model_ids)
    for a in (recs, x64, ri64, *ids.values()):
        a.setflags(write=False)
    return dict(N=N, recs=recs, **ids, x64=x64, ri64=ri64)


@functools.lru_cache(maxsize=None)
def cpu_data(case, s=0, mix="cost"):
    """-> dict(N, recs, ids, x64, ri64) of a case under rotation s of one mix, the other table absent:
    "cost", each row's own weights and alpha; "model", its own instance_mix model, mu and f_max."""
    ids = combo_ids(ps.CASES[case][1], s)
    return _cpu_data(case, ids=ids, **{f"{mix}_ids": ids})


@functools.lru_cache(maxsize=None)
def cpu_data_pairs(case):
    """-> dict(N, recs, mids, cids, x64, ri64) of a case with both tables: the fp64 optimum of every
    instance under its own (model, mu, f_max, cost) pair."""
    mids, cids = pair_ids(ps.CASES[case][1])
    return _cpu_data(case, cids, mids, mids=mids, cids=cids)
