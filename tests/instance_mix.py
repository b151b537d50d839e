"""The per-instance mix of tests/test_instance_params_ref.py and tests/test_gpu_instance_params.py (a
helper module, no tests in it).

Four combos of a robot model (tests/model_ref.py), a friction coefficient and a force limit:

    0  default     mu 0.4  f_max 120     2  "payload"   mu 0.2  f_max 120
    1  "heavy"     mu 0.6  f_max 150     3  "massonly"  mu 0.8  f_max  60   (18 kg on 60 N feet: the
                                                                             limit binds in trot)

Instance i of a batch takes combo (i + s) % 4 for a rotation s, so over s = 0..3 every instance of
every kernel family meets every combo. The records are those of param_sets.CASES. The float64
optimum of every row under this mix is cost_mix.cpu_data(case, s, mix="model"): tests/cost_mix.py
knows both tables and holds everything that needs both.
"""
import numpy as np

import model_ref as mr
from support import package

# combo -> (model name, mu, f_max)
COMBOS = [("default", 0.4, 120.0), ("heavy", 0.6, 150.0), ("payload", 0.2, 120.0), ("massonly", 0.8, 60.0)]
NC = len(COMBOS)


def combo_ids(B, s):
    """Combo (of this mix or of cost_mix: both have NC) of each of B instances under rotation s."""
    return (np.arange(B) + s) % NC


def combo_model(k):
    return mr.model(COMBOS[k][0])


def combo_params(k, N):
    """cmpc_params of horizon N with the combo's mu and f_max (everything else the default)."""
    return package().make_params(N, mu=COMBOS[k][1], f_max=COMBOS[k][2])


def combo_rows(ids):
    """The [B, 6] float64 table whose row i is combo ids[i] (make_instance_params' layout)."""
    cm = package()
    mass = np.array([mr.mass_inertia(combo_model(k))[0] for k in range(len(COMBOS))])
    inertia = np.array([mr.mass_inertia(combo_model(k))[1] for k in range(len(COMBOS))])
    mu = np.array([c[1] for c in COMBOS])
    f_max = np.array([c[2] for c in COMBOS])
    ids = np.asarray(ids)
    return cm.make_instance_params(mass[ids], inertia[ids], mu[ids], f_max[ids])


def table(B, s):
    """The rotated mix for a batch of B."""
    return combo_rows(combo_ids(B, s))

