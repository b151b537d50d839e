"""MI355X-native batched convex-MPC solver (drop-in for SolverMPC's C interface)."""
from .records import (CmpcModel, make_model, CmpcParams, make_params, pack_records, record_words, unpack_gait,  # noqa: F401
                      DEFAULT_WEIGHTS, STATUS_NAMES, CERT_COST, CERT_COST0, CERT_GAP, CERT_VIOL,
                      CERT_SWING, CERT_GRADMAX, CERT_WORDS, SENS_X0, SENS_WEIGHTS, SENS_ALPHA, SENS_FEST3,
                      SENS_FREE, SENS_SLACK, SENS_WORDS, GAIN_K, GAIN_FREE, GAIN_FREE0, GAIN_SLACK, GAIN_WORDS,
                      make_instance_params, INST_MASS, INST_INERTIA,
                      INST_MU, INST_FMAX, INST_WORDS, make_instance_costs, COST_WEIGHTS, COST_ALPHA, COST_WORDS)
from .instances import make_disturbance, make_instances, make_logs, trot_table  # noqa: F401
