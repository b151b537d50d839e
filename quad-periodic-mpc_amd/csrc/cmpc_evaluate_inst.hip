// cmpc_evaluate_inst.hip — cmpc_batch_evaluate for a handle with a per-instance table
// (cmpc_batch_set_instance_params): cmpc_evaluate_inst_kernel and launch_evaluate_inst, the
// per-instance build of cmpc_evaluate.hip in a unit of its own.
#define CMPC_EVALUATE_INST 1
#include "cmpc_evaluate.hip"
