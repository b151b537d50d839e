// cmpc_condense_inst.hip — the condensation hook for a handle with a per-instance table
// (cmpc_batch_set_instance_params): cmpc_condense_inst_kernel and launch_condense_inst, the
// per-instance build of cmpc_condense.hip in a unit of its own.
#define CMPC_CONDENSE_INST 1
#include "cmpc_condense.hip"
