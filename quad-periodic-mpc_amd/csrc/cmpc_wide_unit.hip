// cmpc_wide_unit.hip — one build of the wide kernel template (cmpc_wide.h) per translation unit:
// build.py compiles this file once per row of kWideBuild (cmpc_wide_builds.h), the row given as
// -DCMPC_UNIT_WIDE=NV,PERSIST,REFINE,LIT. (Compiled side by side, the kernels spilled registers.)
#include "cmpc_wide.h"

#ifndef CMPC_UNIT_WIDE
#error "CMPC_UNIT_WIDE=NV,PERSIST,REFINE,LIT: the row of kWideBuild this unit builds"
#endif

namespace cmpc {
template hipError_t launch_wide_build<CMPC_UNIT_WIDE>(const KParams&, const WideCall&);
}  // namespace cmpc
