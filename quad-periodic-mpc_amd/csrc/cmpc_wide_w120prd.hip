// cmpc_wide_w120prd.hip — the default robot's build (the model as literals, CMPC_WIDE_LITERAL) of the
// persistent launch form of the 120-column wide class with the fp64
// refinement step (cmpc_wide.h wide_refine; horizons N > 10).
#define CMPC_WIDE_WAVES_PER_EU 4
#define CMPC_WIDE_BUILD 2
#define CMPC_WIDE_REFINE 1
#define CMPC_WIDE_LITERAL 1
#include "cmpc_wide.h"

namespace cmpc {

hipError_t launch_wide_w120_persist_r_lit(const float* d_recs, const KParams& P, float* d_forces,
                                    uint8_t* d_status, int32_t* d_iters, const int* in_list,
                                    const int* in_count, int* deq, int grid, hipStream_t stream, int base) {
  return launch_wide_impl<120>(d_recs, P, d_forces, d_status, d_iters, in_list, in_count, deq, grid, stream, base);
}

}  // namespace cmpc
