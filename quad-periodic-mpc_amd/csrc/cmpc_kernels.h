// cmpc_kernels.h — internal interface between the HIP kernels and the C-ABI host layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/cmpc_solver.h"
#include "cmpc_plan.h"

namespace cmpc {

// Launch-placement knobs of the A/B experiments (PlanKnobs, cmpc_plan.h, holds the
// ones of launch_solve): read from the environment only
// in a diagnostic build (-DCMPC_DIAG_KNOBS=1, scripts/build_diag_variant.sh); the product build
// always runs the measured defaults.
inline int diag_knob(const char* name, int dflt) {
#if defined(CMPC_DIAG_KNOBS) && CMPC_DIAG_KNOBS
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
#else
  (void)name;
  return dflt;
#endif
}

// Kernel-side form of cmpc_model: the values the kernels use, derived on the host once
// (make_kmodel, cmpc_abi.cpp). The fp32 kernels take (float) of each field, the fp64 refinement
// the reciprocals of the doubles themselves: the mix of literals the code had when the model was
// m = 12, I_body = diag(.07, .26, .242) (RobotState.h:25-26), so that model gives the same bits.
struct KModel {
  float ib[3];       // (float) inertia[i]
  float im;          // 1.f / (float) mass
  double iinv64[3];  // 1.0 / inertia[i]
  double im64;       // 1.0 / mass
};

// One entry of a handle's per-instance table: what instance i uses in place of the handle's model,
// mu and f_max (cmpc_batch_set_instance_params: the first 64-byte line) and in place of its weights
// and alpha (cmpc_batch_set_instance_costs: the second line). KModel first, so the fp32 block
// {ib, im} and the fp64 block {iinv64, im64} sit at the offsets they have in the argument segment's
// KModel and one scalar load each fetches them; neither half straddles a cache line. With only one
// of the two tables set, the other half of every entry holds the handle's shared values
// (launch_inst_fill). (The inertia doubles themselves, which cmpc_batch_evaluate alone needs, are
// read from the handle's snapshot of the rows: launch_evaluate's inst_rows.)
struct KInst {
  KModel mdl;
  float mu_inv;    // 1.f / (float) mu, as KParams::mu_inv
  float f_max;     // (float) f_max
  float pad[2];
  float wts[12];   // as KParams::wts
  float alpha2;    // 2.f * alpha, as KParams::alpha2
  float pad2;
  double alpha64;  // (double) alpha (cmpc_batch_evaluate's fp64 cost; one scalar load, no conversion)
};
static_assert(sizeof(KInst) == 128 && offsetof(KInst, mdl) == 0 && offsetof(KInst, mu_inv) == 48 &&
                  offsetof(KInst, f_max) == 52 && offsetof(KInst, wts) == 64 && offsetof(KInst, alpha2) == 112 &&
                  offsetof(KInst, alpha64) == 120,
              "two 64-byte lines per instance: KModel, 1 / mu, f_max; weights, 2 alpha, (double) alpha");

// Kernel-side copy of cmpc_params (by value, lands in SGPRs).
struct KParams {
  float dt;
  float mu_inv;    // fmat uses 1/mu (SolverMPC.cpp:657)
  float f_max;
  float alpha2;    // 2 * alpha (qH = 2 (B'SB + alpha I))
  float wts[12];
  int N;
  int rec_words;
  int max_iter;    // active-set cap; the kernels allow max_iter + 2 n
  int refine;      // wide classes: one fp64 refinement step of the converged active set (N > 10)
  int out_cols;    // forces written per instance: 12 x the leading horizon steps kept
                   // (cmpc_batch_set_output_steps; 12 N by default)
  int mdl_default; // host side only: mdl is the default robot's (the launchers then take the builds
                   // with the model as literals, where there is one)
  // the step's fp64 powers for that refinement (scalar registers, not per-lane conversions)
  double dt64, dth64, dt3_64;  // dt, dt^2 / 2, dt^3 / 6
  KModel mdl;      // the handle's robot model (cmpc_batch_set_model)
  // the per-instance table (cmpc_batch_set_instance_params, _set_instance_costs): entry i replaces
  // mdl, mu_inv, f_max, wts and alpha2 for instance i; null when neither table is set. Last, so no
  // other field's offset depends on it
  const KInst* inst;
};

// Kernel-side copy of cmpc_loco_params + the handle's horizon / record stride.
struct LocoParams {
  float dt;
  int iters_between_mpc;
  float x_drag_gain;
  int horizon;
  int rec_words;
  float hip_x, hip_y, abad_link, swing_height, bonus_swing;  // foot placement (cmpc_loco_params)
  int out_cols;    // rollout: the forces' stride (the handle's KParams::out_cols)
};

// Scratch ints needed by launch_solve for max_batch instances.
// d_work = [2 headers of kHdr ints: cnt[0] instances above class 1's build, cnt[1 + list] list
// lengths, cnt[kDeq + list] the persistent wide workgroups' dequeue counters (the constants and the
// size class of every list: cmpc_plan.h)] [kLists lists of max_batch]. The solves alternate
// over the two headers: each classify pass zeroes the header the next solve uses (the previous
// solve, which used it, has joined by then), so no memset precedes a solve (zeroed at create)
inline size_t work_ints(int max_batch) { return 2 * kHdr + kLists * (size_t)max_batch; }
// Side streams and events of one handle: the wider size classes run concurrently with class 1
// (they are latency-bound: few instances, long serial solves). Three side streams (the third
// carries only the tail class at N <= 10 below 131072 instances): with the handle's own stream
// that is the four hardware queues a process gets by default (GPU_MAX_HW_QUEUES = 4), so no side
// stream shares a queue with class 1. A process with two handles (parallel.RootPipeline's two
// solver lanes) has eight streams over those four queues: the lanes' streams alias in pairs; the
// lanes alternate pieces, so at most one lane's class 1 runs at a time.
constexpr int kSideStreams = 3;
struct LaunchCtx {
  hipStream_t side[kSideStreams] = {nullptr, nullptr, nullptr};
  hipEvent_t fork = nullptr;
  hipEvent_t classified = nullptr;  // the classify pass (on side 0) is done
  hipEvent_t join[kSideStreams] = {nullptr, nullptr, nullptr};
  int hdr = 0;       // header (0 / 1) of d_work the next solve's lists count into
  // class counts of an earlier solve (a header as the classify kernel left it, copied by a later
  // classify pass): host-mapped pinned memory, read by launch_solve to size the wide classes' grids
  int* h_hint = nullptr;
  int* d_hint = nullptr;
  int last_hdr = 0;  // header of the last solve (its cnt[0] for cmpc_batch_read_timing)
};
// ev (optional): 3 events recorded on `stream`: ev[0] before class 1, ev[1] after it, ev[2]
// after the wider classes (side streams) have joined.
// d_due (optional, cmpc_batch_solve_due): batch bytes; only the instances with d_due[i] != 0 are
// classified, listed and solved, class 1 over its list at every horizon. nullptr: the unmasked
// launch sequence.
hipError_t launch_solve(const float* d_recs, int batch, const KParams& P, float* d_forces,
                        uint8_t* d_status, int32_t* d_iters, int* d_work, int max_batch,
                        hipStream_t stream, LaunchCtx& ctx, hipEvent_t* ev = nullptr,
                        const uint8_t* d_due = nullptr);
// per-class launchers (cmpc_class1.hip; the wide classes' below)
hipError_t launch_class1(int nv, const float* d_recs, int batch, const KParams& P, float* d_forces,
                         uint8_t* d_status, int32_t* d_iters, const int* in_list, const int* in_count,
                         int* ovf_list, int* ovf_count, int grid, hipStream_t stream);
// One launch of a wide class (two lanes per row, NV/32 wavefronts) over a classify list.
struct WideCall {
  const float* recs;
  float* forces;
  uint8_t* status;
  int32_t* iters;
  const int* list;   // the class's instance list and its length (on the device)
  const int* count;
  int* deq;          // the persistent workgroups' dequeue counter; nullptr: workgroup i takes entry i, once
  int grid;
  hipStream_t stream;
  int base;          // persistent form: first list entry it takes (0, or the grid of a one-per-entry launch)
};
// The launcher of one build of the wide kernel template: defined in cmpc_wide.h and instantiated
// once per row of kWideBuild (cmpc_wide_builds.h), each in a unit of its own (cmpc_wide_unit.hip).
// Only launch_wide (cmpc_launch.hip) names them, through the table.
template <int NV, bool PERSIST, bool REFINE, bool LIT>
hipError_t launch_wide_build(const KParams& P, const WideCall& c);
// the tail class (cmpc_tail.hip): 8 tail rows beside class 1's 64 (n <= 72), one wavefront per
// instance over its list, one workgroup per possible entry; an instance whose active set outgrows
// 64 positions is appended to ovf_list (batched) or, with ovf_list == nullptr, gets status
// kHandoffStatus (single-instance path: the host re-launches it in the wide class,
// launch_single(..., allow_tail = false))
constexpr uint8_t kHandoffStatus = 0xFE;
// rest_grid > 0: `grid` covers the first entries only (a predicted count), and a looping kernel of
// rest_grid workgroups follows on the stream for any entries past it
hipError_t launch_tail(const float* d_recs, const KParams& P, float* d_forces, uint8_t* d_status,
                       int32_t* d_iters, const int* in_list, const int* in_count, int* ovf_list,
                       int* ovf_count, int grid, hipStream_t stream, int rest_grid = 0);
hipError_t launch_single(const float* d_rec, int n, const KParams& P, float* d_forces,
                         uint8_t* d_status, int32_t* d_iters, const int* d_one, hipStream_t stream,
                         bool allow_tail = true);
// config 5 estimator (cmpc_estimator.hip). d_gauss: the two normalised float Gaussian kernels
// of gaussian_filter (sigma 7: 43 taps, then sigma 27: 163 taps), built on the host exactly as
// SolverMPC.cpp:404-418 builds them.
constexpr int kGaussR7 = 21;   // ceil(3 * 7)
constexpr int kGaussR27 = 81;  // ceil(3 * 27)
constexpr int kGaussTaps = 2 * kGaussR7 + 1 + 2 * kGaussR27 + 1;
// d_fest_out (optional): f_est(3) of instance i also to d_fest_out[i] (the single-instance ABI
// reads it back with the forces). d_due (optional, cmpc_batch_estimate_due): the workgroup of an
// instance with d_due[i] == 0 exits before it reads or writes anything else
hipError_t launch_estimate(float* d_est, const float* d_logs, const float* d_fext3,
                           const float* d_time, float sim_time, float* d_records, int rec_words,
                           float* d_fext6, const float* d_gauss, int batch, hipStream_t stream,
                           const KModel& mdl, float* d_fest_out = nullptr, const uint8_t* d_due = nullptr,
                           const KInst* inst = nullptr);  // inst: entry i's model for instance i's residual
// batched input assembly (cmpc_assemble.hip): one control tick per instance
hipError_t launch_assemble(float* d_loco, const LocoParams& lp, float* d_recs, uint8_t* d_due,
                           int batch, hipStream_t stream);
// compact records (CMPC_CREC_*) -> solve records, trajAll expanded per ConvexMPCLocomotion.cpp:554-585
hipError_t launch_expand(const float* d_compact, float* d_recs, int batch, int N, int rec_words, float dt,
                         hipStream_t stream);
// single-rigid-body step of every due instance with its solved step-0 forces (cmpc_assemble.hip)
hipError_t launch_rollout(float* d_loco, const float* d_recs, const float* d_forces,
                          const float* d_xi6, const uint8_t* d_due, const LocoParams& lp, float dt,
                          const KModel& mdl, int batch, hipStream_t stream, const KInst* inst = nullptr);
// parity hook and JCQP condensation: full (nothing eliminated) qH [12N x 12N] / qg [12N] per
// instance (cmpc_condense.hip)
hipError_t launch_condense(const float* d_recs, int batch, const KParams& P, float* d_H, float* d_g, bool rows,
                           hipStream_t stream);
// fp64 prediction, cost and optimality gap of given forces [batch x 12N] (cmpc_evaluate.hip), one
// wavefront per instance; alpha = the force regularisation (KParams holds 2 alpha in fp32 only;
// with P.inst, (double) of entry i's alpha instead).
// ib64 = the body inertia's three doubles (KParams holds their reciprocals only).
// d_xpred / d_cert: either may be NULL. With P.inst, inst_rows = the handle's snapshot of the
// caller's rows (CMPC_INST_WORDS doubles each): instance i's inertia doubles come from row i
hipError_t launch_evaluate(const float* d_recs, const float* d_forces, int batch, const KParams& P,
                           double alpha, const double* ib64, float* d_xpred, double* d_cert,
                           hipStream_t stream, const double* inst_rows = nullptr);
// the gradients of a loss through the solve at given forces, by an fp64 Riccati adjoint
// (cmpc_sensitivity.hip), one wavefront per instance. d_gradf = dL/dU [batch x 12N]; alpha, ib64
// and inst_rows as launch_evaluate's; d_sens [batch x CMPC_SENS_WORDS]; d_dtraj / d_dg [batch x 12N]:
// either may be NULL
hipError_t launch_sensitivity(const float* d_recs, const float* d_forces, const float* d_gradf, int batch,
                              const KParams& P, double alpha, const double* ib64, double act_tol, double* d_sens,
                              double* d_dtraj, double* d_dg, hipStream_t stream,
                              const double* inst_rows = nullptr);
// the step-0 feedback gain d u_0* / d x_0 at given forces, by the backward half of that recursion
// (cmpc_gain.hip), one wavefront per instance; alpha, ib64, act_tol and inst_rows as
// launch_sensitivity's; d_gain [batch x CMPC_GAIN_WORDS]
hipError_t launch_gain(const float* d_recs, const float* d_forces, int batch, const KParams& P, double alpha,
                       const double* ib64, double act_tol, double* d_gain, hipStream_t stream,
                       const double* inst_rows = nullptr);
// u = guard(u_0 + G (x - x_0)) of every instance that is not due (cmpc_gain.hip): d_forces at the
// stride P.out_cols, d_states and d_u [batch x 12] fp32, d_due [batch] bytes or NULL; with P.inst,
// entry i's 1 / mu and f_max
hipError_t launch_feedback(const float* d_recs, const float* d_forces, const double* d_gain, const float* d_states,
                           const uint8_t* d_due, int batch, const KParams& P, float* d_u, hipStream_t stream);
// per-instance table (cmpc_inst_table.hip). check: *d_bad += the number of rows that
// cmpc_batch_set_model or cmpc_batch_set_params would refuse (d_bad zeroed by the caller);
// convert: the kernel-side entries and the snapshot of the rows, formed as make_kmodel and
// make_kparams form the handle's values on the host
hipError_t launch_inst_check(const double* d_rows, int count, int* d_bad, hipStream_t stream);
hipError_t launch_inst_convert(const double* d_rows, int count, KInst* d_entries, double* d_snapshot,
                               hipStream_t stream);
// the cost table (cmpc_batch_set_instance_costs), rows of CMPC_COST_WORDS floats. check: *d_bad +=
// the number of bad rows (a weight negative or non-finite, alpha non-finite or <= 0, 2.f * alpha
// not finite); convert: the second line of the entries, alpha2 by make_kparams' expression
hipError_t launch_cost_check(const float* d_rows, int count, int* d_bad, hipStream_t stream);
hipError_t launch_cost_convert(const float* d_rows, int count, KInst* d_entries, hipStream_t stream);
// The half of entries [0, count) that has no table, from the handle's shared values: model = true
// the first line (P.mdl, P.mu_inv, P.f_max) and the snapshot rows (mdl64, mu, f_max: what a row of
// cmpc_batch_set_instance_params holds), model = false the second line (P.wts, P.alpha2, alpha).
// Asynchronous on `stream`, the values by value in the argument segment.
hipError_t launch_inst_fill(KInst* d_entries, double* d_snapshot, int count, bool model, const KParams& P,
                            const cmpc_model& mdl64, double mu, double f_max, float alpha, hipStream_t stream);

// use_jcqp == 1 / 2: batched JCQP ADMM over the full / reduced condensed QP (cmpc_admm.hip).
// Instances whose QP has n > 120 variables run on nslabs persistent workgroups with M in
// d_slabs (nslabs * admm_slab_doubles(N) doubles); may be NULL when no such instance can occur.
size_t admm_slab_doubles(int horizon);
constexpr int kAdmmSlabs = 512;
hipError_t launch_admm(const float* d_recs, const float* d_H, const float* d_g, int batch,
                       const KParams& P, const cmpc_admm_settings& s, float* d_forces,
                       uint8_t* d_status, int32_t* d_iters, double* d_slabs, int nslabs,
                       hipStream_t stream);

}  // namespace cmpc
