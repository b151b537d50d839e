// cmpc_abi.cpp — the C ABI of libcmpc_hip.so (declared in include/cmpc_solver.h).
//
//  * cmpc_batch_*: reentrant batched API, one handle per HIP stream, device scratch allocated
//    at create time (never inside solve, so a caller may capture solve into a hipGraph).
//  * setup_problem / update_problem_data(_floats) / update_solver_settings / update_x_drag /
//    get_solution: the reference's single-instance interface (convexMPC_interface.h:44-52) with
//    the same call protocol and semantics, implemented over a batch-1 handle.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <array>
#include <mutex>
#include <utility>
#include <string>
#include <vector>

#include "../../include/cmpc_solver.h"
#include "cmpc_host_buffers.h"
#include "cmpc_kernels.h"

namespace {
thread_local std::string g_last_error;

int fail(const char* what, hipError_t e) {
  g_last_error = std::string(what) + ": " + hipGetErrorString(e);
  return -(int)e - 1000;
}

// 0, or fail(what, e)
int checked(const char* what, hipError_t e) { return e == hipSuccess ? 0 : fail(what, e); }

int bad_arguments(const char* who) {
  g_last_error = std::string(who) + ": bad arguments";
  return -1;
}

// the two allocators of cmpc::Owned (cmpc_host_buffers.h)
struct DeviceAlloc {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void* p) { (void)hipFree(p); }
};
struct PinnedAlloc {
  static hipError_t alloc(void** p, size_t bytes, unsigned flags = hipHostMallocDefault) {
    return hipHostMalloc(p, bytes, flags);
  }
  static void release(void* p) { (void)hipHostFree(p); }
};
template <class T> using DevBuf = cmpc::Owned<T, DeviceAlloc>;
template <class T> using PinBuf = cmpc::Owned<T, PinnedAlloc>;
using Stage = cmpc::SingleStage;
}  // namespace

// The default robot: m = 12, I_body = diag(.07, .26, .242) (RobotState.h:25-26)
static const cmpc_model kDefaultModel = {12.0, {0.07, 0.26, 0.242}};

// (hidden: the handle is opaque to callers, and its destructor is no export of the library)
struct __attribute__((visibility("hidden"))) cmpc_batch {
  cmpc_params prm;
  cmpc_model model = kDefaultModel;  // cmpc_batch_set_model; kept across set_params
  cmpc::KParams kp;              // rebuilt from the four fields around it by rebuild_kparams alone
  int out_steps = 0;             // cmpc_batch_set_output_steps (0: every step)
  int refine = 1;                // cmpc_batch_set_refine (1: from N = 11, 0: off)
  int max_batch = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  DevBuf<int> d_work;
  DevBuf<float> d_gauss;         // gaussian_filter kernels of the config-5 estimator
  // per-instance table (cmpc_batch_set_instance_params): kernel-side entries, the snapshot of the
  // caller's rows and the validation kernel's counter, allocated for max_batch by the first call
  DevBuf<cmpc::KInst> d_inst;
  DevBuf<double> d_inst_rows;
  DevBuf<int> d_inst_bad;
  int inst_count = 0;            // rows of the parameter table in force (0: none)
  int cost_count = 0;            // rows of the cost table in force (cmpc_batch_set_instance_costs; 0: none)
                                 // (kp.inst is null when both are 0)
  DevBuf<double> d_admm_slabs;   // ADMM inverses of QPs with n > 120 (cmpc_admm.hip)
  size_t admm_slab_doubles = 0;
  int admm_nslabs = 0;
  bool admm_used = false;        // slabs are allocated on the first ADMM call, not at create
  bool staged = false;           // every allocation of ensure_staging succeeded
  DevBuf<float> d_admm_H;        // condensed qH / qg staging of the single-instance ADMM path
  // staging for the host-pointer entry point (allocated lazily, sized max_batch)
  DevBuf<float> d_rec;
  DevBuf<float> d_forces;
  DevBuf<uint8_t> d_status;
  DevBuf<int32_t> d_iters;
  // single-instance fast path of cmpc_batch_solve_host: the one-entry instance list {1, 0}, the
  // instance's forces + status word (one D2H), pinned host staging of record and result (Stage)
  DevBuf<int> d_one;
  DevBuf<float> d_single_out;
  PinBuf<float> h_pin;
  // outputs of cmpc_batch_evaluate_host (allocated on its first call, sized max_batch)
  DevBuf<float> d_xpred;
  DevBuf<double> d_cert;
  // input and outputs of cmpc_batch_sensitivity_host (likewise)
  DevBuf<float> d_gradf;
  DevBuf<double> d_sens, d_dtraj, d_dg;
  // output of cmpc_batch_gain_host (likewise)
  DevBuf<double> d_gain;
  // side streams + fork/join events for the wider size classes (cmpc_launch.hip)
  cmpc::LaunchCtx ctx;
  PinBuf<int> h_hint;            // ctx.h_hint: freed after the own stream is idle (cmpc_batch_destroy)
  bool pooled_sides = false;     // ctx.side came from the process-wide pool (acquire_sides)
  // optional per-launch timing (cmpc_batch_enable_timing)
  std::vector<hipEvent_t> ev;
  int ev_steps = 0, ev_next = 0;
  int ev_every = 1, ev_solves = 0;  // events on every ev_every-th solve (cmpc_batch_enable_timing_every)
};

// copies on the handle's stream and its synchronisation: 0, or the failure's code with its text set
static int stream_h2d(cmpc_batch* h, void* dst, const void* src, size_t bytes) {
  return checked("H2D", hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
}
static int stream_d2h(cmpc_batch* h, void* dst, const void* src, size_t bytes) {
  return checked("D2H", hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
}
static int stream_sync(cmpc_batch* h) {
  return checked("sync", hipStreamSynchronize(h->stream));
}

constexpr int CMPC_REFINE_FROM_N = 11;  // first horizon whose wide classes refine

// Side streams come from a process-wide pool and go back to it when a handle is destroyed; a new
// handle takes the oldest free set. The runtime maps streams onto a few hardware queues
// (GPU_MAX_HW_QUEUES = 4 by default) as they are created, and a set created while other streams
// were alive can share a hardware queue with the caller's stream: its side classes then queue
// behind class 1 (32768 instances 0.90 -> 1.17-1.25 ms per solve, 65536 1.48 -> 1.83 ms;
// scripts/stream_probe.py, profiles/r05_ab/r05_q .. r05_t). With the oldest free set first, one
// handle at a time always runs on the first handle's streams. Pooled per device.
namespace {
struct SideSet {
  int dev;
  bool busy;
  std::array<hipStream_t, cmpc::kSideStreams> s;
};
struct SidePool {
  std::mutex mu;
  std::vector<SideSet> sets;  // in creation order
};
SidePool& side_pool() {
  static SidePool* p = new SidePool();  // never destroyed: the streams live as long as the process
  return *p;
}
hipError_t acquire_sides(std::array<hipStream_t, cmpc::kSideStreams>& out, int prio) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(side_pool().mu);
  for (auto& set : side_pool().sets) {
    if (set.dev == dev && !set.busy) {
      set.busy = true;
      out = set.s;
      return hipSuccess;
    }
  }
  SideSet set{dev, true, {}};
  for (int j = 0; j < cmpc::kSideStreams; j++) {
    e = hipStreamCreateWithPriority(&set.s[j], hipStreamNonBlocking, prio);
    if (e != hipSuccess) {
      for (int k = 0; k < j; k++) (void)hipStreamDestroy(set.s[k]);
      return e;
    }
  }
  side_pool().sets.push_back(set);
  out = set.s;
  return hipSuccess;
}
void release_sides(const std::array<hipStream_t, cmpc::kSideStreams>& s) {
  std::lock_guard<std::mutex> lk(side_pool().mu);
  for (auto& set : side_pool().sets)
    if (set.s[0] == s[0]) set.busy = false;
}
}  // namespace

// The kernels' form of the model, every derived value formed here once. The fp32 kernels get
// (float) of each field and 1.f / (float) mass, the fp64 paths the reciprocals of the doubles:
// for the default these are the values the literals .07f, 1.f / 12.0f, 1.0 / 0.07 and 1.0 / 12.0
// had, so the default gives the same bits as before the model was a parameter.
static cmpc::KModel make_kmodel(const cmpc_model& m) {
  cmpc::KModel k{};
  for (int i = 0; i < 3; i++) {
    k.ib[i] = (float)m.inertia[i];
    k.iinv64[i] = 1.0 / m.inertia[i];
  }
  k.im = 1.f / (float)m.mass;
  k.im64 = 1.0 / m.mass;
  return k;
}

static bool model_ok(const cmpc_model& m) {
  // finite and positive, in double and after the fp32 kernels' cast
  auto ok = [](double v) { return std::isfinite(v) && v > 0.0 && std::isfinite((float)v) && (float)v > 0.f; };
  if (!(ok(m.mass) && ok(m.inertia[0]) && ok(m.inertia[1]) && ok(m.inertia[2]))) return false;
  // and every value derived from them (a denormal mass or inertia has an infinite reciprocal)
  const cmpc::KModel k = make_kmodel(m);
  bool fin = std::isfinite(k.im) && k.im > 0.f && std::isfinite(k.im64) && k.im64 > 0.0;
  for (int i = 0; i < 3; i++) fin = fin && std::isfinite(k.iinv64[i]) && k.iinv64[i] > 0.0;
  return fin;
}

// Every derived field of the kernels' parameters, from the four things a handle is set to: pure, so
// rebuilding all of it where one of them changed gives the same bits as updating that field alone.
// (kp.inst and, with it, kp.mdl_default are the tables' part: apply_inst.)
static cmpc::KParams make_kparams(const cmpc_params& p, const cmpc_model& m, int out_steps, int refine) {
  cmpc::KParams k{};
  k.mdl = make_kmodel(m);
  k.dt = p.dt;
  k.mu_inv = 1.f / p.mu;  // fpt mu = 1.f / setup->mu (SolverMPC.cpp:657)
  k.f_max = p.f_max;
  k.alpha2 = 2.f * p.alpha;
  for (int i = 0; i < 12; i++) k.wts[i] = p.weights[i];
  k.N = p.horizon;
  k.rec_words = CMPC_REC_WORDS(p.horizon);
  k.max_iter = p.max_iter > 0 ? p.max_iter : 100;
  // the fp32 pipelines of the reference and of this solver are within ~1e-5 of the exact optimum
  // at N <= 10 and drift to ~1e-4 beyond: the refinement runs from N = 11
  k.refine = (refine && p.horizon >= CMPC_REFINE_FROM_N) ? 1 : 0;
  k.dt64 = (double)k.dt;
  k.dth64 = 0.5 * k.dt64 * k.dt64;
  k.dt3_64 = k.dt64 * k.dt64 * k.dt64 / 6.0;
  k.out_cols = 12 * ((out_steps > 0 && out_steps < p.horizon) ? out_steps : p.horizon);
  return k;
}

extern "C" int cmpc_record_words(int horizon) { return CMPC_REC_WORDS(horizon); }

// The float kernel of gaussian_filter (SolverMPC.cpp:404-418): taps exp(-0.5 i^2 / sigma^2)
// evaluated in double, stored as float, normalised by their float sum.
static void gauss_kernel(float sigma, int radius, float* out) {
  float sum = 0.0f;
  for (int i = -radius; i <= radius; i++) {
    const float value = std::exp(-0.5 * (i * i) / (sigma * sigma));
    out[i + radius] = value;
    sum += value;
  }
  for (int i = 0; i < 2 * radius + 1; i++) out[i] /= sum;
}

extern "C" const char* cmpc_last_error(void) { return g_last_error.c_str(); }
namespace cmpc {
void set_last_error(const char* msg) { g_last_error = msg; }  // for the other translation units
}  // namespace cmpc

// the ADMM kernel keeps M^-1 of QPs with more than 120 variables in per-workgroup fp64 slabs:
// min(max_batch, kAdmmSlabs) of (12N)^2 doubles (151 MB at N = 16, 236 MB at N = 20). They are
// allocated by the first cmpc_batch_admm call of a handle (and kept across set_params from then
// on), so handles that only run the default qpOASES-equivalent solve never pay for them; the
// solve kernels themselves never allocate.
static int ensure_admm_slabs(cmpc_batch* h) {
  if (!h->admm_used || h->max_batch <= 0 || 12 * h->prm.horizon <= 120) return 0;
  const int ns = h->max_batch < cmpc::kAdmmSlabs ? h->max_batch : cmpc::kAdmmSlabs;
  const size_t need = (size_t)ns * cmpc::admm_slab_doubles(h->prm.horizon);
  if (need <= h->admm_slab_doubles && h->admm_nslabs >= ns) return 0;
  h->admm_slab_doubles = 0;
  h->admm_nslabs = 0;
  // (the smaller slabs are released first)
  if (int r = checked("hipMalloc(ADMM slabs)", h->d_admm_slabs.alloc(need))) return r;
  h->admm_slab_doubles = need;
  h->admm_nslabs = ns;
  return 0;
}

// kp's view of the per-instance tables, after anything that rebuilt kp or changed a table. While
// either is set no launcher takes a literal-model build (they hold the default robot's values).
// With one of the two set, the other half of its entries takes the handle's shared values as they
// now stand: a kernel on the handle's stream, behind every earlier call and ahead of every later
// one, no allocation, no host synchronisation.
static int apply_inst(cmpc_batch* h) {
  h->kp.inst = (h->inst_count > 0 || h->cost_count > 0) ? h->d_inst.get() : nullptr;
  h->kp.mdl_default = !h->kp.inst && std::memcmp(&h->model, &kDefaultModel, sizeof h->model) == 0;
  if (!h->kp.inst || (h->inst_count > 0 && h->cost_count > 0)) return 0;
  const bool model_half = h->inst_count == 0;
  return checked("launch_inst_fill",
                 cmpc::launch_inst_fill(h->d_inst.get(), h->d_inst_rows.get(), model_half ? h->cost_count : h->inst_count,
                                        model_half, h->kp, h->model, (double)h->prm.mu, (double)h->prm.f_max,
                                        h->prm.alpha, h->stream));
}

// h->kp from the handle's prm, model, out_steps and refine, then the tables' view of it: what every
// setter of one of the four calls, so no derived field is stated anywhere else
static int rebuild_kparams(cmpc_batch* h) {
  h->kp = make_kparams(h->prm, h->model, h->out_steps, h->refine);
  return apply_inst(h);
}

// a batch the handle can take: within max_batch and, with a per-instance table, within its rows
static bool batch_ok(const cmpc_batch* h, int batch) {
  return batch >= 0 && batch <= h->max_batch && (h->inst_count == 0 || batch <= h->inst_count) &&
         (h->cost_count == 0 || batch <= h->cost_count);
}

// the tables' buffers, for max_batch, by the first call that sets either table: 128 B of entry and
// 48 B of row snapshot per instance, and the validation kernels' counter
static int ensure_inst_buffers(cmpc_batch* h) {
  if (h->d_inst) return 0;
  DevBuf<cmpc::KInst> ent;
  DevBuf<double> rows;
  DevBuf<int> bad;
  hipError_t e;
  if ((e = ent.alloc((size_t)h->max_batch)) != hipSuccess ||
      (e = rows.alloc(CMPC_INST_WORDS * (size_t)h->max_batch)) != hipSuccess ||
      (e = bad.alloc(1)) != hipSuccess)
    return fail("hipMalloc(instance table)", e);
  h->d_inst = std::move(ent);
  h->d_inst_rows = std::move(rows);
  h->d_inst_bad = std::move(bad);
  return 0;
}

extern "C" int cmpc_batch_set_params(cmpc_batch* h, const cmpc_params* prm) {
  if (!h || !prm) return -1;
  if (prm->horizon < 1 || prm->horizon > CMPC_MAX_HORIZON) {
    g_last_error = "horizon out of range";
    return -2;
  }
  h->prm = *prm;
  if (int r = rebuild_kparams(h)) return r;
  return ensure_admm_slabs(h);
}

extern "C" int cmpc_batch_set_model(cmpc_batch* h, const cmpc_model* m) {
  if (!h) return -1;
  const cmpc_model nm = m ? *m : kDefaultModel;
  if (!model_ok(nm)) {
    g_last_error = "cmpc_batch_set_model: mass and inertia must be finite and positive";
    return -2;
  }
  h->model = nm;
  return rebuild_kparams(h);
}

// What the two per-instance tables differ in, a row each; set_table is the one setter of both.
namespace {
template <class Row>
struct Table {
  const char* name;        // the entry point, for the error texts
  const char* bad_rows;    // what makes a row bad
  int cmpc_batch::*count;  // the rows in force
  const char* check_name;  // check: *d_bad += the number of bad rows
  hipError_t (*check)(const Row* d_rows, int count, int* d_bad, hipStream_t stream);
  const char* convert_name;  // convert: the rows into the handle's entries (and snapshot)
  hipError_t (*convert)(const Row* d_rows, int count, cmpc_batch* h);
};
const Table<double> kParamTable = {
    "cmpc_batch_set_instance_params", "mass, inertia and mu must be finite and positive, f_max finite",
    &cmpc_batch::inst_count, "launch_inst_check", cmpc::launch_inst_check, "launch_inst_convert",
    [](const double* d, int n, cmpc_batch* h) {
      return cmpc::launch_inst_convert(d, n, h->d_inst.get(), h->d_inst_rows.get(), h->stream);
    }};
const Table<float> kCostTable = {
    "cmpc_batch_set_instance_costs", "weights must be finite and >= 0, alpha finite and > 0 with 2 alpha finite",
    &cmpc_batch::cost_count, "launch_cost_check", cmpc::launch_cost_check, "launch_cost_convert",
    [](const float* d, int n, cmpc_batch* h) { return cmpc::launch_cost_convert(d, n, h->d_inst.get(), h->stream); }};

// d_rows null clears the table: the handle's shared values again (the buffers stay for the next one)
template <class Row>
int set_table(cmpc_batch* h, const Table<Row>& t, const Row* d_rows, int count) {
  if (!h) return -1;
  hipError_t e;
  int bad = 0;
  if (d_rows) {
    if (count < 1 || count > h->max_batch) {
      g_last_error = std::string(t.name) + ": count must be in 1..max_batch";
      return -1;
    }
    if (int r = ensure_inst_buffers(h)) return r;  // first call of either table
    int* d_bad = h->d_inst_bad.get();
    if ((e = hipMemsetAsync(d_bad, 0, sizeof(int), h->stream)) != hipSuccess) return fail("memset", e);
    if ((e = t.check(d_rows, count, d_bad, h->stream)) != hipSuccess) return fail(t.check_name, e);
    if (int r = stream_d2h(h, &bad, d_bad, sizeof(int))) return r;
  }
  // (also: every earlier call on the handle's stream that reads the table in force is done)
  if (int r = stream_sync(h)) return r;
  if (bad != 0) {
    g_last_error = std::string(t.name) + ": " + std::to_string(bad) + " bad row(s): " + t.bad_rows;
    return -2;
  }
  if (d_rows && (e = t.convert(d_rows, count, h)) != hipSuccess) return fail(t.convert_name, e);
  h->*t.count = d_rows ? count : 0;
  // (with one table in force, the other half of its entries from the handle's shared values)
  if (int r = apply_inst(h)) return r;
  return stream_sync(h);
}
}  // namespace

extern "C" int cmpc_batch_set_instance_params(cmpc_batch* h, const double* d_inst, int count) {
  return set_table(h, kParamTable, d_inst, count);
}

extern "C" int cmpc_batch_instance_count(const cmpc_batch* h) { return h ? h->inst_count : 0; }

extern "C" int cmpc_batch_set_instance_costs(cmpc_batch* h, const float* d_cost, int count) {
  return set_table(h, kCostTable, d_cost, count);
}

extern "C" int cmpc_batch_instance_cost_count(const cmpc_batch* h) { return h ? h->cost_count : 0; }

extern "C" int cmpc_batch_get_model(const cmpc_batch* h, cmpc_model* out) {
  if (!h || !out) return -1;
  *out = h->model;
  return 0;
}

extern "C" int cmpc_batch_set_refine(cmpc_batch* h, int on) {
  if (!h || on < 0 || on > 1) return bad_arguments("cmpc_batch_set_refine");
  h->refine = on;
  return rebuild_kparams(h);
}

extern "C" int cmpc_batch_set_output_steps(cmpc_batch* h, int steps) {
  if (!h || steps < 0) return bad_arguments("cmpc_batch_set_output_steps");
  h->out_steps = steps;
  return rebuild_kparams(h);
}

// The fork / classified / join events order queues of this one device only: every producer and
// consumer of the data they guard is a kernel on this GPU, whose dispatch packets carry their own
// device-scope acquire / release (the per-XCD L2s written back and invalidated at kernel
// boundaries), and the caller's copies to the host order after the join on its stream. So these
// events are recorded without the system-scope fence HIP adds by default (an L2 writeback and
// invalidate per record, five records per solve): config 2 +3 to +4 %, 32768 instances +0.5 to
// +1 %, config 3 +1 % (profiles/r06_s2/env_ab.log; device scope instead: within noise). The timing
// events (cmpc_batch_enable_timing) are recorded without it too.
// CMPC_EVENT_SCOPE (A/B): 0 HIP's default (system scope), 1 device scope (ordering events only),
// 2 no system fence
static unsigned event_flags(bool timing) {
  const int scope = cmpc::diag_knob("CMPC_EVENT_SCOPE", 2);
  const unsigned fence = scope == 2 ? hipEventDisableSystemFence : 0u;
  if (timing) return fence;
  return hipEventDisableTiming | (scope == 1 ? hipEventReleaseToDevice : fence);
}

// everything a new handle acquires; on a failure cmpc_batch_create destroys what was acquired so far
static int init_handle(cmpc_batch* h, const cmpc_params* prm, int max_batch, void* hip_stream) {
  if (int r = cmpc_batch_set_params(h, prm)) return r;
  h->max_batch = max_batch;
  if (hip_stream) {
    h->stream = (hipStream_t)hip_stream;
  } else {
    if (int r = checked("hipStreamCreate", hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking))) return r;
    h->own_stream = true;
  }
  // side streams at the highest priority: their few, long class-2 solves are dispatched ahead
  // of class 1's queue, so they finish inside class 1's run instead of forming a tail
  int prio_lo = 0, prio_hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  if (cmpc::diag_knob("CMPC_SIDE_PRIORITY", 1) == 0) prio_hi = prio_lo;
  std::array<hipStream_t, cmpc::kSideStreams> sides{};
  if (int r = checked("side streams", acquire_sides(sides, prio_hi))) return r;
  for (int j = 0; j < cmpc::kSideStreams; j++) h->ctx.side[j] = sides[j];
  h->pooled_sides = true;
  const unsigned ev_flags = event_flags(false);
  for (int j = 0; j < cmpc::kSideStreams; j++)
    if (int r = checked("side events", hipEventCreateWithFlags(&h->ctx.join[j], ev_flags))) return r;
  hipError_t e = hipEventCreateWithFlags(&h->ctx.fork, ev_flags);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ctx.classified, ev_flags);
  if (e != hipSuccess) return fail("fork event", e);
  // the class-count hint (cmpc_launch.hip): pinned, mapped, zero (no hint) until a classify pass
  // copies a finished solve's header into it
  e = h->h_hint.alloc(cmpc::kHdr, hipHostMallocMapped);
  if (e == hipSuccess) {
    h->ctx.h_hint = h->h_hint.get();
    std::memset(h->ctx.h_hint, 0, sizeof(int) * cmpc::kHdr);
    e = hipHostGetDevicePointer(reinterpret_cast<void**>(&h->ctx.d_hint), h->ctx.h_hint, 0);
  }
  if (e != hipSuccess) return fail("hint buffer", e);
  e = h->d_work.alloc(cmpc::work_ints(max_batch));
  if (e == hipSuccess) e = hipMemset(h->d_work.get(), 0, sizeof(int) * 2 * cmpc::kHdr);  // both list headers
  if (e != hipSuccess) return fail("hipMalloc(work)", e);
  float taps[cmpc::kGaussTaps];
  gauss_kernel(7.0f, cmpc::kGaussR7, taps);
  gauss_kernel(27.0f, cmpc::kGaussR27, taps + 2 * cmpc::kGaussR7 + 1);
  e = h->d_gauss.alloc(cmpc::kGaussTaps);
  if (e == hipSuccess) e = hipMemcpy(h->d_gauss.get(), taps, sizeof(taps), hipMemcpyHostToDevice);
  return checked("gauss taps", e);
}

extern "C" int cmpc_batch_create(cmpc_batch** out, const cmpc_params* prm, int max_batch,
                                 void* hip_stream) {
  if (!out || !prm || max_batch < 1) return -1;
  auto* h = new cmpc_batch();
  if (int r = init_handle(h, prm, max_batch, hip_stream)) {
    cmpc_batch_destroy(h);  // (leaves cmpc_last_error as the failed step set it)
    return r;
  }
  *out = h;
  return 0;
}

static void free_staging(cmpc_batch* h);

// The order is part of the contract: the buffers first (here, not by the handle's destructor), the
// side streams idle and back in the pool, the events, the own stream idle, then the hint buffer its
// kernels write, then the stream itself.
extern "C" void cmpc_batch_destroy(cmpc_batch* h) {
  if (!h) return;
  h->d_work.reset();
  h->d_gauss.reset();
  h->d_admm_slabs.reset();
  h->d_inst.reset();
  h->d_inst_rows.reset();
  h->d_inst_bad.reset();
  free_staging(h);
  for (auto e : h->ev) (void)hipEventDestroy(e);
  if (h->pooled_sides) {
    // back to the pool once every side stream is idle (the next handle may fork on them at once)
    std::array<hipStream_t, cmpc::kSideStreams> sides{};
    for (int j = 0; j < cmpc::kSideStreams; j++) {
      sides[j] = h->ctx.side[j];
      (void)hipStreamSynchronize(sides[j]);
    }
    release_sides(sides);
  }
  for (int j = 0; j < cmpc::kSideStreams; j++)
    if (h->ctx.join[j]) (void)hipEventDestroy(h->ctx.join[j]);
  if (h->ctx.fork) (void)hipEventDestroy(h->ctx.fork);
  if (h->ctx.classified) (void)hipEventDestroy(h->ctx.classified);
  if (h->own_stream && h->stream) (void)hipStreamSynchronize(h->stream);
  h->h_hint.reset();  // (the classify kernels writing it are done)
  h->ctx.h_hint = nullptr;
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" void* cmpc_batch_stream(cmpc_batch* h) { return h ? (void*)h->stream : nullptr; }

// the events of this solve's launches, where per-launch timing is on and this solve is due for it
static hipEvent_t* next_timing_events(cmpc_batch* h) {
  if (h->ev_steps > 0 && h->ev_next < h->ev_steps && h->ev_solves++ % h->ev_every == 0)
    return &h->ev[3 * h->ev_next++];
  return nullptr;
}

// The masked entry points are the bodies of their plain forms too: the plain form is the masked one
// with a null mask, and says so in its error text.
extern "C" int cmpc_batch_solve_due(cmpc_batch* h, const float* d_records, const uint8_t* d_due, int batch,
                                    float* d_forces, uint8_t* d_status, int32_t* d_iters) {
  if (!h || !batch_ok(h, batch) || (!d_records && batch) || (!d_forces && batch) || (!d_status && batch))
    return bad_arguments(d_due ? "cmpc_batch_solve_due" : "cmpc_batch_solve");
  // (A HIP graph of this launch sequence, replayed while the arguments repeat, measured config 3
  // 41.8 M -> 32.5 M and config 2 14.7 M -> 9.8 M QP/s: the replay lost the overlap of class 1
  // with the side-stream classes, profiles/r04_ab/r04_m*. Direct launches only.)
  return checked("launch_solve",
                 cmpc::launch_solve(d_records, batch, h->kp, d_forces, d_status, d_iters, h->d_work.get(), h->max_batch,
                                    h->stream, h->ctx, next_timing_events(h), d_due));
}

extern "C" int cmpc_batch_solve(cmpc_batch* h, const float* d_records, int batch, float* d_forces,
                                uint8_t* d_status, int32_t* d_iters) {
  return cmpc_batch_solve_due(h, d_records, nullptr, batch, d_forces, d_status, d_iters);
}

extern "C" int cmpc_batch_estimate_due(cmpc_batch* h, float* d_est, const float* d_logs,
                                       const float* d_fext3, const float* d_time, float sim_time,
                                       float* d_records, float* d_fext6, const uint8_t* d_due, int batch) {
  if (!h || !batch_ok(h, batch) || (batch && (!d_est || !d_records)) || (batch && !d_logs && !d_fext3))
    return bad_arguments(d_due ? "cmpc_batch_estimate_due" : "cmpc_batch_estimate");
  return checked("launch_estimate",
                 cmpc::launch_estimate(d_est, d_logs, d_fext3, d_time, sim_time, d_records, h->kp.rec_words, d_fext6,
                                       h->d_gauss.get(), batch, h->stream, h->kp.mdl, nullptr, d_due, h->kp.inst));
}

extern "C" int cmpc_batch_estimate(cmpc_batch* h, float* d_est, const float* d_logs,
                                   const float* d_fext3, const float* d_time, float sim_time,
                                   float* d_records, float* d_fext6, int batch) {
  return cmpc_batch_estimate_due(h, d_est, d_logs, d_fext3, d_time, sim_time, d_records, d_fext6, nullptr, batch);
}

extern "C" int cmpc_batch_assemble(cmpc_batch* h, float* d_loco, const cmpc_loco_params* lp,
                                   float* d_records, uint8_t* d_due, int batch) {
  if (!h || !lp || batch < 0 || batch > h->max_batch ||
      (batch && (!d_loco || !d_records || !d_due)) || !(lp->dt > 0.f) ||
      lp->iters_between_mpc < 1)
    return bad_arguments("cmpc_batch_assemble");
  cmpc::LocoParams kp{lp->dt,        lp->iters_between_mpc, lp->x_drag_gain,  h->kp.N,
                      h->kp.rec_words, lp->hip_x,            lp->hip_y,        lp->abad_link,
                      lp->swing_height, lp->bonus_swing,     h->kp.out_cols};
  return checked("launch_assemble", cmpc::launch_assemble(d_loco, kp, d_records, d_due, batch, h->stream));
}

extern "C" int cmpc_batch_expand(cmpc_batch* h, const float* d_compact, float* d_records, int batch) {
  if (!h || batch < 0 || batch > h->max_batch || (batch && (!d_compact || !d_records)))
    return bad_arguments("cmpc_batch_expand");
  return checked("launch_expand",
                 cmpc::launch_expand(d_compact, d_records, batch, h->kp.N, h->kp.rec_words, h->kp.dt, h->stream));
}

extern "C" int cmpc_batch_rollout(cmpc_batch* h, float* d_loco, const float* d_records,
                                  const float* d_forces, const float* d_xi6, const uint8_t* d_due,
                                  int batch) {
  if (!h || !batch_ok(h, batch) || (batch && (!d_loco || !d_records || !d_forces)))
    return bad_arguments("cmpc_batch_rollout");
  cmpc::LocoParams kp{h->kp.dt, 1, 0.f, h->kp.N, h->kp.rec_words, 0.f, 0.f, 0.f, 0.f, 0.f, h->kp.out_cols};
  return checked("launch_rollout", cmpc::launch_rollout(d_loco, d_records, d_forces, d_xi6, d_due, kp, h->kp.dt,
                                                        h->kp.mdl, batch, h->stream, h->kp.inst));
}

extern "C" int cmpc_batch_enable_timing(cmpc_batch* h, int steps) {
  return cmpc_batch_enable_timing_every(h, steps, 1);
}

extern "C" int cmpc_batch_enable_timing_every(cmpc_batch* h, int steps, int every) {
  if (!h || steps < 0 || every < 1) return -1;
  h->ev_every = every;
  h->ev_solves = 0;
  for (auto e : h->ev) (void)hipEventDestroy(e);
  h->ev.assign(3 * (size_t)steps, nullptr);
  const unsigned tflags = event_flags(true);
  for (auto& e : h->ev)
    if (hipError_t r = hipEventCreateWithFlags(&e, tflags); r != hipSuccess) return fail("hipEventCreate", r);
  h->ev_steps = steps;
  h->ev_next = 0;
  return 0;
}

extern "C" int cmpc_batch_read_timing(cmpc_batch* h, float* ms, int* steps_recorded,
                                      int* class1_overflow) {
  if (!h) return -1;
  if (int r = stream_sync(h)) return r;
  for (int i = 0; i < h->ev_next; i++) {
    float a = 0.f, b = 0.f;
    (void)hipEventElapsedTime(&a, h->ev[3 * i], h->ev[3 * i + 1]);
    (void)hipEventElapsedTime(&b, h->ev[3 * i + 1], h->ev[3 * i + 2]);
    ms[2 * i] = a;
    ms[2 * i + 1] = b;
  }
  (void)hipGetLastError();  // an unrecorded event must not poison the next launch's check
  if (steps_recorded) *steps_recorded = h->ev_next;
  if (class1_overflow) {
    int c = 0;
    const hipError_t e = hipMemcpy(&c, h->d_work.get() + h->ctx.last_hdr * cmpc::kHdr, sizeof(int), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail("D2H", e);
    *class1_overflow = c;
  }
  h->ev_next = 0;
  return 0;
}

static int condense_device(cmpc_batch* h, const float* d_records, int batch, float* d_H, float* d_g, bool rows) {
  if (!h || !batch_ok(h, batch)) return -1;
  return checked("launch_condense", cmpc::launch_condense(d_records, batch, h->kp, d_H, d_g, rows, h->stream));
}

extern "C" int cmpc_batch_condense(cmpc_batch* h, const float* d_records, int batch, float* d_H,
                                   float* d_g) {
  return condense_device(h, d_records, batch, d_H, d_g, false);
}

extern "C" int cmpc_batch_condense_rows(cmpc_batch* h, const float* d_records, int batch, float* d_H,
                                        float* d_g) {
  return condense_device(h, d_records, batch, d_H, d_g, true);
}

extern "C" int cmpc_batch_admm(cmpc_batch* h, const float* d_records, const float* d_H,
                               const float* d_g, int batch, const cmpc_admm_settings* s,
                               float* d_forces, uint8_t* d_status, int32_t* d_iters) {
  if (!h || !s || !batch_ok(h, batch) ||
      (batch && (!d_records || !d_H || !d_g || !d_forces || !d_status)))
    return bad_arguments("cmpc_batch_admm");
  if (!h->admm_used) {
    h->admm_used = true;
    if (int r = ensure_admm_slabs(h)) { h->admm_used = false; return r; }
  }
  return checked("launch_admm", cmpc::launch_admm(d_records, d_H, d_g, batch, h->kp, *s, d_forces, d_status,
                                                  d_iters, h->d_admm_slabs.get(), h->admm_nslabs, h->stream));
}

static void free_staging(cmpc_batch* h) {
  h->d_rec.reset();
  h->d_forces.reset();
  h->d_status.reset();
  h->d_iters.reset();
  h->d_admm_H.reset();
  h->d_one.reset();
  h->d_single_out.reset();
  h->h_pin.reset();
  h->d_xpred.reset();
  h->d_cert.reset();
  h->d_gradf.reset();
  h->d_sens.reset();
  h->d_dtraj.reset();
  h->d_dg.reset();
  h->staged = false;
}

// staging of the host-pointer entry points, allocated on first use; all or nothing (a failed
// allocation frees what was allocated, so a later call retries instead of using null buffers)
static int ensure_staging(cmpc_batch* h) {
  if (h->staged) return 0;
  const size_t B = (size_t)h->max_batch;
  const size_t nv = Stage::kForcesMax;  // qH / qg of one instance (single ADMM path)
  const int one[2] = {1, 0};
  hipError_t e;
  const char* what = "hipMalloc";
  // d_rec: kPad words past the last record, so the single-instance round trip's words behind its
  // one record fit whatever max_batch is
  if ((e = h->d_rec.alloc(Stage::kRecMax * B + Stage::kPad)) == hipSuccess &&
      (e = h->d_forces.alloc(Stage::kForcesMax * B)) == hipSuccess &&
      (e = h->d_status.alloc(B)) == hipSuccess &&
      (e = h->d_iters.alloc(B)) == hipSuccess &&
      (e = h->d_admm_H.alloc(nv * nv + nv)) == hipSuccess &&
      (e = h->d_one.alloc(2)) == hipSuccess &&
      (e = h->d_single_out.alloc(Stage::kOutWords)) == hipSuccess &&
      (what = "hipHostMalloc", e = h->h_pin.alloc(Stage::kPinWords)) == hipSuccess &&
      (what = "H2D", e = hipMemcpy(h->d_one.get(), one, sizeof(one), hipMemcpyHostToDevice)) == hipSuccess) {
    h->staged = true;
    return 0;
  }
  free_staging(h);
  return fail(what, e);
}

// reduced size n = 3 x (stance foot-steps) of one record: eliminated iff |gait * f_max| < 0.01,
// the test of the classify pass and of every solver kernel (SolverMPC.cpp:869-894)
static int host_reduced_size(const float* rec, int N, float f_max) {
  const unsigned char* gait = reinterpret_cast<const unsigned char*>(rec + CMPC_REC_GAIT(N));
  int nfs = 0;
  for (int t = 0; t < 4 * N; t++) {
    const float ub = (float)gait[t] * f_max;
    nfs += (ub < 0.01f && ub > -0.01f) ? 0 : 1;
  }
  return 3 * nfs;
}

// The record of one instance, and `in_extra` words behind it (0, or 2: the reference surface's
// f_ext[3] and simulation_time), through pinned memory to h->d_rec in one H2D. With d_est, the
// estimator step on those two words follows: it writes f_est(3) and the use-f_est flag into the
// device record, and f_est(3) behind the status word of d_single_out.
static int single_upload(cmpc_batch* h, const float* rec, const float* extra, int in_extra, float* d_est) {
  const int N = h->prm.horizon;
  const size_t rw = (size_t)CMPC_REC_WORDS(N);
  float* pin_rec = h->h_pin.get();
  float* d_rec = h->d_rec.get();
  std::memcpy(pin_rec, rec, rw * sizeof(float));
  if (in_extra) std::memcpy(pin_rec + rw, extra, in_extra * sizeof(float));
  if (int r = stream_h2d(h, d_rec, pin_rec, (rw + in_extra) * sizeof(float))) return r;
  if (!d_est) return 0;
  return checked("launch_estimate",
                 cmpc::launch_estimate(d_est, nullptr, d_rec + rw, d_rec + rw + 1, 0.f, d_rec, (int)rw, nullptr,
                                       h->d_gauss.get(), 1, h->stream, h->kp.mdl,
                                       h->d_single_out.get() + Stage::status_word(N) + 1));
}

// One instance from host memory through the kernel of its size class: the round trip of
// cmpc_batch_solve_host's batch of one and of the reference surface's qpOASES-equivalent solve.
// single_upload, launch_single, one D2H of the forces, the status word and `out_extra` words behind
// it (0, or 1: f_est(3)), sync. The result stays in the pinned out area, which is returned through
// `out`, for the caller to unpack.
// The tail classes hand an instance whose active set outgrows 64 positions to the 80-column wide
// class (cmpc_tail.hip), which shows here as the status byte kHandoffStatus: the record, already on
// the device, is then launched once more in the wide class and read again (the words behind the
// status word stay from the first read).
static int single_round_trip(cmpc_batch* h, const float* rec, const float* extra, int in_extra, int out_extra,
                             float* d_est, int32_t* iters, const float** out) {
  if (int r = single_upload(h, rec, extra, in_extra, d_est)) return r;
  const int N = h->prm.horizon;
  const int n = host_reduced_size(rec, N, h->prm.f_max);
  float* pin_out = h->h_pin.get() + Stage::kPinOut;
  float* d_out = h->d_single_out.get();
  uint8_t* d_st = reinterpret_cast<uint8_t*>(d_out + Stage::status_word(N));
  for (const bool first : {true, false}) {
    const hipError_t e = cmpc::launch_single(h->d_rec.get(), n, h->kp, d_out, d_st, h->d_iters.get(), h->d_one.get(),
                                             h->stream, /*allow_tail=*/first);
    if (e != hipSuccess) return fail("launch_single", e);
    if (int r = stream_d2h(h, pin_out, d_out, Stage::out_words(N, first ? out_extra : 0) * sizeof(float))) return r;
    if (iters)
      if (int r = stream_d2h(h, iters, h->d_iters.get(), sizeof(int32_t))) return r;
    if (int r = stream_sync(h)) return r;
    uint8_t st = 0;
    std::memcpy(&st, pin_out + Stage::status_word(N), 1);
    if (st != cmpc::kHandoffStatus) break;
  }
  *out = pin_out;
  return 0;
}

// batch == 1 from host memory: one kernel of the instance's class, pinned copies, one D2H
static int solve_single_host(cmpc_batch* h, const float* record, float* forces, uint8_t* status,
                             int32_t* iters) {
  const float* out = nullptr;
  if (int r = single_round_trip(h, record, nullptr, 0, 0, nullptr, iters, &out)) return r;
  std::memcpy(forces, out, h->kp.out_cols * sizeof(float));
  if (status) std::memcpy(status, out + Stage::status_word(h->prm.horizon), 1);
  return 0;
}

extern "C" int cmpc_batch_solve_host(cmpc_batch* h, const float* records, int batch, float* forces,
                                     uint8_t* status, int32_t* iters) {
  if (!h || !batch_ok(h, batch)) return -1;
  if (batch == 0) return 0;
  if (int r = ensure_staging(h)) return r;
  const int N = h->prm.horizon;
  const size_t rw = (size_t)CMPC_REC_WORDS(N);
  // one instance (the reference ABI's operating mode): the fast path, unless per-launch timing
  // is on (it brackets the batched launch sequence)
  // (with a per-instance table the batched sequence: its classify pass reads the row's f_max)
  if (batch == 1 && h->ev_steps == 0 && !h->kp.inst) return solve_single_host(h, records, forces, status, iters);
  if (int r = stream_h2d(h, h->d_rec.get(), records, rw * batch * sizeof(float))) return r;
  if (int r = cmpc_batch_solve(h, h->d_rec.get(), batch, h->d_forces.get(), h->d_status.get(), h->d_iters.get()))
    return r;
  if (int r = stream_d2h(h, forces, h->d_forces.get(), sizeof(float) * h->kp.out_cols * batch)) return r;
  if (status)
    if (int r = stream_d2h(h, status, h->d_status.get(), batch)) return r;
  if (iters)
    if (int r = stream_d2h(h, iters, h->d_iters.get(), sizeof(int32_t) * batch)) return r;
  return stream_sync(h);
}

// what both evaluate entry points ask of their arguments; `partial`: the entry point's own end of
// the text for a handle that keeps fewer than N output steps
static int evaluate_check(const char* who, const cmpc_batch* h, int batch, const void* records, const void* forces,
                          const void* xpred, const void* cert, const char* partial) {
  if (!h || !batch_ok(h, batch) || (batch && (!records || !forces))) return bad_arguments(who);
  if (!xpred && !cert) {
    g_last_error = std::string(who) + ": both outputs are NULL";
    return -1;
  }
  if (h->kp.out_cols != 12 * h->prm.horizon) {
    g_last_error = std::string(who) + ": the handle keeps fewer than N output steps" + partial;
    return -3;
  }
  return 0;
}

extern "C" int cmpc_batch_evaluate(cmpc_batch* h, const float* d_records, const float* d_forces, int batch,
                                   float* d_xpred, double* d_cert) {
  if (int r = evaluate_check("cmpc_batch_evaluate", h, batch, d_records, d_forces, d_xpred, d_cert,
                             ", its forces are not a full solution"))
    return r;
  return checked("launch_evaluate",
                 cmpc::launch_evaluate(d_records, d_forces, batch, h->kp, (double)h->prm.alpha, h->model.inertia,
                                       d_xpred, d_cert, h->stream, h->d_inst_rows.get()));
}

extern "C" int cmpc_batch_evaluate_host(cmpc_batch* h, const float* records, const float* forces, int batch,
                                        float* xpred, double* cert) {
  if (int r = evaluate_check("cmpc_batch_evaluate_host", h, batch, records, forces, xpred, cert, "")) return r;
  if (batch == 0) return 0;
  if (int r = ensure_staging(h)) return r;
  hipError_t e;
  const size_t B = (size_t)h->max_batch;
  if (!h->d_xpred && (e = h->d_xpred.alloc(Stage::kForcesMax * B)) != hipSuccess) return fail("hipMalloc(x_pred)", e);
  if (!h->d_cert && (e = h->d_cert.alloc(CMPC_CERT_WORDS * B)) != hipSuccess) return fail("hipMalloc(cert)", e);
  const int N = h->prm.horizon;
  const size_t rw = (size_t)CMPC_REC_WORDS(N);
  float* d_rec = h->d_rec.get();
  float* d_forces = h->d_forces.get();
  if (int r = stream_h2d(h, d_rec, records, rw * batch * sizeof(float))) return r;
  if (int r = stream_h2d(h, d_forces, forces, sizeof(float) * 12 * N * batch)) return r;
  if (int r = cmpc_batch_evaluate(h, d_rec, d_forces, batch, xpred ? h->d_xpred.get() : nullptr,
                                  cert ? h->d_cert.get() : nullptr))
    return r;
  if (xpred)
    if (int r = stream_d2h(h, xpred, h->d_xpred.get(), sizeof(float) * 12 * N * batch)) return r;
  if (cert)
    if (int r = stream_d2h(h, cert, h->d_cert.get(), sizeof(double) * CMPC_CERT_WORDS * batch)) return r;
  return stream_sync(h);
}

// what both sensitivity entry points ask of their arguments: evaluate's checks, and act_tol
static int sensitivity_check(const char* who, const cmpc_batch* h, int batch, const void* records,
                             const void* forces, const void* gradf, double act_tol, const void* sens) {
  if (!sens) {
    g_last_error = std::string(who) + ": sens is NULL";
    return -1;
  }
  if (int r = evaluate_check(who, h, batch, records, forces, sens, sens, ", its forces are not a full solution"))
    return r;
  if (batch && !gradf) return bad_arguments(who);
  if (!std::isfinite(act_tol) || act_tol < 0.0) {
    g_last_error = std::string(who) + ": act_tol is negative or not finite";
    return -2;
  }
  return 0;
}

extern "C" int cmpc_batch_sensitivity(cmpc_batch* h, const float* d_records, const float* d_forces,
                                      const float* d_grad_forces, int batch, double act_tol, double* d_sens,
                                      double* d_dtraj, double* d_dg) {
  if (int r = sensitivity_check("cmpc_batch_sensitivity", h, batch, d_records, d_forces, d_grad_forces, act_tol,
                                d_sens))
    return r;
  return checked("launch_sensitivity",
                 cmpc::launch_sensitivity(d_records, d_forces, d_grad_forces, batch, h->kp, (double)h->prm.alpha,
                                          h->model.inertia, act_tol, d_sens, d_dtraj, d_dg, h->stream,
                                          h->d_inst_rows.get()));
}

extern "C" int cmpc_batch_sensitivity_host(cmpc_batch* h, const float* records, const float* forces,
                                           const float* grad_forces, int batch, double act_tol, double* sens,
                                           double* dtraj, double* dg) {
  if (int r = sensitivity_check("cmpc_batch_sensitivity_host", h, batch, records, forces, grad_forces, act_tol, sens))
    return r;
  if (batch == 0) return 0;
  if (int r = ensure_staging(h)) return r;
  hipError_t e;
  const size_t B = (size_t)h->max_batch;
  if (!h->d_gradf && (e = h->d_gradf.alloc(Stage::kForcesMax * B)) != hipSuccess) return fail("hipMalloc(grad_forces)", e);
  if (!h->d_sens && (e = h->d_sens.alloc(CMPC_SENS_WORDS * B)) != hipSuccess) return fail("hipMalloc(sens)", e);
  if (!h->d_dtraj && (e = h->d_dtraj.alloc(Stage::kForcesMax * B)) != hipSuccess) return fail("hipMalloc(dtraj)", e);
  if (!h->d_dg && (e = h->d_dg.alloc(Stage::kForcesMax * B)) != hipSuccess) return fail("hipMalloc(dg)", e);
  const int N = h->prm.horizon;
  const size_t rw = (size_t)CMPC_REC_WORDS(N), nf = (size_t)12 * N * batch;
  if (int r = stream_h2d(h, h->d_rec.get(), records, rw * batch * sizeof(float))) return r;
  if (int r = stream_h2d(h, h->d_forces.get(), forces, sizeof(float) * nf)) return r;
  if (int r = stream_h2d(h, h->d_gradf.get(), grad_forces, sizeof(float) * nf)) return r;
  if (int r = cmpc_batch_sensitivity(h, h->d_rec.get(), h->d_forces.get(), h->d_gradf.get(), batch, act_tol,
                                     h->d_sens.get(), dtraj ? h->d_dtraj.get() : nullptr,
                                     dg ? h->d_dg.get() : nullptr))
    return r;
  if (int r = stream_d2h(h, sens, h->d_sens.get(), sizeof(double) * CMPC_SENS_WORDS * batch)) return r;
  if (dtraj)
    if (int r = stream_d2h(h, dtraj, h->d_dtraj.get(), sizeof(double) * nf)) return r;
  if (dg)
    if (int r = stream_d2h(h, dg, h->d_dg.get(), sizeof(double) * nf)) return r;
  return stream_sync(h);
}

// what both gain entry points ask of their arguments: sensitivity's checks without its gradient
static int gain_check(const char* who, const cmpc_batch* h, int batch, const void* records, const void* forces,
                      double act_tol, const void* gain) {
  if (!gain) {
    g_last_error = std::string(who) + ": gain is NULL";
    return -1;
  }
  if (int r = evaluate_check(who, h, batch, records, forces, gain, gain, ", its forces are not a full solution"))
    return r;
  if (!std::isfinite(act_tol) || act_tol < 0.0) {
    g_last_error = std::string(who) + ": act_tol is negative or not finite";
    return -2;
  }
  return 0;
}

extern "C" int cmpc_batch_gain(cmpc_batch* h, const float* d_records, const float* d_forces, int batch,
                               double act_tol, double* d_gain) {
  if (int r = gain_check("cmpc_batch_gain", h, batch, d_records, d_forces, act_tol, d_gain)) return r;
  return checked("launch_gain",
                 cmpc::launch_gain(d_records, d_forces, batch, h->kp, (double)h->prm.alpha, h->model.inertia, act_tol,
                                   d_gain, h->stream, h->d_inst_rows.get()));
}

extern "C" int cmpc_batch_gain_host(cmpc_batch* h, const float* records, const float* forces, int batch,
                                    double act_tol, double* gain) {
  if (int r = gain_check("cmpc_batch_gain_host", h, batch, records, forces, act_tol, gain)) return r;
  if (batch == 0) return 0;
  if (int r = ensure_staging(h)) return r;
  hipError_t e;
  if (!h->d_gain && (e = h->d_gain.alloc(CMPC_GAIN_WORDS * (size_t)h->max_batch)) != hipSuccess)
    return fail("hipMalloc(gain)", e);
  const int N = h->prm.horizon;
  const size_t rw = (size_t)CMPC_REC_WORDS(N);
  if (int r = stream_h2d(h, h->d_rec.get(), records, rw * batch * sizeof(float))) return r;
  if (int r = stream_h2d(h, h->d_forces.get(), forces, sizeof(float) * 12 * N * batch)) return r;
  if (int r = cmpc_batch_gain(h, h->d_rec.get(), h->d_forces.get(), batch, act_tol, h->d_gain.get())) return r;
  if (int r = stream_d2h(h, gain, h->d_gain.get(), sizeof(double) * CMPC_GAIN_WORDS * batch)) return r;
  return stream_sync(h);
}

extern "C" int cmpc_batch_feedback(cmpc_batch* h, const float* d_records, const float* d_forces,
                                   const double* d_gain, const float* d_states, const uint8_t* d_due, int batch,
                                   float* d_u) {
  if (!h || !batch_ok(h, batch) || (batch && (!d_records || !d_forces || !d_gain || !d_states || !d_u)))
    return bad_arguments("cmpc_batch_feedback");
  if (reinterpret_cast<uintptr_t>(d_gain) % 16 != 0) {
    g_last_error = "cmpc_batch_feedback: d_gain is not 16-byte aligned";
    return -1;
  }
  return checked("launch_feedback", cmpc::launch_feedback(d_records, d_forces, d_gain, d_states, d_due, batch, h->kp,
                                                          d_u, h->stream));
}

// =============================================================================================
// Reference single-instance interface (convexMPC_interface.cpp + the solve_mpc globals).
// =============================================================================================
extern "C" {
// Defined by the reference's caller (ConvexMPCLocomotion.cpp:610; be2r_cmpc_unitree_node.cpp:6);
// weak here so the library also loads on its own. The host program's definitions win.
__attribute__((weak)) float f_ext[6] = {0, 0, 0, 0, 0, 0};
__attribute__((weak)) float simulation_time = 0.f;
// The solver's own globals (SolverMPC.h:72-74, SolverMPC.cpp:390-392; Eigen::Matrix<float,6,1>
// layout): the compensation force of the last call and its two smoothed copies
float f_est[6] = {0, 0, 0, 0, 0, 0};
float f_est_smoothed[6] = {0, 0, 0, 0, 0, 0};
float f_est_static[6] = {0, 0, 0, 0, 0, 0};
}

namespace {
struct SingleState {
  std::mutex mu;
  cmpc_params cfg{};              // problem_configuration (convexMPC_interface.cpp:10)
  bool configured = false;        // the last setup_problem asked for a horizon in 1..CMPC_MAX_HORIZON
  // update_data_t fields (convexMPC_interface.h:23-41)
  float p[3]{}, v[3]{}, q[4]{}, w[3]{}, r[12]{};
  float roll = 0, pitch = 0, yaw = 0, alpha = 0, x_drag = 0;
  float weights[12]{};
  std::vector<float> traj;
  std::vector<unsigned char> gait;
  int max_iterations = 0, use_jcqp = 0;
  cmpc_model model = kDefaultModel;  // cmpc_set_model: the next solve's model
  double rho = 0, sigma = 0, solver_alpha = 0, terminate = 0;
  // solve_mpc state
  std::vector<double> q_soln;
  int has_solved = 0;
  bool eval_ok = false;           // h->d_rec holds the record q_soln solves (cmpc_evaluate_last)
  cmpc_batch* h = nullptr;
  int h_horizon = -1;
  // periodic-disturbance estimator state (SolverMPC.cpp:390-398, 555-563, 688-798): histories,
  // count and fit on the device (cmpc_estimator.hip ring of the last 400 samples); f_est,
  // f_est_smoothed and f_est_static are the exported globals below
  DevBuf<float> d_est;
};
// (never destroyed, like the side-stream pool: its handle and estimator state live as long as the
// process, and nothing of the runtime's is freed while the process unloads it)
SingleState& g = *new SingleState();

// The estimator state of the single-instance ABI lives on the device (one CMPC_EST_WORDS slot,
// cmpc_estimator.hip): the same kernel as the batched config-5 path runs the reference's per-call
// estimator step (SolverMPC.cpp:688-798) ahead of the solve, so one implementation serves both.
int ensure_single_est(SingleState& s) {
  if (s.d_est) return 0;
  DevBuf<float> est;
  hipError_t e = est.alloc(CMPC_EST_WORDS);
  if (e == hipSuccess) e = hipMemset(est.get(), 0, CMPC_EST_WORDS * sizeof(float));
  if (e != hipSuccess) return fail("hipMalloc(estimator state)", e);
  s.d_est = std::move(est);
  return 0;
}

// One instance through condense + ADMM on the handle's stream; the record is already in h->d_rec
// (staged with the estimator step), host forces out.
int admm_device(cmpc_batch* h, int N, const cmpc_admm_settings& as, float* forces, uint8_t* st) {
  const size_t n = 12 * (size_t)N;
  float* d_rec = h->d_rec.get();
  float* dH = h->d_admm_H.get();
  float* dg = dH + n * n;
  if (int r = cmpc_batch_condense(h, d_rec, 1, dH, dg)) return r;
  if (int r = cmpc_batch_admm(h, d_rec, dH, dg, 1, &as, h->d_forces.get(), h->d_status.get(), nullptr)) return r;
  if (int r = stream_d2h(h, forces, h->d_forces.get(), n * sizeof(float))) return r;
  if (int r = stream_d2h(h, st, h->d_status.get(), 1)) return r;
  return stream_sync(h);
}

// One solve_mpc call (SolverMPC.cpp:566-1089) of the single-instance ABI on the batch-1 handle:
// one H2D of the record with (f_ext[3], simulation_time) behind it, the estimator step on the
// device (writes f_est(3) and the use-f_est flag into the device record), then exactly one
// solver kernel of the record's size class (single_round_trip) or, for use_jcqp, condense + ADMM;
// one D2H of forces, status word and f_est(3).
int solve_single_device(SingleState& s, const float* rec, int N, float* forces, uint8_t* st) {
  cmpc_batch* h = s.h;
  if (int r = ensure_staging(h)) return r;
  if (int r = ensure_single_est(s)) return r;
  // diff_history.push_back(f_ext(3)), time_history.push_back(simulation_time)  (SolverMPC.cpp:692, 698)
  const float extra[2] = {f_ext[3], simulation_time};
  const size_t fest = Stage::status_word(N) + 1;  // f_est(3), behind the status word
  if (s.use_jcqp == 1 || s.use_jcqp == 2) {
    // use_jcqp == 1 (SolverMPC.cpp:818-838, 1057-1062): ADMM over the full QP; use_jcqp == 2
    // (:984-1053): over the reduced one; any horizon (QPs beyond 120 variables keep M^-1 in a
    // global slab)
    cmpc_admm_settings as{s.max_iterations, s.rho, s.sigma, s.solver_alpha, s.terminate,
                          s.use_jcqp == 2 ? 1 : 0};
    if (int r = single_upload(h, rec, extra, 2, s.d_est.get())) return r;
    if (int r = admm_device(h, N, as, forces, st)) return r;
    const hipError_t e = hipMemcpy(&f_est[3], h->d_single_out.get() + fest, sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail("D2H", e);
    return 0;
  }
  const float* out = nullptr;
  if (int r = single_round_trip(h, rec, extra, 2, 1, s.d_est.get(), nullptr, &out)) return r;
  std::memcpy(forces, out, 12 * N * sizeof(float));
  std::memcpy(st, out + Stage::status_word(N), 1);
  std::memcpy(&f_est[3], out + fest, sizeof(float));
  return 0;
}

// the batch-1 handle of horizon N, with the model and the parameters of this call
int single_handle(SingleState& s, int N) {
  if (!s.h || s.h_horizon != N) {
    if (s.h) cmpc_batch_destroy(s.h);
    s.h = nullptr;
    if (int r = cmpc_batch_create(&s.h, &s.cfg, 1, nullptr)) return r;
    s.h_horizon = N;
  }
  if (std::memcmp(&s.model, &s.h->model, sizeof(s.model)) != 0)
    if (int r = cmpc_batch_set_model(s.h, &s.model)) return r;
  cmpc_params prm = s.cfg;
  for (int i = 0; i < 12; i++) prm.weights[i] = s.weights[i];
  prm.alpha = s.alpha;
  prm.max_iter = 100;  // nWSR = 100 (SolverMPC.cpp:854)
  if (std::memcmp(&prm, &s.h->prm, sizeof(prm)) != 0) return cmpc_batch_set_params(s.h, &prm);
  return 0;
}

void solve_single(SingleState& s) {
  const int N = s.cfg.horizon;
  s.eval_ok = false;
  if (N < 1 || N > CMPC_MAX_HORIZON) {
    std::fprintf(stderr, "[cmpc] horizon %d out of range\n", N);
    return;
  }

  // the record; f_est(3) and the use-f_est flag are written by the device estimator step
  std::vector<float> rec(CMPC_REC_WORDS(N), 0.f);
  std::memcpy(&rec[CMPC_REC_P], s.p, sizeof(s.p));
  std::memcpy(&rec[CMPC_REC_V], s.v, sizeof(s.v));
  std::memcpy(&rec[CMPC_REC_Q], s.q, sizeof(s.q));
  std::memcpy(&rec[CMPC_REC_W], s.w, sizeof(s.w));
  std::memcpy(&rec[CMPC_REC_R], s.r, sizeof(s.r));
  rec[CMPC_REC_RPY + 0] = s.roll;
  rec[CMPC_REC_RPY + 1] = s.pitch;
  rec[CMPC_REC_RPY + 2] = s.yaw;
  rec[CMPC_REC_XDRAG] = s.x_drag;
  std::memcpy(&rec[CMPC_REC_TRAJ(N)], s.traj.data(), sizeof(float) * 12 * N);
  std::memcpy(&rec[CMPC_REC_GAIT(N)], s.gait.data(), 4 * N);

  std::vector<float> forces(12 * N);
  uint8_t st = 0;
  if (single_handle(s, N) != 0 || solve_single_device(s, rec.data(), N, forces.data(), &st) != 0) {
    std::fprintf(stderr, "[cmpc] %s\n", cmpc_last_error());
    return;
  }
  // SolverMPC.cpp:783, 798 (f_est itself came back with the forces)
  for (int i = 0; i < 6; i++) f_est_smoothed[i] = 0.95f * f_est_smoothed[i] + 0.05f * f_est[i];
  f_est_static[3] = 0.97f * f_est_static[3] + 0.03f * f_ext[3];
  const bool admm = (s.use_jcqp == 1 || s.use_jcqp == 2);
  // a failed qpOASES-equivalent solve prints as the reference does (SolverMPC.cpp:965-968) and
  // stores what the kernel wrote for it (zeros for every force); a failed ADMM
  // solve keeps the previous solution. The reference keeps JCQP's solution whatever its residual
  // (status 0 or 1).
  if (admm ? (st != 0 && st != 1) : (st != CMPC_OK)) {
    std::printf("failed to solve!\n");
    if (admm) return;
  }
  s.q_soln.assign(12 * N, 0.0);
  for (int i = 0; i < 12 * N; i++) s.q_soln[i] = forces[i];
  s.has_solved = 1;
  s.eval_ok = true;
}
}  // namespace

extern "C" void setup_problem(double dt, int horizon, double mu, double f_max) {
  std::lock_guard<std::mutex> lk(g.mu);
  g.cfg.dt = (float)dt;
  g.cfg.horizon = horizon;
  g.cfg.mu = (float)mu;
  g.cfg.f_max = (float)f_max;
  // resize_qp_mats (SolverMPC.cpp:149-250). The staging holds the largest horizon the solver
  // admits, whatever is asked here, so no later copy depends on this call's horizon.
  g.traj.assign(12 * CMPC_MAX_HORIZON, 0.f);
  g.gait.assign(4 * CMPC_MAX_HORIZON, 0);
  g.configured = horizon >= 1 && horizon <= CMPC_MAX_HORIZON;
  if (!g.configured)
    // the reference throws from c2qp above 19 (SolverMPC.cpp:113-116) on the next solve; here
    // every update_problem_data* call refuses until a valid setup_problem and get_solution keeps
    // returning the previous solution
    std::fprintf(stderr, "[cmpc] setup_problem: horizon %d outside 1..%d; solves are refused and "
                 "the previous solution is kept\n", horizon, CMPC_MAX_HORIZON);
  else if (horizon > 19)
    std::fprintf(stderr, "[cmpc] horizon %d > 19: reference c2qp would throw; cap lifted\n", horizon);
}

namespace {
// update_problem_data* before a valid setup_problem: nothing is copied (the staging holds
// CMPC_MAX_HORIZON steps) and nothing is solved
bool refuse_update(const char* who) {
  if (g.configured) return false;
  std::fprintf(stderr, "[cmpc] %s: horizon %d not configured (setup_problem with 1..%d first); "
               "previous solution kept\n", who, g.cfg.horizon, CMPC_MAX_HORIZON);
  return true;
}
}  // namespace

extern "C" void update_solver_settings(int max_iter, double rho, double sigma, double solver_alpha,
                                       double terminate, double use_jcqp) {
  std::lock_guard<std::mutex> lk(g.mu);
  g.max_iterations = max_iter;
  g.rho = rho;
  g.sigma = sigma;
  g.solver_alpha = solver_alpha;
  g.terminate = terminate;
  g.use_jcqp = use_jcqp > 1.5 ? 2 : (use_jcqp > 0.5 ? 1 : 0);
  // use_jcqp == 1 / 2 run the ADMM kernel (full / reduced QP)
}

extern "C" int cmpc_set_model(const cmpc_model* m) {
  const cmpc_model nm = m ? *m : kDefaultModel;
  if (!model_ok(nm)) {
    g_last_error = "cmpc_set_model: mass and inertia must be finite and positive";
    return -2;
  }
  std::lock_guard<std::mutex> lk(g.mu);
  g.model = nm;  // the handle gets it in the next update_problem_data* call (solve_single)
  return 0;
}

extern "C" void update_problem_data_floats(float* p, float* v, float* q, float* w, float* r, float roll,
                                           float pitch, float yaw, float* weights, float* state_trajectory,
                                           float alpha, int* gait) {
  std::lock_guard<std::mutex> lk(g.mu);
  if (refuse_update("update_problem_data_floats")) return;
  const int N = g.cfg.horizon;
  g.alpha = alpha;
  g.roll = roll;
  g.pitch = pitch;
  g.yaw = yaw;
  for (int i = 0; i < 4 * N; i++) g.gait[i] = (unsigned char)gait[i];  // mint_to_u8
  std::memcpy(g.p, p, sizeof(float) * 3);
  std::memcpy(g.v, v, sizeof(float) * 3);
  std::memcpy(g.q, q, sizeof(float) * 4);
  std::memcpy(g.w, w, sizeof(float) * 3);
  std::memcpy(g.r, r, sizeof(float) * 12);
  std::memcpy(g.weights, weights, sizeof(float) * 12);
  std::memcpy(g.traj.data(), state_trajectory, sizeof(float) * 12 * N);
  solve_single(g);
}

extern "C" void update_problem_data(double* p, double* v, double* q, double* w, double* r, double yaw,
                                    double* weights, double* state_trajectory, double alpha, int* gait) {
  std::lock_guard<std::mutex> lk(g.mu);
  if (refuse_update("update_problem_data")) return;
  const int N = g.cfg.horizon;
  for (int i = 0; i < 3; i++) { g.p[i] = (float)p[i]; g.v[i] = (float)v[i]; g.w[i] = (float)w[i]; }
  for (int i = 0; i < 4; i++) g.q[i] = (float)q[i];
  for (int i = 0; i < 12; i++) { g.r[i] = (float)r[i]; g.weights[i] = (float)weights[i]; }
  g.yaw = (float)yaw;
  for (int i = 0; i < 12 * N; i++) g.traj[i] = (float)state_trajectory[i];
  g.alpha = (float)alpha;
  for (int i = 0; i < 4 * N; i++) g.gait[i] = (unsigned char)gait[i];
  solve_single(g);
}

void update_x_drag(float x_drag) {
  std::lock_guard<std::mutex> lk(g.mu);
  g.x_drag = x_drag;
}

// The record and the forces of the last update_problem_data* call, for cmpc_evaluate_last,
// cmpc_sensitivity_last and cmpc_gain_last (g.mu held): 0, or a negative error with its text set
static int last_solve(const char* who, std::vector<float>& rec, std::vector<float>& forces) {
  if (!g.has_solved || !g.eval_ok || !g.h) {
    g_last_error = std::string(who) + ": no solved update_problem_data* call to evaluate";
    return -4;
  }
  // the record as the solve read it (f_est(3) and its flag written by the device estimator step)
  // is still in the handle's staging; the forces are q_soln, which get_solution returns
  const int N = g.h_horizon;
  if ((int)g.q_soln.size() != 12 * N) {
    g_last_error = std::string(who) + ": the last solution is of another horizon";
    return -4;
  }
  rec.resize(CMPC_REC_WORDS(N));
  forces.resize(12 * N);
  hipError_t e = hipStreamSynchronize(g.h->stream);
  if (e == hipSuccess) e = hipMemcpy(rec.data(), g.h->d_rec.get(), rec.size() * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail("D2H", e);
  for (int i = 0; i < 12 * N; i++) forces[i] = (float)g.q_soln[i];
  return 0;
}

extern "C" int cmpc_evaluate_last(float* x_pred, double* cert) {
  std::lock_guard<std::mutex> lk(g.mu);
  std::vector<float> rec, forces;
  if (int r = last_solve("cmpc_evaluate_last", rec, forces)) return r;
  return cmpc_batch_evaluate_host(g.h, rec.data(), forces.data(), 1, x_pred, cert);
}

extern "C" int cmpc_sensitivity_last(const float* grad_forces, double act_tol, double* sens, double* dtraj,
                                     double* dg) {
  std::lock_guard<std::mutex> lk(g.mu);
  std::vector<float> rec, forces;
  if (int r = last_solve("cmpc_sensitivity_last", rec, forces)) return r;
  return cmpc_batch_sensitivity_host(g.h, rec.data(), forces.data(), grad_forces, 1, act_tol, sens, dtraj, dg);
}

extern "C" int cmpc_gain_last(double act_tol, double* gain) {
  std::lock_guard<std::mutex> lk(g.mu);
  std::vector<float> rec, forces;
  if (int r = last_solve("cmpc_gain_last", rec, forces)) return r;
  return cmpc_batch_gain_host(g.h, rec.data(), forces.data(), 1, act_tol, gain);
}

extern "C" double get_solution(int index) {
  std::lock_guard<std::mutex> lk(g.mu);
  if (!g.has_solved) return 0.f;
  // the reference reads q_soln[index] unchecked (convexMPC_interface.cpp:156-162); past the last
  // solve's 12N values this returns 0
  if (index < 0 || (size_t)index >= g.q_soln.size()) return 0.0;
  return g.q_soln[index];
}
