// cmpc_launch.hip — orchestration of the size classes for one batch solve.
//   plan (cmpc_plan.h, no HIP): the table of the size classes and plan_solve, which decides what
//     launch_solve below issues: which class on which stream, in what order, with what grid;
//   classify (this file): n = 3 x stance foot-steps per instance (SolverMPC.cpp:869-894), the
//     instances with n > 64 appended to the list of their class;
//   class 1 (cmpc_class1.hip): every instance, one wavefront each; exits when n > 64;
//   wide classes (cmpc_wide.h: two lanes per row, NV/32 wavefronts; NV = 80, 96, 120, 128, 144,
//     192, 256; n <= 12 N <= 240 at CMPC_MAX_HORIZON = 20; their builds: the table of
//     cmpc_wide_builds.h, chosen by launch_wide below) each over its own list, on two side
//     streams forked after classify, so they run concurrently with class 1 and with each
//     other. At N = 10 they are a latency-bound tail (few, long solves); at N = 16..20 the 128-
//     and 192-column classes carry the batch and run side by side on the two streams.
//   due form (cmpc_batch_solve_due): the classify pass lists only the due instances and every
//     class, class 1 included, runs over its list.
#include <stdlib.h>

#include <utility>

#include "cmpc_kernels.h"

namespace cmpc {

namespace {

// one thread per instance; wave-aggregated appends to the class lists. One-wave workgroups: beside
// class 1 (whose one-wave workgroups take every wave slot as it frees) a 4-wave workgroup waited
// for four free slots at once, and the pass took 1.0 ms instead of 0.05
// DUE (cmpc_batch_solve_due): a thread whose instance is not due classifies nothing and reads no
// record word; cnt[kHdrBatch] counts the due instances and cnt[kHdrCall] holds the whole batch. The
// unmasked kernel below is the DUE = false body under its unchanged name.
// INST (a handle with a per-instance table): instance i's own f_max, from its table entry.
template <bool DUE, bool INST = false>
__device__ __forceinline__ void classify_body(const float* __restrict__ recs, const uint8_t* __restrict__ due,
                                              int batch, const KParams& P, int* __restrict__ cnt,
                                              int* __restrict__ lists, int max_batch, int c1_max,
                                              int* __restrict__ next_hdr, int c1_listed, int tail,
                                              int* __restrict__ host_hint) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  if (blockIdx.x == 0 && threadIdx.x < kHdr) {
    // the next solve's counters: before zeroing them, the previous solve's final counts (the
    // header alternates) go to the host-mapped hint buffer (launch_solve sizes later grids by them)
    if (host_hint) host_hint[threadIdx.x] = next_hdr[threadIdx.x];
    next_hdr[threadIdx.x] = 0;
  }
  if (!DUE && blockIdx.x == 0 && threadIdx.x == 0) cnt[kHdrBatch] = batch;  // this solve's batch: the hint's scale
  if (DUE && blockIdx.x == 0 && threadIdx.x == 0) cnt[kHdrCall] = batch;
  int cls = -1;
  const bool mine = i < batch && (!DUE || due[i] != 0);
  if (DUE) {  // the hint's scale of a due solve: the instances it solves (the header starts at zero)
    const unsigned long long nd = __ballot(mine);
    if (lane == 0 && nd) atomicAdd(&cnt[kHdrBatch], __popcll(nd));
  }
  if (mine) {
    const uint32_t* g =
        reinterpret_cast<const uint32_t*>(recs + (size_t)i * P.rec_words + CMPC_REC_GAIT(P.N));
    int nfs = 0;
    float f_max = P.f_max;
    if constexpr (INST) f_max = P.inst[i].f_max;
    for (int k = 0; k < P.N; k++) {
      const uint32_t w = g[k];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        // eliminated iff |gait * f_max| < 0.01, exactly as the solver kernels test it
        const float ub = (float)((w >> (8 * j)) & 0xffu) * f_max;
        nfs += (ub < 0.01f && ub > -0.01f) ? 0 : 1;
      }
    }
    cls = size_class(3 * nfs, c1_max, c1_listed != 0, tail != 0);
  }
  const unsigned long long any = __ballot(cls >= 0);
  if (any == 0ull) return;
  const unsigned long long wide = __ballot(cls >= 0 && cls != kClass[kC1].list);  // cnt[0]: n above class 1's build
  if (lane == 0 && wide) atomicAdd(&cnt[0], __popcll(wide));
#pragma unroll
  for (int c = 0; c < kLists; c++) {
    const unsigned long long m = __ballot(cls == c);
    if (m == 0ull) continue;
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&cnt[1 + c], __popcll(m));
    base = __shfl(base, leader);
    if (cls == c) lists[(size_t)c * max_batch + base + __popcll(m & ((1ull << lane) - 1ull))] = i;
  }
}

__global__ __launch_bounds__(64) void cmpc_classify_kernel(const float* __restrict__ recs, int batch,
                                                           KParams P, int* __restrict__ cnt,
                                                           int* __restrict__ lists, int max_batch,
                                                           int c1_max, int* __restrict__ next_hdr,
                                                           int c1_listed, int tail,
                                                           int* __restrict__ host_hint) {
  classify_body<false>(recs, nullptr, batch, P, cnt, lists, max_batch, c1_max, next_hdr, c1_listed, tail,
                       host_hint);
}

__global__ __launch_bounds__(64) void cmpc_classify_due_kernel(const float* __restrict__ recs,
                                                               const uint8_t* __restrict__ due, int batch,
                                                               KParams P, int* __restrict__ cnt,
                                                               int* __restrict__ lists, int max_batch,
                                                               int c1_max, int* __restrict__ next_hdr,
                                                               int tail, int* __restrict__ host_hint) {
  classify_body<true>(recs, due, batch, P, cnt, lists, max_batch, c1_max, next_hdr, 1, tail, host_hint);
}

// the two kernels above for a handle with a per-instance table (kernels of their own names: the
// shared ones keep theirs and their registers)
__global__ __launch_bounds__(64) void cmpc_classify_inst_kernel(const float* __restrict__ recs, int batch,
                                                                KParams P, int* __restrict__ cnt,
                                                                int* __restrict__ lists, int max_batch,
                                                                int c1_max, int* __restrict__ next_hdr,
                                                                int c1_listed, int tail,
                                                                int* __restrict__ host_hint) {
  classify_body<false, true>(recs, nullptr, batch, P, cnt, lists, max_batch, c1_max, next_hdr, c1_listed, tail,
                             host_hint);
}

__global__ __launch_bounds__(64) void cmpc_classify_due_inst_kernel(const float* __restrict__ recs,
                                                                    const uint8_t* __restrict__ due, int batch,
                                                                    KParams P, int* __restrict__ cnt,
                                                                    int* __restrict__ lists, int max_batch,
                                                                    int c1_max, int* __restrict__ next_hdr,
                                                                    int tail, int* __restrict__ host_hint) {
  classify_body<true, true>(recs, due, batch, P, cnt, lists, max_batch, c1_max, next_hdr, 1, tail, host_hint);
}

// the kept placement knobs (cmpc_plan.h), read once
const PlanKnobs& plan_knobs() {
  static const PlanKnobs k = [] {
    PlanKnobs k;
    k.split60_min = diag_knob("CMPC_SPLIT60_MIN", k.split60_min);
    k.classify_side = diag_knob("CMPC_CLASSIFY_SIDE", k.classify_side);
    k.t8_pos = diag_knob("CMPC_T8_POS", k.t8_pos);
    k.tail = diag_knob("CMPC_TAIL", k.tail);
    k.hint = diag_knob("CMPC_HINT", k.hint);
    k.hint_min = diag_knob("CMPC_HINT_MIN", k.hint_min);
    k.wide_form = diag_knob("CMPC_WIDE_FORM", k.wide_form);
    k.pop_f_hi = diag_knob("CMPC_POP_F_HI", k.pop_f_hi);
    k.w120_side = diag_knob("CMPC_W120_SIDE", k.w120_side);
    k.sparse_side = diag_knob("CMPC_SPARSE_SIDE", k.sparse_side);
    return k;
  }();
  return k;
}

// One launch of wide class cls (kW80 .. kW256) in the launch form wanted: the build that
// select_wide_build (cmpc_wide_builds.h) picks for the form, P.refine and P.mdl_default, through a
// table of the launchers of kWideBuild's rows in row order. A class without a one-per-entry build
// gets its persistent one; with c.deq == nullptr that runs its loop once per workgroup.
template <size_t... I>
hipError_t launch_wide_row(int row, const KParams& P, const WideCall& c, std::index_sequence<I...>) {
  using Fn = hipError_t (*)(const KParams&, const WideCall&);
  static constexpr Fn kFn[] = {&launch_wide_build<kWideBuild[I].nv, kWideBuild[I].persistent, kWideBuild[I].refine,
                                                  kWideBuild[I].literal>...};
  return kFn[row](P, c);
}
hipError_t launch_wide(int cls, bool persistent, const KParams& P, const WideCall& c) {
  const int row = select_wide_build(kClass[cls].width, persistent, P.refine != 0, P.mdl_default != 0);
  if (row < 0) return hipErrorInvalidValue;
  return launch_wide_row(row, P, c, std::make_index_sequence<kNumWideBuilds>());
}

}  // namespace

hipError_t launch_solve(const float* d_recs, int batch, const KParams& P, float* d_forces,
                        uint8_t* d_status, int32_t* d_iters, int* d_work, int max_batch,
                        hipStream_t stream, LaunchCtx& ctx, hipEvent_t* ev, const uint8_t* d_due) {
  // The due form (d_due, cmpc_batch_solve_due): the classify pass (its due
  // instantiation) first on the handle's stream at every horizon, class 1 behind it over list 5
  // (and list 7 on side 1 where the 60 / 64 split applies), the tail and wide classes over their
  // lists on the side streams as in the unmasked sequence.
  const bool due = d_due != nullptr;
  // a handle with a per-instance table: the classify kernels that read each instance's own f_max
  // (every solver launcher below picks its per-instance build by P.inst itself)
  const auto classify_k = P.inst ? cmpc_classify_inst_kernel : cmpc_classify_kernel;
  const auto classify_due_k = P.inst ? cmpc_classify_due_inst_kernel : cmpc_classify_due_kernel;
  int* cnt = d_work + ctx.hdr * kHdr;             // zero: zeroed at create or by the last classify
  int* next_hdr = d_work + (ctx.hdr ^ 1) * kHdr;  // the next solve's, zeroed by this one's classify
  int* list[kLists];
  for (int j = 0; j < kLists; j++) list[j] = d_work + 2 * kHdr + (size_t)j * max_batch;
  hipError_t e = hipSuccess;
  if (batch <= 0) {  // keep the timing slots consistent (zero-length launches)
    if (ev)
      for (int i = 0; i < 3; i++) (void)hipEventRecord(ev[i], stream);
    return hipSuccess;
  }
  // the class counts of an earlier solve (the classify kernel copies a finished solve's header to
  // the host-mapped ctx.h_hint, no host wait), read once
  int hint[kHdr];
  if (ctx.h_hint) {
    const volatile int* h = ctx.h_hint;
    for (int j = 0; j < kHdr; j++) hint[j] = h[j];
  }
  const SolvePlan plan = plan_solve(P.N, P.refine != 0, batch, due, ctx.h_hint ? hint : nullptr, plan_knobs());
  const int has_tail = plan.tail != kTailNone ? 1 : 0;
  hipStream_t classify_s = plan.classify == kClassifyOnSide0 ? ctx.side[0] : stream;
  auto classify = [&]() -> hipError_t {
    if (due)
      hipLaunchKernelGGL(classify_due_k, dim3((batch + 63) / 64), dim3(64), 0, classify_s, d_recs, d_due, batch, P,
                         cnt, d_work + 2 * kHdr, max_batch, plan.c1_width, next_hdr, has_tail, ctx.d_hint);
    else
      hipLaunchKernelGGL(classify_k, dim3((batch + 63) / 64), dim3(64), 0, classify_s, d_recs, batch, P, cnt,
                         d_work + 2 * kHdr, max_batch, plan.c1_width, next_hdr, plan.c1_list ? 1 : 0, has_tail,
                         ctx.d_hint);
    const hipError_t r = hipGetLastError();
    if (r == hipSuccess) {
      ctx.last_hdr = ctx.hdr;
      ctx.hdr ^= 1;
    }
    return r;
  };
  auto class1 = [&](int width, int lst, int grid, hipStream_t s) -> hipError_t {
    return launch_class1(width, d_recs, batch, P, d_forces, d_status, d_iters, lst >= 0 ? list[lst] : nullptr,
                         lst >= 0 ? &cnt[1 + lst] : nullptr, nullptr, nullptr, grid, s);
  };
  // the tail class and, behind it on its stream, its hand-offs (list 10): a one-workgroup persistent
  // launch of the 80-column class (it reads the final count once the tail class is done)
  auto tail = [&](hipStream_t s) -> hipError_t {
    constexpr int lt = kClass[kTail].list, lh = kClass[kHandoff].list;
    const hipError_t r = launch_tail(d_recs, P, d_forces, d_status, d_iters, list[lt], &cnt[1 + lt], list[lh],
                                     &cnt[1 + lh], plan.tail_grid, s, plan.tail_rest);
    if (r != hipSuccess) return r;
    return launch_wide(kW80, true, P,
                       {d_recs, d_forces, d_status, d_iters, list[lh], &cnt[1 + lh], &cnt[kDeq + lh], kHandoffGrid, s, 0});
  };
  auto wide = [&](const WideLaunch& w) -> hipError_t {
    const int l = kClass[w.cls].list;
    hipStream_t s = ctx.side[w.side];
    const hipError_t r = launch_wide(w.cls, w.persistent, P,
                                     {d_recs, d_forces, d_status, d_iters, list[l], &cnt[1 + l],
                                      w.persistent ? &cnt[kDeq + l] : nullptr, w.grid, s, 0});
    if (r != hipSuccess || w.rest_grid == 0) return r;
    // the looping launch behind a one-per-entry launch of a predicted grid: the entries from rest_base on
    return launch_wide(w.cls, true, P,
                       {d_recs, d_forces, d_status, d_iters, list[l], &cnt[1 + l], &cnt[kDeq + l], w.rest_grid, s,
                        w.rest_base});
  };

  if (plan.nsides == 0 && plan.classify != kClassifyNone) {
    // the due form at the horizons whose unmasked solve needs no classify pass (every n <= 60): it
    // lists the due instances (all in list 5) and class 1 runs over that list; no side stream is used
    if ((e = classify()) != hipSuccess) return e;
    if (ev) (void)hipEventRecord(ev[0], stream);
    if ((e = class1(plan.c1_width, kClass[kC1].list, batch, stream)) != hipSuccess) return e;
    if (ev) {
      (void)hipEventRecord(ev[1], stream);
      (void)hipEventRecord(ev[2], stream);
    }
    return hipSuccess;
  }
  const bool on_side = plan.classify == kClassifyOnSide0;  // then the handle's stream waits for the lists too
  if (plan.classify != kClassifyNone) {
    if (on_side) {
      if ((e = hipEventRecord(ctx.fork, stream)) != hipSuccess) return e;
      if ((e = hipStreamWaitEvent(ctx.side[0], ctx.fork, 0)) != hipSuccess) return e;
    }
    if ((e = classify()) != hipSuccess) return e;
    if ((e = hipEventRecord(ctx.classified, classify_s)) != hipSuccess) return e;
    for (int s = on_side ? 1 : 0; s < plan.nsides; s++)
      if ((e = hipStreamWaitEvent(ctx.side[s], ctx.classified, 0)) != hipSuccess) return e;
    if (plan.tail == kTailOnSide2 && (e = tail(ctx.side[2])) != hipSuccess) return e;
    if (plan.c1_build64 &&
        (e = class1(kClass[kC1Wide].width, kClass[kC1Wide].list, batch, ctx.side[1])) != hipSuccess)
      return e;
    for (int j = 0; j < plan.nwide; j++)
      if ((e = wide(plan.wide[j])) != hipSuccess) return e;
  }
  if (ev) (void)hipEventRecord(ev[0], stream);
  if (plan.c1_list) {
    // class 1 over the classify list of n <= its row width (one workgroup per possible entry,
    // surplus ones exit after reading the count): behind the classify pass
    if (on_side && (e = hipStreamWaitEvent(stream, ctx.classified, 0)) != hipSuccess) return e;
    e = class1(plan.c1_width, kClass[kC1].list, batch, stream);
  } else {
    // over the whole batch: it skips the instances above its row width itself
    e = class1(plan.c1_width, -1, batch, stream);
  }
  if (e != hipSuccess) return e;
  if (plan.tail == kTailBehindC1) {
    if (on_side && (e = hipStreamWaitEvent(stream, ctx.classified, 0)) != hipSuccess) return e;
    if ((e = tail(stream)) != hipSuccess) return e;
  }
  if (ev) (void)hipEventRecord(ev[1], stream);
  for (int s = 0; s < plan.nsides; s++) {
    if ((e = hipEventRecord(ctx.join[s], ctx.side[s])) != hipSuccess) return e;
    if ((e = hipStreamWaitEvent(stream, ctx.join[s], 0)) != hipSuccess) return e;
  }
  if (ev) (void)hipEventRecord(ev[2], stream);
  return hipSuccess;
}

// One instance whose reduced size n the caller already knows (counted on the host from the
// record's gait table, the same test as the classify pass): exactly one kernel of the right
// class, no classify pass, no side-stream fork/join. d_one = {1, 0}: a one-entry instance list.
hipError_t launch_single(const float* d_rec, int n, const KParams& P, float* d_forces,
                         uint8_t* d_status, int32_t* d_iters, const int* d_one, hipStream_t stream,
                         bool allow_tail) {
  const int* cnt = d_one;
  const int* lst = d_one + 1;
  if (n <= kClass[kC1Wide].hi)
    return launch_class1(n <= kClass[kC1].hi ? kClass[kC1].width : kClass[kC1Wide].width, d_rec, 1, P, d_forces,
                         d_status, d_iters, nullptr, nullptr, nullptr, nullptr, 1, stream);
  const PlanKnobs& knobs = plan_knobs();
  const bool in_tail = knobs.tail != 0 && tail_class(P.refine != 0, P.N, n);
  if (allow_tail && in_tail)
    return launch_tail(d_rec, P, d_forces, d_status, d_iters, lst, cnt, nullptr, nullptr, 1, stream);
  const WideCall one{d_rec, d_forces, d_status, d_iters, lst, cnt, nullptr, 1, stream, 0};
  if (!allow_tail && in_tail)  // a tail-class hand-off: the form the batched launch uses
    return launch_wide(kW80, true, P, one);
  // the launch form the batched launch of this class would pick for a batch of one (one workgroup
  // per entry; the persistent form runs its loop once with deq == nullptr). Both forms round
  // alike (-ffp-contract=on, build.py): tests/test_gpu_parity.py::test_batch_size_invariance
  // solves the same records in a batch of 16384 (persistent sparse classes), in batches of 4096
  // and one at a time and requires bitwise-equal forces
  const int c = wide_class(n);
  return launch_wide(c, !one_per_entry(kClass[c], P.N, 1, knobs), P, one);
}

}  // namespace cmpc
