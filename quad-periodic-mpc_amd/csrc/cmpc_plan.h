// cmpc_plan.h — what one batched solve launches, decided apart from the launching: the table of the
// size classes, the placement knobs still worth re-measuring, and plan_solve, a pure function from
// (horizon, refinement, batch, due form, class counts of an earlier solve) to the launch sequence
// that launch_solve (cmpc_launch.hip) issues. No HIP here: the header compiles with a plain C++17
// compiler, so the placement is checked on a CPU (tools/cmpc_plan_dump.cpp, tests/test_launch_plan.py).
#pragma once
#include <math.h>

#include "cmpc_wide_builds.h"

#if defined(__HIPCC__)
#define CMPC_HD __host__ __device__
#else
#define CMPC_HD
#endif

namespace cmpc {

// The work buffer's header (cmpc_kernels.h: d_work): cnt[0] the instances above class 1's build,
// cnt[1 + list] the lengths of the class lists, cnt[kDeq + list] the persistent wide workgroups'
// dequeue counters.
constexpr int kLists = 11;
constexpr int kHdr = 32;
constexpr int kDeq = 16;  // cnt[kDeq + list]: dequeue counter of a persistent class's workgroups
constexpr int kHdrBatch = 31;  // cnt[kHdrBatch]: the batch of the solve that counted into the header
                               // (a due-masked solve: the number of due instances it counted)
constexpr int kHdrCall = 30;   // cnt[kHdrCall]: a due-masked solve's whole batch (0: an unmasked solve)
static_assert(1 + kLists <= kDeq && kDeq + kLists <= kHdrCall && kHdrCall < kHdrBatch && kHdrBatch < kHdr,
              "list lengths, dequeue counters and the batch tag fit the header");

// ---- the size classes: the one statement of which reduced sizes n = 3 x stance foot-steps go to
// which kernel family and classify list.
enum SizeClassId {
  kC1 = 0,   // class 1 (cmpc_class1.hip), one wavefront per instance: the 60-wide build, or with
             // c1_max = 64 the 64-wide build for every n <= 64. List 5 where class 1 runs over a list
  kC1Wide,   // class 1's 64-wide build beside the 60-wide one (60 < n <= 64)
  kTail,     // the tail class (cmpc_tail.hip): 8 tail rows beside class 1's 64, N <= 10 unrefined
  kHandoff,  // tail-class instances whose active set outgrew 64 positions: to the 80-column class
  kW80, kW96, kW120, kW128, kW144, kW192, kW256,  // the wide classes (cmpc_wide.h), by row width
  kNumClasses
};
struct SizeClass {
  int list;    // its classify list (d_work)
  int width;   // rows of its build
  int lo, hi;  // the reduced sizes it holds
};
constexpr SizeClass kClass[kNumClasses] = {
    {5, 60, 0, 60},       // kC1
    {7, 64, 61, 64},      // kC1Wide
    {9, 72, 65, 72},      // kTail
    {10, 80, 65, 72},     // kHandoff
    {0, 80, 65, 80},      // kW80
    {1, 96, 81, 96},      // kW96
    {8, 120, 97, 120},    // kW120
    {2, 128, 121, 128},   // kW128
    {6, 144, 129, 144},   // kW144
    {3, 192, 145, 192},   // kW192
    {4, 256, 193, 256},   // kW256 (n <= 12 N <= 240 at CMPC_MAX_HORIZON = 20)
};

// the wide class of n > 64 (host side: the single-instance path)
inline int wide_class(int n) {
  for (int c = kW80; c < kW256; c++)
    if (n <= kClass[c].hi) return c;
  return kW256;
}

// the reduced sizes the tail class takes from the 80-column wide class: 64 < n <= 72 at N <= 10
// (the horizons without the fp64 refinement of the wide classes; with the refinement switched
// off, cmpc_batch_set_refine(0), the longer horizons keep the 80-column class, whose parity the
// refine-off tests cover)
CMPC_HD inline bool tail_class(bool refine, int N, int n) {
  return !refine && N <= 10 && n >= kClass[kTail].lo && n <= kClass[kTail].hi;
}

// the list of the wide class of n > 64. The class is a template argument so that the classify
// kernels get the table's entries as the literals of a compare chain: a table indexed at run time
// is a load from constant memory in device code
template <int C>
CMPC_HD inline int wide_list(int n) {
  if constexpr (C == kW256)
    return kClass[C].list;
  else
    return n <= kClass[C].hi ? kClass[C].list : wide_list<C + 1>(n);
}

// The classify list of reduced size n, or -1 for none (class 1 over the whole batch skips the
// instances above its row width itself).
// c1_max: class 1's row width (60 with the 64-wide build beside it, else 64);
// c1_listed: class 1 runs over list 5 instead of the whole batch;
// tail: the tail class (list 9) takes its sizes from the 80-column class (list 0).
CMPC_HD inline int size_class(int n, int c1_max, bool c1_listed, bool tail) {
  if (n <= c1_max) return c1_listed ? kClass[kC1].list : -1;
  if (n <= kClass[kC1Wide].hi) return kClass[kC1Wide].list;
  if (tail && n >= kClass[kTail].lo && n <= kClass[kTail].hi) return kClass[kTail].list;
  return wide_list<kW80>(n);
}

// ---- the placement knobs (A/B switches of DESIGN.md §4.1 that a later measurement may revisit;
// read from the environment in a diagnostic build only, cmpc_kernels.h diag_knob). The defaults are
// the measured choices.
struct PlanKnobs {
  int split60_min = 16384;  // CMPC_SPLIT60_MIN: the smallest batch that gets class 1 as two builds
  int classify_side = -1;   // CMPC_CLASSIFY_SIDE: 0 / 1 the classify pass on the handle's stream / side 0
  int t8_pos = -1;          // CMPC_T8_POS: 1 / 2 the tail class behind class 1 / on side 2
  int tail = 1;             // CMPC_TAIL: 0 the 80-column class for every 64 < n <= 80
  int hint = 1;             // CMPC_HINT: 0 no hinted grids
  int hint_min = 16384;     // CMPC_HINT_MIN: the smallest batch whose grids are hinted
  int wide_form = 0;        // CMPC_WIDE_FORM: 1 every wide class one-per-entry, 2 every class persistent
  int pop_f_hi = 100;       // CMPC_POP_F_HI: the populous half-width from N = 11, percent of a std. dev.
  int w120_side = -1;       // CMPC_W120_SIDE: 0 / 1 the side stream of the 120-column class
  int sparse_side = 1;      // CMPC_SPARSE_SIDE: the sides of the 144 / 192 classes as two digits
};

// Launch form of a wide class with both builds (cmpc_wide_builds.h): one workgroup per list entry for the
// populous classes, persistent workgroups for the sparse ones. Populous: the class meets
// 6N +- 3 sqrt(N), the trot size (two feet in stance at every step) +- one standard deviation of n
// = 3 Bin(4N, 1/2) under random contact tables. Measured (profiles/r03_ab/r03_e): every class
// one-per-entry lost config 5 2 % to the drains of the sparse classes; every class persistent
// lost config 3 / 2 2-6 % to the spills of the 80-column persistent build. Below 16384 instances
// (the same threshold as class 1's split) the drains are short and every class is one-per-entry
// (config 2: 11.3 M -> 11.7 M QP/s).
// (Round 4: only the class holding 6 N itself one-per-entry measured -0.3 % at config 3; the same
// with the 80 class kept one-per-entry at N <= 10, i.e. the 128 class persistent at N = 20 and
// the 120 class at N = 16, -1.0 % at config 5, +0.3 % at N = 16, profiles/r04_ab/r04_t*.)
inline bool one_per_entry(const SizeClass& c, int N, int batch, const PlanKnobs& k) {
  if (k.wide_form == 1 || batch < 16384) return true;
  if (k.wide_form == 2) return false;
  const float f = (N > 10) ? 0.01f * (float)k.pop_f_hi : 1.f;
  const float mode = 6.f * (float)N, half = f * 3.f * sqrtf((float)N);
  return (float)c.hi >= mode - half && (float)c.lo <= mode + half;
}

// workgroups of the 80-column class's persistent launch over the tail class's hand-offs (an
// active set past 64 positions: none in any measured workload; one workgroup solves them in turn)
constexpr int kHandoffGrid = 1;
// workgroups of the looping launch behind a one-per-entry launch of a predicted grid (entries past
// the prediction; none when it held)
constexpr int kRestGrid = 32;

// ---- the plan of one solve
enum ClassifyAt { kClassifyNone = 0, kClassifyOnHandle, kClassifyOnSide0 };
enum TailAt { kTailNone = 0, kTailOnSide2, kTailBehindC1 };
struct WideLaunch {
  int cls;          // kW80 .. kW256
  int side;         // its side stream
  bool persistent;  // persistent workgroups over a dequeue counter, else one workgroup per entry
  int grid;
  int rest_grid;    // one-per-entry over a predicted grid: the looping launch behind it over the
  int rest_base;    // entries from rest_base on; 0: none
};
struct SolvePlan {
  int c1_width = 64;     // class 1's rows: 60 or 64
  bool c1_list = false;  // class 1 over list 5 (behind the classify pass), else over the whole batch
  int classify = kClassifyNone;
  bool c1_build64 = false;  // the 64-wide class-1 build over list 7, first on side 1
  int tail = kTailNone;
  int tail_grid = 0, tail_rest = 0;  // the tail class's grid and the grid of its looping rest launch
  int nsides = 0;        // side streams that wait for the lists and are joined at the end
  int nwide = 0;
  WideLaunch wide[kNumClasses - kW80];  // in launch order
};

// hint: the kHdr ints of a finished solve's header as a classify pass copied them to the host
// (LaunchCtx::h_hint), or null.
inline SolvePlan plan_solve(int N, bool refine, int batch, bool due, const int* hint, const PlanKnobs& k) {
  SolvePlan p;
  const int n_max = 12 * N;  // a class no instance of this horizon can reach is not launched
  // Class 1 as two builds — 60-wide rows over the whole batch (n <= 60) and 64-wide rows over the
  // classify list of 60 < n <= 64 — once the batch fills the GPU (config 3: 28.4 M -> 29.3 M
  // QP/s). Below that the step is latency-bound and the extra kernel lengthens a side-stream
  // chain (config 2, batch 4096: 11.2 M -> 9.9 M), so one 64-wide launch takes all n <= 64.
  const bool split60 = batch >= k.split60_min;
  p.c1_width = (n_max <= kClass[kC1Wide].hi || split60) ? kClass[kC1].width : kClass[kC1Wide].width;
  // from N = 11 the trot size 6N is above class 1's rows and few instances reach class 1: it runs
  // over a classify list (list 5) instead of the whole batch (config 5: 65536 record stagings and
  // exits per step, 84 MB). The due form lists the due instances at every horizon.
  p.c1_list = 6 * N > kClass[kC1Wide].hi || due;
  if (n_max <= kClass[kC1Wide].hi) {  // every instance in class 1: a classify pass for the due form only
    p.classify = due ? kClassifyOnHandle : kClassifyNone;
    return p;
  }
  // The tail class takes 64 < n <= 72 at N <= 10 whatever the batch size (so a record gets the
  // same kernel, and the same forces, in any batch). Its placement depends on the batch (measured
  // on config-3 mixes, profiles/r05_j, r05_k; against the 80-column class for every n <= 80: 4096
  // -0.7 %, 16384 -4 %, 32768 -1.5 %, 65536 +4.4 %, 262144 +7 %): on the handle's stream behind
  // class 1, alone on the GPU once class 1 drains, from 131072 instances (+7 % at 262144 where
  // beside class 1 gave +3 %); below, first on a side stream of its own (side 2) beside class 1.
  if (k.tail != 0 && tail_class(refine, N, kClass[kTail].lo))
    p.tail = (k.t8_pos == 1 || k.t8_pos == 2) ? (k.t8_pos == 1 ? kTailBehindC1 : kTailOnSide2)
                                              : (batch >= 131072 ? kTailBehindC1 : kTailOnSide2);
  p.nsides = p.tail == kTailOnSide2 ? 3 : 2;  // the third only for the tail class's own chain
  // From 16384 instances (and up to 4096) the classify pass runs on side 0 beside class 1 (which
  // needs no list up to N = 10), the other sides waiting for the lists; in between, on the
  // handle's stream ahead of everything. Round-3 batch sweep (profiles/r03_ab/sweep2): beside
  // class 1 +2 % at 16384 .. 131072 instances. Round-4 sweep (profiles/r04_ab/r04_ks, beside vs
  // ahead): 2048 +2.3 %, 4096 (config 2) +3.2 %, 6144 0, 8192 -2 %, 12288 -1.5 %: beside at the
  // smallest batches too, where class 1 starting without the classify pass's queue hop ahead of
  // it pays most. The due form: on the handle's stream, where class 1, which waits for its list,
  // follows it in the same queue.
  const bool cls_side = due ? false
                            : (k.classify_side < 0) ? (batch >= 16384 || batch <= 4096) : (k.classify_side == 1);
  p.classify = cls_side ? kClassifyOnSide0 : kClassifyOnHandle;
  p.c1_build64 = split60;
  // Grids from the class counts of an earlier solve, from 16384 instances: scaled to this batch
  // with a quarter and 64 workgroups of slack they size the wide classes' and the tail class's
  // grids. A class launched one workgroup per possible entry ends only when its empty workgroups
  // have drained, and at mid-size batches those wait for SIMD slots behind class 1: at 32768
  // instances the tail class and the 96 class ended 0.12-0.18 ms after class 1 (profiles/r06_p).
  // The persistent forms dequeue any count, so a hinted grid only bounds their workgroups; a
  // one-per-entry launch over the predicted entries is followed on its stream by a small looping
  // launch over any entries past them, which exits at once when the prediction held. A class
  // carrying the batch predicts more than the batch and keeps a batch-sized grid. Below 16384
  // instances the drains are short and the grids stay batch-sized (a hint there measured +-0.3 %,
  // profiles/r06_hint2).
  // A due solve leaves the number of due instances in cnt[kHdrBatch], so the scaling stays a
  // fraction of the solved instances for whichever form comes next, and its whole batch in
  // cnt[kHdrCall]. The host does not know how many instances are due now, so a due solve scales a
  // due solve's counts by the whole batches instead (the same due fraction as the hinted solve, as
  // a staggered loop has tick after tick), and an unmasked solve's counts as if all were due.
  if (!(k.hint && batch >= k.hint_min)) hint = nullptr;
  const int hint_batch = hint ? hint[kHdrBatch] : 0;
  const bool hinting = hint_batch > 0;  // then entries past a predicted grid are possible
  const int hint_call = (due && hinting) ? hint[kHdrCall] : 0;
  const double hint_den = hint_call > 0 ? (double)hint_call : (double)hint_batch;
  auto grid_of = [&](int list) -> int {
    if (!hinting) return batch;
    const double g = (double)hint[1 + list] * (double)batch / hint_den * 1.25 + 64.0;
    return g < (double)batch ? (int)g : batch;
  };
  if (p.tail != kTailNone) {
    p.tail_grid = grid_of(kClass[kTail].list);
    p.tail_rest = hinting && p.tail_grid < batch ? kRestGrid : 0;
  }
  // The wide classes this horizon can reach, in launch order. Side 0: 80, 120, 144, 256; side 1
  // (behind the 64-wide class-1 build: side 0 carries the 80 class, the longest chain at N = 10):
  // 96, 128, 192.
  // The 120-column class (97..120) runs on side 0 from N = 14 (every trot instance at N = 17..20,
  // beside the 96-column trot class at N = 14..16; at N = 20, where it carries the batch, beside
  // the 128-column class). Below, where it is almost always empty (all-stance tables only), on
  // side 1 behind the sparse 96 class: on side 0 its launch lengthens the 80 class's chain, the
  // step's critical path (config 3 timeline, profiles/r04_prof).
  // The 144 class on side 0 behind the 120 class, the 192 class on side 1 behind the 128 class: at
  // N = 20 the two sparse classes then start as soon as either bulk class drains and run side by
  // side instead of back to back. Config 5 4.21 M -> 4.41 M QP/s against both on side 1
  // (profiles/r03_ab/sparse_side).
  const int w120_side = (k.w120_side >= 0) ? (k.w120_side & 1) : (6 * N <= 80 ? 1 : 0);
  const int side_of[] = {0, 1, w120_side, 1, (k.sparse_side / 10) & 1, k.sparse_side % 10 & 1, 0};
  for (int c = kW80; c <= kW256 && n_max >= kClass[c].lo; c++) {
    WideLaunch& w = p.wide[p.nwide++];
    w.cls = c;
    w.side = side_of[c - kW80];
    // (a class built persistent only is launched persistent whatever its population)
    w.persistent = !wide_has_form(kClass[c].width, false) || !one_per_entry(kClass[c], N, batch, k);
    w.grid = grid_of(kClass[c].list);
    const bool rest = !w.persistent && hinting && w.grid < batch;
    w.rest_grid = rest ? kRestGrid : 0;
    w.rest_base = rest ? w.grid : 0;
  }
  return p;
}

}  // namespace cmpc
