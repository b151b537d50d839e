// cmpc_wide_builds.h — the one statement of which builds of the wide kernel template (cmpc_wide.h)
// exist, and of which build a launch takes. No HIP here (cmpc_plan.h includes it; the host compiler
// alone checks the selector: tools/cmpc_plan_dump.cpp, tests/test_launch_plan.py).
//   * build.py reads the rows below and compiles cmpc_wide_unit.hip once per row, each build in a
//     translation unit of its own: compiled side by side, the kernels spilled registers;
//   * cmpc_launch.hip's launch_wide builds its launcher table from the same rows;
//   * plan_solve (cmpc_plan.h) asks wide_has_form whether a class has a one-per-entry build.
#pragma once

namespace cmpc {

// One build: cmpc_solve_w_kernel<nv, persistent, refine, literal> and, in the builds that read
// the model (literal = false), its per-instance twin cmpc_solve_w_inst_kernel<nv, persistent, refine>.
//   persistent: workgroups dequeue list entries until the list is exhausted; else one workgroup per
//     possible list entry (cmpc_wide.h: the two launch forms);
//   refine: with the fp64 refinement step of the converged active set (wide_refine; horizons
//     N > 10). A refining build skips the step when KParams::refine is 0;
//   literal: the default robot's model (m = 12, I_body = diag(.07, .26, .242)) as literals in place
//     of the kernel's model argument, so the default pays nothing for the parameter. Built for the
//     refining 96- and 120-column classes (N = 16 and N = 20 trot, the measured workloads).
struct WideBuild {
  int nv;
  bool persistent, refine, literal;
};

// clang-format off
constexpr WideBuild kWideBuild[] = {
    // 80 columns: 94 VGPRs, no spills; config 3's n 65-80 instances finish inside class 1's run.
    // The persistent loop costs the build 11 spilled VGPRs (96: 20, 128: 4), hence both forms
    {80, 0, 0, 0}, {80, 1, 0, 0}, {80, 0, 1, 0}, {80, 1, 1, 0},
    // 96 columns: 96 VGPRs, no spills (N = 16 trot, the reference's deployed horizon: every
    // instance n = 96)
    {96, 0, 0, 0}, {96, 1, 0, 0}, {96, 0, 1, 0}, {96, 1, 1, 0}, {96, 0, 1, 1}, {96, 1, 1, 1},
    // 120 columns (n 97-120: every trot instance at N = 20, n = 120; the 128-column build keeps
    // n 121-128): 118 VGPRs and 34 KB of LDS (the stage buffers share P's tail), four four-wave
    // workgroups per CU
    {120, 0, 0, 0}, {120, 1, 0, 0}, {120, 0, 1, 0}, {120, 1, 1, 0}, {120, 0, 1, 1}, {120, 1, 1, 1},
    // 128 columns: 124 VGPRs and 38 KB of LDS, four four-wave workgroups per CU. From here on the
    // refining build alone: it serves the horizons N <= 10 with KParams::refine = 0
    {128, 0, 1, 0}, {128, 1, 1, 0},
    // 144 columns (n 129-144: random contact tables at N = 20), 192, 256: persistent only (no
    // spills from the loop at their occupancy; sparse classes, whose one-per-entry grids drain up
    // to `batch` empty workgroups: 3.5 ms for the one-per-CU 146-KB workgroups of the 256 class at
    // config 5). A launch that wants one workgroup per entry runs the loop once (null dequeue
    // counter: workgroup i takes entry i)
    {144, 1, 1, 0}, {192, 1, 1, 0}, {256, 1, 1, 0},
};
// clang-format on
constexpr int kNumWideBuilds = sizeof(kWideBuild) / sizeof(kWideBuild[0]);

// Waves per SIMD the builds of a width are compiled for (__launch_bounds__): a function of the
// width alone. Five up to 96 columns (94 / 96 VGPRs without spills). Four from 120 to 144; at 144
// that is 128 VGPRs with 42 spilled and 51 KB of LDS (R^-1 kept for 40 active-set positions, not
// 64): three five-wave workgroups per CU where three waves per SIMD (167 VGPRs, no spills) and
// 56 KB admitted two, config 5 4.33 M -> 4.73 M QP/s (same-box A/B r04_c5). Three above.
constexpr int wide_waves(int nv) { return nv <= 96 ? 5 : nv <= 144 ? 4 : 3; }

// s_setprio of a build's waves: 1 exactly in the builds without refinement (N <= 10, where the wide
// classes share their SIMDs with class 1's waves: issue priority over them measured config 2
// +1.9 %, config 3 +0.2 %, r04_p); the default priority 0 in the refining builds.
constexpr int wide_prio(bool refine) { return refine ? 0 : 1; }

// the row of a build in kWideBuild, or -1 when it is not built
constexpr int wide_build_row(WideBuild b) {
  for (int i = 0; i < kNumWideBuilds; i++)
    if (kWideBuild[i].nv == b.nv && kWideBuild[i].persistent == b.persistent && kWideBuild[i].refine == b.refine &&
        kWideBuild[i].literal == b.literal)
      return i;
  return -1;
}

// whether a width has a build of this launch form at all
constexpr bool wide_has_form(int nv, bool persistent) {
  for (int i = 0; i < kNumWideBuilds; i++)
    if (kWideBuild[i].nv == nv && kWideBuild[i].persistent == persistent) return true;
  return false;
}

// The row a launch of the nv-column class takes, given the launch form it wants, KParams::refine
// and KParams::mdl_default: the exact build if there is one, else the nearest one that computes the
// same, giving up in turn
//   the literal model (the model-reading build reads the same values from its argument),
//   the unrefined build (a refining build skips the step when KParams::refine is 0),
//   the one-per-entry form (the persistent build with a null dequeue counter runs its loop once).
// -1: no build of that width.
constexpr int select_wide_build(int nv, bool persistent, bool refine, bool mdl_default) {
  const WideBuild tries[] = {{nv, persistent, refine, refine && mdl_default},
                             {nv, persistent, refine, false},
                             {nv, persistent, true, false},
                             {nv, true, true, false}};
  for (const WideBuild& t : tries)
    if (const int row = wide_build_row(t); row >= 0) return row;
  return -1;
}

}  // namespace cmpc
