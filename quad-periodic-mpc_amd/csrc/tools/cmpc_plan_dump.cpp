// cmpc_plan_dump: the launch plan of one batched solve (cmpc_plan.h), one line per decision, in the
// order launch_solve issues it. Plain C++: no HIP, no library (tests/test_launch_plan.py).
//   cmpc_plan_dump N refine batch due [hint ints ...]   hint: the kHdr ints of a solve's header
//   cmpc_plan_dump classes n_max   size_class(n, ...) for n = 0..n_max, every (c1_max, c1_listed, tail)
//   cmpc_plan_dump builds           the rows of kWideBuild (cmpc_wide_builds.h)
//   cmpc_plan_dump select           the build a launch takes, for every (wide class, form, refine, mdl_default)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../cmpc_plan.h"

using namespace cmpc;

static int dump_classes(int n_max) {
  for (int c1_max = 60; c1_max <= 64; c1_max += 4)
    for (int listed = 0; listed < 2; listed++)
      for (int tail = 0; tail < 2; tail++) {
        printf("c1_max=%d c1_listed=%d tail=%d:", c1_max, listed, tail);
        for (int n = 0; n <= n_max; n++) printf(" %d", size_class(n, c1_max, listed != 0, tail != 0));
        printf("\n");
      }
  return 0;
}

static void print_build(const WideBuild& b) {
  printf("w%d form=%s refine=%d literal=%d\n", b.nv, b.persistent ? "persistent" : "one_per_entry", b.refine,
         b.literal);
}

static int dump_builds() {
  for (const WideBuild& b : kWideBuild) print_build(b);
  return 0;
}

static int dump_select() {
  for (int c = kW80; c <= kW256; c++)
    for (int persistent = 0; persistent < 2; persistent++)
      for (int refine = 0; refine < 2; refine++)
        for (int dflt = 0; dflt < 2; dflt++) {
          const int row = select_wide_build(kClass[c].width, persistent != 0, refine != 0, dflt != 0);
          printf("w%d want=%s refine=%d mdl_default=%d -> ", kClass[c].width,
                 persistent ? "persistent" : "one_per_entry", refine, dflt);
          if (row < 0) {
            printf("none\n");
            return 1;
          }
          print_build(kWideBuild[row]);
        }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "classes")) return dump_classes(atoi(argv[2]));
  if (argc == 2 && !strcmp(argv[1], "builds")) return dump_builds();
  if (argc == 2 && !strcmp(argv[1], "select")) return dump_select();
  if (argc != 5 && argc != 5 + kHdr) {
    fprintf(stderr, "usage: %s N refine batch due [%d hint ints] | %s classes n_max | %s builds | %s select\n", argv[0],
            kHdr, argv[0], argv[0], argv[0]);
    return 2;
  }
  const int N = atoi(argv[1]), refine = atoi(argv[2]), batch = atoi(argv[3]), due = atoi(argv[4]);
  int hint[kHdr];
  for (int j = 0; j < kHdr && argc > 5; j++) hint[j] = atoi(argv[5 + j]);
  const SolvePlan p = plan_solve(N, refine != 0, batch, due != 0, argc > 5 ? hint : nullptr, PlanKnobs());
  const bool on_side = p.classify == kClassifyOnSide0;
  const char* handle_wait = on_side ? "classified" : "none";

  printf("sides %d\n", p.nsides);
  if (p.classify == kClassifyNone) {
    printf("classify none\n");
  } else {
    printf("classify stream=%s fork=%d due=%d c1_max=%d c1_listed=%d tail=%d\n", on_side ? "side0" : "handle",
           on_side ? 1 : 0, due != 0, p.c1_width, p.c1_list ? 1 : 0, p.tail != kTailNone);
    for (int s = on_side ? 1 : 0; s < p.nsides; s++) printf("wait side%d classified\n", s);
  }
  auto tail = [&](const char* stream, const char* wait) {
    printf("tail stream=%s wait=%s list=%d grid=%d rest=%d\n", stream, wait, kClass[kTail].list, p.tail_grid,
           p.tail_rest);
    printf("handoff stream=%s list=%d width=%d form=persistent grid=%d\n", stream, kClass[kHandoff].list,
           kClass[kHandoff].width, kHandoffGrid);
  };
  if (p.tail == kTailOnSide2) tail("side2", "none");
  if (p.c1_build64)
    printf("c1_build64 stream=side1 width=%d list=%d grid=%d\n", kClass[kC1Wide].width, kClass[kC1Wide].list, batch);
  for (int j = 0; j < p.nwide; j++) {
    const WideLaunch& w = p.wide[j];
    printf("wide w%d stream=side%d list=%d form=%s grid=%d rest=%d rest_base=%d\n", kClass[w.cls].width, w.side,
           kClass[w.cls].list, w.persistent ? "persistent" : "one_per_entry", w.grid, w.rest_grid, w.rest_base);
  }
  if (p.c1_list)
    printf("class1 stream=handle wait=%s width=%d over=list%d grid=%d\n", handle_wait, p.c1_width, kClass[kC1].list,
           batch);
  else
    printf("class1 stream=handle wait=none width=%d over=batch grid=%d\n", p.c1_width, batch);
  if (p.tail == kTailBehindC1) tail("handle", handle_wait);
  printf("joins %d\n", p.nsides);
  return 0;
}
