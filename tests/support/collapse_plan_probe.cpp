// collapse_plan_probe — test infrastructure (tests/test_collapse_plan_cpu.py): the route plan and the hand-over table of
// tiebrush_amd/csrc/collapse_plan.hpp as a plain program, without HIP.
//   collapse_plan_probe grid AXIS=v,v,.. (all twelve axes, any order of values)
//       the plan of every point of the product, the axes in the order of AXES below, the first one slowest; one line per point:
//       route part use_runs runs_min lean arena_lean   (arena_lean: collapse_arena_lean for a tile on the device)
//   collapse_plan_probe after     (stdin: lines "route part use_runs runs_min lean err_bits")
//       one line per input line: action route part use_runs runs_min lean raw_handed_back big_bucket
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../tiebrush_amd/csrc/collapse_plan.hpp"

static const char* AXES[12] = {"n", "cig", "k", "tbm", "prio", "carried", "strategy", "store_frac", "collapse_same", "path", "raw", "sort"};

static CollapsePlanIn point(const long long* v) {
  CollapsePlanIn in;
  in.n_records = (uint32_t)v[0];
  in.n_cigar_ops = (uint32_t)v[1];
  in.n_files = (uint32_t)v[2];
  in.tbm_none = v[3] == 0;  // tbm: 0 none of the files, 1 some, 2 all
  in.tbm_any = v[3] != 0;
  in.tbm_all = v[3] == 2;
  in.has_prio = v[4] != 0;
  in.has_carried = v[5] != 0;
  in.strategy = (int)v[6];
  in.store_frac = (int)v[7];
  in.collapse_same = (int)v[8];
  in.path = (int)v[9];
  in.raw = (int)v[10];
  in.sort = (int)v[11];
  return in;
}

static int grid(int argc, char** argv) {
  std::vector<long long> axis[12];
  for (int a = 0; a < argc; ++a) {
    const char* eq = strchr(argv[a], '=');
    int which = -1;
    for (int i = 0; i < 12 && eq; ++i)
      if (strlen(AXES[i]) == (size_t)(eq - argv[a]) && !strncmp(AXES[i], argv[a], eq - argv[a])) which = i;
    if (which < 0) return fprintf(stderr, "unknown axis: %s\n", argv[a]), 2;
    for (const char* p = eq + 1; *p;) {
      char* end;
      axis[which].push_back(strtoll(p, &end, 10));
      if (end == p) return fprintf(stderr, "bad value: %s\n", argv[a]), 2;
      p = *end == ',' ? end + 1 : end;
    }
  }
  for (int i = 0; i < 12; ++i)
    if (axis[i].empty()) return fprintf(stderr, "axis %s has no value\n", AXES[i]), 2;
  size_t at[12] = {0};
  for (;;) {
    long long v[12];
    for (int i = 0; i < 12; ++i) v[i] = axis[i][at[i]];
    const CollapsePlanIn in = point(v);
    const CollapsePlan p = collapse_plan(in);
    printf("%d %d %d %u %d %d\n", p.route, (int)p.part, (int)p.use_runs, p.runs_min, (int)p.lean, (int)collapse_arena_lean(in, p, true));
    int i = 11;
    while (i >= 0 && ++at[i] == axis[i].size()) at[i--] = 0;
    if (i < 0) return 0;
  }
}

static int after() {
  int route, part, use_runs, lean;
  unsigned runs_min, eb;
  while (scanf("%d %d %d %u %d %u", &route, &part, &use_runs, &runs_min, &lean, &eb) == 6) {
    CollapsePlan p;
    p.route = route, p.part = part != 0, p.use_runs = use_runs != 0, p.runs_min = runs_min, p.lean = lean != 0;
    const CollapseNext r = collapse_plan_after(p, eb);
    printf("%d %d %d %d %u %d %d %d\n", r.action, r.plan.route, (int)r.plan.part, (int)r.plan.use_runs, r.plan.runs_min, (int)r.plan.lean,
           (int)r.raw_handed_back, (int)r.big_bucket);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "grid")) return grid(argc - 2, argv + 2);
  if (argc == 2 && !strcmp(argv[1], "after")) return after();
  fprintf(stderr, "usage: collapse_plan_probe grid AXIS=v,v,.. | after\n");
  return 2;
}
