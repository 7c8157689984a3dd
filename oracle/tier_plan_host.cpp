// tier_plan_host.cpp -- the library's tier policy (cassierl_amd/csrc/cassie_tier_plan.h) on the CPU: a stand-alone program that answers
// queries read from standard input, one line each (tests/test_tier_plan_host.py; `make tier_plan_host` builds it with ASan + UBSan):
//   plan <n_envs> <simds> <flags> <g16> <leg> <duo>   ->  "<n_envs> <simds> <flags> <g16> <leg> <duo> -> <g16> <leg> <duo_envs>"
//                                                         (overrides: what CASSIE2D_G16 / _LEG / _DUO say, -1 = unset)
//   seg2d <n_sub> <max_segments>                      ->  "seg2d <n_sub> <max_segments> -> <len> <len> ..."
//   seg3d <n_sub> <segments>                          ->  "seg3d <n_sub> <segments> -> <len> <len> ..."
#include <stdio.h>
#include <string.h>

#include "../cassierl_amd/csrc/cassie_tier_plan.h"

int main() {
  char line[256], what[16];
  while (fgets(line, sizeof line, stdin)) {
    int a[6];
    const int got = sscanf(line, "%15s %d %d %d %d %d %d", what, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]);
    if (got == 7 && !strcmp(what, "plan") && a[0] > 0 && a[1] > 0) {
      cassie::plan::TierOverrides env;
      env.g16 = a[3]; env.leg = a[4]; env.duo = a[5];
      const cassie::plan::TierPlan t = cassie::plan::plan_tiers(a[0], a[1], a[2], env);
      printf("%d %d %d %d %d %d -> %d %d %d\n", a[0], a[1], a[2], a[3], a[4], a[5], (int)t.g16, (int)t.leg, t.duo_envs);
    } else if (got == 3 && (!strcmp(what, "seg2d") || !strcmp(what, "seg3d")) && a[0] > 0 && a[1] > 0 && a[1] <= 16) {
      int len[16];
      const int n = what[3] == '2' ? cassie::plan::segment_lengths_2d(a[0], a[1], len) : cassie::plan::segment_lengths_3d(a[0], a[1], len);
      printf("%s %d %d ->", what, a[0], a[1]);
      for (int j = 0; j < n; j++) printf(" %d", len[j]);
      printf("\n");
    } else {
      fprintf(stderr, "tier_plan_host: bad query: %s", line);
      return 2;
    }
  }
  return 0;
}
