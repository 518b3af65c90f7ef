// Prints the decisions of attn_ext_plan (csrc/gvl_attn_plan.h, host-only) for the cases on stdin: built with the host C++ compiler by tests/test_attn_ext_plan_cpu.py.
// One case per line:
//   H KV D Dout causal vl_n vl_rows[0..8] vl_pos0[0..7] vl_tables O16 lazy          vl_tables: bit u = table of sequence u
//     -> "-1"  or  "D NWAVES NS grid block lds lazy"
// With the argument "list": GVL_ATTN_EXT_LIST instead, one "D NWAVES NS" per line.
#include <cstdio>
#include <cstring>
#include "gvl_attn_plan.h"

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "list")) {
#define P3(D, NW, NS) printf("%d %d %d\n", D, NW, NS);
    GVL_ATTN_EXT_LIST(P3)
    return 0;
  }
  for (;;) {
    AttnExtGeometry g{};
    int tables, o16, ok = 1;
    float lazy;
    if (scanf("%d", &g.H) != 1) return 0;
    int* f[] = {&g.KV, &g.D, &g.Dout, &g.causal, &g.vl_n};
    for (int* p : f) ok &= scanf("%d", p) == 1;
    for (int& r : g.vl_rows) ok &= scanf("%d", &r) == 1;
    for (int& r : g.vl_pos0) ok &= scanf("%d", &r) == 1;
    ok &= scanf("%d %d %f", &tables, &o16, &lazy) == 3;
    if (!ok) return 2;
    for (int u = 0; u < GVL_MAX_PREFILL_BATCH; ++u) g.vl_tables[u] = tables >> u & 1;
    g.O16 = o16 != 0;
    AttnExtLaunch l;
    if (attn_ext_plan(g, AttnKnobs{lazy, false}, &l) < 0) { printf("-1\n"); continue; }
    printf("%d %d %d %u %d %d %.9g\n", l.D, l.NWAVES, l.NS, l.grid, l.block, l.lds, (double)l.lazy);
  }
}
