// Prints prefill_plan's decisions (csrc/gvl_prefill_plan.h, host-only) for geometries that carry the `score` flag: built with the host C++ compiler by
// tests/test_prefill_score_plan_cpu.py.  One case per line, tests/c/prefill_plan_dump.cc's "P" line with one more field at its end:
//   P nb lens[0..8) pos0[0..8) rope_orig_max_pos long_table loss page_id_cap hidden qkv_width gate_up_width fused_weights varlen_attn varlen_extend last_layer_tail norm_fused score
//     -> the refusal (-1 .. -5)  or  "M batched_table nf tail last_rows n_chunks chunks.. n_steps" then per step "kind form first count B S pos0 Sk use_long", then " | off[0..nb]"
// With the argument "reasons": the refusal messages, one "-k message" per line.
#include <cstdio>
#include <cstring>
#include "gvl_prefill_plan.h"

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "reasons")) {
    for (int rc = -1; rc >= -5; --rc) printf("%d %s\n", rc, prefill_refusal_reason(rc));
    return 0;
  }
  char kind;
  while (scanf(" %c", &kind) == 1) {
    if (kind != 'P') return 2;
    PrefillGeometry g{};
    PrefillKnobs k{};
    int ok = scanf("%d", &g.nb) == 1, b[7];
    for (int& v : g.lens) ok &= scanf("%d", &v) == 1;
    for (int& v : g.pos0) ok &= scanf("%d", &v) == 1;
    ok &= scanf("%d %d %d %d %d %d %d %d", &g.rope_orig_max_pos, &b[0], &b[1], &g.page_id_cap, &g.hidden, &g.qkv_width, &g.gate_up_width, &b[2]) == 8;
    ok &= scanf("%d %d %d %d %d", &k.varlen_attn, &b[3], &b[4], &b[5], &b[6]) == 5;
    if (!ok) return 2;
    g.long_table = b[0]; g.loss = b[1]; g.fused_weights = b[2]; k.varlen_extend = b[3]; k.last_layer_tail = b[4]; k.norm_fused = b[5]; g.score = b[6];
    PrefillPlan p;
    const int rc = prefill_plan(g, k, &p);
    if (rc) { printf("%d\n", rc); continue; }
    printf("%d %d %d %d %d %d", p.M, p.batched_table, p.nf, p.tail, p.last_rows, p.n_chunks);
    for (int i = 0; i < p.n_chunks; ++i) printf(" %d", p.chunks[i]);
    printf(" %d", p.n_steps);
    for (int i = 0; i < p.n_steps; ++i) {
      const PrefillStep& s = p.steps[i];
      printf(" %d %d %d %d %d %d %d %d %d", s.kind, s.form, s.first, s.count, s.B, s.S, s.pos0, s.Sk, s.use_long);
    }
    printf(" |");
    for (int i = 0; i <= g.nb; ++i) printf(" %d", p.off[i]);
    printf("\n");
  }
  return 0;
}
