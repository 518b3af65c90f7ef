// Prints the decisions of csrc/gvl_prefill_plan.h (host-only) for the cases on stdin: built with the host C++ compiler by tests/prefill_plan.py.
// One case per line, the first word says which function:
//   P nb lens[0..8) pos0[0..8) rope_orig_max_pos long_table loss page_id_cap hidden qkv_width gate_up_width fused_weights varlen_attn varlen_extend last_layer_tail norm_fused
//     -> the refusal (-1 .. -4)  or  "M batched_table nf tail last_rows n_chunks chunks.. n_steps" then per step "kind form first count B S pos0 Sk use_long"
//   G left cap max_rows lens[0..left)
//     -> the group's size
// With the argument "reasons": the refusal messages instead, one "-k message" per line.
#include <cstdio>
#include <cstring>
#include "gvl_prefill_plan.h"

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "reasons")) {
    for (int rc = -1; rc >= -4; --rc) printf("%d %s\n", rc, prefill_refusal_reason(rc));
    return 0;
  }
  char kind;
  while (scanf(" %c", &kind) == 1) {
    if (kind == 'P') {
      PrefillGeometry g{};
      PrefillKnobs k{};
      int ok = scanf("%d", &g.nb) == 1, b[8];
      for (int& v : g.lens) ok &= scanf("%d", &v) == 1;
      for (int& v : g.pos0) ok &= scanf("%d", &v) == 1;
      ok &= scanf("%d %d %d %d %d %d %d %d", &g.rope_orig_max_pos, &b[0], &b[1], &g.page_id_cap, &g.hidden, &g.qkv_width, &g.gate_up_width, &b[2]) == 8;
      ok &= scanf("%d %d %d %d", &k.varlen_attn, &b[3], &b[4], &b[5]) == 4;
      if (!ok) return 2;
      g.long_table = b[0]; g.loss = b[1]; g.fused_weights = b[2]; k.varlen_extend = b[3]; k.last_layer_tail = b[4]; k.norm_fused = b[5];
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
      printf("\n");
    } else if (kind == 'G') {
      int left, cap, max_rows, lens[64];
      if (scanf("%d %d %d", &left, &cap, &max_rows) != 3 || left < 1 || left > 64) return 2;
      for (int i = 0; i < left; ++i) if (scanf("%d", &lens[i]) != 1) return 2;
      printf("%d\n", prefill_group_size(lens, left, cap, max_rows));
    } else {
      return 2;
    }
  }
  return 0;
}
