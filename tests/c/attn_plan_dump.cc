// Prints the decisions of csrc/gvl_attn_plan.h (host-only) for the cases on stdin: built with the host C++ compiler by tests/attn_plan.py.
// One case per line, the first word says which function:
//   A B H KV S D Dout Sk qpos0 causal ones_row k_ones ring pipe pipe_rows v_ld q_ld k_ld max_pages vl_n vl_rows[0..8] present vl_tables aligned lazy no_ones
//       present: bit 0 block table, 1 Vrows, 2 Qrows, 3 Krows, 4 q_rs, 5 q_nw;  vl_tables: bit u = table of sequence u;  aligned: bit 0 O, 1 Vrows, 2 Qrows, 3 Krows, 4 q_nw
//     -> "-1"  or per launch  "mode family D NWAVES NS ONES VROW VL grid block lds q_begin q_rows lazy"
//   D H KV D nsplit batch hpb cpb gsplit no_gqa gqa_valu gqa_direct
//     -> "-1"  or  "family D t1 t2 grid_x grid_y grid_z batch cpb gsplit hpb"
//   S B H KV nsplit force_cpb force_hpb capturing pos[0..B)
//     -> "gsplit cpb hpb"
// With the argument "lists": the instantiation lists instead, one "fwd|iv2_pipe|gqa|head <template arguments>" per line.
#include <cstdio>
#include <cstring>
#include "gvl_attn_plan.h"

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "lists")) {
#define P6(D, NW, NS, ONES, VROW, VL) printf("fwd %d %d %d %d %d %d\n", D, NW, NS, ONES, VROW, VL);
#define P1(NW) printf("iv2_pipe %d\n", NW);
#define PG(D, GM, STG) printf("gqa %d %d %d\n", D, GM, STG);
#define PH(D, PHASE) printf("head %d %d\n", D, PHASE);
    GVL_ATTN_FWD_LIST(P6) GVL_ATTN_IV2_PIPE_LIST(P1) GVL_DECODE_ATTN_GQA_LIST(PG) GVL_DECODE_ATTN_HEAD_LIST(PH)
    return 0;
  }
  char kind;
  while (scanf(" %c", &kind) == 1) {
    if (kind == 'A') {
      AttnGeometry g{};
      int present, tables, aligned, no_ones, ok = 1;
      float lazy;
      int* f[] = {&g.B, &g.H, &g.KV, &g.S, &g.D, &g.Dout, &g.Sk, &g.qpos0, &g.causal, &g.ones_row, &g.k_ones, &g.ring, &g.pipe, &g.pipe_rows, &g.v_ld, &g.q_ld, &g.k_ld, &g.max_pages, &g.vl_n};
      for (int* p : f) ok &= scanf("%d", p) == 1;
      for (int& r : g.vl_rows) ok &= scanf("%d", &r) == 1;
      ok &= scanf("%d %d %d %f %d", &present, &tables, &aligned, &lazy, &no_ones) == 5;
      if (!ok) return 2;
      g.block_table = present & 1; g.Vrows = present & 2; g.Qrows = present & 4; g.Krows = present & 8; g.q_rs = present & 16; g.q_nw = present & 32;
      for (int u = 0; u < GVL_MAX_PREFILL_BATCH; ++u) g.vl_tables[u] = tables >> u & 1;
      g.O16 = aligned & 1; g.Vrows16 = aligned & 2; g.Qrows16 = aligned & 4; g.Krows16 = aligned & 8; g.q_nw16 = aligned & 16;
      AttnLaunch out[GVL_ATTN_MAX_LAUNCHES];
      const int n = attn_plan(g, AttnKnobs{lazy, no_ones != 0}, out);
      if (n < 0) { printf("-1\n"); continue; }
      for (int i = 0; i < n; ++i) {
        const AttnLaunch& l = out[i];
        printf("%s%d %d %d %d %d %d %d %d %u %d %d %d %d %.9g", i ? " " : "", l.mode, l.family, l.D, l.NWAVES, l.NS, l.ONES, l.VROW, l.VL, l.grid, l.block, l.lds, l.q_begin, l.q_rows, (double)l.lazy);
      }
      printf("\n");
    } else if (kind == 'D') {
      DecodeAttnGeometry g{};
      int k0, k1, k2;
      if (scanf("%d %d %d %d %d %d %d %d %d %d %d", &g.H, &g.KV, &g.D, &g.nsplit, &g.batch, &g.hpb, &g.cpb, &g.gsplit, &k0, &k1, &k2) != 11) return 2;
      DecodeAttnLaunch l;
      if (decode_attn_plan(g, DecodeAttnKnobs{k0 != 0, k1 != 0, k2 != 0}, &l) < 0) { printf("-1\n"); continue; }
      printf("%d %d %d %d %u %u %u %d %d %d %d\n", l.family, l.D, l.t1, l.t2, l.grid_x, l.grid_y, l.grid_z, l.batch, l.cpb, l.gsplit, l.hpb);
    } else if (kind == 'S') {
      int B, H, KV, nsplit, fc, fh, cap, pos[GVL_MAX_DECODE_BATCH];
      if (scanf("%d %d %d %d %d %d %d", &B, &H, &KV, &nsplit, &fc, &fh, &cap) != 7 || B < 0 || B > GVL_MAX_DECODE_BATCH) return 2;
      for (int b = 0; b < B; ++b) if (scanf("%d", &pos[b]) != 1) return 2;
      const DecodeAttnShape s = decode_attn_shape(pos, B, H, KV, nsplit, fc, fh, cap != 0);
      printf("%d %d %d\n", s.gsplit, s.cpb, s.hpb);
    } else {
      return 2;
    }
  }
  return 0;
}
