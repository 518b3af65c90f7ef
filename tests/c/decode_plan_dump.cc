// Prints the decisions of csrc/gvl_decode_plan.h (host-only) for the cases on stdin: built with the host C++ compiler by tests/decode_plan.py.
// One case per line, the first word says which function:
//   P B layers hidden mfma fmt folded norm_fused
//     -> the refusal (-1)  or  "embed_norm attn_out_tiled norm_launches n_gemv n_attn n_other" then per projection kind (qkv of layer 0, qkv of later layers, o_proj,
//        gate_up, down_proj, lm_head) "launcher weight scales input sq_out out_tiled"
//   G mfma n                              -> the step sizes n waiting sequences are cut into, in order (nothing for n = 0)
//   A mfma B                              -> decode_batch_ok
//   S mfma left                           -> decode_group_size
//   M hidden inter heads head_dim         -> decode_mfma_ok
//   Q fmt hidden inter attn_width         -> decode_quant_ok
//   R mfma fmt norm_fused folded hidden   -> decode_rs_ok
// With the argument "reasons": the refusal messages instead, one "-k message" per line.
#include <cstdio>
#include <cstring>
#include "gvl_decode_plan.h"

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "reasons")) {
    printf("%d %s\n", GVL_DECODE_BAD_BATCH, decode_refusal_reason(GVL_DECODE_BAD_BATCH));
    return 0;
  }
  char kind;
  int v[7];
  while (scanf(" %c", &kind) == 1) {
    const char* kinds = "PGASMQR";
    const int counts[] = {7, 2, 2, 2, 4, 4, 5};
    const char* at = strchr(kinds, kind);
    if (!at) return 2;
    for (int i = 0; i < counts[at - kinds]; ++i) if (scanf("%d", &v[i]) != 1) return 2;
    if (kind == 'P') {
      DecodePlan p;
      const int rc = decode_plan(DecodeGeometry{v[0], v[1], v[2], v[3] != 0, v[4], v[5] != 0}, DecodeKnobs{v[6] != 0}, &p);
      if (rc) { printf("%d\n", rc); continue; }
      printf("%d %d %d %d %d %d", p.embed_norm, p.attn_out_tiled, p.norm_launches, p.n_gemv, p.n_attn, p.n_other);
      for (const DecodeProjPlan& e : p.proj) printf(" %d %d %d %d %d %d", e.launcher, e.weight, e.scales, e.input, e.sq_out, e.out_tiled);
      printf("\n");
    } else if (kind == 'G') {
      int sizes[1024];
      if (v[1] < 0 || v[1] > 1024) return 2;
      const int k = decode_parts(v[0] != 0, v[1], sizes);
      for (int i = 0; i < k; ++i) printf(i ? " %d" : "%d", sizes[i]);
      printf("\n");
    } else if (kind == 'A') printf("%d\n", decode_batch_ok(v[0] != 0, v[1]));
    else if (kind == 'S') printf("%d\n", decode_group_size(v[0] != 0, v[1]));
    else if (kind == 'M') printf("%d\n", decode_mfma_ok(v[0], v[1], v[2], v[3]));
    else if (kind == 'Q') printf("%d\n", decode_quant_ok(v[0], v[1], v[2], v[3]));
    else printf("%d\n", decode_rs_ok(v[0] != 0, v[1], v[2] != 0, v[3] != 0, v[4]));
  }
  return 0;
}
