// Prints gemm_plan's decisions (csrc/gvl_gemm_plan.h, host-only) for the cases on stdin: built with the host C++ compiler by tests/gemm_plan.py.
// One case per line, 17 integers:  M N K lda ldw ldc ldr grp_rows rowsq_ld epi tile_cfg ptr16 a4_mode n_cu lab_cfg small_pct small64   (small_pct / small64 < 0: default)
// One answer per line:  "-1"  or  "0 <whole cost> <chosen cost>" followed by "form epi m_begin m_end n_begin n_end" per launch.
#include <cstdio>
#include "gvl_gemm_plan.h"

int main() {
  int M, N, K, lda, ldw, ldc, ldr, grp, rsld, epi, cfg, p16, a4m, ncu, lab, pct, s64;
  while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &M, &N, &K, &lda, &ldw, &ldc, &ldr, &grp, &rsld, &epi, &cfg, &p16, &a4m, &ncu, &lab, &pct, &s64) == 17) {
    const GemmGeometry g{M, N, K, lda, ldw, ldc, ldr, grp, rsld, epi, cfg, p16 != 0};
    const GemmKnobs k{ncu, lab, a4m, pct < 0 ? GVL_GEMM_KNOBS_DEFAULT.small_unit : pct / 100.0, s64 < 0 ? GVL_GEMM_KNOBS_DEFAULT.small64 : s64, GVL_GEMM_KNOBS_DEFAULT.narrow};
    GemmLaunch out[GVL_GEMM_MAX_LAUNCHES];
    GemmPlanCost c;
    const int n = gemm_plan(g, k, out, &c);
    if (n < 0) { printf("-1\n"); continue; }
    printf("0 %.17g %.17g", c.whole, c.chosen);
    for (int i = 0; i < n; ++i) printf(" %d %d %d %d %d %d", out[i].form, out[i].epi, out[i].m_begin, out[i].m_end, out[i].n_begin, out[i].n_end);
    printf("\n");
  }
  return 0;
}
