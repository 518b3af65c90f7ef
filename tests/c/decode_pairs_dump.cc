// Prints decode_parts_paired (csrc/gvl_decode_plan.h, host-only) for the cases on stdin: built with the host C++ compiler by tests/test_guidance_ref_cpu.py.
// One case per line: "mfma n r0 r1 ... r(n-1)" (rows[i] = 1 a plain sequence, 2 a guided pair) -> the UNITS each step takes, in order (an empty line for n = 0).
#include <cstdio>
#include "gvl_decode_plan.h"

int main() {
  int mfma, n;
  while (scanf("%d %d", &mfma, &n) == 2) {
    int rows[1024], units[1024];
    if (n < 0 || n > 1024) return 2;
    for (int i = 0; i < n; ++i) if (scanf("%d", &rows[i]) != 1 || (rows[i] != 1 && rows[i] != 2)) return 2;
    const int k = decode_parts_paired(mfma != 0, rows, n, units);
    for (int i = 0; i < k; ++i) printf(i ? " %d" : "%d", units[i]);
    printf("\n");
  }
  return 0;
}
