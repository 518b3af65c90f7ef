// gvl_gemm_plan.h -- which kernel form(s) a GEMM launch takes: a PURE host function of the geometry and a handful of knobs.
// Host-only: no HIP header, no statics, no environment -- any C++17 compiler builds it (tests/c/gemm_plan_dump.cc does, and tests/test_gemm_plan_cpu.py pins
// every decision against recorded ones).  All forms are bit-identical by design, so no RESULT test can notice a wrong choice of form: this file is what says
// which kernel ran.  gvl_launch_gemm (gvl_gemm.hip) = gemm_plan + a switch on the form.
#pragma once
#include "gvl_gemm4p_loop.inc"   // #defines only: GVL_A4P_EPI_LIST, GVL_A4P_MIN_NK_E<epi>

// ---- tile_cfg values (GemmArgs.tile_cfg, gvl_op_gemm, GVL_GEMM_CFG of LAB builds; documented in gvl.h) ---------------------------------------------------------
enum : int {
  GVL_CFG_AUTO = 0,        // the library chooses (K and tile count, below), then the wave-quantisation planner
  GVL_CFG_LOCKSTEP = 1,    // 128 x 128, every wave requests the next k-tile at the top of the iteration, per-lane epilogue (baseline of tests / A-B)
  GVL_CFG_128 = 21,        // 128 x 128, 2 blocks / CU; an explicit 21 small enough for the 64 x 128 rule takes 64 x 128, like a planner remainder
  GVL_CFG_64x128 = 22,     // 64 x 128 tiles of the same kernel, 3-slot ring
  GVL_CFG_BIG = 80,        // the 256 x 256 kernel, the library's choice of form (big_form_preferred); an explicit 80 is not re-planned
  GVL_CFG_PP = 82,         // 8-wave ping-pong
  GVL_CFG_A4_S0 = 84,      // 4-wave kernel (gvl_gemm4.hip), loop schedule 0
  GVL_CFG_PP_LANE = 85,    // LAB: was "ping-pong with the per-lane epilogue"; since the 4-wave forms it behaves as 86, but refuses the fused-RMSNorm epilogues
  GVL_CFG_A4_S1 = 86,      // 4-wave kernel, loop schedule 1 (the shipped one)
  GVL_CFG_A4_S2 = 87,      // 4-wave kernel, loop schedule 2
  GVL_CFG_A4P = 88,        // 4-wave kernel with the epilogue pipelined into the next tile's main loop (gvl_gemm4p.hip)
};
// An explicit 84 ... 88 that does not serve the (epilogue, geometry) falls back: 88 -> 86 -> 82.

// ---- kernel forms: what a launch actually runs ------------------------------------------------------------------------------------------------------------------
enum GemmForm : int {
  GVL_FORM_LOCKSTEP_128 = 0, GVL_FORM_128, GVL_FORM_64x128,   // gemm_bf16_kernel
  GVL_FORM_PP_STAGED, GVL_FORM_PP_LANE,                       // gemm_pp_kernel: LDS-staged whole-row epilogue / generic per-lane epilogue
  GVL_FORM_A4_S0, GVL_FORM_A4_S1, GVL_FORM_A4_S2,             // gemm_a4_kernel
  GVL_FORM_A4P,                                               // gemm_a4p_kernel
};
constexpr bool gemm_form_is_256(int form) { return form >= GVL_FORM_PP_STAGED; }   // 32-bit DMA offsets, persistent grid, rasterisation band

// ---- fused-epilogue code: a bit set; the staged epilogues are compile-time specialised per code ----------------------------------------------------------------
enum : int {
  GVL_EPI_ACT = 3,         // the activation field, values as GVL_ACT_* (checked in gvl_gemm.hip)
  GVL_EPI_QGELU = 1, GVL_EPI_GELU = 2, GVL_EPI_SWIGLU = 3,
  GVL_EPI_F32 = 4,         // C and the residual are f32
  GVL_EPI_RESID = 8, GVL_EPI_GAMMA = 16, GVL_EPI_BIAS = 32,
  GVL_EPI_ROWSCALE = 64,   // fused RMSNorm, consumer side: the row scale multiplies the accumulator
  GVL_EPI_ROWSQ = 128,     // fused RMSNorm, producer side: row sums of squares of the rounded outputs
  GVL_EPI_GENERIC = -1,    // a launch's epilogue when the generic per-lane code runs (reads GemmArgs at run time)
};
constexpr int epi_code(int act, bool out_f32, bool resid, bool gamma, bool bias, bool rowscale, bool rowsq) {
  return (act & GVL_EPI_ACT) | (out_f32 ? GVL_EPI_F32 : 0) | (resid ? GVL_EPI_RESID : 0) | (gamma ? GVL_EPI_GAMMA : 0) | (bias ? GVL_EPI_BIAS : 0) |
         (rowscale ? GVL_EPI_ROWSCALE : 0) | (rowsq ? GVL_EPI_ROWSQ : 0);
}
// THE list of staged epilogues (the 128 x 128, 64 x 128 and ping-pong dispatch switches); the 4-wave kernel serves the bf16-output part of it.
// (The pipelined kernel's list is generated with its loops: GVL_A4P_EPI_LIST.)
#define GVL_EPI_STAGED_BF16(X)                                                                                                                          \
  X(0) X(GVL_EPI_BIAS) X(GVL_EPI_BIAS | GVL_EPI_QGELU) X(GVL_EPI_BIAS | GVL_EPI_GELU) X(GVL_EPI_SWIGLU)                                                 \
  X(GVL_EPI_BIAS | GVL_EPI_GAMMA | GVL_EPI_RESID) X(GVL_EPI_RESID)                                                                                      \
  X(GVL_EPI_ROWSCALE) X(GVL_EPI_ROWSCALE | GVL_EPI_SWIGLU) X(GVL_EPI_ROWSCALE | GVL_EPI_BIAS | GVL_EPI_GELU)                                            \
  X(GVL_EPI_ROWSQ) X(GVL_EPI_ROWSQ | GVL_EPI_RESID) X(GVL_EPI_ROWSQ | GVL_EPI_BIAS | GVL_EPI_GAMMA | GVL_EPI_RESID)
#define GVL_EPI_STAGED_F32(X) X(GVL_EPI_F32) X(GVL_EPI_F32 | GVL_EPI_BIAS) X(GVL_EPI_F32 | GVL_EPI_BIAS | GVL_EPI_RESID)
#define GVL_EPI_STAGED(X) GVL_EPI_STAGED_BF16(X) GVL_EPI_STAGED_F32(X)
#define GVL_EPI_A4(X) GVL_EPI_STAGED_BF16(X)

#define GVL_PLAN_CASE_TRUE(E) case (E): return true;
inline bool gemm_epi_is_staged(int epi) { switch (epi) { GVL_EPI_STAGED(GVL_PLAN_CASE_TRUE) default: return false; } }
inline bool gemm_epi_a4(int epi) { switch (epi) { GVL_EPI_A4(GVL_PLAN_CASE_TRUE) default: return false; } }
#undef GVL_PLAN_CASE_TRUE
// fewest k-tiles (K / 64) the pipelined kernel's statement for `epi` runs with; 0 = it has none
inline int gemm_a4p_min_nk(int epi) {
  switch (epi) {
#define GVL_PLAN_CASE_NK(E) case E: return GVL_A4P_MIN_NK_E##E;
    GVL_A4P_EPI_LIST(GVL_PLAN_CASE_NK)
#undef GVL_PLAN_CASE_NK
    default: return 0;
  }
}
constexpr int GVL_A4_MIN_NK = 3;

// Which form of the 256 x 256 kernel an (epilogue) takes when the library chooses (cfg 80), from same-box interleaved runs on the model's shapes
// (profiles/r06_gemm4_lab_model.txt; tools/gemm4_lab.py 82,86,88 model):
//   pipelined 4-wave (88): the epilogues with real VALU / LDS work behind the bf16 rounding -- erf-GELU (98: +5 % over the 8-wave kernel, +10 % over the plain 4-wave
//                          one), SwiGLU (67: +4.5 %), residual + row statistics (136: +3 ... +7 %; 184: +1 ... +5 %) -- that work rides in the next tile's MFMA gaps;
//                          bias alone (32: +2 %, its slice read once per tile into dead fragment registers);
//   plain 4-wave (86):     the store-only epilogues (64, 0, 3, 8, 128: +2 ... +4 %; pipelining them buys nothing: what remains exposed either way is the accumulator drain);
//   8-wave ping-pong (82): CLIP's quick-GELU (33: the 4-wave forms lose 1 ... 2 % there), the f32-output epilogues and everything the 4-wave kernels do not serve.
inline int big_form_preferred(int epi) {
  switch (epi) {
    case GVL_EPI_ROWSCALE | GVL_EPI_BIAS | GVL_EPI_GELU: case GVL_EPI_ROWSCALE | GVL_EPI_SWIGLU: case GVL_EPI_ROWSQ | GVL_EPI_RESID:
    case GVL_EPI_ROWSQ | GVL_EPI_BIAS | GVL_EPI_GAMMA | GVL_EPI_RESID: case GVL_EPI_BIAS: return GVL_CFG_A4P;
    case GVL_EPI_ROWSCALE: case 0: case GVL_EPI_SWIGLU: case GVL_EPI_RESID: case GVL_EPI_ROWSQ: return GVL_CFG_A4_S1;
    default: return GVL_CFG_PP;
  }
}

// ---- inputs and output of the decision --------------------------------------------------------------------------------------------------------------------------
struct GemmGeometry {            // only what the decision reads
  int M, N, K;
  int lda, ldw, ldc, ldr;        // row pitches in elements; ldw = 0 means K
  int grp_rows, rowsq_ld;
  int epi;                       // epi_code(...)
  int tile_cfg;                  // GVL_CFG_*
  bool ptr16;                    // C and the residual are 16-byte aligned (the caller's: it reads pointers)
};
struct GemmKnobs {
  int n_cu;                      // compute units of the device, UNMASKED: the planner costs in whole CUs (the persistent grids round down to 8 XCDs)
  int lab_cfg;                   // LAB: GVL_GEMM_CFG, replaces tile_cfg 0 and switches the planner and the 64 x 128 rule off (0 = none)
  int a4_mode;                   // gemm_a4 (gvl_debug_set): 0 = cfg 80 is the 8-wave kernel, 1 (default) = big_form_preferred, 2 = the plain 4-wave kernel wherever it
                                 // serves, 3 = the pipelined one wherever it serves (then the plain one)
  double small_unit;             // cost of up to one CU-count of 128 x 128 tiles, in 256 x 256 tile times (0.5; LAB: GVL_GEMM_SMALLCOST percent)
  int small64;                   // 64 x 128 rule: a remainder of at most small64 * n_cu / 2 128 x 128 tiles takes 64 x 128 tiles (3; LAB: GVL_GEMM_SMALL64, 0 = off)
  int narrow;                    // gemm_narrow (gvl_debug_set): passed through to the pipelined kernel; no form depends on it
};
constexpr GemmKnobs GVL_GEMM_KNOBS_DEFAULT = {256, 0, 1, 0.5, 3, 1};
struct GemmLaunch {
  int form;                      // GemmForm
  int epi;                       // the staged epilogue's code, or GVL_EPI_GENERIC
  int m_begin, m_end, n_begin, n_end;   // output rows / columns of this launch
};
struct GemmPlanCost { double whole, chosen; };   // planner's estimate, in 256 x 256 tile times, of the unsplit launch and of the plan taken (0, 0: not planned)
constexpr int GVL_GEMM_MAX_LAUNCHES = 3;

// Returns the number of launches written to out (1 ... 3: they tile [0, M) x [0, N) exactly once, in launch order), or -1: the arguments are not served.
inline int gemm_plan(const GemmGeometry& g, const GemmKnobs& k, GemmLaunch out[GVL_GEMM_MAX_LAUNCHES], GemmPlanCost* cost = nullptr) {
  if (cost) *cost = GemmPlanCost{0, 0};
  if (g.M <= 0 || g.N <= 0 || g.K <= 0) return -1;
  const int ldw = g.ldw ? g.ldw : g.K;
  const int act = g.epi & GVL_EPI_ACT;
  const bool f32 = g.epi & GVL_EPI_F32, resid = g.epi & GVL_EPI_RESID, rows = g.epi & (GVL_EPI_ROWSCALE | GVL_EPI_ROWSQ);
  if (g.K % 64 != 0 || g.N % 4 != 0 || g.lda % 8 != 0 || ldw % 8 != 0 || ldw < g.K) return -1;   // K padded to 64 by the packer; 16-byte rows
  if (act == GVL_EPI_SWIGLU && (g.epi & (GVL_EPI_F32 | GVL_EPI_RESID | GVL_EPI_GAMMA))) return -1;
  if ((g.epi & GVL_EPI_ROWSQ) && (g.N % 64 != 0 || f32 || act == GVL_EPI_SWIGLU || g.rowsq_ld < g.N / 64 || g.grp_rows)) return -1;

  const bool automatic = g.tile_cfg == GVL_CFG_AUTO && k.lab_cfg == 0;
  int cfg = g.tile_cfg != GVL_CFG_AUTO ? g.tile_cfg : k.lab_cfg;
  if (cfg == GVL_CFG_AUTO) {
    // measured on MI355X (tools/gemm_bench.py, profiles/r01_gemm_microbench*.txt):
    //  * the 256x256 kernel: best whenever K is long enough to amortise its un-overlapped prologue/epilogue (one block / CU) and there are enough tiles
    //    (CLIP qkv / fc1, K = 1024, 336 / 448 tiles: +8...17 % over 128x128);
    //  * 128x128, 2 blocks / CU: short K or few tiles (CLIP out / fc2: 112 tiles).
    // short K but thousands of tiles (the three-pass patch GEMM at the bench's M: K = 640, 864 / 4 608 tiles): the big kernel measured 76.6 vs 83.2 us (CLIP) and
    // 454.6 vs 477.7 us (InternVideo2, bias) -- profiles/r05_patch_gemm_floor.txt
    const long t256 = (long)((g.M + 255) / 256) * ((g.N + 255) / 256);
    cfg = ((g.K >= 1024 && t256 >= 128) || (g.K >= 512 && t256 >= 512)) ? GVL_CFG_BIG : GVL_CFG_128;
  }
  // 32-bit DMA offsets: every 256 x 256 form hands an operand of 4 GiB or more to 128 x 128 -- the whole launch here, every sub-launch of a split in resolve()
  auto over_4g = [&](long rows_a, long rows_w) { return (unsigned long long)rows_w * ldw * 2 >= (1ull << 32) || (unsigned long long)rows_a * g.lda * 2 >= (1ull << 32); };
  auto is_big_cfg = [](int c) { return c == GVL_CFG_BIG || c == GVL_CFG_PP || (c >= GVL_CFG_A4_S0 && c <= GVL_CFG_A4P); };
  if (is_big_cfg(cfg) && over_4g(g.M, g.N)) cfg = GVL_CFG_128;

  struct Piece { int cfg; bool remainder; int m0, m1, n0, n1; } piece[GVL_GEMM_MAX_LAUNCHES];
  int np = 0;
  if (cfg == GVL_CFG_BIG && automatic) {
    // Wave-quantisation planner.  The persistent 256x256 kernel runs one block per CU, so a launch costs ceil(tiles / CUs)
    // tile times, and a partial last tile column (N = 1408 = 5.5 x 256) wastes half of its MFMA work.  Candidate plans, costed
    // in units of one 256x256 tile time (the small kernel: see small_unit):
    //   W  whole GEMM on the big kernel;
    //   M  whole rounds of tile ROWS on the big kernel, the remaining rows on the small kernel;
    //   N  the full 256-wide tile columns through W or M, the N % 256 tail columns on the small kernel.
    // e.g. InternVideo2 proj/fc2 (M = 24588, N = 1408): W = 3, M = 3.0, N = 2.5 (485 big tiles in 2 rounds + 193 small).
    // small_unit: half the FLOPs at ~0.76x the rate would be 0.33, but an under-filled small launch runs its lone blocks far below that rate: same-box A/B of
    // the whole bench, 0.33 / 0.45-0.75 / 0.90 -> GEMM time 73.4 / 73.0 / 75.7 ms per clip.  A split must win by 0.1 tile times (hysteresis).
    const int n_cu = k.n_cu;
    auto small_cost = [&](long t) { const long halves = (t + n_cu - 1) / n_cu; return t > 0 ? k.small_unit * (double)halves : 0.0; };
    struct Plan { double cost; int big_rows; };   // big_rows = tile rows given to the big kernel (all of them: no M split)
    auto plan_mw = [&](int M, int N) {            // best of W and M for an [M, N] problem
      const int tiles_m = (M + 255) / 256, tiles_n = (N + 255) / 256;
      const long tiles = (long)tiles_m * tiles_n, rounds = tiles / n_cu;
      Plan best{(double)((tiles + n_cu - 1) / n_cu), tiles_m};
      if (rounds >= 1 && tiles % n_cu != 0) {
        const int br = (int)((rounds * n_cu) / tiles_n);
        if (br >= 1 && br < tiles_m) {
          const double c = (double)rounds + small_cost((long)((M - br * 256 + 127) / 128) * ((N + 127) / 128));
          if (c < best.cost - 0.1) best = Plan{c, br};
        }
      }
      return best;
    };
    const Plan whole = plan_mw(g.M, g.N);
    int n_big = g.N;
    Plan chosen = whole;
    if (g.N % 256 != 0 && g.N > 256 && act != GVL_EPI_SWIGLU) {   // (SwiGLU: output column n comes from W rows 2n, 2n + 1 -- the column offsets below would not hold)
      const int nb = (g.N / 256) * 256;
      const Plan p = plan_mw(g.M, nb);
      const double c = p.cost + small_cost((long)((g.M + 127) / 128) * ((g.N - nb + 127) / 128));
      if (c < whole.cost - 0.1) { chosen = Plan{c, p.big_rows}; n_big = nb; }
    }
    if (cost) *cost = GemmPlanCost{(double)(((long)((g.M + 255) / 256) * ((g.N + 255) / 256) + n_cu - 1) / n_cu), chosen.cost};
    const int big_m = chosen.big_rows < (g.M + 255) / 256 ? chosen.big_rows * 256 : g.M;
    piece[np++] = Piece{GVL_CFG_BIG, false, 0, big_m, 0, n_big};
    if (big_m != g.M) piece[np++] = Piece{GVL_CFG_128, true, big_m, g.M, 0, n_big};
    if (n_big != g.N) piece[np++] = Piece{GVL_CFG_128, true, 0, g.M, n_big, g.N};
  } else {
    piece[np++] = Piece{cfg, g.tile_cfg == GVL_CFG_128 && k.lab_cfg == 0, 0, g.M, 0, g.N};
  }

  const int es = f32 ? 4 : 2;
  for (int i = 0; i < np; ++i) {
    const Piece& p = piece[i];
    const int N = p.n1 - p.n0;           // p.m1 stays absolute: the kernels address rows [m_begin, M) from the operands' row 0
    int c = p.cfg;
    if (is_big_cfg(c) && over_4g(p.m1, N)) c = GVL_CFG_128;
    // whole 16-byte output rows: the LDS-staged epilogue.  (Column offsets of a split are multiples of 256 elements: they keep the pointers' alignment.)
    const bool stg_ok = g.ptr16 && N % 16 == 0 && g.grp_rows == 0 && ((long)g.ldc * es) % 16 == 0 && (!resid || ((long)g.ldr * es) % 16 == 0);
    const bool staged = stg_ok && gemm_epi_is_staged(g.epi);
    if (rows && (!staged || c == GVL_CFG_LOCKSTEP || c == GVL_CFG_PP_LANE)) return -1;   // the fused-RMSNorm epilogues exist in the staged (whole-row) form only
    // 64x128 tiles: twice the blocks of 128x128 for launches that would leave most CUs with ONE 128x128 block (remainder rows / tail columns of the planner:
    // 193-264 tiles on 512 slots); measured -0.6 ms of GEMM time per clip
    if (c == GVL_CFG_128 && p.remainder && k.small64) {
      const long t128 = (long)((p.m1 - p.m0 + 127) / 128) * ((N + 127) / 128);
      if (t128 * 2 <= (long)k.small64 * k.n_cu) c = GVL_CFG_64x128;
    }
    GemmLaunch& l = out[i];
    l = GemmLaunch{0, staged ? g.epi : GVL_EPI_GENERIC, p.m0, p.m1, p.n0, p.n1};
    if (is_big_cfg(c) && c != GVL_CFG_PP) {
      int want = c != GVL_CFG_BIG ? c : (k.a4_mode == 0 ? GVL_CFG_PP : (k.a4_mode == 1 ? big_form_preferred(g.epi) : (k.a4_mode == 2 ? GVL_CFG_A4_S1 : GVL_CFG_A4P)));
      // 32-bit buffer offsets of the 4-wave kernels: rows up to 256 past the matrix are addressed (and clamped by the descriptor)
      const bool a4_geo = stg_ok && !over_4g((long)p.m1 + 256, (long)N + 256);
      const int nk = g.K / 64;
      if (want == GVL_CFG_A4P) {
        const int min_nk = gemm_a4p_min_nk(g.epi);
        const bool out_32bit = (unsigned long long)g.ldc * 2 * 136 < (1ull << 31) && (!resid || (unsigned long long)g.ldr * 2 * 136 < (1ull << 31));
        if (a4_geo && out_32bit && min_nk > 0 && nk >= min_nk) { l.form = GVL_FORM_A4P; continue; }
        want = GVL_CFG_A4_S1;
      }
      if (want >= GVL_CFG_A4_S0 && want <= GVL_CFG_A4_S2 && a4_geo && nk >= GVL_A4_MIN_NK && gemm_epi_a4(g.epi)) {
        l.form = want == GVL_CFG_A4_S0 ? GVL_FORM_A4_S0 : (want == GVL_CFG_A4_S2 ? GVL_FORM_A4_S2 : GVL_FORM_A4_S1);
        continue;
      }
      c = GVL_CFG_PP;
    }
    switch (c) {
      case GVL_CFG_LOCKSTEP: l.form = GVL_FORM_LOCKSTEP_128; l.epi = GVL_EPI_GENERIC; break;
      case GVL_CFG_128: l.form = GVL_FORM_128; break;
      case GVL_CFG_64x128: l.form = GVL_FORM_64x128; break;
      case GVL_CFG_PP: l.form = staged ? GVL_FORM_PP_STAGED : GVL_FORM_PP_LANE; break;
      default: return -1;
    }
  }
  return np;
}
