// gvl_attn_plan.h -- which kernel(s) an attention launch takes, on which grid: PURE host functions of the geometry and a handful of knobs.
// Host-only: no HIP header, no statics, no environment -- any C++17 compiler builds it (tests/c/attn_plan_dump.cc does, and tests/test_attn_plan_cpu.py pins
// every decision against recorded ones).  All forms are bit-identical by design, so no RESULT test can notice a wrong choice of form: this file is what says
// which kernel ran.  gvl_launch_attention / gvl_launch_decode_attention (gvl_attn.hip) = read the knobs, plan, dispatch on the planned instantiation;
// the decode step (gvl_llm.hip) takes its launch shape from decode_attn_shape.  The LDS and grid formulas exist here and nowhere else.
#pragma once
#include "gvl_limits.h"

// =================================================================================================================================================================
// prefill / vision attention
// =================================================================================================================================================================
// Operand modes (AttnArgs, gvl_internal.h): where q, k and v are read from.  attn_fwd_kernel's VROW / VL template arguments are a function of the mode.
enum AttnMode : int {
  GVL_ATTN_PAGED = 0,        // q as [B][H][S][D], K / V^T in 64-token pages (block table, or null: page(b, t) = b * n_tiles + t)        VROW 0
  GVL_ATTN_V_ROWS,           // V as token rows, read in place from a tower's fused-qkv GEMM output (no V^T pass); q, K as above          VROW 1
  GVL_ATTN_QKV_ROWS,         // q, k and v as token rows (CLIP: no per-token transform of q / k, so no qkv_post pass at all)              VROW 2
  GVL_ATTN_QNORM_V_ROWS,     // q as token rows, RMS-normalised as its fragments are loaded, V in place, K in pages (InternVideo2)        VROW 3
  GVL_ATTN_RAGGED,           // ragged causal prefill: vl_n sequences packed back to back, one grid, a block table per sequence           VL 1
};
enum AttnFamily : int { GVL_ATTN_FWD = 0, GVL_ATTN_IV2_PIPE };   // attn_fwd_kernel<D, NWAVES, NS, ONES, VROW, VL> / attn_iv2_pipe_kernel<NWAVES>

// THE lists of instantiations: the dispatch switches and their per-instantiation LDS once-guards (gvl_attn.hip) and the test's expected set
// (tests/c/attn_plan_dump.cc prints them) all come from here.  Adding a form = one entry + one rule in attn_plan.
//   X(D, NWAVES, NS, ONES, VROW, VL)
#define GVL_ATTN_FWD_LIST(X)                                                                                     \
  X(64, 4, 2, 0, 0, 0) X(64, 4, 2, 0, 1, 0) X(64, 4, 2, 0, 2, 0)                                                 \
  X(96, 4, 2, 0, 0, 0) X(96, 4, 2, 1, 0, 0) X(96, 4, 3, 0, 0, 0) X(96, 4, 2, 0, 1, 0) X(96, 4, 2, 1, 1, 0)       \
  X(96, 4, 2, 0, 3, 0) X(96, 4, 2, 1, 3, 0)                                                                      \
  X(128, 4, 2, 0, 0, 0) X(128, 4, 3, 0, 0, 0)                                                                    \
  X(64, 4, 2, 0, 0, 1) X(96, 4, 2, 0, 0, 1) X(128, 4, 2, 0, 0, 1)
//   X(NWAVES): the hand-pipelined InternVideo2 kernel is attn_fwd_kernel<96, NWAVES, 2, 1, 3, 0>'s arithmetic on 32 * NWAVES query rows per block
#define GVL_ATTN_IV2_PIPE_LIST(X) X(4) X(8)
constexpr int attn_fwd_key(int D, int NWAVES, int NS, int ONES, int VROW, int VL) { return ((((D * 16 + NWAVES) * 4 + NS) * 2 + ONES) * 4 + VROW) * 2 + VL; }

struct AttnGeometry {            // only what the decision reads
  int B, H, KV, S, D, Dout, Sk, qpos0, causal, ones_row, k_ones, ring, pipe, pipe_rows, v_ld, q_ld, k_ld, max_pages;
  int vl_n, vl_rows[GVL_MAX_PREFILL_BATCH + 1];
  bool block_table, Vrows, Qrows, Krows, q_rs, q_nw, vl_tables[GVL_MAX_PREFILL_BATCH];   // which optional operands are present
  bool O16, Vrows16, Qrows16, Krows16, q_nw16;                                          // 16-byte alignment of the pointers (the caller's: it reads them)
};
struct AttnKnobs {
  float lazy;                    // LAB GVL_ATTN_LAZY: the running max moves only when a tile max exceeds it by more than this (log2 units); 0 = whenever a max grows
  bool no_ones;                  // LAB GVL_ATTN_NO_ONES: never the ONES forms (row sums from the V^T ones row)
};
constexpr AttnKnobs GVL_ATTN_KNOBS_DEFAULT = {8.f, false};
struct AttnLaunch {
  int mode;                      // AttnMode
  int family;                    // AttnFamily
  int D, NWAVES, NS, ONES, VROW, VL;   // template arguments (iv2_pipe: NWAVES is the only real one, the rest say which attn_fwd_kernel it equals)
  unsigned grid; int block, lds;       // blocks, threads per block, dynamic LDS bytes
  int q_begin, q_rows;           // the query rows this launch covers (AttnArgs.q_begin / q_rows of an iv2_pipe launch)
  float lazy;                    // the clamped knob (AttnArgs.lazy)
};
constexpr int GVL_ATTN_MAX_LAUNCHES = 2;

inline int attn_mode_of(const AttnGeometry& g) {
  return g.vl_n ? GVL_ATTN_RAGGED : (g.q_rs || g.q_nw) ? GVL_ATTN_QNORM_V_ROWS : (g.Krows || g.Qrows) ? GVL_ATTN_QKV_ROWS : g.Vrows ? GVL_ATTN_V_ROWS : GVL_ATTN_PAGED;
}
inline bool attn_pitch_ok(int ld, long long width, bool ptr16) { return ld >= width && (ld & 7) == 0 && ptr16; }   // whole rows, 16-byte loads
inline bool attn_tile_below_4g(int ld) { return (unsigned long long)64 * (unsigned long long)ld * 2 < 0xffffffffull; }   // a 64-row tile is addressed with 32-bit byte offsets
// ---- one predicate per operand mode: what the kernels assume of it ----------------------------------------------------------------------------------------------
// Every mode: at most 256 key tiles of 64 (the LDS page-id table holds 256 ids), whole query groups per KV head, 16-byte O stores of Dout <= D elements.
inline bool attn_common_ok(const AttnGeometry& g) {
  return g.B > 0 && g.H > 0 && g.KV > 0 && g.S > 0 && g.S <= 256 * 64 && g.Sk <= 256 * 64 && g.H % g.KV == 0 && g.Dout <= g.D && (g.Dout & 7) == 0 && g.O16;
}
// Paged: a context longer than the queries (extend prefill: query i at position qpos0 + i of Sk >= qpos0 + S keys) lives in pages of a block table; without
// one the pages are the queries' own (Sk = 0 = S keys, qpos0 = 0).
inline bool attn_paged_ok(const AttnGeometry& g) {
  return g.Sk >= 0 && g.qpos0 >= 0 && (g.Sk > 0 ? g.Sk >= g.S + g.qpos0 && g.block_table : g.qpos0 == 0);
}
// V in place (this mode and the two below): V[b][s][kv head][0 .. Dout) = Vrows[(b * S + s) * v_ld + head * Dout + d] -- plain self attention over the S rows
// of the fused-qkv output, so no block table and no longer context; row-major V is the vision towers' mode (head dims 64 and 88), there is no D = 128 form.
inline bool attn_v_rows_ok(const AttnGeometry& g) {
  return g.Vrows && !g.block_table && g.Sk == 0 && g.qpos0 == 0 && attn_pitch_ok(g.v_ld, (long long)g.KV * g.Dout, g.Vrows16) && attn_tile_below_4g(g.v_ld) && g.D != 128;
}
// q, k, v in place (CLIP): q and k need no per-token transform, so they are read as token rows too -- both or neither; unpadded 64-wide heads only.
inline bool attn_qkv_rows_ok(const AttnGeometry& g) {
  return attn_v_rows_ok(g) && g.Qrows && g.Krows && g.D == 64 && g.Dout == g.D && attn_pitch_ok(g.k_ld, (long long)g.KV * g.D, g.Krows16) &&
         attn_pitch_ok(g.q_ld, (long long)g.H * g.D, g.Qrows16) && attn_tile_below_4g(g.k_ld);
}
// q normalised on load + V in place (InternVideo2): q'[d] = q_nw[head * Dout + d] * bf16(q[d] * q_rs[token]) -- row scale and norm weight come together; K
// stays in pages, whose pad column Dout must hold 1.0 (k_ones): the mode folds the softmax shift into the S^T MFMAs.  88-wide heads padded to 96 only.
inline bool attn_qnorm_v_rows_ok(const AttnGeometry& g) {
  return attn_v_rows_ok(g) && g.q_rs && g.q_nw && g.Qrows && !g.Krows && g.D == 96 && g.Dout == 88 && g.k_ones && attn_pitch_ok(g.q_ld, (long long)g.H * g.Dout, g.Qrows16 && g.q_nw16);
}
// Ragged causal prefill: one grid for all sequences of the group -- B = 1, sequence u owns rows [vl_rows[u], vl_rows[u + 1]) (not empty, at most S = the longest)
// and the block table vl_tables[u]; paged K / V only, no extend, and the per-batch block table is replaced by the per-sequence ones.
inline bool attn_ragged_ok(const AttnGeometry& g) {
  if (g.vl_n < 1 || g.vl_n > GVL_MAX_PREFILL_BATCH || g.B != 1 || !g.causal || g.Sk || g.qpos0 || g.Vrows || g.Qrows || g.Krows || g.q_rs || g.q_nw || g.block_table) return false;
  for (int u = 0; u < g.vl_n; ++u)
    if (!g.vl_tables[u] || g.vl_rows[u + 1] <= g.vl_rows[u] || g.vl_rows[u + 1] - g.vl_rows[u] > g.S) return false;
  return true;
}

// Returns the number of launches written to out (1 or 2: their query rows cover [0, S) exactly once, in launch order), or -1: the arguments are not served
// (that includes a grid of more than 2^31 - 1 blocks).
inline int attn_plan(const AttnGeometry& g, const AttnKnobs& k, AttnLaunch out[GVL_ATTN_MAX_LAUNCHES]) {
  if (g.D != 64 && g.D != 96 && g.D != 128) return -1;
  if (!attn_common_ok(g)) return -1;
  const int mode = attn_mode_of(g);
  switch (mode) {
    case GVL_ATTN_PAGED: if (!attn_paged_ok(g)) return -1; break;
    case GVL_ATTN_V_ROWS: if (!attn_v_rows_ok(g)) return -1; break;
    case GVL_ATTN_QKV_ROWS: if (!attn_qkv_rows_ok(g)) return -1; break;
    case GVL_ATTN_QNORM_V_ROWS: if (!attn_qnorm_v_rows_ok(g)) return -1; break;
    default: if (!attn_ragged_ok(g)) return -1; break;
  }
  const float lazy = k.lazy >= 0.f && k.lazy <= 64.f ? k.lazy : GVL_ATTN_KNOBS_DEFAULT.lazy;
  const long long groups8 = (((long long)g.KV * g.B + 7) / 8) * 8;      // (KV head, batch) pairs, padded to the 8 XCDs
  const int vrow = mode == GVL_ATTN_RAGGED ? 0 : mode, vl = mode == GVL_ATTN_RAGGED;
  // ONES forms (D = 96 only): the P.V MFMAs deliver the softmax row sum in O^T[Dout] when the V^T pad row Dout holds 1.0 and sits in the first half of its 8-row group
  const int lr = g.Dout - 64;
  const bool ones = g.D == 96 && !vl && g.ones_row && !k.no_ones && g.Dout < 96 && lr >= 0 && (lr & 7) < 4 && !g.causal;

  if (mode == GVL_ATTN_QNORM_V_ROWS && ones && g.pipe && g.H == g.KV) {
    // The hand-placed pipelined loop (round 4), bit-identical to attn_fwd_kernel<96, 4, 2, 1, 3>.  pipe_rows == 256 (gvl_debug_set "attn_pipe_rows", tests / A-B):
    // whole 256-row query blocks go to the 8-wave form (half the DMA pieces per MFMA), the remaining rows (S = 2049: one) to the 4-wave form in a second launch.
    // MEASURED SLOWER and therefore not the default: 106.5-106.8 against 95.3-95.9 ms per 39 launches, same box (profiles/r04_attention_pipe_lab.txt) -- eight
    // waves in lock-step behind one barrier and one block per CU lose more than the halved DMA issue gives back (round 2 saw the same with 6-wave blocks).
    // A row's arithmetic does not depend on which form computes it (asserted): the 8-wave form votes its safe re-pass per 128-row half of a block.
    const int lds = 2 * 2 * 64 * 96 * 2 + 64 * 96 * 2;                   // the ring + the partial-last-tile V slot: 60 KB
    const int rows8 = g.pipe_rows == 256 ? (g.S / 256) * 256 : 0;
    int n = 0;
    for (int nw = 8; nw >= 4; nw -= 4) {
      const int q_begin = nw == 8 ? 0 : rows8, q_rows = nw == 8 ? rows8 : g.S - rows8;
      if (q_rows <= 0) continue;
      const long long grid = groups8 * ((q_rows + 32 * nw - 1) / (32 * nw));
      if (grid > 0x7fffffffll) return -1;
      out[n++] = AttnLaunch{mode, GVL_ATTN_IV2_PIPE, 96, nw, 2, 1, 3, 0, (unsigned)grid, 64 * nw, lds, q_begin, q_rows, lazy};
    }
    return n;
  }
  // Ring depth 2: 48 KB (D = 96) -> 3 blocks / CU at 151 VGPRs (measured 427 us vs 461 us for the 73 KB depth-3 ring, which caps residency at 2 blocks / CU; DMA
  // latency is not the limiter -- PMC shows the kernel is VALU-issue-bound).  Depth 3 on request (AttnArgs.ring), paged operands only; no ONES / D = 64 / ragged form.
  // (192-query blocks of 6 waves -- 3 % instead of 5.9 % tail waste at S = 2049, K/V tiles shared by more waves -- measured 24.6 ms of attention per clip
  //  against 18.0: two 98 KB blocks per CU hide less latency than three 49 KB ones.  Round 2, dropped.)
  const int ns = g.ring == 3 && mode == GVL_ATTN_PAGED && g.D != 64 && !ones ? 3 : 2;
  const int nwaves = 4, rows = 32 * nwaves;                              // query rows per block
  long long nq = (g.S + rows - 1) / rows;
  if (vl) { nq = 0; for (int u = 0; u < g.vl_n; ++u) nq += (g.vl_rows[u + 1] - g.vl_rows[u] + rows - 1) / rows; }
  const long long grid = groups8 * (g.H / g.KV) * nq;
  if (grid > 0x7fffffffll) return -1;
  out[0] = AttnLaunch{mode, GVL_ATTN_FWD, g.D, nwaves, ns, ones, vrow, vl, (unsigned)grid, 64 * nwaves, ns * 2 * 64 * g.D * 2 + 1024 /* ring + page-id table (256 pages) */,
                      0, g.S, lazy};
  return 1;
}

// =================================================================================================================================================================
// ragged EXTEND prefill (gvl_prefill_extend_varlen): the ragged form with a cached prefix per sequence
// =================================================================================================================================================================
// One causal grid for vl_n sequences packed back to back; sequence u already holds vl_pos0[u] tokens (whole pages: a multiple of 64, 0 = empty), its S_u = vl_rows[u + 1] -
// vl_rows[u] queries sit at positions vl_pos0[u] + i and see the vl_pos0[u] + S_u keys of vl_tables[u].  attn_fwd_kernel<D, NWAVES, NS, 0, 0, 2>: the VL = 1 decode of
// (sequence, query block) plus that sequence's own qpos0 / Sk, after which it is the single-sequence extend kernel -- bit-identical per row to a launch of its sequence alone.
// Paged K / V only; grid, block and LDS are the ragged form's formulas.  A list of its own (the four above are pinned by recorded plans): a new form = one entry + one rule here.
//   X(D, NWAVES, NS)
#define GVL_ATTN_EXT_LIST(X) X(64, 4, 2) X(96, 4, 2) X(128, 4, 2)
constexpr int attn_ext_key(int D, int NWAVES, int NS) { return (D * 16 + NWAVES) * 4 + NS; }

struct AttnExtGeometry {         // only what the decision reads
  int H, KV, D, Dout, causal;
  int vl_n, vl_rows[GVL_MAX_PREFILL_BATCH + 1], vl_pos0[GVL_MAX_PREFILL_BATCH];
  bool vl_tables[GVL_MAX_PREFILL_BATCH];   // which block tables are present
  bool O16;                                // 16-byte alignment of O
};
struct AttnExtLaunch {
  int D, NWAVES, NS;             // template arguments (ONES = VROW = 0, VL = 2)
  unsigned grid; int block, lds; // blocks, threads per block, dynamic LDS bytes
  float lazy;                    // the clamped knob (AttnArgs.lazy)
};
// What the kernel assumes: whole query groups per KV head, 16-byte O stores, causal, and per sequence a table, at least one query, a prefix of whole pages and at most
// 256 key tiles (the LDS page-id table) -- every member checked, a refusal names no member.
inline bool attn_ext_ok(const AttnExtGeometry& g) {
  if (g.H <= 0 || g.KV <= 0 || g.H % g.KV || g.Dout <= 0 || g.Dout > g.D || (g.Dout & 7) || !g.O16 || !g.causal) return false;
  if (g.vl_n < 1 || g.vl_n > GVL_MAX_PREFILL_BATCH || g.vl_rows[0] != 0) return false;
  for (int u = 0; u < g.vl_n; ++u) {
    const long long S = (long long)g.vl_rows[u + 1] - g.vl_rows[u];
    if (!g.vl_tables[u] || S <= 0 || g.vl_pos0[u] < 0 || (g.vl_pos0[u] & 63) || g.vl_pos0[u] + S > 256 * 64) return false;
  }
  return true;
}
// Returns 0, or -1: the arguments are not served (that includes a grid of more than 2^31 - 1 blocks).
inline int attn_ext_plan(const AttnExtGeometry& g, const AttnKnobs& k, AttnExtLaunch* out) {
  if (g.D != 64 && g.D != 96 && g.D != 128) return -1;
  if (!attn_ext_ok(g)) return -1;
  const int nwaves = 4, rows = 32 * nwaves, ns = 2;                       // as the ragged form: query rows per block, ring depth 2
  const long long groups8 = (((long long)g.KV + 7) / 8) * 8;              // KV heads, padded to the 8 XCDs
  long long nq = 0;
  for (int u = 0; u < g.vl_n; ++u) nq += (g.vl_rows[u + 1] - g.vl_rows[u] + rows - 1) / rows;
  const long long grid = groups8 * (g.H / g.KV) * nq;
  if (grid > 0x7fffffffll) return -1;
  *out = AttnExtLaunch{g.D, nwaves, ns, (unsigned)grid, 64 * nwaves, ns * 2 * 64 * g.D * 2 + 1024 /* ring + page-id table (256 pages) */,
                       k.lazy >= 0.f && k.lazy <= 64.f ? k.lazy : GVL_ATTN_KNOBS_DEFAULT.lazy};
  return 0;
}

// =================================================================================================================================================================
// decode attention
// =================================================================================================================================================================
enum DecodeAttnFamily : int { GVL_DECODE_ATTN_GQA = 0, GVL_DECODE_ATTN_HEAD };   // decode_attn_gqa_kernel<D, GM, STG> / decode_attn_kernel<D, 1, PH>
//   X(D, GM, STG): GM = MFMA rows that hold heads (4: up to 4 heads per block, 16: up to 16); STG = 1: pages staged through LDS (power-of-two rows only: the
//   two D = 96 entries are never planned -- the launcher this plan replaced compiled them all the same, and the list keeps the code object as it was)
#define GVL_DECODE_ATTN_GQA_LIST(X) \
  X(64, 4, 1) X(64, 16, 1) X(64, 4, 0) X(64, 16, 0) X(96, 4, 1) X(96, 16, 1) X(96, 4, 0) X(96, 16, 0) X(128, 4, 1) X(128, 16, 1) X(128, 4, 0) X(128, 16, 0)
//   X(D, PH): PH = 0 one query head per KV head, grid (H, gsplit, batch); 1 the XCD-aware grid for groups; 2 the round-1 grid for groups (LAB)
#define GVL_DECODE_ATTN_HEAD_LIST(X) X(64, 0) X(64, 1) X(64, 2) X(96, 0) X(96, 1) X(96, 2) X(128, 0) X(128, 1) X(128, 2)
constexpr int decode_attn_key(int D, int a, int b) { return (D * 32 + a) * 4 + b; }

struct DecodeAttnGeometry { int H, KV, D, nsplit, batch, hpb, cpb, gsplit; };   // DecodeAttnArgs' integers that the decision reads, as the caller passed them
struct DecodeAttnKnobs {         // LAB, A/B
  bool no_gqa;                   // GVL_DECODE_ATTN_NOGQA: the round-1 grid for grouped-query models
  bool gqa_valu;                 // GVL_DECODE_ATTN_GQA_VALU: the per-head VALU kernel on the XCD-aware grid
  bool gqa_direct;               // GVL_DECODE_ATTN_GQA_DIRECT: MFMA operands straight from global memory
};
constexpr DecodeAttnKnobs GVL_DECODE_ATTN_KNOBS_DEFAULT = {false, false, false};
struct DecodeAttnLaunch {
  int batch, cpb, gsplit, hpb;   // normalised: what the kernel gets (hpb: normalised for the GQA family only, the other one does not read it)
  int family;                    // DecodeAttnFamily
  int D, t1, t2;                 // template arguments: (D, GM, STG) or (D, PH) with t2 = 0
  unsigned grid_x, grid_y, grid_z;   // 256 threads per block, no dynamic LDS
};

// Returns 0, or -1: the arguments are not served (that includes a grid of more than 2^31 - 1 blocks).
inline int decode_attn_plan(const DecodeAttnGeometry& g, const DecodeAttnKnobs& k, DecodeAttnLaunch* out) {
  DecodeAttnLaunch l{};
  l.batch = g.batch <= 0 ? 1 : g.batch;                                   // 0 = one sequence
  if (l.batch > GVL_MAX_DECODE_BATCH) return -1;
  if (g.H <= 0 || g.KV <= 0 || g.H % g.KV) return -1;
  l.cpb = g.cpb < 1 ? 1 : g.cpb;                                           // consecutive splits per block; 0 = 1
  if (g.nsplit < 1 || g.nsplit > 16) return -1;                            // the merge buffers hold 16 partial records
  l.gsplit = g.gsplit <= 0 || g.gsplit > g.nsplit ? (g.nsplit + l.cpb - 1) / l.cpb : g.gsplit;   // block slots along the context; 0 (or nonsense) = every split
  if (g.D != 64 && g.D != 96 && g.D != 128) return -1;
  l.D = g.D; l.hpb = g.hpb;
  const int G = g.H / g.KV;
  long long gx, gy = 1, gz = 1;
  if (G > 1 && G <= 16 && !k.no_gqa && !k.gqa_valu) {                      // one block serves hpb heads of a group on the matrix pipe (16 MFMA rows)
    if (l.hpb < 1 || l.hpb > G || G % l.hpb) l.hpb = G;                    // heads per block: 0 (or no divisor of G) = the whole group
    l.family = GVL_DECODE_ATTN_GQA;
    l.t1 = l.hpb <= 4 ? 4 : 16;
    l.t2 = !(k.gqa_direct || (g.D & (g.D - 1)) != 0);                      // the staged tiles need power-of-two rows (64 / 128)
    gx = (long long)(g.H / l.hpb) * l.gsplit * l.batch;
  } else {
    l.family = GVL_DECODE_ATTN_HEAD;
    l.t1 = G == 1 ? 0 : k.no_gqa ? 2 : 1;
    if (l.t1 == 1) { gx = 8; gy = ((long long)g.KV * l.gsplit * l.batch + 7) / 8 * G; }   // unit (KV head, split, sequence) = (y / G) * 8 + x: a group shares one XCD's L2
    else { gx = g.H; gy = l.gsplit; gz = l.batch; }
  }
  if (gx * gy * gz > 0x7fffffffll) return -1;
  l.grid_x = (unsigned)gx; l.grid_y = (unsigned)gy; l.grid_z = (unsigned)gz;
  *out = l;
  return 0;
}

// The decode step's launch shape.  A sequence always uses one context split per 4 pages of ITS OWN length and one partial per split (its arithmetic never
// depends on the batch); how many block slots the grid offers (gsplit) and how many consecutive splits one block works through (cpb) are free.  cpb stays 1:
// letting a block amortise its publish -> ticket tail over 8 / 16 pages was measured neutral to slower (Phi-3.5, 3.5 k context, 16 sequences: 2631 tok/s at
// cpb 1, 2613 at 2, 2574 at 4; one sequence: 455 / 445 / 408) -- at 5.5 TB/s over pages scattered through a 244 GB pool the page reads, not the tail, are the
// limit.  force_cpb / force_hpb: gvl_debug_set("decode_attn_cpb" / "decode_attn_hpb"), tests vary these result-neutral launch parameters (0 = none).
// positions[b] = index of sequence b's new token (its cache then holds positions[b] + 1 tokens).  Under stream capture the shape must stay valid for later
// steps, whatever the positions are by then: every slot, one split per block, the launcher's choice of heads per block.
struct DecodeAttnShape { int gsplit, cpb, hpb; };
inline DecodeAttnShape decode_attn_shape(const int* positions, int B, int H, int KV, int nsplit, int force_cpb, int force_hpb, bool capturing) {
  DecodeAttnShape s{nsplit, 1, 0};
  if (capturing) return s;
  if (force_cpb >= 1 && force_cpb <= 16) s.cpb = force_cpb;
  long splits = 0;                                                         // blocks along the context, summed over the sequences
  s.gsplit = 1;
  for (int b = 0; b < B; ++b) {
    const int np = (positions[b] + 1 + 63) >> 6, n = (np + 3) >> 2;
    const int ns = n < 1 ? 1 : (n > nsplit ? nsplit : n), blocks = (ns + s.cpb - 1) / s.cpb;
    s.gsplit = blocks > s.gsplit ? blocks : s.gsplit;
    splits += blocks;
  }
  // grouped-query models: the whole group per block when that still gives >= ~1.5 blocks per CU, else fewer heads per block
  // (measured, Llama-3-8B at 3.5 k context: one sequence 268 / 278 / 273 tok/s at 4 / 2 / 1 heads per block, two sequences 520 / 525)
  const int G = H / KV;
  if (G > 1) {
    s.hpb = G;
    while (s.hpb > 2 && s.hpb % 2 == 0 && (long)(H / s.hpb) * splits < 400) s.hpb >>= 1;
    if (s.hpb == 2 && (long)(H / 2) * splits < 200) s.hpb = 1;
    if (force_hpb >= 1 && G % force_hpb == 0) s.hpb = force_hpb;
  }
  return s;
}
