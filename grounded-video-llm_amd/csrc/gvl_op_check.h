// gvl_op_check.h -- what the six descriptor entries of the operator level (gvl_op_patch_embed, gvl_op_decode_proj, gvl_op_decode_attention, gvl_op_qkv_post,
// gvl_op_prefill_attention, gvl_op_iv2_attention; include/gvl.h) refuse.  Host-only, no HIP: tests/c/op_check.cc drives it on a CPU, tests/test_op_check_cpu.py holds it
// to the refusals recorded in tests/golden/op_refusals.json and to the rules of include/gvl.h written out once more.
// Per entry: check_<entry>(descriptor) decides everything the descriptor alone decides (the launch plans and the pointers' alignment included); the four entries whose
// kernels trust positions and page numbers then read pos and the block tables back (gvl_ops.hip) and hand the HOST copies to tables_<entry>, which is ONE walk
// (walk_tables) over what each member reads or writes.  Both return the text behind "gvl_op_<entry>: " or null; every such text lives here and nowhere else.
// The admitted path allocates nothing (gvl_op_qkv_post's once-only page marks excepted).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/gvl.h"
#include "gvl_limits.h"
#include "gvl_attn_plan.h"
#include "gvl_decode_plan.h"

namespace gvl_op {

enum { ACT_NONE = 0, ACT_SILU_MUL = 3 };   // gvl_internal.h's GVL_ACT_* (gvl_ops.hip asserts that they agree)

constexpr char kPatchNotFused[] = "geometry outside the fused kernel";   // gvl_launch_patch_embed's own refusal reads the same
// what two entries say in the same words
constexpr char kBatch[] = "1 <= batch <= 16", kMembers[] = "0 <= vl_n <= 8", kPosition[] = "position outside the tables";

inline bool al16(const void* q) { return ((uintptr_t)q & 15) == 0; }

// ---- the table walk --------------------------------------------------------------------------------------------------------------------------------------------------
// One member of a launch: `bad` (a refusal of the member's own position or length, found by its entry) or the tiles [t0, t1) it reads or writes -- tile t on page
// tab[t] of its table of `len` entries, or, tab null, on the implicit page page0 + t.
struct Tiles { const char* bad; long long t0, t1; const int* tab; long long len, page0; };
// Members 0 .. n - 1 in order, member(i) -> Tiles; the first refusal is the answer: the member's own, `short_text` for a table that ends before t1, a page outside
// [0, n_pages), and -- `used` (n_pages marks, all zero) given -- a page named twice.
template <class F>
const char* walk_tables(int n, F member, long long n_pages, const char* short_text, char* used) {
  for (int i = 0; i < n; ++i) {
    const Tiles m = member(i);
    if (m.bad) return m.bad;
    if (m.tab && m.t1 > m.len) return short_text;
    for (long long t = m.t0; t < m.t1; ++t) {
      const long long page = m.tab ? m.tab[t] : m.page0 + t;
      if (page < 0 || page >= n_pages) return "page outside the pools";
      if (used) {
        if (used[page]) return "a page named twice among the pages the launch writes";
        used[page] = 1;
      }
    }
  }
  return nullptr;
}
// the tables of a paged launch on the host: the single form's [B][max_pages] (null: implicit pages), or a ragged group's, member by member (null: table_len < 1)
struct HostTables { const int* block; const int* vl[GVL_MAX_PREFILL_BATCH]; };

// ---- gvl_op_patch_embed ----------------------------------------------------------------------------------------------------------------------------------------------
inline const char* check_patch_embed(const gvl_patch_embed& p) {
  if (p.mode != 0 && p.mode != 1) return "mode is 0 (CLIP) or 1 (InternVideo2)";
  if (p.path != 0 && p.path != 1) return "path is 0 (fused) or 1 (three passes)";
  if (p.n <= 0 || p.T <= 0 || p.image <= 0 || p.patch <= 0 || p.C <= 0 || p.Kp <= 0) return "n, T, image, patch, C and Kp must be positive";
  if (p.image % p.patch) return "image must be a multiple of patch";
  if (p.Kp % 8 || p.Kp < 3 * p.patch * p.patch) return "Kp must be a multiple of 8 and hold 3 patch^2 columns";
  if (!p.px || !p.W || !p.cls || !p.pos || !p.out) return "px, W, cls, pos and out are required";
  if (p.mode == 0 && (!p.lnw || !p.lnb)) return "CLIP needs lnw and lnb";
  if (p.mode == 0 && p.T != 1) return "CLIP has one frame per image (T = 1)";
  if (p.mode == 1 && !p.bias) return "InternVideo2 needs the conv bias";
  if (p.path == 0 && p.im2col) return "the fused path forms no im2col matrix";
  if (p.path == 1 && (p.Kp % 64 || p.C % 8 || (p.mode == 0 && p.C > 4096))) return "the three passes need Kp % 64 == 0 and C % 8 == 0 (CLIP: C <= 4096)";
  const int g = p.image / p.patch;
  if ((long)p.n * p.T * g * g > (1l << 30)) return "too many patch rows";
  if (p.path == 0 && (p.C % 16 || p.patch > 16 || (p.patch & 1))) return kPatchNotFused;
  return nullptr;
}

// ---- gvl_op_decode_proj ----------------------------------------------------------------------------------------------------------------------------------------------
inline int decode_proj_out_row(const gvl_decode_proj& p) { return p.act == ACT_SILU_MUL ? p.N / 2 : p.N; }
inline const char* check_decode_proj(const gvl_decode_proj& p) {
  const int N = p.N, K = p.K, B = p.batch;
  if (N <= 0 || K <= 0 || !p.W || !p.x) return "N, K > 0 and W, x set";
  if (B < 1 || B > GVL_MAX_DECODE_BATCH) return kBatch;
  if (p.path < 0 || p.path > 1 || p.w_fmt < 0 || p.w_fmt > 2) return "path 0 / 1, w_fmt 0 / 1 / 2";
  if (K % (p.path == 0 ? 32 : 8)) return "K % 32 == 0 (tile order; the VALU GEMV: K % 8 == 0)";
  if (p.act != ACT_NONE && p.act != ACT_SILU_MUL) return "act is NONE or SILU_MUL";
  if (p.x_is_tiled && (p.norm_w || p.path == 1)) return "a tiled x feeds the skinny GEMM without norm_w only";
  if (p.path == 1 && (p.variant || p.w_fmt || p.out_tiled || p.sq_in || p.sq_out || p.out_tiled2)) return "the VALU GEMV has no variants, quantised weights, tiled outputs or fused-norm sums";
  if (p.out_stride < 0 || (p.out_stride && p.out_stride < decode_proj_out_row(p))) return "out_stride >= the output row length";
  if (!p.rope_on && !p.out_bf16 && !p.out_f32) return "an output buffer";
  if (p.path == 0 && B > 1 && !p.rope_on && (p.out_f32 || p.resid || (p.out_bf16 && !p.out_tiled)) && (p.out_stride ? p.out_stride : decode_proj_out_row(p)) % 4)
    return "out_stride % 4 == 0 for batch > 1 (8- and 16-byte epilogue stores)";
  if (p.rope_on) {
    if (p.H < 1 || p.KV < 1 || p.Dr < 2 || (p.Dr & 1) || p.D < p.Dr || (long)N != (long)(p.H + 2 * p.KV) * p.Dr) return "rope: Dr even, D >= Dr, N == (H + 2 KV) Dr";
    if (!p.cos_s || !p.sin_s || !p.pos || !p.tables || !p.Q || !p.Kt || !p.Vt) return "rope: tables, pos, page tables, Q, Kt, Vt set";
    if (p.rope_switch > 0 && (!p.cos_l || !p.sin_l)) return "rope: long tables set when rope_switch > 0";
    if (p.max_pos < 1 || p.n_pages < 1 || p.table_stride < 1 || p.q_stride < p.H * p.D) return "rope: max_pos, n_pages, table_stride >= 1, q_stride >= H D";
    if (p.act || p.bias || p.resid) return "rope: no other epilogue";
  }
  if (p.path == 0 && p.w_fmt && K % (p.w_fmt == 2 ? 1024 : 512)) return "FP8 needs K % 512 == 0, MXFP4 K % 1024 == 0";
  return nullptr;
}
// rope_on: sequence b writes the one slot of its newest token, on page tables[b][pos[b] / 64]
inline const char* tables_decode_proj(const gvl_decode_proj& p, const int* pos, const int* tables) {
  return walk_tables(p.batch, [&](int b) {
    const long long t = pos[b] >> 6;
    const bool out = pos[b] < 0 || pos[b] >= p.max_pos || t >= p.table_stride;
    return Tiles{out ? kPosition : nullptr, t, t + 1, tables + (size_t)b * p.table_stride, p.table_stride, 0};
  }, p.n_pages, nullptr, nullptr);
}

// ---- gvl_op_decode_attention -----------------------------------------------------------------------------------------------------------------------------------------
inline DecodeAttnGeometry decode_attn_geometry(const gvl_decode_attn& p) { return DecodeAttnGeometry{p.H, p.KV, p.D, p.nsplit, p.batch, p.hpb, p.cpb, p.gsplit}; }
inline const char* check_decode_attention(const gvl_decode_attn& p) {
  DecodeAttnLaunch l;
  if (!p.q || !p.Kt || !p.Vt || !p.tables || !p.pos || !p.part || !p.counters || !p.out) return "q, Kt, Vt, tables, pos, part, counters, out set";
  if (p.batch < 1 || p.batch > GVL_MAX_DECODE_BATCH) return kBatch;
  if (decode_attn_plan(decode_attn_geometry(p), GVL_DECODE_ATTN_KNOBS_DEFAULT, &l) < 0)
    return "the launch plan does not serve this geometry (H % KV == 0, D 64 / 96 / 128, 1 <= nsplit <= 16)";
  if (p.Dout < 1 || p.Dout > p.D) return "1 <= Dout <= D";
  if (p.q_stride < p.H * p.D || (p.q_stride & 7) || !al16(p.q)) return "q_stride >= H D, q rows 16-byte aligned";
  if (!p.out_tiled && p.out_stride < p.H * p.Dout) return "out_stride >= H Dout";
  if (p.n_pages < 1 || p.table_stride < 1) return "n_pages, table_stride >= 1";
  return nullptr;
}
// sequence b reads its first ceil((pos[b] + 1) / 64) pages; then the launch shape against the split count of the longest sequence (one split per 4 pages of its own
// length, at most nsplit).  Behind check_decode_attention: the plan serves the geometry
inline const char* tables_decode_attention(const gvl_decode_attn& p, const int* pos, const int* tables) {
  int longest = 1;
  const char* bad = walk_tables(p.batch, [&](int b) {
    const bool out = pos[b] < 0 || (long long)pos[b] >= (long long)p.table_stride * 64;
    const int np = out ? 0 : (pos[b] + 1 + 63) >> 6, n4 = (np + 3) >> 2, ns = n4 > p.nsplit ? p.nsplit : n4;
    longest = ns > longest ? ns : longest;
    return Tiles{out ? kPosition : nullptr, 0, np, tables + (size_t)b * p.table_stride, p.table_stride, 0};
  }, p.n_pages, nullptr, nullptr);
  if (bad) return bad;
  DecodeAttnLaunch l;
  decode_attn_plan(decode_attn_geometry(p), GVL_DECODE_ATTN_KNOBS_DEFAULT, &l);
  if ((long long)l.gsplit * l.cpb < longest) return "gsplit * cpb is smaller than the longest sequence's split count (the ticket would never complete)";
  return nullptr;
}

// ---- gvl_op_qkv_post -------------------------------------------------------------------------------------------------------------------------------------------------
inline const char* check_qkv_post(const gvl_qkv_post& p) {
  const int n = p.vl_n;
  if (!p.qkv || !p.Kt || (!p.Q && !p.q_rs)) return "qkv, Kt and Q (or q_rs) set";
  if (p.mode < 0 || p.mode > 2) return "mode 0, 1 or 2";
  if (p.H < 1 || p.KV < 1 || p.B < 1 || p.n_pages < 1) return "H, KV, B, n_pages >= 1";
  if ((p.Dr & 7) || (p.mode == 2 && (p.Dr & 15)) || (p.D & 7) || p.D < p.Dr || p.Dr < 8 || p.Dr > 128) return "Dr % 8 == 0 (mode 2: % 16), 8 <= Dr <= 128, D % 8 == 0, D >= Dr";
  if ((p.ld & 7) || (long long)p.ld < (long long)(p.H + 2 * p.KV) * p.Dr) return "ld % 8 == 0, ld >= (H + 2 KV) Dr";
  if (p.mode == 1 && (!p.qn || !p.kn)) return "mode 1 needs qn and kn";
  if (p.mode == 2 && (!p.cos || !p.sin || p.max_pos < 1)) return "mode 2 needs cos, sin and max_pos";
  if (p.q_rs && p.mode != 1) return "q_rs is a mode 1 form";
  if (p.q_rs && !p.k_ones) return "q_rs needs k_ones";
  if ((p.ones_row || p.k_ones) && p.D == p.Dr) return "ones_row / k_ones need D > Dr";
  if (n < 0 || n > GVL_MAX_PREFILL_BATCH) return kMembers;
  if (p.ext && (n < 1 || p.q_rs || !p.Vt)) return "ext needs a ragged group, Vt and no q_rs";
  if (n && (p.mode != 2 || p.B != 1 || p.pos0 != 0 || p.block_table)) return "a ragged group needs mode 2, B == 1, pos0 == 0 and no block_table";
  if (!n && (p.S < 1 || p.pos0 < 0)) return "S >= 1, pos0 >= 0";
  if (!n && p.Vt && (p.pos0 & 63)) return "Vt needs pos0 % 64 == 0 (V^T pages are written whole)";
  if (!n && !p.block_table && p.pos0) return "pos0 > 0 needs a block table";
  if (!n && p.block_table && p.max_pages < 1) return "max_pages >= 1";
  if (n && p.vl_rows[0] != 0) return "vl_rows[0] must be 0";
  for (int u = 0; u < n; ++u) {
    if ((long long)p.vl_rows[u + 1] - p.vl_rows[u] < 1) return "an empty ragged member";
    if (!p.vl_tables[u] || p.table_len[u] < 1) return "every ragged member needs a block table";
    if (p.ext && (p.vl_pos0[u] < 0 || (p.vl_pos0[u] & 63))) return "vl_pos0 must be a multiple of 64";
  }
  return nullptr;
}
// a member WRITES the tiles of its new positions [pos0, pos0 + rows): no page twice.  Mode 2: every position inside the cos / sin tables
inline const char* tables_qkv_post(const gvl_qkv_post& p, const HostTables& h) {
  std::vector<char> used((size_t)p.n_pages, 0);
  const long long nt = ((long long)p.S + 63) >> 6;
  return walk_tables(p.vl_n ? p.vl_n : p.B, [&](int i) {
    const long long pos0 = p.vl_n ? (p.ext ? p.vl_pos0[i] : 0) : p.pos0, end = pos0 + (p.vl_n ? (long long)p.vl_rows[i + 1] - p.vl_rows[i] : p.S);
    Tiles m{p.mode == 2 && end > p.max_pos ? "a position outside the cos / sin tables" : nullptr, pos0 >> 6, (end + 63) >> 6, nullptr, 0, i * nt};
    if (p.vl_n) { m.tab = h.vl[i]; m.len = p.table_len[i]; }
    else if (h.block) { m.tab = h.block + (size_t)i * p.max_pages; m.len = p.max_pages; }
    return m;
  }, p.n_pages, "a block table shorter than ceil((pos0 + S) / 64)", used.data());
}

// ---- gvl_op_prefill_attention ----------------------------------------------------------------------------------------------------------------------------------------
inline const char* check_prefill_attention(const gvl_prefill_attn& p) {
  const int n = p.vl_n;
  if (!p.Q || !p.Kt || !p.Vt || !p.O) return "Q, Kt, Vt, O set";
  if (p.n_pages < 1) return "n_pages >= 1";
  if (n < 0 || n > GVL_MAX_PREFILL_BATCH) return kMembers;
  if (p.ext && n < 1) return "ext needs a ragged group";
  if (!n && (!p.block_table || p.max_pages < 1)) return "the single form needs a block table (implicit pages: gvl_op_attention)";
  if (p.ring != 0 && p.ring != 2 && p.ring != 3) return "ring 0, 2 or 3";
  if (p.ext) {
    AttnExtGeometry g{};
    g.H = p.H; g.KV = p.KV; g.D = p.D; g.Dout = p.Dout; g.causal = p.causal; g.vl_n = n; g.O16 = al16(p.O);
    for (int u = 0; u <= n; ++u) g.vl_rows[u] = p.vl_rows[u];
    for (int u = 0; u < n; ++u) { g.vl_tables[u] = p.vl_tables[u] != nullptr; g.vl_pos0[u] = p.vl_pos0[u]; }
    AttnExtLaunch l;
    if (p.B != 1 || p.Sk || p.qpos0 || p.block_table || attn_ext_plan(g, GVL_ATTN_KNOBS_DEFAULT, &l) < 0)
      return "attn_ext_plan does not serve this launch (causal, B == 1, Sk == qpos0 == 0, no block_table, vl_rows[0] == 0, per member a table, >= 1 query, vl_pos0 % 64 == 0)";
  } else {
    AttnGeometry g{};
    g.B = p.B; g.H = p.H; g.KV = p.KV; g.S = p.S; g.D = p.D; g.Dout = p.Dout; g.Sk = p.Sk; g.qpos0 = p.qpos0; g.causal = p.causal; g.ring = p.ring;
    g.max_pages = p.max_pages; g.vl_n = n; g.block_table = p.block_table != nullptr; g.O16 = al16(p.O);
    for (int u = 0; u <= n; ++u) g.vl_rows[u] = p.vl_rows[u];
    for (int u = 0; u < n; ++u) g.vl_tables[u] = p.vl_tables[u] != nullptr;
    AttnLaunch l[GVL_ATTN_MAX_LAUNCHES];
    if (attn_plan(g, GVL_ATTN_KNOBS_DEFAULT, l) < 0 || (n && p.vl_rows[0] != 0))
      return "attn_plan does not serve this launch (D 64 / 96 / 128, Dout % 8 == 0, H % KV == 0, Sk == 0 or Sk >= qpos0 + S; ragged: causal, B == 1, Sk == qpos0 == 0, no block_table, per member a table and 1 .. S queries)";
  }
  return nullptr;
}
// a sequence READS its key tiles from the first one: causal up to its last query's, else all ceil(Sk / 64)
inline const char* tables_prefill_attention(const gvl_prefill_attn& p, const HostTables& h) {
  return walk_tables(p.vl_n ? p.vl_n : p.B, [&](int i) {
    const long long q0 = p.vl_n ? (p.ext ? p.vl_pos0[i] : 0) : p.qpos0, S = p.vl_n ? (long long)p.vl_rows[i + 1] - p.vl_rows[i] : p.S;
    const long long Sk = p.vl_n ? q0 + S : (p.Sk > 0 ? p.Sk : p.S);
    Tiles m{nullptr, 0, p.causal ? ((q0 + S - 1) >> 6) + 1 : (Sk + 63) >> 6, nullptr, 0, 0};
    if (p.vl_n) { m.bad = p.table_len[i] < 1 ? "table_len >= 1" : nullptr; m.tab = h.vl[i]; m.len = p.table_len[i]; }
    else { m.tab = h.block + (size_t)i * p.max_pages; m.len = p.max_pages; }
    return m;
  }, p.n_pages, "a block table shorter than the key tiles the launch reads", nullptr);
}

// ---- gvl_op_iv2_attention --------------------------------------------------------------------------------------------------------------------------------------------
// the launch's geometry as attn_plan reads it (the operands a form reads in place: V behind q and k in qkv's rows)
inline AttnGeometry iv2_geometry(const gvl_iv2_attn& p) {
  const int f = p.form;
  const uintptr_t Vrows = f ? (uintptr_t)p.qkv + (uintptr_t)2 * p.H * p.Dr * sizeof(uint16_t) : 0;
  AttnGeometry g{};
  g.B = p.B; g.H = p.H; g.KV = p.H; g.S = p.S; g.D = pad_head(p.Dr); g.Dout = p.Dr; g.ones_row = 1;
  g.v_ld = f ? p.ld : 0; g.Vrows = Vrows != 0;
  if (f == 2) { g.k_ones = 1; g.pipe = p.pipe; g.pipe_rows = p.pipe_rows; g.q_ld = p.ld; g.Qrows = p.qkv != nullptr; g.q_rs = p.q_rs != nullptr; g.q_nw = p.q_nw != nullptr; }
  g.O16 = al16(p.out); g.Vrows16 = (Vrows & 15) == 0; g.Qrows16 = f == 2 ? al16(p.qkv) : true; g.Krows16 = true; g.q_nw16 = f == 2 ? al16(p.q_nw) : true;
  return g;
}
inline const char* check_iv2_attention(const gvl_iv2_attn& p) {
  const int f = p.form;
  if (f < 0 || f > 2) return "form 0, 1 or 2";
  if (!p.Kt || !p.out) return "Kt and out set";
  if (f == 0 && (!p.Q || !p.Vt || p.qkv || p.q_rs || p.q_nw)) return "form 0 takes Q, Kt, Vt and no qkv, q_rs, q_nw";
  if (f == 1 && (!p.Q || !p.qkv || p.Vt || p.q_rs || p.q_nw)) return "form 1 takes Q, Kt, qkv and no Vt, q_rs, q_nw";
  if (f == 2 && (!p.qkv || !p.q_rs || !p.q_nw || p.Q || p.Vt)) return "form 2 takes qkv, Kt, q_rs, q_nw and no Q, Vt";
  if (p.B < 1 || p.S < 1 || p.H < 1) return "B, S, H >= 1";
  if ((p.Dr & 7) || p.Dr <= 64 || p.Dr >= 96) return "Dr 72, 80 or 88 (a padded head on the D = 96 kernels: the ones row needs D > Dr)";
  if (f == 2 && p.Dr != 88) return "form 2 needs Dr == 88";
  if (f == 2 && (p.pipe < 0 || p.pipe > 2)) return "pipe 0, 1 or 2";
  if (f == 2 && p.pipe_rows != 0 && p.pipe_rows != 256) return "pipe_rows 0 or 256";
  if (f && ((p.ld & 7) || (long long)p.ld < 3ll * p.H * p.Dr)) return "ld % 8 == 0, ld >= 3 H Dr";
  AttnLaunch l[GVL_ATTN_MAX_LAUNCHES];
  if (attn_plan(iv2_geometry(p), GVL_ATTN_KNOBS_DEFAULT, l) < 0) return "attn_plan does not serve this launch (at most 256 key tiles, out / qkv / q_nw 16-byte aligned, a 64-row tile of qkv below 4 GiB)";
  if (!l[0].ONES) return "the plan chose no ONES kernel for this launch";
  return nullptr;
}

}  // namespace gvl_op
