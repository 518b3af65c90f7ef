// gvl_decode_plan.h -- which launches ONE decode step takes, and what each projection reads: a PURE host function of the group's size, the model's geometry and one knob.
// Host-only: no HIP header, no statics, no environment -- any C++17 compiler builds it (tests/c/decode_plan_dump.cc does, and tests/test_decode_plan_cpu.py pins
// every decision against recorded ones).  The batched forms are bit-identical to the single-sequence ones and the fused-RMSNorm form differs from the unfused one in
// rounding only, so no RESULT test can notice a model that silently lost a form: this file is what says which launches ran.  decode_step (gvl_llm.hip) = plan, then
// walk; the geometry predicates that choose the path (gvl_create, gvl_finalize_weights), the batch sizes a step admits and the cut of n sequences into steps
// (gvl_decode_greedy_batch, gvl_decode_steps, decode_group, gvl_beam_search) are written here and nowhere else.
#pragma once
#include "gvl_limits.h"

// ---- the path ------------------------------------------------------------------------------------------------------------------------------------------------------
// The skinny-GEMM (MFMA) decode path needs every projection's K to split over 8 waves x 32-wide MFMA steps, and rows that one wave normalises; any other geometry
// decodes on the VALU GEMV.  (The GVL_DECODE_VALU lab override is gvl_create's business: it ANDs its own bool with this.)
inline bool decode_mfma_ok(int hidden, int inter, int heads, int head_dim) {
  return hidden % 256 == 0 && inter % 256 == 0 && (heads * head_dim) % 256 == 0 && hidden <= 4096 && (head_dim & 1) == 0;
}
// A quantised weight format (1 = FP8 e4m3, 2 = MXFP4; 0 = bf16: always fine) needs wider multiples of every K -- on the MFMA path, which the caller checks.
inline bool decode_quant_ok(int fmt, int hidden, int inter, int attn_width) {
  const int mult = fmt == 2 ? 1024 : 512;
  return fmt == 0 || (hidden % mult == 0 && inter % mult == 0 && attn_width % mult == 0);
}
// Fused RMSNorm on the decode path ("rs"): o_proj / down_proj leave partial sums of squares of the new residual rows (one per 16 columns) and a raw tile-order copy;
// qkv (layers >= 1) / gate_up / lm_head run on that copy with the norm weight folded into their tile-order weights.  bf16 weights only; the consumer's epilogue waves sum
// hidden / 16 partials, 32 at a time, 256 at the most.  (hidden = 256: 16 partials -- no rs; 512 is the smallest hidden that has it.)
inline bool decode_rs_ok(bool mfma, int fmt, bool norm_fused, bool folded, int hidden) {
  const int nblk = hidden >> 4;
  return mfma && !fmt && norm_fused && folded && hidden % 64 == 0 && (nblk & 31) == 0 && nblk <= 256;
}

// ---- batch admission and grouping ------------------------------------------------------------------------------------------------------------------------------------
// The sizes ONE step takes: 1 .. 16 on the MFMA path (the 16 columns of the MFMA B operand), 1 / 2 / 4 on the VALU path (vectors the GEMV holds in LDS).
inline bool decode_batch_ok(bool mfma, int B) { return mfma ? (B >= 1 && B <= GVL_MAX_DECODE_BATCH) : (B == 1 || B == 2 || B == 4); }
// the largest admitted size for `left` waiting sequences
inline int decode_group_size(bool mfma, int left) {
  if (mfma) return left < GVL_MAX_DECODE_BATCH ? left : GVL_MAX_DECODE_BATCH;
  return left >= 4 ? 4 : (left >= 2 ? 2 : 1);
}
// n waiting sequences, in order, as the sizes of the steps that take them (three survivors on the VALU path run as 2 + 1): sizes[] holds up to n, returns how many
inline int decode_parts(bool mfma, int n, int* sizes) {
  int k = 0;
  for (int o = 0; o < n; o += sizes[k++]) sizes[k] = decode_group_size(mfma, n - o);
  return k;
}
// The same cut when some of the waiting sequences lead a guided PAIR (gvl_seq_set_guidance): unit i takes rows[i] rows of a step -- 1 for a plain sequence, 2 for a
// leader, whose follower rides in the same step -- and a unit is never split.  In order, each step takes the longest run of units whose row total is an admitted size:
// up to 16 rows (8 pairs, or any mix) on the MFMA path; 1 / 2 / 4 rows on the VALU path, where a pair and a plain sequence run as 2 + 1.  units[] holds up to n counts of
// UNITS per step, returns how many.  With every rows[i] == 1 the cut is decode_parts'.  (A unit of 2 is itself admitted on both paths, so every step takes at least one.)
inline int decode_parts_paired(bool mfma, const int* rows, int n, int* units) {
  int k = 0;
  for (int o = 0; o < n; o += units[k++]) {
    int best = 1, total = 0;
    for (int j = o; j < n && total + rows[j] <= GVL_MAX_DECODE_BATCH; ++j) {
      total += rows[j];
      if (decode_batch_ok(mfma, total)) best = j - o + 1;
    }
    units[k] = best;
  }
  return k;
}

// ---- the step ---------------------------------------------------------------------------------------------------------------------------------------------------------
enum DecodeProj : int { GVL_DPROJ_QKV0 = 0, GVL_DPROJ_QKV, GVL_DPROJ_O, GVL_DPROJ_GATE_UP, GVL_DPROJ_DOWN, GVL_DPROJ_HEAD, GVL_DPROJ_KINDS };   // QKV0: layer 0's, QKV: later layers'
enum DecodeLauncher : int { GVL_DLAUNCH_GEMV = 0, GVL_DLAUNCH_DGEMM };                   // gvl_launch_gemv (VALU), gvl_launch_dgemm (skinny MFMA GEMM)
enum DecodeWeight : int { GVL_DW_ROW_MAJOR = 0, GVL_DW_TILED, GVL_DW_TILED_FOLDED };    // the prefill's copy; MFMA tile order; tile order with the norm weight folded in
enum DecodeInput : int {
  GVL_DIN_X_NORM = 0,   // d_x, normalised inside the consumer (GemvArgs.norm_w)
  GVL_DIN_XN,           // d_xn: a launch in front has normalised it
  GVL_DIN_XT_SQ,        // d_xt, the raw tile-order copy, with the partial sums of squares (GemvArgs.sq_in)
  GVL_DIN_ATTN,         // d_attn (o_proj)
  GVL_DIN_ACT,          // d_act (down_proj)
};
struct DecodeProjPlan {
  int launcher, weight;   // DecodeLauncher, DecodeWeight
  bool scales;            // the quantised format and its scales go with the weight (GemvArgs.w_fp8 / wscale)
  int input;              // DecodeInput
  bool sq_out;            // it leaves partial sums of squares and the raw tile-order copy of its output rows (GemvArgs.sq_out / out_tiled2)
  bool out_tiled;         // its output is written in B-operand tile order (GemvArgs.out_tiled)
};
enum DecodeRefusal : int { GVL_DECODE_BAD_BATCH = -1 };
inline const char* decode_refusal_reason(int rc) { return rc == GVL_DECODE_BAD_BATCH ? "decode_step: unsupported batch" : ""; }

struct DecodeGeometry {   // only what the decision reads
  int B, layers, hidden;
  bool mfma;              // the path (ctx->decode_mfma)
  int fmt;                // format of the decode weight copies: 0 bf16, 1 FP8, 2 MXFP4
  bool folded;            // the norm-folded tile copies exist
};
struct DecodeKnobs { bool norm_fused; };   // gvl_debug_set

struct DecodePlan {
  bool embed_norm;        // the step starts with gather + layer 0's input norm in one launch (gvl_launch_embed_norm); false: the token rows are gathered only
  DecodeProjPlan proj[GVL_DPROJ_KINDS];
  bool attn_out_tiled;    // decode attention writes d_attn in B-operand tile order (o_proj reads it so on the MFMA path)
  bool norm_launches;     // a layer's two separate norm launches run: after o_proj (ln2), and after down_proj (the next layer's ln1, or the final norm)
  int n_gemv, n_attn;     // launches of one step booked as GVL_PROF_GEMV / GVL_PROF_DECODE_ATTN
  int n_other;            // GVL_PROF_OTHER launches in front of token selection (whose own launches are not the plan's)
};

// Returns 0, or a DecodeRefusal (decode_refusal_reason says why).  B enters through admission and B <= GVL_MAX_VALU_BATCH only.
inline int decode_plan(const DecodeGeometry& g, const DecodeKnobs& k, DecodePlan* out) {
  if (!decode_batch_ok(g.mfma, g.B)) return GVL_DECODE_BAD_BATCH;
  // RMSNorm in front of qkv / gate_up / lm_head: groups of <= 4 normalise inside the consumer (LDS, like the VALU kernel); larger groups run one norm launch per
  // projection, whose output every block of the consumer shares.  With rs neither happens -- except for layer 0's qkv, whose input no projection produced.
  const bool in_consumer = !g.mfma || g.B <= GVL_MAX_VALU_BATCH;
  const bool rs = decode_rs_ok(g.mfma, g.fmt, k.norm_fused, g.folded, g.hidden);
  DecodePlan p{};
  const DecodeProjPlan plain{g.mfma ? GVL_DLAUNCH_DGEMM : GVL_DLAUNCH_GEMV, g.mfma ? GVL_DW_TILED : GVL_DW_ROW_MAJOR, g.mfma && g.fmt != 0, 0, false, false};
  DecodeProjPlan normed = plain, consumer = plain, producer = plain;
  normed.input = in_consumer ? GVL_DIN_X_NORM : GVL_DIN_XN;
  if (rs) { consumer.weight = GVL_DW_TILED_FOLDED; consumer.input = GVL_DIN_XT_SQ; } else consumer.input = normed.input;
  producer.sq_out = rs;
  p.proj[GVL_DPROJ_QKV0] = normed;
  p.proj[GVL_DPROJ_QKV] = p.proj[GVL_DPROJ_GATE_UP] = p.proj[GVL_DPROJ_HEAD] = consumer;
  p.proj[GVL_DPROJ_O] = p.proj[GVL_DPROJ_DOWN] = producer;
  p.proj[GVL_DPROJ_O].input = GVL_DIN_ATTN;
  p.proj[GVL_DPROJ_DOWN].input = GVL_DIN_ACT;
  p.proj[GVL_DPROJ_GATE_UP].out_tiled = p.attn_out_tiled = g.mfma;   // d_act and d_attn feed a skinny GEMM
  p.embed_norm = !in_consumer;
  p.norm_launches = !in_consumer && !rs;
  p.n_gemv = 4 * g.layers + 1;
  p.n_attn = g.layers;
  p.n_other = 1 + (p.norm_launches ? 2 * g.layers : 0);
  *out = p;
  return 0;
}
