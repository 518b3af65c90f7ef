// gvl_prefill_plan.h -- which launches a prefill group takes, in which order: a PURE host function of the group's lengths and prefixes and a handful of knobs.
// Host-only: no HIP header, no statics, no environment -- any C++17 compiler builds it (tests/c/prefill_plan_dump.cc does, and tests/test_prefill_plan_cpu.py pins
// every decision against recorded ones).  Every form is bit-identical per row to the single-sequence path by design, so no RESULT test can notice a group that
// silently fell back to per-sequence launches: this file is what says which launches ran.  llm_prefill (gvl_llm.hip) = plan, allocate, walk the plan's steps;
// gvl_prefill_varlen / gvl_prefill_extend_varlen (gvl_model.hip) cut their sequences into groups with prefill_group_size.
#pragma once
#include "gvl_limits.h"

// How the members of a group share a launch (RoPE + KV append + V^T pages = "post", and causal attention):
enum PrefillForm : int {
  GVL_PREFILL_ONE = 0,       // one member, the single-sequence kernels at (pos0, Sk): its own block table
  GVL_PREFILL_BATCHED,       // every member, equal lengths and no prefix: the single-sequence kernels with a batch dimension over ONE [nb][P0] page-id table
  GVL_PREFILL_RAGGED,        // every member, any lengths, no prefix: one grid over rows packed back to back (QkvPostArgs / AttnArgs vl_*), a block table per member
  GVL_PREFILL_RAGGED_EXT,    // as RAGGED with a cached prefix per member (vl_pos0): gvl_launch_qkv_post_ext / gvl_launch_attention_ext
};
enum PrefillStepKind : int { GVL_PREFILL_POST = 0, GVL_PREFILL_ATTN };
enum PrefillLastRows : int {   // where the lm_head reads the members' last rows
  GVL_PREFILL_LAST_STRIDED = 0,   // in place: row S - 1 of every member, S rows apart (one member, or a BATCHED group)
  GVL_PREFILL_LAST_GATHERED,      // copied together first (ragged rows are not equally spaced)
  GVL_PREFILL_LAST_TAIL,          // the rows the last layer's tail left
};
enum PrefillRefusal : int { GVL_PREFILL_BAD_BATCH = -1, GVL_PREFILL_BAD_PREFIX = -2, GVL_PREFILL_LOSS_BEHIND_PREFIX = -3, GVL_PREFILL_LOSS_GROUP = -4, GVL_PREFILL_SCORE_AND_LOSS = -5,
                            GVL_PREFILL_KEEP_HIDDEN_GROUP = -6 };
inline const char* prefill_refusal_reason(int rc) {
  switch (rc) {
    case GVL_PREFILL_BAD_BATCH: return "llm_prefill: batch must be 1 .. 8 sequences";
    case GVL_PREFILL_BAD_PREFIX: return "llm_prefill: a cached prefix is whole pages";
    case GVL_PREFILL_LOSS_BEHIND_PREFIX: return "llm_prefill: no loss tail behind a cached prefix";
    case GVL_PREFILL_LOSS_GROUP: return "llm_prefill: loss tail takes one sequence";
    case GVL_PREFILL_SCORE_AND_LOSS: return "llm_prefill: a score tail and a loss tail exclude each other";
    case GVL_PREFILL_KEEP_HIDDEN_GROUP: return "llm_prefill: a keep-hidden sequence is prefilled alone, from empty, without a loss or score tail";
    default: return "";
  }
}

struct PrefillGeometry {         // only what the decision reads
  int nb, lens[GVL_MAX_PREFILL_BATCH], pos0[GVL_MAX_PREFILL_BATCH];   // members, their new rows, the tokens each already holds (0 = empty)
  int rope_orig_max_pos;         // LongRoPE: short factors for a sequence that ends within it, long factors past it (0 = one table)
  bool long_table;               // the model has a long table
  bool loss;                     // a loss tail is requested (the training forward)
  int page_id_cap;               // page ids one by-value list carries (IntList: 256)
  int hidden, qkv_width, gate_up_width;   // the fused RMSNorm's widths: hidden, (H + 2 KV) * Dr, 2 * inter
  bool fused_weights;            // the norm-folded weights were loaded
  bool score;                    // a score tail is requested (gvl_score_extend_varlen): any group, behind any prefixes.  A value-initialised geometry reads false
  bool keep_hidden;              // the member keeps its hidden states (gvl_seq_keep_hidden): every row's last-layer output is read.  LAST member: value-initialised = false
};
struct PrefillKnobs { int varlen_attn; bool varlen_extend, last_layer_tail, norm_fused; };   // gvl_debug_set

struct PrefillStep {
  int kind, form;                // PrefillStepKind, PrefillForm
  int first, count;              // the members it serves: [first, first + count)
  int B, S;                      // batch dimension and rows per batch entry (RAGGED*: 1 and the longest member)
  int pos0, Sk;                  // ONE: the member's prefix; attention: the keys its queries see (0 = its S own, no prefix).  0 in the other forms (RAGGED_EXT: per member)
  bool use_long;                 // post: the LongRoPE table of this launch
};
constexpr int GVL_PREFILL_MAX_STEPS = 2 * GVL_MAX_PREFILL_BATCH;
struct PrefillPlan {
  int off[GVL_MAX_PREFILL_BATCH + 1], M;   // member b owns rows [off[b], off[b + 1]) of the M packed rows
  bool batched_table;            // the group's page ids go into one [nb][P0] table (the BATCHED form reads it)
  bool nf;                       // fused RMSNorm: the GEMMs leave / consume row statistics
  int n_steps;                   // the launches of ONE layer, in order -- every layer takes the same
  PrefillStep steps[GVL_PREFILL_MAX_STEPS];
  bool tail;                     // the last layer runs its MLP on the members' last rows only
  int last_rows;                 // PrefillLastRows
  int n_chunks, chunks[GVL_MAX_PREFILL_BATCH];   // the lm_head GEMV holds 4, 2 or 1 vectors in LDS: last rows per launch, in order
};

// LongRoPE: short factors up to the original context, long factors past it (modeling_phi3.py:381-385), judged by where a member ENDS.  THE one place that chooses.
inline bool prefill_use_long(const PrefillGeometry& g, int u) { return g.rope_orig_max_pos > 0 && g.long_table && g.pos0[u] + g.lens[u] > g.rope_orig_max_pos; }

// Member u on its own: the ONE steps, and what the flops of a ragged grid are the sum of.
inline PrefillStep prefill_member_step(const PrefillGeometry& g, int kind, int u) {
  const int p = g.pos0[u];
  if (kind == GVL_PREFILL_POST) return PrefillStep{kind, GVL_PREFILL_ONE, u, 1, 1, g.lens[u], p, 0, prefill_use_long(g, u)};
  return PrefillStep{kind, GVL_PREFILL_ONE, u, 1, 1, g.lens[u], p, p ? p + g.lens[u] : 0, false};
}

// Returns 0, or a PrefillRefusal (prefill_refusal_reason says why).  The caller has checked lens[b] > 0.
inline int prefill_plan(const PrefillGeometry& g, const PrefillKnobs& k, PrefillPlan* out) {
  if (g.nb < 1 || g.nb > GVL_MAX_PREFILL_BATCH) return GVL_PREFILL_BAD_BATCH;
  const int nb = g.nb;
  bool ext = false;                                    // some member sits behind a cached prefix
  for (int b = 0; b < nb; ++b) { if (g.pos0[b] < 0 || (g.pos0[b] & 63)) return GVL_PREFILL_BAD_PREFIX; ext = ext || g.pos0[b] != 0; }
  if (g.score && g.loss) return GVL_PREFILL_SCORE_AND_LOSS;
  if (ext && g.loss) return GVL_PREFILL_LOSS_BEHIND_PREFIX;
  if (g.loss && nb != 1) return GVL_PREFILL_LOSS_GROUP;
  if (g.keep_hidden && (nb != 1 || ext || g.loss || g.score)) return GVL_PREFILL_KEEP_HIDDEN_GROUP;
  PrefillPlan p{};
  bool uniform = !ext, same_table = true;              // the batched launch shares one qpos0: empty sequences only.  same_table: one LongRoPE table serves every member
  for (int b = 0; b < nb; ++b) {
    p.off[b + 1] = p.off[b] + g.lens[b];
    uniform = uniform && g.lens[b] == g.lens[0];
    same_table = same_table && prefill_use_long(g, b) == prefill_use_long(g, 0);
  }
  p.M = p.off[nb];
  if (uniform && nb * ((g.lens[0] + 63) / 64) > g.page_id_cap) uniform = false;   // the [nb][P0] table is filled from ONE by-value list of page ids
  p.batched_table = nb > 1 && uniform;
  // fused RMSNorm (see vision_norm_fused_ok, gvl_vision_plan.h): the widths the staged epilogue takes
  p.nf = k.norm_fused && g.hidden % 64 == 0 && g.qkv_width % 16 == 0 && g.gate_up_width % 16 == 0 && g.fused_weights;

  // ---- the steps of one layer --------------------------------------------------------------------------------------------------------------------------------
  // One member, or a BATCHED group: one post, one attention launch.  Otherwise a group is ragged, and the knobs say how much of it shares a launch:
  //  * no prefix, varlen_attn != 0: ONE causal-attention grid over the query blocks of all members (8 launches of ~900 blocks on 768 block slots each -> one of
  //    ~7 000: the causal tail is paid once).  varlen_attn == 1 (default) also runs RoPE / KV append / the V^T pages of the group as ONE launch each (2 launches per
  //    layer instead of 2 per member: HBM-bound passes of 3.5 k rows, 25 + 14 us each); 2 keeps those per member.
  //  * some prefix, varlen_extend: the same two steps with a prefix per member (the *_ext launchers).
  //  * a post launch reads ONE LongRoPE table: a group on both sides of rope_orig_max_pos keeps its posts per member and still shares the attention grid.
  //  * knob off: post(u), attention(u) per member, the single-sequence kernels -- the GEMMs are shared whatever the form.
  // Per member the order is post(u), attn(u); with a shared grid every post comes first.
  auto push = [&p](const PrefillStep& s) { p.steps[p.n_steps++] = s; };
  int longest = 0;
  for (int b = 0; b < nb; ++b) longest = g.lens[b] > longest ? g.lens[b] : longest;
  if (nb == 1 || uniform) {
    for (int kind = GVL_PREFILL_POST; kind <= GVL_PREFILL_ATTN; ++kind) {
      PrefillStep s = prefill_member_step(g, kind, 0);
      if (nb > 1) { s.form = GVL_PREFILL_BATCHED; s.count = s.B = nb; }
      push(s);
    }
  } else {
    const int grid = ext ? (k.varlen_extend ? GVL_PREFILL_RAGGED_EXT : GVL_PREFILL_ONE) : (k.varlen_attn ? GVL_PREFILL_RAGGED : GVL_PREFILL_ONE);
    const bool one_post = grid != GVL_PREFILL_ONE && same_table && (ext || k.varlen_attn == 1);
    if (one_post) push(PrefillStep{GVL_PREFILL_POST, grid, 0, nb, 1, longest, 0, 0, prefill_use_long(g, 0)});
    for (int u = 0; u < nb; ++u) {
      if (!one_post) push(prefill_member_step(g, GVL_PREFILL_POST, u));
      if (grid == GVL_PREFILL_ONE) push(prefill_member_step(g, GVL_PREFILL_ATTN, u));
    }
    if (grid != GVL_PREFILL_ONE) push(PrefillStep{GVL_PREFILL_ATTN, grid, 0, nb, 1, longest, 0, 0, false});
  }

  // LAST layer, no loss request: nothing downstream reads the MLP output of any row but a member's last (the KV cache is complete after the post launches, the
  // lm_head takes last rows only) -- gate_up / down run on the nb last rows alone: -2 x M x hidden x 3 inter flops (2.1 % of the prefill's GEMM work at S = 3.5 k).
  // The gathered row statistics of the fused norm are finished four partial sums at a time.  A score tail reads rows anywhere in the group, so it keeps the full pass
  // (the MLP on scored rows + last rows only is left out on purpose: DESIGN.md 3.9).
  // A keep-hidden member's bank takes the last layer's output of EVERY row: the full pass, whatever the knob says.
  p.tail = !g.loss && !g.score && !g.keep_hidden && k.last_layer_tail && (!p.nf || (g.hidden / 64) % 4 == 0);
  p.last_rows = p.tail ? GVL_PREFILL_LAST_TAIL : (nb == 1 || uniform) ? GVL_PREFILL_LAST_STRIDED : GVL_PREFILL_LAST_GATHERED;
  for (int b0 = 0; b0 < nb; b0 += p.chunks[p.n_chunks - 1]) p.chunks[p.n_chunks++] = nb - b0 >= 4 ? 4 : (nb - b0 >= 2 ? 2 : 1);   // row results do not depend on the chunking
  *out = p;
  return 0;
}

// How many of the next `left` sequences (lens[0 .. left)) form one group: at most `cap`, and as many as fit max_rows packed rows together -- one always goes.
inline int prefill_group_size(const int* lens, int left, int cap, int max_rows) {
  int n = left < cap ? left : cap;
  for (;; --n) {
    long rows = 0;
    for (int b = 0; b < n; ++b) rows += lens[b];
    if (n <= 1 || rows <= max_rows) return n;
  }
}
