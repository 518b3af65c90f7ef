// gvl_llm.hip -- the decoder's launch sequences: ragged / batched prefill (+ the training-forward loss tail), the decode step and its hipGraph replay, the greedy decode
// loop over a group of sequences (host code; the kernels live in gvl_gemm*.hip, gvl_attn.hip, gvl_decode.hip, gvl_elem.hip).  Which launches a prefill group takes is
// decided in gvl_prefill_plan.h, which launches a decode step takes and what its projections read in gvl_decode_plan.h, the decode-attention launch shape in
// gvl_attn_plan.h (all three host-only, tested on the CPU).  Restates (file:line in the reference):
//   LLM             models/modeling_phi3.py:1034-1095,1249-1383,1512-1526 / models/modeling_llama.py:699-760
//   generate()      models/llava_next_video.py:655-661 (greedy; transformers GenerationMixin [ext])
#include "gvl_model.h"
#include "gvl_attn_plan.h"
#include "gvl_prefill_plan.h"

namespace gvlm {

size_t prefill_bytes(const gvl_ctx* c, int S) {
  const gvl_config& f = c->cfg;
  const size_t qkvw = (size_t)(f.heads + 2 * f.kv_heads) * c->l_Dr;
  size_t b = 0;
  b += 2 * al256((size_t)S * f.hidden * 2) + al256((size_t)S * qkvw * 2) + al256((size_t)S * f.heads * c->l_Dr * 2);
  b += al256((size_t)S * f.inter * 2) + al256((size_t)f.heads * S * c->l_D * 2);
  b += al256((size_t)kLossChunk * f.vocab * 2 + kScoreChunk * 12) + al256((size_t)kLossChunk * f.hidden * 2) + 3 * al256((size_t)S * 4);   // loss tail (gvl_forward_loss) / score tail (fp32 rows, pitch rounded up to 4)
  b += al256((size_t)S * ((f.hidden + 63) / 64) * 4) + al256((size_t)S * 4);                                          // fused RMSNorm: row statistics + row scale
  b += (size_t)GVL_MAX_PREFILL_BATCH * (al256((size_t)f.hidden * 2) * 2 + al256((size_t)f.inter * 2) + al256(((f.hidden + 63) / 64) * 4) + 256) + 1024;   // last-layer tail rows
  return b + 4096;
}

// page ids of a batch of equal-length sequences, passed by value to a stream-ordered fill (no host buffer lifetime)
__global__ void fill_ints_kernel(int* dst, const IntList l) { for (int i = threadIdx.x; i < l.n; i += blockDim.x) dst[i] = l.v[i]; }

// A sequence's page ids -> its device block table, by value in the kernel arguments (256 per launch) on the stream that is about to use the table:
// no host -> device copy (the runtime implements small ones as a blit kernel plus a staging buffer) and no host buffer lifetime to respect.
int upload_table(gvl_ctx* ctx, Seq& s, hipStream_t st) {
  if (!s.table_dirty) return 0;
  const int np = (int)s.pages.size();
  for (int p0 = 0; p0 < np; p0 += 256) {
    IntList l; l.n = np - p0 < 256 ? np - p0 : 256;
    for (int i = 0; i < l.n; ++i) l.v[i] = s.pages[p0 + i];
    hipLaunchKernelGGL(fill_ints_kernel, dim3(1), dim3(256), 0, st, s.d_block_table + p0, l);
  }
  if (hipGetLastError() != hipSuccess) return fail(ctx, GVL_ERR_HIP, "block table upload failed");
  s.table_dirty = false;
  return 0;
}

// The next token of every row of `am`: argmax (greedy), or one draw per row when gvl_set_sampling switched sampling on.  When a sequence of the
// group has logits processors (gvl_seq_set_processors), one launch applies them to the rows first; its history is the sequence's output list
// (host-mapped) up to its device-side generation count, so a captured decode step replays with nothing baked in per step.  With every processor
// off the launch sequence is the one without processors.  A sequence's token rules (gvl_seq_set_token_rules) ride in the same launch: it runs
// when a member has processors OR rules OR a grammar (gvl_seq_set_grammar), and with none of them nothing changes.  Sequences with log-probabilities on (gvl_seq_set_logprobs) get them from the same
// launch (a second instantiation of the selection kernel); with every sequence of the group off it is the kernel without them.
// Guided pairs (gvl_seq_set_guidance; `pairs` non-null): am / sqs cover the rows a token is selected for -- the followers' rows are not among them.  ONE guidance launch
// rewrites the leaders' rows first (HF runs classifier-free guidance as the first processor), everything below then applies to the guided rows, and ONE launch behind
// the selection hands every follower its leader's token.  Without pairs neither launch exists and the sequence of launches is the one it was.
static int pick_tokens_rows(gvl_ctx* ctx, ArgmaxArgs& am, Seq* const* sqs, hipStream_t st);
int pick_tokens(gvl_ctx* ctx, ArgmaxArgs& am, Seq* const* sqs, hipStream_t st, const PairLaunches* pairs) {
  if (!pairs) return pick_tokens_rows(ctx, am, sqs, st);
  if (const int rc = gvl_launch_guidance_rows(pairs->g, st)) return rc;
  if (const int rc = pick_tokens_rows(ctx, am, sqs, st)) return rc;
  return gvl_launch_follow_commit(pairs->f, st);
}
int step_rows(gvl_ctx* ctx, Seq* const* named, int n, Seq** rows) {
  int k = 0;
  for (int b = 0; b < n; ++b) rows[k++] = named[b];
  for (int b = 0; b < n; ++b) if (named[b]->follow >= 0) rows[k++] = &ctx->seqs[named[b]->follow];
  return k;
}
int named_parts(gvl_ctx* ctx, Seq* const* named, int n, int* sizes) {
  int rows[gvl_ctx::kMaxSeqs];
  for (int i = 0; i < n; ++i) rows[i] = named[i]->follow >= 0 ? 2 : 1;
  return decode_parts_paired(ctx->decode_mfma, rows, n, sizes);
}
static int pick_tokens_rows(gvl_ctx* ctx, ArgmaxArgs& am, Seq* const* sqs, hipStream_t st) {
  bool any_proc = false;
  for (int b = 0; b < am.batch; ++b) any_proc = any_proc || sqs[b]->sel.proc.on() || sqs[b]->sel.rules >= 0 || sqs[b]->sel.grammar >= 0;
  if (any_proc) {
    LogitsProcArgs lp; memset(&lp, 0, sizeof(lp));
    lp.logits = const_cast<float*>(am.logits); lp.n = am.n; lp.ld = am.n; lp.batch = am.batch;
    lp.cap = ctx->outlist_cap < GVL_LOGITS_HIST_CAP ? ctx->outlist_cap : GVL_LOGITS_HIST_CAP;
    for (int b = 0; b < am.batch; ++b) {
      const LogitsProc& q = sqs[b]->sel.proc;
      lp.hist[b] = sqs[b]->d_out; lp.len_ptrs[b] = sqs[b]->d_ngen;
      lp.penalty[b] = q.penalty; lp.ngram[b] = q.ngram; lp.min_new[b] = q.eos >= 0 ? q.min_new : 0; lp.eos[b] = q.eos;
      lp.rules[b] = sqs[b]->sel.rules >= 0 ? (const TokenRulesDev*)ctx->rule_sets[sqs[b]->sel.rules].d : nullptr;
      lp.grammar[b] = sqs[b]->sel.grammar >= 0 ? (const GrammarDev*)ctx->grammars[sqs[b]->sel.grammar].d : nullptr;
    }
    const int rc = gvl_launch_logits_process(lp, st);
    if (rc) return rc;
  }
  return select_tokens(ctx, am, sqs, st);
}
// the selection alone, on rows that ARE processed already (gvl_seq_fanout selects its siblings' first tokens from the row the source's prefill processed: a second
// application would show -- sequence_bias is not idempotent)
int select_tokens(gvl_ctx* ctx, ArgmaxArgs& am, Seq* const* sqs, hipStream_t st) {
  for (int b = 0; b < am.batch; ++b) {             // log-probabilities (gvl_seq_set_logprobs): the sequence's slot lists, indexed by its device-side count
    const Seq& q = *sqs[b];
    if (q.sel.top_n < 0 || !q.d_lp) continue;
    am.top_n[b] = q.sel.top_n; am.lp_lists[b] = q.d_lp;
    if (q.sel.top_n > 0) { am.top_ids[b] = q.d_top_ids; am.top_lp[b] = q.d_top_lp; }
  }
  // Sampling: a sequence follows the ctx setting unless it has its own (gvl_seq_set_sampling).  With no own setting in the group and none of the warpers past top-p in
  // the ctx setting the launch is exactly the one below, as before; otherwise ONE launch of the per-row kernel selects for every row with that row's setting -- an own
  // setting draws from its own (seed, stream), a follower from (ctx seed, its prefill-order stream), so a row's token does not depend on the group it travels in.
  bool per_row = ctx->sample.warps();
  for (int b = 0; b < am.batch; ++b) per_row = per_row || sqs[b]->sel.own_sampling;
  if (per_row) {
    SelRowsArgs sa; memset(&sa, 0, sizeof(sa)); sa.am = am;
    for (int b = 0; b < am.batch; ++b) {
      SelRow& r = sa.row[b];
      if (sqs[b]->sel.own_sampling) {
        const Sampling& q = sqs[b]->sel.sampling;
        r.on = q.on; r.inv_temp = q.inv_temp; r.top_k = q.top_k; r.top_p = q.top_p; r.min_p = q.min_p; r.typical_p = q.typical_p; r.eps = q.eps; r.eta = q.eta;
        r.seed_lo = (unsigned)q.seed; r.seed_hi = (unsigned)(q.seed >> 32); r.stream = q.stream;
      } else {
        const auto& q = ctx->sample;
        r.on = q.on; r.inv_temp = q.inv_temp; r.top_k = q.top_k; r.top_p = q.top_p; r.min_p = q.min_p; r.typical_p = q.typical_p; r.eps = q.eps; r.eta = q.eta;
        r.seed_lo = (unsigned)q.seed; r.seed_hi = (unsigned)(q.seed >> 32); r.stream = sqs[b]->rng_stream;
      }
    }
    return gvl_launch_select_rows(sa, st);
  }
  if (!ctx->sample.on) return gvl_launch_argmax(am, st);
  am.inv_temp = ctx->sample.inv_temp; am.top_p = ctx->sample.top_p; am.top_k = ctx->sample.top_k;
  am.seed_lo = (unsigned)ctx->sample.seed; am.seed_hi = (unsigned)(ctx->sample.seed >> 32);
  for (int b = 0; b < am.batch; ++b) am.stream[b] = sqs[b]->rng_stream;
  return gvl_launch_sample(am, st);
}

// Prefill of nb = 1 .. 8 sequences together (lens[b] tokens each).  The decoder GEMMs run over the rows of all of them
// (packed back to back, no padding); RoPE / KV append / causal attention run per sequence on its own pages.  Every kernel is
// batch-invariant, so each sequence's result is bit-identical to a prefill on its own.
// pos0s (null = all 0): EXTEND -- sequence b already holds pos0s[b] tokens (a multiple of 64: whole pages, possibly shared with other sequences; 0 = empty); its new
// rows take positions pos0s[b] .. pos0s[b] + lens[b] - 1 and attend to the cached prefix plus themselves.  One sequence: the single-sequence kernels at (qpos0, Sk).
// WHICH launches a group takes -- one per member, one with a batch dimension, one ragged grid, the same behind prefixes -- is prefill_plan's decision
// (gvl_prefill_plan.h: pure, tested on the CPU); this function is plan, allocate, walk.  The GEMMs are shared whatever the form, and every row is bit-identical to the
// sequence's own prefill / extend.  Everything the plan refuses is refused before the first launch.
int llm_prefill(gvl_ctx* ctx, Seq* const* sqs, int nb, const bf16_t* const* embeds, const int* lens, hipStream_t st, const LossReq* loss, const int* pos0s, const ScoreReq* score,
                bool keep_hidden) {
  const gvl_config& f = ctx->cfg;
  const int Hd = f.hidden, H = f.heads, KV = f.kv_heads, Dr = ctx->l_Dr, D = ctx->l_D, I = f.inter;
  const int qkvw = (H + 2 * KV) * Dr;
  PrefillGeometry geo{};
  geo.nb = nb;
  for (int b = 0; b < nb && b < GVL_MAX_PREFILL_BATCH; ++b) { geo.lens[b] = lens[b]; geo.pos0[b] = pos0s ? pos0s[b] : 0; }
  geo.rope_orig_max_pos = f.rope_orig_max_pos; geo.long_table = ctx->cos_l != nullptr; geo.loss = loss != nullptr; geo.page_id_cap = (int)(sizeof(IntList::v) / sizeof(int));
  geo.hidden = Hd; geo.qkv_width = qkvw; geo.gate_up_width = 2 * I; geo.fused_weights = !ctx->ll.empty() && ctx->ll[0].qkvw_f; geo.score = score != nullptr;
  geo.keep_hidden = keep_hidden;
  if (keep_hidden && (sqs[0]->bank_rows != 0 || lens[0] > sqs[0]->bank_cap)) return fail(ctx, GVL_ERR_STATE, "llm_prefill: the hidden bank is not empty or too small");
  PrefillPlan plan;
  { const int rc = prefill_plan(geo, PrefillKnobs{ctx->dbg.varlen_attn, ctx->dbg.varlen_extend != 0, ctx->dbg.last_layer_tail != 0, ctx->dbg.norm_fused != 0}, &plan);
    if (rc) return fail(ctx, GVL_ERR_ARG, prefill_refusal_reason(rc)); }
  for (int b = 0; b < nb; ++b) { const int rc = upload_table(ctx, *sqs[b], st); if (rc) return rc; }
  const int* off = plan.off; const int* p0 = geo.pos0;
  const int M = plan.M, S0 = lens[0], P0 = (S0 + 63) / 64;
  ArenaScope arena_scope(ctx->arena_l_off);
  LALLOC(x, bf16_t, (size_t)M * Hd); LALLOC(h, bf16_t, (size_t)M * Hd); LALLOC(qkv, bf16_t, (size_t)M * qkvw);
  LALLOC(att, bf16_t, (size_t)M * H * Dr); LALLOC(act, bf16_t, (size_t)M * I); LALLOC(Q, bf16_t, (size_t)M * H * D);
  const int* group_table = nullptr;
  if (plan.batched_table) {   // [nb][P0] page ids of the batch, written by a stream-ordered kernel (ids passed by value: no host buffer lifetime)
    LALLOC(tb, int, (size_t)nb * P0);
    IntList l; l.n = nb * P0;
    for (int b = 0; b < nb; ++b) for (int p = 0; p < P0; ++p) l.v[b * P0 + p] = sqs[b]->pages[p];
    hipLaunchKernelGGL(fill_ints_kernel, dim3(1), dim3(256), 0, st, tb, l);
    group_table = tb;
  }
  for (int b = 0; b < nb; ++b) RUN(GVL_PROF_OTHER, 0, gvl_launch_copy_bytes(embeds[b], x + (size_t)off[b] * Hd, (size_t)lens[b] * Hd * 2, st));
  // fused RMSNorm (see gvl_vision_plan.h): o_proj / down_proj leave the row statistics of the new residual stream, qkv_proj / gate_up_proj consume the raw
  // stream with the norm weight folded in and scale their accumulator rows; layer 0's input norm keeps the pass
  const int NBLK = Hd / 64;
  const bool nf = plan.nf;
  LALLOC(sq, float, (size_t)M * (nf ? NBLK : 1)); LALLOC(nrs, float, (size_t)M);
  const bf16_t* tail_rows = nullptr;                  // [nb][Hd]: the sequences' last rows after the last layer, when only they went through its MLP
  // The arguments of a planned launch.  Whose pages: the member's own block table (ONE), the group's [nb][P0] table (BATCHED), or a table, a row range and a prefix per
  // member (RAGGED*: the whole group, rows packed back to back).
  auto members = [&](auto& a, const PrefillStep& s) {
    if (s.form == GVL_PREFILL_ONE) { a.block_table = sqs[s.first]->d_block_table; a.max_pages = sqs[s.first]->n_pages; }
    else if (s.form == GVL_PREFILL_BATCHED) { a.block_table = group_table; a.max_pages = P0; }
    else {
      a.vl_n = s.count;
      for (int u = 0; u < s.count; ++u) { a.vl_rows[u] = off[u]; a.vl_tables[u] = sqs[u]->d_block_table; a.vl_pos0[u] = p0[u]; }
      a.vl_rows[s.count] = off[s.count];
    }
  };
  auto post_args = [&](const PrefillStep& s, bf16_t* Kt, bf16_t* Vt) {
    QkvPostArgs q; memset(&q, 0, sizeof(q)); q.qkv = qkv + (size_t)off[s.first] * qkvw; q.ld = qkvw; q.Q = Q + (size_t)off[s.first] * H * D; q.Kt = Kt; q.Vt = Vt;
    q.B = s.B; q.S = s.S; q.H = H; q.KV = KV; q.Dr = Dr; q.D = D; q.mode = 2; q.cos = s.use_long ? ctx->cos_l : ctx->cos_s; q.sin = s.use_long ? ctx->sin_l : ctx->sin_s; q.pos0 = s.pos0;
    members(q, s);
    return q;
  };
  auto attn_args = [&](const PrefillStep& s, const bf16_t* Kt, const bf16_t* Vt) {
    AttnArgs a; memset(&a, 0, sizeof(a)); a.Q = Q + (size_t)off[s.first] * H * D; a.Kt = Kt; a.Vt = Vt; a.O = att + (size_t)off[s.first] * H * Dr;
    a.B = s.B; a.H = H; a.KV = KV; a.S = s.S; a.D = D; a.Dout = Dr; a.scale = 1.0f / sqrtf((float)Dr); a.causal = 1; a.Sk = s.Sk; a.qpos0 = s.pos0;
    if (s.form == GVL_PREFILL_ONE || s.form == GVL_PREFILL_BATCHED) a.ring = ctx->dbg.attn_ring;   // the ring depth is a knob of the single-sequence kernels only
    members(a, s);
    return a;
  };
  // the work an attention launch is booked with: its members' own sums, whatever grid serves them
  double attn_flops[GVL_PREFILL_MAX_STEPS] = {};
  for (int i = 0; i < plan.n_steps; ++i) {
    const PrefillStep& s = plan.steps[i];
    if (s.kind != GVL_PREFILL_ATTN) continue;
    if (s.form == GVL_PREFILL_ONE || s.form == GVL_PREFILL_BATCHED) attn_flops[i] = gvl_attn_flops(attn_args(s, nullptr, nullptr));
    else for (int u = s.first; u < s.first + s.count; ++u) attn_flops[i] += gvl_attn_flops(attn_args(prefill_member_step(geo, GVL_PREFILL_ATTN, u), nullptr, nullptr));
  }
  for (int l = 0; l < f.layers; ++l) {
    const LlmLayerW& w = ctx->ll[l];
    bf16_t* Kt = ctx->kpool + (size_t)l * ctx->layer_stride; bf16_t* Vt = ctx->vpool + (size_t)l * ctx->layer_stride;
    if (nf && l > 0) {
      RUN(GVL_PROF_OTHER, 0, gvl_launch_rowsq_finish(sq, NBLK, 0, NBLK, nrs, M, Hd, f.rms_eps, st));
      GemmArgs g = gemm(x, Hd, w.qkvw_f, qkv, qkvw, M, qkvw, Hd); g.rowscale = nrs; RUN(GVL_PROF_GEMM, gvl_gemm_flops(g), gvl_launch_gemm(g, st));
    } else {
      RUN(GVL_PROF_OTHER, 0, gvl_launch_rmsnorm_bf16(x, w.ln1, h, M, Hd, f.rms_eps, st));
      GemmArgs g = gemm(h, Hd, w.qkvw, qkv, qkvw, M, qkvw, Hd); RUN(GVL_PROF_GEMM, gvl_gemm_flops(g), gvl_launch_gemm(g, st));
    }
    // RoPE + KV append + V^T pages (post) and causal attention, as planned: the same steps in every layer
    for (int i = 0; i < plan.n_steps; ++i) {
      const PrefillStep& s = plan.steps[i];
      if (s.kind == GVL_PREFILL_POST) {
        const QkvPostArgs q = post_args(s, Kt, Vt);
        switch (s.form) {
          case GVL_PREFILL_RAGGED_EXT: RUN(GVL_PROF_OTHER, 0, gvl_launch_qkv_post_ext(q, st)); break;
          default: RUN(GVL_PROF_OTHER, 0, gvl_launch_qkv_post(q, st));
        }
      } else {
        const AttnArgs a = attn_args(s, Kt, Vt);
        switch (s.form) {
          case GVL_PREFILL_RAGGED_EXT: RUN(GVL_PROF_ATTN, attn_flops[i], gvl_launch_attention_ext(a, st)); break;
          default: RUN(GVL_PROF_ATTN, attn_flops[i], gvl_launch_attention(a, st));
        }
      }
    }
    { GemmArgs g = gemm(att, H * Dr, w.ow, x, Hd, M, Hd, H * Dr); g.resid = x; g.ldr = Hd; if (nf) { g.rowsq = sq; g.rowsq_ld = NBLK; }
      RUN(GVL_PROF_GEMM, gvl_gemm_flops(g), gvl_launch_gemm(g, st)); }
    // LAST layer's tail (PrefillPlan.tail says when): gate_up / down on the nb last rows alone.  The rows are gathered (x and, fused norm, their row statistics); GEMM
    // rows do not depend on their neighbours, so the logits are bit-identical to the full pass (asserted; gvl_debug_set("last_layer_tail", 0) = the full pass).
    if (l == f.layers - 1 && plan.tail) {
      int ids[GVL_MAX_PREFILL_BATCH];
      for (int b = 0; b < nb; ++b) ids[b] = off[b + 1] - 1;
      LALLOC(xl, bf16_t, (size_t)nb * Hd); LALLOC(actl, bf16_t, (size_t)nb * I);
      RUN(GVL_PROF_OTHER, 0, gvl_launch_gather_rows_host_ids(x, ids, nb, xl, Hd, st));
      if (nf) {
        LALLOC(sql, float, (size_t)nb * NBLK); LALLOC(rsl, float, nb);
        RUN(GVL_PROF_OTHER, 0, gvl_launch_gather_rows_host_ids((const bf16_t*)sq, ids, nb, (bf16_t*)sql, NBLK * 2, st));      // a row of partial sums = NBLK floats
        RUN(GVL_PROF_OTHER, 0, gvl_launch_rowsq_finish(sql, NBLK, 0, NBLK, rsl, nb, Hd, f.rms_eps, st));
        GemmArgs g = gemm(xl, Hd, w.guw_f, actl, I, nb, 2 * I, Hd); g.act = GVL_ACT_SILU_MUL; g.rowscale = rsl; RUN(GVL_PROF_GEMM, gvl_gemm_flops(g), gvl_launch_gemm(g, st));
      } else {
        LALLOC(hl, bf16_t, (size_t)nb * Hd);
        RUN(GVL_PROF_OTHER, 0, gvl_launch_rmsnorm_bf16(xl, w.ln2, hl, nb, Hd, f.rms_eps, st));
        GemmArgs g = gemm(hl, Hd, w.guw, actl, I, nb, 2 * I, Hd); g.act = GVL_ACT_SILU_MUL; RUN(GVL_PROF_GEMM, gvl_gemm_flops(g), gvl_launch_gemm(g, st));
      }
      { GemmArgs g = gemm(actl, I, w.downw, xl, Hd, nb, Hd, I); g.resid = xl; g.ldr = Hd; RUN(GVL_PROF_GEMM, gvl_gemm_flops(g), gvl_launch_gemm(g, st)); }
      tail_rows = xl;
      continue;
    }
    if (nf) {
      RUN(GVL_PROF_OTHER, 0, gvl_launch_rowsq_finish(sq, NBLK, 0, NBLK, nrs, M, Hd, f.rms_eps, st));
      GemmArgs g = gemm(x, Hd, w.guw_f, act, I, M, 2 * I, Hd); g.act = GVL_ACT_SILU_MUL; g.rowscale = nrs; RUN(GVL_PROF_GEMM, gvl_gemm_flops(g), gvl_launch_gemm(g, st));
    } else {
      RUN(GVL_PROF_OTHER, 0, gvl_launch_rmsnorm_bf16(x, w.ln2, h, M, Hd, f.rms_eps, st));
      GemmArgs g = gemm(h, Hd, w.guw, act, I, M, 2 * I, Hd); g.act = GVL_ACT_SILU_MUL; RUN(GVL_PROF_GEMM, gvl_gemm_flops(g), gvl_launch_gemm(g, st));
    }
    { GemmArgs g = gemm(act, I, w.downw, x, Hd, M, Hd, I); g.resid = x; g.ldr = Hd; if (nf && l + 1 < f.layers) { g.rowsq = sq; g.rowsq_ld = NBLK; }
      RUN(GVL_PROF_GEMM, gvl_gemm_flops(g), gvl_launch_gemm(g, st)); }
  }
  if (loss && loss->n > 0) {
    // training forward (llava_next_video.py:598-614 -> Phi3ForCausalLM.forward labels branch, modeling_phi3.py:1512-1539): only rows
    // whose NEXT token carries a label need logits.  gather -> final RMSNorm -> lm_head GEMM (+bias, bf16 logits as under
    // autocast) -> f32 cross entropy per row; the host adds the rows up in order (deterministic).
    LALLOC(d_rows, int, loss->n); LALLOC(d_tgt, int, loss->n); LALLOC(d_nll, float, loss->n);
    LALLOC(hs, bf16_t, (size_t)kLossChunk * Hd); LALLOC(lg, bf16_t, (size_t)kLossChunk * f.vocab);
    HIPCHK(ctx, hipMemcpyAsync(d_rows, loss->h_rows, (size_t)loss->n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_tgt, loss->h_targets, (size_t)loss->n * 4, hipMemcpyHostToDevice, st));
    for (int r0 = 0; r0 < loss->n; r0 += kLossChunk) {
      const int n = loss->n - r0 < kLossChunk ? loss->n - r0 : kLossChunk;
      RUN(GVL_PROF_OTHER, 0, gvl_launch_gather_rows(x, d_rows + r0, hs, n, Hd, st));
      RUN(GVL_PROF_OTHER, 0, gvl_launch_rmsnorm_bf16(hs, ctx->l_norm, h, n, Hd, f.rms_eps, st));      // h is free by now; n <= S - 1 rows
      { GemmArgs g = gemm(h, Hd, ctx->l_headw, lg, f.vocab, n, f.vocab, Hd); g.bias = ctx->l_headb; RUN(GVL_PROF_GEMM, gvl_gemm_flops(g), gvl_launch_gemm(g, st)); }
      RUN(GVL_PROF_OTHER, 0, gvl_launch_ce_rows(lg, f.vocab, d_tgt + r0, d_nll + r0, n, f.vocab, st));
    }
    HIPCHK(ctx, hipMemcpyAsync(loss->h_nll, d_nll, (size_t)loss->n * 4, hipMemcpyDeviceToHost, st));
  }
  if (score && score->n > 0) {
    // score tail (gvl_score_extend_varlen): the loss tail's walk over the scored rows of the whole group -- gather -> final RMSNorm -> lm_head GEMM -- with fp32 logits (+bias),
    // the format the generate path selects from, and score_rows_kernel on every chunk.  ONE weight stream per kScoreChunk rows (the last-row GEMV below would take one per 4).
    // A GEMM row does not depend on its neighbours, so a row's results do not depend on the chunk or the group it travels in.  The indices and targets go by value in the
    // arguments of a stream-ordered fill (no host buffer lifetime); lg is the loss tail's reservation (kLossChunk bf16 rows = kScoreChunk fp32 rows) plus the row pitch's
    // rounding up to 4 floats (prefill_bytes: kScoreChunk * 12 bytes).
    // gvl_launch_gemm takes N % 4 == 0 and stages whole rows for N % 16 == 0; the fine-tuned vocabularies are 32 366 and 128 558: the GEMM computes the columns up to
    // the last multiple of 16, head_cols_kernel the up to 15 behind it.
    static_assert(kScoreChunk * 4 == kLossChunk * 2, "score tail: the fp32 logits chunk is the loss tail's reservation");
    const int ldv = (f.vocab + 3) & ~3, n16 = f.vocab & ~15;
    LALLOC(d_rows, int, score->n); LALLOC(d_tgt, int, score->n);
    LALLOC(hs, bf16_t, (size_t)kScoreChunk * Hd); LALLOC(lg, float, (size_t)kScoreChunk * ldv);
    for (int r0 = 0; r0 < score->n; r0 += 256) {
      IntList lr, lt; lr.n = lt.n = score->n - r0 < 256 ? score->n - r0 : 256;
      for (int i = 0; i < lr.n; ++i) { lr.v[i] = score->h_rows[r0 + i]; lt.v[i] = score->h_targets[r0 + i]; }
      hipLaunchKernelGGL(fill_ints_kernel, dim3(1), dim3(256), 0, st, d_rows + r0, lr);
      hipLaunchKernelGGL(fill_ints_kernel, dim3(1), dim3(256), 0, st, d_tgt + r0, lt);
    }
    if (hipGetLastError() != hipSuccess) return fail(ctx, GVL_ERR_HIP, "score tail: row list upload failed");
    for (int r0 = 0; r0 < score->n; r0 += kScoreChunk) {
      const int n = score->n - r0 < kScoreChunk ? score->n - r0 : kScoreChunk;
      RUN(GVL_PROF_OTHER, 0, gvl_launch_gather_rows(x, d_rows + r0, hs, n, Hd, st));
      RUN(GVL_PROF_OTHER, 0, gvl_launch_rmsnorm_bf16(hs, ctx->l_norm, h, n, Hd, f.rms_eps, st));      // h is free by now; n <= M rows
      if (n16 > 0) { GemmArgs g = gemm(h, Hd, ctx->l_headw, lg, ldv, n, n16, Hd); g.bias = ctx->l_headb; g.out_f32 = 1; RUN(GVL_PROF_GEMM, gvl_gemm_flops(g), gvl_launch_gemm(g, st)); }
      if (n16 < f.vocab) RUN(GVL_PROF_OTHER, 0, gvl_launch_head_cols(h, Hd, ctx->l_headw, Hd, ctx->l_headb, lg, ldv, n16, f.vocab - n16, n, st));
      ScoreRowsArgs sr; memset(&sr, 0, sizeof(sr)); sr.logits = lg; sr.n = f.vocab; sr.ld = ldv; sr.rows = n; sr.top_n = score->top_n; sr.targets = d_tgt + r0;
      sr.lp = score->d_lp + r0; sr.rank = score->d_rank + r0;
      if (score->top_n > 0) { sr.top_ids = score->d_top_ids + (size_t)r0 * GVL_MAX_TOP_LOGPROBS; sr.top_lp = score->d_top_lp + (size_t)r0 * GVL_MAX_TOP_LOGPROBS; }
      RUN(GVL_PROF_OTHER, 0, gvl_launch_score_rows(sr, st));
    }
  }
  // hidden bank (gvl_seq_keep_hidden): the plan ran the last layer on every row, so x IS the final residual stream -- one launch normalises the M rows into the bank
  if (keep_hidden) { const int rc = bank_append(ctx, *sqs[0], x, Hd, M, st); if (rc) return rc; }
  // last-row-only lm_head: final RMSNorm fused into the GEMV; one weight stream for the nb last rows
  const bf16_t* last = x + (size_t)(S0 - 1) * Hd;
  int last_stride = S0 * Hd;
  if (plan.last_rows == GVL_PREFILL_LAST_TAIL) { last = tail_rows; last_stride = Hd; }
  else if (plan.last_rows == GVL_PREFILL_LAST_GATHERED) {   // ragged: gather the nb last rows (h is free by now)
    for (int b = 0; b < nb; ++b) RUN(GVL_PROF_OTHER, 0, gvl_launch_copy_bytes(x + (size_t)(off[b + 1] - 1) * Hd, h + (size_t)b * Hd, (size_t)Hd * 2, st));
    last = h; last_stride = Hd;
  }
  for (int c = 0, b0 = 0; c < plan.n_chunks; ++c) {   // the GEMV holds 1, 2 or 4 vectors in LDS: chunks of 4 / 2 / 1 last rows
    const int nbc = plan.chunks[c];
    GemvArgs g; memset(&g, 0, sizeof(g)); g.W = ctx->l_headw; g.N = f.vocab; g.K = Hd; g.x = last + (size_t)b0 * last_stride; g.norm_w = ctx->l_norm; g.eps = f.rms_eps;
    g.batch = nbc; g.x_stride = last_stride; g.out_stride = f.vocab;
    g.bias = ctx->l_headb; g.out_f32 = ctx->d_logits + (size_t)b0 * f.vocab; RUN(GVL_PROF_GEMV, 2.0 * f.vocab * Hd, gvl_launch_gemv(g, st));
    b0 += nbc;
  }
  for (int b = 0; b < nb; ++b) RUN(GVL_PROF_OTHER, 0, gvl_launch_set_int(sqs[b]->d_ngen, 0, st));
  { ArgmaxArgs am; memset(&am, 0, sizeof(am)); am.logits = ctx->d_logits; am.n = f.vocab; am.batch = nb;
    for (int b = 0; b < nb; ++b) { am.tok_ptrs[b] = sqs[b]->d_tok; am.out_lists[b] = sqs[b]->d_out; am.ngen_ptrs[b] = sqs[b]->d_ngen; }   // first generated token
    for (int b = 0; b < nb; ++b) sqs[b]->rng_stream = ctx->sample.next_stream++;     // a fresh random stream per prefilled sequence
    RUN(GVL_PROF_OTHER, 0, pick_tokens(ctx, am, sqs, st)); }
  for (int b = 0; b < nb; ++b) {
    RUN(GVL_PROF_OTHER, 0, gvl_launch_set_int(sqs[b]->d_pos, p0[b] + lens[b], st));
    sqs[b]->pos = p0[b] + lens[b]; sqs[b]->n_gen = 1;
  }
  return 0;
}

// The GemvArgs of one decode projection: the kind's own operands and constants, and what the plan's entry decides about it (gvl_decode_plan.h: which weight copy, with
// or without scales, which input, what it leaves behind).  `l` is the layer (any for lm_head); qkv carries the fused epilogue RoPE + Q write + paged-KV append.
static GemvArgs proj_args(const gvl_ctx* ctx, int kind, int l, const DecodeProjPlan& e, Seq* const* sqs, int B) {
  const gvl_config& f = ctx->cfg;
  const int Hd = f.hidden, H = f.heads, KV = f.kv_heads, Dr = ctx->l_Dr, D = ctx->l_D, I = f.inter;
  const LlmLayerW& w = ctx->ll[l];
  GemvArgs g; memset(&g, 0, sizeof(g)); g.batch = B;
  struct { const bf16_t *row_major, *tiled, *folded; } W{};   // by DecodeWeight
  const float* scales = nullptr; const bf16_t* norm_w = nullptr;
  switch (kind) {
    case GVL_DPROJ_QKV0: case GVL_DPROJ_QKV:
      W = {w.qkvw, w.qkvd, w.qkvd_f}; scales = w.qkvs; norm_w = w.ln1; g.N = (H + 2 * KV) * Dr; g.K = Hd;
      g.rope_on = 1; g.cos_s = ctx->cos_s; g.sin_s = ctx->sin_s; g.cos_l = ctx->cos_l; g.sin_l = ctx->sin_l;
      g.rope_switch = ctx->cos_l ? f.rope_orig_max_pos : 0;
      for (int b = 0; b < B; ++b) { g.pos_ptrs[b] = sqs[b]->d_pos; g.tables[b] = sqs[b]->d_block_table; }
      g.Q = ctx->d_q; g.q_stride = H * D; g.Kt = ctx->kpool + (size_t)l * ctx->layer_stride; g.Vt = ctx->vpool + (size_t)l * ctx->layer_stride;
      g.H = H; g.KV = KV; g.Dr = Dr; g.D = D;
      break;
    case GVL_DPROJ_O:
      W = {w.ow, w.od, nullptr}; scales = w.os; g.N = Hd; g.K = H * Dr; g.resid = ctx->d_x; g.out_bf16 = ctx->d_x; g.out_stride = Hd;
      break;
    case GVL_DPROJ_GATE_UP:
      W = {w.guw, w.gud, w.gud_f}; scales = w.gus; norm_w = w.ln2; g.N = 2 * I; g.K = Hd; g.act = GVL_ACT_SILU_MUL; g.out_bf16 = ctx->d_act; g.out_stride = I;
      break;
    case GVL_DPROJ_DOWN:
      W = {w.downw, w.downd, nullptr}; scales = w.downs; g.N = Hd; g.K = I; g.resid = ctx->d_x; g.out_bf16 = ctx->d_x; g.out_stride = Hd;
      break;
    default:   // GVL_DPROJ_HEAD
      W = {ctx->l_headw, ctx->l_headd, ctx->l_headd_f}; scales = ctx->l_heads; norm_w = ctx->l_norm; g.N = f.vocab; g.K = Hd; g.bias = ctx->l_headb;
      g.out_f32 = ctx->d_logits; g.out_stride = f.vocab;
  }
  g.x_stride = g.K;
  g.W = e.weight == GVL_DW_ROW_MAJOR ? W.row_major : e.weight == GVL_DW_TILED ? W.tiled : W.folded;
  if (e.scales) { g.w_fp8 = ctx->fp8; g.wscale = scales; }
  switch (e.input) {
    case GVL_DIN_X_NORM: g.x = ctx->d_x; g.norm_w = norm_w; g.eps = f.rms_eps; break;
    case GVL_DIN_XN: g.x = ctx->d_xn; break;
    case GVL_DIN_XT_SQ: g.x = ctx->d_xt; g.sq_in = ctx->d_sqpart; g.sq_n = Hd >> 4; g.eps = f.rms_eps; break;
    case GVL_DIN_ATTN: g.x = ctx->d_attn; break;
    default: g.x = ctx->d_act;   // GVL_DIN_ACT
  }
  if (e.sq_out) { g.sq_out = ctx->d_sqpart; g.out_tiled2 = ctx->d_xt; }
  g.out_tiled = e.out_tiled ? 1 : 0;
  return g;
}

// One greedy decode step for B sequences together (1..16 on the skinny-GEMM path, 1 / 2 / 4 on the VALU fallback): each weight
// matrix is streamed ONCE for the whole batch, attention / RoPE / KV append run per sequence on its own pages.  Every launch
// argument is a device pointer or a constant of the group: the step can be replayed (hipGraph) without host-side counters.
// WHICH launches it takes and what each projection reads is decode_plan's decision (gvl_decode_plan.h: pure, tested on the CPU): 4 * layers + 1 projections, `layers`
// attention launches, 1 launch in front (+ 2 * layers norm launches for an unfused group of more than 4), then token selection.  This function is plan, then walk.
// Guided pairs: the rows are step_rows' -- plain sequences and leaders first, then the followers (a row's results do not depend on its place).  The forward pass treats
// a follower like any row; the selection covers the rows in front only, with the pairs' two launches around it (pick_tokens).
int decode_step(gvl_ctx* ctx, Seq* const* sqs, int B, hipStream_t st) {
  const gvl_config& f = ctx->cfg;
  const int Hd = f.hidden, H = f.heads, KV = f.kv_heads, Dr = ctx->l_Dr, D = ctx->l_D, I = f.inter;
  const int qkvw = (H + 2 * KV) * Dr;
  DecodePlan plan;
  { const int rc = decode_plan(DecodeGeometry{B, f.layers, Hd, ctx->decode_mfma, ctx->fp8, ctx->l_headd_f != nullptr}, DecodeKnobs{ctx->dbg.norm_fused != 0}, &plan);
    if (rc) return fail(ctx, GVL_ERR_ARG, decode_refusal_reason(rc)); }
  for (int b = 0; b < B; ++b) { const int rc = upload_table(ctx, *sqs[b], st); if (rc) return rc; }   // (a no-op after the sequence's prefill; under capture it would be part of the graph -- never dirty there)
  TokPtrs tp; memset(&tp, 0, sizeof(tp)); tp.n = B; for (int b = 0; b < B; ++b) tp.p[b] = sqs[b]->d_tok;
  if (plan.embed_norm) RUN(GVL_PROF_OTHER, 0, gvl_launch_embed_norm(ctx->l_embed, tp, ctx->d_x, ctx->d_xn, ctx->ll[0].ln1, Hd, f.rms_eps, st));
  else RUN(GVL_PROF_OTHER, 0, gvl_launch_gather_tok_rows(ctx->l_embed, tp, ctx->d_x, Hd, st));
  double ctx_tokens = 0; for (int b = 0; b < B; ++b) ctx_tokens += sqs[b]->pos + 1;
  // Decode-attention launch shape (decode_attn_shape, gvl_attn_plan.h): block slots along the context, splits and heads per block -- from the sequences' positions and
  // the gvl_debug_set overrides; under stream capture the shape that stays valid for later steps
  int gsplit, cpb, hpb;
  { hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = st != nullptr && hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
    int positions[GVL_MAX_DECODE_BATCH];
    for (int b = 0; b < B; ++b) positions[b] = sqs[b]->pos;
    const DecodeAttnShape s = decode_attn_shape(positions, B, H, KV, ctx->nsplit, ctx->dbg.decode_attn_cpb, ctx->dbg.decode_attn_hpb, capturing);
    gsplit = s.gsplit; cpb = s.cpb; hpb = s.hpb; }
  auto project = [&](int kind, int l, double flops) -> int {
    const DecodeProjPlan& e = plan.proj[kind];
    const GemvArgs g = proj_args(ctx, kind, l, e, sqs, B);
    RUN(GVL_PROF_GEMV, flops, e.launcher == GVL_DLAUNCH_DGEMM ? gvl_launch_dgemm(g, st) : gvl_launch_gemv(g, st));
    return 0;
  };
  for (int l = 0; l < f.layers; ++l) {
    if (const int rc = project(l ? GVL_DPROJ_QKV : GVL_DPROJ_QKV0, l, 2.0 * qkvw * Hd)) return rc;
    { DecodeAttnArgs a; memset(&a, 0, sizeof(a)); a.q = ctx->d_q; a.q_stride = H * D;
      a.Kt = ctx->kpool + (size_t)l * ctx->layer_stride; a.Vt = ctx->vpool + (size_t)l * ctx->layer_stride;
      for (int b = 0; b < B; ++b) { a.tables[b] = sqs[b]->d_block_table; a.pos_ptrs[b] = sqs[b]->d_pos; }
      a.part = ctx->d_part; a.counters = ctx->d_counters; a.batch = B; a.gsplit = gsplit; a.cpb = cpb; a.hpb = hpb;
      a.out = ctx->d_attn; a.out_stride = H * Dr; a.out_tiled = plan.attn_out_tiled ? 1 : 0; a.H = H; a.KV = KV; a.D = D; a.Dout = Dr; a.nsplit = ctx->nsplit; a.scale = 1.0f / sqrtf((float)Dr);
      RUN(GVL_PROF_DECODE_ATTN, 4.0 * ctx_tokens * (double)KV * D, gvl_launch_decode_attention(a, st)); }
    if (const int rc = project(GVL_DPROJ_O, l, 2.0 * Hd * H * Dr)) return rc;
    if (plan.norm_launches) RUN(GVL_PROF_OTHER, 0, gvl_launch_norm_tiled(ctx->d_x, ctx->d_xn, ctx->ll[l].ln2, B, Hd, f.rms_eps, st));     // post_attention_layernorm
    if (const int rc = project(GVL_DPROJ_GATE_UP, l, 4.0 * I * Hd)) return rc;
    if (const int rc = project(GVL_DPROJ_DOWN, l, 2.0 * Hd * I)) return rc;
    if (plan.norm_launches)   // the next layer's input_layernorm, or the final norm in front of lm_head
      RUN(GVL_PROF_OTHER, 0, gvl_launch_norm_tiled(ctx->d_x, ctx->d_xn, l + 1 < f.layers ? ctx->ll[l + 1].ln1 : ctx->l_norm, B, Hd, f.rms_eps, st));
  }
  if (const int rc = project(GVL_DPROJ_HEAD, 0, 2.0 * f.vocab * Hd)) return rc;
  int nsel = B;                                        // rows a token is selected for: everything in front of the followers
  while (nsel > 0 && sqs[nsel - 1]->lead >= 0) --nsel;
  PairLaunches pl;
  if (nsel < B) {                                      // any pair in this group
    memset(&pl, 0, sizeof(pl)); pl.g.n = f.vocab;
    for (int b = 0; b < nsel; ++b) {
      if (sqs[b]->follow < 0) continue;
      int r = nsel; while (r < B && sqs[r] != &ctx->seqs[sqs[b]->follow]) ++r;
      if (r == B || pl.g.n_pairs >= GVL_MAX_GUIDANCE_PAIRS) return fail(ctx, GVL_ERR_STATE, "decode_step: a guided leader without its follower's row");
      const int p = pl.g.n_pairs++;
      pl.g.cond[p] = ctx->d_logits + (size_t)b * f.vocab; pl.g.neg[p] = ctx->d_logits + (size_t)r * f.vocab; pl.g.scale[p] = sqs[b]->guide;
      pl.f.lead_tok[p] = sqs[b]->d_tok; pl.f.tok[p] = sqs[r]->d_tok; pl.f.out[p] = sqs[r]->d_out; pl.f.ngen[p] = sqs[r]->d_ngen; pl.f.pos[p] = sqs[r]->d_pos;
    }
    pl.f.n = pl.g.n_pairs;
    if (pl.g.n_pairs != B - nsel) return fail(ctx, GVL_ERR_STATE, "decode_step: a follower's row without its leader");
  }
  { ArgmaxArgs am; memset(&am, 0, sizeof(am)); am.logits = ctx->d_logits; am.n = f.vocab; am.batch = nsel;   // token, output list, n_gen++ and pos++ on the device
    for (int b = 0; b < nsel; ++b) { am.tok_ptrs[b] = sqs[b]->d_tok; am.out_lists[b] = sqs[b]->d_out; am.ngen_ptrs[b] = sqs[b]->d_ngen; am.pos_ptrs[b] = sqs[b]->d_pos; }
    if (ctx->watch_eos >= 0) { am.eos_id = ctx->watch_eos; for (int b = 0; b < nsel; ++b) am.eos_flags[b] = sqs[b]->d_eos; }
    RUN(GVL_PROF_OTHER, 0, pick_tokens(ctx, am, sqs, st, nsel < B ? &pl : nullptr)); }
  for (int b = 0; b < B; ++b) { sqs[b]->pos += 1; sqs[b]->n_gen += 1; }
  return 0;
}

// A decode step's launches carry device pointers and group constants only, so ONE captured step can be replayed for the following
// tokens of the same group (hipGraph): the host pays one graph launch instead of the step's kernel launches per token
// (decode_plan: 4 * layers + 1 projections, `layers` attention launches, 1 or 1 + 2 * layers in front, then token selection: 162 + selection at 32 layers).
struct StepGraph {
  hipGraph_t g = nullptr; hipGraphExec_t e = nullptr; bool failed = false;
  ~StepGraph() { if (e) hipGraphExecDestroy(e); if (g) hipGraphDestroy(g); }
};
int decode_step_replay(gvl_ctx* ctx, Seq* const* sqs, int B, hipStream_t st, StepGraph& sg) {
  if (!ctx->dbg.decode_graph || ctx->prof || st == nullptr || sg.failed) return decode_step(ctx, sqs, B, st);
  if (!sg.e) {
    if (hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed) != hipSuccess) { (void)hipGetLastError(); sg.failed = true; return decode_step(ctx, sqs, B, st); }
    bool was_dirty[GVL_MAX_DECODE_BATCH];                      // upload_table clears table_dirty when it ENQUEUES the upload -- inside a capture that is a recording only
    for (int b = 0; b < B; ++b) was_dirty[b] = sqs[b]->table_dirty;
    const int rc = decode_step(ctx, sqs, B, st);               // recorded, not executed; the host counters advance once
    const hipError_t ce = hipStreamEndCapture(st, &sg.g);
    if (rc) return rc;
    if (ce != hipSuccess || hipGraphInstantiate(&sg.e, sg.g, nullptr, nullptr, 0) != hipSuccess) {
      (void)hipGetLastError(); sg.failed = true; sg.e = nullptr;
      // the capture never ran: the block tables it would have written are still unwritten -- the eager step below must upload them
      for (int b = 0; b < B; ++b) { sqs[b]->pos -= 1; sqs[b]->n_gen -= 1; if (was_dirty[b]) sqs[b]->table_dirty = true; }
      return decode_step(ctx, sqs, B, st);
    }
    HIPCHK(ctx, hipGraphLaunch(sg.e, st));
    return 0;
  }
  HIPCHK(ctx, hipGraphLaunch(sg.e, st));
  for (int b = 0; b < B; ++b) { sqs[b]->pos += 1; sqs[b]->n_gen += 1; }
  return 0;
}

// decode of one group (prefilled sequences at the same generation step) until every member hit eos / max_new / its capacity.
// eos: the token-selection kernel stores a sequence's generation count into its host-mapped flag word the moment it picks eos; the host
// keeps at most two steps ahead of the GPU (an event per step) and reads the flags after each event -- at most two steps are decoded in
// vain and the stream is never drained mid-answer (round 1 drained it every 16 steps and could run 15 steps past eos).
int decode_group(gvl_ctx* ctx, Seq* const* sqs, int B, int max_new, int eos_id, int32_t* const* out_ids, int* const* n_out, hipStream_t st) {
  const int start_gen = sqs[0]->n_gen;   // members of a group must be in the same generation step
  for (int b = 1; b < B; ++b) if (sqs[b]->n_gen != start_gen) return fail(ctx, GVL_ERR_STATE, "decode batch: sequences are at different generation steps");
  struct Watch { gvl_ctx* c; ~Watch() { c->watch_eos = -1; } } watch{ctx};
  bool done[GVL_MAX_DECODE_BATCH] = {false};
  if (eos_id >= 0) {
    // the tokens produced so far (the prefill's first token) were selected without a watch: look at them once, then arm the flags
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b) {
      memcpy(out_ids[b], sqs[b]->h_out, (size_t)start_gen * 4);          // host-mapped list; the stream was synchronised above
      for (int i = 0; i < start_gen && !done[b]; ++i) if (out_ids[b][i] == eos_id) done[b] = true;
      *sqs[b]->h_eos = 0;
    }
    ctx->watch_eos = eos_id;
  }
  // Only LIVE members are stepped: a sequence that produced eos (seen two steps late) or reached its own capacity / max_new leaves the
  // group, so it can neither truncate the answers of longer-running members nor append past its pages.  A sequence's ids do not depend
  // on the group it is decoded in (gvl_decode.hip), so shrinking the group changes no result; the captured step is re-recorded.
  // The live set is stepped as PARTS of sizes the decode path takes (decode_parts, gvl_decode_plan.h: any size up to 16 on the skinny-MFMA path;
  // 4 / 2 / 1 on the VALU fallback, so three survivors of a group of four run as 2 + 1), one captured step graph per part.
  // A guided pair (gvl_seq_set_guidance) is one member here: the leader is named, its follower is the part's extra row and leaves with it -- the follower's own eos,
  // capacity and count are never looked at (its capacity was checked when the pair was bound, its ids are the leader's).
  // Retired graphs are destroyed after the final synchronise only: up to two replays may still be in flight when a member leaves.
  struct Part { Seq* m[GVL_MAX_DECODE_BATCH]; int n; std::unique_ptr<StepGraph> sg; };
  std::vector<Part> parts;
  std::vector<std::unique_ptr<StepGraph>> retired;
  Seq* live[GVL_MAX_DECODE_BATCH]; int n_live = -1;
  int enq = 0;
  for (;;) {
    if (eos_id >= 0 && enq >= 2) {
      HIPCHK(ctx, hipEventSynchronize(ctx->step_ev[(enq - 2) % 3]));
      for (int b = 0; b < B; ++b) if (!done[b] && *sqs[b]->h_eos != 0) done[b] = true;
    }
    Seq* now[GVL_MAX_DECODE_BATCH]; int n_now = 0;
    for (int b = 0; b < B; ++b) if (!done[b] && sqs[b]->n_gen < max_new && sqs[b]->pos < sqs[b]->max_tokens) now[n_now++] = sqs[b];
    if (n_now == 0) break;
    if (n_now != n_live || memcmp(now, live, sizeof(Seq*) * n_now) != 0) {
      for (auto& p : parts) retired.push_back(std::move(p.sg));
      parts.clear();
      int sizes[GVL_MAX_DECODE_BATCH];   // a leader takes two rows of its part: its follower's comes with it
      for (int k = 0, o = 0, nk = named_parts(ctx, now, n_now, sizes); k < nk; ++k) {
        Part p; p.n = step_rows(ctx, now + o, sizes[k], p.m); p.sg.reset(new StepGraph());
        o += sizes[k]; parts.push_back(std::move(p));
      }
      memcpy(live, now, sizeof(Seq*) * n_now); n_live = n_now;
    }
    for (auto& p : parts) {
      const int rc = decode_step_replay(ctx, p.m, p.n, st, *p.sg);
      if (rc) { (void)hipStreamSynchronize(st); return rc; }
    }
    if (eos_id >= 0) HIPCHK(ctx, hipEventRecord(ctx->step_ev[enq % 3], st));
    ++enq;
  }
  HIPCHK(ctx, hipStreamSynchronize(st));
  for (int b = 0; b < B; ++b) {
    const int n = sqs[b]->n_gen < max_new ? sqs[b]->n_gen : max_new;
    memcpy(out_ids[b], sqs[b]->h_out, (size_t)n * 4);
    int cut = n;
    if (eos_id >= 0) for (int i = 0; i < n; ++i) if (out_ids[b][i] == eos_id) { cut = i + 1; break; }
    *n_out[b] = cut;
  }
  return 0;
}


}  // namespace gvlm
