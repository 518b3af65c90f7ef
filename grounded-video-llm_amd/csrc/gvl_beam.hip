// gvl_beam.hip -- beam search behind the C ABI (include/gvl.h): gvl_beam_search = HF generate(num_beams = k, do_sample = False) (the reference: inference.py:46,170-176 ->
// models/llava_next_video.py:655-661 -> transformers 4.40.1 GenerationMixin._beam_search [ext]) inside the library, and the operator-level entries of its kernels.  Host code
// only: the bookkeeping, the value refusals and the cache reorder's plan are gvl_beam.h (host-only, CPU-tested), the per-step candidates are beam_rows_kernel /
// beam_merge_kernel / beam_normalize_kernel (gvl_pick.hip); the clones of the caller's sequence, the buffers, the processor launch, the teacher-forced step and the copy of
// the hypotheses are the SearchSession's (gvl_search.hip).  gvl_group_beam_search = HF's diverse (group) beam search (_group_beam_search [ext]): the same pieces per
// group, chained on the stream through beam_group_merge_kernel's choice and logits_process_hamming_kernel.
#include "gvl_model.h"
#include "gvl_beam.h"

using namespace gvlm;

namespace {

bool shape_ok(int n, int k) { return k >= 2 && k <= GVL_MAX_DECODE_BATCH && n >= 2 * k && (long long)n * k <= 0x7fffffffLL; }
int beam_status(int rc) { return rc == gvl_beam::BEAM_ERR_ARG ? GVL_ERR_HIP : (rc == gvl_beam::BEAM_ERR_FEW ? GVL_ERR_STATE : GVL_ERR_ARG); }

}  // namespace

extern "C" {

int gvl_op_beam_candidates(gvl_ctx* ctx, const float* rows, int n, int k, int row_stride, const float* beam_scores_host, int rows_are_logprobs, float* vals_dev,
                           int32_t* idx_dev, float* proc_dev, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!rows || !beam_scores_host || !vals_dev || !idx_dev || !proc_dev) return fail(ctx, GVL_ERR_ARG, "gvl_op_beam_candidates: bad arguments");
  if (k < 2 || k > GVL_MAX_DECODE_BATCH) return fail(ctx, GVL_ERR_ARG, "gvl_op_beam_candidates: k (num_beams) must be 2 .. 16");
  if (!shape_ok(n, k)) return fail(ctx, GVL_ERR_ARG, "gvl_op_beam_candidates: n must be >= 2 k and k * n must fit an int32");
  if (row_stride != 0 && row_stride < n) return fail(ctx, GVL_ERR_ARG, "gvl_op_beam_candidates: row_stride must be 0 (every beam reads row 0) or >= n");
  if (const int rc = SearchSession::ensure_scratch(ctx)) return rc;
  hipStream_t st = (hipStream_t)stream;
  BeamCandArgs a; SearchSession::cand_args(ctx, a, rows, n, k, row_stride, beam_scores_host, rows_are_logprobs ? 0 : 1, vals_dev, idx_dev, proc_dev);
  RUN(GVL_PROF_OTHER, 0, gvl_launch_beam_candidates(a, st));
  return 0;
}

int gvl_op_beam_normalize(gvl_ctx* ctx, float* rows, int n, int k, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!rows || k < 1 || k > GVL_MAX_DECODE_BATCH || n < 1) return fail(ctx, GVL_ERR_ARG, "gvl_op_beam_normalize: rows [k][n], k 1 .. 16");
  hipStream_t st = (hipStream_t)stream;
  RUN(GVL_PROF_OTHER, 0, gvl_launch_beam_normalize(rows, n, k, st));
  return 0;
}

int gvl_op_beam_group(gvl_ctx* ctx, const float* rows, int n, int s, int row_stride, const float* beam_scores_host, int rows_are_logprobs, int eos_id, int pad_id,
                      int group_done, float* vals_dev, int32_t* idx_dev, float* proc_dev, int32_t* chosen_dev, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!chosen_dev || s < 1 || s > GVL_MAX_DECODE_BATCH) return fail(ctx, GVL_ERR_ARG, "gvl_op_beam_group: s (beams of the group) must be 1 .. 16, chosen_dev [s]");
  if (!group_done) {
    if (!rows || !beam_scores_host || !vals_dev || !idx_dev || !proc_dev) return fail(ctx, GVL_ERR_ARG, "gvl_op_beam_group: bad arguments");
    if (n < 2 * s || (long long)n * s > 0x7fffffffLL) return fail(ctx, GVL_ERR_ARG, "gvl_op_beam_group: n must be >= 2 s and s * n must fit an int32");
    if (row_stride != 0 && row_stride < n) return fail(ctx, GVL_ERR_ARG, "gvl_op_beam_group: row_stride must be 0 (every beam reads row 0) or >= n");
  }
  if (const int rc = SearchSession::ensure_scratch(ctx)) return rc;
  hipStream_t st = (hipStream_t)stream;
  BeamGroupArgs g; memset(&g, 0, sizeof(g));
  if (!group_done) SearchSession::cand_args(ctx, g.c, rows, n, s, row_stride, beam_scores_host, rows_are_logprobs ? 0 : 1, vals_dev, idx_dev, proc_dev);
  g.c.k = s; g.current = chosen_dev; g.mirror = nullptr; g.eos = eos_id < 0 ? -1 : eos_id; g.pad = pad_id; g.done = group_done ? 1 : 0;
  RUN(GVL_PROF_OTHER, 0, gvl_launch_beam_group(g, st));
  return 0;
}

int gvl_debug_group_beam_tokens(gvl_ctx* ctx, int32_t* out_host, int cap, int* n_out) {
  if (!ctx) return GVL_ERR_ARG;
  if (!n_out || cap < 0 || (cap > 0 && !out_host)) return fail(ctx, GVL_ERR_ARG, "gvl_debug_group_beam_tokens: bad arguments");
  *n_out = (int)ctx->group_beam_tokens.size();
  for (int i = 0; i < cap && i < *n_out; ++i) out_host[i] = ctx->group_beam_tokens[i];
  return 0;
}

int gvl_debug_group_beam_pool(gvl_ctx* ctx, int32_t* out_host, int cap, int* n_out) {
  if (!ctx) return GVL_ERR_ARG;
  if (!n_out || cap < 0 || (cap > 0 && !out_host)) return fail(ctx, GVL_ERR_ARG, "gvl_debug_group_beam_pool: bad arguments");
  *n_out = (int)ctx->group_beam_pool.size();
  for (int i = 0; i < cap && i < *n_out; ++i) out_host[i] = ctx->group_beam_pool[i];
  return 0;
}

int gvl_beam_search(gvl_ctx* ctx, int seq_id, const float* first_logits, const gvl_beam_params* p, int32_t* out_ids_host, int cap, int* n_out, double* sequences_score,
                    float* transition_scores_host, void* stream) {
  return gvl_beam_search_n(ctx, seq_id, first_logits, p, 1, out_ids_host, cap, n_out, sequences_score, transition_scores_host, stream);
}
// the search itself; the num_return best hypotheses leave through BeamState::finalize_n (messages name gvl_beam_search: one search, two entry points)
int gvl_beam_search_n(gvl_ctx* ctx, int seq_id, const float* first_logits, const gvl_beam_params* p, int num_return, int32_t* out_ids_host, int cap, int* n_out,
                      double* sequences_scores, float* transition_scores_host, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_beam_search");
  if (!p || !first_logits || !out_ids_host || !n_out) return fail(ctx, GVL_ERR_ARG, "gvl_beam_search: bad arguments");
  const int k = p->num_beams, V = ctx->cfg.vocab, max_new = p->max_new_tokens;
  const std::string why = gvl_beam::refusal(false, k, 0, 0.f, num_return, V, max_new, ctx->outlist_cap, cap, p->early_stopping, p->length_penalty, p->penalty, p->ngram, p->min_new);
  if (!why.empty()) return fail(ctx, GVL_ERR_ARG, "gvl_beam_search: " + why);
  hipStream_t st = (hipStream_t)stream;
  SearchSession ss(ctx, "gvl_beam_search", st);
  if (const int rc = ss.open(seq_id, p->penalty, p->ngram, p->min_new, p->proc_eos_id, p->rules_id, max_new, false)) return rc;

  gvl_beam::BeamState bs;
  if (bs.init(k, V, max_new, p->eos_id, p->length_penalty, p->early_stopping) < 0) return fail(ctx, GVL_ERR_ARG, "gvl_beam_search: bad arguments");

  std::vector<int> beams(1, ss.root), parents(k), toks(k);
  const float* rows = first_logits; int stride = 0, n_rows = 1;       // the first step: every beam reads the prompt's row

  for (;;) {
    if (ss.processed) {
      // HF's order: log-softmax -> processors (token rules around them) -> + beam score -> top-2k.  In place on the library's rows; the caller's first_logits are copied first.
      float* work = const_cast<float*>(rows);
      if (stride == 0) { if (const int rc = ss.copy_first(first_logits, &work)) return rc; rows = work; }
      RUN(GVL_PROF_OTHER, 0, gvl_launch_beam_normalize(work, V, n_rows, st));
      const std::vector<int>* hist[GVL_MAX_DECODE_BATCH];
      for (int b = 0; b < n_rows; ++b) hist[b] = &bs.seqs[b];
      if (const int rc = ss.upload_histories(n_rows, (int)bs.seqs[0].size(), hist)) return rc;
      if (const int rc = ss.process(work, 0, n_rows)) return rc;
    }
    BeamCandArgs ca; SearchSession::cand_args(ctx, ca, rows, V, k, stride, bs.scores.data(), ss.processed ? 0 : 1, ss.d_vals, ss.d_idx, ss.d_proc);
    RUN(GVL_PROF_OTHER, 0, gvl_launch_beam_candidates(ca, st));
    HIPCHK(ctx, hipStreamSynchronize(st));               // the ONE synchronise of the step: the candidates sit in host-mapped memory
    const int rc = bs.step(ss.h_vals, ss.h_idx, ss.h_proc, 2 * k, parents.data(), toks.data());
    if (rc < 0) return fail(ctx, beam_status(rc), std::string("gvl_beam_search: ") + gvl_beam::status_text(rc));
    if (rc == gvl_beam::BEAM_FINISHED) break;

    if (const int rrc = ss.reorder(beams, parents.data(), k)) return rrc;
    Seq* sqs[GVL_MAX_DECODE_BATCH];
    for (int j = 0; j < k; ++j) sqs[j] = &ctx->seqs[beams[j]];
    float* next_rows = nullptr;
    if (const int arc = ss.advance(sqs, k, toks.data(), nullptr, &next_rows)) return arc;
    rows = next_rows; stride = V; n_rows = k;
  }

  std::vector<std::vector<int>> ids; std::vector<double> score; std::vector<std::vector<float>> ts;
  const int got = bs.finalize_n(num_return, &ids, &score, &ts);
  return ss.write_hypotheses(got, num_return, ids, score, ts, out_ids_host, cap, n_out, sequences_scores, transition_scores_host);
}

// Diverse (group) beam search (gvl.h).  beams[j] = the sequence of global beam j, -1 once its group is done (closed at once).  The live beams are stepped together; their
// rows sit compacted, in beam order, so a group's rows are contiguous.
int gvl_group_beam_search(gvl_ctx* ctx, int seq_id, const float* first_logits, const gvl_group_beam_params* gp, int num_return, int32_t* out_ids_host, int cap, int* n_out,
                          double* sequences_scores, float* transition_scores_host, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_group_beam_search");
  if (!gp || !first_logits || !out_ids_host || !n_out) return fail(ctx, GVL_ERR_ARG, "gvl_group_beam_search: bad arguments");
  const gvl_beam_params* p = &gp->base;
  const int k = p->num_beams, G = gp->num_beam_groups, V = ctx->cfg.vocab, max_new = p->max_new_tokens;
  const float lambda = gp->diversity_penalty;
  const std::string why = gvl_beam::refusal(true, k, G, lambda, num_return, V, max_new, ctx->outlist_cap, cap, p->early_stopping, p->length_penalty, p->penalty, p->ngram, p->min_new);
  if (!why.empty()) return fail(ctx, GVL_ERR_ARG, "gvl_group_beam_search: " + why);
  const int s = k / G;
  hipStream_t st = (hipStream_t)stream;
  SearchSession ss(ctx, "gvl_group_beam_search", st);
  if (const int rc = ss.open(seq_id, p->penalty, p->ngram, p->min_new, p->proc_eos_id, p->rules_id, max_new, false)) return rc;

  gvl_beam::GroupBeamState gs;
  if (gs.init(k, G, V, max_new, p->eos_id, gp->pad_id, p->length_penalty, p->early_stopping) < 0) return fail(ctx, GVL_ERR_ARG, "gvl_group_beam_search: bad arguments");
  ctx->group_beam_tokens.clear(); ctx->group_beam_pool.clear();

  std::vector<int> beams(1, ss.root), parents(k), toks(k), row_of(k, 0);
  bool first = true;
  float* rows = nullptr;                                   // the first step: one work row per GROUP (the groups' rows differ after processing), every beam of a group reads it

  for (;;) {
    // every row is normalised once; the first step's G work rows are copies of the normalised prompt row
    int n_rows = 0;
    if (first) {
      if (const int rc = ss.copy_first(first_logits, &rows)) return rc;
      RUN(GVL_PROF_OTHER, 0, gvl_launch_beam_normalize(rows, V, 1, st));
      for (int g = 1; g < G; ++g) HIPCHK(ctx, hipMemcpyAsync(rows + (size_t)g * V, rows, (size_t)V * 4, hipMemcpyDeviceToDevice, st));
      for (int j = 0; j < k; ++j) row_of[j] = j / s;
      n_rows = G;
    } else {
      for (int j = 0; j < k; ++j) if (beams[j] >= 0) row_of[j] = n_rows++;
      RUN(GVL_PROF_OTHER, 0, gvl_launch_beam_normalize(rows, V, n_rows, st));
    }
    // the live beams' histories, one upload per step (row r of the work rows <-> history r)
    const std::vector<int>* hist[GVL_MAX_DECODE_BATCH] = {};
    for (int j = 0; j < k; ++j) if (!gs.group_done(j / s) && !(first && j % s != 0)) hist[row_of[j]] = &gs.seq(j);
    if (const int rc = ss.upload_histories(n_rows, gs.n_gen, hist)) return rc;

    for (int g = 0; g < G; ++g) {
      BeamGroupArgs ga; memset(&ga, 0, sizeof(ga));
      ga.c.k = s; ga.current = ss.d_chosen + g * s; ga.mirror = ss.d_chosen_mirror + g * s; ga.eos = p->eos_id < 0 ? -1 : p->eos_id; ga.pad = gp->pad_id; ga.done = gs.group_done(g) ? 1 : 0;
      if (!ga.done) {
        const int r0 = row_of[g * s], nb = first ? 1 : s;
        float* work = rows + (size_t)r0 * V;
        // the Hamming term against the tokens the groups before this one chose at this step rides in the processor launch
        if (ss.processed || g > 0) { if (const int rc = ss.process(work, r0, nb, ss.d_chosen, g * s, lambda)) return rc; }
        float sc[GVL_MAX_DECODE_BATCH];
        for (int b = 0; b < s; ++b) sc[b] = gs.score(g * s + b);
        SearchSession::cand_args(ctx, ga.c, work, V, s, first ? 0 : V, sc, 0, ss.d_vals + g * 2 * s, ss.d_idx + g * 2 * s, ss.d_proc + g * 2 * s);
      }
      RUN(GVL_PROF_OTHER, 0, gvl_launch_beam_group(ga, st));
    }
    HIPCHK(ctx, hipStreamSynchronize(st));               // the ONE synchronise of the step: candidates and chosen tokens sit in host-mapped memory
    const int rc = gs.step(ss.h_vals, ss.h_idx, ss.h_proc, 2 * s, parents.data(), toks.data());
    if (rc < 0) return fail(ctx, beam_status(rc), std::string("gvl_group_beam_search: ") + gvl_beam::status_text(rc));
    for (int j = 0; j < k; ++j) {
      ctx->group_beam_tokens.push_back(ss.h_chosen[j]);
      if (ss.h_chosen[j] != toks[j]) return fail(ctx, GVL_ERR_HIP, "gvl_group_beam_search: the device's choice of a group's tokens differs from the host bookkeeping's");
    }
    if (rc == gvl_beam::BEAM_FINISHED) break;
    for (int j = 0; j < k; ++j) if (gs.group_done(j / s)) parents[j] = -1;      // a group that is done now is never read again: its beams are not even stepped once more

    // a parent without a child -- every beam of a group that is done now -- goes back to the pool at once
    if (const int rrc = ss.reorder(beams, parents.data(), k)) return rrc;
    ctx->group_beam_pool.push_back((int)ss.ids.size()); ctx->group_beam_pool.push_back((int)ctx->free_pages.size());

    Seq* sqs[GVL_MAX_DECODE_BATCH]; int live_toks[GVL_MAX_DECODE_BATCH], n_live = 0;
    for (int j = 0; j < k; ++j) if (beams[j] >= 0) { sqs[n_live] = &ctx->seqs[beams[j]]; live_toks[n_live++] = toks[j]; }
    if (const int arc = ss.advance(sqs, n_live, live_toks, nullptr, &rows)) return arc;
    first = false;
  }

  std::vector<std::vector<int>> ids; std::vector<double> score; std::vector<std::vector<float>> ts;
  const int got = gs.finalize_n(num_return, &ids, &score, &ts);
  return ss.write_hypotheses(got, num_return, ids, score, ts, out_ids_host, cap, n_out, sequences_scores, transition_scores_host);
}

}  // extern "C"
