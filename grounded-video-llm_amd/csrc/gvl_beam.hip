// gvl_beam.hip -- beam search behind the C ABI (include/gvl.h): gvl_beam_search = HF generate(num_beams = k, do_sample = False) (the reference: inference.py:46,170-176 ->
// models/llava_next_video.py:655-661 -> transformers 4.40.1 GenerationMixin._beam_search [ext]) inside the library, and the operator-level entries of its kernels.  Host code
// only: the bookkeeping is gvl_beam.h (host-only, CPU-tested), the per-step candidates are beam_rows_kernel / beam_merge_kernel / beam_normalize_kernel (gvl_pick.hip), the
// beams advance through decode_step (gvl_llm.hip) on clones of the caller's sequence.  gvl_group_beam_search = HF's diverse (group) beam search (_group_beam_search [ext]):
// the same pieces per group, chained on the stream through beam_group_merge_kernel's choice and logits_process_hamming_kernel.
#include "gvl_model.h"
#include "gvl_beam.h"

using namespace gvlm;

namespace {

constexpr int kMaxCand = 2 * GVL_MAX_DECODE_BATCH;
// behind the survivors (device) and behind one step's candidates (host-mapped): the tokens the groups of a diverse beam search chose at this step
constexpr size_t kScratchFloats = (size_t)GVL_MAX_DECODE_BATCH * kMaxCand * 3, kCandFloats = (size_t)kMaxCand * 3;

// the small buffers every candidate launch needs: the per-row survivors between the two launches (device) and one step's result (host-mapped, as the generated ids are)
int ensure_beam_scratch(gvl_ctx* ctx) {
  if (!ctx->d_beam_scratch) HIPCHK(ctx, hipMalloc((void**)&ctx->d_beam_scratch, (kScratchFloats + GVL_MAX_DECODE_BATCH) * 4));
  if (!ctx->h_beam_cand) {
    HIPCHK(ctx, hipHostMalloc((void**)&ctx->h_beam_cand, (kCandFloats + GVL_MAX_DECODE_BATCH) * 4, hipHostMallocMapped));
    memset(ctx->h_beam_cand, 0, (kCandFloats + GVL_MAX_DECODE_BATCH) * 4);
    HIPCHK(ctx, hipHostGetDevicePointer((void**)&ctx->d_beam_cand, ctx->h_beam_cand, 0));
  }
  return 0;
}
// ... and what a whole search needs: [16][vocab] work rows (beams stepped in several parts are gathered here; the processors' in-place target on the first step) and the
// beams' histories for the logits processors
int ensure_beam_search_buffers(gvl_ctx* ctx) {
  if (const int rc = ensure_beam_scratch(ctx)) return rc;
  if (!ctx->d_beam_rows) HIPCHK(ctx, hipMalloc((void**)&ctx->d_beam_rows, (size_t)GVL_MAX_DECODE_BATCH * ctx->cfg.vocab * 4));
  if (!ctx->d_beam_hist) HIPCHK(ctx, hipMalloc((void**)&ctx->d_beam_hist, ((size_t)GVL_MAX_DECODE_BATCH * GVL_LOGITS_HIST_CAP + GVL_MAX_DECODE_BATCH) * 4));
  return 0;
}
void fill_cand_args(gvl_ctx* ctx, BeamCandArgs& a, const float* rows, int n, int k, int row_stride, const float* scores, int norm, float* vals, int* idx, float* proc) {
  memset(&a, 0, sizeof(a));
  a.rows = rows; a.n = n; a.k = k; a.row_stride = row_stride; a.norm = norm;
  for (int b = 0; b < k; ++b) a.scores[b] = scores[b];
  float* s = (float*)ctx->d_beam_scratch;
  a.row_v = s; a.row_i = (int*)(s + GVL_MAX_DECODE_BATCH * kMaxCand); a.row_lp = s + 2 * GVL_MAX_DECODE_BATCH * kMaxCand;
  a.vals = vals; a.idx = idx; a.proc = proc;
}
bool shape_ok(int n, int k) { return k >= 2 && k <= GVL_MAX_DECODE_BATCH && n >= 2 * k && (long long)n * k <= 0x7fffffffLL; }

// every sequence the search made goes back on every return path
struct Owned {
  gvl_ctx* ctx; std::vector<int> ids;
  explicit Owned(gvl_ctx* c) : ctx(c) {}
  ~Owned() { for (int id : ids) ctx->close(id); }
  void drop(int id) { ids.erase(std::find(ids.begin(), ids.end(), id)); ctx->close(id); }
};

}  // namespace

// what gvl_contrastive_search (gvl_contrastive.hip) shares with the beam searches: the work buffers and the candidate launch's arguments
int gvlm::beam_search_buffers(gvl_ctx* ctx) { return ensure_beam_search_buffers(ctx); }
void gvlm::beam_cand_args(gvl_ctx* ctx, BeamCandArgs& a, const float* rows, int n, int k, int row_stride, const float* scores, int norm, float* vals, int* idx, float* proc) {
  fill_cand_args(ctx, a, rows, n, k, row_stride, scores, norm, vals, idx, proc);
}
gvlm::BeamCandBufs gvlm::beam_cand_bufs(gvl_ctx* ctx) {
  BeamCandBufs b;
  b.h_vals = (float*)ctx->h_beam_cand; b.h_idx = (int*)(b.h_vals + kMaxCand); b.h_proc = b.h_vals + 2 * kMaxCand;
  b.d_vals = (float*)ctx->d_beam_cand; b.d_idx = (int*)(b.d_vals + kMaxCand); b.d_proc = b.d_vals + 2 * kMaxCand;
  return b;
}

extern "C" {

int gvl_op_beam_candidates(gvl_ctx* ctx, const float* rows, int n, int k, int row_stride, const float* beam_scores_host, int rows_are_logprobs, float* vals_dev,
                           int32_t* idx_dev, float* proc_dev, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!rows || !beam_scores_host || !vals_dev || !idx_dev || !proc_dev) return fail(ctx, GVL_ERR_ARG, "gvl_op_beam_candidates: bad arguments");
  if (k < 2 || k > GVL_MAX_DECODE_BATCH) return fail(ctx, GVL_ERR_ARG, "gvl_op_beam_candidates: k (num_beams) must be 2 .. 16");
  if (!shape_ok(n, k)) return fail(ctx, GVL_ERR_ARG, "gvl_op_beam_candidates: n must be >= 2 k and k * n must fit an int32");
  if (row_stride != 0 && row_stride < n) return fail(ctx, GVL_ERR_ARG, "gvl_op_beam_candidates: row_stride must be 0 (every beam reads row 0) or >= n");
  if (const int rc = ensure_beam_scratch(ctx)) return rc;
  hipStream_t st = (hipStream_t)stream;
  BeamCandArgs a; fill_cand_args(ctx, a, rows, n, k, row_stride, beam_scores_host, rows_are_logprobs ? 0 : 1, vals_dev, idx_dev, proc_dev);
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
  if (const int rc = ensure_beam_scratch(ctx)) return rc;
  hipStream_t st = (hipStream_t)stream;
  BeamGroupArgs g; memset(&g, 0, sizeof(g));
  if (!group_done) fill_cand_args(ctx, g.c, rows, n, s, row_stride, beam_scores_host, rows_are_logprobs ? 0 : 1, vals_dev, idx_dev, proc_dev);
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
  if (num_return < 1 || num_return > k) return fail(ctx, GVL_ERR_ARG, "gvl_beam_search: num_return must be 1 .. num_beams");
  if (k < 2 || k > GVL_MAX_DECODE_BATCH) return fail(ctx, GVL_ERR_ARG, "gvl_beam_search: num_beams must be 2 .. 16");
  if (V < 2 * k) return fail(ctx, GVL_ERR_ARG, "gvl_beam_search: vocabulary smaller than 2 x num_beams");
  if (!shape_ok(V, k)) return fail(ctx, GVL_ERR_ARG, "gvl_beam_search: num_beams x vocabulary must fit an int32");
  if (max_new < 1 || max_new > ctx->outlist_cap) return fail(ctx, GVL_ERR_ARG, "gvl_beam_search: max_new_tokens must be 1 .. " + std::to_string(ctx->outlist_cap));
  if (cap < max_new) return fail(ctx, GVL_ERR_ARG, "gvl_beam_search: cap (room of out_ids_host) must be >= max_new_tokens");
  if (p->early_stopping < 0 || p->early_stopping > 2) return fail(ctx, GVL_ERR_ARG, "gvl_beam_search: early_stopping must be 0 (False), 1 (True) or 2 (\"never\")");
  if (p->early_stopping == 2 && p->length_penalty > 0.0) return fail(ctx, GVL_ERR_ARG, std::string("gvl_beam_search: ") + gvl_beam::status_text(gvl_beam::BEAM_ERR_NEVER));
  if (!(p->length_penalty == p->length_penalty)) return fail(ctx, GVL_ERR_ARG, "gvl_beam_search: length_penalty is NaN");
  if (!(p->penalty > 0.f) || p->ngram < 0 || p->min_new < 0) return fail(ctx, GVL_ERR_ARG, "gvl_beam_search: penalty must be > 0, ngram >= 0, min_new >= 0");
  if (p->rules_id != -1 && (p->rules_id < 0 || ctx->check_rules(p->rules_id))) return seq_fail(ctx, "gvl_beam_search", SEQ_NO_RULES);
  if (!ctx->lookup(seq_id)) return seq_fail(ctx, "gvl_beam_search", SEQ_BAD);
  if (const int rc = pair_refuse(ctx, "gvl_beam_search", seq_id, true)) return rc;
  if (const int rc = bank_refuse(ctx, "gvl_beam_search", seq_id)) return rc;
  const int pos0 = ctx->seqs[seq_id].pos;
  if (pos0 <= 0) return fail(ctx, GVL_ERR_STATE, "gvl_beam_search: the sequence is not prefilled");
  if (const int rc = ensure_beam_search_buffers(ctx)) return rc;
  hipStream_t st = (hipStream_t)stream;

  LogitsProc proc{p->penalty, p->ngram, p->min_new, p->proc_eos_id < 0 ? -1 : p->proc_eos_id};
  // the grammar the caller's sequence carries (gvl_seq_set_grammar) constrains every beam; read here, before the clones' options go off below.  The sequence holds
  // its reference for the whole call, so the blob outlives every launch
  const int grammar_id = ctx->seqs[seq_id].sel.grammar;
  const GrammarDev* grammar = grammar_id >= 0 ? (const GrammarDev*)ctx->grammars[grammar_id].d : nullptr;
  const bool processed = proc.on() || p->rules_id >= 0 || grammar;
  const TokenRulesDev* rules = p->rules_id >= 0 ? (const TokenRulesDev*)ctx->rule_sets[p->rules_id].d : nullptr;
  const int seq_cap = std::min(pos0 + max_new + 1, (int)ctx->cfg.max_seq);

  gvl_beam::BeamState bs;
  if (bs.init(k, V, max_new, p->eos_id, p->length_penalty, p->early_stopping) < 0) return fail(ctx, GVL_ERR_ARG, "gvl_beam_search: bad arguments");

  // The beams are clones of the caller's sequence (it is never stepped: on return it is where it was).  Their selection options are off -- clones copy that -- so a step's
  // own token pick leaves the logits rows raw; the scores come from the candidate kernels below.
  Owned own(ctx);
  auto clone = [&](int src, int* dst) {
    const int rc = seq_clone(ctx, src, seq_cap, dst, (hipStream_t)stream, false);   // the search keeps the beams' histories itself (d_beam_hist)
    if (rc == 0) own.ids.push_back(*dst);
    return rc;
  };
  std::vector<int> beams(1, -1);
  if (const int rc = clone(seq_id, &beams[0])) return rc;
  { SeqSelect& sel = ctx->seqs[beams[0]].sel;
    sel.proc = LogitsProc(); ctx->set_rules(sel, -1); ctx->set_grammar(sel, -1); sel.top_n = -1;
    const Sampling greedy; ctx->set_sampling(sel, &greedy); }

  float* h_vals = (float*)ctx->h_beam_cand; int* h_idx = (int*)(h_vals + kMaxCand); float* h_proc = h_vals + 2 * kMaxCand;
  float* d_vals = (float*)ctx->d_beam_cand; int* d_idx = (int*)(d_vals + kMaxCand); float* d_proc = d_vals + 2 * kMaxCand;
  int* d_hist = ctx->d_beam_hist; int* d_lens = ctx->d_beam_hist + (size_t)GVL_MAX_DECODE_BATCH * GVL_LOGITS_HIST_CAP;
  std::vector<int> h_hist, parents(k), toks(k);
  const float* rows = first_logits; int stride = 0, n_rows = 1;       // the first step: every beam reads the prompt's row

  for (;;) {
    if (processed) {
      // HF's order: log-softmax -> processors (token rules around them) -> + beam score -> top-2k.  In place on the library's rows; the caller's first_logits are copied first.
      float* work = const_cast<float*>(rows);
      if (stride == 0) { work = ctx->d_beam_rows; HIPCHK(ctx, hipMemcpyAsync(work, first_logits, (size_t)V * 4, hipMemcpyDeviceToDevice, st)); rows = work; }
      RUN(GVL_PROF_OTHER, 0, gvl_launch_beam_normalize(work, V, n_rows, st));
      const int len = (int)bs.seqs[0].size(), hs = len > 0 ? std::min(len, (int)GVL_LOGITS_HIST_CAP) : 1;
      h_hist.assign((size_t)n_rows * hs + GVL_MAX_DECODE_BATCH, 0);
      for (int b = 0; b < n_rows; ++b) for (int i = 0; i < hs && i < len; ++i) h_hist[(size_t)b * hs + i] = bs.seqs[b][i];
      for (int b = 0; b < n_rows; ++b) h_hist[(size_t)n_rows * hs + b] = len;
      HIPCHK(ctx, hipMemcpyAsync(d_hist, h_hist.data(), (size_t)n_rows * hs * 4, hipMemcpyHostToDevice, st));
      HIPCHK(ctx, hipMemcpyAsync(d_lens, h_hist.data() + (size_t)n_rows * hs, (size_t)n_rows * 4, hipMemcpyHostToDevice, st));
      LogitsProcArgs lp; memset(&lp, 0, sizeof(lp));
      lp.logits = work; lp.n = V; lp.ld = V; lp.batch = n_rows; lp.cap = hs;
      for (int b = 0; b < n_rows; ++b) {
        lp.hist[b] = d_hist + (size_t)b * hs; lp.len_ptrs[b] = d_lens + b;
        lp.penalty[b] = proc.penalty; lp.ngram[b] = proc.ngram; lp.eos[b] = proc.eos; lp.min_new[b] = proc.eos >= 0 ? proc.min_new : 0; lp.rules[b] = rules; lp.grammar[b] = grammar;
      }
      RUN(GVL_PROF_OTHER, 0, gvl_launch_logits_process(lp, st));
    }
    BeamCandArgs ca; fill_cand_args(ctx, ca, rows, V, k, stride, bs.scores.data(), processed ? 0 : 1, d_vals, d_idx, d_proc);
    RUN(GVL_PROF_OTHER, 0, gvl_launch_beam_candidates(ca, st));
    HIPCHK(ctx, hipStreamSynchronize(st));               // the candidates sit in host-mapped memory; h_hist is free again
    const int rc = bs.step(h_vals, h_idx, h_proc, 2 * k, parents.data(), toks.data());
    if (rc < 0) return fail(ctx, rc == gvl_beam::BEAM_ERR_ARG ? GVL_ERR_HIP : (rc == gvl_beam::BEAM_ERR_FEW ? GVL_ERR_STATE : GVL_ERR_ARG), std::string("gvl_beam_search: ") + gvl_beam::status_text(rc));
    if (rc == gvl_beam::BEAM_FINISHED) break;

    // HF's cache reorder: the first child of a parent keeps the parent's sequence, every further child is a clone of it (made while the parent is still at the length the
    // children continue from); parents without a child go back to the pool
    std::vector<int> keep(beams.size(), -1), next(k, -1);
    for (int j = 0; j < k; ++j) {
      const int pj = parents[j];
      if (keep[pj] >= 0) { if (const int crc = clone(beams[pj], &next[j])) return crc; }
      else keep[pj] = j;
    }
    for (size_t q = 0; q < beams.size(); ++q) if (keep[q] >= 0) next[keep[q]] = beams[q];
    for (size_t q = 0; q < beams.size(); ++q) if (keep[q] < 0) own.drop(beams[q]);
    beams = next;

    // one teacher-forced step of the k beams, in the parts the decode path takes (any size up to 16 on the skinny-MFMA path: one part; 4 / 2 / 1 on the VALU fallback); a
    // row does not depend on the part it was computed in
    Seq* sqs[GVL_MAX_DECODE_BATCH];
    for (int j = 0; j < k; ++j) {
      sqs[j] = &ctx->seqs[beams[j]];
      if (sqs[j]->pos >= sqs[j]->max_tokens) return fail(ctx, GVL_ERR_ARG, "gvl_beam_search: the context is full (cfg.max_seq) before max_new_tokens");
      RUN(GVL_PROF_OTHER, 0, gvl_launch_set_int(sqs[j]->d_tok, toks[j], st));
    }
    int sizes[GVL_MAX_DECODE_BATCH];
    const int n_parts = decode_parts(ctx->decode_mfma, k, sizes);
    const bool one_part = n_parts == 1;
    for (int p = 0, o = 0; p < n_parts; ++p) {
      const int nb = sizes[p];
      if (const int drc = decode_step(ctx, sqs + o, nb, st)) return drc;
      if (!one_part) HIPCHK(ctx, hipMemcpyAsync(ctx->d_beam_rows + (size_t)o * V, ctx->d_logits, (size_t)nb * V * 4, hipMemcpyDeviceToDevice, st));
      o += nb;
    }
    rows = one_part ? ctx->d_logits : ctx->d_beam_rows; stride = V; n_rows = k;
  }

  std::vector<std::vector<int>> ids; std::vector<double> score; std::vector<std::vector<float>> ts;
  const int got = bs.finalize_n(num_return, &ids, &score, &ts);
  if (got < num_return) return fail(ctx, GVL_ERR_STATE, "gvl_beam_search: fewer hypotheses than num_return");
  for (int r = 0; r < num_return; ++r) {
    const int n = (int)ids[r].size();                     // <= max_new <= cap
    for (int i = 0; i < n; ++i) out_ids_host[(size_t)r * cap + i] = ids[r][i];
    n_out[r] = n;
    if (sequences_scores) sequences_scores[r] = score[r];
    if (transition_scores_host) for (int i = 0; i < n && i < (int)ts[r].size(); ++i) transition_scores_host[(size_t)r * cap + i] = ts[r][i];
  }
  return 0;
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
  if (k < 2 || k > GVL_MAX_DECODE_BATCH) return fail(ctx, GVL_ERR_ARG, "gvl_group_beam_search: num_beams must be 2 .. 16");
  if (G < 2 || G > k || k % G != 0) return fail(ctx, GVL_ERR_ARG, "gvl_group_beam_search: num_beam_groups must be 2 .. num_beams and divide num_beams");
  if (!(lambda > 0.f)) return fail(ctx, GVL_ERR_ARG, "gvl_group_beam_search: diversity_penalty must be > 0");
  const int s = k / G;
  if (num_return < 1 || num_return > k) return fail(ctx, GVL_ERR_ARG, "gvl_group_beam_search: num_return must be 1 .. num_beams");
  if (V < 2 * s) return fail(ctx, GVL_ERR_ARG, "gvl_group_beam_search: vocabulary smaller than 2 x the beams of a group");
  if ((long long)V * s > 0x7fffffffLL) return fail(ctx, GVL_ERR_ARG, "gvl_group_beam_search: beams of a group x vocabulary must fit an int32");
  if (max_new < 1 || max_new > ctx->outlist_cap) return fail(ctx, GVL_ERR_ARG, "gvl_group_beam_search: max_new_tokens must be 1 .. " + std::to_string(ctx->outlist_cap));
  if (cap < max_new) return fail(ctx, GVL_ERR_ARG, "gvl_group_beam_search: cap (room of out_ids_host) must be >= max_new_tokens");
  if (p->early_stopping < 0 || p->early_stopping > 2) return fail(ctx, GVL_ERR_ARG, "gvl_group_beam_search: early_stopping must be 0 (False), 1 (True) or 2 (\"never\")");
  if (p->early_stopping == 2 && p->length_penalty > 0.0) return fail(ctx, GVL_ERR_ARG, std::string("gvl_group_beam_search: ") + gvl_beam::status_text(gvl_beam::BEAM_ERR_NEVER));
  if (!(p->length_penalty == p->length_penalty)) return fail(ctx, GVL_ERR_ARG, "gvl_group_beam_search: length_penalty is NaN");
  if (!(p->penalty > 0.f) || p->ngram < 0 || p->min_new < 0) return fail(ctx, GVL_ERR_ARG, "gvl_group_beam_search: penalty must be > 0, ngram >= 0, min_new >= 0");
  if (p->rules_id != -1 && (p->rules_id < 0 || ctx->check_rules(p->rules_id))) return seq_fail(ctx, "gvl_group_beam_search", SEQ_NO_RULES);
  if (!ctx->lookup(seq_id)) return seq_fail(ctx, "gvl_group_beam_search", SEQ_BAD);
  if (const int rc = pair_refuse(ctx, "gvl_group_beam_search", seq_id, true)) return rc;
  if (const int rc = bank_refuse(ctx, "gvl_group_beam_search", seq_id)) return rc;
  const int pos0 = ctx->seqs[seq_id].pos;
  if (pos0 <= 0) return fail(ctx, GVL_ERR_STATE, "gvl_group_beam_search: the sequence is not prefilled");
  if (const int rc = ensure_beam_search_buffers(ctx)) return rc;
  hipStream_t st = (hipStream_t)stream;

  LogitsProc proc{p->penalty, p->ngram, p->min_new, p->proc_eos_id < 0 ? -1 : p->proc_eos_id};
  const int grammar_id = ctx->seqs[seq_id].sel.grammar;
  const GrammarDev* grammar = grammar_id >= 0 ? (const GrammarDev*)ctx->grammars[grammar_id].d : nullptr;
  const bool processed = proc.on() || p->rules_id >= 0 || grammar;
  const TokenRulesDev* rules = p->rules_id >= 0 ? (const TokenRulesDev*)ctx->rule_sets[p->rules_id].d : nullptr;
  const int seq_cap = std::min(pos0 + max_new + 1, (int)ctx->cfg.max_seq);

  gvl_beam::GroupBeamState gs;
  if (gs.init(k, G, V, max_new, p->eos_id, gp->pad_id, p->length_penalty, p->early_stopping) < 0) return fail(ctx, GVL_ERR_ARG, "gvl_group_beam_search: bad arguments");
  ctx->group_beam_tokens.clear(); ctx->group_beam_pool.clear();

  Owned own(ctx);
  auto clone = [&](int src, int* dst) {
    const int rc = seq_clone(ctx, src, seq_cap, dst, (hipStream_t)stream, false);
    if (rc == 0) own.ids.push_back(*dst);
    return rc;
  };
  std::vector<int> beams(1, -1);
  if (const int rc = clone(seq_id, &beams[0])) return rc;
  { SeqSelect& sel = ctx->seqs[beams[0]].sel;
    sel.proc = LogitsProc(); ctx->set_rules(sel, -1); ctx->set_grammar(sel, -1); sel.top_n = -1;
    const Sampling greedy; ctx->set_sampling(sel, &greedy); }

  float* h_vals = (float*)ctx->h_beam_cand; int* h_idx = (int*)(h_vals + kMaxCand); float* h_proc = h_vals + 2 * kMaxCand; int* h_cur = (int*)(h_vals + kCandFloats);
  float* d_vals = (float*)ctx->d_beam_cand; int* d_idx = (int*)(d_vals + kMaxCand); float* d_proc = d_vals + 2 * kMaxCand; int* d_cur_mirror = (int*)(d_vals + kCandFloats);
  int* d_cur = (int*)((float*)ctx->d_beam_scratch + kScratchFloats);
  int* d_hist = ctx->d_beam_hist; int* d_lens = ctx->d_beam_hist + (size_t)GVL_MAX_DECODE_BATCH * GVL_LOGITS_HIST_CAP;
  std::vector<int> h_hist, parents(k), toks(k), row_of(k, 0);
  bool first = true;
  float* rows = ctx->d_beam_rows;                          // the first step: one work row per GROUP (the groups' rows differ after processing), every beam of a group reads it

  for (;;) {
    // every row is normalised once; the first step's G work rows are copies of the normalised prompt row
    int n_rows = 0;
    if (first) {
      HIPCHK(ctx, hipMemcpyAsync(rows, first_logits, (size_t)V * 4, hipMemcpyDeviceToDevice, st));
      RUN(GVL_PROF_OTHER, 0, gvl_launch_beam_normalize(rows, V, 1, st));
      for (int g = 1; g < G; ++g) HIPCHK(ctx, hipMemcpyAsync(rows + (size_t)g * V, rows, (size_t)V * 4, hipMemcpyDeviceToDevice, st));
      for (int j = 0; j < k; ++j) row_of[j] = j / s;
      n_rows = G;
    } else {
      for (int j = 0; j < k; ++j) if (beams[j] >= 0) row_of[j] = n_rows++;
      RUN(GVL_PROF_OTHER, 0, gvl_launch_beam_normalize(rows, V, n_rows, st));
    }
    // the live beams' histories, one upload per step (row r of the work rows <-> history r)
    const int len = gs.n_gen, hs = len > 0 ? std::min(len, (int)GVL_LOGITS_HIST_CAP) : 1;
    h_hist.assign((size_t)n_rows * hs + GVL_MAX_DECODE_BATCH, 0);
    for (int j = 0; j < k; ++j) {
      if (gs.group_done(j / s) || (first && j % s != 0)) continue;
      const std::vector<int>& q = gs.seq(j);
      for (int i = 0; i < hs && i < len; ++i) h_hist[(size_t)row_of[j] * hs + i] = q[i];
    }
    for (int r = 0; r < n_rows; ++r) h_hist[(size_t)n_rows * hs + r] = len;
    HIPCHK(ctx, hipMemcpyAsync(d_hist, h_hist.data(), (size_t)n_rows * hs * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_lens, h_hist.data() + (size_t)n_rows * hs, (size_t)n_rows * 4, hipMemcpyHostToDevice, st));

    for (int g = 0; g < G; ++g) {
      BeamGroupArgs ga; memset(&ga, 0, sizeof(ga));
      ga.c.k = s; ga.current = d_cur + g * s; ga.mirror = d_cur_mirror + g * s; ga.eos = p->eos_id < 0 ? -1 : p->eos_id; ga.pad = gp->pad_id; ga.done = gs.group_done(g) ? 1 : 0;
      if (!ga.done) {
        const int r0 = row_of[g * s], nb = first ? 1 : s;
        float* work = rows + (size_t)r0 * V;
        if (processed || g > 0) {
          LogitsProcArgs lp; memset(&lp, 0, sizeof(lp));
          lp.logits = work; lp.n = V; lp.ld = V; lp.batch = nb; lp.cap = hs;
          for (int b = 0; b < nb; ++b) {
            lp.hist[b] = d_hist + (size_t)(r0 + b) * hs; lp.len_ptrs[b] = d_lens + r0 + b;
            lp.penalty[b] = proc.penalty; lp.ngram[b] = proc.ngram; lp.eos[b] = proc.eos; lp.min_new[b] = proc.eos >= 0 ? proc.min_new : 0; lp.rules[b] = rules; lp.grammar[b] = grammar;
            lp.ham_tok[b] = d_cur; lp.ham_n[b] = g * s; lp.ham_lambda[b] = lambda;
          }
          RUN(GVL_PROF_OTHER, 0, gvl_launch_logits_process(lp, st));
        }
        float sc[GVL_MAX_DECODE_BATCH];
        for (int b = 0; b < s; ++b) sc[b] = gs.score(g * s + b);
        fill_cand_args(ctx, ga.c, work, V, s, first ? 0 : V, sc, 0, d_vals + g * 2 * s, d_idx + g * 2 * s, d_proc + g * 2 * s);
      }
      RUN(GVL_PROF_OTHER, 0, gvl_launch_beam_group(ga, st));
    }
    HIPCHK(ctx, hipStreamSynchronize(st));               // the ONE synchronise of the step: candidates and chosen tokens sit in host-mapped memory
    const int rc = gs.step(h_vals, h_idx, h_proc, 2 * s, parents.data(), toks.data());
    if (rc < 0) return fail(ctx, rc == gvl_beam::BEAM_ERR_ARG ? GVL_ERR_HIP : (rc == gvl_beam::BEAM_ERR_FEW ? GVL_ERR_STATE : GVL_ERR_ARG), std::string("gvl_group_beam_search: ") + gvl_beam::status_text(rc));
    for (int j = 0; j < k; ++j) {
      ctx->group_beam_tokens.push_back(h_cur[j]);
      if (h_cur[j] != toks[j]) return fail(ctx, GVL_ERR_HIP, "gvl_group_beam_search: the device's choice of a group's tokens differs from the host bookkeeping's");
    }
    if (rc == gvl_beam::BEAM_FINISHED) break;
    for (int j = 0; j < k; ++j) if (gs.group_done(j / s)) parents[j] = -1;      // a group that is done now is never read again: its beams are not even stepped once more

    // the cache reorder of gvl_beam_search over the beams that live on; a parent without a child -- every beam of a group that is done now -- goes back to the pool at once
    std::vector<int> keep(beams.size(), -1), next(k, -1);
    for (int j = 0; j < k; ++j) {
      const int pj = parents[j];
      if (pj < 0) continue;
      if (pj >= (int)beams.size() || beams[pj] < 0) return fail(ctx, GVL_ERR_HIP, "gvl_group_beam_search: a beam continues a closed beam");
      if (keep[pj] >= 0) { if (const int crc = clone(beams[pj], &next[j])) return crc; }
      else keep[pj] = j;
    }
    for (size_t q = 0; q < beams.size(); ++q) if (keep[q] >= 0) next[keep[q]] = beams[q];
    for (size_t q = 0; q < beams.size(); ++q) if (keep[q] < 0 && beams[q] >= 0) own.drop(beams[q]);
    beams = next;
    ctx->group_beam_pool.push_back((int)own.ids.size()); ctx->group_beam_pool.push_back((int)ctx->free_pages.size());

    Seq* sqs[GVL_MAX_DECODE_BATCH]; int n_live = 0;
    for (int j = 0; j < k; ++j) {
      if (beams[j] < 0) continue;
      Seq* sq = &ctx->seqs[beams[j]];
      if (sq->pos >= sq->max_tokens) return fail(ctx, GVL_ERR_ARG, "gvl_group_beam_search: the context is full (cfg.max_seq) before max_new_tokens");
      RUN(GVL_PROF_OTHER, 0, gvl_launch_set_int(sq->d_tok, toks[j], st));
      sqs[n_live++] = sq;
    }
    int sizes[GVL_MAX_DECODE_BATCH];
    const int n_parts = decode_parts(ctx->decode_mfma, n_live, sizes);
    const bool one_part = n_parts == 1;
    for (int q = 0, o = 0; q < n_parts; ++q) {
      const int nb = sizes[q];
      if (const int drc = decode_step(ctx, sqs + o, nb, st)) return drc;
      if (!one_part) HIPCHK(ctx, hipMemcpyAsync(ctx->d_beam_rows + (size_t)o * V, ctx->d_logits, (size_t)nb * V * 4, hipMemcpyDeviceToDevice, st));
      o += nb;
    }
    rows = one_part ? ctx->d_logits : ctx->d_beam_rows; first = false;
  }

  std::vector<std::vector<int>> ids; std::vector<double> score; std::vector<std::vector<float>> ts;
  const int got = gs.finalize_n(num_return, &ids, &score, &ts);
  if (got < num_return) return fail(ctx, GVL_ERR_STATE, "gvl_group_beam_search: fewer hypotheses than num_return");
  for (int r = 0; r < num_return; ++r) {
    const int n = (int)ids[r].size();
    for (int i = 0; i < n; ++i) out_ids_host[(size_t)r * cap + i] = ids[r][i];
    n_out[r] = n;
    if (sequences_scores) sequences_scores[r] = score[r];
    if (transition_scores_host) for (int i = 0; i < n && i < (int)ts[r].size(); ++i) transition_scores_host[(size_t)r * cap + i] = ts[r][i];
  }
  return 0;
}

}  // extern "C"
