// gvl_search.hip -- what the searches inside the library share (SearchSession, gvl_model.h): gvl_beam_search_n / gvl_group_beam_search (gvl_beam.hip) and
// gvl_contrastive_search (gvl_contrastive.hip) all run on clones of the caller's prefilled sequence, keep the clones' histories themselves, process logits rows with the
// one processor launch, take their candidates through the beam candidate launches and advance by one teacher-forced decode step per token.  Host code only.  The session
// owns every sequence the search opened (they go back to the pool on every return path), the search's work buffers and the views into them, the history upload and the
// processor launch, the step, the cache reorder (planned in gvl_beam.h, CPU-tested) and the copy of the best hypotheses to the caller.
#include "gvl_model.h"
#include "gvl_beam.h"

using namespace gvlm;

namespace {

constexpr int kMaxCand = 2 * GVL_MAX_DECODE_BATCH;
// behind the survivors (device) and behind one step's candidates (host-mapped): the tokens the groups of a diverse beam search chose at this step
constexpr size_t kScratchFloats = (size_t)GVL_MAX_DECODE_BATCH * kMaxCand * 3, kCandFloats = (size_t)kMaxCand * 3;
constexpr size_t kHistInts = (size_t)GVL_MAX_DECODE_BATCH * GVL_LOGITS_HIST_CAP;

}  // namespace

// the small buffers every candidate launch needs: the per-row survivors between the two launches (device) and one step's result (host-mapped, as the generated ids are)
int SearchSession::ensure_scratch(gvl_ctx* ctx) {
  if (!ctx->d_beam_scratch) HIPCHK(ctx, hipMalloc((void**)&ctx->d_beam_scratch, (kScratchFloats + GVL_MAX_DECODE_BATCH) * 4));
  if (!ctx->h_beam_cand) {
    HIPCHK(ctx, hipHostMalloc((void**)&ctx->h_beam_cand, (kCandFloats + GVL_MAX_DECODE_BATCH) * 4, hipHostMallocMapped));
    memset(ctx->h_beam_cand, 0, (kCandFloats + GVL_MAX_DECODE_BATCH) * 4);
    HIPCHK(ctx, hipHostGetDevicePointer((void**)&ctx->d_beam_cand, ctx->h_beam_cand, 0));
  }
  return 0;
}
// ... and what a whole search needs: [16][vocab] work rows (sequences stepped in several parts are gathered here; the processors' in-place target on the first step) and
// the histories for the logits processors
int SearchSession::ensure_buffers(gvl_ctx* ctx) {
  if (const int rc = ensure_scratch(ctx)) return rc;
  if (!ctx->d_beam_rows) HIPCHK(ctx, hipMalloc((void**)&ctx->d_beam_rows, (size_t)GVL_MAX_DECODE_BATCH * ctx->cfg.vocab * 4));
  if (!ctx->d_beam_hist) HIPCHK(ctx, hipMalloc((void**)&ctx->d_beam_hist, (kHistInts + GVL_MAX_DECODE_BATCH) * 4));
  return 0;
}
void SearchSession::cand_args(gvl_ctx* ctx, BeamCandArgs& a, const float* rows, int n, int k, int row_stride, const float* scores, int norm, float* vals, int* idx, float* proc) {
  memset(&a, 0, sizeof(a));
  a.rows = rows; a.n = n; a.k = k; a.row_stride = row_stride; a.norm = norm;
  for (int b = 0; b < k; ++b) a.scores[b] = scores[b];
  float* s = (float*)ctx->d_beam_scratch;
  a.row_v = s; a.row_i = (int*)(s + GVL_MAX_DECODE_BATCH * kMaxCand); a.row_lp = s + 2 * GVL_MAX_DECODE_BATCH * kMaxCand;
  a.vals = vals; a.idx = idx; a.proc = proc;
}

SearchSession::~SearchSession() { for (int id : ids) ctx->close(id); }

int SearchSession::open(int seq_id, float penalty, int ngram, int min_new, int proc_eos_id, int rules_id, int max_new, bool ranks_hidden) {
  if (rules_id != -1 && (rules_id < 0 || ctx->check_rules(rules_id))) return seq_fail(ctx, fn, SEQ_NO_RULES);
  if (const int rc = admit(ctx, ranks_hidden ? gvl_admit::SEARCH_HIDDEN : gvl_admit::SEARCH, &seq_id, 1, nullptr, 0, fn)) return rc;
  pos0 = ctx->seqs[seq_id].pos;
  if (const int rc = ensure_buffers(ctx)) return rc;
  V = ctx->cfg.vocab;
  h_vals = (float*)ctx->h_beam_cand; h_idx = (int*)(h_vals + kMaxCand); h_proc = h_vals + 2 * kMaxCand; h_chosen = (int*)(h_vals + kCandFloats);
  d_vals = (float*)ctx->d_beam_cand; d_idx = (int*)(d_vals + kMaxCand); d_proc = d_vals + 2 * kMaxCand; d_chosen_mirror = (int*)(d_vals + kCandFloats);
  d_chosen = (int*)((float*)ctx->d_beam_scratch + kScratchFloats);
  d_hist = ctx->d_beam_hist; d_lens = ctx->d_beam_hist + kHistInts;

  proc = LogitsProc{penalty, ngram, min_new, proc_eos_id < 0 ? -1 : proc_eos_id};
  // the grammar the caller's sequence carries (gvl_seq_set_grammar) constrains the whole search; read here, before the root clone's options go off below.  The sequence
  // holds its reference for the whole call, so the blob outlives every launch
  const int grammar_id = ctx->seqs[seq_id].sel.grammar;
  grammar = grammar_id >= 0 ? (const GrammarDev*)ctx->grammars[grammar_id].d : nullptr;
  rules = rules_id >= 0 ? (const TokenRulesDev*)ctx->rule_sets[rules_id].d : nullptr;
  processed = proc.on() || rules || grammar;
  seq_cap = std::min(pos0 + max_new + 1, (int)ctx->cfg.max_seq);

  // The search runs on clones of the caller's sequence (it is never stepped: on return it is where it was).  Their selection options are off -- clones copy that -- so a
  // step's own token pick leaves the logits rows raw; the scores come from the search's own launches.
  if (const int rc = clone(seq_id, &root)) return rc;
  SeqSelect& sel = ctx->seqs[root].sel;
  sel.proc = LogitsProc(); ctx->set_rules(sel, -1); ctx->set_grammar(sel, -1); sel.top_n = -1;
  const Sampling greedy; ctx->set_sampling(sel, &greedy);
  return 0;
}

int SearchSession::clone(int src, int* dst) {
  const int rc = seq_clone(ctx, src, seq_cap, dst, st, false);   // the search keeps the histories itself (d_beam_hist)
  if (rc == 0) ids.push_back(*dst);
  return rc;
}
int SearchSession::clone_many(int src, int n, int* dst) {
  ProfScope clones(ctx, GVL_PROF_CS_CLONE, 0, st);   // all or nothing; the partial-page copies of all n are one launch
  if (const int rc = seq_clone_many(ctx, src, seq_cap, n, dst, st)) return rc;
  ids.insert(ids.end(), dst, dst + n);
  return 0;
}
void SearchSession::drop(int id) { ids.erase(std::find(ids.begin(), ids.end(), id)); ctx->close(id); }

int SearchSession::upload_histories(int n_rows, int len, const std::vector<int>* const* row_ids) {
  hs = len > 0 ? std::min(len, (int)GVL_LOGITS_HIST_CAP) : 1;
  h_hist.assign((size_t)n_rows * hs + GVL_MAX_DECODE_BATCH, 0);
  for (int r = 0; r < n_rows; ++r) {
    if (row_ids[r]) for (int i = 0; i < hs && i < len; ++i) h_hist[(size_t)r * hs + i] = (*row_ids[r])[i];
    h_hist[(size_t)n_rows * hs + r] = len;
  }
  HIPCHK(ctx, hipMemcpyAsync(d_hist, h_hist.data(), (size_t)n_rows * hs * 4, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_lens, h_hist.data() + (size_t)n_rows * hs, (size_t)n_rows * 4, hipMemcpyHostToDevice, st));
  return 0;
}

int SearchSession::process(float* work, int first_row, int n_rows, const int* ham_tok, int ham_n, float ham_lambda) {
  LogitsProcArgs lp; memset(&lp, 0, sizeof(lp));
  lp.logits = work; lp.n = V; lp.ld = V; lp.batch = n_rows; lp.cap = hs;
  for (int b = 0; b < n_rows; ++b) {
    lp.hist[b] = d_hist + (size_t)(first_row + b) * hs; lp.len_ptrs[b] = d_lens + first_row + b;
    lp.penalty[b] = proc.penalty; lp.ngram[b] = proc.ngram; lp.eos[b] = proc.eos; lp.min_new[b] = proc.eos >= 0 ? proc.min_new : 0; lp.rules[b] = rules; lp.grammar[b] = grammar;
    if (ham_tok) { lp.ham_tok[b] = ham_tok; lp.ham_n[b] = ham_n; lp.ham_lambda[b] = ham_lambda; }
  }
  RUN(GVL_PROF_OTHER, 0, gvl_launch_logits_process(lp, st));
  return 0;
}

int SearchSession::copy_first(const float* first_logits, float** work) {
  *work = ctx->d_beam_rows;
  HIPCHK(ctx, hipMemcpyAsync(*work, first_logits, (size_t)V * 4, hipMemcpyDeviceToDevice, st));
  return 0;
}

int SearchSession::advance(Seq* const* sqs, int n, const int* toks, const PartHook& after_part, float** rows) {
  for (int j = 0; j < n; ++j) {
    if (sqs[j]->pos >= sqs[j]->max_tokens) return fail(ctx, GVL_ERR_ARG, std::string(fn) + ": the context is full (cfg.max_seq) before max_new_tokens");
    if (toks) RUN(GVL_PROF_OTHER, 0, gvl_launch_set_int(sqs[j]->d_tok, toks[j], st));
  }
  // in the parts the decode path takes (any size up to 16 on the skinny-MFMA path: one part; 4 / 2 / 1 on the VALU fallback); a row does not depend on the part it was
  // computed in
  int sizes[GVL_MAX_DECODE_BATCH];
  const int n_parts = decode_parts(ctx->decode_mfma, n, sizes);
  const bool one_part = n_parts == 1;
  for (int p = 0, o = 0; p < n_parts; ++p) {
    const int nb = sizes[p];
    if (const int rc = decode_step(ctx, sqs + o, nb, st)) return rc;
    if (after_part) { if (const int rc = after_part(o, nb)) return rc; }
    if (!one_part) HIPCHK(ctx, hipMemcpyAsync(ctx->d_beam_rows + (size_t)o * V, ctx->d_logits, (size_t)nb * V * 4, hipMemcpyDeviceToDevice, st));
    o += nb;
  }
  *rows = one_part ? ctx->d_logits : ctx->d_beam_rows;
  return 0;
}

int SearchSession::reorder(std::vector<int>& beams, const int* parents, int k) {
  gvl_beam::ReorderPlan plan;
  if (!gvl_beam::reorder(beams, parents, k, &plan)) return fail(ctx, GVL_ERR_HIP, std::string(fn) + ": a beam continues a closed beam");
  std::vector<int> next(k, -1);
  for (int j : plan.clones) if (const int rc = clone(beams[plan.src[j]], &next[j])) return rc;
  for (int j = 0; j < k; ++j) if (plan.src[j] >= 0 && next[j] < 0) next[j] = beams[plan.src[j]];
  for (int q : plan.closed) drop(beams[q]);
  beams = next;
  return 0;
}

int SearchSession::write_hypotheses(int got, int num_return, const std::vector<std::vector<int>>& hyp_ids, const std::vector<double>& score,
                                    const std::vector<std::vector<float>>& ts, int32_t* out_ids_host, int cap, int* n_out, double* sequences_scores,
                                    float* transition_scores_host) {
  if (got < num_return) return fail(ctx, GVL_ERR_STATE, std::string(fn) + ": fewer hypotheses than num_return");
  for (int r = 0; r < num_return; ++r) {
    const int n = (int)hyp_ids[r].size();                 // <= max_new <= cap
    for (int i = 0; i < n; ++i) out_ids_host[(size_t)r * cap + i] = hyp_ids[r][i];
    n_out[r] = n;
    if (sequences_scores) sequences_scores[r] = score[r];
    if (transition_scores_host) for (int i = 0; i < n && i < (int)ts[r].size(); ++i) transition_scores_host[(size_t)r * cap + i] = ts[r][i];
  }
  return 0;
}
