// gvl_select.hip -- the token-selection part of the C ABI of include/gvl.h: sampling parameters, HF logits processors, token rule sets, log-probabilities of the selected tokens -- the settings a sequence
// carries (SeqSelect, gvl_seq_table.h; applied per step by pick_tokens, gvl_llm.hip) and the operator-level entries of their kernels (gvl_elem.hip, gvl_logits.hip).  Host code only.
#include "gvl_model.h"

using namespace gvlm;
extern "C" {

int gvl_set_sampling(gvl_ctx* ctx, int do_sample, float temperature, int top_k, float top_p, uint64_t seed) {
  if (!ctx) return GVL_ERR_ARG;
  if (!do_sample) { ctx->sample.on = false; return 0; }
  if (!(temperature > 0.f) || top_k < 0 || !(top_p >= 0.f) || top_p > 1.f)
    return fail(ctx, GVL_ERR_ARG, "gvl_set_sampling: temperature must be > 0, top_k >= 0, 0 <= top_p <= 1");
  ctx->sample.on = true; ctx->sample.inv_temp = 1.0f / temperature; ctx->sample.top_k = top_k; ctx->sample.top_p = top_p;
  ctx->sample.min_p = ctx->sample.typical_p = ctx->sample.eps = ctx->sample.eta = 0.f;
  // stream numbering restarts with the call (same seed + same prefill order = same draws) -- unless sequences are LIVE: a scheduler that
  // changes the sampling parameters mid-flight must not hand the stream ids of running sequences to newcomers
  if (!ctx->any_live() || seed != ctx->sample.seed) ctx->sample.next_stream = 0;
  ctx->sample.seed = seed;
  return 0;
}
// a gvl_sampling as the entry point `what` takes it -> `out`; every bad value is an error with a message, never a clamp (NaN fails every range test)
static int check_sampling(gvl_ctx* ctx, const gvl_sampling& g, const char* what, Sampling* out) {
  Sampling q;
  if (!g.do_sample) { *out = q; return 0; }
  const std::string w = std::string(what) + ": ";
  if (!(g.temperature > 0.f)) return fail(ctx, GVL_ERR_ARG, w + "temperature must be > 0");
  if (g.top_k < 0) return fail(ctx, GVL_ERR_ARG, w + "top_k must be >= 0");
  if (!(g.top_p >= 0.f && g.top_p <= 1.f)) return fail(ctx, GVL_ERR_ARG, w + "top_p must be in [0, 1]");
  if (!(g.min_p >= 0.f && g.min_p <= 1.f)) return fail(ctx, GVL_ERR_ARG, w + "min_p must be in [0, 1]");
  if (!(g.typical_p >= 0.f && g.typical_p < 1.f)) return fail(ctx, GVL_ERR_ARG, w + "typical_p must be in [0, 1) (0 = off)");
  if (!(g.epsilon_cutoff >= 0.f && g.epsilon_cutoff < 1.f)) return fail(ctx, GVL_ERR_ARG, w + "epsilon_cutoff must be in [0, 1) (0 = off)");
  if (!(g.eta_cutoff >= 0.f && g.eta_cutoff < 1.f)) return fail(ctx, GVL_ERR_ARG, w + "eta_cutoff must be in [0, 1) (0 = off)");
  q.on = true; q.inv_temp = 1.0f / g.temperature; q.top_k = g.top_k; q.top_p = g.top_p; q.min_p = g.min_p; q.typical_p = g.typical_p;
  q.eps = g.epsilon_cutoff; q.eta = g.eta_cutoff; q.seed = g.seed; q.stream = g.stream;
  *out = q; return 0;
}
int gvl_set_sampling_ex(gvl_ctx* ctx, const gvl_sampling* g) {
  if (!ctx) return GVL_ERR_ARG;
  if (!g) return fail(ctx, GVL_ERR_ARG, "gvl_set_sampling_ex: bad arguments");
  Sampling q;
  if (const int rc = check_sampling(ctx, *g, "gvl_set_sampling_ex", &q)) return rc;
  if (const int rc = gvl_set_sampling(ctx, g->do_sample, g->temperature, g->top_k, g->top_p, g->seed)) return rc;   // the stream numbering rule lives there
  if (q.on) { ctx->sample.min_p = q.min_p; ctx->sample.typical_p = q.typical_p; ctx->sample.eps = q.eps; ctx->sample.eta = q.eta; }
  return 0;
}
int gvl_seq_set_sampling(gvl_ctx* ctx, int seq_id, const gvl_sampling* g) {
  if (!ctx) return GVL_ERR_ARG;
  Seq* sq = ctx->lookup(seq_id);
  if (!sq) return seq_fail(ctx, "gvl_seq_set_sampling", SEQ_BAD);
  if (!g) { ctx->set_sampling(sq->sel, nullptr); return 0; }
  Sampling q;
  if (const int rc = check_sampling(ctx, *g, "gvl_seq_set_sampling", &q)) return rc;
  ctx->set_sampling(sq->sel, &q);
  return 0;
}

int gvl_op_sample(gvl_ctx* ctx, const float* logits, int n, int batch, float temperature, int top_k, float top_p, uint64_t seed,
                  const uint32_t* streams, const int32_t* steps_dev, int32_t* tokens_dev, void* stream) {
  if (!ctx || !logits || !streams || !steps_dev || !tokens_dev || n < 1 || batch < 1 || batch > GVL_MAX_DECODE_BATCH || !(temperature > 0.f) || top_k < 0 || !(top_p >= 0.f) || top_p > 1.f)
    return fail(ctx, GVL_ERR_ARG, "gvl_op_sample: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  ArgmaxArgs am; memset(&am, 0, sizeof(am)); am.logits = logits; am.n = n; am.batch = batch;
  am.inv_temp = 1.0f / temperature; am.top_k = top_k; am.top_p = top_p; am.seed_lo = (unsigned)seed; am.seed_hi = (unsigned)(seed >> 32);
  am.step_override = steps_dev;
  for (int b = 0; b < batch; ++b) { am.tok_ptrs[b] = tokens_dev + b; am.stream[b] = streams[b]; }
  RUN(GVL_PROF_OTHER, 0, gvl_launch_sample(am, st));
  return 0;
}

// ---- HF logits processors (gvl_logits.hip): repetition penalty -> no-repeat n-gram -> min length, on the generated ids of each sequence
static int check_processors(gvl_ctx* ctx, float penalty, int ngram, int min_new, const char* what) {
  if (!(penalty > 0.f) || ngram < 0 || min_new < 0) return fail(ctx, GVL_ERR_ARG, std::string(what) + ": penalty must be > 0, ngram >= 0, min_new >= 0");
  return 0;
}
int gvl_set_logits_processors(gvl_ctx* ctx, float penalty, int ngram, int min_new, int eos_id) {
  if (!ctx) return GVL_ERR_ARG;
  if (const int rc = check_processors(ctx, penalty, ngram, min_new, "gvl_set_logits_processors")) return rc;
  ctx->sel_default.proc = LogitsProc{penalty, ngram, min_new, eos_id < 0 ? -1 : eos_id};
  return 0;
}
int gvl_seq_set_processors(gvl_ctx* ctx, int seq_id, float penalty, int ngram, int min_new, int eos_id) {
  if (!ctx) return GVL_ERR_ARG;
  Seq* sq = ctx->lookup(seq_id);
  if (!sq) return seq_fail(ctx, "gvl_seq_set_processors", SEQ_BAD);
  if (const int rc = check_processors(ctx, penalty, ngram, min_new, "gvl_seq_set_processors")) return rc;
  sq->sel.proc = LogitsProc{penalty, ngram, min_new, eos_id < 0 ? -1 : eos_id};
  return 0;
}
// the processors, with rules_ids (entry points gvl_op_logits_process_rules / _ex) the rule sets and with grammar_ids (gvl_op_logits_process_ex) the grammars, on `batch` rows of logits
static int op_logits_process(gvl_ctx* ctx, const char* what, float* logits, int n, int batch, const int32_t* hist_dev, int hist_stride, const int32_t* lens_dev,
                             const float* penalty, const int* ngram, const int* min_new, const int* eos_ids, const int* rules_ids, void* stream, const int* grammar_ids = nullptr,
                             const int32_t* ham_dev = nullptr, int n_ham = 0, float ham_lambda = 0.f) {
  if (!ctx || !logits || !lens_dev || !penalty || !ngram || !min_new || !eos_ids || n < 1 || batch < 1 || batch > GVL_MAX_DECODE_BATCH ||
      hist_stride < 0 || (hist_stride > 0 && !hist_dev))
    return fail(ctx, GVL_ERR_ARG, std::string(what) + ": bad arguments");
  if (n_ham < 0 || n_ham > GVL_MAX_DECODE_BATCH || (n_ham > 0 && (!ham_dev || !(ham_lambda == ham_lambda)))) return fail(ctx, GVL_ERR_ARG, std::string(what) + ": 0 .. 16 Hamming tokens on the device and a penalty that is a number");
  hipStream_t st = (hipStream_t)stream;
  LogitsProcArgs lp; memset(&lp, 0, sizeof(lp));
  lp.logits = logits; lp.n = n; lp.ld = n; lp.batch = batch; lp.cap = hist_stride < GVL_LOGITS_HIST_CAP ? hist_stride : GVL_LOGITS_HIST_CAP;
  for (int b = 0; b < batch; ++b) {
    if (const int rc = check_processors(ctx, penalty[b], ngram[b], min_new[b], what)) return rc;
    if (const int rc = rules_ids ? ctx->check_rules(rules_ids[b]) : 0) return seq_fail(ctx, what, rc);
    lp.hist[b] = hist_dev ? hist_dev + (size_t)b * hist_stride : nullptr; lp.len_ptrs[b] = lens_dev + b;
    lp.penalty[b] = penalty[b]; lp.ngram[b] = ngram[b]; lp.eos[b] = eos_ids[b] < 0 ? -1 : eos_ids[b]; lp.min_new[b] = lp.eos[b] >= 0 ? min_new[b] : 0;
    lp.rules[b] = rules_ids && rules_ids[b] >= 0 ? (const TokenRulesDev*)ctx->rule_sets[rules_ids[b]].d : nullptr;
    lp.ham_tok[b] = ham_dev; lp.ham_n[b] = n_ham; lp.ham_lambda[b] = ham_lambda;
    if (grammar_ids && grammar_ids[b] != -1) {
      if (const int rc = ctx->check_grammar(grammar_ids[b])) return seq_fail(ctx, what, rc);
      const GrammarSet& g = ctx->grammars[grammar_ids[b]];
      if (g.vocab != n) return fail(ctx, GVL_ERR_ARG, std::string(what) + ": the grammar classifies " + std::to_string(g.vocab) + " ids, the rows hold " + std::to_string(n));
      lp.grammar[b] = (const GrammarDev*)g.d;
    }
  }
  RUN(GVL_PROF_OTHER, 0, gvl_launch_logits_process(lp, st));
  return 0;
}
int gvl_op_logits_process(gvl_ctx* ctx, float* logits, int n, int batch, const int32_t* hist_dev, int hist_stride, const int32_t* lens_dev,
                          const float* penalty, const int* ngram, const int* min_new, const int* eos_ids, void* stream) {
  return op_logits_process(ctx, "gvl_op_logits_process", logits, n, batch, hist_dev, hist_stride, lens_dev, penalty, ngram, min_new, eos_ids, nullptr, stream);
}

// ---- token rules (TokenRulesDev, gvl_logits.hip): sequence_bias / bad_words_ids / forced eos / suppress lists as immutable device objects
static int check_ids(gvl_ctx* ctx, const int32_t* ids, int n, const char* what) {
  if (n < 0 || (n > 0 && !ids)) return fail(ctx, GVL_ERR_ARG, std::string("gvl_rules_create: ") + what + ": bad list");
  if (n > GVL_RULES_MAX_IDS) return fail(ctx, GVL_ERR_ARG, std::string("gvl_rules_create: ") + what + " holds " + std::to_string(n) + " ids, the limit is " + std::to_string(GVL_RULES_MAX_IDS));
  for (int i = 0; i < n; ++i) if (ids[i] < 0) return fail(ctx, GVL_ERR_ARG, std::string("gvl_rules_create: ") + what + ": negative token id");
  return 0;
}
static int check_table(gvl_ctx* ctx, const gvl_bias_table& t, const char* what, int* n_multi) {
  const std::string w = std::string("gvl_rules_create: ") + what;
  if (t.n_targets < 0 || t.n_entries < 0 || t.n_prefix < 0 || (t.n_targets > 0 && !t.targets) || (t.n_entries > 0 && (!t.entry_bias || !t.entry_prefix)) || (t.n_prefix > 0 && !t.prefix))
    return fail(ctx, GVL_ERR_ARG, w + ": bad table");
  int multi = 0;
  for (int e = 0; e < t.n_entries; ++e) {
    const int po = t.entry_prefix[2 * e], pl = t.entry_prefix[2 * e + 1];
    if (pl < 0 || po < 0) return fail(ctx, GVL_ERR_ARG, w + ": bad prefix range");
    if (pl + 1 > GVL_RULES_MAX_SEQ_LEN) return fail(ctx, GVL_ERR_ARG, w + ": an entry holds " + std::to_string(pl + 1) + " ids, the limit is " + std::to_string(GVL_RULES_MAX_SEQ_LEN));
    if ((int64_t)po + pl > t.n_prefix) return fail(ctx, GVL_ERR_ARG, w + ": bad prefix range");
    multi += pl > 0;
  }
  if (multi > GVL_RULES_MAX_SEQS) return fail(ctx, GVL_ERR_ARG, w + " holds " + std::to_string(multi) + " multi-token entries, the limit is " + std::to_string(GVL_RULES_MAX_SEQS));
  if (t.n_entries - multi > GVL_RULES_MAX_IDS) return fail(ctx, GVL_ERR_ARG, w + " holds " + std::to_string(t.n_entries - multi) + " single-token entries, the limit is " + std::to_string(GVL_RULES_MAX_IDS));
  if (t.n_targets > t.n_entries) return fail(ctx, GVL_ERR_ARG, w + ": more targets than entries");
  std::vector<int> seen; seen.reserve(t.n_targets);
  for (int g = 0; g < t.n_targets; ++g) {
    const int tk = t.targets[3 * g], e0 = t.targets[3 * g + 1], ne = t.targets[3 * g + 2];
    if (tk < 0 || e0 < 0 || ne < 1 || (int64_t)e0 + ne > t.n_entries) return fail(ctx, GVL_ERR_ARG, w + ": bad target group");
    seen.push_back(tk);
  }
  for (int i = 0; i < t.n_prefix; ++i) if (t.prefix[i] < 0) return fail(ctx, GVL_ERR_ARG, w + ": negative token id");
  std::sort(seen.begin(), seen.end());
  if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return fail(ctx, GVL_ERR_ARG, w + ": a target token appears in two groups (one thread owns one target)");
  *n_multi += multi;
  return 0;
}
int gvl_rules_create(gvl_ctx* ctx, const gvl_rules_desc* d, int* rules_id) {
  if (!ctx) return GVL_ERR_ARG;
  if (!d || !rules_id) return fail(ctx, GVL_ERR_ARG, "gvl_rules_create: bad arguments");
  if (const int rc = check_ids(ctx, d->suppress, d->n_suppress, "suppress")) return rc;
  if (const int rc = check_ids(ctx, d->begin_suppress, d->n_begin_suppress, "begin_suppress")) return rc;
  if (const int rc = check_ids(ctx, d->force_ids, d->n_force, "force_ids")) return rc;
  if ((d->n_begin_suppress > 0 && d->begin_index < 0) || (d->n_force > 0 && d->force_at < 0)) return fail(ctx, GVL_ERR_ARG, "gvl_rules_create: begin_index / force_at must be >= 0");
  int n_multi = 0;
  if (const int rc = check_table(ctx, d->bias[0], "bias[0] (sequence_bias)", &n_multi)) return rc;
  if (const int rc = check_table(ctx, d->bias[1], "bias[1] (bad_words_ids)", &n_multi)) return rc;
  const int id = ctx->add_rules(nullptr);              // the slot first: its blob follows below, a failure there gives the slot back
  if (id < 0) return seq_fail(ctx, "gvl_rules_create", id);
  // the blob: header, then every array, as 32-bit words
  static_assert(sizeof(TokenRulesDev) % 4 == 0, "header is whole words");
  std::vector<int32_t> w(sizeof(TokenRulesDev) / 4, 0);
  TokenRulesDev h; memset(&h, 0, sizeof(h));
  auto put = [&w](const int32_t* p, size_t n) { const int off = (int)w.size(); if (n) w.insert(w.end(), p, p + n); return off; };
  h.n_suppress = d->n_suppress; h.off_suppress = put(d->suppress, d->n_suppress);
  h.n_begin = d->n_begin_suppress; h.off_begin = put(d->begin_suppress, d->n_begin_suppress); h.begin_at = d->begin_index;
  h.n_force = d->n_force; h.off_force = put(d->force_ids, d->n_force); h.force_at = d->force_at;
  h.n_multi = n_multi;
  for (int st = 0; st < 2; ++st) {
    const gvl_bias_table& t = d->bias[st];
    h.n_tgt[st] = t.n_targets; h.off_tgt[st] = put(t.targets, (size_t)t.n_targets * 3);
    h.off_ent[st] = (int)w.size();
    for (int e = 0; e < t.n_entries; ++e) {
      int32_t bits; memcpy(&bits, &t.entry_bias[e], 4);
      w.push_back(bits); w.push_back(t.entry_prefix[2 * e]); w.push_back(t.entry_prefix[2 * e + 1]);
    }
    h.off_pre[st] = put(t.prefix, t.n_prefix);
  }
  memcpy(w.data(), &h, sizeof(h));
  RuleSet& r = ctx->rule_sets[id];
  hipError_t e = hipMalloc((void**)&r.d, w.size() * 4);
  if (e != hipSuccess) { r = RuleSet(); return gvl_hipfail(ctx, e, "hipMalloc((void**)&r.d, w.size() * 4)"); }
  e = hipMemcpy(r.d, w.data(), w.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) { hipFree(r.d); r = RuleSet(); return gvl_hipfail(ctx, e, "gvl_rules_create: hipMemcpy"); }
  *rules_id = id;
  return 0;
}
int gvl_rules_destroy(gvl_ctx* ctx, int rules_id) {
  if (!ctx) return GVL_ERR_ARG;
  if (const int rc = ctx->destroy_rules(rules_id, nullptr)) return seq_fail(ctx, "gvl_rules_destroy", rc);   // asks only
  HIPCHK(ctx, hipDeviceSynchronize());                 // every launch that read the set has finished before its memory goes
  void* blob = nullptr; ctx->destroy_rules(rules_id, &blob); hipFree(blob);
  return 0;
}
int gvl_set_token_rules(gvl_ctx* ctx, int rules_id) {
  if (!ctx) return GVL_ERR_ARG;
  return seq_fail(ctx, "gvl_set_token_rules", ctx->set_rules(ctx->sel_default, rules_id));
}
int gvl_seq_set_token_rules(gvl_ctx* ctx, int seq_id, int rules_id) {
  if (!ctx) return GVL_ERR_ARG;
  Seq* sq = ctx->lookup(seq_id);
  if (!sq) return seq_fail(ctx, "gvl_seq_set_token_rules", SEQ_BAD);
  return seq_fail(ctx, "gvl_seq_set_token_rules", ctx->set_rules(sq->sel, rules_id));
}
int gvl_op_logits_process_rules(gvl_ctx* ctx, float* logits, int n, int batch, const int32_t* hist_dev, int hist_stride, const int32_t* lens_dev,
                                const float* penalty, const int* ngram, const int* min_new, const int* eos_ids, const int* rules_ids, void* stream) {
  if (!rules_ids) return fail(ctx, GVL_ERR_ARG, "gvl_op_logits_process_rules: bad arguments");
  return op_logits_process(ctx, "gvl_op_logits_process_rules", logits, n, batch, hist_dev, hist_stride, lens_dev, penalty, ngram, min_new, eos_ids, rules_ids, stream);
}
int gvl_op_logits_process_hamming(gvl_ctx* ctx, float* logits, int n, int batch, const int32_t* hist_dev, int hist_stride, const int32_t* lens_dev,
                                  const float* penalty, const int* ngram, const int* min_new, const int* eos_ids, const int* rules_ids, const int* grammar_ids,
                                  const int32_t* ham_tokens_dev, int n_ham, float diversity_penalty, void* stream) {
  return op_logits_process(ctx, "gvl_op_logits_process_hamming", logits, n, batch, hist_dev, hist_stride, lens_dev, penalty, ngram, min_new, eos_ids, rules_ids, stream, grammar_ids,
                           ham_tokens_dev, n_ham, diversity_penalty);
}
int gvl_op_logits_process_ex(gvl_ctx* ctx, float* logits, int n, int batch, const int32_t* hist_dev, int hist_stride, const int32_t* lens_dev,
                             const float* penalty, const int* ngram, const int* min_new, const int* eos_ids, const int* rules_ids, const int* grammar_ids, void* stream) {
  return op_logits_process(ctx, "gvl_op_logits_process_ex", logits, n, batch, hist_dev, hist_stride, lens_dev, penalty, ngram, min_new, eos_ids, rules_ids, stream, grammar_ids);
}

// ---- decoding grammars (gvl_grammar.h; the GRAMMAR stage of gvl_logits.hip): a DFA over token classes with one register, an immutable device object
int gvl_grammar_create(gvl_ctx* ctx, const gvl_grammar_desc* d, int* grammar_id) {
  if (!ctx) return GVL_ERR_ARG;
  if (!d || !grammar_id) return fail(ctx, GVL_ERR_ARG, "gvl_grammar_create: bad arguments");
  const gvl_grammar::Desc desc{d->n_states, d->n_classes, d->start, d->vocab, d->token_class, d->class_base, d->trans};
  const std::string bad = gvl_grammar::check(desc);
  if (!bad.empty()) return fail(ctx, GVL_ERR_ARG, "gvl_grammar_create: " + bad);
  const int id = ctx->add_grammar(nullptr, d->vocab);   // the slot first: its blob follows below, a failure there gives the slot back
  if (id < 0) return seq_fail(ctx, "gvl_grammar_create", id);
  const std::vector<uint32_t> w = gvl_grammar::pack(desc);
  GrammarSet& g = ctx->grammars[id];
  hipError_t e = hipMalloc((void**)&g.d, w.size() * 4);
  if (e != hipSuccess) { g = GrammarSet(); return gvl_hipfail(ctx, e, "gvl_grammar_create: hipMalloc"); }
  e = hipMemcpy(g.d, w.data(), w.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) { hipFree(g.d); g = GrammarSet(); return gvl_hipfail(ctx, e, "gvl_grammar_create: hipMemcpy"); }
  *grammar_id = id;
  return 0;
}
int gvl_grammar_destroy(gvl_ctx* ctx, int grammar_id) {
  if (!ctx) return GVL_ERR_ARG;
  if (const int rc = ctx->destroy_grammar(grammar_id, nullptr)) return seq_fail(ctx, "gvl_grammar_destroy", rc);   // asks only
  HIPCHK(ctx, hipDeviceSynchronize());                 // every launch that read the grammar has finished before its memory goes
  void* blob = nullptr; ctx->destroy_grammar(grammar_id, &blob); hipFree(blob);
  return 0;
}
// a grammar bound to sequences classifies exactly the model's vocabulary: the rows it masks are cfg.vocab wide
static int check_seq_grammar(gvl_ctx* ctx, const char* what, int grammar_id) {
  if (const int rc = ctx->check_grammar(grammar_id)) return seq_fail(ctx, what, rc);
  if (grammar_id >= 0 && ctx->grammars[grammar_id].vocab != ctx->cfg.vocab)
    return fail(ctx, GVL_ERR_ARG, std::string(what) + ": the grammar classifies " + std::to_string(ctx->grammars[grammar_id].vocab) + " ids, the model's vocabulary holds " + std::to_string(ctx->cfg.vocab));
  return 0;
}
int gvl_set_grammar(gvl_ctx* ctx, int grammar_id) {
  if (!ctx) return GVL_ERR_ARG;
  if (const int rc = check_seq_grammar(ctx, "gvl_set_grammar", grammar_id)) return rc;
  return seq_fail(ctx, "gvl_set_grammar", ctx->set_grammar(ctx->sel_default, grammar_id));
}
int gvl_seq_set_grammar(gvl_ctx* ctx, int seq_id, int grammar_id) {
  if (!ctx) return GVL_ERR_ARG;
  Seq* sq = ctx->lookup(seq_id);
  if (!sq) return seq_fail(ctx, "gvl_seq_set_grammar", SEQ_BAD);
  if (const int rc = check_seq_grammar(ctx, "gvl_seq_set_grammar", grammar_id)) return rc;
  return seq_fail(ctx, "gvl_seq_set_grammar", ctx->set_grammar(sq->sel, grammar_id));
}

// ---- log-probabilities of the selected tokens (ArgmaxArgs.top_n / lp_lists / top_ids / top_lp; gvl_elem.hip)
// the slot lists a setting needs, allocated on first use (never during a decode call: the setters run between calls); live sequences are rebound
static int ensure_logprob_lists(gvl_ctx* ctx, int top_n, const char* what) {
  if (top_n < -1 || top_n > GVL_MAX_TOP_LOGPROBS) return fail(ctx, GVL_ERR_ARG, std::string(what) + ": top_n must be -1 (off), 0 (selected token) or 1 .. 8");
  if (top_n < 0) return 0;
  if (!ctx->has_llm) return fail(ctx, GVL_ERR_STATE, std::string(what) + ": no language model configured");
  const size_t n = (size_t)gvl_ctx::kMaxSeqs * ctx->outlist_cap;
  bool grew = false;
  if (!ctx->d_seq_lp) { HIPCHK(ctx, hipMalloc((void**)&ctx->d_seq_lp, n * 4)); grew = true; }
  if (top_n > 0 && !ctx->d_seq_top_ids) {
    HIPCHK(ctx, hipMalloc((void**)&ctx->d_seq_top_ids, n * GVL_MAX_TOP_LOGPROBS * 4));
    HIPCHK(ctx, hipMalloc((void**)&ctx->d_seq_top_lp, n * GVL_MAX_TOP_LOGPROBS * 4));
    grew = true;
  }
  if (grew) for (size_t i = 0; i < ctx->seqs.size(); ++i) if (ctx->seqs[i].used) bind_logprobs(ctx, ctx->seqs[i], (int)i);
  return 0;
}
int gvl_set_logprobs(gvl_ctx* ctx, int top_n) {
  if (!ctx) return GVL_ERR_ARG;
  if (const int rc = ensure_logprob_lists(ctx, top_n, "gvl_set_logprobs")) return rc;
  ctx->sel_default.top_n = top_n;
  return 0;
}
int gvl_seq_set_logprobs(gvl_ctx* ctx, int seq_id, int top_n) {
  if (!ctx) return GVL_ERR_ARG;
  Seq* sq = ctx->lookup(seq_id);
  if (!sq) return seq_fail(ctx, "gvl_seq_set_logprobs", SEQ_BAD);
  if (const int rc = ensure_logprob_lists(ctx, top_n, "gvl_seq_set_logprobs")) return rc;
  sq->sel.top_n = top_n;
  return 0;
}
int gvl_seq_read_logprobs(gvl_ctx* ctx, int seq_id, int first, int cap, float* lp, int32_t* top_ids, float* top_lp, int* n_gen, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_seq_read_logprobs");
  if (!ctx->lookup(seq_id) || !n_gen || first < 0 || cap < 0) return fail(ctx, GVL_ERR_ARG, "gvl_seq_read_logprobs: bad arguments");
  const Seq& sq = ctx->seqs[seq_id];
  if (lp && (sq.sel.top_n < 0 || !sq.d_lp)) return fail(ctx, GVL_ERR_STATE, "gvl_seq_read_logprobs: the sequence has log-probabilities off");
  if ((top_ids || top_lp) && (sq.sel.top_n < 1 || !sq.d_top_ids)) return fail(ctx, GVL_ERR_STATE, "gvl_seq_read_logprobs: the sequence keeps no top-N lists");
  *n_gen = sq.n_gen;
  int n = sq.n_gen - first; if (n > cap) n = cap;
  if (n > 0) {
    hipStream_t st = (hipStream_t)stream;
    const size_t K = GVL_MAX_TOP_LOGPROBS;
    if (lp) HIPCHK(ctx, hipMemcpyAsync(lp, sq.d_lp + first, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (top_ids) HIPCHK(ctx, hipMemcpyAsync(top_ids, sq.d_top_ids + (size_t)first * K, (size_t)n * K * 4, hipMemcpyDeviceToHost, st));
    if (top_lp) HIPCHK(ctx, hipMemcpyAsync(top_lp, sq.d_top_lp + (size_t)first * K, (size_t)n * K * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
  }
  return 0;
}
int gvl_op_select_logprobs(gvl_ctx* ctx, const float* logits, int n, int batch, int do_sample, float temperature, int top_k, float top_p, uint64_t seed,
                           const uint32_t* streams, const int32_t* steps_dev, const int* top_n, int32_t* tokens_dev, float* lp_dev, int32_t* top_ids_dev,
                           float* top_lp_dev, void* stream) {
  if (!ctx || !logits || !top_n || !tokens_dev || !lp_dev || n < 1 || batch < 1 || batch > GVL_MAX_DECODE_BATCH)
    return fail(ctx, GVL_ERR_ARG, "gvl_op_select_logprobs: bad arguments");
  if (do_sample && (!streams || !steps_dev || !(temperature > 0.f) || top_k < 0 || !(top_p >= 0.f) || top_p > 1.f))
    return fail(ctx, GVL_ERR_ARG, "gvl_op_select_logprobs: bad sampling arguments");
  hipStream_t st = (hipStream_t)stream;
  ArgmaxArgs am; memset(&am, 0, sizeof(am)); am.logits = logits; am.n = n; am.batch = batch;
  for (int b = 0; b < batch; ++b) {
    if (top_n[b] < -1 || top_n[b] > GVL_MAX_TOP_LOGPROBS || (top_n[b] > 0 && (!top_ids_dev || !top_lp_dev)))
      return fail(ctx, GVL_ERR_ARG, "gvl_op_select_logprobs: top_n must be -1 .. 8 (top lists needed for > 0)");
    am.tok_ptrs[b] = tokens_dev + b;
    am.top_n[b] = top_n[b]; am.lp_lists[b] = lp_dev + b;
    if (top_n[b] > 0) { am.top_ids[b] = top_ids_dev + (size_t)b * GVL_MAX_TOP_LOGPROBS; am.top_lp[b] = top_lp_dev + (size_t)b * GVL_MAX_TOP_LOGPROBS; }
  }
  if (!do_sample) { RUN(GVL_PROF_OTHER, 0, gvl_launch_argmax(am, st)); return 0; }
  am.inv_temp = 1.0f / temperature; am.top_k = top_k; am.top_p = top_p; am.seed_lo = (unsigned)seed; am.seed_hi = (unsigned)(seed >> 32);
  am.step_override = steps_dev;
  for (int b = 0; b < batch; ++b) am.stream[b] = streams[b];
  RUN(GVL_PROF_OTHER, 0, gvl_launch_sample(am, st));
  return 0;
}

// per-row selection on raw rows (select_rows_kernel): row b is greedy or sampled with rows[b]; outputs as gvl_op_select_logprobs, plus the kept mask
int gvl_op_select_rows(gvl_ctx* ctx, const float* logits, int n, int batch, const gvl_sampling* rows, const int32_t* steps_dev, const int* top_n,
                       int32_t* tokens_dev, float* lp_dev, int32_t* top_ids_dev, float* top_lp_dev, uint8_t* kept_dev, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!logits || !rows || !top_n || !tokens_dev || !lp_dev || n < 1 || batch < 1 || batch > GVL_MAX_DECODE_BATCH)
    return fail(ctx, GVL_ERR_ARG, "gvl_op_select_rows: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  SelRowsArgs sa; memset(&sa, 0, sizeof(sa));
  ArgmaxArgs& am = sa.am; am.logits = logits; am.n = n; am.batch = batch; am.step_override = steps_dev; sa.kept = kept_dev;
  for (int b = 0; b < batch; ++b) {
    if (top_n[b] < -1 || top_n[b] > GVL_MAX_TOP_LOGPROBS || (top_n[b] > 0 && (!top_ids_dev || !top_lp_dev)))
      return fail(ctx, GVL_ERR_ARG, "gvl_op_select_rows: top_n must be -1 .. 8 (top lists needed for > 0)");
    Sampling q;
    if (const int rc = check_sampling(ctx, rows[b], "gvl_op_select_rows", &q)) return rc;
    if (q.on && !steps_dev) return fail(ctx, GVL_ERR_ARG, "gvl_op_select_rows: a sampled row needs steps_dev");
    SelRow& r = sa.row[b];
    r.on = q.on; r.inv_temp = q.inv_temp; r.top_k = q.top_k; r.top_p = q.top_p; r.min_p = q.min_p; r.typical_p = q.typical_p; r.eps = q.eps; r.eta = q.eta;
    r.seed_lo = (unsigned)q.seed; r.seed_hi = (unsigned)(q.seed >> 32); r.stream = q.stream;
    am.tok_ptrs[b] = tokens_dev + b; am.top_n[b] = top_n[b]; am.lp_lists[b] = lp_dev + b;
    if (top_n[b] > 0) { am.top_ids[b] = top_ids_dev + (size_t)b * GVL_MAX_TOP_LOGPROBS; am.top_lp[b] = top_lp_dev + (size_t)b * GVL_MAX_TOP_LOGPROBS; }
  }
  RUN(GVL_PROF_OTHER, 0, gvl_launch_select_rows(sa, st));
  return 0;
}

// ---- classifier-free guidance against a negative sequence (guidance_rows_kernel / follow_commit_kernel, gvl_pick.hip; the per-step side is decode_step's, gvl_llm.hip)
// Everything is checked before the first launch: a refusal leaves both sequences as their prefills left them.
int gvl_seq_set_guidance(gvl_ctx* ctx, int seq_id, int neg_seq_id, float scale, float* cond_logits, float* neg_logits, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_seq_set_guidance");
  Seq* lead = ctx->lookup(seq_id);
  if (!lead) return seq_fail(ctx, "gvl_seq_set_guidance", SEQ_BAD);
  if (neg_seq_id == -1) {                              // unbind: both members go on as plain sequences
    if (lead->lead >= 0) return pair_refuse(ctx, "gvl_seq_set_guidance", seq_id, false);
    ctx->unpair(seq_id);
    return 0;
  }
  Seq* fol = ctx->lookup(neg_seq_id);
  if (!fol) return seq_fail(ctx, "gvl_seq_set_guidance", SEQ_BAD);
  if (seq_id == neg_seq_id) return fail(ctx, GVL_ERR_ARG, "gvl_seq_set_guidance: the negative sequence must be another sequence");
  if (const int rc = bank_refuse(ctx, "gvl_seq_set_guidance", seq_id)) return rc;
  if (const int rc = bank_refuse(ctx, "gvl_seq_set_guidance", neg_seq_id)) return rc;
  if (!cond_logits || !neg_logits || cond_logits == neg_logits) return fail(ctx, GVL_ERR_ARG, "gvl_seq_set_guidance: the two prefills' last_logits are needed (two device buffers)");
  if (!std::isfinite(scale)) return fail(ctx, GVL_ERR_ARG, "gvl_seq_set_guidance: scale must be finite");
  if (lead->lead >= 0 || lead->follow >= 0 || fol->lead >= 0 || fol->follow >= 0) return fail(ctx, GVL_ERR_STATE, "gvl_seq_set_guidance: a sequence is already part of a guided pair");
  if (lead->n_gen != 1 || fol->n_gen != 1)
    return fail(ctx, GVL_ERR_STATE, "gvl_seq_set_guidance: both sequences must be freshly prefilled (exactly the one token their own prefill selected)");
  if (fol->max_tokens - fol->pos < lead->max_tokens - lead->pos)
    return fail(ctx, GVL_ERR_STATE, "gvl_seq_set_guidance: the negative sequence has less capacity left than the conditional one");
  hipStream_t st = (hipStream_t)stream;
  // The FIRST token again, from the guided row: the counters go back to 0, so the processors see an empty history, the draw is the one of step 0 and slot 0 of every
  // list is rewritten -- both sequences end where a prefill that had selected from the guided row would have left them (the positions never moved: a prefill's
  // selection carries no position pointer either).
  RUN(GVL_PROF_OTHER, 0, gvl_launch_set_int(lead->d_ngen, 0, st));
  RUN(GVL_PROF_OTHER, 0, gvl_launch_set_int(fol->d_ngen, 0, st));
  PairLaunches pl; memset(&pl, 0, sizeof(pl));
  pl.g.n = ctx->cfg.vocab; pl.g.n_pairs = 1; pl.g.cond[0] = cond_logits; pl.g.neg[0] = neg_logits; pl.g.scale[0] = scale;
  pl.f.n = 1; pl.f.lead_tok[0] = lead->d_tok; pl.f.tok[0] = fol->d_tok; pl.f.out[0] = fol->d_out; pl.f.ngen[0] = fol->d_ngen;
  ArgmaxArgs am; memset(&am, 0, sizeof(am)); am.logits = cond_logits; am.n = ctx->cfg.vocab; am.batch = 1;
  am.tok_ptrs[0] = lead->d_tok; am.out_lists[0] = lead->d_out; am.ngen_ptrs[0] = lead->d_ngen;
  Seq* one[1] = {lead};
  RUN(GVL_PROF_OTHER, 0, pick_tokens(ctx, am, one, st, &pl));
  lead->follow = neg_seq_id; lead->guide = scale; fol->lead = seq_id;
  return 0;
}
// guidance_rows_kernel on caller rows: pair p overwrites row pairs[2p] with the guided row against row pairs[2p + 1] (row r = logits + r * ld), scale scales[p]
int gvl_op_guidance(gvl_ctx* ctx, float* logits, int n, int ld, const int* pairs, int n_pairs, const float* scales, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!logits || !pairs || !scales || n < 1 || ld < n || n_pairs < 1 || n_pairs > GVL_MAX_GUIDANCE_PAIRS)
    return fail(ctx, GVL_ERR_ARG, "gvl_op_guidance: bad arguments (1 .. 8 pairs)");
  GuidanceArgs g; memset(&g, 0, sizeof(g)); g.n = n; g.n_pairs = n_pairs;
  for (int p = 0; p < n_pairs; ++p) {
    const int c = pairs[2 * p], u = pairs[2 * p + 1];
    if (c < 0 || u < 0 || c == u || !std::isfinite(scales[p])) return fail(ctx, GVL_ERR_ARG, "gvl_op_guidance: a pair needs two different rows >= 0 and a finite scale");
    for (int q = 0; q < n_pairs; ++q)                  // a conditional row is written: no other pair may read or write it
      if (q != p && (pairs[2 * q] == c || pairs[2 * q + 1] == c)) return fail(ctx, GVL_ERR_ARG, "gvl_op_guidance: a conditional row appears in another pair");
    g.cond[p] = logits + (size_t)c * ld; g.neg[p] = logits + (size_t)u * ld; g.scale[p] = scales[p];
  }
  hipStream_t st = (hipStream_t)stream;
  RUN(GVL_PROF_OTHER, 0, gvl_launch_guidance_rows(g, st));
  return 0;
}

// score_rows_kernel on raw rows, any number of them (the targets live on the device: one outside [0, n) scores lp = -inf, rank = -1 and never indexes its row)
int gvl_op_score_rows(gvl_ctx* ctx, const float* logits_dev, int n, int ld, int rows, const int32_t* targets_dev, int top_n, float* lp_dev, int32_t* rank_dev,
                      int32_t* top_ids_dev, float* top_lp_dev, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!logits_dev || !targets_dev || !lp_dev || !rank_dev || n < 1 || ld < n || rows < 0) return fail(ctx, GVL_ERR_ARG, "gvl_op_score_rows: bad arguments");
  if (top_n < 0 || top_n > GVL_MAX_TOP_LOGPROBS || (top_n > 0 && (!top_ids_dev || !top_lp_dev)))
    return fail(ctx, GVL_ERR_ARG, "gvl_op_score_rows: top_n must be 0 .. 8 (top lists needed for > 0)");
  hipStream_t st = (hipStream_t)stream;
  ScoreRowsArgs sr; memset(&sr, 0, sizeof(sr));
  sr.logits = logits_dev; sr.n = n; sr.ld = ld; sr.rows = rows; sr.top_n = top_n; sr.targets = targets_dev; sr.lp = lp_dev; sr.rank = rank_dev;
  if (top_n > 0) { sr.top_ids = top_ids_dev; sr.top_lp = top_lp_dev; }
  RUN(GVL_PROF_OTHER, 0, gvl_launch_score_rows(sr, st));
  return 0;
}

}  // extern "C"
