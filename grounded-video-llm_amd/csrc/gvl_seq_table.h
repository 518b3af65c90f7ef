// gvl_seq_table.h -- host bookkeeping of the paged KV cache's sequences: slots, KV pages and their reference counts, per-sequence token-selection settings, rule-set
// references.  Host-only, no HIP (tests/c/seq_table_check.cc drives it on a CPU); gvl_ctx derives from SeqTable<Seq> and adds the device side.
#pragma once
#include <utility>
#include <vector>

// HF logits processors of one sequence (gvl_logits.hip); the defaults switch every one of them off
struct LogitsProc {
  float penalty = 1.0f; int ngram = 0, min_new = 0, eos = -1;
  bool on() const { return penalty != 1.0f || ngram > 0 || (min_new > 0 && eos >= 0); }
};
// The token-selection settings of one sequence as one value: gvl_seq_alloc copies the table's sel_default (gvl_set_logits_processors / gvl_set_logprobs / gvl_set_token_rules),
// fork and clone copy the source's (an own sampling setting included), the gvl_seq_set_* setters override.  top_n: -1 off, 0 the selected token's log-probability, 1 .. 8 also the top N.  rules: a rule set (-1 none), counted in its refs
// Sampling of one sequence, or the table-wide setting the others follow: greedy unless `on`; then scores * inv_temp -> top-k -> top-p -> min_p -> typical_p -> epsilon -> eta
// (0 = off each; top_p / typical_p are also off at 1) -> one draw from random stream `stream` of `seed`
struct Sampling {
  bool on = false; float inv_temp = 1.0f; int top_k = 0; float top_p = 0.f, min_p = 0.f, typical_p = 0.f, eps = 0.f, eta = 0.f;
  unsigned long long seed = 0; unsigned stream = 0;
  bool warps() const { return on && (min_p > 0.f || (typical_p > 0.f && typical_p < 1.f) || eps > 0.f || eta > 0.f); }   // uses a warper past top-p
};
// own_sampling: the sequence has its own `sampling` (gvl_seq_set_sampling) instead of following the table-wide setting at every selection
// grammar: a decoding grammar (gvl_grammar_create; -1 none), counted in its refs exactly like rules
struct SeqSelect { LogitsProc proc; int top_n = -1; int rules = -1; bool own_sampling = false; Sampling sampling; int grammar = -1; };
// a token rule set: one opaque device blob (gvl_rules_create) and how many sequences / the default reference it
struct RuleSet { bool used = false; void* d = nullptr; int refs = 0; };
// a decoding grammar (gvl_grammar.h): one opaque device blob, the vocabulary it classifies, and how many sequences / the default reference it
struct GrammarSet { bool used = false; void* d = nullptr; int refs = 0; int vocab = 0; };
// the host state of one sequence slot; Seq (gvl_ctx.h) adds the slot's device pointers
struct SeqCore {
  bool used = false; int max_tokens = 0, n_pages = 0, pos = 0, n_gen = 0;
  std::vector<int> pages;   // KV pages in position order, 64 tokens each: whole pages of a prefix may be shared with other sequences (page_ref)
  SeqSelect sel;
  // classifier-free guidance (gvl_seq_set_guidance): a LEADER names its follower in `follow` and carries the pair's scale; the FOLLOWER names its leader in `lead`.
  // A follower takes its leader's token every step and is stepped only as the leader's extra row.  -1: not part of a pair.  A copy (fork / clone) starts unpaired.
  int lead = -1, follow = -1; float guide = 1.0f;
  // hidden bank (gvl_seq_keep_hidden), the host side: room for bank_cap rows (> 0: the sequence keeps its hidden states), bank_rows of them written, row j = position j.
  // The rows themselves are Seq's (gvl_ctx.h); a copy (fork / clone) starts without a bank
  int bank_cap = 0, bank_rows = 0;
};
enum SeqStatus { SEQ_OK = 0, SEQ_BAD = -1, SEQ_DUPLICATE = -2, SEQ_NO_PAGES = -3, SEQ_TOO_MANY = -4, SEQ_NO_RULES = -5, SEQ_RULES_BUSY = -6, SEQ_RULES_FULL = -7,
                 SEQ_NO_GRAMMAR = -8, SEQ_GRAMMAR_BUSY = -9, SEQ_GRAMMAR_FULL = -10, SEQ_FOLLOWER = -11, SEQ_NOT_FRESH = -12, SEQ_PAIRED = -13 };

template <class S = SeqCore>
struct SeqTable {
  std::vector<S> seqs; std::vector<RuleSet> rule_sets; std::vector<GrammarSet> grammars;
  std::vector<int> free_pages, page_ref;   // page_ref: sequences holding each page -- full pages of a shared prefix are referenced, never copied (gvl_seq_fork)
  SeqSelect sel_default;                   // what a sequence without a source starts with (off / none by default)
  const int max_seqs, max_rule_sets;       // slots of the device-side tables; live rule sets
  const int max_grammars;                  // live grammars

  SeqTable(int max_seqs_, int max_rule_sets_, int max_grammars_ = 64) : max_seqs(max_seqs_), max_rule_sets(max_rule_sets_), max_grammars(max_grammars_) {}
  void reset_pool(int pages) { free_pages.clear(); page_ref.assign(pages, 0); for (int p = pages - 1; p >= 0; --p) free_pages.push_back(p); }
  template <class V> static int first_unused(const V& v) { int i = 0; while (i < (int)v.size() && v[i].used) ++i; return i; }   // v.size(): none
  S* lookup(int id) { return id >= 0 && id < (int)seqs.size() && seqs[id].used ? &seqs[id] : nullptr; }
  const S* lookup(int id) const { return id >= 0 && id < (int)seqs.size() && seqs[id].used ? &seqs[id] : nullptr; }
  // ids[i] names a sequence that an earlier member of the group named already
  static bool repeats(const int* ids, int i) { for (int j = 0; j < i; ++j) if (ids[j] == ids[i]) return true; return false; }
  // tests (gvl_debug_seq_pages): the pages of live sequence `id` in position order -> SEQ_OK with *n (may be null) = how many it holds and the first min(cap, that
  // many) of them in out (may be null when cap is 0); SEQ_BAD with nothing written: not a live sequence, cap < 0, cap > 0 without out
  int pages_of(int id, int* out, int cap, int* n) const {
    if (id < 0 || id >= (int)seqs.size() || !seqs[id].used || cap < 0 || (cap > 0 && !out)) return SEQ_BAD;
    const std::vector<int>& p = seqs[id].pages;
    if (n) *n = (int)p.size();
    for (int i = 0; i < cap && i < (int)p.size(); ++i) out[i] = p[i];
    return SEQ_OK;
  }
  bool any_live() const { for (const S& q : seqs) if (q.used) return true; return false; }
  // A new sequence of up to max_tokens tokens -> its id, or a negative SeqStatus with nothing changed.  src < 0 (pos 0): empty, default settings.  src >= 0: it starts with the source's
  // first `pos` tokens and settings; the pos / 64 whole pages of that prefix are shared (immutable from now on for both holders: appends go to later pages), later pages are its own.
  int open(int max_tokens, int src, int pos) {
    const int shared = pos >> 6, np = (max_tokens + 63) / 64;
    if (pos < 0 || max_tokens <= pos || (src < 0 ? pos != 0 : !lookup(src) || shared > (int)seqs[src].pages.size())) return SEQ_BAD;
    if ((int)free_pages.size() < np - shared) return SEQ_NO_PAGES;
    const int id = first_unused(seqs);
    if (id >= max_seqs) return SEQ_TOO_MANY;
    S s;                                   // built aside: growing `seqs` may move the source
    s.used = true; s.max_tokens = max_tokens; s.n_pages = np; s.pos = pos;
    s.sel = src >= 0 ? seqs[src].sel : sel_default;
    if (s.sel.rules >= 0) ++rule_sets[s.sel.rules].refs;
    if (s.sel.grammar >= 0) ++grammars[s.sel.grammar].refs;
    if (src >= 0) s.pages.assign(seqs[src].pages.begin(), seqs[src].pages.begin() + shared);
    for (int p : s.pages) ++page_ref[p];
    for (int i = shared; i < np; ++i) { s.pages.push_back(free_pages.back()); free_pages.pop_back(); page_ref[s.pages.back()] = 1; }
    if (id == (int)seqs.size()) seqs.push_back(std::move(s)); else seqs[id] = std::move(s);
    return id;
  }
  // n clones of `src` at its current length, max_tokens each -> their ids in ids[0 .. n), or a negative SeqStatus with NOTHING changed: pages and slots are counted
  // before the first one opens, so all n open or none does.  Otherwise exactly what n open(max_tokens, src, pos) calls give
  int open_many(int src, int n, int max_tokens, int* ids) {
    const S* s = lookup(src);
    if (!s || n < 1 || !ids || max_tokens <= s->pos) return SEQ_BAD;
    const int pos = s->pos, own_pages = (max_tokens + 63) / 64 - (pos >> 6);
    if ((long long)free_pages.size() < (long long)n * own_pages) return SEQ_NO_PAGES;
    int slots = max_seqs - (int)seqs.size();
    for (const S& q : seqs) slots += !q.used;
    if (slots < n) return SEQ_TOO_MANY;
    for (int i = 0; i < n; ++i) ids[i] = open(max_tokens, src, pos);   // cannot fail: pages and slots were counted above
    return SEQ_OK;
  }
  // gvl_seq_fanout: n_new siblings of the freshly prefilled `src` (n_gen == 1: it holds the one token its own prefill selected) -> their ids in ids[0 .. n_new), or a
  // negative SeqStatus with NOTHING changed -- all siblings open or none does, slots and pages alike.  A sibling is a clone of the source at its current length (whole
  // pages shared, later pages its own) with the source's settings, except that it takes the source's EFFECTIVE sampling -- the source's own setting, else `followed`
  // (the table-wide one at the time of the call, which the caller keeps) -- as a setting of its own, drawing from random stream streams[i].  n_gen = 1: a sibling
  // stands where its own prefill would have left it, its first token selected by the caller from the source's row.
  int fanout(int src, int n_new, int max_tokens, const Sampling& followed, const unsigned* streams, int* ids) {
    const S* s = lookup(src);
    if (!s || n_new < 1 || !streams || !ids || s->pos <= 0 || max_tokens <= s->pos) return SEQ_BAD;
    if (s->lead >= 0 || s->follow >= 0) return SEQ_PAIRED;
    if (s->n_gen != 1) return SEQ_NOT_FRESH;
    Sampling eff = s->sel.own_sampling ? s->sel.sampling : followed;   // by value: open() may move the source
    if (const int rc = open_many(src, n_new, max_tokens, ids)) return rc;
    for (int i = 0; i < n_new; ++i) {
      eff.stream = streams[i];
      set_sampling(seqs[ids[i]].sel, &eff);
      seqs[ids[i]].n_gen = 1;
    }
    return SEQ_OK;
  }
  // the sequence's pages, rule set and grammar go back; a page shared with a fork lives on until its last holder is closed.  A bound follower is refused with nothing
  // changed (its leader's steps write its pages); closing a leader unbinds the pair, and the follower lives on as a plain sequence
  int close(int id) {
    S* s = lookup(id); if (!s) return SEQ_BAD;
    if (s->lead >= 0) return SEQ_FOLLOWER;
    if (s->follow >= 0) unpair(id);
    for (int p : s->pages) if (--page_ref[p] == 0) free_pages.push_back(p);
    if (s->sel.rules >= 0) --rule_sets[s->sel.rules].refs;
    if (s->sel.grammar >= 0) --grammars[s->sel.grammar].refs;
    *s = S(); return SEQ_OK;
  }
  // leader `id` and its follower become plain sequences again (a no-op for a sequence that leads nobody)
  void unpair(int id) {
    S* s = lookup(id); if (!s || s->follow < 0) return;
    if (S* f = lookup(s->follow)) f->lead = -1;
    s->follow = -1; s->guide = 1.0f;
  }
  // `sel` (a sequence's) takes its own sampling setting; q null: back to following the table-wide setting, as a new sequence does
  static void set_sampling(SeqSelect& sel, const Sampling* q) { sel.own_sampling = q != nullptr; sel.sampling = q ? *q : Sampling(); }
  // -1 (none) or a live rule set
  int check_rules(int id) const { return id < -1 || id >= (int)rule_sets.size() || (id >= 0 && !rule_sets[id].used) ? SEQ_NO_RULES : SEQ_OK; }
  int add_rules(void* d) {
    const int id = first_unused(rule_sets);
    if (id >= max_rule_sets) return SEQ_RULES_FULL;
    if (id == (int)rule_sets.size()) rule_sets.emplace_back();
    rule_sets[id] = RuleSet{true, d, 0}; return id;
  }
  // `sel` (a sequence's, or sel_default) takes rule set `id` (-1: none) and drops the one it held
  int set_rules(SeqSelect& sel, int id) {
    if (check_rules(id)) return SEQ_NO_RULES;
    if (id >= 0) ++rule_sets[id].refs;               // before the drop: `id` may be the set it holds
    if (sel.rules >= 0) --rule_sets[sel.rules].refs;
    sel.rules = id; return SEQ_OK;
  }
  // refused while a sequence or the default references the set.  d null: only asks; otherwise the set goes and *d is its blob, which the caller now owns
  int destroy_rules(int id, void** d) {
    if (id < 0 || check_rules(id)) return SEQ_NO_RULES;
    if (rule_sets[id].refs > 0) return SEQ_RULES_BUSY;
    if (d) { *d = rule_sets[id].d; rule_sets[id] = RuleSet(); }
    return SEQ_OK;
  }
  // ---- grammars: the same life cycle as rule sets
  // -1 (none) or a live grammar
  int check_grammar(int id) const { return id < -1 || id >= (int)grammars.size() || (id >= 0 && !grammars[id].used) ? SEQ_NO_GRAMMAR : SEQ_OK; }
  int add_grammar(void* d, int vocab) {
    const int id = first_unused(grammars);
    if (id >= max_grammars) return SEQ_GRAMMAR_FULL;
    if (id == (int)grammars.size()) grammars.emplace_back();
    grammars[id] = GrammarSet{true, d, 0, vocab}; return id;
  }
  // `sel` (a sequence's, or sel_default) takes grammar `id` (-1: none) and drops the one it held
  int set_grammar(SeqSelect& sel, int id) {
    if (check_grammar(id)) return SEQ_NO_GRAMMAR;
    if (id >= 0) ++grammars[id].refs;                // before the drop: `id` may be the grammar it holds
    if (sel.grammar >= 0) --grammars[sel.grammar].refs;
    sel.grammar = id; return SEQ_OK;
  }
  // A grammar's mask is a function of the sequence's generated ids, so a copy taken mid-answer must know them.  Generated id i of `s` sits at position
  // first_generated(s) + i once it is fed (prefill leaves n_gen = 1 with id 0 picked and not yet fed; every step adds one position and one id).
  static int first_generated(const SeqCore& s) { return s.n_gen > 0 ? s.pos - s.n_gen + 1 : s.pos; }
  // a fork's shared prefix of n_tokens would hold generated ids of a source with a grammar: the rows gvl_prefill_extend appends behind it are embeddings whose
  // ids nobody tells the library, so the fork's walk could not be continued -- such a fork is refused (gvl_seq_clone carries the ids instead)
  static bool fork_cuts_answer(const SeqCore& s, int n_tokens) { return s.sel.grammar >= 0 && s.n_gen > 0 && n_tokens > first_generated(s); }
  // refused while a sequence or the default references the grammar.  d null: only asks; otherwise the grammar goes and *d is its blob, which the caller now owns
  int destroy_grammar(int id, void** d) {
    if (id < 0 || check_grammar(id)) return SEQ_NO_GRAMMAR;
    if (grammars[id].refs > 0) return SEQ_GRAMMAR_BUSY;
    if (d) { *d = grammars[id].d; grammars[id] = GrammarSet(); }
    return SEQ_OK;
  }
};
