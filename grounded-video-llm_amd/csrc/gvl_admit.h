// gvl_admit.h -- which sequences an entry of include/gvl.h takes: ONE table (a row per entry) and ONE function over the sequence table (gvl_seq_table.h).  Host-only,
// no HIP: tests/c/admit_check.cc drives it on a CPU, tests/test_admit_cpu.py holds it to the refusals recorded in tests/golden/entry_refusals.json.
// An entry checks its own pointers and counts, then calls admit() once, then works: everything is refused before the first launch, with every sequence and the pool
// as they were.  Every text of a sequence-side refusal lives here and nowhere else (seq_fail / pair_refuse / bank_refuse of gvl_model.h are wrappers).
#pragma once
#include <cstdio>
#include "gvl_seq_table.h"

namespace gvl_admit {

enum { ERR_ARG = -1, ERR_STATE = -2, ERR_OOM = -4 };   // include/gvl.h's GVL_ERR_* (gvl_model.h asserts that they agree)

// status 0: admitted, the message is empty.  A fixed buffer: the admitted path builds no string and allocates nothing
struct Verdict {
  int status = 0; char message[320];
  Verdict() { message[0] = 0; }
  explicit operator bool() const { return status != 0; }
};
struct Limits { int max_prefill, max_seq, outlist_cap, vocab; };

enum Entry { PREFILL, PREFILL_EXTEND, FORWARD_LOSS, PREFILL_VARLEN, PREFILL_EXTEND_VARLEN, SCORE_EXTEND_VARLEN, DECODE_GREEDY_BATCH, DECODE_STEPS, DECODE_STEP_LOGITS,
             DECODE_STEP_LOGITS_BATCH, SEQ_CLONE, SEQ_CLONE_PLAIN, SEARCH, SEARCH_HIDDEN, N_ENTRIES };

enum Pair { PAIR_ANY, PAIR_NO_FOLLOWER, PAIR_NONE };   // not checked; a bound follower is refused; a leader too (entries that would copy or move one member alone)
// the hidden bank of a keep-hidden sequence: refused (the entry does not fill it); allowed as it is; where there is one it must be in step AND have room for a row;
// where there is one it must be in step (a clone copies its rows); there must be one, in step
enum Bank { BANK_REFUSED, BANK_ALLOWED, BANK_IN_STEP_ROOM, BANK_IN_STEP, BANK_REQUIRED };
// where the sequence must stand: empty; a non-empty prefix of whole pages; empty or whole pages; prefilled with n_gen >= 1; pos > 0 with room left; pos > 0
enum Pos { POS_EMPTY, POS_WHOLE_PREFIX, POS_EMPTY_OR_WHOLE, POS_GENERATED, POS_ROOM_LEFT, POS_PREFILLED };
// the member's number x: none; rows to append (x > 0, behind what the sequence holds within its capacity, x <= max_prefill); steps (pos + x within the capacity, n_gen + x
// within outlist_cap); a fed token (0 <= x < vocab); the capacity of a copy (pos < x <= max_seq)
enum Num { NUM_NONE, NUM_ROWS, NUM_STEPS, NUM_TOKEN, NUM_COPY_CAP };

struct Row {
  const char* fn;          // the prefix of every message (the searches pass their own)
  const char* bad_seq;     // the text for a member that is not a live sequence
  Pair pair; Bank bank; Pos pos; Num num;
  bool num_first;          // the number is checked in front of the position (else behind it)
  bool dups;               // a member named twice is refused
  int pos_status; const char* pos_text;
  const char* num_text;          // null: the position's text and status (one condition in the entry)
  const char* prefill_text;      // NUM_ROWS: an own text for x > max_prefill (null: num_text)
  const char* pos_fn;            // null: fn
};

inline const Row& row_of(Entry e) {
  static const char kHolds[] = "sequence already holds tokens", kBadLen[] = "bad length", kFirst[] = "call gvl_prefill first";
  static const char kWhole[] = "every sequence must be empty or hold a prefix of whole pages (gvl_seq_fork)";
  static const char kStep[] = "bad token / sequence full / not prefilled";
  static const char kCopy[] = "the source must hold tokens and max_tokens must exceed them (and fit cfg.max_seq)";
  static const Row rows[N_ENTRIES] = {
    // today's behaviour: gvl_prefill, gvl_forward_loss and gvl_prefill_varlen never look at guided pairs (the extend and score entries refuse a follower)
    // today's behaviour: gvl_prefill alone takes a keep-hidden sequence (its bank gets a row per prompt row)
    {"gvl_prefill", "bad seq", PAIR_ANY, BANK_ALLOWED, POS_EMPTY, NUM_ROWS, true, false, ERR_STATE, kHolds, kBadLen, nullptr, nullptr},
    {"gvl_prefill_extend", "bad seq", PAIR_NO_FOLLOWER, BANK_REFUSED, POS_WHOLE_PREFIX, NUM_ROWS, false, false, ERR_STATE,
     "the sequence must hold a prefix of whole pages (gvl_seq_fork)", kBadLen, nullptr, nullptr},
    {"gvl_forward_loss", "bad seq", PAIR_ANY, BANK_REFUSED, POS_EMPTY, NUM_ROWS, true, false, ERR_STATE, kHolds, "bad arguments / length", nullptr, nullptr},
    // today's behaviour: only gvl_prefill_varlen has a text of its own for max_prefill
    {"gvl_prefill_varlen", "bad seq / embeds", PAIR_ANY, BANK_REFUSED, POS_EMPTY, NUM_ROWS, true, true, ERR_STATE, kHolds, kBadLen, "seq_len exceeds cfg.max_prefill", nullptr},
    {"gvl_prefill_extend_varlen", "bad seq / embeds", PAIR_NO_FOLLOWER, BANK_REFUSED, POS_EMPTY_OR_WHOLE, NUM_ROWS, false, true, ERR_STATE, kWhole, kBadLen, nullptr, nullptr},
    {"gvl_score_extend_varlen", "bad seq / embeds / next ids", PAIR_NO_FOLLOWER, BANK_REFUSED, POS_EMPTY_OR_WHOLE, NUM_ROWS, false, true, ERR_STATE, kWhole, kBadLen, nullptr, nullptr},
    // today's behaviour: "not prefilled" is reported as gvl_decode_greedy, whichever of the two greedy entries was called
    {"gvl_decode_greedy_batch", "bad seq", PAIR_NO_FOLLOWER, BANK_REFUSED, POS_GENERATED, NUM_NONE, false, true, ERR_STATE, kFirst, nullptr, nullptr, "gvl_decode_greedy"},
    {"gvl_decode_steps", "bad seq", PAIR_NO_FOLLOWER, BANK_REFUSED, POS_GENERATED, NUM_STEPS, false, true, ERR_STATE, kFirst, "sequence would exceed its capacity", nullptr, nullptr},
    {"gvl_decode_step_logits", "bad seq", PAIR_NONE, BANK_IN_STEP_ROOM, POS_ROOM_LEFT, NUM_TOKEN, false, false, ERR_ARG, kStep, nullptr, nullptr, nullptr},
    {"gvl_decode_step_logits_batch", "bad seq", PAIR_NONE, BANK_IN_STEP_ROOM, POS_ROOM_LEFT, NUM_TOKEN, false, true, ERR_ARG, kStep, nullptr, nullptr, nullptr},
    // gvl_seq_clone; the searches' history-less, bank-less clones (one or n at once: today's behaviour, both report as gvl_seq_clone) never look at the bank
    {"gvl_seq_clone", "bad arguments", PAIR_NONE, BANK_IN_STEP, POS_PREFILLED, NUM_COPY_CAP, false, false, ERR_ARG, kCopy, nullptr, nullptr, nullptr},
    {"gvl_seq_clone", "bad arguments", PAIR_NONE, BANK_ALLOWED, POS_PREFILLED, NUM_COPY_CAP, false, false, ERR_ARG, kCopy, nullptr, nullptr, nullptr},
    // SearchSession::open, without and with ranks_hidden (fn is the search's)
    {"", "bad seq", PAIR_NONE, BANK_REFUSED, POS_PREFILLED, NUM_NONE, false, false, ERR_STATE, "the sequence is not prefilled", nullptr, nullptr, nullptr},
    {"", "bad seq", PAIR_NONE, BANK_REQUIRED, POS_PREFILLED, NUM_NONE, false, false, ERR_STATE, "the sequence is not prefilled", nullptr, nullptr, nullptr},
  };
  return rows[e];
}

inline Verdict refusal(int status, const char* fn, const char* text) {
  Verdict v; v.status = status;
  snprintf(v.message, sizeof v.message, "%s: %s", fn, text);
  return v;
}
// a SeqStatus of the sequence table as the result of entry `fn`: admitted for status >= 0
inline Verdict seq_refusal(const char* fn, int status) {
  if (status >= 0) return Verdict();
  static const struct { int code; const char* text; } e[] = {   // indexed by -1 - status: SEQ_BAD .. SEQ_PAIRED
    {ERR_ARG, "bad seq"}, {ERR_ARG, "duplicate seq"}, {ERR_OOM, "KV pages exhausted"}, {ERR_OOM, "too many live sequences"}, {ERR_ARG, "no such rule set"},
    {ERR_STATE, "the rule set is still referenced by a live sequence or is the default (gvl_seq_free / gvl_set_token_rules(-1) first)"},
    {ERR_ARG, "too many live rule sets (limit 1024)"}, {ERR_ARG, "no such grammar"},
    {ERR_STATE, "the grammar is still referenced by a live sequence or is the default (gvl_seq_free / gvl_set_grammar(-1) first)"},
    {ERR_ARG, "too many live grammars (limit 64)"},
    {ERR_STATE, "the sequence follows a guided leader (gvl_seq_set_guidance): free or unbind the leader first"},
    {ERR_STATE, "the sequence must be freshly prefilled (exactly the one token its own prefill selected)"},
    {ERR_STATE, "the sequence is a member of a guided pair (gvl_seq_set_guidance)"}};
  const auto& x = e[status >= SEQ_PAIRED ? -1 - status : 0];
  return refusal(x.code, fn, x.text);
}
// Guided pairs (gvl_seq_set_guidance): `fn` cannot take sequence `id` -- a bound follower always (it is stepped as its leader's extra row and nowhere else), a leader
// too where `leader_too`.  A sequence that is not live is admitted here (the caller has refused it already)
inline Verdict pair_refusal(const SeqCore* s, const char* fn, int id, bool leader_too) {
  Verdict v;
  if (s && s->lead >= 0) { v.status = ERR_STATE; snprintf(v.message, sizeof v.message, "%s: sequence %d follows guided leader %d; name the leader", fn, id, s->lead); }
  else if (s && leader_too && s->follow >= 0) { v.status = ERR_STATE; snprintf(v.message, sizeof v.message, "%s: sequence %d leads a guided pair (gvl_seq_set_guidance(seq, -1, ...) unbinds)", fn, id); }
  return v;
}
// Entries that are not taught the hidden bank refuse a keep-hidden sequence: its bank would fall out of step with its position
inline Verdict bank_refusal(const SeqCore* s, const char* fn, int id) {
  Verdict v;
  if (s && s->bank_cap > 0) { v.status = ERR_STATE; snprintf(v.message, sizeof v.message, "%s: sequence %d keeps its hidden states (gvl_seq_keep_hidden); this entry does not fill the bank", fn, id); }
  return v;
}

// Members ids[0 .. n) of a call of entry `e`, in call order; per member the checks in the entry's order: live, guided pair, bank refused, position and number (num_first:
// the number in front), duplicate, the bank's state.  The first refusal is the answer.  nums[i * num_stride] is member i's number (num_stride 0: one for all).
template <class S>
Verdict admit(const SeqTable<S>& t, Entry e, const int* ids, int n, const int* nums, int num_stride, const Limits& lim, const char* fn = nullptr) {
  const Row& r = row_of(e);
  if (!fn) fn = r.fn;
  for (int i = 0; i < n; ++i) {
    const int id = ids[i];
    const SeqCore* s = t.lookup(id);
    if (!s) return refusal(ERR_ARG, fn, r.bad_seq);
    if (r.pair != PAIR_ANY) if (Verdict v = pair_refusal(s, fn, id, r.pair == PAIR_NONE)) return v;
    if (r.bank == BANK_REFUSED) if (Verdict v = bank_refusal(s, fn, id)) return v;
    const int x = nums ? nums[(size_t)i * num_stride] : 0;
    bool pos_ok = true, num_ok = true, prefill_ok = true;
    switch (r.pos) {
      case POS_EMPTY: pos_ok = s->pos == 0; break;
      case POS_WHOLE_PREFIX: pos_ok = s->pos > 0 && !(s->pos & 63); break;
      case POS_EMPTY_OR_WHOLE: pos_ok = s->pos >= 0 && !(s->pos & 63); break;
      case POS_GENERATED: pos_ok = s->n_gen >= 1; break;
      case POS_ROOM_LEFT: pos_ok = s->pos > 0 && s->pos < s->max_tokens; break;
      case POS_PREFILLED: pos_ok = s->pos > 0; break;
    }
    switch (r.num) {
      case NUM_NONE: break;
      case NUM_ROWS:   // an entry for empty sequences measures x against the capacity alone: its length check stands in front of its position check
        num_ok = x > 0 && (long long)(r.pos == POS_EMPTY ? 0 : s->pos) + x <= s->max_tokens; prefill_ok = x <= lim.max_prefill; break;
      case NUM_STEPS: num_ok = (long long)s->pos + x <= s->max_tokens && (long long)s->n_gen + x <= lim.outlist_cap; break;
      case NUM_TOKEN: num_ok = x >= 0 && x < lim.vocab; break;
      case NUM_COPY_CAP: num_ok = x > s->pos && x <= lim.max_seq; break;
    }
    const char* num_text = r.num_text ? r.num_text : r.pos_text;
    const int num_status = r.num_text ? ERR_ARG : r.pos_status;
    if (r.num_first) {
      if (!num_ok) return refusal(num_status, fn, num_text);
      if (!prefill_ok) return refusal(num_status, fn, r.prefill_text ? r.prefill_text : num_text);
    }
    if (!pos_ok) return refusal(r.pos_status, r.pos_fn ? r.pos_fn : fn, r.pos_text);
    if (!r.num_first) {
      if (!num_ok) return refusal(num_status, fn, num_text);
      if (!prefill_ok) return refusal(num_status, fn, r.prefill_text ? r.prefill_text : num_text);
    }
    if (r.dups && SeqTable<S>::repeats(ids, i)) return seq_refusal(fn, SEQ_DUPLICATE);
    const bool has = s->bank_cap > 0;
    if (r.bank == BANK_REQUIRED && !has) return refusal(ERR_STATE, fn, "the sequence keeps no hidden states (gvl_seq_keep_hidden before its prefill)");
    if (r.bank == BANK_IN_STEP) {            // gvl_seq_clone: what the clone takes along must fit and be whole
      if (s->sel.grammar >= 0 && s->n_gen > lim.outlist_cap) return refusal(ERR_STATE, fn, "the source generated more ids than an output list holds");
      if (has && s->bank_rows != s->pos) return refusal(ERR_STATE, fn, "the source's hidden bank is not in step with its position");
    }
    if ((r.bank == BANK_REQUIRED && s->bank_rows != s->pos) || (r.bank == BANK_IN_STEP_ROOM && has && (s->bank_rows != s->pos || s->bank_rows >= s->bank_cap)))
      return refusal(ERR_STATE, fn, "the hidden bank is not in step with the sequence");
  }
  return Verdict();
}

}  // namespace gvl_admit
