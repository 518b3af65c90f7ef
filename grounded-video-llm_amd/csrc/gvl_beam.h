// gvl_beam.h -- host bookkeeping of beam search (gvl_beam_search): transformers 4.40.1 GenerationMixin._beam_search + BeamSearchScorer / BeamHypotheses [ext] for a
// batch of one and one beam group (GroupBeamState below: several), as grounded_video_llm_amd/beam.py restates them (`_Hyps` and the loop body of `beam_search` with sample = None).  Host-only, no HIP
// (tests/c/beam_check.cc drives it on a CPU and tests/test_beam_host_cpu.py compares it with beam.py step by step); the per-step candidates -- the best 2k of the k x vocab
// grid -- come from the device (gvl_beam.hip).
//   * every score is a double: a candidate value is the fp32 the device added, widened; a hypothesis scores sum / pow((double)generated_len, length_penalty)
//   * an eos candidate of rank < k closes a hypothesis (generated_len counts the eos), of rank >= k is skipped; the first k non-eos candidates are the next beams
//   * done: k hypotheses exist and (early_stopping True, or the worst of them >= max(candidate values) / pow(cur_len, length_penalty)); "never" with a positive
//     length_penalty is an error at the moment the rule would be evaluated, as in beam.py
//   * at max_new_tokens the open beams become hypotheses; among equal best scores the LAST added wins; eos is appended while the output is shorter than max_new_tokens
#pragma once
#include <cmath>
#include <cstddef>
#include <string>
#include <vector>

namespace gvl_beam {

enum Status { BEAM_CONTINUE = 0, BEAM_FINISHED = 1, BEAM_ERR_NEVER = -1, BEAM_ERR_FEW = -2, BEAM_ERR_ARG = -3 };
enum EarlyStopping { EARLY_FALSE = 0, EARLY_TRUE = 1, EARLY_NEVER = 2 };

inline const char* status_text(int s) {
  switch (s) {
    case BEAM_ERR_NEVER: return "early_stopping \"never\" with length_penalty > 0 needs a maximum length: not supported";
    case BEAM_ERR_FEW: return "fewer than num_beams non-eos candidates among the top 2 x num_beams";
    case BEAM_ERR_ARG: return "bad beam-search arguments or candidate list";
    default: return "";
  }
}

// What gvl_beam_search_n (groups 0) and gvl_group_beam_search (groups = num_beam_groups) refuse by the VALUES of their arguments alone, each in its own order: "" or
// what is wrong (the entry prefixes its name).  max_new_cap: the room of a sequence's output list.
inline std::string refusal(bool grouped, int k, int groups, float diversity_penalty, int num_return, int vocab, int max_new, int max_new_cap, int cap, int early_stopping,
                           double length_penalty, float penalty, int ngram, int min_new) {
  const char* nr = num_return < 1 || num_return > k ? "num_return must be 1 .. num_beams" : nullptr;
  if (!grouped && nr) return nr;
  if (k < 2 || k > 16) return "num_beams must be 2 .. 16";
  if (grouped) {
    if (groups < 2 || groups > k || k % groups != 0) return "num_beam_groups must be 2 .. num_beams and divide num_beams";
    if (!(diversity_penalty > 0.f)) return "diversity_penalty must be > 0";
    if (nr) return nr;
  }
  const int s = grouped ? k / groups : k;                  // the rows of one candidate launch
  if (vocab < 2 * s) return grouped ? "vocabulary smaller than 2 x the beams of a group" : "vocabulary smaller than 2 x num_beams";
  if ((long long)vocab * s > 0x7fffffffLL) return grouped ? "beams of a group x vocabulary must fit an int32" : "num_beams x vocabulary must fit an int32";
  if (max_new < 1 || max_new > max_new_cap) return "max_new_tokens must be 1 .. " + std::to_string(max_new_cap);
  if (cap < max_new) return "cap (room of out_ids_host) must be >= max_new_tokens";
  if (early_stopping < 0 || early_stopping > 2) return "early_stopping must be 0 (False), 1 (True) or 2 (\"never\")";
  if (early_stopping == 2 && length_penalty > 0.0) return status_text(BEAM_ERR_NEVER);
  if (!(length_penalty == length_penalty)) return "length_penalty is NaN";
  if (!(penalty > 0.f) || ngram < 0 || min_new < 0) return "penalty must be > 0, ngram >= 0, min_new >= 0";
  return "";
}

// HF's cache reorder as a plan over beam SLOTS: new beam j continues old slot parents[j] (< 0: slot j dies).  The first child of a parent keeps the parent's sequence,
// every further child is a clone of it -- made while the parent is still at the length the children continue from, so before anything is closed --, and a live parent
// without a child is closed.  beams[q] < 0: slot q is closed already.
struct ReorderPlan {
  std::vector<int> src;      // [k] the slot new beam j continues, -1: dies
  std::vector<int> clones;   // the j that get a clone of beams[src[j]], ascending; every other live j takes beams[src[j]] itself
  std::vector<int> closed;   // the live slots nobody continues, ascending
};
// false (plan unusable): a parent out of range or closed already
inline bool reorder(const std::vector<int>& beams, const int* parents, int k, ReorderPlan* plan) {
  plan->src.assign(k, -1); plan->clones.clear(); plan->closed.clear();
  std::vector<char> kept(beams.size(), 0);
  for (int j = 0; j < k; ++j) {
    const int pj = parents[j];
    if (pj < 0) continue;
    if (pj >= (int)beams.size() || beams[pj] < 0) return false;
    plan->src[j] = pj;
    if (kept[pj]) plan->clones.push_back(j); else kept[pj] = 1;
  }
  for (size_t q = 0; q < beams.size(); ++q) if (!kept[q] && beams[q] >= 0) plan->closed.push_back((int)q);
  return true;
}

struct Hyp { double score = 0.0; std::vector<int> ids; bool by_eos = false; std::vector<float> token_scores; };

// BeamHypotheses: at most k hypotheses; `worst` as beam.py's _Hyps.add updates it
struct Hyps {
  int k = 0; double length_penalty = 1.0; int early = EARLY_FALSE;
  std::vector<Hyp> beams; double worst = 1e9;

  void add(const std::vector<int>& ids, double sum_logprobs, int generated_len, bool by_eos, const std::vector<float>& token_scores) {
    const double score = sum_logprobs / std::pow((double)generated_len, length_penalty);
    if ((int)beams.size() >= k && !(score > worst)) return;
    Hyp h; h.score = score; h.ids = ids; h.by_eos = by_eos; h.token_scores = token_scores;
    beams.push_back(std::move(h));
    if ((int)beams.size() > k) {
      // sorted((score, index)): the lowest score goes, the earliest added among equals; the second lowest is the new worst
      size_t lo = 0;
      for (size_t i = 1; i < beams.size(); ++i) if (beams[i].score < beams[lo].score) lo = i;
      size_t lo2 = lo == 0 ? 1 : 0;
      for (size_t i = 0; i < beams.size(); ++i) if (i != lo && beams[i].score < beams[lo2].score) lo2 = i;
      worst = beams[lo2].score;
      beams.erase(beams.begin() + (std::ptrdiff_t)lo);
    } else {
      worst = score < worst ? score : worst;
    }
  }
  // BEAM_CONTINUE (not done), BEAM_FINISHED (done) or BEAM_ERR_NEVER
  int is_done(double best_sum_logprobs, int cur_len) const {
    if ((int)beams.size() < k) return BEAM_CONTINUE;
    if (early == EARLY_TRUE) return BEAM_FINISHED;
    if (early == EARLY_NEVER && length_penalty > 0.0) return BEAM_ERR_NEVER;
    return worst >= best_sum_logprobs / std::pow((double)cur_len, length_penalty) ? BEAM_FINISHED : BEAM_CONTINUE;
  }
};

struct BeamState {
  int k = 0, vocab = 0, max_new = 0, eos = -1;
  Hyps hyps;
  std::vector<std::vector<int>> seqs;            // the ids every running beam generated so far
  std::vector<std::vector<float>> tsc;           // ... and the processed log-probability each of them had in its parent's row
  std::vector<float> scores;                     // running sums, fp32 as the device adds them: [0, -1e9, ...] before the first step
  bool done = false, finished = false;

  // eos_id < 0: none.  BEAM_CONTINUE or BEAM_ERR_ARG
  int init(int num_beams, int vocab_, int max_new_tokens, int eos_id, double length_penalty, int early_stopping) {
    if (num_beams < 2) return BEAM_ERR_ARG;
    return init_sub(num_beams, vocab_, max_new_tokens, eos_id, length_penalty, early_stopping);
  }
  // the same for the s >= 1 beams of one group of a GroupBeamState (a group of one beam is legal; a search of one beam is not)
  int init_sub(int num_beams, int vocab_, int max_new_tokens, int eos_id, double length_penalty, int early_stopping) {
    if (num_beams < 1 || vocab_ < 2 * num_beams || max_new_tokens < 1 || early_stopping < EARLY_FALSE || early_stopping > EARLY_NEVER) return BEAM_ERR_ARG;
    k = num_beams; vocab = vocab_; max_new = max_new_tokens; eos = eos_id < 0 ? -1 : eos_id;
    hyps = Hyps(); hyps.k = k; hyps.length_penalty = length_penalty; hyps.early = early_stopping;
    seqs.assign(k, std::vector<int>()); tsc.assign(k, std::vector<float>());
    scores.assign(k, -1e9f); scores[0] = 0.f;
    done = finished = false;
    return BEAM_CONTINUE;
  }
  int cur_len() const { return (int)seqs[0].size() + 1; }

  // One step's candidates, best first: n (value, flat index beam * vocab + token, processed log-probability) triples, n = 2k from the device.
  // parents / tokens [k]: new beam j continues old beam parents[j] with tokens[j] (first step: parent 0).  BEAM_CONTINUE: advance the beams and come back;
  // BEAM_FINISHED: the search is over (parents / tokens still describe the last beams); < 0: error, nothing usable.
  int step(const float* vals, const int* idx, const float* proc, int n, int* parents, int* tokens) {
    if (finished || n < k || !vals || !idx || !proc) return BEAM_ERR_ARG;
    const int len = cur_len();
    struct Next { float v; int tok, b; float t; };
    std::vector<Next> nxt;
    double best = (double)vals[0];
    for (int r = 0; r < n; ++r) {
      if ((double)vals[r] > best) best = (double)vals[r];
      if (idx[r] < 0 || idx[r] / vocab >= k) return BEAM_ERR_ARG;
    }
    for (int r = 0; r < n && (int)nxt.size() < k; ++r) {
      const int b = idx[r] / vocab, tok = idx[r] % vocab;
      if (eos >= 0 && tok == eos) {
        if (r >= k) continue;
        std::vector<float> ts = tsc[b]; ts.push_back(proc[r]);
        hyps.add(seqs[b], (double)vals[r], len, true, ts);
      } else {
        nxt.push_back(Next{vals[r], tok, b, proc[r]});
      }
    }
    if ((int)nxt.size() < k) return BEAM_ERR_FEW;
    if (!done) {
      const int d = hyps.is_done(best, len);
      if (d < 0) return d;
      done = d == BEAM_FINISHED;
    }
    std::vector<std::vector<int>> s2(k); std::vector<std::vector<float>> t2(k);
    for (int j = 0; j < k; ++j) {
      parents[j] = len == 1 ? 0 : nxt[j].b; tokens[j] = nxt[j].tok;
      s2[j] = seqs[nxt[j].b]; s2[j].push_back(nxt[j].tok);
      t2[j] = tsc[nxt[j].b]; t2[j].push_back(nxt[j].t);
      scores[j] = nxt[j].v;
    }
    seqs.swap(s2); tsc.swap(t2);
    if (done || (int)seqs[0].size() >= max_new) { finished = true; return BEAM_FINISHED; }
    return BEAM_CONTINUE;
  }

  // The n best hypotheses after BEAM_FINISHED (BeamSearchScorer.finalize with num_beam_hyps_to_keep = n, 1 <= n <= k; call it once): popped from
  // sorted(beams, key = score), best first -- among equal scores the LATER added comes first.  Per hypothesis: its new ids (eos included when it ended by eos and there
  // is room), its score, one transition score per id.  Returns how many were written (n; fewer only if fewer hypotheses exist).
  int finalize_n(int n, std::vector<std::vector<int>>* ids, std::vector<double>* score, std::vector<std::vector<float>>* transition) {
    add_open();
    std::vector<const Hyp*> pool;
    for (const Hyp& h : hyps.beams) pool.push_back(&h);
    return emit_best(pool, n, eos, max_new, ids, score, transition);
  }
  // finalize()'s first half: unless the search is done, the open beams become hypotheses
  void add_open() { if (!done) for (int j = 0; j < k; ++j) hyps.add(seqs[j], (double)scores[j], (int)seqs[j].size(), false, tsc[j]); }
  // ... and its second half over `pool` (hypotheses in the order they were added; GroupBeamState pools several Hyps): the n best, best first
  static int emit_best(const std::vector<const Hyp*>& pool, int n, int eos, int max_new, std::vector<std::vector<int>>* ids, std::vector<double>* score,
                       std::vector<std::vector<float>>* transition) {
    std::vector<size_t> order(pool.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    // descending score, the later added first among equals: the reverse of Python's stable ascending sort
    for (size_t i = 1; i < order.size(); ++i)
      for (size_t j = i; j > 0 && (pool[order[j]]->score > pool[order[j - 1]]->score ||
                                   (pool[order[j]]->score == pool[order[j - 1]]->score && order[j] > order[j - 1])); --j) { const size_t t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
    if (n < 1) n = 1;
    const int m = n < (int)order.size() ? n : (int)order.size();
    if (ids) ids->clear();
    if (score) score->clear();
    if (transition) transition->clear();
    for (int r = 0; r < m; ++r) {
      const Hyp& h = *pool[order[r]];
      std::vector<int> out = h.ids;
      if (h.by_eos && eos >= 0 && (int)out.size() < max_new) out.push_back(eos);
      std::vector<float> ts = h.token_scores;
      if (ts.size() > out.size()) ts.resize(out.size());
      if (ids) ids->push_back(out);
      if (score) score->push_back(h.score);
      if (transition) transition->push_back(ts);
    }
    return m;
  }
  // The best hypothesis alone: finalize_n(1)
  void finalize(std::vector<int>* ids, double* score, std::vector<float>* transition) {
    std::vector<std::vector<int>> i1; std::vector<double> s1; std::vector<std::vector<float>> t1;
    if (finalize_n(1, &i1, &s1, &t1) < 1) { i1.assign(1, seqs[0]); s1.assign(1, 0.0); t1.assign(1, tsc[0]); }
    if (ids) *ids = i1[0];
    if (score) *score = s1[0];
    if (transition) *transition = t1[0];
  }
};

// Diverse (group) beam search (gvl_group_beam_search; transformers 4.40.1 _group_beam_search + BeamSearchScorer(num_beam_groups = G), as beam.py's group_beam_search
// restates them): G of the states above, s = k / G beams each, ONE step counter, `done` per group.  Group g owns the global beams g*s .. g*s + s - 1.
//   * a step consumes G candidate lists of 2s triples (flat index = LOCAL beam * vocab + token), group after group; a group that was done when the step began is not
//     looked at: its beams leave with parent -1 and token pad (they are never read again and never become hypotheses)
//   * parents are global: g*s + the local parent (0 at the first step: every beam continues the prompt)
//   * the search is over when every group is done or max_new_tokens ids exist; then every open group adds its beams and the hypotheses of all groups are pooled in group
//     order and ranked as one BeamState ranks its own
struct GroupBeamState {
  int k = 0, G = 0, s = 0, vocab = 0, max_new = 0, eos = -1, pad = -1, n_gen = 0;
  std::vector<BeamState> groups;
  bool finished = false;

  // pad_id < 0: an id that counts nowhere (-1).  BEAM_CONTINUE or BEAM_ERR_ARG
  int init(int num_beams, int num_groups, int vocab_, int max_new_tokens, int eos_id, int pad_id, double length_penalty, int early_stopping) {
    if (num_groups < 2 || num_beams < num_groups || num_beams % num_groups != 0) return BEAM_ERR_ARG;
    k = num_beams; G = num_groups; s = k / G; vocab = vocab_; max_new = max_new_tokens; eos = eos_id < 0 ? -1 : eos_id; pad = pad_id < 0 ? -1 : pad_id; n_gen = 0;
    finished = false;
    groups.assign(G, BeamState());
    for (BeamState& b : groups) if (b.init_sub(s, vocab, max_new, eos_id, length_penalty, early_stopping) < 0) return BEAM_ERR_ARG;
    return BEAM_CONTINUE;
  }
  bool group_done(int g) const { return groups[g].done; }
  float score(int beam) const { return groups[beam / s].done ? 0.f : groups[beam / s].scores[beam % s]; }
  const std::vector<int>& seq(int beam) const { return groups[beam / s].seqs[beam % s]; }

  // vals / idx / proc [G][n]: group g's candidates at + g * n (n = 2s from the device; a done group's are not read).  parents / tokens [k].  BEAM_CONTINUE,
  // BEAM_FINISHED or < 0 as BeamState::step
  int step(const float* vals, const int* idx, const float* proc, int n, int* parents, int* tokens) {
    if (finished || !parents || !tokens) return BEAM_ERR_ARG;
    bool all_done = true;
    for (int g = 0; g < G; ++g) {
      BeamState& b = groups[g];
      if (b.done) { for (int j = 0; j < s; ++j) { parents[g * s + j] = -1; tokens[g * s + j] = pad; } continue; }
      const int rc = b.step(vals + (size_t)g * n, idx + (size_t)g * n, proc + (size_t)g * n, n, parents + g * s, tokens + g * s);
      if (rc < 0) return rc;
      b.finished = false;                                  // the group's own end is not the search's: `done` alone keeps it from being stepped again
      if (n_gen > 0) for (int j = 0; j < s; ++j) parents[g * s + j] += g * s;
      all_done = all_done && b.done;
    }
    ++n_gen;
    if (all_done || n_gen >= max_new) { finished = true; return BEAM_FINISHED; }
    return BEAM_CONTINUE;
  }

  // after BEAM_FINISHED, once: the n best hypotheses over all groups (1 <= n <= k), as BeamState::finalize_n
  int finalize_n(int n, std::vector<std::vector<int>>* ids, std::vector<double>* score_, std::vector<std::vector<float>>* transition) {
    std::vector<const Hyp*> pool;
    for (BeamState& b : groups) { b.add_open(); for (const Hyp& h : b.hyps.beams) pool.push_back(&h); }
    return BeamState::emit_best(pool, n, eos, max_new, ids, score_, transition);
  }
};

}  // namespace gvl_beam
