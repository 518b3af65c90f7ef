// gvl_contrastive.h -- host bookkeeping of contrastive search (gvl_contrastive_search): transformers 4.40.1 GenerationMixin._contrastive_search [ext] for a batch of one,
// as tests/contrastive_ref.py restates it.  Host-only, no HIP (tests/c/contrastive_check.cc drives it on a CPU); the per-step candidates, their degeneration penalties
// and the selected rank come from the device (gvl_contrastive.hip).
//   * a step's k candidates ran on k sequences: the one the search continued from and k - 1 clones of it.  The selected rank's sequence lives on (it takes over the
//     hidden bank), every other one goes back to the pool -- in candidate order, so the pool's free list is a function of the trace alone
//   * the chosen id is appended; the search is finished behind eos (the eos is part of the output) or when max_new ids exist
#pragma once
#include <vector>

namespace gvl_contrastive {

enum Status { CS_CONTINUE = 0, CS_FINISHED = 1, CS_ERR_ARG = -1 };
constexpr int kMaxK = 16;   // GVL_MAX_DECODE_BATCH: the candidates of a step advance in one decode batch

// The limits of gvl_contrastive_search: null, or what is wrong.  The candidate launches give 2 * cand_beams(k) >= k entries of the row, so the row must hold that many.
inline int cand_beams(int k) { return k <= 4 ? 2 : (k + 1) / 2; }
// the ranking kernel keeps the candidates in LDS, padded to 4, 8 or 16 rows of `hidden` bf16: at most 128 KiB
inline int rank_rows(int k) { return k <= 4 ? 4 : (k <= 8 ? 8 : 16); }
constexpr int kRankLdsBytes = 128 * 1024;
inline const char* refusal(int top_k, float alpha, int max_new, int max_new_cap, int cap, int vocab, int hidden) {
  if (top_k < 2 || top_k > kMaxK) return "top_k must be 2 .. 16";
  if (hidden < 64 || hidden % 64) return "hidden must be a multiple of 64";
  if ((long long)rank_rows(top_k) * hidden * 2 > kRankLdsBytes) return "the candidate rows exceed the ranking kernel's 128 KiB of LDS (top_k <= 8 up to hidden 8192, top_k 9 .. 16 up to hidden 4096)";
  if (!(alpha >= 0.f && alpha <= 1.f)) return "penalty_alpha must be in [0, 1]";
  if (vocab < 2 * cand_beams(top_k)) return "vocabulary smaller than the candidate launch's 2 * ((top_k + 1) / 2) entries";
  if (max_new < 1 || max_new > max_new_cap) return "max_new_tokens out of range";
  if (cap < max_new) return "cap (room of out_ids_host) must be >= max_new_tokens";
  return nullptr;
}

struct State {
  int k = 0, max_new = 0, eos = -1;
  std::vector<int> ids;          // the ids chosen so far
  std::vector<int> ranks;        // ... and the rank each had among its step's candidates
  bool finished = false;

  int init(int k_, int max_new_, int eos_) {
    if (k_ < 2 || k_ > kMaxK || max_new_ < 1) return CS_ERR_ARG;
    k = k_; max_new = max_new_; eos = eos_ < 0 ? -1 : eos_; ids.clear(); ranks.clear(); finished = false;
    return CS_CONTINUE;
  }
  // One step.  cand_ids [k]: the candidates in rank order; sel: the rank the device selected; seqs [k]: the sequence candidate i ran on.  *winner = seqs[sel];
  // losers [k - 1] = the others in candidate order.  CS_FINISHED: the chosen id is eos, or it is the max_new-th; CS_ERR_ARG (nothing changed): a rank outside
  // [0, k), a step behind the end, or one sequence named twice.
  int step(const int* cand_ids, int sel, const int* seqs, int* winner, int* losers) {
    if (finished || !cand_ids || !seqs || !winner || !losers || sel < 0 || sel >= k) return CS_ERR_ARG;
    for (int i = 0; i < k; ++i) for (int j = 0; j < i; ++j) if (seqs[i] == seqs[j]) return CS_ERR_ARG;
    *winner = seqs[sel];
    for (int i = 0, n = 0; i < k; ++i) if (i != sel) losers[n++] = seqs[i];
    ids.push_back(cand_ids[sel]); ranks.push_back(sel);
    finished = (eos >= 0 && cand_ids[sel] == eos) || (int)ids.size() >= max_new;
    return finished ? CS_FINISHED : CS_CONTINUE;
  }
};

}  // namespace gvl_contrastive
