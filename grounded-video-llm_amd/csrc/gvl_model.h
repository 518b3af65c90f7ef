// gvl_model.h -- what the host translation units of libgvl.so share: gvl_model.hip (context, weights, paged KV pool, the sequence / prefill / decode
// entry points of include/gvl.h), gvl_ops.hip (the operator entry points), gvl_select.hip (the token-selection entry points), gvl_vision.hip (the towers' launch sequences) and
// gvl_llm.hip (prefill, the decode step -- planned in gvl_decode_plan.h --, the decode loop).  Internal: nothing here is part of the ABI.
// The sequence entries are wrappers: REQUIRE_READY, their own pointer and count checks, ONE admit() call (the table of gvl_admit.h decides which sequences the entry
// takes and says why not), then the work.
#pragma once
#include "gvl_ctx.h"
#include "gvl_admit.h"      // which sequences an entry takes: the admission table and its one function (host-only, tested on the CPU)
#include <functional>
#include "gvl_decode_plan.h"   // the decode path's predicates, batch admission and grouping, and decode_step's launch plan (host-only, tested on the CPU)

namespace gvlm {

inline int fail(gvl_ctx* c, int code, const std::string& msg) { return gvl_fail(c, code, msg); }

#define REQUIRE_READY(cond, what) do { if (!ctx) return GVL_ERR_ARG; if (!ctx->finalized || !(cond)) return fail(ctx, GVL_ERR_STATE, what ": weights not finalized or tower not configured"); } while (0)

// Which sequences an entry takes is decided in gvl_admit.h (one table, one function, tested on the CPU); these turn its verdicts into an entry's result: 0, or the
// status with the message as gvl_last_error.  Nothing is built on the admitted path.
static_assert(gvl_admit::ERR_ARG == GVL_ERR_ARG && gvl_admit::ERR_STATE == GVL_ERR_STATE && gvl_admit::ERR_OOM == GVL_ERR_OOM, "gvl_admit.h restates include/gvl.h's codes");
inline int refuse(gvl_ctx* c, const gvl_admit::Verdict& v) { return v.status ? fail(c, v.status, v.message) : 0; }
// a SeqStatus of the sequence table (gvl_seq_table.h) as the result of entry point `fn`
inline int seq_fail(gvl_ctx* c, const char* fn, int status) { return status >= 0 ? 0 : refuse(c, gvl_admit::seq_refusal(fn, status)); }
// entry `fn` cannot take sequence `id`: a bound follower always, a guided leader too where `leader_too`; a keep-hidden sequence (the entry is not taught the bank)
inline int pair_refuse(gvl_ctx* c, const char* fn, int id, bool leader_too) { return refuse(c, gvl_admit::pair_refusal(c->lookup(id), fn, id, leader_too)); }
inline int bank_refuse(gvl_ctx* c, const char* fn, int id) { return refuse(c, gvl_admit::bank_refusal(c->lookup(id), fn, id)); }
// the members of a call of entry `e` (nums: one number per member `stride` apart, stride 0: one for all); fn: the searches' own name
inline int admit(gvl_ctx* c, gvl_admit::Entry e, const int* ids, int n, const int* nums, int stride, const char* fn = nullptr) {
  const gvl_admit::Limits lim{c->cfg.max_prefill, c->cfg.max_seq, c->outlist_cap, c->cfg.vocab};
  return refuse(c, gvl_admit::admit(*c, e, ids, n, nums, stride, lim, fn));
}
// the log-probability lists of slot `id` (null while the ctx has not allocated them)
inline void bind_logprobs(gvl_ctx* ctx, Seq& s, int id) {
  const size_t cap = (size_t)ctx->outlist_cap;
  s.d_lp = ctx->d_seq_lp ? ctx->d_seq_lp + (size_t)id * cap : nullptr;
  s.d_top_ids = ctx->d_seq_top_ids ? ctx->d_seq_top_ids + (size_t)id * cap * GVL_MAX_TOP_LOGPROBS : nullptr;
  s.d_top_lp = ctx->d_seq_top_lp ? ctx->d_seq_top_lp + (size_t)id * cap * GVL_MAX_TOP_LOGPROBS : nullptr;
}

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

struct ProfScope {
  gvl_ctx* c; hipStream_t st; int idx = -1;
  ProfScope(gvl_ctx* c_, int cat, double work, hipStream_t st_) : c(c_), st(st_) {
    if (!c->prof) return;
    ProfRec r; r.cat = cat; r.work = work;
    hipEventCreate(&r.e0); hipEventCreate(&r.e1);
    hipEventRecord(r.e0, st);
    c->recs.push_back(r); idx = (int)c->recs.size() - 1;
  }
  ~ProfScope() { if (idx >= 0) hipEventRecord(c->recs[idx].e1, st); }
};
#define RUN(cat, work, expr) do { ProfScope _ps(ctx, cat, work, st); int _rc = (expr); if (_rc) return fail(ctx, _rc == -1 ? GVL_ERR_ARG : GVL_ERR_HIP, std::string("launch failed: ") + #expr); } while (0)

inline void* arena_alloc(gvl_ctx* c, size_t bytes) {
  const size_t off = al256(c->arena_off);
  if (off + bytes > c->arena_bytes) return nullptr;
  c->arena_off = off + bytes;
  return c->arena + off;
}
#define AALLOC(var, type, count) type* var = (type*)arena_alloc(ctx, (size_t)(count) * sizeof(type)); if (!var) return fail(ctx, GVL_ERR_OOM, "workspace arena too small for " #var)
inline void* arena_l_alloc(gvl_ctx* c, size_t bytes) {
  const size_t off = al256(c->arena_l_off);
  if (off + bytes > c->arena_l_bytes) return nullptr;
  c->arena_l_off = off + bytes;
  return c->arena_l + off;
}
#define LALLOC(var, type, count) type* var = (type*)arena_l_alloc(ctx, (size_t)(count) * sizeof(type)); if (!var) return fail(ctx, GVL_ERR_OOM, "LLM workspace arena too small for " #var)
// workspace arenas are bump allocators: a call takes a mark and every exit path -- errors included -- must give the space back
struct ArenaScope { size_t& off; const size_t mark; explicit ArenaScope(size_t& o) : off(o), mark(o) {} ~ArenaScope() { off = mark; } };

inline GemmArgs gemm(const bf16_t* A, int lda, const bf16_t* W, void* C, int ldc, int M, int N, int K) {
  GemmArgs g; memset(&g, 0, sizeof(g));
  g.A = A; g.lda = lda; g.W = W; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
  return g;
}

constexpr int kLossChunk = 128;    // rows of logits materialised at a time by the training-forward loss tail
// labelled rows of a training forward: device lists (row index into the sequence, target id) and the per-row nll output
struct LossReq { int n; const int* h_rows; const int* h_targets; float* h_nll; };
constexpr int kScoreChunk = 64;    // rows of fp32 logits a score tail materialises at a time: kScoreChunk * 4 bytes = kLossChunk * 2, the loss tail's reservation serves both
// scored rows of a prefill group (gvl_score_extend_varlen): host lists of n packed row indices (into the group's rows) and their target ids, read before the call returns;
// device outputs [n] (lists [n][GVL_MAX_TOP_LOGPROBS], top_n 1 .. 8 only), written on the call's stream
struct ScoreReq { int n; const int* h_rows; const int* h_targets; int top_n; float* d_lp; int* d_rank; int* d_top_ids; float* d_top_lp; };

// workspace sizes of one call (gvl_create sizes the arenas from them)
size_t clip_bytes(const gvl_ctx* c, int n);
size_t iv2_bytes(const gvl_ctx* c, int n);
size_t visual_bytes(const gvl_ctx* c, int n);
size_t feats_bytes(const gvl_ctx* c, int n);
size_t prefill_bytes(const gvl_ctx* c, int S);

// gvl_vision.hip
int clip_encode(gvl_ctx* ctx, const float* px, int n, float* out, hipStream_t st);
int iv2_encode(gvl_ctx* ctx, const float* px, int n, bf16_t* out, hipStream_t st);
int build_visual(gvl_ctx* ctx, const float* clip_feats, const bf16_t* iv2_feats, int n, bf16_t* visual, hipStream_t st);

// gvl_model.hip: gvl_seq_clone.  carry: the clone of a source with a grammar also takes the source's generated ids, their count and the id to feed next, and the clone of a
// keep-hidden source gets its own bank with a copy of the source's rows (gvl_seq_clone); false: a plain sequence whose history starts empty (the searches' clones: they
// keep the histories and rank the rows themselves)
int seq_clone(gvl_ctx* ctx, int src_seq, int max_tokens, int* dst_seq, hipStream_t stream, bool carry);
// n plain clones at once (gvl_contrastive_search's candidates): all or nothing, one launch for the n partial-page copies, one for the counters; dst_seqs [n]
int seq_clone_many(gvl_ctx* ctx, int src_seq, int max_tokens, int n, int* dst_seqs, hipStream_t stream);
// hidden bank (gvl_seq_keep_hidden; gvl_ctx.h Seq::bank).  bank_alloc: one allocation for `cap` rows, all or nothing.  bank_append (gvl_contrastive.hip): n residual rows x (ldx elements apart) -> final RMSNorm -> bank rows
// [bank_rows, bank_rows + n) and their inverse norms; bank_rows += n
int bank_alloc(gvl_ctx* ctx, Seq& s, int cap);
int bank_append(gvl_ctx* ctx, Seq& s, const bf16_t* x, int ldx, int n, hipStream_t st);

// gvl_search.hip: one search inside the library (gvl_beam_search_n, gvl_group_beam_search, gvl_contrastive_search), entry point `fn`, on `stream`.  Every int result is
// 0 or the error the entry returns (gvl_fail has the message, prefixed with fn).  The searches keep their own loops; this is what they share.
struct SearchSession {
  gvl_ctx* ctx; const char* fn; hipStream_t st;
  SearchSession(gvl_ctx* c, const char* fn_, hipStream_t s) : ctx(c), fn(fn_), st(s) {}
  ~SearchSession();                              // every sequence the search still holds goes back to the pool (its bank with it: gvl_ctx::close)
  SearchSession(const SearchSession&) = delete;
  SearchSession& operator=(const SearchSession&) = delete;

  // The sequence-side refusals, in this order: rules_id, seq_id, guided pairs, the hidden bank (ranks_hidden false: a keep-hidden sequence is refused; true: the bank
  // must be there and in step), "not prefilled" in front of the bank's state.  Then the buffers, the processors / rules / the CALLER's grammar, and `root`: a clone of
  // the caller's sequence with every selection option off (further clones copy that).
  int open(int seq_id, float penalty, int ngram, int min_new, int proc_eos_id, int rules_id, int max_new, bool ranks_hidden);
  int V = 0, pos0 = 0, seq_cap = 0, root = -1;
  LogitsProc proc; const TokenRulesDev* rules = nullptr; const GrammarDev* grammar = nullptr; bool processed = false;

  std::vector<int> ids;                          // the sequences the search holds
  int clone(int src, int* dst);                  // history-less, bank-less clones of seq_cap tokens
  int clone_many(int src, int n, int* dst);      // n at once, all or nothing (seq_clone_many), one GVL_PROF_CS_CLONE record
  void drop(int id);

  // one step's candidates in host-mapped memory, [2 * 16] each: (value, flat index, log-probability), and behind them the [16] tokens the groups of a diverse beam
  // search chose (d_chosen: where the device chains them; d_chosen_mirror / h_chosen: the host-mapped copy)
  float *h_vals = nullptr, *h_proc = nullptr, *d_vals = nullptr, *d_proc = nullptr;
  int *h_idx = nullptr, *d_idx = nullptr, *h_chosen = nullptr, *d_chosen_mirror = nullptr, *d_chosen = nullptr;
  static int ensure_scratch(gvl_ctx* ctx);       // what a candidate launch alone needs (the operator entries)
  static int ensure_buffers(gvl_ctx* ctx);
  static void cand_args(gvl_ctx* ctx, BeamCandArgs& a, const float* rows, int n, int k, int row_stride, const float* scores, int norm, float* vals, int* idx, float* proc);

  // the caller's first_logits -> the first work row (the processors work in place and never on the caller's memory)
  int copy_first(const float* first_logits, float** work);
  // histories of n_rows work rows, `len` ids each (the last GVL_LOGITS_HIST_CAP are kept); row_ids[r] null: zeros.  Two copies on the stream; the staging vector is
  // free again behind the step's synchronise
  int upload_histories(int n_rows, int len, const std::vector<int>* const* row_ids);
  // the processor launch over work rows [n_rows][V] whose histories are rows first_row .. of the last upload; ham_tok: the Hamming term over ham_n chosen tokens
  int process(float* work, int first_row, int n_rows, const int* ham_tok = nullptr, int ham_n = 0, float ham_lambda = 0.f);

  // One teacher-forced step of n sequences: "the context is full", toks[j] -> sequence j's input (null: the caller fed them on the stream), then decode_step per
  // part of the decode path; after_part(first row, rows) runs between a part's step and the gather of its logits rows (d_x still holds the part's residual rows).
  // *rows: [n][V], valid until the next step
  using PartHook = std::function<int(int, int)>;
  int advance(Seq* const* sqs, int n, const int* toks, const PartHook& after_part, float** rows);
  // HF's cache reorder (gvl_beam::reorder, gvl_beam.h) over sequence ids: beams[j] = the sequence of beam j, -1 closed; new beam j continues parents[j] (< 0: dies)
  int reorder(std::vector<int>& beams, const int* parents, int k);
  // the num_return best hypotheses (finalize_n's output, `got` of them) -> the caller's arrays, rows `cap` apart
  int write_hypotheses(int got, int num_return, const std::vector<std::vector<int>>& hyp_ids, const std::vector<double>& score, const std::vector<std::vector<float>>& ts,
                       int32_t* out_ids_host, int cap, int* n_out, double* sequences_scores, float* transition_scores_host);

 private:
  int* d_hist = nullptr; int* d_lens = nullptr; int hs = 1;
  std::vector<int> h_hist;
};

// gvl_llm.hip
int upload_table(gvl_ctx* ctx, Seq& s, hipStream_t st);
// pairs (null: none): the guidance launch in front of the processors and the followers' commit behind the selection -- a group without pairs takes neither
int pick_tokens(gvl_ctx* ctx, ArgmaxArgs& am, Seq* const* sqs, hipStream_t st, const PairLaunches* pairs = nullptr);
// what pick_tokens does behind the processors / rules / grammar launch: log-probability lists, per-row or ctx sampling, the selection launch
int select_tokens(gvl_ctx* ctx, ArgmaxArgs& am, Seq* const* sqs, hipStream_t st);
// the rows of one step for `n` named sequences (plain ones and leaders): rows[] = the named ones in order, then the leaders' followers in order; returns how many
int step_rows(gvl_ctx* ctx, Seq* const* named, int n, Seq** rows);
// the parts one step of `n` named sequences is cut into -> how many, sizes[k] named sequences each: groups of up to 16 rows (VALU fallback: 4, 2, 1), one weight stream
// per step per part.  A guided leader counts two rows: its follower is stepped with it and never split from it (decode_parts_paired; without pairs the cut is decode_parts')
int named_parts(gvl_ctx* ctx, Seq* const* named, int n, int* sizes);
// one group of 1 .. GVL_MAX_PREFILL_BATCH sequences: plans its launches (prefill_plan, gvl_prefill_plan.h -- it refuses before the first launch), then walks the plan
int llm_prefill(gvl_ctx* ctx, Seq* const* sqs, int nb, const bf16_t* const* embeds, const int* lens, hipStream_t st, const LossReq* loss = nullptr, const int* pos0s = nullptr,
                const ScoreReq* score = nullptr, bool keep_hidden = false);   // keep_hidden: one keep-hidden member -- no last-layer tail, every row joins its bank; pos0s: tokens each sequence already holds (null = none); score: rows of the group to score on the way (not with loss)
// one step of B sequences (decode_batch_ok): plans its launches (decode_plan, gvl_decode_plan.h -- it refuses before the first launch), then walks the plan
int decode_step(gvl_ctx* ctx, Seq* const* sqs, int B, hipStream_t st);
int decode_group(gvl_ctx* ctx, Seq* const* sqs, int B, int max_new, int eos_id, int32_t* const* out_ids, int* const* n_out, hipStream_t st);

}  // namespace gvlm
