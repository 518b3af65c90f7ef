// gvl_logits.hip -- HF generate()'s logits processors on the fp32 logit rows of every token-selection site, in place, before argmax_kernel /
// sample_kernel read them (the reference forwards **generate_kwargs to language_model.generate, models/llava_next_video.py:655-661; transformers
// generation/logits_process.py [ext]).  In HF's order:
//   RepetitionPenaltyLogitsProcessor   every DISTINCT token t of the history: s[t] = s[t] < 0 ? s[t] * p : s[t] / p (gather, then scatter)
//   NoRepeatNGramLogitsProcessor       every window h[i .. i + n - 1) equal to the last n - 1 ids bans its next id: s[h[i + n - 1]] = -inf
//   MinLength / MinNewTokensLength     s[eos] = -inf while the history is shorter than min_new
// Token rules (gvl_rules_create; TokenRulesDev in gvl_internal.h) add HF's other token-level processors around them, in HF's order:
//   SequenceBiasLogitsProcessor        BEFORE the penalty: s[t] += the fp32 sum (from 0.0f) of t's length-1 bias, then of every multi-token entry
//                                      ending in t whose first len - 1 ids equal the last len - 1 history ids; entries longer than the history are skipped
//   HammingDiversityLogitsProcessor    (diverse beam search, later groups only) after sequence_bias, BEFORE the penalty: s[t] -= fp32(lambda * count of t among
//                                      the tokens the earlier groups chose at this step), the list read from device memory
//   NoBadWordsLogitsProcessor          after the n-gram bans: the same mechanism with bias -inf
//   PrefixConstrainedLogitsProcessor   after the min-length ban: a decoding grammar (gvl_grammar_create, gvl_grammar.h) -- allowed s[t] += 0.0f, forbidden -inf
//   ForcedEOSTokenLogitsProcessor      after the grammar, when the history holds force_at ids: every score -inf, the forced ids 0
//   SuppressTokens / ...AtBegin        the listed scores -inf (at every step / when the history holds begin_at ids)
// The history is the GENERATED ids only: the reference calls generate(inputs_embeds=...) without input_ids, so HF's input_ids start empty.
// gfx950 only.
#include "gvl_internal.h"

#define CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -3)

// One block of 1024 threads per row.  The history is staged in LDS once (the decode path's history is the sequence's host-mapped output list:
// one coalesced read of L ids instead of n reads per window).  The penalty pass is duplicate-safe: every thread reads all of its s[h[i]] before
// the barrier and writes after it, so a token that occurs several times is stored several times with the SAME value (penalised once, as HF's
// gather -> scatter).  The bans come after a second barrier: no penalty store can overwrite a -inf.  Every operation is one IEEE fp32 multiply,
// divide (correctly rounded: __fdiv_rn) or store -- the result is bit-identical to a torch restatement on the CPU.
// RULES = true is the instantiation for launches in which a row has token rules (a null rules[b] = a row without).  One thread owns one target
// token of a bias table: it sums that target's applicable entries in order and adds once, so no two threads store to one address and the sum
// order is HF's.  Every stage that may store to an address another stage reads or stores differently is fenced by a block barrier (all
// barrier conditions are uniform per block); RULES = false is the kernel without any of it.
__device__ __forceinline__ void bias_stage(float* s, int n, const int* blob, const TokenRulesDev& R, int st, const int* h, int L, int tid) {
  const int* tgt = blob + R.off_tgt[st]; const int* ent = blob + R.off_ent[st]; const int* pre = blob + R.off_pre[st];
  for (int g = tid; g < R.n_tgt[st]; g += 1024) {
    const int tk = tgt[3 * g], e0 = tgt[3 * g + 1], ne = tgt[3 * g + 2];
    if (tk < 0 || tk >= n) continue;
    float sum = 0.f; bool hit = false;
    for (int e = e0; e < e0 + ne; ++e) {
      const int po = ent[3 * e + 1], pl = ent[3 * e + 2];
      if (pl > 0 && pl + 1 > L) continue;                    // HF: `len(sequence_ids) > input_ids.shape[1]` -> ignored
      bool eq = true;
      for (int j = 0; j < pl && eq; ++j) eq = h[L - pl + j] == pre[po + j];
      if (eq) { sum = __fadd_rn(sum, __int_as_float(ent[3 * e])); hit = true; }
    }
    if (hit) s[tk] = __fadd_rn(s[tk], sum);
  }
}

// GRAMMAR = true (with RULES) is the instantiation for launches in which a row has a decoding grammar (a null grammar[b] = a row without): HF's
// PrefixConstrainedLogitsProcessor, after the min-length ban and before forced eos.  The mask is a pure function of the grammar blob and the staged history
// (gvl_grammar.h: the same pack_id / step / edge_allows / is_end as the host's reference walk): the history is rewritten in place as class | ordinal << 8
// (no earlier stage reads it afterwards), the transition table is copied to LDS, thread 0 walks the L entries, and every thread sweeps the row:
// allowed s[t] = s[t] + 0.0f (HF's `scores + mask`: -0.0 becomes +0.0), forbidden -inf.  An OFF walk or an END state leaves the row untouched.
// The barriers are uniform per block: grammar[b] is per row.
__device__ __forceinline__ void grammar_stage(float* s, int n, const GrammarDev* G, int* h, int Lraw, int L, int cap, int tid) {
  namespace gg = gvl_grammar;
  __shared__ unsigned short tr[gg::MAX_TRANS];
  __shared__ int base[gg::MAX_CLASSES];
  __shared__ int at[2];                                      // (state, reg) after the walk; state -1: OFF or END
  const int* blob = reinterpret_cast<const int*>(G);
  const gg::Header H = *G;
  const unsigned char* cls = reinterpret_cast<const unsigned char*>(blob + H.off_class);
  const int* gbase = blob + H.off_base;
  const unsigned short* gtr = reinterpret_cast<const unsigned short*>(blob + H.off_trans);
  const int nt = H.n_states * H.n_classes;
  for (int i = tid; i < L; i += 1024) h[i] = gg::pack_id(h[i], H.vocab, cls, gbase);
  for (int i = tid; i < nt; i += 1024) tr[i] = gtr[i];
  if (tid < H.n_classes) base[tid] = gbase[tid];
  __syncthreads();
  if (tid == 0) {
    int state = H.start, reg = 0;
    bool on = Lraw <= cap;                                   // a history longer than the staged window cannot be walked
    for (int i = 0; on && i < L; ++i) on = gg::step(tr, H.n_classes, state, reg, h[i]);
    at[0] = on && !gg::is_end(tr, H.n_classes, state) ? state : -1; at[1] = reg;
  }
  __syncthreads();
  const int state = at[0], reg = at[1];
  if (state < 0) return;
  const unsigned short* row = tr + state * H.n_classes;
  for (int t = tid; t < n; t += 1024) {
    bool ok = false;
    if (t < H.vocab) { const int c = cls[t], bs = base[c]; ok = gg::edge_allows(row[c], bs >= 0 ? t - bs : 0, reg); }
    s[t] = ok ? __fadd_rn(s[t], 0.0f) : -INFINITY;
  }
}

// HAMMING = true (with RULES and GRAMMAR: one more instantiation, logits_process_hamming_kernel) is the launch for a later group of diverse beam search: HF's
// HammingDiversityLogitsProcessor, after sequence_bias and before the penalty's gather.  ham_tok[b] lists the ham_n[b] <= 16 tokens the earlier groups chose at this
// step -- in DEVICE memory, read at run time: the previous group's choice is made by the kernel in front of this one (beam_group_merge_kernel).  The thread that holds a
// listed token's FIRST occurrence counts its occurrences c and stores once: s[t] = fp32(s[t] - fp32(lambda * fp32(c))), the product rounded, then one subtract (torch's
// `scores -= lambda * bincount` on fp32).  Ids outside [0, n) are ignored.  Its barrier is unconditional: uniform per block.
template <bool RULES, bool GRAMMAR, bool HAMMING>
__device__ __forceinline__ void logits_process_rows(const LogitsProcArgs& a) {
  static_assert(RULES || !GRAMMAR, "the grammar instantiation carries the rules");
  static_assert(!HAMMING || (RULES && GRAMMAR), "the Hamming instantiation carries the rules and the grammar");
  __shared__ int h[GVL_LOGITS_HIST_CAP];
  const int b = blockIdx.x, tid = threadIdx.x;
  float* s = a.logits + (size_t)b * a.ld;
  const int Lraw = a.len_ptrs[b] ? *a.len_ptrs[b] : 0;
  const int L = Lraw < 0 ? 0 : (Lraw > a.cap ? a.cap : Lraw);
  TokenRulesDev R = {};                                      // all zero: every rule off
  const int* blob = nullptr;
  if constexpr (RULES) if (a.rules[b]) { R = *a.rules[b]; blob = reinterpret_cast<const int*>(a.rules[b]); }
  const float p = a.penalty[b];
  const int ng = a.ngram[b];
  const bool pen = p != 1.0f && L > 0, ban = ng > 0 && L >= ng;
  const GrammarDev* G = nullptr;
  if constexpr (GRAMMAR) G = a.grammar[b];
  if (pen || ban || R.n_multi > 0 || G)
    for (int i = tid; i < L; i += 1024) h[i] = a.hist[b][i];
  __syncthreads();
  if constexpr (RULES) {                                     // sequence_bias lands before the penalty's gather
    if (R.n_tgt[0] > 0) bias_stage(s, a.n, blob, R, 0, h, L, tid);
    __syncthreads();
  }
  if constexpr (HAMMING) {
    const int hn = a.ham_n[b] < GVL_MAX_DECODE_BATCH ? a.ham_n[b] : GVL_MAX_DECODE_BATCH;
    if (tid < hn) {
      const int* ht = a.ham_tok[b];
      const int tk = ht[tid];
      if (tk >= 0 && tk < a.n) {
        int c = 0; bool first = true;
        for (int j = 0; j < hn; ++j) if (ht[j] == tk) { ++c; first = first && j >= tid; }
        if (first) {
          // __fsub_rn(s, __fmul_rn(lambda, c)) in plain operators with contraction OFF for this block: the _rn wrappers are ordinary operators, and with contraction
          // allowed the multiply and the subtract fuse into one FMA -- one rounding instead of two, 1 ulp off torch's two ops (guidance_rows_kernel's lesson)
#pragma clang fp contract(off)
          const float pr = a.ham_lambda[b] * (float)c;
          s[tk] = s[tk] - pr;
        }
      }
    }
    __syncthreads();
  }
  if (pen) {
    constexpr int PER = GVL_LOGITS_HIST_CAP / 1024;
    float v[PER]; int t[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = tid + j * 1024;
      t[j] = -1; v[j] = 0.f;
      if (i < L) {
        const int tk = h[i];
        if (tk >= 0 && tk < a.n) { const float x = s[tk]; t[j] = tk; v[j] = x < 0.f ? __fmul_rn(x, p) : __fdiv_rn(x, p); }
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER; ++j) if (t[j] >= 0) s[t[j]] = v[j];
  }
  __syncthreads();
  if (ban) {
    const int m = ng - 1;                    // length of the suffix a window must start with
    const int* suf = h + (L - m);
    for (int i = tid; i <= L - ng; i += 1024) {
      bool eq = true;
      for (int j = 0; j < m && eq; ++j) eq = h[i + j] == suf[j];
      if (eq) { const int tk = h[i + m]; if (tk >= 0 && tk < a.n) s[tk] = -INFINITY; }
    }
  }
  if constexpr (RULES) {                                     // bad_words_ids: after the penalty's scatter and the n-gram bans
    __syncthreads();
    if (R.n_tgt[1] > 0) bias_stage(s, a.n, blob, R, 1, h, L, tid);
    __syncthreads();
  }
  if (tid == 0 && L < a.min_new[b] && a.eos[b] >= 0 && a.eos[b] < a.n) s[a.eos[b]] = -INFINITY;
  if constexpr (GRAMMAR) {
    __syncthreads();                                         // the min-length ban has landed; every reader of the raw history is done
    if (G) grammar_stage(s, a.n, G, h, Lraw, L, a.cap, tid);
  }
  if constexpr (RULES) {
    const bool force = R.n_force > 0 && Lraw == R.force_at;
    __syncthreads();
    if (force) for (int i = tid; i < a.n; i += 1024) s[i] = -INFINITY;
    __syncthreads();
    if (force) for (int j = tid; j < R.n_force; j += 1024) { const int tk = blob[R.off_force + j]; if (tk >= 0 && tk < a.n) s[tk] = 0.f; }
    __syncthreads();
    for (int j = tid; j < R.n_suppress; j += 1024) { const int tk = blob[R.off_suppress + j]; if (tk >= 0 && tk < a.n) s[tk] = -INFINITY; }
    if (R.n_begin > 0 && Lraw == R.begin_at)
      for (int j = tid; j < R.n_begin; j += 1024) { const int tk = blob[R.off_begin + j]; if (tk >= 0 && tk < a.n) s[tk] = -INFINITY; }
  }
}
template <bool RULES, bool GRAMMAR>
__global__ __launch_bounds__(1024) void logits_process_kernel(const LogitsProcArgs a) { logits_process_rows<RULES, GRAMMAR, false>(a); }
__global__ __launch_bounds__(1024) void logits_process_hamming_kernel(const LogitsProcArgs a) { logits_process_rows<true, true, true>(a); }

int gvl_launch_logits_process(const LogitsProcArgs& a, hipStream_t st) {
  if (a.batch < 1 || a.batch > GVL_MAX_DECODE_BATCH || !a.logits || a.n < 1 || a.ld < a.n || a.cap < 0 || a.cap > GVL_LOGITS_HIST_CAP) return -1;
  bool rules = false, grammar = false, hamming = false;
  for (int b = 0; b < a.batch; ++b) {
    if (a.ham_n[b] < 0 || a.ham_n[b] > GVL_MAX_DECODE_BATCH || (a.ham_n[b] > 0 && (!a.ham_tok[b] || !(a.ham_lambda[b] == a.ham_lambda[b])))) return -1;
    hamming = hamming || a.ham_n[b] > 0;
    if (!(a.penalty[b] > 0.f) || a.ngram[b] < 0 || a.min_new[b] < 0) return -1;
    if (a.cap > 0 && (a.penalty[b] != 1.0f || a.ngram[b] > 0 || a.rules[b] || a.grammar[b]) && a.len_ptrs[b] && !a.hist[b]) return -1;
    rules = rules || a.rules[b];
    grammar = grammar || a.grammar[b];
  }
  if (hamming) hipLaunchKernelGGL(logits_process_hamming_kernel, dim3(a.batch), dim3(1024), 0, st, a);
  else if (grammar) hipLaunchKernelGGL((logits_process_kernel<true, true>), dim3(a.batch), dim3(1024), 0, st, a);
  else if (rules) hipLaunchKernelGGL((logits_process_kernel<true, false>), dim3(a.batch), dim3(1024), 0, st, a);
  else hipLaunchKernelGGL((logits_process_kernel<false, false>), dim3(a.batch), dim3(1024), 0, st, a);
  return CHECK_LAUNCH();
}
