// gvl_logits.hip -- HF generate()'s logits processors on the fp32 logit rows of every token-selection site, in place, before argmax_kernel /
// sample_kernel read them (the reference forwards **generate_kwargs to language_model.generate, models/llava_next_video.py:655-661; transformers
// generation/logits_process.py [ext]).  In HF's order:
//   RepetitionPenaltyLogitsProcessor   every DISTINCT token t of the history: s[t] = s[t] < 0 ? s[t] * p : s[t] / p (gather, then scatter)
//   NoRepeatNGramLogitsProcessor       every window h[i .. i + n - 1) equal to the last n - 1 ids bans its next id: s[h[i + n - 1]] = -inf
//   MinLength / MinNewTokensLength     s[eos] = -inf while the history is shorter than min_new
// The history is the GENERATED ids only: the reference calls generate(inputs_embeds=...) without input_ids, so HF's input_ids start empty.
// gfx950 only.
#include "gvl_internal.h"

#define CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -3)

// One block of 1024 threads per row.  The history is staged in LDS once (the decode path's history is the sequence's host-mapped output list:
// one coalesced read of L ids instead of n reads per window).  The penalty pass is duplicate-safe: every thread reads all of its s[h[i]] before
// the barrier and writes after it, so a token that occurs several times is stored several times with the SAME value (penalised once, as HF's
// gather -> scatter).  The bans come after a second barrier: no penalty store can overwrite a -inf.  Every operation is one IEEE fp32 multiply,
// divide (correctly rounded: __fdiv_rn) or store -- the result is bit-identical to a torch restatement on the CPU.
__global__ __launch_bounds__(1024) void logits_process_kernel(const LogitsProcArgs a) {
  __shared__ int h[GVL_LOGITS_HIST_CAP];
  const int b = blockIdx.x, tid = threadIdx.x;
  float* s = a.logits + (size_t)b * a.ld;
  int L = a.len_ptrs[b] ? *a.len_ptrs[b] : 0;
  L = L < 0 ? 0 : (L > a.cap ? a.cap : L);
  const float p = a.penalty[b];
  const int ng = a.ngram[b];
  const bool pen = p != 1.0f && L > 0, ban = ng > 0 && L >= ng;
  if (pen || ban)
    for (int i = tid; i < L; i += 1024) h[i] = a.hist[b][i];
  __syncthreads();
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
  if (tid == 0 && L < a.min_new[b] && a.eos[b] >= 0 && a.eos[b] < a.n) s[a.eos[b]] = -INFINITY;
}

int gvl_launch_logits_process(const LogitsProcArgs& a, hipStream_t st) {
  if (a.batch < 1 || a.batch > GVL_MAX_DECODE_BATCH || !a.logits || a.n < 1 || a.ld < a.n || a.cap < 0 || a.cap > GVL_LOGITS_HIST_CAP) return -1;
  for (int b = 0; b < a.batch; ++b) {
    if (!(a.penalty[b] > 0.f) || a.ngram[b] < 0 || a.min_new[b] < 0) return -1;
    if (a.cap > 0 && (a.penalty[b] != 1.0f || a.ngram[b] > 0) && a.len_ptrs[b] && !a.hist[b]) return -1;
  }
  hipLaunchKernelGGL(logits_process_kernel, dim3(a.batch), dim3(1024), 0, st, a);
  return CHECK_LAUNCH();
}
