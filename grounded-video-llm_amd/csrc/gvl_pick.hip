// gvl_pick.hip -- token selection of a decode step: greedy argmax, the sampler, per-row selection with HF's further warpers, the log-probability pass and the beam-search
// candidates; and, at the end of the file, the scores of GIVEN ids (score_rows_kernel).  gfx950 only.  One block of 1024 threads per logit row; every pass re-reads the row from L2.
// Shared stages, each a __device__ __forceinline__ function that exists once: pick_row_max (both samplers, beam_row_norm), pick_greedy_row (argmax_kernel and the greedy
// rows of select_rows_kernel; pick_wave_pair / pick_pair_finish inside it), pick_radix_select (top-k in both samplers, the beam candidates), pick_commit (all four
// selections), lp_after_draw (both samplers) and the launcher launch_lp_mode.  The kernel declares its LDS and tid and hands them in; inputs go by value, results come
// back through references that are only written.
// NOT shared: the sampled row's normaliser, top-p bisection and Gumbel draw (stages 3 - 5) are written out in sample_kernel and in select_rows_kernel, in the same
// words.  As functions they compiled to another instruction stream (the compiler then evaluates expf for every entry and selects), slower for sample_kernel
// (profiles/pick_refactor_asm.txt); written out, sample_kernel<0> and argmax_kernel<0> are instruction for instruction what they were.  That was observed with ROCm's hipcc as of this change
// and nothing pins it: after a compiler update or a change to a stage's signature, re-take profiles/pick_refactor_asm.txt (tools/asm_diff.py).
// Operation order is part of the contract between the kernels: every reduction order, every barrier that orders a reuse of LDS and every float expression is kept as written.
#include "gvl_internal.h"

#define CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -3)

// ---- log-probabilities of the selected token and the best N alternatives (ArgmaxArgs.top_n / lp_lists / top_ids / top_lp).  The selection
// kernels take a mode LPM: 0 = off (today's kernels, instruction for instruction), 1 = the selected token's log-probability, 2 = also the top N.
// The distribution is the one the token was selected from: log_softmax of the (processed) row for greedy, the warped distribution for sampling
// ((s - m) * invT over the final kept set, everything else -inf).  One extra pass over the row (in L2 by then): a fixed-order sum of
// exp((s - m) * invT) over the kept set (strided per thread, then the smp_block_sum butterfly -- a pure function of the row), and a per-thread
// register list of the best 8 finite kept entries, merged per wave (8 rounds of a butterfly max over the list heads) and across the 16 waves
// through LDS.  The order is (value descending, lower id first), a strict total order: the merged list does not depend on who held what.
// The token path is untouched: the pass runs after the selection's own passes and never feeds them.
__device__ __forceinline__ unsigned smp_fmix32(unsigned h) { h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16; return h; }
__device__ __forceinline__ unsigned smp_key(float v) { const unsigned b = __float_as_uint(v); return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }   // order-preserving
__device__ __forceinline__ float smp_block_sum(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);          // butterfly: bitwise the same total in every lane
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < 16; ++w) t += sh[w];
  return t;
}
// row maximum, in every thread (fixed order: a pure function of the row)
__device__ __forceinline__ float pick_row_max(const float* l, int n, int tid, float (&shf)[16]) {
  float m = -3.4e38f;
  for (int i = tid; i < n; i += 1024) m = fmaxf(m, l[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((tid & 63) == 0) shf[tid >> 6] = m;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 16; ++w) m = fmaxf(m, shf[w]);
  return m;
}
struct PickPair { float best; int idx; };      // a (score, index) candidate; the better of two: higher score, then lower index
// the wave's best pair, in every lane
__device__ __forceinline__ void pick_wave_pair(float best, int idx, PickPair& out) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(idx, o, 64);
    if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
  }
  out.best = best; out.idx = idx;
}
// wave 0's pair -> the block's, from the per-wave pairs in LDS
__device__ __forceinline__ void pick_pair_finish(const float (&shf)[16], const int (&shi)[16], float best, int idx, PickPair& out) {
  for (int w = 1; w < 16; ++w) if (shf[w] > best || (shf[w] == best && shi[w] < idx)) { best = shf[w]; idx = shi[w]; }
  out.best = best; out.idx = idx;
}
__device__ __forceinline__ bool lp_better(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }
// (v, i) into a thread's descending list: the carried entry swaps with every slot it beats (the list stays sorted, the last entry drops out)
__device__ __forceinline__ void lp_insert(float (&tv)[GVL_MAX_TOP_LOGPROBS], int (&ti)[GVL_MAX_TOP_LOGPROBS], float v, int i) {
  if (!lp_better(v, i, tv[GVL_MAX_TOP_LOGPROBS - 1], ti[GVL_MAX_TOP_LOGPROBS - 1])) return;
#pragma unroll
  for (int j = 0; j < GVL_MAX_TOP_LOGPROBS; ++j)
    if (lp_better(v, i, tv[j], ti[j])) { const float t = tv[j]; const int u = ti[j]; tv[j] = v; ti[j] = i; v = t; i = u; }
}
// the best GVL_MAX_TOP_LOGPROBS entries of the 64 lists of a wave, in order, in every lane (wv / wi); the lists are consumed
__device__ __forceinline__ void lp_wave_merge(float (&tv)[GVL_MAX_TOP_LOGPROBS], int (&ti)[GVL_MAX_TOP_LOGPROBS], float (&wv)[GVL_MAX_TOP_LOGPROBS],
                                              int (&wi)[GVL_MAX_TOP_LOGPROBS]) {
#pragma unroll
  for (int r = 0; r < GVL_MAX_TOP_LOGPROBS; ++r) {
    float bv = tv[0]; int bi = ti[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
      if (lp_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    wv[r] = bv; wi[r] = bi;
    if (bi >= 0 && ti[0] == bi) {          // ids are unique across lanes: exactly the owner pops its head
#pragma unroll
      for (int j = 0; j + 1 < GVL_MAX_TOP_LOGPROBS; ++j) { tv[j] = tv[j + 1]; ti[j] = ti[j + 1]; }
      tv[GVL_MAX_TOP_LOGPROBS - 1] = -INFINITY; ti[GVL_MAX_TOP_LOGPROBS - 1] = -1;
    }
  }
}
// Whole block, row b on (block-uniform).  Kept set: keys >= thr (0: every entry).  Returns log(sum over the kept set of exp((s - m) * invT));
// with LPM == 2 and top_n[b] > 0 it also stores row b's top list at generation index g.  BAND (select_rows_kernel): the kept set is thr <= key <= hi.
template <int LPM, bool BAND = false>
__device__ float lp_row_pass(const ArgmaxArgs& a, int b, const float* l, float m, float inv_temp, unsigned thr, int g, [[maybe_unused]] unsigned hi = 0xffffffffu) {
  __shared__ float shz[16];
  const int tid = threadIdx.x, n = a.n;
  const bool top = LPM == 2 && a.top_n[b] > 0 && a.top_ids[b] && a.top_lp[b];
  float tv[GVL_MAX_TOP_LOGPROBS]; int ti[GVL_MAX_TOP_LOGPROBS];
#pragma unroll
  for (int j = 0; j < GVL_MAX_TOP_LOGPROBS; ++j) { tv[j] = -INFINITY; ti[j] = -1; }
  float z = 0.f;
  for (int i = tid; i < n; i += 1024) {
    const float v = l[i];
    if (smp_key(v) < thr) continue;
    if constexpr (BAND) if (smp_key(v) > hi) continue;
    z += expf((v - m) * inv_temp);
    if (LPM == 2 && top && fabsf(v) < INFINITY) lp_insert(tv, ti, v, i);
  }
  const float lz = logf(smp_block_sum(z, shz));
  if constexpr (LPM == 2) {
    if (top) {
      __shared__ float s_tv[16 * GVL_MAX_TOP_LOGPROBS];
      __shared__ int s_ti[16 * GVL_MAX_TOP_LOGPROBS];
      float wv[GVL_MAX_TOP_LOGPROBS]; int wi[GVL_MAX_TOP_LOGPROBS];
      lp_wave_merge(tv, ti, wv, wi);
      if ((tid & 63) == 0) {
#pragma unroll
        for (int r = 0; r < GVL_MAX_TOP_LOGPROBS; ++r) { s_tv[(tid >> 6) * GVL_MAX_TOP_LOGPROBS + r] = wv[r]; s_ti[(tid >> 6) * GVL_MAX_TOP_LOGPROBS + r] = wi[r]; }
      }
      __syncthreads();
      if (tid < 64) {
        const int lane = tid;
#pragma unroll
        for (int j = 0; j < GVL_MAX_TOP_LOGPROBS; ++j) {
          tv[j] = lane < 16 ? s_tv[lane * GVL_MAX_TOP_LOGPROBS + j] : -INFINITY; ti[j] = lane < 16 ? s_ti[lane * GVL_MAX_TOP_LOGPROBS + j] : -1;
        }
        lp_wave_merge(tv, ti, wv, wi);
        float v = -INFINITY; int id = -1;
#pragma unroll
        for (int r = 0; r < GVL_MAX_TOP_LOGPROBS; ++r) if (lane == r) { v = wv[r]; id = wi[r]; }
        if (lane < GVL_MAX_TOP_LOGPROBS) {
          const bool ok = lane < a.top_n[b] && id >= 0;
          a.top_ids[b][(size_t)g * GVL_MAX_TOP_LOGPROBS + lane] = ok ? id : -1;
          a.top_lp[b][(size_t)g * GVL_MAX_TOP_LOGPROBS + lane] = ok ? (v - m) * inv_temp - lz : -INFINITY;
        }
      }
    }
  }
  return lz;
}
__device__ __forceinline__ bool lp_row_on(const ArgmaxArgs& a, int b) { return a.top_n[b] >= 0 && a.lp_lists[b] != nullptr; }
__device__ __forceinline__ int lp_row_step(const ArgmaxArgs& a, int b) { return a.ngen_ptrs[b] ? *a.ngen_ptrs[b] : 0; }
// The commit of row b's token (the caller is thread 0, after it finished the per-wave pairs): the token, the output list, the generation count, the eos flag (a system-scope
// store: the host polls the word) and the position.  LPM > 0 (greedy rows only): the token's log-probability 0 - lz (s_tok - m = 0) goes between the token and the counters,
// indexed by the step the bump ends.
template <int LPM = 0>
__device__ __forceinline__ void pick_commit(const ArgmaxArgs& a, int b, int idx, [[maybe_unused]] float lz = 0.f) {
  *a.tok_ptrs[b] = idx;
  if constexpr (LPM > 0) if (lp_row_on(a, b)) a.lp_lists[b][lp_row_step(a, b)] = 0.f - lz;
  if (a.ngen_ptrs[b]) {
    const int g = *a.ngen_ptrs[b]; if (a.out_lists[b]) a.out_lists[b][g] = idx; *a.ngen_ptrs[b] = g + 1;
    if (a.eos_flags[b] && idx == a.eos_id && *a.eos_flags[b] == 0) __hip_atomic_store(a.eos_flags[b], g + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (a.pos_ptrs[b]) (*a.pos_ptrs[b])++;
}
// A greedy row, whole block: first index of the maximum (torch.argmax tie rule).  kept: select_rows_kernel's operator output, by reference so that it is read where it is used (null in argmax_kernel: the store compiles out).
// The log-probability pass runs BEFORE the commit here: thread 0 stores the token's log-probability inside it, at the step the commit then bumps.
template <int LPM>
__device__ __forceinline__ void pick_greedy_row(const ArgmaxArgs& a, int b, int tid, const float* l, float (&shf)[16], int (&shi)[16], unsigned char* const& kept) {
  const int n = a.n;
  float best = -3.4e38f; int idx = 0x7fffffff;
  for (int i = tid; i < n; i += 1024) {
    const float v = l[i];
    if (v > best) { best = v; idx = i; }
  }
  PickPair p; pick_wave_pair(best, idx, p);
  if ((tid & 63) == 0) { shf[tid >> 6] = p.best; shi[tid >> 6] = p.idx; }
  __syncthreads();
  [[maybe_unused]] float lz = 0.f;
  if constexpr (LPM > 0) {
    if (lp_row_on(a, b)) {                   // every thread needs the row maximum: the same scan thread 0 makes in the commit
      PickPair f; pick_pair_finish(shf, shi, shf[0], shi[0], f);
      const float m = f.best;
      lz = lp_row_pass<LPM>(a, b, l, m, 1.0f, 0u, lp_row_step(a, b));
    }
  }
  if (kept) for (int i = tid; i < n; i += 1024) kept[(size_t)b * n + i] = fabsf(l[i]) < INFINITY ? 1 : 0;
  if (tid == 0) { PickPair f; pick_pair_finish(shf, shi, p.best, p.idx, f); pick_commit<LPM>(a, b, f.idx, lz); }
}
// greedy sampling; one block per logit row
template <int LPM>
__global__ __launch_bounds__(1024) void argmax_kernel(const ArgmaxArgs a) {
  __shared__ float bv[16];
  __shared__ int bi[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  pick_greedy_row<LPM>(a, b, tid, a.logits + (size_t)b * a.n, bv, bi, nullptr);
}
// 0: no row wants log-probabilities (the launch is today's), 1: chosen tokens only, 2: some row wants its top N as well; -1: bad top_n
static int lp_mode(const ArgmaxArgs& a) {
  int mode = 0;
  for (int b = 0; b < a.batch; ++b) {
    if (a.top_n[b] > GVL_MAX_TOP_LOGPROBS) return -1;
    if (a.top_n[b] < 0 || !a.lp_lists[b]) continue;
    const int m = a.top_n[b] > 0 && a.top_ids[b] && a.top_lp[b] ? 2 : 1;
    mode = m > mode ? m : mode;
  }
  return mode;
}
// one launch of the instantiation the rows' log-probability settings ask for, one block per row
template <class Args>
static int launch_lp_mode(void (*k0)(Args), void (*k1)(Args), void (*k2)(Args), const ArgmaxArgs& a, const Args& args, hipStream_t st) {
  const int mode = lp_mode(a);
  if (mode < 0) return -1;
  void (*k)(Args) = mode == 0 ? k0 : mode == 1 ? k1 : k2;
  hipLaunchKernelGGL(k, dim3(a.batch), dim3(1024), 0, st, args);
  return CHECK_LAUNCH();
}
int gvl_launch_argmax(const ArgmaxArgs& a, hipStream_t st) {
  if (a.batch < 1 || a.batch > GVL_MAX_DECODE_BATCH) return -1;
  return launch_lp_mode(argmax_kernel<0>, argmax_kernel<1>, argmax_kernel<2>, a, a, st);
}
// ---- sampling (do_sample=True): the reference forwards do_sample / temperature / top_p to HF generate (models/llava_next_video.py:655-661;
// inference.py:45-49 defaults do_sample=True, T=0.2, top_p=None; HF's GenerationConfig adds top_k=50).  HF order [ext: transformers
// generation/logits_process.py]: scores / T -> top-k (keep scores >= the k-th largest, ties kept) -> top-p (sorted ascending, drop while
// the cumulative probability <= 1 - top_p, i.e. keep a token iff the mass of strictly larger scores is < top_p) -> softmax -> one draw.
// The draw is Gumbel-max, token = argmax_i (l_i - max) / T - log(-log u_i), u_i = counter hash of (seed, stream, step, i): a sample of
// exactly softmax(l / T) restricted to the kept set, with no sort and no prefix sum.  torch.multinomial's Philox stream cannot be
// reproduced, so parity is: same kept set and same token as the CPU restatement `sample_token` used by the tests (same hash), and the right distribution.
// One block per row; every pass re-reads the row from L2 (32 k - 128 k floats).  All reductions run in a fixed order and every
// thread sees the same totals, so the thresholds are wave-uniform and the result does not depend on the batch a row travels in.

// Whole block: the key of the `want`-th largest of the keys keyf hands out for i in [0, n) (keyf returns false for an entry outside the set), by an 8-bit radix select
// (integer counts: exact).  TIES (beam search): *take = how many entries AT that key belong to the best `want`, *ties = how many entries hold it, and sel is three words of
// LDS; without it sel is two words and the loop carries neither.
template <bool TIES, class F>
__device__ __forceinline__ void pick_radix_select(int tid, int n, int want, F keyf, int (&hist)[256], unsigned (&sel)[TIES ? 3 : 2], unsigned& kth, [[maybe_unused]] int* take = nullptr,
                                                  [[maybe_unused]] int* ties = nullptr) {
  unsigned prefix = 0; int remaining = want;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
      unsigned k;
      if (!keyf(i, k)) continue;
      if (shift == 24 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(k >> shift) & 255], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int c = 0, bsel = 0;
      for (int q = 255; q >= 0; --q) { if (c + hist[q] >= remaining) { bsel = q; break; } c += hist[q]; }
      sel[0] = prefix | ((unsigned)bsel << shift); sel[1] = (unsigned)(remaining - c);
      if constexpr (TIES) sel[2] = (unsigned)hist[bsel];
    }
    __syncthreads();
    prefix = sel[0]; remaining = (int)sel[1];
    if constexpr (TIES) *ties = (int)sel[2];
    __syncthreads();
  }
  kth = prefix;
  if constexpr (TIES) *take = remaining;
}
// the sampler's key functor: every entry of the row, by its order-preserving key
struct SmpRowKeys { const float* l; __device__ __forceinline__ bool operator()(int i, unsigned& k) const { k = smp_key(l[i]); return true; } };
// A sampled row's log-probabilities, AFTER the commit (the selection's code is then the LPM = 0 kernel's, instruction for instruction): the normaliser and top N over the
// FINAL kept set, keys in [lo, hi] -- not the sum top-p saw.  Thread 0's token / counter stores are visible to the block after the barrier.
template <int LPM, bool BAND>
__device__ __forceinline__ void lp_after_draw(const ArgmaxArgs& a, int b, int tid, const float* l, float ref, float inv_temp, unsigned lo, unsigned hi) {
  if constexpr (LPM > 0) {
    if (lp_row_on(a, b)) {
      __syncthreads();
      const int g = a.ngen_ptrs[b] ? *a.ngen_ptrs[b] - 1 : 0;
      const float lz = lp_row_pass<LPM, BAND>(a, b, l, ref, inv_temp, lo, g, hi);
      if (tid == 0) { const int tok = *a.tok_ptrs[b]; a.lp_lists[b][g] = tok >= 0 && tok < a.n ? (l[tok] - ref) * inv_temp - lz : -INFINITY; }
    }
  }
}
template <int LPM>
__global__ __launch_bounds__(1024) void sample_kernel(const ArgmaxArgs a) {
  __shared__ float shf[16];
  __shared__ int shi[16];
  __shared__ int hist[256];
  __shared__ unsigned s_sel[2];
  const int b = blockIdx.x, tid = threadIdx.x, n = a.n;
  const float* l = a.logits + (size_t)b * n;
  const float m = pick_row_max(l, n, tid, shf);
  unsigned kth = 0;                                                       // top-k: key of the k-th largest score (0: off, every key is kept)
  if (a.top_k > 0 && a.top_k < n) pick_radix_select<false>(tid, n, a.top_k, SmpRowKeys{l}, hist, s_sel, kth);
  // 3. normaliser of the kept scores
  float z = 0.f;
  for (int i = tid; i < n; i += 1024) { const float v = l[i]; if (smp_key(v) >= kth) z += expf((v - m) * a.inv_temp); }
  const float Z = smp_block_sum(z, shf);
  // 4. top-p: smallest key t such that the mass of keys > t is < top_p * Z (the maximum itself always qualifies: min_tokens_to_keep = 1)
  unsigned thr = kth;
  if (a.top_p > 0.f && a.top_p < 1.f) {
    const float target = a.top_p * Z;
    unsigned hi = smp_key(m), lo = kth;          // (declared in this order: the other one swaps two instructions of the <0> stream)
    while (lo < hi) {
      const unsigned mid = lo + ((hi - lo) >> 1);
      float s = 0.f;
      for (int i = tid; i < n; i += 1024) { const float v = l[i]; if (smp_key(v) > mid) s += expf((v - m) * a.inv_temp); }
      const float S = smp_block_sum(s, shf);
      if (S < target) hi = mid; else lo = mid + 1;
    }
    thr = lo;
  }
  // 5. Gumbel-max draw over the kept set
  const int step = a.ngen_ptrs[b] ? *a.ngen_ptrs[b] : (a.step_override ? a.step_override[b] : 0);          // falls back to step_override (lp_row_step does not)
  const unsigned k0 = smp_fmix32(a.seed_lo ^ 0x9e3779b9u), k1 = smp_fmix32(a.seed_hi ^ k0 ^ 0x85ebca77u);
  const unsigned kk = smp_fmix32(k1 ^ smp_fmix32(a.stream[b] * 0x9e3779b1u + 0x7f4a7c15u) ^ smp_fmix32((unsigned)step * 0x85ebca77u + 0x165667b1u));
  const unsigned kk2 = smp_fmix32(kk + 0x632be5abu);
  float best = -3.4e38f; int idx = 0x7fffffff;
  for (int i = tid; i < n; i += 1024) {
    const float v = l[i];
    if (smp_key(v) < thr) continue;
    const unsigned h = smp_fmix32(smp_fmix32((unsigned)i + kk) ^ kk2);
    const float u = ((float)(h >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float sc = (v - m) * a.inv_temp - logf(-logf(u));
    if (sc > best) { best = sc; idx = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(idx, o, 64);
    if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
  }
  __syncthreads();
  if ((tid & 63) == 0) { shf[tid >> 6] = best; shi[tid >> 6] = idx; }
  __syncthreads();
  if (tid == 0) for (int w = 1; w < 16; ++w) if (shf[w] > best || (shf[w] == best && shi[w] < idx)) { best = shf[w]; idx = shi[w]; }
  if (tid == 0) pick_commit(a, b, idx);          // (two statements: one block flips a branch of the <0> stream)
  lp_after_draw<LPM, false>(a, b, tid, l, m, a.inv_temp, thr, 0xffffffffu);
}
int gvl_launch_sample(const ArgmaxArgs& a, hipStream_t st) {
  if (a.batch < 1 || a.batch > GVL_MAX_DECODE_BATCH || !(a.inv_temp > 0.f) || a.top_k < 0 || a.top_p < 0.f) return -1;
  return launch_lp_mode(sample_kernel<0>, sample_kernel<1>, sample_kernel<2>, a, a, st);
}
// ---- per-row selection (SelRowsArgs): a decode group whose rows do not share one setting -- greedy rows next to sampled rows of different temperature / top-k / top-p /
// seed -- or whose setting uses HF's further warpers (MinP, Typical, Epsilon, Eta; transformers generation/logits_process.py [ext]).  One block per row, the row's
// parameters by value.  A greedy row is pick_greedy_row, a sampled row runs sample_kernel's stages up to top-p (same arithmetic, same reduction order: with the further warpers off
// the token and log-probabilities are bit-identical to those kernels'), then, with e_i = exp((s_i - ref) / T), ref = the largest kept score, Z = sum of e over the kept set:
//   min_p      keep e_i >= min_p                          (p_i >= min_p * p_max; p_max = 1 / Z)
//   typical_p  xbar = sum(e x) / Z, x = (s - ref) / T; d_i = |x_i - xbar| (= |-log p_i - H|: -log p_i = log Z - x_i, H = log Z - xbar); t = the smallest d with
//              mass{d_j <= t} >= typical_p * Z, by bisection on d's bit pattern (d >= 0: the bits order like the values); keep d_i <= t, ties at t included
//   epsilon    keep e_i >= eps * Z, and the largest kept score
//   eta        H = log Z - xbar over the current set, c = min(eta, sqrt(eta) exp(-H)); keep e_i >= c * Z, and the largest kept score
// Scores are monotone in p, so every stage leaves an INTERVAL [lo, hi] of keys (typical_p alone may lower hi: it can drop the maximum); a stage is one fixed-order
// sum pass plus one min / max pass over the keys that qualify.  min_tokens_to_keep = 1 throughout, as in sample_kernel.
__device__ __forceinline__ float smp_unkey(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }
// min of lo / max of hi over the block, in every thread (integers: the order of the reduction cannot matter)
__device__ __forceinline__ void smp_block_minmax(unsigned& lo, unsigned& hi, unsigned* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned ol = __shfl_xor(lo, o, 64), oh = __shfl_xor(hi, o, 64);
    lo = ol < lo ? ol : lo; hi = oh > hi ? oh : hi;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = lo; sh[16 + (threadIdx.x >> 6)] = hi; }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 16; ++w) { lo = sh[w] < lo ? sh[w] : lo; hi = sh[16 + w] > hi ? sh[16 + w] : hi; }
}
template <int LPM>
__global__ __launch_bounds__(1024) void select_rows_kernel(const SelRowsArgs sa) {
  __shared__ float shf[16];
  __shared__ int shi[16];
  __shared__ int hist[256];
  __shared__ unsigned s_sel[2];
  __shared__ unsigned shk[32];
  const ArgmaxArgs& a = sa.am;
  const int b = blockIdx.x, tid = threadIdx.x, n = a.n;
  const float* l = a.logits + (size_t)b * n;
  if (!sa.row[b].on) { pick_greedy_row<LPM>(a, b, tid, l, shf, shi, sa.kept); return; }       // block-uniform
  // ---- sampled row.  1 - 4 as in sample_kernel: row maximum and top-k (shared), normaliser and top-p bisection (its words)
  const float iT = sa.row[b].inv_temp;
  const int top_k = sa.row[b].top_k;
  const float top_p = sa.row[b].top_p;
  const float m = pick_row_max(l, n, tid, shf);
  unsigned kth = 0;
  if (top_k > 0 && top_k < n) pick_radix_select<false>(tid, n, top_k, SmpRowKeys{l}, hist, s_sel, kth);
  unsigned lo = kth, hi = smp_key(m);
  if (top_p > 0.f && top_p < 1.f) {          // the normaliser only when top-p is on (sample_kernel: always)
    float z = 0.f;
    for (int i = tid; i < n; i += 1024) { const float v = l[i]; if (smp_key(v) >= kth) z += expf((v - m) * iT); }
    const float Z = smp_block_sum(z, shf);
    const float target = top_p * Z;
    unsigned blo = kth, bhi = smp_key(m);
    while (blo < bhi) {
      const unsigned mid = blo + ((bhi - blo) >> 1);
      float s = 0.f;
      for (int i = tid; i < n; i += 1024) { const float v = l[i]; if (smp_key(v) > mid) s += expf((v - m) * iT); }
      const float S = smp_block_sum(s, shf);
      if (S < target) bhi = mid; else blo = mid + 1;
    }
    lo = blo;
  }
  // ---- the further warpers on the interval [lo, hi]; ref = the largest kept score (the row maximum until typical_p drops it)
  float ref = m;
  // Z = sum of e, S1 = sum of e * x over the current set, fixed order (-inf entries: e = 0, left out of S1)
  auto set_sums = [&](float& Z, float& S1) {
    float z = 0.f, s1 = 0.f;
    for (int i = tid; i < n; i += 1024) {
      const float v = l[i]; const unsigned k = smp_key(v);
      if (k < lo || k > hi) continue;
      const float x = (v - ref) * iT, e = expf(x);
      z += e; if (x > -INFINITY) s1 += e * x;
    }
    Z = smp_block_sum(z, shf); S1 = smp_block_sum(s1, shf);
  };
  // lo <- the smallest key of the current set with e >= cut (the largest kept score always stays)
  auto raise_lo = [&](float cut) {
    unsigned kl = hi, kh = 0u;
    for (int i = tid; i < n; i += 1024) {
      const float v = l[i]; const unsigned k = smp_key(v);
      if (k < lo || k > hi) continue;
      if (expf((v - ref) * iT) >= cut && k < kl) kl = k;
    }
    smp_block_minmax(kl, kh, shk);
    lo = kl;
  };
  const float min_p = sa.row[b].min_p, typ = sa.row[b].typical_p, eps = sa.row[b].eps, eta = sa.row[b].eta;
  if (min_p > 0.f) raise_lo(min_p);
  if (typ > 0.f && typ < 1.f) {
    float Z, S1; set_sums(Z, S1);
    const float xbar = S1 / Z, target = typ * Z;
    unsigned dl = 0u, dh = 0x7f800000u;
    while (dl < dh) {
      const unsigned mid = dl + ((dh - dl) >> 1);
      float s = 0.f;
      for (int i = tid; i < n; i += 1024) {
        const float v = l[i]; const unsigned k = smp_key(v);
        if (k < lo || k > hi) continue;
        const float x = (v - ref) * iT;
        if (__float_as_uint(fabsf(x - xbar)) <= mid) s += expf(x);
      }
      const float S = smp_block_sum(s, shf);
      if (S >= target) dh = mid; else dl = mid + 1;
    }
    unsigned kl = 0xffffffffu, kh = 0u;
    for (int i = tid; i < n; i += 1024) {
      const float v = l[i]; const unsigned k = smp_key(v);
      if (k < lo || k > hi) continue;
      if (__float_as_uint(fabsf((v - ref) * iT - xbar)) <= dl) { kl = k < kl ? k : kl; kh = k > kh ? k : kh; }
    }
    smp_block_minmax(kl, kh, shk);
    if (kl <= kh) { lo = kl; hi = kh; ref = smp_unkey(hi); }     // (an all-NaN band cannot empty the set)
  }
  if (eps > 0.f) { float Z, S1; set_sums(Z, S1); raise_lo(eps * Z); }
  if (eta > 0.f) {
    float Z, S1; set_sums(Z, S1);
    const float H = logf(Z) - S1 / Z;
    raise_lo(fminf(eta, sqrtf(eta) * expf(-H)) * Z);
  }
  // ---- Gumbel-max draw over [lo, hi]: sample_kernel's hash and score, the row's own seed and stream
  const int step = a.ngen_ptrs[b] ? *a.ngen_ptrs[b] : (a.step_override ? a.step_override[b] : 0);
  const unsigned k0 = smp_fmix32(sa.row[b].seed_lo ^ 0x9e3779b9u), k1 = smp_fmix32(sa.row[b].seed_hi ^ k0 ^ 0x85ebca77u);
  const unsigned kk = smp_fmix32(k1 ^ smp_fmix32(sa.row[b].stream * 0x9e3779b1u + 0x7f4a7c15u) ^ smp_fmix32((unsigned)step * 0x85ebca77u + 0x165667b1u));
  const unsigned kk2 = smp_fmix32(kk + 0x632be5abu);
  float best = -3.4e38f; int idx = 0x7fffffff;
  for (int i = tid; i < n; i += 1024) {
    const float v = l[i]; const unsigned k = smp_key(v);
    if (k < lo || k > hi) continue;
    const unsigned h = smp_fmix32(smp_fmix32((unsigned)i + kk) ^ kk2);
    const float u = ((float)(h >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float sc = (v - ref) * iT - logf(-logf(u));
    if (sc > best) { best = sc; idx = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(idx, o, 64);
    if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
  }
  __syncthreads();
  if ((tid & 63) == 0) { shf[tid >> 6] = best; shi[tid >> 6] = idx; }
  __syncthreads();
  if (sa.kept) for (int i = tid; i < n; i += 1024) { const float v = l[i]; const unsigned k = smp_key(v); sa.kept[(size_t)b * n + i] = k >= lo && k <= hi && fabsf(v) < INFINITY ? 1 : 0; }
  if (tid == 0) for (int w = 1; w < 16; ++w) if (shf[w] > best || (shf[w] == best && shi[w] < idx)) { best = shf[w]; idx = shi[w]; }
  if (tid == 0) pick_commit(a, b, idx);
  lp_after_draw<LPM, true>(a, b, tid, l, ref, iT, lo, hi);
}
int gvl_launch_select_rows(const SelRowsArgs& sa, hipStream_t st) {
  const ArgmaxArgs& a = sa.am;
  if (a.batch < 1 || a.batch > GVL_MAX_DECODE_BATCH) return -1;
  for (int b = 0; b < a.batch; ++b) {
    const SelRow& r = sa.row[b];
    if (r.on && (!(r.inv_temp > 0.f) || r.top_k < 0 || !(r.top_p >= 0.f) || !(r.min_p >= 0.f) || !(r.typical_p >= 0.f) || !(r.eps >= 0.f) || !(r.eta >= 0.f))) return -1;
  }
  return launch_lp_mode(select_rows_kernel<0>, select_rows_kernel<1>, select_rows_kernel<2>, a, sa, st);
}
// ---- beam search: the 2k candidates of one step (BeamCandArgs; HF _beam_search [ext]: log-softmax -> processors -> + beam score -> top-2k over the k x vocab grid).
// Two launches; the kernel boundary is the only hand-off between workgroups.
//   beam_rows_kernel<NORM>   one block per running beam.  NORM: the row holds raw logits; m = its maximum, lz = logf(sum exp(l - m)) summed strided per thread and
//                            finished with smp_block_sum -- the quantity lp_row_pass<1> computes, so lp = (l - m) - lz is bit for bit what greedy selection reports for
//                            the token.  !NORM: the row holds processed log-probabilities already (beam_normalize_kernel, then the logits processors).  The candidate
//                            value is t = lp + score[b], ONE fp32 add, and the selection runs on t, not on lp: distinct lp can collide after the add (at a score of
//                            -1e9 every entry does).  Order: the strict total order (t descending, index ascending) over ALL entries, -inf included.  The key of the
//                            2k-th largest t comes from pick_radix_select over smp_key(t), with its take / ties outputs; the entries above it are taken, and
//                            of the ties AT it the lowest indices -- when there are more ties than places a second radix select, over ~index among the ties, finds
//                            the last index taken.  The <= 32 survivors are ordered by counting in LDS and stored as (t, token, lp).
//   beam_merge_kernel        one wave: the best 2k of the k x 2k row survivors in the same order -- an entry's rank = the sum over the (sorted) rows of how many of
//                            their entries beat it, a binary search per row; flat index = beam * n + token.
//   beam_normalize_kernel    the NORM arithmetic alone, in place (when processors or token rules sit between the log-softmax and the beam scores): normalize followed by
//                            beam_rows_kernel<false> is bit-identical to beam_rows_kernel<true>.
// Keys, not float compares, order everything: every count is an integer and every store index is bounded whatever the row holds (NaN rows are outside the contract: their
// order is the keys', not IEEE's).  t + 0.0f folds -0.0 onto +0.0 before the key is taken, so the two compare equal as floats do.
__device__ __forceinline__ unsigned beam_key(float t) { return smp_key(t + 0.0f); }
template <bool NORM> __device__ __forceinline__ float beam_lp(float l, float m, float lz) { if constexpr (NORM) return __fsub_rn(__fsub_rn(l, m), lz); else return l; }
// row maximum and log of the normaliser, in every thread (pick_row_max, lp_row_pass's sum: fixed order, a pure function of the row)
__device__ __forceinline__ void beam_row_norm(const float* l, int n, int tid, float (&shf)[16], float& m, float& lz) {
  m = pick_row_max(l, n, tid, shf);
  float z = 0.f;
  for (int i = tid; i < n; i += 1024) z += expf((l[i] - m) * 1.0f);
  lz = logf(smp_block_sum(z, shf));
}
constexpr int GVL_BEAM_MAX_CAND = 2 * GVL_MAX_DECODE_BATCH;
template <bool NORM>
__global__ __launch_bounds__(1024) void beam_rows_kernel(const BeamCandArgs a) {
  __shared__ float shf[16];
  __shared__ int hist[256];
  __shared__ unsigned s_sel[3];
  __shared__ float c_t[GVL_BEAM_MAX_CAND], c_lp[GVL_BEAM_MAX_CAND];
  __shared__ int c_i[GVL_BEAM_MAX_CAND];
  __shared__ int s_cnt;
  const int b = blockIdx.x, tid = threadIdx.x, n = a.n, K2 = 2 * a.k;
  const float* l = a.rows + (size_t)b * (size_t)a.row_stride;
  const float sc = a.scores[b];
  float m = 0.f, lz = 0.f;
  if constexpr (NORM) beam_row_norm(l, n, tid, shf, m, lz);
  unsigned kth, ikey = 0; int take, ties;
  pick_radix_select<true>(tid, n, K2, [&](int i, unsigned& k) { k = beam_key(__fadd_rn(beam_lp<NORM>(l[i], m, lz), sc)); return true; }, hist, s_sel, kth, &take, &ties);
  if (ties > take) {                         // block-uniform: more entries at the 2k-th key than places -> the lowest indices among them
    int t2, n2;
    pick_radix_select<true>(tid, n, take, [&](int i, unsigned& k) { k = ~(unsigned)i; return beam_key(__fadd_rn(beam_lp<NORM>(l[i], m, lz), sc)) == kth; }, hist, s_sel, ikey, &t2, &n2);
  }
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 1024) {
    const float lp = beam_lp<NORM>(l[i], m, lz), t = __fadd_rn(lp, sc);
    const unsigned k = beam_key(t);
    if (k > kth || (k == kth && ~(unsigned)i >= ikey)) {
      const int s = atomicAdd(&s_cnt, 1);
      if (s < GVL_BEAM_MAX_CAND) { c_t[s] = t; c_lp[s] = lp; c_i[s] = i; }
    }
  }
  __syncthreads();
  const int cnt = s_cnt < K2 ? s_cnt : K2;   // == K2: integer counts
  if (tid < cnt) {
    const unsigned mk = beam_key(c_t[tid]); const int mi = c_i[tid];
    int rank = 0;
    for (int j = 0; j < cnt; ++j) { const unsigned kj = beam_key(c_t[j]); rank += (kj > mk || (kj == mk && c_i[j] < mi)) ? 1 : 0; }
    const size_t o = (size_t)b * K2 + rank;
    a.row_v[o] = c_t[tid]; a.row_i[o] = mi; a.row_lp[o] = c_lp[tid];
  }
}
// the merge of one wave, shared by beam_merge_kernel and beam_group_merge_kernel; sorted (null or LDS [2k]): the merged flat indices, rank by rank, for the caller
__device__ __forceinline__ void beam_merge_wave(const BeamCandArgs& a, unsigned (&mk)[GVL_MAX_DECODE_BATCH * GVL_BEAM_MAX_CAND], int (&mi)[GVL_MAX_DECODE_BATCH * GVL_BEAM_MAX_CAND],
                                                int* sorted) {
  const int lane = threadIdx.x, K2 = 2 * a.k, total = a.k * K2;
  for (int e = lane; e < total; e += 64) { mk[e] = beam_key(a.row_v[e]); mi[e] = (e / K2) * a.n + a.row_i[e]; }
  __syncthreads();
  for (int e = lane; e < total; e += 64) {
    const unsigned ke = mk[e]; const int ie = mi[e];
    int rank = 0;
    for (int r = 0; r < a.k; ++r) {          // a row's survivors are sorted in this very order: those better than e are a prefix of the row -> binary search
      const int base = r * K2;
      int lo = 0, hi = K2;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (mk[base + mid] > ke || (mk[base + mid] == ke && mi[base + mid] < ie)) lo = mid + 1; else hi = mid;
      }
      rank += lo;
    }
    if (rank < K2) { a.vals[rank] = a.row_v[e]; a.idx[rank] = ie; a.proc[rank] = a.row_lp[e]; if (sorted) sorted[rank] = ie; }
  }
}
__global__ __launch_bounds__(64) void beam_merge_kernel(const BeamCandArgs a) {
  __shared__ unsigned mk[GVL_MAX_DECODE_BATCH * GVL_BEAM_MAX_CAND];
  __shared__ int mi[GVL_MAX_DECODE_BATCH * GVL_BEAM_MAX_CAND];
  beam_merge_wave(a, mk, mi, nullptr);
}
// One group of diverse beam search (BeamGroupArgs): the merge over the group's s rows, then the group's CHOICE as HF's BeamSearchScorer.process makes it -- the tokens of the
// first s candidates, in candidate order, that are not eos -- written to `current` for the next group's Hamming stage (logits_process_hamming_kernel, the next launch on the
// stream) and to the host's mirror.  Lane j finds the j-th non-eos candidate by counting the non-eos candidates in front of each rank: integer counts over <= 32 LDS
// entries.  A done group has no candidates: its s entries are the pad id.  Every index is bounded by s <= 16 and 2s <= 32 whatever the rows hold.
__global__ __launch_bounds__(64) void beam_group_merge_kernel(const BeamGroupArgs g) {
  __shared__ unsigned mk[GVL_MAX_DECODE_BATCH * GVL_BEAM_MAX_CAND];
  __shared__ int mi[GVL_MAX_DECODE_BATCH * GVL_BEAM_MAX_CAND];
  __shared__ int sorted[GVL_BEAM_MAX_CAND];
  const int lane = threadIdx.x, s = g.c.k, K2 = 2 * s;
  if (g.done) {
    if (lane < s) { const int t = g.pad < 0 ? -1 : g.pad; g.current[lane] = t; if (g.mirror) g.mirror[lane] = t; }
    return;
  }
  if (lane < K2) sorted[lane] = -1;
  __syncthreads();
  beam_merge_wave(g.c, mk, mi, sorted);
  __syncthreads();
  if (lane < s) { g.current[lane] = -1; if (g.mirror) g.mirror[lane] = -1; }
  __syncthreads();
  if (lane < K2 && sorted[lane] >= 0) {
    const int tok = sorted[lane] % g.c.n;
    if (tok != g.eos) {
      int before = 0;
      for (int r = 0; r < lane; ++r) before += (sorted[r] >= 0 && sorted[r] % g.c.n != g.eos) ? 1 : 0;
      if (before < s) { g.current[before] = tok; if (g.mirror) g.mirror[before] = tok; }
    }
  }
}
__global__ __launch_bounds__(1024) void beam_normalize_kernel(float* rows, int n) {
  __shared__ float shf[16];
  float* l = rows + (size_t)blockIdx.x * n;
  float m, lz;
  beam_row_norm(l, n, threadIdx.x, shf, m, lz);           // every thread has read the entries it is about to overwrite, and the block sum is behind its barriers
  for (int i = threadIdx.x; i < n; i += 1024) l[i] = beam_lp<true>(l[i], m, lz);
}
static bool beam_shape_ok(int n, int k) { return k >= 2 && k <= GVL_MAX_DECODE_BATCH && n >= 2 * k && (long long)n * k <= 0x7fffffffLL; }
int gvl_launch_beam_candidates(const BeamCandArgs& a, hipStream_t st) {
  if (!beam_shape_ok(a.n, a.k) || !a.rows || a.row_stride < 0 || !a.row_v || !a.row_i || !a.row_lp || !a.vals || !a.idx || !a.proc) return -1;
  if (a.norm) hipLaunchKernelGGL(beam_rows_kernel<true>, dim3(a.k), dim3(1024), 0, st, a);
  else hipLaunchKernelGGL(beam_rows_kernel<false>, dim3(a.k), dim3(1024), 0, st, a);
  hipLaunchKernelGGL(beam_merge_kernel, dim3(1), dim3(64), 0, st, a);
  return CHECK_LAUNCH();
}
int gvl_launch_beam_group(const BeamGroupArgs& g, hipStream_t st) {
  const BeamCandArgs& a = g.c;
  if (a.k < 1 || a.k > GVL_MAX_DECODE_BATCH || !g.current) return -1;
  if (!g.done) {
    if (a.n < 2 * a.k || (long long)a.n * a.k > 0x7fffffffLL || !a.rows || a.row_stride < 0 || !a.row_v || !a.row_i || !a.row_lp || !a.vals || !a.idx || !a.proc) return -1;
    if (a.norm) hipLaunchKernelGGL(beam_rows_kernel<true>, dim3(a.k), dim3(1024), 0, st, a);
    else hipLaunchKernelGGL(beam_rows_kernel<false>, dim3(a.k), dim3(1024), 0, st, a);
  }
  hipLaunchKernelGGL(beam_group_merge_kernel, dim3(1), dim3(64), 0, st, g);
  return CHECK_LAUNCH();
}
int gvl_launch_beam_normalize(float* rows, int n, int k, hipStream_t st) {
  if (!rows || n < 1 || k < 1 || k > GVL_MAX_DECODE_BATCH) return -1;
  hipLaunchKernelGGL(beam_normalize_kernel, dim3(k), dim3(1024), 0, st, rows, n);
  return CHECK_LAUNCH();
}
// ---- classifier-free guidance against a negative sequence (GuidanceArgs / FollowArgs; HF UnbatchedClassifierFreeGuidanceLogitsProcessor [ext]: the FIRST processor, so
// it runs in front of gvl_launch_logits_process and the selection, which then see the guided row where they saw the raw one).
//   guidance_rows_kernel   one block per PAIR: cond[p] <- scale * (log_softmax(cond[p]) - log_softmax(neg[p])) + log_softmax(neg[p]), the negative row only read.  Per row
//                          m and lz are beam_row_norm's (pick_row_max, the strided sum, smp_block_sum, logf) and lc / lu are beam_lp<true>'s two subtractions, so each is bit
//                          for bit what beam_normalize_kernel leaves; then ONE fp32 subtract, ONE multiply, ONE add, each rounded (no FMA contraction: the exact test compares
//                          against three separate device ops).  A pair's result is a pure function of its two rows and its scale.  Rows are finite by contract (gvl.h).
//   follow_commit_kernel   after the selection, one thread per follower: the leader's just-selected token into the follower's token word and output list, its generation
//                          count and position bumped -- pick_commit's stores for a row nobody selected for.  Not part of pick_commit or the selection kernels: their
//                          instruction streams are pinned (profiles/pick_refactor_asm.txt), and a group without pairs launches neither kernel.
__global__ __launch_bounds__(1024) void guidance_rows_kernel(const GuidanceArgs a) {
  __shared__ float shf[16];
  const int p = blockIdx.x, tid = threadIdx.x, n = a.n;
  float* c = a.cond[p]; const float* u = a.neg[p];
  float mc, zc, mu, zu;
  beam_row_norm(c, n, tid, shf, mc, zc);
  __syncthreads();                          // every thread has read the first row's wave sums before the second row's maxima overwrite them
  beam_row_norm(u, n, tid, shf, mu, zu);
  const float s = a.scale[p];
  for (int i = tid; i < n; i += 1024) {     // every thread has read the entries it is about to overwrite (beam_normalize_kernel's argument)
    // __fadd_rn(__fmul_rn(s, __fsub_rn(lc, lu)), lu) in plain operators with contraction OFF for this block: the _rn wrappers are ordinary operators compiled where
    // they are defined, contraction allowed, and the multiply and the add then fuse into one FMA -- one rounding instead of two, 1 ulp off the three separate ops
#pragma clang fp contract(off)
    const float lc = beam_lp<true>(c[i], mc, zc), lu = beam_lp<true>(u[i], mu, zu);
    const float d = lc - lu;
    const float t = s * d;
    c[i] = t + lu;
  }
}
int gvl_launch_guidance_rows(const GuidanceArgs& a, hipStream_t st) {
  if (a.n < 1 || a.n_pairs < 1 || a.n_pairs > GVL_MAX_GUIDANCE_PAIRS) return -1;
  for (int p = 0; p < a.n_pairs; ++p) if (!a.cond[p] || !a.neg[p] || !(fabsf(a.scale[p]) < INFINITY)) return -1;
  hipLaunchKernelGGL(guidance_rows_kernel, dim3(a.n_pairs), dim3(1024), 0, st, a);
  return CHECK_LAUNCH();
}
__global__ __launch_bounds__(64) void follow_commit_kernel(const FollowArgs a) {
  const int p = threadIdx.x;
  if (p >= a.n) return;
  const int t = *a.lead_tok[p];
  *a.tok[p] = t;
  const int g = *a.ngen[p]; a.out[p][g] = t; *a.ngen[p] = g + 1;
  if (a.pos[p]) (*a.pos[p])++;
}
int gvl_launch_follow_commit(const FollowArgs& a, hipStream_t st) {
  if (a.n < 1 || a.n > GVL_MAX_GUIDANCE_PAIRS) return -1;
  for (int p = 0; p < a.n; ++p) if (!a.lead_tok[p] || !a.tok[p] || !a.out[p] || !a.ngen[p]) return -1;
  hipLaunchKernelGGL(follow_commit_kernel, dim3(1), dim3(64), 0, st, a);
  return CHECK_LAUNCH();
}
// ---- teacher-forced scoring (ScoreRowsArgs; gvl_score_extend_varlen's tail and gvl_op_score_rows): what the raw distribution of a row says about a GIVEN id.  One block
// per row of fp32 logits, any number of rows.  Per row, with t the target, m the row maximum and lz = logf(sum exp(s - m)):
//   lp    (s_t - m) - lz.  m is pick_row_max's, the sum is strided per thread and finished by smp_block_sum -- lp_row_pass<1>'s order at thr = 0, inv_temp = 1 (beam_row_norm's
//         too) -- so lp is bit for bit what greedy selection reports for the row when t is its argmax (s_t - m = 0), and the top list's entry for t when t is listed.
//   rank  how many entries beat t in the strict order (value descending, lower id first): an integer count over keys (beam_key: -0.0 folded onto +0.0, as float compares see
//         them) and indices, over ALL entries, -inf included.  0: t is the greedy choice.  A target at -inf gets lp = -inf and its rank by the same order.
//   top   TOP only: the best top_n finite entries as (id, log-probability), padded with (-1, -inf): lp_insert per thread, lp_wave_merge per wave and across the waves -- argmax_kernel<2>'s lists.  The
//         merge-and-store is WRITTEN OUT below in lp_row_pass's words: as a function shared with lp_row_pass it changed the instruction streams of argmax_kernel<2>,
//         sample_kernel<2> and select_rows_kernel<2> (profiles/score_rows_asm.txt), the rule the sampled row's stages already live by (file header).
// A target outside [0, n) never indexes the row: lp = -inf, rank = -1 (the entry points refuse such a target on the host where they see it).  Every barrier is reached by
// the whole block: TOP is a template parameter and nothing else guards one.
template <bool TOP>
__global__ __launch_bounds__(1024) void score_rows_kernel(const ScoreRowsArgs a) {
  __shared__ float shf[16];
  __shared__ int shc[16];
  const int b = blockIdx.x, tid = threadIdx.x, n = a.n;
  const float* l = a.logits + (size_t)b * (size_t)a.ld;
  const int t = a.targets[b];
  const bool in = t >= 0 && t < n;
  const float st = in ? l[t] : -INFINITY;
  const unsigned kt = beam_key(st);
  const float m = pick_row_max(l, n, tid, shf);
  [[maybe_unused]] float tv[GVL_MAX_TOP_LOGPROBS]; [[maybe_unused]] int ti[GVL_MAX_TOP_LOGPROBS];
  if constexpr (TOP) {
#pragma unroll
    for (int j = 0; j < GVL_MAX_TOP_LOGPROBS; ++j) { tv[j] = -INFINITY; ti[j] = -1; }
  }
  float z = 0.f; int c = 0;
  for (int i = tid; i < n; i += 1024) {
    const float v = l[i];
    z += expf((v - m) * 1.0f);
    const unsigned k = beam_key(v);
    c += (k > kt || (k == kt && i < t)) ? 1 : 0;
    if constexpr (TOP) if (fabsf(v) < INFINITY) lp_insert(tv, ti, v, i);
  }
  const float lz = logf(smp_block_sum(z, shf));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);          // integers: the order of the reduction cannot matter
  if ((tid & 63) == 0) shc[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    int r = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) r += shc[w];
    a.lp[b] = in ? __fsub_rn(__fsub_rn(st, m), lz) : -INFINITY;
    a.rank[b] = in ? r : -1;
  }
  if constexpr (TOP) {          // lp_row_pass<2>'s merge and store, in its words
    __shared__ float s_tv[16 * GVL_MAX_TOP_LOGPROBS];
    __shared__ int s_ti[16 * GVL_MAX_TOP_LOGPROBS];
    float wv[GVL_MAX_TOP_LOGPROBS]; int wi[GVL_MAX_TOP_LOGPROBS];
    lp_wave_merge(tv, ti, wv, wi);
    if ((tid & 63) == 0) {
#pragma unroll
      for (int r = 0; r < GVL_MAX_TOP_LOGPROBS; ++r) { s_tv[(tid >> 6) * GVL_MAX_TOP_LOGPROBS + r] = wv[r]; s_ti[(tid >> 6) * GVL_MAX_TOP_LOGPROBS + r] = wi[r]; }
    }
    __syncthreads();
    if (tid < 64) {
      const int lane = tid;
#pragma unroll
      for (int j = 0; j < GVL_MAX_TOP_LOGPROBS; ++j) {
        tv[j] = lane < 16 ? s_tv[lane * GVL_MAX_TOP_LOGPROBS + j] : -INFINITY; ti[j] = lane < 16 ? s_ti[lane * GVL_MAX_TOP_LOGPROBS + j] : -1;
      }
      lp_wave_merge(tv, ti, wv, wi);
      float v = -INFINITY; int id = -1;
#pragma unroll
      for (int r = 0; r < GVL_MAX_TOP_LOGPROBS; ++r) if (lane == r) { v = wv[r]; id = wi[r]; }
      if (lane < GVL_MAX_TOP_LOGPROBS) {
        const bool ok = lane < a.top_n && id >= 0;
        a.top_ids[(size_t)b * GVL_MAX_TOP_LOGPROBS + lane] = ok ? id : -1;
        a.top_lp[(size_t)b * GVL_MAX_TOP_LOGPROBS + lane] = ok ? (v - m) * 1.0f - lz : -INFINITY;
      }
    }
  }
}
int gvl_launch_score_rows(const ScoreRowsArgs& a, hipStream_t st) {
  if (!a.logits || !a.targets || !a.lp || !a.rank || a.n < 1 || a.ld < a.n || a.rows < 0 || a.top_n < 0 || a.top_n > GVL_MAX_TOP_LOGPROBS ||
      (a.top_n > 0 && (!a.top_ids || !a.top_lp))) return -1;
  if (a.rows == 0) return 0;
  if (a.top_n > 0) hipLaunchKernelGGL(score_rows_kernel<true>, dim3(a.rows), dim3(1024), 0, st, a);
  else hipLaunchKernelGGL(score_rows_kernel<false>, dim3(a.rows), dim3(1024), 0, st, a);
  return CHECK_LAUNCH();
}
// The lm_head columns the GEMM leaves to the score tail: gvl_launch_gemm's contract is N % 4 == 0 and its whole-row epilogue wants N % 16 == 0, the fine-tuned vocabularies
// are 32 366 and 128 558.  out[r][c0 + j] = sum_k x[r][k] * W[c0 + j][k] (+ bias[c0 + j]) for r < rows, j < nc: one wave per (row, column), bf16 operands, fp32
// accumulation in a fixed order (strided per lane, then the butterfly) -- a pure function of the row, like the GEMM's columns beside it.
__global__ __launch_bounds__(64) void head_cols_kernel(const bf16_t* x, int ldx, const bf16_t* W, int K, const float* bias, float* out, int ld, int c0, int nc) {
  const int r = blockIdx.x / nc, c = c0 + blockIdx.x % nc, lane = threadIdx.x;
  const bf16_t* xr = x + (size_t)r * ldx; const bf16_t* wc = W + (size_t)c * K;
  float acc = 0.f;
  for (int k = lane; k < K; k += 64) acc += bf2f(xr[k]) * bf2f(wc[k]);
  acc = wave_sum(acc);
  if (lane == 0) out[(size_t)r * ld + c] = bias ? acc + bias[c] : acc;
}
int gvl_launch_head_cols(const bf16_t* x, int ldx, const bf16_t* W, int K, const float* bias, float* out, int ld, int c0, int nc, int rows, hipStream_t st) {
  if (!x || !W || !out || K < 1 || ldx < K || c0 < 0 || nc < 1 || ld < c0 + nc || rows < 1) return -1;
  hipLaunchKernelGGL(head_cols_kernel, dim3(rows * nc), dim3(64), 0, st, x, ldx, W, K, bias, out, ld, c0, nc);
  return CHECK_LAUNCH();
}
