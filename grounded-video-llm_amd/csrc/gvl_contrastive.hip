// gvl_contrastive.hip -- contrastive search behind the C ABI (include/gvl.h): gvl_contrastive_search = HF generate(penalty_alpha > 0, top_k > 1) (transformers 4.40.1
// GenerationMixin._contrastive_search / _ranking_fast [ext], restated in tests/contrastive_ref.py) inside the library, the hidden bank it ranks against
// (gvl_seq_keep_hidden / gvl_seq_read_hidden) and the operator-level entries of its two kernels.  The bookkeeping is gvl_contrastive.h (host-only, CPU-tested); the top-k
// of the probabilities are gvl_beam_search's candidate launches (gvl_pick.hip: the fixed-order log-softmax, ties to the lower id); the candidates advance through
// the SearchSession (gvl_search.hip: the clones of the caller's sequence, the processor launch, the teacher-forced step).
//   hidden_bank_append_kernel   residual rows -> final RMSNorm (rmsnorm_bf16_kernel's arithmetic, statement for statement: bit-identical rows) -> bf16 bank row + its
//                               inverse norm 1 / sqrtf(sum h^2) over the ROUNDED row, one wave per row
//   contrastive_rank_kernel     every context row against the k candidate rows in LDS: the bank is read once, 16 bytes per lane.  Eight lanes share a row: lane l takes
//                               the 8-element chunks l, l + 8, l + 16, ... in order, one fma per element in index order (the product of two bf16 values is exact in
//                               fp32, so an fma is product-then-add with one rounding), then the xor butterfly 4, 2, 1 -- an order that depends on D only.
//                               cos = (dot * inv_row) * inv_cand; the running maxima leave per block
//   contrastive_finish_kernel   the maximum over the blocks (order-free), score = fmaf(-alpha, pen, (1 - alpha) * p), the arg-max with ties to the lower rank, and the
//                               winner's row committed behind the bank
#include "gvl_model.h"
#include "gvl_contrastive.h"

using namespace gvlm;

namespace {

constexpr int kRankThreads = 256, kRankMaxBlocks = 1024, kPartStride = GVL_MAX_DECODE_BATCH;

template <int MAXV>  // MAXV 16-byte vectors per lane: cols <= MAXV * 512
__global__ __launch_bounds__(256) void hidden_bank_append_kernel(const bf16_t* __restrict__ x, int ldx, const bf16_t* __restrict__ w, bf16_t* __restrict__ y,
                                                                 float* __restrict__ inv, int rows, int cols, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const bf16_t* xr = x + (size_t)row * ldx;
  u32x4_t v[MAXV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = (lane + 64 * i) * 8;
    if (c < cols) {
      v[i] = *(const u32x4_t*)(xr + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float a = lo_bf(v[i][e]), bb = hi_bf(v[i][e]); s += a * a + bb * bb; }
    }
  }
  const float rs = rsqrtf(wave_sum(s) / cols + eps);
  float s2 = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = (lane + 64 * i) * 8;
    if (c < cols) {
      const u32x4_t wv = *(const u32x4_t*)(w + c);
      u32x4_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {   // weight * bf16(x * rsqrt), both factors bf16, product rounded to bf16; then the squares of what was stored
        o[e] = pack2bf(lo_bf(wv[e]) * rbf(lo_bf(v[i][e]) * rs), hi_bf(wv[e]) * rbf(hi_bf(v[i][e]) * rs));
        const float a = lo_bf(o[e]), bb = hi_bf(o[e]);
        s2 = __builtin_fmaf(a, a, s2); s2 = __builtin_fmaf(bb, bb, s2);
      }
      *(u32x4_t*)(y + (size_t)row * cols + c) = o;
    }
  }
  s2 = wave_sum(s2);
  if (lane == 0) inv[row] = 1.0f / sqrtf(s2);
}

struct RankArgs {
  const bf16_t* bank; const float* bank_inv; int n_ctx, D, k;
  const bf16_t* cand; const float* cand_inv;
  const float* p; int p_is_logprob; float alpha;
  float* part; int blocks;                 // [blocks][16] maxima of the blocks' rows
  float *pen, *score, *p_out; int* sel;    // [k], [k], [k] (p_out may be null), [1]
  bf16_t* commit_row; float* commit_inv;   // null, or where the winner's row and inverse norm go
};

template <int KP>  // candidates padded to KP rows of zeros: a candidate's sums never see its neighbours
__global__ __launch_bounds__(kRankThreads) void contrastive_rank_kernel(const RankArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* cs = (bf16_t*)smem;                                  // [KP][D]
  __shared__ float wmax[kRankThreads / 64][GVL_MAX_DECODE_BATCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, D = a.D, nchunk = D >> 3;
  for (int e = tid; e < KP * nchunk; e += kRankThreads) {
    const int i = e / nchunk;
    u32x4_t v = {0u, 0u, 0u, 0u};
    if (i < a.k) v = *(const u32x4_t*)(a.cand + (size_t)e * 8);
    *(u32x4_t*)(cs + (size_t)e * 8) = v;
  }
  float cinv[KP], m[KP];
#pragma unroll
  for (int i = 0; i < KP; ++i) { cinv[i] = i < a.k ? a.cand_inv[i] : 0.f; m[i] = -INFINITY; }
  __syncthreads();
  const int sub = lane >> 3, l = lane & 7, per = D >> 6;       // per: chunks of one lane
  const int octets = (a.n_ctx + 7) >> 3;
  for (int o = blockIdx.x * (kRankThreads / 64) + wave; o < octets; o += gridDim.x * (kRankThreads / 64)) {
    const int row = o * 8 + sub;
    const bool live = row < a.n_ctx;
    const bf16_t* br = a.bank + (size_t)(live ? row : a.n_ctx - 1) * D;   // a dead sub-group re-reads the last row and drops the result
    float acc[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) acc[i] = 0.f;
#pragma unroll 4
    for (int c = 0; c < per; ++c) {
      const int ch = l + 8 * c;
      const u32x4_t bv = *(const u32x4_t*)(br + ch * 8);
      float b[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) { b[2 * e] = lo_bf(bv[e]); b[2 * e + 1] = hi_bf(bv[e]); }
#pragma unroll
      for (int i = 0; i < KP; ++i) {
        const u32x4_t cv = *(const u32x4_t*)(cs + (size_t)i * D + ch * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[i] = __builtin_fmaf(b[2 * e], lo_bf(cv[e]), acc[i]);
          acc[i] = __builtin_fmaf(b[2 * e + 1], hi_bf(cv[e]), acc[i]);
        }
      }
    }
    const float rinv = a.bank_inv[live ? row : a.n_ctx - 1];
#pragma unroll
    for (int i = 0; i < KP; ++i) {
      float d = acc[i];
      d += __shfl_xor(d, 4, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 1, 64);
      const float cosv = __fmul_rn(__fmul_rn(d, rinv), cinv[i]);
      if (live) m[i] = fmaxf(m[i], cosv);
    }
  }
#pragma unroll
  for (int i = 0; i < KP; ++i) { const float r = wave_max(m[i]); if (lane == 0) wmax[wave][i] = r; }
  __syncthreads();
  if (tid < KP) {
    float r = wmax[0][tid];
    for (int q = 1; q < kRankThreads / 64; ++q) r = fmaxf(r, wmax[q][tid]);
    a.part[(size_t)blockIdx.x * kPartStride + tid] = r;
  }
}

__global__ __launch_bounds__(64) void contrastive_finish_kernel(const RankArgs a) {
  __shared__ float sc[GVL_MAX_DECODE_BATCH];
  __shared__ int s_sel;
  const int lane = threadIdx.x;
  if (lane < a.k) {
    float pen = -INFINITY;
    for (int b = 0; b < a.blocks; ++b) pen = fmaxf(pen, a.part[(size_t)b * kPartStride + lane]);
    const float p = a.p_is_logprob ? expf(a.p[lane]) : a.p[lane];
    float s = __builtin_fmaf(-a.alpha, pen, __fmul_rn(__fsub_rn(1.0f, a.alpha), p));
    if (a.p_is_logprob && a.p[lane] == -INFINITY) s = -INFINITY;   // a masked id (grammar, bad words) fills a place when fewer than k ids are allowed: it is never chosen
    a.pen[lane] = pen; a.score[lane] = s; if (a.p_out) a.p_out[lane] = p;
    sc[lane] = s;
  }
  __syncthreads();
  if (lane == 0) {
    int best = 0;
    for (int i = 1; i < a.k; ++i) if (sc[i] > sc[best]) best = i;   // strictly greater: ties go to the lower rank
    *a.sel = best; s_sel = best;
  }
  __syncthreads();
  if (a.commit_row) {
    const int w = s_sel;
    for (int e = lane; e < (a.D >> 3); e += 64) *(u32x4_t*)(a.commit_row + (size_t)e * 8) = *(const u32x4_t*)(a.cand + (size_t)w * a.D + (size_t)e * 8);
    if (lane == 0 && a.commit_inv) *a.commit_inv = a.cand_inv[w];
  }
}

// the candidates' ids -> the input tokens of their sequences, on the stream: the host does not wait for the candidate launch before it enqueues the step
struct FeedArgs { const int* idx; int* tok[GVL_MAX_DECODE_BATCH]; int k; };
__global__ void contrastive_feed_kernel(const FeedArgs a) { if ((int)threadIdx.x < a.k) *a.tok[threadIdx.x] = a.idx[threadIdx.x]; }

int launch_hidden_append(const bf16_t* x, int ldx, const bf16_t* w, float eps, bf16_t* y, float* inv, int n, int cols, hipStream_t st) {
  if (n < 1 || cols % 64 || cols < 64 || cols > 8192 || ldx < cols || ldx % 8) return -1;
  dim3 g((n + 3) / 4), t(256);
  if (cols <= 2048) hipLaunchKernelGGL(hidden_bank_append_kernel<4>, g, t, 0, st, x, ldx, w, y, inv, n, cols, eps);
  else hipLaunchKernelGGL(hidden_bank_append_kernel<16>, g, t, 0, st, x, ldx, w, y, inv, n, cols, eps);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

GvlDevOnce g_rank_lds[3];
template <int KP> int launch_rank_kp(RankArgs a, int slot, hipStream_t st) {
  const int lds = KP * a.D * 2;
  if (lds > gvl_contrastive::kRankLdsBytes) return -1;
  if (lds > 48 * 1024) { if (const int rc = gvl_set_max_lds(g_rank_lds[slot], (const void*)contrastive_rank_kernel<KP>, 128 * 1024)) return rc; }   // set once per device: the largest
  hipLaunchKernelGGL(contrastive_rank_kernel<KP>, dim3(a.blocks), dim3(kRankThreads), lds, st, a);
  return 0;
}
// part: room for kRankMaxBlocks x 16 floats
int launch_rank(RankArgs a, hipStream_t st) {
  if (a.k < 2 || a.k > GVL_MAX_DECODE_BATCH || a.n_ctx < 1 || a.D % 64 || a.D < 64 || a.D > 8192 || !(a.alpha >= 0.f && a.alpha <= 1.f)) return -1;
  if (!a.bank || !a.bank_inv || !a.cand || !a.cand_inv || !a.p || !a.part || !a.pen || !a.score || !a.sel) return -1;
  const int octets = (a.n_ctx + 7) / 8, per_block = kRankThreads / 64;
  a.blocks = std::min(kRankMaxBlocks, (octets + per_block - 1) / per_block);
  int rc;
  switch (gvl_contrastive::rank_rows(a.k)) {
    case 4: rc = launch_rank_kp<4>(a, 0, st); break;
    case 8: rc = launch_rank_kp<8>(a, 1, st); break;
    default: rc = launch_rank_kp<16>(a, 2, st);
  }
  if (rc) return rc;
  hipLaunchKernelGGL(contrastive_finish_kernel, dim3(1), dim3(64), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// scratch of a step: [16][hidden] candidate rows, [16] inverse norms, the blocks' maxima (device); p / pen / score [16] each and the selected rank (host-mapped)
struct CsBufs { bf16_t* cand; float* cand_inv; float* part; float *h_p, *h_pen, *h_score; int* h_sel; float *d_p, *d_pen, *d_score; int* d_sel; };
int cs_buffers(gvl_ctx* ctx, CsBufs* b) {
  const size_t rows = al256((size_t)GVL_MAX_DECODE_BATCH * ctx->cfg.hidden * 2);
  if (!ctx->d_cs_scratch) HIPCHK(ctx, hipMalloc(&ctx->d_cs_scratch, rows + 256 + (size_t)kRankMaxBlocks * kPartStride * 4));
  if (!ctx->h_cs_out) {
    HIPCHK(ctx, hipHostMalloc(&ctx->h_cs_out, 4 * GVL_MAX_DECODE_BATCH * 4, hipHostMallocMapped));
    memset(ctx->h_cs_out, 0, 4 * GVL_MAX_DECODE_BATCH * 4);
    HIPCHK(ctx, hipHostGetDevicePointer(&ctx->d_cs_out, ctx->h_cs_out, 0));
  }
  b->cand = (bf16_t*)ctx->d_cs_scratch; b->cand_inv = (float*)((char*)ctx->d_cs_scratch + rows); b->part = (float*)((char*)ctx->d_cs_scratch + rows + 256);
  float* h = (float*)ctx->h_cs_out; float* d = (float*)ctx->d_cs_out;
  b->h_p = h; b->h_pen = h + 16; b->h_score = h + 32; b->h_sel = (int*)(h + 48);
  b->d_p = d; b->d_pen = d + 16; b->d_score = d + 32; b->d_sel = (int*)(d + 48);
  return 0;
}

}  // namespace

int gvlm::bank_append(gvl_ctx* ctx, Seq& s, const bf16_t* x, int ldx, int n, hipStream_t st) {
  if (!s.bank || s.bank_rows + n > s.bank_cap) return fail(ctx, GVL_ERR_STATE, "hidden bank: no room for the new rows");
  const int Hd = ctx->cfg.hidden;
  RUN(GVL_PROF_OTHER, 0, launch_hidden_append(x, ldx, ctx->l_norm, ctx->cfg.rms_eps, s.bank + (size_t)s.bank_rows * Hd, s.bank_inv + s.bank_rows, n, Hd, st));
  s.bank_rows += n;
  return 0;
}

extern "C" {

int gvl_seq_keep_hidden(gvl_ctx* ctx, int seq_id, int on) {
  REQUIRE_READY(ctx->has_llm, "gvl_seq_keep_hidden");
  Seq* s = ctx->lookup(seq_id);
  if (!s) return seq_fail(ctx, "gvl_seq_keep_hidden", SEQ_BAD);
  if (const int rc = pair_refuse(ctx, "gvl_seq_keep_hidden", seq_id, true)) return rc;
  if (!on) { ctx->drop_bank(*s); return 0; }
  if (s->pos != 0) return fail(ctx, GVL_ERR_STATE, "gvl_seq_keep_hidden: the sequence already holds tokens (call it before the prefill)");
  return bank_alloc(ctx, *s, s->max_tokens);
}

int gvl_seq_read_hidden(gvl_ctx* ctx, int seq_id, int first, int n, uint16_t* rows_dev, float* inv_dev, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_seq_read_hidden");
  Seq* s = ctx->lookup(seq_id);
  if (!s) return seq_fail(ctx, "gvl_seq_read_hidden", SEQ_BAD);
  if (!s->bank) return fail(ctx, GVL_ERR_STATE, "gvl_seq_read_hidden: the sequence keeps no hidden states (gvl_seq_keep_hidden)");
  if (first < 0 || n < 1 || first + n > s->bank_rows) return fail(ctx, GVL_ERR_ARG, "gvl_seq_read_hidden: rows [first, first + n) must lie within the " + std::to_string(s->bank_rows) + " rows written");
  hipStream_t st = (hipStream_t)stream;
  const int Hd = ctx->cfg.hidden;
  if (rows_dev) RUN(GVL_PROF_OTHER, 0, gvl_launch_copy_bytes(s->bank + (size_t)first * Hd, rows_dev, (size_t)n * Hd * 2, st));
  if (inv_dev) RUN(GVL_PROF_OTHER, 0, gvl_launch_copy_bytes(s->bank_inv + first, inv_dev, (size_t)n * 4, st));
  return 0;
}

int gvl_op_hidden_bank_append(gvl_ctx* ctx, const uint16_t* x, int ldx, const uint16_t* w, float eps, uint16_t* rows_out, float* inv_out, int n, int cols, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!x || !w || !rows_out || !inv_out) return fail(ctx, GVL_ERR_ARG, "gvl_op_hidden_bank_append: bad arguments");
  if (n < 1 || cols % 64 || cols < 64 || cols > 8192 || ldx < cols || ldx % 8) return fail(ctx, GVL_ERR_ARG, "gvl_op_hidden_bank_append: n >= 1, cols a multiple of 64 up to 8192, ldx >= cols and a multiple of 8");
  hipStream_t st = (hipStream_t)stream;
  RUN(GVL_PROF_OTHER, 0, launch_hidden_append(x, ldx, w, eps, rows_out, inv_out, n, cols, st));
  return 0;
}

int gvl_op_contrastive_rank(gvl_ctx* ctx, const uint16_t* bank, const float* bank_inv, int n_ctx, int D, const uint16_t* cand, const float* cand_inv, const float* p, int k,
                            float alpha, float* pen, float* score, int32_t* sel, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!bank || !bank_inv || !cand || !cand_inv || !p || !pen || !score || !sel) return fail(ctx, GVL_ERR_ARG, "gvl_op_contrastive_rank: bad arguments");
  if (k < 2 || k > GVL_MAX_DECODE_BATCH) return fail(ctx, GVL_ERR_ARG, "gvl_op_contrastive_rank: k (top_k) must be 2 .. 16");
  if (D % 64 || D < 64 || D > 8192) return fail(ctx, GVL_ERR_ARG, "gvl_op_contrastive_rank: D must be a multiple of 64 up to 8192");
  if (n_ctx < 1) return fail(ctx, GVL_ERR_ARG, "gvl_op_contrastive_rank: n_ctx must be >= 1");
  if (!(alpha >= 0.f && alpha <= 1.f)) return fail(ctx, GVL_ERR_ARG, "gvl_op_contrastive_rank: alpha must be in [0, 1]");
  if ((long long)gvl_contrastive::rank_rows(k) * D * 2 > gvl_contrastive::kRankLdsBytes)
    return fail(ctx, GVL_ERR_ARG, "gvl_op_contrastive_rank: the candidate rows exceed 128 KiB of LDS (k <= 8 up to D 8192, k 9 .. 16 up to D 4096)");
  hipStream_t st = (hipStream_t)stream;
  CsBufs cb;                                               // the blocks' maxima go through the context's scratch, as in the search
  if (const int rc = cs_buffers(ctx, &cb)) return rc;
  RankArgs a; memset(&a, 0, sizeof(a));
  a.bank = bank; a.bank_inv = bank_inv; a.n_ctx = n_ctx; a.D = D; a.k = k; a.cand = cand; a.cand_inv = cand_inv; a.p = p; a.alpha = alpha; a.part = cb.part;
  a.pen = pen; a.score = score; a.sel = sel;
  RUN(GVL_PROF_CS_RANK, 0, launch_rank(a, st));
  return 0;
}

int gvl_contrastive_search(gvl_ctx* ctx, int seq_id, const float* first_logits, const gvl_contrastive_params* p, int32_t* out_ids_host, int cap, int* n_out,
                           int32_t* trace_ids, float* trace_p, float* trace_pen, int32_t* trace_sel, float* trace_rows_dev, uint16_t* final_hidden_dev, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_contrastive_search");
  if (!p || !first_logits || !out_ids_host || !n_out) return fail(ctx, GVL_ERR_ARG, "gvl_contrastive_search: bad arguments");
  const int k = p->top_k, V = ctx->cfg.vocab, Hd = ctx->cfg.hidden, max_new = p->max_new_tokens;
  const float alpha = p->penalty_alpha;
  if (const char* why = gvl_contrastive::refusal(k, alpha, max_new, ctx->outlist_cap, cap, V, Hd)) return fail(ctx, GVL_ERR_ARG, std::string("gvl_contrastive_search: ") + why);
  if (!(p->penalty > 0.f) || p->ngram < 0 || p->min_new < 0) return fail(ctx, GVL_ERR_ARG, "gvl_contrastive_search: penalty must be > 0, ngram >= 0, min_new >= 0");
  hipStream_t st = (hipStream_t)stream;
  // The current sequence -- at first the session's root clone -- carries a private copy of the caller's bank.
  SearchSession ss(ctx, "gvl_contrastive_search", st);
  if (const int rc = ss.open(seq_id, p->penalty, p->ngram, p->min_new, p->proc_eos_id, p->rules_id, max_new, true)) return rc;
  CsBufs cb;
  if (const int rc = cs_buffers(ctx, &cb)) return rc;
  const int pos0 = ss.pos0;

  gvl_contrastive::State cs;
  if (cs.init(k, max_new, p->eos_id) < 0) return fail(ctx, GVL_ERR_ARG, "gvl_contrastive_search: bad arguments");

  int cur = ss.root;
  if (const int rc = bank_alloc(ctx, ctx->seqs[cur], ss.seq_cap)) return fail(ctx, rc, "gvl_contrastive_search: no device memory for the search's copy of the hidden bank");
  { const Seq& from = ctx->seqs[seq_id]; Seq& to = ctx->seqs[cur];
    RUN(GVL_PROF_OTHER, 0, gvl_launch_copy_bytes(from.bank, to.bank, (size_t)pos0 * Hd * 2, st));
    RUN(GVL_PROF_OTHER, 0, gvl_launch_copy_bytes(from.bank_inv, to.bank_inv, (size_t)pos0 * 4, st));
    to.bank_rows = pos0; }

  const int kb = gvl_contrastive::cand_beams(k);
  float cand_scores[GVL_MAX_DECODE_BATCH];
  for (int b = 0; b < GVL_MAX_DECODE_BATCH; ++b) cand_scores[b] = b == 0 ? 0.f : -INFINITY;   // every "beam" reads the one row; only the first one's entries can rank
  float* row = nullptr;                                    // the current context's last logits; null: the caller's first_logits
  int n_ctx = pos0;

  for (int step = 0;; ++step) {
    if (ss.processed) {
      // HF's order: processors (token rules around them, then the grammar) on the RAW logits, then the softmax.  In place on the library's rows; first_logits are copied.
      if (!row) { if (const int rc = ss.copy_first(first_logits, &row)) return rc; }
      const std::vector<int>* hist = &cs.ids;
      if (const int rc = ss.upload_histories(1, (int)cs.ids.size(), &hist)) return rc;
      if (const int rc = ss.process(row, 0, 1)) return rc;
    }
    if (trace_rows_dev) HIPCHK(ctx, hipMemcpyAsync(trace_rows_dev + (size_t)step * V, row ? row : first_logits, (size_t)V * 4, hipMemcpyDeviceToDevice, st));
    // the top_k of the probabilities: the log-softmax and the strict order (value descending, id ascending) of gvl_beam_search's candidate launches
    BeamCandArgs ca; SearchSession::cand_args(ctx, ca, row ? row : first_logits, V, kb, 0, cand_scores, 1, ss.d_vals, ss.d_idx, ss.d_proc);
    RUN(GVL_PROF_OTHER, 0, gvl_launch_beam_candidates(ca, st));

    // k - 1 clones of the current sequence; candidate i runs on seqs[i]
    int seqs[GVL_MAX_DECODE_BATCH]; seqs[0] = cur;
    if (const int crc = ss.clone_many(cur, k - 1, seqs + 1)) return crc;
    Seq* sqs[GVL_MAX_DECODE_BATCH];
    FeedArgs fa; memset(&fa, 0, sizeof(fa)); fa.idx = ss.d_idx; fa.k = k;
    for (int i = 0; i < k; ++i) { sqs[i] = &ctx->seqs[seqs[i]]; fa.tok[i] = sqs[i]->d_tok; }
    Seq& cs_seq = *sqs[0];
    if (cs_seq.bank_rows != n_ctx || n_ctx >= cs_seq.bank_cap) return fail(ctx, GVL_ERR_STATE, "gvl_contrastive_search: the hidden bank is out of step");
    hipLaunchKernelGGL(contrastive_feed_kernel, dim3(1), dim3(64), 0, st, fa);
    if (hipGetLastError() != hipSuccess) return fail(ctx, GVL_ERR_HIP, "gvl_contrastive_search: launch failed");

    // one teacher-forced step of the k candidates; a part's residual rows become candidate rows before the next part overwrites them
    float* rows = nullptr;
    const auto append_cand = [&](int o, int nb) -> int {
      RUN(GVL_PROF_OTHER, 0, launch_hidden_append(ctx->d_x, Hd, ctx->l_norm, ctx->cfg.rms_eps, cb.cand + (size_t)o * Hd, cb.cand_inv + o, nb, Hd, st));
      return 0;
    };
    if (const int arc = ss.advance(sqs, k, nullptr, append_cand, &rows)) return arc;
    RankArgs ra; memset(&ra, 0, sizeof(ra));
    ra.bank = cs_seq.bank; ra.bank_inv = cs_seq.bank_inv; ra.n_ctx = n_ctx; ra.D = Hd; ra.k = k; ra.cand = cb.cand; ra.cand_inv = cb.cand_inv;
    ra.p = ss.d_proc; ra.p_is_logprob = 1; ra.alpha = alpha; ra.part = cb.part; ra.pen = cb.d_pen; ra.score = cb.d_score; ra.p_out = cb.d_p; ra.sel = cb.d_sel;
    ra.commit_row = cs_seq.bank + (size_t)n_ctx * Hd; ra.commit_inv = cs_seq.bank_inv + n_ctx;
    RUN(GVL_PROF_CS_RANK, 0, launch_rank(ra, st));
    HIPCHK(ctx, hipStreamSynchronize(st));               // the ONE synchronise of the step: candidate ids, p, pen and the selected rank sit in host-mapped memory

    const int sel = *cb.h_sel;
    int cand_ids[GVL_MAX_DECODE_BATCH];
    for (int i = 0; i < k; ++i) {
      cand_ids[i] = ss.h_idx[i];
      if (cand_ids[i] < 0 || cand_ids[i] >= V) return fail(ctx, GVL_ERR_HIP, "gvl_contrastive_search: a candidate id outside the vocabulary");
      if (trace_ids) trace_ids[(size_t)step * k + i] = cand_ids[i];
      if (trace_p) trace_p[(size_t)step * k + i] = cb.h_p[i];
      if (trace_pen) trace_pen[(size_t)step * k + i] = cb.h_pen[i];
    }
    if (trace_sel) trace_sel[step] = sel;
    int winner = -1, losers[GVL_MAX_DECODE_BATCH];
    const int rc = cs.step(cand_ids, sel, seqs, &winner, losers);
    if (rc < 0) return fail(ctx, GVL_ERR_HIP, "gvl_contrastive_search: the device selected a rank outside the candidates");
    if (winner != cur) {                                   // the winner takes over the bank (its own row is in it already)
      Seq& w = ctx->seqs[winner]; Seq& c = ctx->seqs[cur];
      std::swap(w.bank, c.bank); std::swap(w.bank_inv, c.bank_inv); std::swap(w.bank_cap, c.bank_cap); std::swap(w.bank_rows, c.bank_rows);
    }
    ctx->seqs[winner].bank_rows = ++n_ctx;
    for (int i = 0; i < k - 1; ++i) ss.drop(losers[i]);
    cur = winner;
    row = rows + (size_t)sel * V;
    if (rc == gvl_contrastive::CS_FINISHED) break;
  }

  const int n = (int)cs.ids.size();                        // <= max_new <= cap
  for (int i = 0; i < n; ++i) out_ids_host[i] = cs.ids[i];
  *n_out = n;
  if (final_hidden_dev) {
    RUN(GVL_PROF_OTHER, 0, gvl_launch_copy_bytes(ctx->seqs[cur].bank + (size_t)pos0 * Hd, final_hidden_dev, (size_t)n * Hd * 2, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
  }
  return 0;
}

}  // extern "C"
