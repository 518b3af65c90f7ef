// gvl_ops.hip -- the operator-level entries of include/gvl.h (gvl_op_*): one kernel or one launcher at a time on caller-owned tensors, for the operator tests and the
// lab tools.  No kernel lives here.  A simple entry is its own argument check and ONE launch (SIMPLE_OP).  A descriptor entry is: ctx and descriptor non-null,
// check_<entry> (gvl_op_check.h: everything the descriptor alone decides), where the kernels trust positions and page numbers the read-back of pos and the block tables
// (read_back) and tables_<entry> over the host copies, then the argument struct, the launch and the trailing synchronise.  Every refusal of those six comes from
// gvl_op_check.h -- host-only, tested on a CPU -- and is returned before anything is launched or written.
#include "gvl_model.h"
#include "gvl_op_check.h"
#include "gvl_vision_plan.h"

using namespace gvlm;

static_assert(gvl_op::ACT_NONE == GVL_ACT_NONE && gvl_op::ACT_SILU_MUL == GVL_ACT_SILU_MUL, "gvl_op_check.h restates gvl_internal.h's activations");

namespace {

// a simple entry: its own argument check (`ok`, else `what`), the stream, one launch under a profile record.  A macro: RUN's message quotes the launch expression
#define SIMPLE_OP(ok, what, cat, work, expr) do { \
    if (!ctx) return GVL_ERR_ARG; \
    if (!(ok)) return fail(ctx, GVL_ERR_ARG, what); \
    hipStream_t st = (hipStream_t)stream; \
    RUN(cat, work, expr); \
    return 0; \
  } while (0)

// what the three GEMM entries share: row-major operands, the output row length of the activation, every epilogue operand they all take
GemmArgs op_gemm_args(const uint16_t* A, const uint16_t* W, void* C, int M, int N, int K, const float* bias, const float* gamma, const void* resid, int act, int out_f32, int tile_cfg) {
  GemmArgs g = gemm(A, K, W, C, act == GVL_ACT_SILU_MUL ? N / 2 : N, M, N, K);
  g.bias = bias; g.gamma = gamma; g.resid = resid; g.ldr = N; g.act = act; g.out_f32 = out_f32; g.round_pre_resid = 1; g.tile_cfg = tile_cfg;
  return g;
}

// the result of descriptor entry `fn` for a verdict of gvl_op_check.h (null: admitted)
int refused(gvl_ctx* ctx, const char* fn, const char* text) { return text ? fail(ctx, GVL_ERR_ARG, std::string(fn) + ": " + text) : 0; }

// What a table check reads: the stream is drained, then the device arrays dev[0 .. n) of count[i] ints (count < 1: none, host[i] null) are copied behind one another into buf
int read_back(gvl_ctx* ctx, hipStream_t st, int n, const int* const* dev, const long long* count, std::vector<int>& buf, const int** host) {
  size_t total = 0, at = 0;
  for (int i = 0; i < n; ++i) total += count[i] > 0 ? (size_t)count[i] : 0;
  buf.resize(total);
  HIPCHK(ctx, hipStreamSynchronize(st));
  for (int i = 0; i < n; ++i) {
    host[i] = nullptr;
    if (count[i] < 1) continue;
    HIPCHK(ctx, hipMemcpy(buf.data() + at, dev[i], sizeof(int) * (size_t)count[i], hipMemcpyDeviceToHost));
    host[i] = buf.data() + at;
    at += (size_t)count[i];
  }
  return 0;
}
// the tables of a paged descriptor (gvl_qkv_post, gvl_prefill_attn): the single form's block table, or the ragged members' up to the first one without a length
template <class P>
int read_tables(gvl_ctx* ctx, hipStream_t st, const P& p, std::vector<int>& buf, gvl_op::HostTables& h) {
  const int* dev[1 + GVL_MAX_PREFILL_BATCH] = {p.block_table}; long long count[1 + GVL_MAX_PREFILL_BATCH] = {0}; const int* host[1 + GVL_MAX_PREFILL_BATCH];
  if (!p.vl_n && p.block_table) count[0] = (long long)p.B * p.max_pages;
  for (int u = 0; u < p.vl_n && p.table_len[u] >= 1; ++u) { dev[1 + u] = p.vl_tables[u]; count[1 + u] = p.table_len[u]; }
  if (int rc = read_back(ctx, st, 1 + GVL_MAX_PREFILL_BATCH, dev, count, buf, host)) return rc;
  h.block = host[0];
  for (int u = 0; u < GVL_MAX_PREFILL_BATCH; ++u) h.vl[u] = host[1 + u];
  return 0;
}

// the work of gvl_op_decode_proj and gvl_op_dgemm (`who`) behind their checks: private tiled / quantised copies of the row-major operands, the launch, what the quantiser left
int decode_proj_run(gvl_ctx* ctx, const gvl_decode_proj* p, hipStream_t st, const char* who) {
  const int N = p->N, K = p->K, B = p->batch;
  struct Bufs { void* v[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; ~Bufs() { for (void* q : v) if (q) hipFree(q); } } bufs;
  void *&wc = bufs.v[0], *&wt = bufs.v[1], *&ws = bufs.v[2], *&xt = bufs.v[3];
  const size_t nb16 = (size_t)((N + 15) / 16);
  const int Dr = p->rope_on ? p->Dr : 0, nqk = p->rope_on ? p->H + p->KV : 0;
  GemvArgs g; memset(&g, 0, sizeof(g));
  int rc = 0;
  if (p->path == 0) {
    if (p->w_fmt) {                                // the quantisers rewrite their row-major source: work on a copy
      HIPCHK(ctx, hipMalloc(&wc, (size_t)N * K * 2));
      HIPCHK(ctx, hipMemcpyAsync(wc, p->W, (size_t)N * K * 2, hipMemcpyDeviceToDevice, st));
      HIPCHK(ctx, hipMalloc(&wt, nb16 * 16 * K));
      HIPCHK(ctx, hipMalloc(&ws, p->w_fmt == 1 ? (size_t)N * 4 : nb16 * (K / 128) * 16 * 4));
      rc = p->w_fmt == 1 ? gvl_fp8_quantise_decode_weight((bf16_t*)wc, (unsigned char*)wt, (float*)ws, N, K, Dr, nqk, st)
                         : gvl_mxfp4_quantise_decode_weight((bf16_t*)wc, (unsigned char*)wt, (unsigned*)ws, N, K, Dr, nqk, st);
      g.wscale = (const float*)ws;
    } else {
      HIPCHK(ctx, hipMalloc(&wt, nb16 * 16 * K * 2));
      rc = gvl_retile_decode_weight(p->W, (bf16_t*)wt, N, K, Dr, nqk, st);
    }
    g.W = (const bf16_t*)wt; g.w_fp8 = p->w_fmt;
    if (!rc && !p->x_is_tiled && !p->norm_w) {
      HIPCHK(ctx, hipMalloc(&xt, (size_t)16 * K * 2));
      HIPCHK(ctx, hipMemsetAsync(xt, 0, (size_t)16 * K * 2, st));
      rc = gvl_launch_rows_to_tiled(p->x, (bf16_t*)xt, B, K, K, st);
      g.x = (const bf16_t*)xt;
    } else g.x = p->x;
  } else { g.W = p->W; g.x = p->x; }
  g.N = N; g.K = K; g.batch = B; g.x_stride = K;
  g.out_stride = p->out_stride ? p->out_stride : (p->act == GVL_ACT_SILU_MUL ? N / 2 : N);
  g.norm_w = p->norm_w; g.eps = p->eps; g.bias = p->bias; g.resid = p->resid; g.act = p->act; g.out_bf16 = p->out_bf16; g.out_f32 = p->out_f32;
  g.variant = p->variant; g.out_tiled = p->out_tiled; g.sq_in = p->sq_in; g.sq_n = p->sq_n; g.sq_out = p->sq_out; g.out_tiled2 = p->out_tiled2;
  if (p->rope_on) {
    g.rope_on = 1; g.cos_s = p->cos_s; g.sin_s = p->sin_s; g.cos_l = p->cos_l; g.sin_l = p->sin_l; g.rope_switch = p->rope_switch;
    for (int b = 0; b < B; ++b) { g.pos_ptrs[b] = p->pos + b; g.tables[b] = p->tables + (size_t)b * p->table_stride; }
    g.Q = p->Q; g.Kt = p->Kt; g.Vt = p->Vt; g.H = p->H; g.KV = p->KV; g.Dr = p->Dr; g.D = p->D; g.q_stride = p->q_stride;
  }
  if (!rc) { ProfScope _ps(ctx, GVL_PROF_GEMV, 2.0 * N * K, st); rc = p->path == 0 ? gvl_launch_dgemm(g, st) : gvl_launch_gemv(g, st); }
  if (!rc && p->w_fmt) {                           // read back what the quantiser left, only once the launcher has accepted the call
    if (p->w_deq) HIPCHK(ctx, hipMemcpyAsync(p->w_deq, wc, (size_t)N * K * 2, hipMemcpyDeviceToDevice, st));
    if (p->w_scale) HIPCHK(ctx, hipMemcpyAsync(p->w_scale, ws, p->w_fmt == 1 ? (size_t)N * 4 : nb16 * (K / 128) * 16 * 4, hipMemcpyDeviceToDevice, st));
  }
  const hipError_t se = hipStreamSynchronize(st);
  if (rc) return fail(ctx, rc == -1 ? GVL_ERR_ARG : GVL_ERR_HIP, std::string(who) + (rc == -1 ? ": the launcher does not serve this combination" : ": launch failed"));
  if (se != hipSuccess) return gvl_hipfail(ctx, se, (std::string(who) + ": hipStreamSynchronize").c_str());
  return 0;
}

}  // namespace

extern "C" {

int gvl_op_gemm(gvl_ctx* ctx, const uint16_t* A, const uint16_t* W, void* C, int M, int N, int K, const float* bias, const float* gamma,
                const void* resid, int act, int out_f32, int tile_cfg, void* stream) {
  GemmArgs g = op_gemm_args(A, W, C, M, N, K, bias, gamma, resid, act, out_f32, tile_cfg);
  if (const char* e = gvl_lab_env("GVL_LAB_LD")) { int la = 0, lw = 0; if (sscanf(e, "%d,%d", &la, &lw) == 2) { g.lda = la; g.ldw = lw; } }   // LAB: operand row pitches (tools/gemm_lab.py)
  SIMPLE_OP(true, "", GVL_PROF_GEMM, gvl_gemm_flops(g), gvl_launch_gemm(g, st));
}
// The fused-RMSNorm epilogues at operator level (bf16 output): rowscale [M] f32 or null multiplies the accumulator rows before bias / activation; rowsq
// [M][rowsq_ld] f32 or null receives the sums of squares of the rounded outputs per aligned 64-column block (N % 64 == 0).
int gvl_op_gemm_rows(gvl_ctx* ctx, const uint16_t* A, const uint16_t* W, uint16_t* C, int M, int N, int K, const float* bias, const float* gamma,
                     const uint16_t* resid, int act, const float* rowscale, float* rowsq, int rowsq_ld, int tile_cfg, void* stream) {
  GemmArgs g = op_gemm_args(A, W, C, M, N, K, bias, gamma, resid, act, 0, tile_cfg);
  g.rowscale = rowscale; g.rowsq = rowsq; g.rowsq_ld = rowsq_ld;
  SIMPLE_OP(true, "", GVL_PROF_GEMM, gvl_gemm_flops(g), gvl_launch_gemm(g, st));
}
// The row-remapping store of build_visual at operator level: GEMM row m lands at row (m / grp_rows) * grp_stride + m % grp_rows + row_off of C.
int gvl_op_gemm_grouped(gvl_ctx* ctx, const uint16_t* A, const uint16_t* W, void* C, int M, int N, int K, const float* bias, const float* gamma,
                        const void* resid, int act, int out_f32, float* rowsq, int rowsq_ld, int grp_rows, int grp_stride, int row_off, int tile_cfg,
                        void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!A || !W || !C) return fail(ctx, GVL_ERR_ARG, "gvl_op_gemm_grouped: null operand");
  if (grp_rows < 1 || row_off < 0 || (long)row_off + grp_rows > grp_stride) return fail(ctx, GVL_ERR_ARG, "gvl_op_gemm_grouped: needs grp_rows >= 1, row_off >= 0 and row_off + grp_rows <= grp_stride");
  GemmArgs g = op_gemm_args(A, W, C, M, N, K, bias, gamma, resid, act, out_f32, tile_cfg);
  g.rowsq = rowsq; g.rowsq_ld = rowsq_ld; g.grp_rows = grp_rows; g.grp_stride = grp_stride; g.row_off = row_off;
  SIMPLE_OP(true, "", GVL_PROF_GEMM, gvl_gemm_flops(g), gvl_launch_gemm(g, st));
}
// W' = bf16(W diag(gamma)) and rs = rsqrt(sum of the blocks [b0, b0 + nblk) / cols + eps): the two small kernels around those epilogues
int gvl_op_fold_gamma(gvl_ctx* ctx, const uint16_t* W, const uint16_t* gamma, uint16_t* Wo, int64_t rows, int cols, void* stream) {
  SIMPLE_OP(true, "", GVL_PROF_OTHER, 0, gvl_launch_fold_gamma(W, gamma, Wo, (long)rows, cols, st));
}
int gvl_op_rowsq_finish(gvl_ctx* ctx, const float* rowsq, int ld, int b0, int nblk, float* rs, int rows, int cols, float eps, void* stream) {
  SIMPLE_OP(true, "", GVL_PROF_OTHER, 0, gvl_launch_rowsq_finish(rowsq, ld, b0, nblk, rs, rows, cols, eps, st));
}
int gvl_op_attention(gvl_ctx* ctx, const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out, int B, int S, int H, int KV, int Dr,
                     float scale, int causal, void* stream) {
  // q/k/v here are column blocks of ONE fused row-major qkv tensor [B*S][(H+2KV)*Dr]: q points at column 0;
  // k and v must equal q + H*Dr and q + (H+KV)*Dr (checked) -- the layout every tower produces.
  if (!ctx) return GVL_ERR_ARG;
  if (k != q + (size_t)H * Dr || v != q + (size_t)(H + KV) * Dr) return fail(ctx, GVL_ERR_ARG, "gvl_op_attention: q,k,v must be the column blocks of one fused qkv tensor");
  const int D = pad_head(Dr);
  if (D < 0 || (Dr & 7)) return fail(ctx, GVL_ERR_ARG, "gvl_op_attention: head dim unsupported");
  hipStream_t st = (hipStream_t)stream;
  const int tiles = (S + 63) / 64;
  ArenaScope arena_scope(ctx->arena_off);
  AALLOC(Q, bf16_t, (size_t)B * H * S * D); AALLOC(Kt, bf16_t, (size_t)B * tiles * KV * 64 * D); AALLOC(Vt, bf16_t, (size_t)B * tiles * KV * 64 * D);
  // non-causal (vision) attention reads v -- and, when no head-dim padding is needed, q and k -- in place: the towers' own decision (gvl_vision_plan.h), CLIP's form
  const int ld = (H + 2 * KV) * Dr;
  const VisionOperandPath path = vision_operand_path(ctx->dbg.vision_in_place, D, Dr, causal != 0, GVL_TOWER_CLIP);
  if (path.qkv_post) { QkvPostArgs p; memset(&p, 0, sizeof(p)); p.qkv = q; p.ld = ld; p.Q = Q; p.Kt = Kt; p.Vt = path.vt_pages ? Vt : nullptr; p.B = B; p.S = S; p.H = H; p.KV = KV; p.Dr = Dr; p.D = D; p.mode = 0;
    RUN(GVL_PROF_OTHER, 0, gvl_launch_qkv_post(p, st)); }
  { AttnArgs a; memset(&a, 0, sizeof(a)); a.Q = Q; a.Kt = Kt; a.Vt = Vt; a.O = out; a.B = B; a.H = H; a.KV = KV; a.S = S; a.D = D; a.Dout = Dr; a.scale = scale; a.causal = causal; a.ring = ctx->dbg.attn_ring;
    if (!path.vt_pages) { a.Vrows = v; a.v_ld = ld; }
    if (path.qk_rows) { a.Qrows = q; a.Krows = k; a.q_ld = a.k_ld = ld; }
    RUN(GVL_PROF_ATTN, gvl_attn_flops(a), gvl_launch_attention(a, st)); }
  return 0;
}
int gvl_op_layernorm(gvl_ctx* ctx, const float* x, const float* w, const float* b, uint16_t* y, int rows, int cols, float eps, void* stream) {
  SIMPLE_OP(true, "", GVL_PROF_OTHER, 0, gvl_launch_layernorm_f32(x, w, b, y, rows, cols, eps, st));
}
int gvl_op_rmsnorm(gvl_ctx* ctx, const uint16_t* x, const uint16_t* w, uint16_t* y, int rows, int cols, float eps, void* stream) {
  SIMPLE_OP(true, "", GVL_PROF_OTHER, 0, gvl_launch_rmsnorm_bf16(x, w, y, rows, cols, eps, st));
}
// ---- the vision front end and the glue of the visual prefix at operator level (tests/test_gpu_vision_ops.py; fields and geometry: include/gvl.h) ----------------
// The patch embedding of either tower by EITHER path, chosen by the caller: a geometry the fused launcher refuses is an error here, not a fall-back.
int gvl_op_patch_embed(gvl_ctx* ctx, const gvl_patch_embed* p, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!p) return fail(ctx, GVL_ERR_ARG, "gvl_op_patch_embed: null descriptor");
  if (int rc = refused(ctx, "gvl_op_patch_embed", gvl_op::check_patch_embed(*p))) return rc;
  const int g = p->image / p->patch;
  const int M = p->n * p->T * g * g, TL = p->T * g * g, C = p->C;
  hipStream_t st = (hipStream_t)stream;
  ArenaScope arena_scope(ctx->arena_off);
  if (p->path == 0) {
    AALLOC(Wt, bf16_t, (size_t)(C / 16) * (3 * p->patch / 2) * 512);
    PatchEmbedArgs e; memset(&e, 0, sizeof(e)); e.px = p->px; e.Wt = Wt; e.n_img = p->n; e.T = p->T; e.image = p->image; e.patch = p->patch; e.C = C;
    e.M = M; e.S = TL + 1; e.mode = p->mode; e.eps = p->eps;
    if (p->mode == 0) { e.cls_f32 = (const float*)p->cls; e.pos_f32 = (const float*)p->pos; e.lnw = p->lnw; e.lnb = p->lnb; e.x_f32 = (float*)p->out; }
    else { e.bias = p->bias; e.cls_bf = (const bf16_t*)p->cls; e.pos_bf = (const bf16_t*)p->pos; e.x_bf = (bf16_t*)p->out; }
    RUN(GVL_PROF_OTHER, 0, gvl_retile_patch_weight(p->W, Wt, C, p->Kp, p->patch, st));
    const int rc = gvl_launch_patch_embed(e, st);
    if (rc) return rc == -1 ? refused(ctx, "gvl_op_patch_embed", gvl_op::kPatchNotFused) : fail(ctx, GVL_ERR_HIP, "gvl_op_patch_embed: launch failed");
    return 0;
  }
  bf16_t* pA = p->im2col;
  if (!pA) { AALLOC(pA_, bf16_t, (size_t)M * p->Kp); pA = pA_; }
  AALLOC(pO, bf16_t, (size_t)M * C);
  GemmArgs gm = gemm(pA, p->Kp, p->W, pO, C, M, C, p->Kp);
  if (p->mode == 1) gm.bias = p->bias;
  RUN(GVL_PROF_OTHER, 0, gvl_launch_patchify(p->px, pA, p->n, p->T, p->image, p->patch, p->Kp, st));
  RUN(GVL_PROF_GEMM, gvl_gemm_flops(gm), gvl_launch_gemm(gm, st));
  if (p->mode == 0) RUN(GVL_PROF_OTHER, 0, gvl_launch_clip_embed_ln(pO, (const float*)p->cls, (const float*)p->pos, p->lnw, p->lnb, (float*)p->out, p->n, TL, C, p->eps, st));
  else RUN(GVL_PROF_OTHER, 0, gvl_launch_iv2_embed(pO, (const bf16_t*)p->cls, (const bf16_t*)p->pos, (bf16_t*)p->out, p->n, TL, C, st));
  return 0;
}
int gvl_op_patchify(gvl_ctx* ctx, const float* px, uint16_t* A, int n, int T, int image, int patch, int Kp, void* stream) {
  SIMPLE_OP(px && A && n > 0 && T > 0 && image > 0 && patch > 0 && Kp > 0, "gvl_op_patchify: bad arguments", GVL_PROF_OTHER, 0, gvl_launch_patchify(px, A, n, T, image, patch, Kp, st));
}
int gvl_op_hd_merge(gvl_ctx* ctx, const float* f, const float* sub_gn, uint16_t* out, int n, int C, void* stream) {
  SIMPLE_OP(f && sub_gn && out && n > 0 && C > 0, "gvl_op_hd_merge: bad arguments", GVL_PROF_OTHER, 0, gvl_launch_hd_merge(f, sub_gn, out, n, C, st));
}
int gvl_op_pool_spatial(gvl_ctx* ctx, const float* f, uint16_t* out, int n, int C, void* stream) {
  SIMPLE_OP(f && out && n > 0 && C > 0, "gvl_op_pool_spatial: bad arguments", GVL_PROF_OTHER, 0, gvl_launch_pool_spatial(f, out, n, C, st));
}
int gvl_op_pool_temporal(gvl_ctx* ctx, const uint16_t* f, uint16_t* out, int n, int T, int C, void* stream) {
  SIMPLE_OP(f && out && n > 0 && T > 0 && C > 0, "gvl_op_pool_temporal: bad arguments", GVL_PROF_OTHER, 0, gvl_launch_pool_temporal(f, out, n, T, C, st));
}
int gvl_op_strip_cls(gvl_ctx* ctx, const void* x, void* y, int n, int S, int C, int elem_bytes, void* stream) {
  SIMPLE_OP(x && y && n > 0 && S >= 2 && C > 0 && (elem_bytes == 2 || elem_bytes == 4), "gvl_op_strip_cls: bad arguments", GVL_PROF_OTHER, 0, gvl_launch_strip_cls(x, y, n, S, C, elem_bytes, st));
}
int gvl_op_bcast_row(gvl_ctx* ctx, const uint16_t* row, uint16_t* dst, int n, int stride_rows, int row_off, int cols, void* stream) {
  SIMPLE_OP(row && dst && n > 0 && cols > 0 && row_off >= 0 && row_off < stride_rows, "gvl_op_bcast_row: bad arguments", GVL_PROF_OTHER, 0, gvl_launch_bcast_row(row, dst, n, stride_rows, row_off, cols, st));
}
// operator-level entry for the WHOLE GemvArgs surface (tests/test_gpu_decode_proj.py): row-major operands in, private tiled / quantised copies made by decode_proj_run, every
// launcher refusal returned as GVL_ERR_ARG before anything is written.  See include/gvl.h for the fields.  rope_on: the kernel trusts positions and page numbers
int gvl_op_decode_proj(gvl_ctx* ctx, const gvl_decode_proj* p, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!p) return fail(ctx, GVL_ERR_ARG, "gvl_op_decode_proj: null descriptor");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = refused(ctx, "gvl_op_decode_proj", gvl_op::check_decode_proj(*p))) return rc;
  if (p->rope_on) {
    const int* dev[2] = {p->pos, p->tables}; const long long count[2] = {p->batch, (long long)p->batch * p->table_stride}; const int* host[2];
    std::vector<int> buf;
    if (int rc = read_back(ctx, st, 2, dev, count, buf, host)) return rc;
    if (int rc = refused(ctx, "gvl_op_decode_proj", gvl_op::tables_decode_proj(*p, host[0], host[1]))) return rc;
  }
  return decode_proj_run(ctx, p, st, "gvl_op_decode_proj");
}
// y f32 [batch][N] = x W^T + bias on the skinny GEMM: the plain form of the descriptor above, under this entry's own precondition (any N; K % 256 == 0)
int gvl_op_dgemm(gvl_ctx* ctx, const uint16_t* W, const uint16_t* x, const float* bias, float* y, int N, int K, int batch, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (N <= 0 || K <= 0 || K % 256 || batch < 1 || batch > GVL_MAX_DECODE_BATCH) return fail(ctx, GVL_ERR_ARG, "gvl_op_dgemm: K % 256 == 0 and 1 <= batch <= 16");
  gvl_decode_proj p; memset(&p, 0, sizeof(p));
  p.W = W; p.x = x; p.bias = bias; p.out_f32 = y; p.N = N; p.K = K; p.batch = batch;
  return decode_proj_run(ctx, &p, (hipStream_t)stream, "gvl_op_dgemm");
}
// operator-level entry for the WHOLE DecodeAttnArgs surface (tests/test_gpu_decode_attn_exact.py): the caller supplies every device tensor, the workspace (part, counters)
// included, so a test can poison it before a launch and look at it afterwards.  The kernels trust positions and page numbers: they are read back and checked here, on
// the host, and every refusal comes back as GVL_ERR_ARG before anything is launched or written.  Otherwise DecodeAttnArgs is filled as decode_step fills it.
int gvl_op_decode_attention(gvl_ctx* ctx, const gvl_decode_attn* p, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!p) return fail(ctx, GVL_ERR_ARG, "gvl_op_decode_attention: null descriptor");
  hipStream_t st = (hipStream_t)stream;
  const int B = p->batch;
  if (int rc = refused(ctx, "gvl_op_decode_attention", gvl_op::check_decode_attention(*p))) return rc;
  const int* dev[2] = {p->pos, p->tables}; const long long count[2] = {B, (long long)B * p->table_stride}; const int* host[2];
  std::vector<int> buf;
  if (int rc = read_back(ctx, st, 2, dev, count, buf, host)) return rc;
  if (int rc = refused(ctx, "gvl_op_decode_attention", gvl_op::tables_decode_attention(*p, host[0], host[1]))) return rc;
  DecodeAttnArgs a; memset(&a, 0, sizeof(a));
  a.q = p->q; a.q_stride = p->q_stride; a.Kt = p->Kt; a.Vt = p->Vt;
  for (int b = 0; b < B; ++b) { a.tables[b] = p->tables + (size_t)b * p->table_stride; a.pos_ptrs[b] = p->pos + b; }
  a.part = p->part; a.counters = p->counters; a.batch = B; a.gsplit = p->gsplit; a.cpb = p->cpb; a.hpb = p->hpb;
  a.out = p->out; a.out_stride = p->out_stride; a.out_tiled = p->out_tiled ? 1 : 0; a.H = p->H; a.KV = p->KV; a.D = p->D; a.Dout = p->Dout; a.nsplit = p->nsplit; a.scale = p->scale;
  RUN(GVL_PROF_DECODE_ATTN, 0, gvl_launch_decode_attention(a, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  return 0;
}
// operator-level entry for the WHOLE QkvPostArgs surface and both launchers (tests/test_gpu_qkv_post.py).  The kernels trust page numbers, positions and the ragged
// row offsets: the tables are read back and everything is checked here, on the host; every refusal comes back as GVL_ERR_ARG before anything is launched or written.
int gvl_op_qkv_post(gvl_ctx* ctx, const gvl_qkv_post* p, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!p) return fail(ctx, GVL_ERR_ARG, "gvl_op_qkv_post: null descriptor");
  hipStream_t st = (hipStream_t)stream;
  const int n = p->vl_n;
  if (int rc = refused(ctx, "gvl_op_qkv_post", gvl_op::check_qkv_post(*p))) return rc;
  std::vector<int> buf; gvl_op::HostTables h;
  if (int rc = read_tables(ctx, st, *p, buf, h)) return rc;
  if (int rc = refused(ctx, "gvl_op_qkv_post", gvl_op::tables_qkv_post(*p, h))) return rc;
  QkvPostArgs a; memset(&a, 0, sizeof(a));
  a.qkv = p->qkv; a.ld = p->ld; a.Q = p->Q; a.Kt = p->Kt; a.Vt = p->Vt; a.block_table = p->block_table; a.max_pages = p->max_pages;
  a.B = p->B; a.S = p->S; a.H = p->H; a.KV = p->KV; a.Dr = p->Dr; a.D = p->D; a.mode = p->mode; a.qn = p->qn; a.kn = p->kn; a.eps = p->eps;
  a.cos = p->cos; a.sin = p->sin; a.pos0 = p->pos0; a.ones_row = p->ones_row ? 1 : 0; a.k_ones = p->k_ones ? 1 : 0; a.q_rs = p->q_rs; a.vl_n = n;
  for (int u = 0; u <= n; ++u) a.vl_rows[u] = p->vl_rows[u];
  for (int u = 0; u < n; ++u) { a.vl_tables[u] = p->vl_tables[u]; a.vl_pos0[u] = p->vl_pos0[u]; }
  if (p->ext) RUN(GVL_PROF_OTHER, 0, gvl_launch_qkv_post_ext(a, st));
  else RUN(GVL_PROF_OTHER, 0, gvl_launch_qkv_post(a, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  return 0;
}
// operator-level entry for the paged forms of attn_fwd_kernel behind a cached prefix (tests/test_gpu_prefill_attn.py): a caller-supplied block table with qpos0 / Sk, the
// ragged grid and the ragged-extend grid, on caller-owned pages.  The plans are asked first (a refusal names them), then the tables are read back and every page the
// launch will read is checked: GVL_ERR_ARG before anything is launched or written.
int gvl_op_prefill_attention(gvl_ctx* ctx, const gvl_prefill_attn* p, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!p) return fail(ctx, GVL_ERR_ARG, "gvl_op_prefill_attention: null descriptor");
  hipStream_t st = (hipStream_t)stream;
  const int n = p->vl_n;
  if (int rc = refused(ctx, "gvl_op_prefill_attention", gvl_op::check_prefill_attention(*p))) return rc;
  std::vector<int> buf; gvl_op::HostTables h;
  if (int rc = read_tables(ctx, st, *p, buf, h)) return rc;
  if (int rc = refused(ctx, "gvl_op_prefill_attention", gvl_op::tables_prefill_attention(*p, h))) return rc;
  AttnArgs a; memset(&a, 0, sizeof(a));
  a.Q = p->Q; a.Kt = p->Kt; a.Vt = p->Vt; a.O = p->O; a.block_table = p->block_table; a.max_pages = p->max_pages;
  a.B = p->B; a.H = p->H; a.KV = p->KV; a.S = p->S; a.D = p->D; a.Dout = p->Dout; a.Sk = p->Sk; a.qpos0 = p->qpos0; a.scale = p->scale; a.causal = p->causal ? 1 : 0; a.ring = p->ring;
  a.vl_n = n;
  for (int u = 0; u <= n; ++u) a.vl_rows[u] = p->vl_rows[u];
  for (int u = 0; u < n; ++u) { a.vl_tables[u] = p->vl_tables[u]; a.vl_pos0[u] = p->ext ? p->vl_pos0[u] : 0; }
  if (p->ext) RUN(GVL_PROF_ATTN, 0, gvl_launch_attention_ext(a, st));
  else RUN(GVL_PROF_ATTN, gvl_attn_flops(a), gvl_launch_attention(a, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  return 0;
}
// operator-level entry for the attention launch of an InternVideo2 block (tests/test_gpu_iv2_attn.py): the ONES instantiations of attn_fwd_kernel, the q-normalised-on-load
// operand mode and attn_iv2_pipe_kernel, on caller-owned buffers.  ONE gvl_launch_attention (two kernel launches where the plan splits the rows), no arena allocation,
// no qkv_post; the form, pipe and pipe_rows come from the descriptor, never from gvl_debug_set.  The plan is asked first: GVL_ERR_ARG before anything is launched or written.
int gvl_op_iv2_attention(gvl_ctx* ctx, const gvl_iv2_attn* p, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!p) return fail(ctx, GVL_ERR_ARG, "gvl_op_iv2_attention: null descriptor");
  hipStream_t st = (hipStream_t)stream;
  const int f = p->form;
  if (int rc = refused(ctx, "gvl_op_iv2_attention", gvl_op::check_iv2_attention(*p))) return rc;
  AttnArgs a; memset(&a, 0, sizeof(a));
  a.Q = p->Q; a.Kt = p->Kt; a.Vt = p->Vt; a.O = p->out; a.B = p->B; a.H = p->H; a.KV = p->H; a.S = p->S; a.D = pad_head(p->Dr); a.Dout = p->Dr;
  a.scale = p->scale; a.causal = 0; a.ones_row = 1;
  if (f) { a.Vrows = p->qkv + (size_t)2 * p->H * p->Dr; a.v_ld = p->ld; }
  if (f == 2) { a.Qrows = p->qkv; a.q_ld = p->ld; a.q_rs = p->q_rs; a.q_nw = p->q_nw; a.k_ones = 1; a.pipe = p->pipe; a.pipe_rows = p->pipe_rows; }
  RUN(GVL_PROF_ATTN, gvl_attn_flops(a), gvl_launch_attention(a, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  return 0;
}
// micro-benchmark of the decode projection kernels on synthetic operands (tools/decode_bench.py): mode 0 = skinny MFMA GEMM (variant:
// see gvl_launch_dgemm), 1 = round-1 VALU GEMV (batch 1, 2, 4), 2 / 3 = the same two with the fused RMSNorm prologue (batch <= 4).  `rounds` distinct weight matrices are cycled so that the
// Infinity Cache cannot hold the stream; returns the average microseconds per launch.
int gvl_op_decode_bench(gvl_ctx* ctx, int N, int K, int batch, int mode, int variant, int rounds, int iters, double* us_per_launch, void* stream) {
  if (!ctx || !us_per_launch || N <= 0 || K <= 0 || K % 256 || batch < 1 || batch > GVL_MAX_DECODE_BATCH || rounds < 1 || iters < 1) return fail(ctx, GVL_ERR_ARG, "gvl_op_decode_bench: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const size_t wbytes = (size_t)((N + 15) / 16) * 16 * K * 2;
  char *w = nullptr, *x = nullptr, *y = nullptr;
  HIPCHK(ctx, hipMalloc((void**)&w, wbytes * rounds));
  HIPCHK(ctx, hipMalloc((void**)&x, (size_t)16 * K * 2));
  HIPCHK(ctx, hipMalloc((void**)&y, (size_t)16 * N * 4));
  hipMemsetAsync(w, 0x11, wbytes * rounds, st); hipMemsetAsync(x, 0x22, (size_t)16 * K * 2, st);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  int rc = 0;
  for (int pass = 0; pass < 2 && !rc; ++pass) {          // pass 0 = warm-up
    if (pass == 1) hipEventRecord(e0, st);
    for (int it = 0; it < (pass ? iters : 3) && !rc; ++it) {
      GemvArgs g; memset(&g, 0, sizeof(g)); g.W = (const bf16_t*)(w + wbytes * (it % rounds)); g.N = N; g.K = K; g.x = (const bf16_t*)x; g.out_f32 = (float*)y;
      g.batch = batch; g.x_stride = K; g.out_stride = N; g.variant = variant;
      if (mode == 2 || mode == 3) { g.norm_w = (const bf16_t*)x; g.eps = 1e-5f; }   // fused RMSNorm prologue: 2 = skinny GEMM (LDS), 3 = VALU GEMV
      rc = (mode == 1 || mode == 3) ? gvl_launch_gemv(g, st) : gvl_launch_dgemm(g, st);
    }
    if (pass == 1) hipEventRecord(e1, st);
  }
  hipStreamSynchronize(st);
  float ms = 0.f; hipEventElapsedTime(&ms, e0, e1);
  hipEventDestroy(e0); hipEventDestroy(e1);
  hipFree(w); hipFree(x); hipFree(y);
  if (rc) return fail(ctx, rc == -1 ? GVL_ERR_ARG : GVL_ERR_HIP, "gvl_op_decode_bench: launch failed (unsupported variant / geometry)");
  *us_per_launch = 1e3 * ms / iters;
  return 0;
}
int gvl_op_gemv(gvl_ctx* ctx, const uint16_t* W, const uint16_t* x, const float* bias, float* y, int N, int K, void* stream) {
  GemvArgs g; memset(&g, 0, sizeof(g)); g.W = W; g.N = N; g.K = K; g.x = x; g.bias = bias; g.out_f32 = y;
  SIMPLE_OP(true, "", GVL_PROF_GEMV, 2.0 * N * K, gvl_launch_gemv(g, st));
}

}  // extern "C"
