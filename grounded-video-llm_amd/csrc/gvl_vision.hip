// gvl_vision.hip -- the launch sequences of the two vision towers and of the glue / projectors (host code; the kernels live in gvl_gemm*.hip, gvl_attn.hip,
// gvl_elem.hip, gvl_patch.hip).  Each sequence = plan (gvl_vision_plan.h: which launches, in which order, in which workspace), allocate by the plan's table, walk:
// the sinks below hold what a step passes to its launcher and nothing that decides.  Restates (file:line in the reference):
//   CLIP tower      models/modeling_clip.py:182-191,355-393,626-651,851   (23 of 24 layers, hidden_states[-2])
//   InternVideo2    models/internvideo2.py:680-684,721-725,970-1040      (39 of 40 blocks)
//   glue/projectors models/llava_next_video.py:454-489,507-564
#include "gvl_model.h"
#include "gvl_vision_plan.h"

namespace gvlm {

static VisionGeometry clip_geometry(const gvl_ctx* c, int n) {
  const gvl_config& f = c->cfg;
  return VisionGeometry{GVL_TOWER_CLIP, n, f.clip_hidden, f.clip_inter, f.clip_heads, c->c_S, c->c_P, c->c_Kp, c->c_Dr, c->c_D, 1, f.clip_image, f.clip_patch, f.clip_layers_run,
                        c->c_patchwt != nullptr, false};
}
static VisionGeometry iv2_geometry(const gvl_ctx* c, int n) {
  const gvl_config& f = c->cfg;
  return VisionGeometry{GVL_TOWER_IV2, n, f.iv2_dim, f.iv2_inter, f.iv2_heads, c->v_S, c->v_TL, c->v_Kp, c->v_Dr, c->v_D, f.iv2_frames_per_seg, f.iv2_image, f.iv2_patch, f.iv2_blocks_run,
                        c->v_patchwt != nullptr, !c->vb.empty() && c->vb[0].qkvw_f};
}
static GlueGeometry glue_geometry(const gvl_ctx* c, int n) {
  const gvl_config& f = c->cfg;
  return GlueGeometry{f.llm_kind == GVL_LLM_PHI3, n, f.hidden, c->img_tok, c->seg_tok, c->tok_per_seg, f.clip_hidden, f.iv2_dim, f.iv2_frames_per_seg, c->c_P, c->v_TL};
}
static VisionKnobs vision_knobs(const gvl_ctx* c) { return VisionKnobs{c->dbg.patch_fused, c->dbg.vision_in_place, c->dbg.norm_fused, c->dbg.attn_pipe, c->dbg.attn_pipe_rows}; }

// ---------------------------------------------------------------------------------------------------
size_t clip_bytes(const gvl_ctx* c, int n) { WorkspaceEntry t[GVL_VB_COUNT]; return workspace_bytes(t, vision_workspace(clip_geometry(c, n), t), GVL_WS_TAIL); }
size_t iv2_bytes(const gvl_ctx* c, int n) { WorkspaceEntry t[GVL_VB_COUNT]; return workspace_bytes(t, vision_workspace(iv2_geometry(c, n), t), GVL_WS_TAIL); }
size_t visual_bytes(const gvl_ctx* c, int n) { WorkspaceEntry t[GVL_GB_COUNT]; return workspace_bytes(t, glue_workspace(glue_geometry(c, n), t), GVL_WS_TAIL); }
size_t feats_bytes(const gvl_ctx* c, int n) { WorkspaceEntry t[GVL_FB_COUNT]; return workspace_bytes(t, feats_workspace(glue_geometry(c, n), t), GVL_WS_FEATS_TAIL); }

// every entry of a workspace table, in order, from the arena
static int alloc_table(gvl_ctx* ctx, const WorkspaceEntry* t, int n, void** buf) {
  for (int i = 0; i < n; ++i)
    if (!(buf[i] = arena_alloc(ctx, t[i].elem_bytes * t[i].count))) return fail(ctx, GVL_ERR_OOM, std::string("workspace arena too small for ") + t[i].name);
  return 0;
}

// ---------------------------------------------------------------------------------------------------
// What both towers' steps share: the geometry, the plan, the workspace, and the argument structs whose fields the plan decides.
struct TowerSink {
  gvl_ctx* ctx; const VisionGeometry& g; const VisionPlan& p; const float* px; hipStream_t st;
  void* buf[GVL_VB_COUNT] = {};
  const int C = g.C, I = g.inter, H = g.heads, S = g.S, n = g.n, M = g.n * g.S, D = g.D, Dr = g.Dr, NBLK = g.C / 64;
  bf16_t* b16(int i) const { return (bf16_t*)buf[i]; }
  float* f32(int i) const { return (float*)buf[i]; }
  double patch_flops() const { return 2.0 * n * g.rows * (double)C * 3 * g.patch * g.patch; }   // algorithmic flops use the real K = 3*p*p, not the padded one

  PatchEmbedArgs patch_embed_args(const bf16_t* Wt, int mode) const {
    PatchEmbedArgs e; memset(&e, 0, sizeof(e)); e.px = px; e.Wt = Wt; e.n_img = n; e.T = g.T; e.image = g.image; e.patch = g.patch; e.C = C; e.M = n * g.rows; e.S = S; e.mode = mode;
    return e;
  }
  int patchify() { RUN(GVL_PROF_OTHER, 0, gvl_launch_patchify(px, b16(GVL_VB_PA), n, g.T, g.image, g.patch, g.Kp, st)); return 0; }
  QkvPostArgs qkv_post_args(int mode) const {
    QkvPostArgs q; memset(&q, 0, sizeof(q)); q.qkv = b16(GVL_VB_QKV); q.ld = 3 * C; q.Q = b16(GVL_VB_Q); q.Kt = b16(GVL_VB_KT); q.Vt = p.path.vt_pages ? b16(GVL_VB_VT) : nullptr;
    q.B = n; q.S = S; q.H = H; q.KV = H; q.Dr = Dr; q.D = D; q.mode = mode;
    return q;
  }
  AttnArgs attn_args() const {
    const bf16_t* qkv = b16(GVL_VB_QKV);
    AttnArgs a; memset(&a, 0, sizeof(a)); a.Q = b16(GVL_VB_Q); a.Kt = b16(GVL_VB_KT); a.Vt = b16(GVL_VB_VT);
    if (!p.path.vt_pages) { a.Vrows = qkv + 2 * C; a.v_ld = 3 * C; }
    if (p.path.qk_rows) { a.Qrows = qkv; a.Krows = qkv + C; a.q_ld = a.k_ld = 3 * C; }     // q, k, v read by the attention kernel straight from the fused-qkv matrix
    if (p.path.q_on_load) { a.Qrows = qkv; a.q_ld = 3 * C; a.q_rs = f32(GVL_VB_QRS); }     // q read in place, normalised by the attention prologue: no Q write pass
    a.O = b16(GVL_VB_ATT); a.B = n; a.H = H; a.KV = H; a.S = S; a.D = D; a.Dout = Dr; a.scale = 1.0f / sqrtf((float)Dr); a.causal = 0;
    a.ones_row = p.path.attn_ones_row; a.k_ones = p.path.attn_k_ones; a.pipe = p.pipe; a.pipe_rows = p.pipe_rows;
    return a;
  }
  int rowsq_finish() { RUN(GVL_PROF_OTHER, 0, gvl_launch_rowsq_finish(f32(GVL_VB_SQ), NBLK, 0, NBLK, f32(GVL_VB_NRS), M, C, 1e-6f, st)); return 0; }
  int gemm_run(GemmArgs& a, bool rowscale, bool rowsq, double work = -1) {
    if (rowscale) a.rowscale = f32(GVL_VB_NRS);
    if (rowsq) { a.rowsq = f32(GVL_VB_SQ); a.rowsq_ld = NBLK; }
    RUN(GVL_PROF_GEMM, work < 0 ? gvl_gemm_flops(a) : work, gvl_launch_gemm(a, st));
    return 0;
  }
  int strip_cls(void* out, int elem_bytes) { RUN(GVL_PROF_OTHER, 0, gvl_launch_strip_cls(buf[GVL_VB_X], out, n, S, C, elem_bytes, st)); return 0; }
};

// CLIP: the residual stream in f32, LayerNorm passes, biases everywhere, QuickGELU.  (The fused RMSNorm is InternVideo2's: vision_plan never asks for it here.)
struct ClipSink : TowerSink {
  float* out;
  float* x() const { return f32(GVL_VB_X); }
  const ClipLayerW& w(int l) const { return ctx->cl[l]; }
  int patch_embed() {   // ONE kernel: im2col in the operand loader, patch GEMM, CLS + position rows, pre_layrnorm (gvl_patch.hip)
    PatchEmbedArgs e = patch_embed_args(ctx->c_patchwt, 0);
    e.cls_f32 = ctx->c_cls; e.pos_f32 = ctx->c_pos; e.lnw = ctx->c_prelnw; e.lnb = ctx->c_prelnb; e.eps = 1e-5f; e.x_f32 = x();
    RUN(GVL_PROF_GEMM, patch_flops(), gvl_launch_patch_embed(e, st)); return 0;
  }
  int patch_gemm() { GemmArgs a = gemm(b16(GVL_VB_PA), g.Kp, ctx->c_patchw, b16(GVL_VB_PO), C, n * g.rows, C, g.Kp); return gemm_run(a, false, false, patch_flops()); }
  int embed() { RUN(GVL_PROF_OTHER, 0, gvl_launch_clip_embed_ln(b16(GVL_VB_PO), ctx->c_cls, ctx->c_pos, ctx->c_prelnw, ctx->c_prelnb, x(), n, g.rows, C, 1e-5f, st)); return 0; }
  int norm(int l, int which, bool) {
    RUN(GVL_PROF_OTHER, 0, gvl_launch_layernorm_f32(x(), which == 1 ? w(l).ln1w : w(l).ln2w, which == 1 ? w(l).ln1b : w(l).ln2b, b16(GVL_VB_H), M, C, 1e-5f, st)); return 0;
  }
  int qkv(int l, bool) { GemmArgs a = gemm(b16(GVL_VB_H), C, w(l).qkvw, b16(GVL_VB_QKV), 3 * C, M, 3 * C, C); a.bias = w(l).qkvb; return gemm_run(a, false, false); }
  int qkv_post(int) { QkvPostArgs q = qkv_post_args(0); RUN(GVL_PROF_OTHER, 0, gvl_launch_qkv_post(q, st)); return 0; }
  int attention(int) { AttnArgs a = attn_args(); RUN(GVL_PROF_ATTN, gvl_attn_flops(a), gvl_launch_attention(a, st)); return 0; }
  int resid_gemm(const bf16_t* A, int K, const bf16_t* W, const float* bias) {
    GemmArgs a = gemm(A, K, W, x(), C, M, C, K); a.bias = bias; a.resid = x(); a.ldr = C; a.out_f32 = 1; a.round_pre_resid = 1; return gemm_run(a, false, false);
  }
  int proj(int l, bool) { return resid_gemm(b16(GVL_VB_ATT), C, w(l).outw, w(l).outb); }
  int fc1(int l, bool) { GemmArgs a = gemm(b16(GVL_VB_H), C, w(l).fc1w, b16(GVL_VB_MLP), I, M, I, C); a.bias = w(l).fc1b; a.act = GVL_ACT_QUICK_GELU; return gemm_run(a, false, false); }
  int fc2(int l, bool) { return resid_gemm(b16(GVL_VB_MLP), I, w(l).fc2w, w(l).fc2b); }
  int strip_cls() { return TowerSink::strip_cls(out, 4); }
};

// InternVideo2: the residual stream in bf16, RMSNorm passes or their fused form, q / k RMSNorm in qkv_post (or q's on load), LayerScale, erf-GELU.
// (Taking the q / k RMSNorm statistics the fused-norm way -- row sums of squares of the qkv GEMM's 3 C outputs, qkv_post reading k only -- was built and measured a
//  net loss: +0.8 ms of GEMM per clip for the 66 blocks per row, two more small launches per block, and a K pass that is bound by its scattered page writes, not by
//  the q read it lost.  profiles/r05_ab_norm_fused_with_qk_stats.json; removed.)
struct Iv2Sink : TowerSink {
  bf16_t* out;
  bf16_t* x() const { return b16(GVL_VB_X); }
  const Iv2BlockW& w(int l) const { return ctx->vb[l]; }
  int patch_embed() {   // ONE kernel: im2col in the operand loader, patch GEMM + bias, CLS + position rows (gvl_patch.hip)
    PatchEmbedArgs e = patch_embed_args(ctx->v_patchwt, 1);
    e.bias = ctx->v_patchb; e.cls_bf = ctx->v_cls; e.pos_bf = ctx->v_pos; e.x_bf = x();
    RUN(GVL_PROF_GEMM, patch_flops(), gvl_launch_patch_embed(e, st)); return 0;
  }
  int patch_gemm() { GemmArgs a = gemm(b16(GVL_VB_PA), g.Kp, ctx->v_patchw, b16(GVL_VB_PO), C, n * g.rows, C, g.Kp); a.bias = ctx->v_patchb; return gemm_run(a, false, false, patch_flops()); }
  int embed() { RUN(GVL_PROF_OTHER, 0, gvl_launch_iv2_embed(b16(GVL_VB_PO), ctx->v_cls, ctx->v_pos, x(), n, g.rows, C, st)); return 0; }
  int norm(int l, int which, bool fused) {
    if (fused) return rowsq_finish();
    RUN(GVL_PROF_OTHER, 0, gvl_launch_rmsnorm_bf16(x(), which == 1 ? w(l).n1 : w(l).n2, b16(GVL_VB_H), M, C, 1e-6f, st)); return 0;
  }
  int qkv(int l, bool folded) { GemmArgs a = gemm(folded ? x() : b16(GVL_VB_H), C, folded ? w(l).qkvw_f : w(l).qkvw, b16(GVL_VB_QKV), 3 * C, M, 3 * C, C); return gemm_run(a, folded, false); }
  int qkv_post(int l) {
    QkvPostArgs q = qkv_post_args(1);
    q.qn = w(l).qn; q.kn = w(l).kn; q.eps = 1e-6f; q.ones_row = p.path.ones_row; q.k_ones = p.path.k_ones; q.q_rs = p.path.q_on_load ? f32(GVL_VB_QRS) : nullptr;
    RUN(GVL_PROF_OTHER, 0, gvl_launch_qkv_post(q, st)); return 0;
  }
  int attention(int l) {   // head dim 88 padded to 96: the pad row of V^T carries the softmax row sum
    AttnArgs a = attn_args(); if (p.path.q_on_load) a.q_nw = w(l).qn;
    RUN(GVL_PROF_ATTN, gvl_attn_flops(a), gvl_launch_attention(a, st)); return 0;
  }
  int resid_gemm(const bf16_t* A, int K, const bf16_t* W, const float* bias, const float* gamma, bool rowsq) {
    GemmArgs a = gemm(A, K, W, x(), C, M, C, K); a.bias = bias; a.gamma = gamma; a.resid = x(); a.ldr = C; return gemm_run(a, false, rowsq);
  }
  int proj(int l, bool rowsq) { return resid_gemm(b16(GVL_VB_ATT), C, w(l).projw, w(l).projb, w(l).ls1, rowsq); }
  int fc1(int l, bool folded) {
    GemmArgs a = gemm(folded ? x() : b16(GVL_VB_H), C, folded ? w(l).fc1w_f : w(l).fc1w, b16(GVL_VB_MLP), I, M, I, C); a.bias = w(l).fc1b; a.act = GVL_ACT_GELU; return gemm_run(a, folded, false);
  }
  int fc2(int l, bool rowsq) { return resid_gemm(b16(GVL_VB_MLP), I, w(l).fc2w, w(l).fc2b, w(l).ls2, rowsq); }
  int strip_cls() { return TowerSink::strip_cls(out, 2); }
};

template <class Sink, class Out>
static int tower_encode(gvl_ctx* ctx, const VisionGeometry& g, const float* px, Out* out, hipStream_t st) {
  VisionPlan p;
  vision_plan(g, vision_knobs(ctx), &p);
  Sink s{{ctx, g, p, px, st}, out};
  WorkspaceEntry t[GVL_VB_COUNT];
  ArenaScope arena_scope(ctx->arena_off);
  if (int rc = alloc_table(ctx, t, vision_workspace(g, t), s.buf)) return rc;
  return vision_walk(g, p, s);
}
int clip_encode(gvl_ctx* ctx, const float* px, int n, float* out, hipStream_t st) { return tower_encode<ClipSink>(ctx, clip_geometry(ctx, n), px, out, st); }
int iv2_encode(gvl_ctx* ctx, const float* px, int n, bf16_t* out, hipStream_t st) { return tower_encode<Iv2Sink>(ctx, iv2_geometry(ctx, n), px, out, st); }

// ---------------------------------------------------------------------------------------------------
struct GlueSink {
  gvl_ctx* ctx; const GlueGeometry& g; const float* clip_feats; const bf16_t* iv2_feats; bf16_t* visual; hipStream_t st;
  void* buf[GVL_GB_COUNT] = {};
  const int Hd = g.hidden, cin = glue_cin(g), L = g.tok_per_seg, IT = g.img_tok, ST = g.seg_tok, n = g.n;
  bf16_t* b16(int i) const { return (bf16_t*)buf[i]; }
  int run(const GemmArgs& a) { RUN(GVL_PROF_GEMM, gvl_gemm_flops(a), gvl_launch_gemm(a, st)); return 0; }
  int hd_merge() { RUN(GVL_PROF_OTHER, 0, gvl_launch_hd_merge(clip_feats, ctx->sub_gn, b16(GVL_GB_A1), n, g.clip_hidden, st)); return 0; }
  int pool_spatial() { RUN(GVL_PROF_OTHER, 0, gvl_launch_pool_spatial(clip_feats, b16(GVL_GB_A1), n, g.clip_hidden, st)); return 0; }
  int mm0() { GemmArgs a = gemm(b16(GVL_GB_A1), cin, ctx->mm0w, b16(GVL_GB_T1), Hd, n * IT, Hd, cin); a.bias = ctx->mm0b; a.act = GVL_ACT_GELU; return run(a); }
  int mm1() { GemmArgs a = gemm(b16(GVL_GB_T1), Hd, ctx->mm1w, visual, Hd, n * IT, Hd, Hd); a.bias = ctx->mm1b; a.grp_rows = IT; a.grp_stride = L; a.row_off = 0; return run(a); }
  int pool_temporal() { RUN(GVL_PROF_OTHER, 0, gvl_launch_pool_temporal(iv2_feats, b16(GVL_GB_A2), n, g.T, g.iv2_dim, st)); return 0; }
  int vp0() { GemmArgs a = gemm(b16(GVL_GB_A2), g.iv2_dim, ctx->vp0w, b16(GVL_GB_T2), Hd, n * ST, Hd, g.iv2_dim); a.bias = ctx->vp0b; a.act = GVL_ACT_GELU; return run(a); }
  int vp1() { GemmArgs a = gemm(b16(GVL_GB_T2), Hd, ctx->vp1w, visual, Hd, n * ST, Hd, Hd); a.bias = ctx->vp1b; a.grp_rows = ST; a.grp_stride = L; a.row_off = IT; return run(a); }
  // glb_GN through the image projector (llava_next_video.py:560-561); one row, broadcast (App. C #5)
  int glb0() { GemmArgs a = gemm(ctx->glb_gn, cin, ctx->mm0w, b16(GVL_GB_NL1), Hd, 1, Hd, cin); a.bias = ctx->mm0b; a.act = GVL_ACT_GELU; return run(a); }
  int glb1() { GemmArgs a = gemm(b16(GVL_GB_NL1), Hd, ctx->mm1w, b16(GVL_GB_NL2), Hd, 1, Hd, Hd); a.bias = ctx->mm1b; return run(a); }
  int bcast_newline(bool glb) { RUN(GVL_PROF_OTHER, 0, gvl_launch_bcast_row(glb ? b16(GVL_GB_NL2) : ctx->newline, visual, n, L, IT + ST, Hd, st)); return 0; }
};

int build_visual(gvl_ctx* ctx, const float* clip_feats, const bf16_t* iv2_feats, int n, bf16_t* visual, hipStream_t st) {
  const GlueGeometry g = glue_geometry(ctx, n);
  GluePlan p;
  glue_plan(g, &p);
  GlueSink s{ctx, g, clip_feats, iv2_feats, visual, st};
  WorkspaceEntry t[GVL_GB_COUNT];
  ArenaScope arena_scope(ctx->arena_off);
  if (int rc = alloc_table(ctx, t, glue_workspace(g, t), s.buf)) return rc;
  return glue_walk(p, s);
}

}  // namespace gvlm
