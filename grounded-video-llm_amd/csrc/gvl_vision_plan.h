// gvl_vision_plan.h -- which launches one call of a vision tower (clip_encode, iv2_encode) or of the glue (build_visual) takes, in which order, and the workspace it
// walks them in: PURE host functions of the geometry and of five gvl_debug_set knobs.  Host-only: no HIP header, no statics, no environment -- any C++17 compiler builds
// it (tests/c/vision_plan_dump.cc does, and tests/test_vision_plan_cpu.py pins every launch against recorded ones).  The forms are bit-identical (operand paths, the
// pipelined attention kernel, the fused patch embedding) or equal within the towers' tolerances (fused RMSNorm), so no RESULT test can notice a tower that silently
// lost one: this file is what says which launches ran.  gvl_vision.hip = plan, allocate by the table, walk; what a step passes to its launcher stays there.
#pragma once
#include <cstddef>

enum VisionTower : int { GVL_TOWER_CLIP = 0, GVL_TOWER_IV2 };

// ---- where the attention kernel reads q, k and v ------------------------------------------------------------------------------------------------------------------------
// vision_in_place (gvl_debug_set) 0: q, k and V^T all go through pages written by qkv_post (the round-2 path, bit-identical); 2: V is read as rows of the fused-qkv
// matrix; 1 (default): q and k too where they need no per-token transform (CLIP, head dim 64 = 64: no qkv_post at all), and q normalised as it is loaded where only
// the RMS factor is missing (InternVideo2, 88 in 96).  Causal attention and head dims 97 .. 128 always take V^T pages.  Used by both towers and by gvl_op_attention
// (tower kind CLIP: mode 0, no normalisation).
struct VisionOperandPath {
  bool vt_pages;        // qkv_post writes V^T pages (QkvPostArgs.Vt); false: AttnArgs.Vrows / v_ld read V in place
  bool qk_rows;         // AttnArgs.Qrows / Krows read q and k in place
  bool q_on_load;       // AttnArgs.Qrows / q_rs / q_nw: q read in place and normalised by the attention prologue; qkv_post leaves its RMS factor (QkvPostArgs.q_rs), no Q pass
  bool qkv_post;        // the pass runs
  int ones_row, k_ones; // QkvPostArgs: the pad row of V^T / the pad column of K hold 1.0 (InternVideo2's 88 in 96: the P.V MFMAs deliver the softmax row sum)
  int attn_ones_row, attn_k_ones;   // AttnArgs: what the kernel relies on
};
inline VisionOperandPath vision_operand_path(int vision_in_place, int D, int Dr, bool causal, int tower) {
  VisionOperandPath p{};
  p.vt_pages = !vision_in_place || causal || D == 128;
  p.qk_rows = tower == GVL_TOWER_CLIP && vision_in_place == 1 && !p.vt_pages && D == Dr && D == 64;
  p.q_on_load = tower == GVL_TOWER_IV2 && vision_in_place == 1 && !p.vt_pages && D == 96 && Dr == 88;
  p.qkv_post = !p.qk_rows;
  p.ones_row = p.k_ones = p.attn_ones_row = tower == GVL_TOWER_IV2 && D > Dr;
  p.attn_k_ones = p.q_on_load;
  return p;
}

// ---- the fused patch embedding -------------------------------------------------------------------------------------------------------------------------------------------
// The geometries patch_embed_kernel serves (gvl_patch.hip): 14 x 14 patches, width 1024 or 1408 (CLIP: 1024, one frame), pixel offsets of one call in 32 bits.
// gvl_launch_patch_embed asks this and keeps its pointer checks; the towers ask it through vision_plan, BEFORE anything is booked.
inline bool patch_embed_fused_ok(int tower, long long n_img, int T, int image, int patch, int C, long long M) {
  if (patch != 14 || image % patch || C % 128 || (C != 1024 && C != 1408) || M <= 0 || T <= 0) return false;
  if ((unsigned long long)n_img * 3 * T * image * image >= 0xffffffffull) return false;
  return tower == GVL_TOWER_IV2 || (C == 1024 && T == 1);
}

// ---- a tower's call -------------------------------------------------------------------------------------------------------------------------------------------------------
struct VisionGeometry {   // only what the decisions and the workspace read
  int tower;              // VisionTower
  int n;                  // items of the call (images / segments)
  int C, inter, heads;
  int S, rows;            // tokens per item (1 + rows); patch rows per item (CLIP: P, InternVideo2: T * L)
  int Kp, Dr, D;          // padded im2col width; real and padded head dim
  int T, image, patch;    // frames per item (CLIP: 1)
  int layers_run;
  bool patch_tiled;       // the tile-order patch weight exists (gvl_finalize_weights)
  bool folded;            // the norm-folded qkv / fc1 weights exist
};
struct VisionKnobs { int patch_fused, vision_in_place, norm_fused, attn_pipe, attn_pipe_rows; };   // gvl_debug_set

// Fused RMSNorm (InternVideo2; norm_fused, default on): the two norm passes of a block are gone.  The GEMM that writes the residual stream (proj / fc2) leaves the row
// sums of squares of its bf16 outputs per 64-column block (GemmArgs.rowsq), rowsq_finish turns them into rs[m] = rsqrt(mean + eps), and the consuming GEMM (qkv / fc1)
// reads the RAW stream against the weight with the norm weight folded in and multiplies its accumulator rows by rs (GemmArgs.rowscale).  The widths are the ones the
// staged (whole-row) epilogue takes.  Block 0's first norm has no producer GEMM and keeps the pass; the last block's fc2 has no consumer.
inline bool vision_norm_fused_ok(int tower, bool norm_fused, bool folded, int C, int inter) {
  return tower == GVL_TOWER_IV2 && norm_fused && folded && C % 64 == 0 && (3 * C) % 16 == 0 && inter % 16 == 0;
}
enum VisionBlockClass : int { GVL_VBLOCK_FIRST = 0, GVL_VBLOCK_MIDDLE, GVL_VBLOCK_LAST, GVL_VBLOCK_CLASSES };
inline int vision_block_class(int l, int layers_run) { return l == 0 ? GVL_VBLOCK_FIRST : (l + 1 == layers_run ? GVL_VBLOCK_LAST : GVL_VBLOCK_MIDDLE); }
struct VisionBlockPlan {
  bool norm1_pass, norm2_pass;   // in front of qkv / fc1: the norm pass and the plain weight; false: rowsq_finish, the folded weight and rowscale
  bool proj_rowsq, fc2_rowsq;    // the producer leaves rowsq
};

struct VisionPlan {
  bool patch_fused;              // ONE kernel: im2col in the operand loader, patch GEMM, CLS + position rows (+ CLIP's pre-LayerNorm); false: patchify, GEMM, embed
  VisionOperandPath path;
  bool nf;
  VisionBlockPlan block[GVL_VBLOCK_CLASSES];   // a call of one block runs it as FIRST
  int pipe, pipe_rows;           // AttnArgs: read by the q_on_load form only
  int n_gemm, n_attn, n_other;   // launches the whole call books as GVL_PROF_GEMM / GVL_PROF_ATTN / GVL_PROF_OTHER
};
inline void vision_plan(const VisionGeometry& g, const VisionKnobs& k, VisionPlan* out) {
  VisionPlan p{};
  p.patch_fused = k.patch_fused && g.patch_tiled && patch_embed_fused_ok(g.tower, g.n, g.T, g.image, g.patch, g.C, (long long)g.n * g.rows);
  p.path = vision_operand_path(k.vision_in_place, g.D, g.Dr, false, g.tower);
  p.nf = vision_norm_fused_ok(g.tower, k.norm_fused != 0, g.folded, g.C, g.inter);
  for (int c = 0; c < GVL_VBLOCK_CLASSES; ++c) p.block[c] = VisionBlockPlan{!p.nf || c == GVL_VBLOCK_FIRST, !p.nf, p.nf, p.nf && c != GVL_VBLOCK_LAST};
  p.block[GVL_VBLOCK_FIRST].fc2_rowsq = p.nf && g.layers_run > 1;
  if (p.path.q_on_load) { p.pipe = k.attn_pipe; p.pipe_rows = k.attn_pipe_rows; }
  p.n_gemm = 1 + 4 * g.layers_run;
  p.n_attn = g.layers_run;
  p.n_other = (p.patch_fused ? 0 : 2) + (2 + (p.path.qkv_post ? 1 : 0)) * g.layers_run + 1;
  *out = p;
}
// THE order of a tower's launches: the sink turns a step into its launcher call (gvl_vision.hip) or into a line (tests/c/vision_plan_dump.cc).  A step's non-zero
// result ends the walk and is returned.
template <class Sink>
inline int vision_walk(const VisionGeometry& g, const VisionPlan& p, Sink& s) {
  int rc = 0;
  if (p.patch_fused) rc = s.patch_embed();
  else if (!(rc = s.patchify()) && !(rc = s.patch_gemm())) rc = s.embed();
  for (int l = 0; l < g.layers_run && !rc; ++l) {
    const VisionBlockPlan& b = p.block[vision_block_class(l, g.layers_run)];
    if ((rc = s.norm(l, 1, !b.norm1_pass)) || (rc = s.qkv(l, !b.norm1_pass))) break;
    if (p.path.qkv_post && (rc = s.qkv_post(l))) break;
    if ((rc = s.attention(l)) || (rc = s.proj(l, b.proj_rowsq))) break;
    if ((rc = s.norm(l, 2, !b.norm2_pass)) || (rc = s.fc1(l, !b.norm2_pass))) break;
    rc = s.fc2(l, b.fc2_rowsq);
  }
  return rc ? rc : s.strip_cls();
}

// ---- the glue: both projectors into the visual prefix ------------------------------------------------------------------------------------------------------------------
struct GlueGeometry {
  bool phi;               // llm_kind: Phi-3.5 (HD merge, glb_GN through the image projector) against Llama-3 (3 x 3 pooling, the learned newline row)
  int n, hidden, img_tok, seg_tok, tok_per_seg, clip_hidden, iv2_dim, T;
  int P, TL;              // patch rows per image / per segment (the feature buffers of an encode_segments call)
};
inline int glue_cin(const GlueGeometry& g) { return g.phi ? 4 * g.clip_hidden : g.clip_hidden; }
struct GluePlan {
  bool hd_merge;          // gvl_launch_hd_merge; false: gvl_launch_pool_spatial
  bool glb_row;           // the newline row is glb_GN through mm0 / mm1 (two one-row GEMMs); false: the model's newline row
  int n_gemm, n_attn, n_other;
};
inline void glue_plan(const GlueGeometry& g, GluePlan* out) { *out = GluePlan{g.phi, g.phi, g.phi ? 6 : 4, 0, 3}; }
template <class Sink>
inline int glue_walk(const GluePlan& p, Sink& s) {
  int rc = p.hd_merge ? s.hd_merge() : s.pool_spatial();
  if (rc || (rc = s.mm0()) || (rc = s.mm1()) || (rc = s.pool_temporal()) || (rc = s.vp0()) || (rc = s.vp1())) return rc;
  if (p.glb_row && ((rc = s.glb0()) || (rc = s.glb1()))) return rc;
  return s.bcast_newline(p.glb_row);
}

// ---- the workspace ------------------------------------------------------------------------------------------------------------------------------------------------------
// One table per sequence, a function of the geometry ALONE (gvl_create sizes the arena before any knob is set): the *_bytes functions sum it, the sequences allocate by
// walking it, in this order, each entry at the next multiple of 256 bytes.
struct WorkspaceEntry { const char* name; size_t elem_bytes, count; };
inline size_t workspace_al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t workspace_bytes(const WorkspaceEntry* t, int n, size_t tail) {
  size_t b = tail;
  for (int i = 0; i < n; ++i) b += workspace_al256(t[i].elem_bytes * t[i].count);
  return b;
}
constexpr size_t GVL_WS_TAIL = 4096, GVL_WS_FEATS_TAIL = 1024;

enum VisionBuf : int { GVL_VB_X = 0, GVL_VB_H, GVL_VB_QKV, GVL_VB_ATT, GVL_VB_MLP, GVL_VB_PA, GVL_VB_PO, GVL_VB_Q, GVL_VB_KT, GVL_VB_VT,
                       GVL_VB_QRS, GVL_VB_SQ, GVL_VB_NRS, GVL_VB_COUNT };   // CLIP's table ends in front of QRS
inline int vision_workspace(const VisionGeometry& g, WorkspaceEntry* t) {
  const bool clip = g.tower == GVL_TOWER_CLIP;
  const size_t n = (size_t)g.n, M = n * g.S, C = (size_t)g.C, tiles = ((size_t)g.S + 63) / 64, pages = n * tiles * g.heads * 64 * g.D;
  t[GVL_VB_X] = {"x", clip ? 4u : 2u, M * C};         // the residual stream: f32 in CLIP, bf16 in InternVideo2
  t[GVL_VB_H] = {"h", 2, M * C};
  t[GVL_VB_QKV] = {"qkv", 2, M * 3 * C};
  t[GVL_VB_ATT] = {"att", 2, M * C};
  t[GVL_VB_MLP] = {"mlp", 2, M * g.inter};
  t[GVL_VB_PA] = {"pA", 2, n * g.rows * g.Kp};        // three-pass patch embedding: im2col rows and the patch GEMM's output
  t[GVL_VB_PO] = {"pO", 2, n * g.rows * C};
  t[GVL_VB_Q] = {"Q", 2, n * g.heads * g.S * g.D};
  t[GVL_VB_KT] = {"Kt", 2, pages};
  t[GVL_VB_VT] = {"Vt", 2, pages};
  if (clip) return GVL_VB_QRS;
  t[GVL_VB_QRS] = {"qrs", 4, M};                      // per-token RMS factor of q (q_on_load)
  t[GVL_VB_SQ] = {"sq", 4, M * ((C + 63) / 64)};      // fused RMSNorm: row sums of squares per 64-column block, and the row scale
  t[GVL_VB_NRS] = {"nrs", 4, M};
  return GVL_VB_COUNT;
}
enum GlueBuf : int { GVL_GB_A1 = 0, GVL_GB_T1, GVL_GB_A2, GVL_GB_T2, GVL_GB_NL1, GVL_GB_NL2, GVL_GB_SPARE0, GVL_GB_SPARE1, GVL_GB_COUNT };
inline int glue_workspace(const GlueGeometry& g, WorkspaceEntry* t) {
  const size_t n = (size_t)g.n, cin = (size_t)glue_cin(g), Hd = (size_t)g.hidden;
  t[GVL_GB_A1] = {"A1", 2, n * g.img_tok * cin};
  t[GVL_GB_T1] = {"T1", 2, n * g.img_tok * Hd};
  t[GVL_GB_A2] = {"A2", 2, n * g.seg_tok * g.iv2_dim};
  t[GVL_GB_T2] = {"T2", 2, n * g.seg_tok * Hd};
  // the newline row through mm0 and mm1 (hidden elements each are used), reserved as four rows of hidden + cin since the arena was first sized
  t[GVL_GB_NL1] = {"nl1", 2, Hd + cin};
  t[GVL_GB_NL2] = {"nl2", 2, Hd + cin};
  t[GVL_GB_SPARE0] = {"nl_spare0", 2, Hd + cin};
  t[GVL_GB_SPARE1] = {"nl_spare1", 2, Hd + cin};
  return GVL_GB_COUNT;
}
enum FeatsBuf : int { GVL_FB_CLIP = 0, GVL_FB_IV2, GVL_FB_COUNT };   // encode_segments: both towers' outputs, kept beside the workspace of whichever sequence runs
inline int feats_workspace(const GlueGeometry& g, WorkspaceEntry* t) {
  t[GVL_FB_CLIP] = {"clip_feats", 4, (size_t)g.n * g.P * g.clip_hidden};
  t[GVL_FB_IV2] = {"iv2_feats", 2, (size_t)g.n * g.TL * g.iv2_dim};
  return GVL_FB_COUNT;
}
