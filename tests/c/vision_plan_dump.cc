// Prints the decisions of csrc/gvl_vision_plan.h (host-only) for the cases on stdin: built with the host C++ compiler by tests/vision_plan.py.  Every answer ends with a
// line "end".  One case per line, the first word says which function:
//   T tower n C inter heads S rows Kp Dr D T image patch layers_run patch_tiled folded  patch_fused vision_in_place norm_fused attn_pipe attn_pipe_rows
//     -> "plan patch_fused vt_pages qk_rows q_on_load qkv_post nf pipe pipe_rows n_gemm n_attn n_other" + per block class (first, middle, last) "norm1_pass norm2_pass
//        proj_rowsq fc2_rowsq"; "bytes B" (the workspace sum); per table entry "ws name elem_bytes count"; then one line per launch of vision_walk, as the golden records
//        them: "CATEGORY work launcher arg=value ..." -- pointers by the name of the buffer or weight, zero / null arguments left out
//   G phi n hidden img_tok seg_tok tok_per_seg clip_hidden iv2_dim T P TL
//     -> "plan hd_merge glb_row n_gemm n_attn n_other", "bytes B", "feats_bytes B", "ws ..." per entry of the glue's table, the launch lines of glue_walk
//   P vision_in_place D Dr causal tower   -> "path vt_pages qk_rows q_on_load qkv_post ones_row k_ones attn_ones_row attn_k_ones"
//   F tower n T image patch C M           -> "ok 0|1" (patch_embed_fused_ok)
// The sinks below hold what a step passes to its launcher; the ORDER of the steps is vision_walk's / glue_walk's, shared with gvl_vision.hip through the header.
#include <cmath>
#include <cstdio>
#include <string>
#include "gvl_vision_plan.h"

namespace {
using std::string;
const double GEMM_FLOPS = -1, ATTN_FLOPS = -2;   // the work is gvl_gemm_flops / gvl_attn_flops of the arguments

struct Line {
  string s;
  Line(const char* cat, double work, const char* launcher) {
    char w[64];
    if (work == GEMM_FLOPS) snprintf(w, sizeof w, "gemm_flops");
    else if (work == ATTN_FLOPS) snprintf(w, sizeof w, "attn_flops");
    else if (work == 0) snprintf(w, sizeof w, "-");
    else snprintf(w, sizeof w, "%.17g", work);
    s = string(cat) + " " + w + " " + launcher;
  }
  Line& i(const char* k, long long v) { if (v) s += string(" ") + k + "=" + std::to_string(v); return *this; }
  Line& f(const char* k, float v) { if (v != 0) { char b[64]; snprintf(b, sizeof b, " %s=%.9g", k, (double)v); s += b; } return *this; }
  Line& p(const char* k, const string& name, long long off = 0) { if (!name.empty()) s += string(" ") + k + "=" + name + (off ? "+" + std::to_string(off) : ""); return *this; }
  int out() { printf("%s\n", s.c_str()); return 0; }
};
// GemmArgs as gemm() fills them
Line gemm(const string& A, int lda, const string& W, const string& C, int ldc, int M, int N, int K, double work = GEMM_FLOPS) {
  Line l("GEMM", work, "gvl_launch_gemm");
  return l.p("A", A).i("lda", lda).p("W", W).p("C", C).i("ldc", ldc).i("M", M).i("N", N).i("K", K);
}

struct TowerSink {
  const VisionGeometry& g; const VisionPlan& p;
  const bool clip = g.tower == GVL_TOWER_CLIP;
  const int M = g.n * g.S, C = g.C;
  const float eps = clip ? 1e-5f : 1e-6f;
  string w(int l, const char* name) const { return string(clip ? "cl[" : "vb[") + std::to_string(l) + "]." + name; }
  double patch_flops() const { return 2.0 * g.n * g.rows * (double)C * 3 * g.patch * g.patch; }

  int patch_embed() {
    Line l("GEMM", patch_flops(), "gvl_launch_patch_embed");
    l.p("px", "px").p("Wt", clip ? "c_patchwt" : "v_patchwt").i("n_img", g.n).i("T", g.T).i("image", g.image).i("patch", g.patch).i("C", C).i("M", g.n * g.rows).i("S", g.S).i("mode", clip ? 0 : 1);
    if (clip) l.p("cls_f32", "c_cls").p("pos_f32", "c_pos").p("lnw", "c_prelnw").p("lnb", "c_prelnb").f("eps", 1e-5f).p("x_f32", "x");
    else l.p("bias", "v_patchb").p("cls_bf", "v_cls").p("pos_bf", "v_pos").p("x_bf", "x");
    return l.out();
  }
  int patchify() { return Line("OTHER", 0, "gvl_launch_patchify").p("px", "px").p("A", "pA").i("n_img", g.n).i("T", g.T).i("image", g.image).i("patch", g.patch).i("Kp", g.Kp).out(); }
  int patch_gemm() {
    Line l = gemm("pA", g.Kp, clip ? "c_patchw" : "v_patchw", "pO", C, g.n * g.rows, C, g.Kp, patch_flops());   // the real K = 3 p p, not the padded one
    if (!clip) l.p("bias", "v_patchb");
    return l.out();
  }
  int embed() {
    if (clip) return Line("OTHER", 0, "gvl_launch_clip_embed_ln").p("patch", "pO").p("cls", "c_cls").p("pos", "c_pos").p("lnw", "c_prelnw").p("lnb", "c_prelnb").p("x", "x").i("n_img", g.n).i("P", g.rows).i("C", C).f("eps", 1e-5f).out();
    return Line("OTHER", 0, "gvl_launch_iv2_embed").p("patch", "pO").p("cls", "v_cls").p("pos", "v_pos").p("x", "x").i("B", g.n).i("TL", g.rows).i("C", C).out();
  }
  int norm(int l, int which, bool fused) {
    if (fused) return Line("OTHER", 0, "gvl_launch_rowsq_finish").p("sq", "sq").i("ld", C / 64).i("nblk", C / 64).p("rs", "nrs").i("rows", M).i("cols", C).f("eps", eps).out();
    if (clip) return Line("OTHER", 0, "gvl_launch_layernorm_f32").p("x", "x").p("w", w(l, which == 1 ? "ln1w" : "ln2w")).p("b", w(l, which == 1 ? "ln1b" : "ln2b")).p("y", "h").i("rows", M).i("cols", C).f("eps", eps).out();
    return Line("OTHER", 0, "gvl_launch_rmsnorm_bf16").p("x", "x").p("w", w(l, which == 1 ? "n1" : "n2")).p("y", "h").i("rows", M).i("cols", C).f("eps", eps).out();
  }
  int qkv(int l, bool folded) {
    Line ln = gemm(folded ? "x" : "h", C, w(l, folded ? "qkvw_f" : "qkvw"), "qkv", 3 * C, M, 3 * C, C);
    if (clip) ln.p("bias", w(l, "qkvb"));
    if (folded) ln.p("rowscale", "nrs");
    return ln.out();
  }
  int qkv_post(int l) {
    Line ln("OTHER", 0, "gvl_launch_qkv_post");
    ln.p("qkv", "qkv").i("ld", 3 * C).p("Q", "Q").p("Kt", "Kt").p("Vt", p.path.vt_pages ? "Vt" : "").i("B", g.n).i("S", g.S).i("H", g.heads).i("KV", g.heads).i("Dr", g.Dr).i("D", g.D).i("mode", clip ? 0 : 1);
    if (!clip) ln.p("qn", w(l, "qn")).p("kn", w(l, "kn")).f("eps", eps).i("ones_row", p.path.ones_row).i("k_ones", p.path.k_ones).p("q_rs", p.path.q_on_load ? "qrs" : "");
    return ln.out();
  }
  int attention(int l) {
    Line ln("ATTN", ATTN_FLOPS, "gvl_launch_attention");
    ln.p("Q", "Q").p("Kt", "Kt").p("Vt", "Vt");
    if (!p.path.vt_pages) ln.p("Vrows", "qkv", 2 * C).i("v_ld", 3 * C);
    if (p.path.qk_rows) ln.p("Qrows", "qkv").p("Krows", "qkv", C).i("q_ld", 3 * C).i("k_ld", 3 * C);
    if (p.path.q_on_load) ln.p("Qrows", "qkv").i("q_ld", 3 * C).i("k_ones", p.path.attn_k_ones).p("q_rs", "qrs").p("q_nw", w(l, "qn"));
    ln.p("O", "att").i("B", g.n).i("H", g.heads).i("KV", g.heads).i("S", g.S).i("D", g.D).i("Dout", g.Dr).f("scale", 1.0f / sqrtf((float)g.Dr)).i("ones_row", p.path.attn_ones_row);
    return ln.i("pipe", p.pipe).i("pipe_rows", p.pipe_rows).out();
  }
  Line resid_gemm(const string& A, int K, int l, const char* W, const char* bias, const char* gamma, bool rowsq) {
    Line ln = gemm(A, K, w(l, W), "x", C, M, C, K);
    ln.p("bias", w(l, bias));
    if (!clip) ln.p("gamma", w(l, gamma));
    ln.p("resid", "x").i("ldr", C);
    if (clip) ln.i("out_f32", 1).i("round_pre_resid", 1);
    if (rowsq) ln.p("rowsq", "sq").i("rowsq_ld", C / 64);
    return ln;
  }
  int proj(int l, bool rowsq) { return resid_gemm("att", C, l, clip ? "outw" : "projw", clip ? "outb" : "projb", "ls1", rowsq).out(); }
  int fc1(int l, bool folded) {
    Line ln = gemm(folded ? "x" : "h", C, w(l, folded ? "fc1w_f" : "fc1w"), "mlp", g.inter, M, g.inter, C);
    ln.p("bias", w(l, "fc1b")).i("act", clip ? 1 : 2);
    if (folded) ln.p("rowscale", "nrs");
    return ln.out();
  }
  int fc2(int l, bool rowsq) { return resid_gemm("mlp", g.inter, l, "fc2w", "fc2b", "ls2", rowsq).out(); }
  int strip_cls() { return Line("OTHER", 0, "gvl_launch_strip_cls").p("x", "x").p("y", "out").i("n", g.n).i("S", g.S).i("C", C).i("elem_bytes", clip ? 4 : 2).out(); }
};

struct GlueSink {
  const GlueGeometry& g;
  const int Hd = g.hidden, cin = glue_cin(g), L = g.tok_per_seg, IT = g.img_tok, ST = g.seg_tok;
  int hd_merge() { return Line("OTHER", 0, "gvl_launch_hd_merge").p("f", "clip_feats").p("sub_gn", "sub_gn").p("out", "A1").i("n", g.n).i("C", g.clip_hidden).out(); }
  int pool_spatial() { return Line("OTHER", 0, "gvl_launch_pool_spatial").p("f", "clip_feats").p("out", "A1").i("n", g.n).i("C", g.clip_hidden).out(); }
  int mm0() { return gemm("A1", cin, "mm0w", "T1", Hd, g.n * IT, Hd, cin).p("bias", "mm0b").i("act", 2).out(); }
  int mm1() { return gemm("T1", Hd, "mm1w", "visual", Hd, g.n * IT, Hd, Hd).p("bias", "mm1b").i("grp_rows", IT).i("grp_stride", L).out(); }
  int pool_temporal() { return Line("OTHER", 0, "gvl_launch_pool_temporal").p("f", "iv2_feats").p("out", "A2").i("n", g.n).i("T", g.T).i("C", g.iv2_dim).out(); }
  int vp0() { return gemm("A2", g.iv2_dim, "vp0w", "T2", Hd, g.n * ST, Hd, g.iv2_dim).p("bias", "vp0b").i("act", 2).out(); }
  int vp1() { return gemm("T2", Hd, "vp1w", "visual", Hd, g.n * ST, Hd, Hd).p("bias", "vp1b").i("grp_rows", ST).i("grp_stride", L).i("row_off", IT).out(); }
  int glb0() { return gemm("glb_gn", cin, "mm0w", "nl1", Hd, 1, Hd, cin).p("bias", "mm0b").i("act", 2).out(); }
  int glb1() { return gemm("nl1", Hd, "mm1w", "nl2", Hd, 1, Hd, Hd).p("bias", "mm1b").out(); }
  int bcast_newline(bool glb) { return Line("OTHER", 0, "gvl_launch_bcast_row").p("row", glb ? "nl2" : "newline").p("dst", "visual").i("n", g.n).i("stride_rows", L).i("row_off", IT + ST).i("cols", Hd).out(); }
};

void print_table(const char* tag, const WorkspaceEntry* t, int n) {
  for (int i = 0; i < n; ++i) printf("%s %s %zu %zu\n", tag, t[i].name, t[i].elem_bytes, t[i].count);
}
}  // namespace

int main() {
  char kind;
  int v[21];
  while (scanf(" %c", &kind) == 1) {
    const int want = kind == 'T' ? 21 : kind == 'G' ? 11 : kind == 'P' ? 5 : kind == 'F' ? 7 : -1;
    if (want < 0) return 2;
    for (int i = 0; i < want; ++i) if (scanf("%d", &v[i]) != 1) return 2;
    if (kind == 'T') {
      const VisionGeometry g{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12], v[13], v[14] != 0, v[15] != 0};
      const VisionKnobs k{v[16], v[17], v[18], v[19], v[20]};
      VisionPlan p;
      vision_plan(g, k, &p);
      printf("plan %d %d %d %d %d %d %d %d %d %d %d", p.patch_fused, p.path.vt_pages, p.path.qk_rows, p.path.q_on_load, p.path.qkv_post, p.nf, p.pipe, p.pipe_rows, p.n_gemm, p.n_attn, p.n_other);
      for (const VisionBlockPlan& b : p.block) printf(" %d %d %d %d", b.norm1_pass, b.norm2_pass, b.proj_rowsq, b.fc2_rowsq);
      printf("\n");
      WorkspaceEntry t[GVL_VB_COUNT];
      const int nt = vision_workspace(g, t);
      printf("bytes %zu\n", workspace_bytes(t, nt, GVL_WS_TAIL));
      print_table("ws", t, nt);
      TowerSink s{g, p};
      if (vision_walk(g, p, s)) return 3;
    } else if (kind == 'G') {
      const GlueGeometry g{v[0] != 0, v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10]};
      GluePlan p;
      glue_plan(g, &p);
      printf("plan %d %d %d %d %d\n", p.hd_merge, p.glb_row, p.n_gemm, p.n_attn, p.n_other);
      WorkspaceEntry t[GVL_GB_COUNT], ft[GVL_FB_COUNT];
      const int nt = glue_workspace(g, t), nf = feats_workspace(g, ft);
      printf("bytes %zu\nfeats_bytes %zu\n", workspace_bytes(t, nt, GVL_WS_TAIL), workspace_bytes(ft, nf, GVL_WS_FEATS_TAIL));
      print_table("ws", t, nt);
      GlueSink s{g};
      if (glue_walk(p, s)) return 3;
    } else if (kind == 'P') {
      const VisionOperandPath p = vision_operand_path(v[0], v[1], v[2], v[3] != 0, v[4]);
      printf("path %d %d %d %d %d %d %d %d\n", p.vt_pages, p.qk_rows, p.q_on_load, p.qkv_post, p.ones_row, p.k_ones, p.attn_ones_row, p.attn_k_ones);
    } else {
      printf("ok %d\n", patch_embed_fused_ok(v[0], v[1], v[2], v[3], v[4], v[5], v[6]));
    }
    printf("end\n");
  }
  return 0;
}
