// gvl_model.hip -- host side of libgvl.so: context, packed weights, workspace arenas, paged KV pool and the C ABI of include/gvl.h except its token-selection part (gvl_select.hip):
// the towers, splice, the sequence / prefill / decode entry points over the sequence table (gvl_seq_table.h), the operator-level entries.  The launch sequences behind the ABI live in gvl_vision.hip
// (CLIP, InternVideo2, glue / projectors) and gvl_llm.hip (prefill, decode step, decode loop); gvl_model.h is what the four share.  Restates (file:line in the reference):
//   splice          models/llava_next_video.py:568-596
//   generate()      models/llava_next_video.py:655-661 (greedy; transformers GenerationMixin [ext])
#include "gvl_model.h"
#include "gvl_prefill_plan.h"   // prefill_group_size: how the *_varlen entry points cut their sequences into llm_prefill groups
#include "gvl_attn_plan.h"      // decode_attn_plan: gvl_op_decode_attention refuses what the plan refuses, before anything is launched

std::string& gvl_create_error() { static std::string e; return e; }

using namespace gvlm;

namespace {

const Tensor* find(gvl_ctx* c, const std::string& n) { auto it = c->w.find(n); return it == c->w.end() ? nullptr : &it->second; }

template <typename T>
int need(gvl_ctx* c, const std::string& name, int dtype, int64_t numel, const T** out, bool optional = false) {
  const Tensor* t = find(c, name);
  if (!t) { if (optional) { *out = nullptr; return 0; } return fail(c, GVL_ERR_STATE, "missing weight: " + name); }
  if (t->dtype != dtype) return fail(c, GVL_ERR_ARG, "wrong dtype for weight: " + name);
  if (t->numel != numel) return fail(c, GVL_ERR_ARG, "wrong size for weight: " + name + " (have " + std::to_string(t->numel) + ", want " + std::to_string(numel) + ")");
  *out = (const T*)t->p;
  return 0;
}
#define NEED(name, dt, n, outp) do { int _r = need(ctx, name, dt, (int64_t)(n), outp); if (_r) return _r; } while (0)

// paged KV pool: [layer][page][KV][64][D] for K and for V^T, zero-initialised (padded keys / values must be finite)
int alloc_kv_pool(gvl_ctx* ctx, int pages) {
  const gvl_config& f = ctx->cfg;
  ctx->layer_stride = (size_t)pages * f.kv_heads * 64 * ctx->l_D;
  const size_t pool = ctx->layer_stride * f.layers * 2;
  if (hipMalloc((void**)&ctx->kpool, pool) != hipSuccess || hipMalloc((void**)&ctx->vpool, pool) != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, GVL_ERR_OOM, "hipMalloc(kv pool) failed: " + std::to_string(pages) + " pages = " + std::to_string(2 * pool >> 20) + " MiB");
  }
  if (hipMemset(ctx->kpool, 0, pool) != hipSuccess || hipMemset(ctx->vpool, 0, pool) != hipSuccess) return fail(ctx, GVL_ERR_HIP, "hipMemset(kv pool) failed");
  ctx->reset_pool(pages);
  ctx->kv_total_pages = pages;
  return 0;
}
// pages that fit in the HBM still free now (weights and workspaces are resident): `frac` of it, minus a fixed reserve for the
// caller's own tensors (pixels, embeddings, logits) and the runtime
int auto_kv_pages(const gvl_ctx* ctx, double frac, size_t reserve) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return -1;
  const gvl_config& f = ctx->cfg;
  const size_t page_bytes = (size_t)f.kv_heads * 64 * ctx->l_D * 2 /*bf16*/ * 2 /*K and V^T*/ * f.layers;
  double usable = (double)free_b * frac - (double)reserve;
  if (usable < (double)page_bytes) return 1;
  double pages = usable / (double)page_bytes;
  const double cap = (double)gvl_ctx::kMaxSeqs * ((f.max_seq + 63) / 64);   // more than every slot at full context is never reachable
  if (pages > cap) pages = cap;
  return (int)pages;
}

}  // namespace

// =====================================================================================================
// C ABI
// =====================================================================================================
extern "C" {

const char* gvl_last_error(const gvl_ctx* ctx) { return ctx ? ctx->err.c_str() : gvl_create_error().c_str(); }

int gvl_device_info(char* arch_out, int arch_len, int* num_cus) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return GVL_ERR_NOGPU;
  hipDeviceProp_t p; int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) return GVL_ERR_HIP;
  if (arch_out && arch_len > 0) { strncpy(arch_out, p.gcnArchName, arch_len - 1); arch_out[arch_len - 1] = 0; }
  if (num_cus) *num_cus = p.multiProcessorCount;
  return 0;
}

int gvl_create(const gvl_config* cfg, gvl_ctx** out) {
  if (!cfg || !out) return fail(nullptr, GVL_ERR_ARG, "null argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(nullptr, GVL_ERR_NOGPU, "no HIP device: libgvl has no CPU fallback");
  gvl_ctx* ctx = new gvl_ctx();
  ctx->cfg = *cfg;
  const gvl_config& f = ctx->cfg;
  ctx->has_clip = f.clip_hidden > 0 && f.clip_layers_run >= 0 && f.clip_heads > 0;
  ctx->has_iv2 = f.iv2_dim > 0 && f.iv2_heads > 0;
  ctx->has_llm = f.hidden > 0 && f.layers > 0;
  ctx->has_proj = ctx->has_clip && ctx->has_iv2 && f.hidden > 0;
  auto bad = [&](const char* m) { std::string s = m; delete ctx; return fail(nullptr, GVL_ERR_ARG, s); };
  if (ctx->has_clip) {
    if (f.clip_hidden % 64 || f.clip_inter % 64 || f.clip_hidden % f.clip_heads || f.clip_image % f.clip_patch) return bad("clip geometry: hidden/inter must be multiples of 64");
    const int g = f.clip_image / f.clip_patch;
    ctx->c_P = g * g; ctx->c_S = ctx->c_P + 1; ctx->c_Kp = round_up(3 * f.clip_patch * f.clip_patch, 64);
    ctx->c_Dr = f.clip_hidden / f.clip_heads; ctx->c_D = pad_head(ctx->c_Dr);
    if (ctx->c_D < 0 || (ctx->c_Dr & 7)) return bad("clip head dim unsupported");
  }
  if (ctx->has_iv2) {
    if (f.iv2_dim % 64 || f.iv2_inter % 64 || f.iv2_dim % f.iv2_heads || f.iv2_image % f.iv2_patch || f.iv2_frames_per_seg <= 0) return bad("iv2 geometry");
    const int g = f.iv2_image / f.iv2_patch;
    ctx->v_L = g * g; ctx->v_TL = ctx->v_L * f.iv2_frames_per_seg; ctx->v_S = ctx->v_TL + 1; ctx->v_Kp = round_up(3 * f.iv2_patch * f.iv2_patch, 64);
    ctx->v_Dr = f.iv2_dim / f.iv2_heads; ctx->v_D = pad_head(ctx->v_Dr);
    if (ctx->v_D < 0 || (ctx->v_Dr & 7)) return bad("iv2 head dim unsupported");
  }
  if (f.hidden > 0) {
    if (f.hidden % 64) return bad("llm hidden must be a multiple of 64");
    if (ctx->has_llm) {
      if (f.inter % 64 || f.hidden % f.heads || f.heads % f.kv_heads || f.vocab <= 0 || f.max_seq <= 0) return bad("llm geometry");
      ctx->l_Dr = f.hidden / f.heads; ctx->l_D = pad_head(ctx->l_Dr);
      if (ctx->l_D < 0 || (ctx->l_Dr & 15) || ((f.heads * ctx->l_Dr) % 64)) return bad("llm head dim unsupported");
    }
  }
  if (ctx->has_proj) {
    ctx->img_tok = f.llm_kind == GVL_LLM_PHI3 ? 156 : 64;
    ctx->seg_tok = f.iv2_frames_per_seg * 16;
    ctx->tok_per_seg = ctx->img_tok + ctx->seg_tok + 1;
  }
  // workspace arena
  const int ns = f.max_segs > 0 ? f.max_segs : 1;
  size_t need_b = 1 << 20;
  if (ctx->has_clip) need_b = std::max(need_b, clip_bytes(ctx, ns));
  if (ctx->has_iv2) need_b = std::max(need_b, iv2_bytes(ctx, ns));
  if (ctx->has_proj) need_b = std::max(need_b, visual_bytes(ctx, ns));
  if (ctx->has_clip && ctx->has_iv2) need_b += feats_bytes(ctx, ns);
  need_b += 64 << 20;   // slack for the operator-level test entry points
  ctx->arena_bytes = need_b;
  if (hipMalloc((void**)&ctx->arena, need_b) != hipSuccess) { delete ctx; return fail(nullptr, GVL_ERR_OOM, "hipMalloc(arena) failed"); }
  if (ctx->has_llm && f.max_prefill > 0) {
    ctx->arena_l_bytes = prefill_bytes(ctx, f.max_prefill) + (1 << 20);
    if (hipMalloc((void**)&ctx->arena_l, ctx->arena_l_bytes) != hipSuccess) { gvl_destroy(ctx); return fail(nullptr, GVL_ERR_OOM, "hipMalloc(LLM arena) failed"); }
  }
  // KV pool + decode buffers.  cfg.kv_pages > 0: a pool of exactly that many pages, now.  cfg.kv_pages <= 0: the pool is sized from
  // the HBM that is still free once the weights are resident (gvl_finalize_weights) -- "paged KV cache sized for 288 GB".
  if (ctx->has_llm) {
    if (f.kv_pages > 0) { const int rc = alloc_kv_pool(ctx, f.kv_pages); if (rc) { std::string e = ctx->err; gvl_destroy(ctx); return fail(nullptr, rc, e); } }
    const int qkvw = (f.heads + 2 * f.kv_heads) * ctx->l_Dr;
    bool ok = true;
    const size_t NB = GVL_MAX_DECODE_BATCH;
    ok &= hipMalloc((void**)&ctx->d_x, NB * f.hidden * 2) == hipSuccess;
    ok &= hipMalloc((void**)&ctx->d_xn, NB * f.hidden * 2) == hipSuccess;
    ok &= hipMalloc((void**)&ctx->d_seq_ngen, (size_t)gvl_ctx::kMaxSeqs * 4) == hipSuccess;
    ok &= hipHostMalloc((void**)&ctx->h_eos_flags, (size_t)gvl_ctx::kMaxSeqs * 4, hipHostMallocMapped) == hipSuccess;
    if (ok) { memset(ctx->h_eos_flags, 0, (size_t)gvl_ctx::kMaxSeqs * 4); ok &= hipHostGetDevicePointer((void**)&ctx->d_eos_flags, ctx->h_eos_flags, 0) == hipSuccess; }
    for (int i = 0; i < 3 && ok; ++i) ok &= hipEventCreateWithFlags(&ctx->step_ev[i], hipEventDisableTiming) == hipSuccess;
    {   // the skinny-GEMM decode path needs every projection's K to split over 8 waves x 32-wide MFMA steps, and rows that one wave normalises
      const char* e = gvl_lab_env("GVL_DECODE_VALU");
      ctx->decode_mfma = !(e && atoi(e)) && decode_mfma_ok(f.hidden, f.inter, f.heads, ctx->l_Dr);
    }
    ok &= hipMalloc((void**)&ctx->d_qkv, (size_t)qkvw * 2) == hipSuccess;
    ok &= hipMalloc((void**)&ctx->d_q, NB * f.heads * ctx->l_D * 2) == hipSuccess && hipMemset(ctx->d_q, 0, NB * f.heads * ctx->l_D * 2) == hipSuccess;
    ok &= hipMalloc((void**)&ctx->d_attn, NB * f.heads * ctx->l_Dr * 2) == hipSuccess;
    ok &= hipMalloc((void**)&ctx->d_act, NB * f.inter * 2) == hipSuccess;
    ok &= hipMalloc((void**)&ctx->d_logits, NB * f.vocab * 4) == hipSuccess;
    ok &= hipMalloc((void**)&ctx->d_part, NB * f.heads * ctx->nsplit * (ctx->l_D + 2) * 4) == hipSuccess;
    ok &= hipMalloc((void**)&ctx->d_counters, NB * f.heads * 4) == hipSuccess && hipMemset(ctx->d_counters, 0, NB * f.heads * 4) == hipSuccess;
    ok &= hipMalloc((void**)&ctx->d_xt, NB * f.hidden * 2) == hipSuccess && hipMemset(ctx->d_xt, 0, NB * f.hidden * 2) == hipSuccess;
    ok &= hipMalloc((void**)&ctx->d_sqpart, NB * ((f.hidden + 15) / 16) * 4) == hipSuccess && hipMemset(ctx->d_sqpart, 0, NB * ((f.hidden + 15) / 16) * 4) == hipSuccess;
    ok &= hipMalloc((void**)&ctx->d_seq_tok, (size_t)gvl_ctx::kMaxSeqs * 4) == hipSuccess;
    // generated ids live in host-mapped memory: 4 bytes per token cross PCIe as they are produced, and gvl_decode_greedy* / gvl_seq_read read them after
    // their stream sync without a device -> host copy (the step's trace holds no runtime blit kernel)
    ok &= hipHostMalloc((void**)&ctx->h_seq_out, (size_t)gvl_ctx::kMaxSeqs * ctx->outlist_cap * 4, hipHostMallocMapped) == hipSuccess &&
          hipHostGetDevicePointer((void**)&ctx->d_seq_out, ctx->h_seq_out, 0) == hipSuccess;
    ctx->seq_table_cap = (f.max_seq + 63) / 64;
    ok &= hipMalloc((void**)&ctx->d_seq_tables, (size_t)gvl_ctx::kMaxSeqs * ctx->seq_table_cap * 4) == hipSuccess;
    ok &= hipMalloc((void**)&ctx->d_seq_pos, (size_t)gvl_ctx::kMaxSeqs * 4) == hipSuccess;
    if (!ok) { gvl_destroy(ctx); return fail(nullptr, GVL_ERR_OOM, "hipMalloc(decode buffers) failed"); }
  }
  *out = ctx;
  return 0;
}

int gvl_destroy(gvl_ctx* ctx) {
  if (!ctx) return 0;
  hipDeviceSynchronize();
  if (ctx->h_eos_flags) hipHostFree(ctx->h_eos_flags);
  if (ctx->h_seq_out) hipHostFree(ctx->h_seq_out);
  if (ctx->h_beam_cand) hipHostFree(ctx->h_beam_cand);
  if (ctx->h_cs_out) hipHostFree(ctx->h_cs_out);
  for (Seq& q : ctx->seqs) ctx->drop_bank(q);
  for (int i = 0; i < 3; ++i) if (ctx->step_ev[i]) hipEventDestroy(ctx->step_ev[i]);
  for (auto& kv : ctx->w) if (kv.second.p) hipFree(kv.second.p);
  for (void* p : ctx->dw_allocs) if (p) hipFree(p);
  for (void* p : ctx->pw_allocs) if (p) hipFree(p);
  ctx->pw_allocs.clear();
  for (void* p : ctx->nf_allocs) if (p) hipFree(p);
  ctx->nf_allocs.clear();
  if (ctx->comm) gvl_comm_destroy(ctx);
  for (RuleSet& r : ctx->rule_sets) if (r.used && r.d) hipFree(r.d);
  for (GrammarSet& g : ctx->grammars) if (g.used && g.d) hipFree(g.d);
  void* ptrs[] = {ctx->d_xn, ctx->d_seq_ngen, ctx->d_seq_lp, ctx->d_seq_top_ids, ctx->d_seq_top_lp, ctx->arena, ctx->arena_l, ctx->kpool, ctx->vpool, ctx->d_x, ctx->d_qkv, ctx->d_q, ctx->d_attn, ctx->d_act, ctx->d_logits, ctx->d_part, ctx->d_counters, ctx->d_xt, ctx->d_sqpart, ctx->d_seq_tok, ctx->d_seq_tables, ctx->d_seq_pos, ctx->pre_scratch, ctx->d_beam_scratch, ctx->d_beam_rows, ctx->d_beam_hist, ctx->d_cs_scratch};
  for (void* p : ptrs) if (p) hipFree(p);
  for (auto& r : ctx->recs) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
  delete ctx;
  return 0;
}

int gvl_load_weight(gvl_ctx* ctx, const char* name, const void* data, int dtype, const int64_t* shape, int ndim, int is_device) {
  if (!ctx || !name || !data || ndim < 0 || ndim > 8) return fail(ctx, GVL_ERR_ARG, "gvl_load_weight: bad argument");
  if (dtype != GVL_F32 && dtype != GVL_BF16) return fail(ctx, GVL_ERR_ARG, "gvl_load_weight: dtype must be f32 or bf16");
  Tensor t; t.dtype = dtype; t.numel = 1;
  for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); t.numel *= shape[i]; }
  const size_t bytes = (size_t)t.numel * (dtype == GVL_F32 ? 4 : 2);
  auto it = ctx->w.find(name);
  if (it != ctx->w.end()) { hipFree(it->second.p); ctx->w.erase(it); }
  HIPCHK(ctx, hipMalloc(&t.p, bytes ? bytes : 16));
  HIPCHK(ctx, hipMemcpy(t.p, data, bytes, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  ctx->w[name] = t;
  ctx->finalized = false;
  return 0;
}

int gvl_finalize_weights(gvl_ctx* ctx) {
  if (!ctx) return GVL_ERR_ARG;
  const gvl_config& f = ctx->cfg;
  char nm[128];
  if (ctx->has_clip) {
    const int C = f.clip_hidden, I = f.clip_inter;
    NEED("clip.patch.w", GVL_BF16, (int64_t)C * ctx->c_Kp, &ctx->c_patchw);
    NEED("clip.cls", GVL_F32, C, &ctx->c_cls); NEED("clip.pos", GVL_F32, (int64_t)ctx->c_S * C, &ctx->c_pos);
    NEED("clip.preln.w", GVL_F32, C, &ctx->c_prelnw); NEED("clip.preln.b", GVL_F32, C, &ctx->c_prelnb);
    ctx->cl.assign(f.clip_layers_run, ClipLayerW());
    for (int l = 0; l < f.clip_layers_run; ++l) {
      ClipLayerW& w = ctx->cl[l];
#define CN(s) (snprintf(nm, sizeof nm, "clip.L%d." s, l), nm)
      NEED(CN("ln1.w"), GVL_F32, C, &w.ln1w); NEED(CN("ln1.b"), GVL_F32, C, &w.ln1b); NEED(CN("ln2.w"), GVL_F32, C, &w.ln2w); NEED(CN("ln2.b"), GVL_F32, C, &w.ln2b);
      NEED(CN("qkv.w"), GVL_BF16, (int64_t)3 * C * C, &w.qkvw); NEED(CN("qkv.b"), GVL_F32, 3 * C, &w.qkvb);
      NEED(CN("out.w"), GVL_BF16, (int64_t)C * C, &w.outw); NEED(CN("out.b"), GVL_F32, C, &w.outb);
      NEED(CN("fc1.w"), GVL_BF16, (int64_t)I * C, &w.fc1w); NEED(CN("fc1.b"), GVL_F32, I, &w.fc1b);
      NEED(CN("fc2.w"), GVL_BF16, (int64_t)C * I, &w.fc2w); NEED(CN("fc2.b"), GVL_F32, C, &w.fc2b);
#undef CN
    }
  }
  // fused RMSNorm (round 5): the norm weight is folded into the projection that consumes the norm -- W' = bf16(W diag(gamma)), a second copy beside the
  // original (the unfused path, gvl_debug_set("norm_fused", 0), and the decode tile copies keep reading the original).  Memory: the prefill copies are 1.1 GB
  // (InternVideo2-1B) / 5 GB (Phi-3.5) / 9 GB (Llama-3-8B); with bf16 decode weights their decode tile copies and the folded lm_head come on top: ~10 GB
  // (Phi-3.5) / ~18 GB (Llama-3-8B) of the 288 GB in all.  They are an OPTIMISATION: env GVL_NORM_FOLD=0 skips them, and a failed allocation releases every
  // folded copy made so far and carries on -- the launch sequences test the *_f pointers and take the separate norm pass.
  if (!ctx->nf_allocs.empty()) HIPCHK(ctx, hipDeviceSynchronize());
  for (void* p : ctx->nf_allocs) if (p) hipFree(p);
  ctx->nf_allocs.clear();
  bool nf_on = !(getenv("GVL_NORM_FOLD") && atoi(getenv("GVL_NORM_FOLD")) == 0);
  auto nf_give_up = [&]() {                          // out of memory: no folded copy at all (a half-folded model would mix the two rounding orders)
    (void)hipGetLastError();
    (void)hipDeviceSynchronize();                     // fold / retile kernels may still be writing the copies
    for (void* p : ctx->nf_allocs) if (p) hipFree(p);
    ctx->nf_allocs.clear();
    for (auto& w : ctx->vb) w.qkvw_f = w.fc1w_f = nullptr;
    for (auto& w : ctx->ll) w.qkvw_f = w.guw_f = w.qkvd_f = w.gud_f = nullptr;
    ctx->l_headd_f = nullptr;
    nf_on = false;
    fprintf(stderr, "libgvl: no memory for the norm-folded weight copies: RMSNorm runs as separate passes\n");
  };
  auto folded = [&](const bf16_t* W, const bf16_t* gamma, long rows, int cols, const bf16_t** out) -> int {
    if (!nf_on) return 0;
    void* q = nullptr;
    if (hipMalloc(&q, (size_t)rows * cols * 2) != hipSuccess) { nf_give_up(); return 0; }
    ctx->nf_allocs.push_back(q);
    if (gvl_launch_fold_gamma(W, gamma, (bf16_t*)q, rows, cols, nullptr)) return fail(ctx, GVL_ERR_HIP, "fold_gamma launch failed");
    *out = (const bf16_t*)q;
    return 0;
  };
  // fused patch embedding (gvl_patch.hip): tile-order copies of the conv weights, for the geometries the kernel is built for.
  // A repeated finalize frees the previous copies: encodes still in flight on other streams may be reading them -- drain the device first.
  if (!ctx->pw_allocs.empty()) HIPCHK(ctx, hipDeviceSynchronize());
  for (void* p : ctx->pw_allocs) if (p) hipFree(p);
  ctx->pw_allocs.clear(); ctx->c_patchwt = ctx->v_patchwt = nullptr;
  auto patch_tiled = [&](const bf16_t* W, int C, int Kp, int p, int image, const bf16_t** out) -> int {
    if (p != 14 || image % p || (C != 1024 && C != 1408)) return 0;
    void* q = nullptr;
    if (hipMalloc(&q, (size_t)(C / 16) * (3 * p / 2) * 512 * 2) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, GVL_ERR_OOM, "hipMalloc(patch weight copy) failed"); }
    ctx->pw_allocs.push_back(q);
    if (gvl_retile_patch_weight(W, (bf16_t*)q, C, Kp, p, nullptr)) return fail(ctx, GVL_ERR_HIP, "patch weight retile launch failed");
    *out = (const bf16_t*)q;
    return 0;
  };
  if (ctx->has_clip && f.clip_hidden == 1024) { const int rc = patch_tiled(ctx->c_patchw, f.clip_hidden, ctx->c_Kp, f.clip_patch, f.clip_image, &ctx->c_patchwt); if (rc) return rc; }
  if (ctx->has_iv2) {
    const int C = f.iv2_dim, I = f.iv2_inter;
    NEED("iv2.patch.w", GVL_BF16, (int64_t)C * ctx->v_Kp, &ctx->v_patchw); NEED("iv2.patch.b", GVL_F32, C, &ctx->v_patchb);
    { const int rc = patch_tiled(ctx->v_patchw, C, ctx->v_Kp, f.iv2_patch, f.iv2_image, &ctx->v_patchwt); if (rc) return rc; }
    NEED("iv2.cls", GVL_BF16, C, &ctx->v_cls); NEED("iv2.pos", GVL_BF16, (int64_t)ctx->v_S * C, &ctx->v_pos);
    ctx->vb.assign(f.iv2_blocks_run, Iv2BlockW());
    for (int l = 0; l < f.iv2_blocks_run; ++l) {
      Iv2BlockW& w = ctx->vb[l];
#define VN(s) (snprintf(nm, sizeof nm, "iv2.B%d." s, l), nm)
      NEED(VN("n1.w"), GVL_BF16, C, &w.n1); NEED(VN("n2.w"), GVL_BF16, C, &w.n2);
      NEED(VN("qkv.w"), GVL_BF16, (int64_t)3 * C * C, &w.qkvw); NEED(VN("qn.w"), GVL_BF16, C, &w.qn); NEED(VN("kn.w"), GVL_BF16, C, &w.kn);
      NEED(VN("proj.w"), GVL_BF16, (int64_t)C * C, &w.projw); NEED(VN("proj.b"), GVL_F32, C, &w.projb);
      NEED(VN("ls1"), GVL_F32, C, &w.ls1); NEED(VN("ls2"), GVL_F32, C, &w.ls2);
      NEED(VN("fc1.w"), GVL_BF16, (int64_t)I * C, &w.fc1w); NEED(VN("fc1.b"), GVL_F32, I, &w.fc1b);
      NEED(VN("fc2.w"), GVL_BF16, (int64_t)C * I, &w.fc2w); NEED(VN("fc2.b"), GVL_F32, C, &w.fc2b);
#undef VN
      if (C % 64 == 0) {
        int rc = folded(w.qkvw, w.n1, (long)3 * C, C, &w.qkvw_f);
        if (!rc) rc = folded(w.fc1w, w.n2, (long)I, C, &w.fc1w_f);
        if (rc) return rc;
      }
    }
  }
  if (ctx->has_proj) {
    const int Hd = f.hidden; const bool phi = f.llm_kind == GVL_LLM_PHI3; const int cin = phi ? 4 * f.clip_hidden : f.clip_hidden;
    NEED("mm.0.w", GVL_BF16, (int64_t)Hd * cin, &ctx->mm0w); NEED("mm.0.b", GVL_F32, Hd, &ctx->mm0b);
    NEED("mm.1.w", GVL_BF16, (int64_t)Hd * Hd, &ctx->mm1w); NEED("mm.1.b", GVL_F32, Hd, &ctx->mm1b);
    NEED("vp.0.w", GVL_BF16, (int64_t)Hd * f.iv2_dim, &ctx->vp0w); NEED("vp.0.b", GVL_F32, Hd, &ctx->vp0b);
    NEED("vp.1.w", GVL_BF16, (int64_t)Hd * Hd, &ctx->vp1w); NEED("vp.1.b", GVL_F32, Hd, &ctx->vp1b);
    if (phi) { NEED("sub_gn", GVL_F32, cin, &ctx->sub_gn); NEED("glb_gn", GVL_BF16, cin, &ctx->glb_gn); }
    else NEED("newline", GVL_BF16, Hd, &ctx->newline);
  }
  if (ctx->has_llm) {
    const int Hd = f.hidden, I = f.inter, Dr = ctx->l_Dr, qkvw = (f.heads + 2 * f.kv_heads) * Dr;
    NEED("llm.embed", GVL_BF16, (int64_t)f.vocab * Hd, &ctx->l_embed); NEED("llm.norm.w", GVL_BF16, Hd, &ctx->l_norm);
    NEED("llm.head.w", GVL_BF16, (int64_t)f.vocab * Hd, &ctx->l_headw);
    if (f.lm_head_bias) NEED("llm.head.b", GVL_F32, f.vocab, &ctx->l_headb); else ctx->l_headb = nullptr;
    NEED("rope.cos_s", GVL_F32, (int64_t)f.max_seq * (Dr / 2), &ctx->cos_s); NEED("rope.sin_s", GVL_F32, (int64_t)f.max_seq * (Dr / 2), &ctx->sin_s);
    if (f.rope_orig_max_pos > 0) { NEED("rope.cos_l", GVL_F32, (int64_t)f.max_seq * (Dr / 2), &ctx->cos_l); NEED("rope.sin_l", GVL_F32, (int64_t)f.max_seq * (Dr / 2), &ctx->sin_l); }
    else { ctx->cos_l = ctx->sin_l = nullptr; }
    ctx->ll.assign(f.layers, LlmLayerW());
    for (int l = 0; l < f.layers; ++l) {
      LlmLayerW& w = ctx->ll[l];
#define LN(s) (snprintf(nm, sizeof nm, "llm.L%d." s, l), nm)
      NEED(LN("ln1.w"), GVL_BF16, Hd, &w.ln1); NEED(LN("ln2.w"), GVL_BF16, Hd, &w.ln2);
      NEED(LN("qkv.w"), GVL_BF16, (int64_t)qkvw * Hd, &w.qkvw); NEED(LN("o.w"), GVL_BF16, (int64_t)Hd * f.heads * Dr, &w.ow);
      NEED(LN("gu.w"), GVL_BF16, (int64_t)2 * I * Hd, &w.guw); NEED(LN("down.w"), GVL_BF16, (int64_t)Hd * I, &w.downw);
#undef LN
    }
    // decode copies in MFMA tile order (one wave load = 1 KiB of consecutive addresses; the rotate_half row permutation of qkv
    // is baked in): 288 GB of HBM pay for the second copy of the LLM -- the prefill GEMM keeps the row-major one
    for (void* p : ctx->dw_allocs) if (p) hipFree(p);
    ctx->dw_allocs.clear();
    ctx->fp8 = 0;
    if (f.decode_fp8) {
      if (f.decode_fp8 != 1 && f.decode_fp8 != 2) return fail(ctx, GVL_ERR_ARG, "cfg.decode_fp8: 0 = bf16, 1 = FP8 e4m3, 2 = MXFP4");
      if (!ctx->decode_mfma || !decode_quant_ok(f.decode_fp8, Hd, I, f.heads * Dr))
        return fail(ctx, GVL_ERR_ARG, "cfg.decode_fp8 needs hidden, inter and heads*head_dim to be multiples of 512 (FP8) / 1024 (MXFP4) (skinny-GEMM decode path)");
      ctx->fp8 = f.decode_fp8;
    }
    if (ctx->decode_mfma) {
      // bf16: a re-tiled copy.  FP8: per-row scales + the e4m3 tile copy.  MXFP4: E8M0 block scales + the E2M1 tile copy.  In both
      // quantised formats the row-major weight is replaced by its de-quantised values (prefill and decode evaluate ONE model).
      auto tiled = [&](const bf16_t* W, int N, int K, int dr, int nqk, const bf16_t** out, const float** sc_out) -> int {
        void* p = nullptr;
        const size_t n16 = (size_t)((N + 15) / 16) * 16;
        const size_t bytes = ctx->fp8 == 2 ? n16 * K / 2 : n16 * K * (ctx->fp8 ? 1 : 2);
        if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, GVL_ERR_OOM, "hipMalloc(decode weight copy) failed"); }
        ctx->dw_allocs.push_back(p);
        *out = (const bf16_t*)p;
        if (ctx->fp8) {
          void* sc = nullptr;
          const size_t sbytes = ctx->fp8 == 2 ? n16 * (K / 32) : (size_t)N * 4;
          if (hipMalloc(&sc, sbytes) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, GVL_ERR_OOM, "hipMalloc(weight scales) failed"); }
          ctx->dw_allocs.push_back(sc);
          *sc_out = (const float*)sc;
          const int qrc = ctx->fp8 == 2 ? gvl_mxfp4_quantise_decode_weight(const_cast<bf16_t*>(W), (unsigned char*)p, (unsigned*)sc, N, K, dr, nqk, nullptr)
                                        : gvl_fp8_quantise_decode_weight(const_cast<bf16_t*>(W), (unsigned char*)p, (float*)sc, N, K, dr, nqk, nullptr);
          if (qrc) return fail(ctx, GVL_ERR_HIP, "weight quantise launch failed");
        } else {
          *sc_out = nullptr;
          if (gvl_retile_decode_weight(W, (bf16_t*)p, N, K, dr, nqk, nullptr)) return fail(ctx, GVL_ERR_HIP, "retile launch failed");
        }
        return 0;
      };
      for (int l = 0; l < f.layers; ++l) {
        LlmLayerW& w = ctx->ll[l];
        int rc = tiled(w.qkvw, qkvw, Hd, Dr, f.heads + f.kv_heads, &w.qkvd, &w.qkvs);
        if (!rc) rc = tiled(w.ow, Hd, f.heads * Dr, 0, 0, &w.od, &w.os);
        if (!rc) rc = tiled(w.guw, 2 * I, Hd, 0, 0, &w.gud, &w.gus);
        if (!rc) rc = tiled(w.downw, Hd, I, 0, 0, &w.downd, &w.downs);
        if (rc) return rc;
      }
      { const int rc = tiled(ctx->l_headw, f.vocab, Hd, 0, 0, &ctx->l_headd, &ctx->l_heads); if (rc) return rc; }
    }
    // norm-folded prefill weights LAST: the quantised decode formats above replace the row-major weights by their de-quantised values (same stream, in
    // order), and the fused-RMSNorm prefill must evaluate that same model
    if (Hd % 64 == 0) {
      for (int l = 0; l < f.layers; ++l) {
        LlmLayerW& w = ctx->ll[l];
        int rc = folded(w.qkvw, w.ln1, (long)qkvw, Hd, &w.qkvw_f);
        if (!rc) rc = folded(w.guw, w.ln2, (long)2 * I, Hd, &w.guw_f);
        if (rc) return rc;
      }
      // the decode path's copies of the folded weights (bf16 decode weights only: a quantised format would quantise gamma * W, another model than
      // the prefill's): tile order like every decode weight; plus lm_head with the final norm weight
      ctx->l_headd_f = nullptr;
      if (ctx->decode_mfma && !ctx->fp8 && nf_on) {
        auto tiled_f = [&](const bf16_t* W, int N, int K, int dr, int nqk, const bf16_t** out) -> int {
          if (!nf_on || !W) return 0;
          void* p = nullptr;
          if (hipMalloc(&p, (size_t)((N + 15) / 16) * 16 * K * 2) != hipSuccess) { nf_give_up(); return 0; }
          ctx->nf_allocs.push_back(p);
          if (gvl_retile_decode_weight(W, (bf16_t*)p, N, K, dr, nqk, nullptr)) return fail(ctx, GVL_ERR_HIP, "retile launch failed");
          *out = (const bf16_t*)p;
          return 0;
        };
        for (int l = 0; l < f.layers; ++l) {
          LlmLayerW& w = ctx->ll[l];
          int rc = tiled_f(w.qkvw_f, qkvw, Hd, Dr, f.heads + f.kv_heads, &w.qkvd_f);
          if (!rc) rc = tiled_f(w.guw_f, 2 * I, Hd, 0, 0, &w.gud_f);
          if (rc) return rc;
        }
        const bf16_t* headf = nullptr;
        int rc = folded(ctx->l_headw, ctx->l_norm, (long)f.vocab, Hd, &headf);
        if (!rc) rc = tiled_f(headf, f.vocab, Hd, 0, 0, &ctx->l_headd_f);
        if (rc) return rc;
      }
    }
  }
  // the retile kernels above (patch weights, decode tile copies) ran on the null stream: a first encode / decode on a NON-blocking stream (torch pool
  // streams, the bench's sV / sL) is not ordered behind them -- finalize returns only when every derived copy is complete
  HIPCHK(ctx, hipDeviceSynchronize());
  if (ctx->has_llm && !ctx->kpool) {          // cfg.kv_pages <= 0: size the pool from what is free NOW (weights resident)
    const char* fe = getenv("GVL_KV_FRACTION");
    const double frac = fe ? atof(fe) : 0.85;
    const int pages = auto_kv_pages(ctx, frac > 0 && frac <= 1 ? frac : 0.85, (size_t)4 << 30);
    if (pages <= 0) return fail(ctx, GVL_ERR_HIP, "hipMemGetInfo failed");
    const int rc = alloc_kv_pool(ctx, pages);
    if (rc) return rc;
  }
  ctx->finalized = true;
  return 0;
}

int gvl_clip_encode(gvl_ctx* ctx, const float* px, int n, float* out, void* stream) {
  REQUIRE_READY(ctx->has_clip, "gvl_clip_encode");
  if (!px || !out || n <= 0 || n > std::max(1, ctx->cfg.max_segs)) return fail(ctx, GVL_ERR_ARG, "gvl_clip_encode: bad n/pointers");
  return clip_encode(ctx, px, n, out, (hipStream_t)stream);
}
int gvl_iv2_encode(gvl_ctx* ctx, const float* px, int n, uint16_t* out, void* stream) {
  REQUIRE_READY(ctx->has_iv2, "gvl_iv2_encode");
  if (!px || !out || n <= 0 || n > std::max(1, ctx->cfg.max_segs)) return fail(ctx, GVL_ERR_ARG, "gvl_iv2_encode: bad n/pointers");
  return iv2_encode(ctx, px, n, out, (hipStream_t)stream);
}
int gvl_tokens_per_seg(const gvl_ctx* ctx) { return ctx ? ctx->tok_per_seg : 0; }
int gvl_build_visual(gvl_ctx* ctx, const float* clip_feats, const uint16_t* iv2_feats, int n, uint16_t* visual, void* stream) {
  REQUIRE_READY(ctx->has_proj, "gvl_build_visual");
  if (!clip_feats || !iv2_feats || !visual || n <= 0 || n > std::max(1, ctx->cfg.max_segs)) return fail(ctx, GVL_ERR_ARG, "gvl_build_visual: bad n/pointers");
  if (ctx->c_P != 576) return fail(ctx, GVL_ERR_ARG, "gvl_build_visual: needs the 24x24 CLIP grid (llava_next_video.py:460)");
  if (ctx->v_L != 256) return fail(ctx, GVL_ERR_ARG, "gvl_build_visual: needs the 16x16 InternVideo2 grid");
  return build_visual(ctx, clip_feats, iv2_feats, n, visual, (hipStream_t)stream);
}
int gvl_encode_segments(gvl_ctx* ctx, const float* spatial_px, const float* temporal_px, int n, uint16_t* visual, void* stream) {
  REQUIRE_READY(ctx->has_proj, "gvl_encode_segments");
  if (!spatial_px || !temporal_px || !visual || n <= 0 || n > std::max(1, ctx->cfg.max_segs)) return fail(ctx, GVL_ERR_ARG, "gvl_encode_segments: bad n/pointers");
  hipStream_t st = (hipStream_t)stream;
  ArenaScope arena_scope(ctx->arena_off);
  AALLOC(cf, float, (size_t)n * ctx->c_P * ctx->cfg.clip_hidden);
  AALLOC(vf, bf16_t, (size_t)n * ctx->v_TL * ctx->cfg.iv2_dim);
  int rc = clip_encode(ctx, spatial_px, n, cf, st);
  if (!rc) rc = iv2_encode(ctx, temporal_px, n, vf, st);
  if (!rc) rc = gvl_build_visual(ctx, cf, vf, n, visual, stream);
  return rc;
}

int gvl_splice(gvl_ctx* ctx, const int64_t* ids, int n_ids, const uint16_t* visual, int n_visual, uint16_t* embeds, int* seq_len_out, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_splice");
  if (!ids || (!visual && n_visual > 0) || !embeds || n_ids <= 0 || n_visual < 0 || n_ids > ctx->ids_cap) return fail(ctx, GVL_ERR_ARG, "gvl_splice: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  int idx = -1, cnt = 0;
  std::vector<int> text; text.reserve(n_ids);
  for (int i = 0; i < n_ids; ++i) {
    if (ids[i] == -200) { if (idx < 0) idx = i; ++cnt; }
    else { if (ids[i] < 0 || ids[i] >= ctx->cfg.vocab) return fail(ctx, GVL_ERR_ARG, "gvl_splice: token id out of range"); text.push_back((int)ids[i]); }
  }
  if (cnt != 1) return fail(ctx, GVL_ERR_ARG, "gvl_splice: exactly one IMAGE_TOKEN_INDEX (-200) expected");
  const int Hd = ctx->cfg.hidden, n_post = n_ids - 1 - idx;
  // ids travel by value in the kernel arguments: stream ordered, nothing shared between back-to-back splices
  RUN(GVL_PROF_OTHER, 0, gvl_launch_gather_rows_host_ids(ctx->l_embed, text.data(), idx, embeds, Hd, st));
  if (n_visual > 0) RUN(GVL_PROF_OTHER, 0, gvl_launch_copy_bytes(visual, embeds + (size_t)idx * Hd, (size_t)n_visual * Hd * 2, st));
  RUN(GVL_PROF_OTHER, 0, gvl_launch_gather_rows_host_ids(ctx->l_embed, text.data() + idx, n_post, embeds + (size_t)(idx + n_visual) * Hd, Hd, st));
  if (seq_len_out) *seq_len_out = n_ids - 1 + n_visual;
  return 0;
}

// Slot `id`'s views of the preallocated device-side tables: no hipMalloc / hipFree / device-wide sync per clip.  Work that uses the slot is stream
// ordered; a freed slot or page may be handed out again only for work enqueued later on the same stream (one stream per ctx for the LLM path -- the
// reference is single-stream too).
static void bind_slot(gvl_ctx* ctx, Seq& s, int id) {
  s.d_block_table = ctx->d_seq_tables + (size_t)id * ctx->seq_table_cap;
  s.d_pos = ctx->d_seq_pos + id;
  s.d_tok = ctx->d_seq_tok + id;
  s.d_out = ctx->d_seq_out + (size_t)id * ctx->outlist_cap; s.h_out = ctx->h_seq_out + (size_t)id * ctx->outlist_cap;
  s.d_ngen = ctx->d_seq_ngen + id;
  bind_logprobs(ctx, s, id);
  s.d_eos = ctx->d_eos_flags + id; s.h_eos = ctx->h_eos_flags + id;
  s.table_dirty = true;                               // written by the first prefill / decode on ITS stream (upload_table); d_pos likewise
}

int gvl_seq_alloc(gvl_ctx* ctx, int max_tokens, int* seq_id) {
  REQUIRE_READY(ctx->has_llm, "gvl_seq_alloc");
  if (max_tokens <= 0 || !seq_id) return fail(ctx, GVL_ERR_ARG, "gvl_seq_alloc: bad arguments");
  if (max_tokens > ctx->cfg.max_seq) return fail(ctx, GVL_ERR_ARG, "gvl_seq_alloc: max_tokens exceeds cfg.max_seq (rope tables)");
  const int id = ctx->open(max_tokens, -1, 0);
  if (id < 0) return seq_fail(ctx, "gvl_seq_alloc", id);
  bind_slot(ctx, ctx->seqs[id], id);
  *seq_id = id;
  return 0;
}
int gvl_seq_free(gvl_ctx* ctx, int seq_id) {
  return seq_fail(ctx, "gvl_seq_free", ctx ? ctx->close(seq_id) : (int)SEQ_BAD);
}
int gvl_seq_fork(gvl_ctx* ctx, int src_seq, int n_tokens, int max_tokens, int* dst_seq) {
  REQUIRE_READY(ctx->has_llm, "gvl_seq_fork");
  if (!dst_seq || !ctx->lookup(src_seq)) return fail(ctx, GVL_ERR_ARG, "gvl_seq_fork: bad arguments");
  if (const int rc = pair_refuse(ctx, "gvl_seq_fork", src_seq, true)) return rc;
  if (const int rc = bank_refuse(ctx, "gvl_seq_fork", src_seq)) return rc;
  if (n_tokens <= 0 || (n_tokens & 63) || n_tokens > ctx->seqs[src_seq].pos) return fail(ctx, GVL_ERR_ARG, "gvl_seq_fork: n_tokens must be a positive multiple of 64 within the source's tokens");
  if (max_tokens <= n_tokens || max_tokens > ctx->cfg.max_seq) return fail(ctx, GVL_ERR_ARG, "gvl_seq_fork: max_tokens must exceed n_tokens and fit cfg.max_seq");
  if (ctx->fork_cuts_answer(ctx->seqs[src_seq], n_tokens))
    return fail(ctx, GVL_ERR_STATE, "gvl_seq_fork: the source has a grammar and the prefix holds ids it generated; the rows appended behind a fork are embeddings, so its walk "
                                    "could not continue (fork within the prompt, gvl_seq_clone, or gvl_seq_set_grammar(src, -1) first)");
  const int id = ctx->open(max_tokens, src_seq, n_tokens);
  if (id < 0) return seq_fail(ctx, "gvl_seq_fork", id);
  bind_slot(ctx, ctx->seqs[id], id);
  *dst_seq = id;
  return 0;
}

int gvl_prefill(gvl_ctx* ctx, int seq_id, const uint16_t* embeds, int S, float* last_logits, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_prefill");
  if (!embeds) return fail(ctx, GVL_ERR_ARG, "gvl_prefill: bad length");
  if (const int rc = admit(ctx, gvl_admit::PREFILL, &seq_id, 1, &S, 0)) return rc;
  Seq& sq = ctx->seqs[seq_id];
  hipStream_t st = (hipStream_t)stream;
  Seq* one[1] = {&sq}; const bf16_t* e1[1] = {embeds};
  int rc = llm_prefill(ctx, one, 1, e1, &S, st, nullptr, nullptr, nullptr, sq.bank != nullptr);   // a keep-hidden sequence: the bank takes one row per prompt row
  if (rc) return rc;
  if (last_logits) HIPCHK(ctx, hipMemcpyAsync(last_logits, ctx->d_logits, (size_t)ctx->cfg.vocab * 4, hipMemcpyDeviceToDevice, st));
  return 0;
}

int gvl_seq_clone(gvl_ctx* ctx, int src_seq, int max_tokens, int* dst_seq, void* stream) {
  // A source with a grammar hands its answer so far to the clone: the mask is a function of the generated ids, so without them the clone's walk would start over
  // mid-answer.  Without a grammar a clone's history starts empty, as ever.
  return seq_clone(ctx, src_seq, max_tokens, dst_seq, (hipStream_t)stream, true);
}

// The device side of n new copies of `src_seq` at its length `pos` (gvl_seq_fanout's siblings, seq_clone_many's clones; ids[] from SeqTable::open_many): slots bound, the
// block tables up -- one launch each, by value, on the call's stream: ordered behind the source's pending work there --, then ONE launch for the n private copies of the
// partial last page (all layers, K and V^T; none when pos ends on a page boundary).  fa: the copies' position and count pointers, for the caller's own launch behind
static int bind_copies(gvl_ctx* ctx, int src_seq, int pos, const int* ids, int n, FanoutArgs& fa, Seq** sqs, hipStream_t st) {
  memset(&fa, 0, sizeof(fa)); fa.n = n;
  for (int i = 0; i < n; ++i) {                           // after the last open(): `seqs` no longer moves
    Seq& s = ctx->seqs[ids[i]];
    bind_slot(ctx, s, ids[i]);
    sqs[i] = &s; fa.pos[i] = s.d_pos; fa.ngen[i] = s.d_ngen;
    if (pos & 63) fa.dst_page[i] = s.pages[pos >> 6];
  }
  for (int i = 0; i < n; ++i) { const int rc = upload_table(ctx, *sqs[i], st); if (rc) return rc; }
  if (pos & 63)
    RUN(GVL_PROF_OTHER, 0, gvl_launch_kv_page_fanout(ctx->kpool, ctx->vpool, ctx->layer_stride, (size_t)ctx->cfg.kv_heads * 64 * ctx->l_D, ctx->cfg.layers, ctx->kv_total_pages,
                                                     ctx->seqs[src_seq].pages[pos >> 6], fa, st));
  return 0;
}

// n_new siblings of a freshly prefilled sequence: n answers to one prompt from ONE prefill.  The table operation opens all of them or none (SeqTable::fanout); behind it
// three launches serve every sibling at once -- the partial last page (kv_page_fanout_kernel; none when the prompt ends on a page boundary), positions, counters and the
// logits rows (fanout_rows_kernel), and the first tokens (select_tokens: warpers and draw only -- first_logits is the row the source's prefill PROCESSED, and at step 0
// every sibling's processed row is that row).  Everything is checked before the first launch.
int gvl_seq_fanout(gvl_ctx* ctx, int src_seq, int n_new, int max_tokens, const uint32_t* streams, float* first_logits, int* dst_seqs, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_seq_fanout");
  if (!streams || !first_logits || !dst_seqs) return fail(ctx, GVL_ERR_ARG, "gvl_seq_fanout: streams, first_logits and dst_seqs are needed");
  if (!ctx->lookup(src_seq)) return seq_fail(ctx, "gvl_seq_fanout", SEQ_BAD);
  if (const int rc = bank_refuse(ctx, "gvl_seq_fanout", src_seq)) return rc;
  if (n_new < 1 || n_new > GVL_MAX_DECODE_BATCH - 1) return fail(ctx, GVL_ERR_ARG, "gvl_seq_fanout: n_new must be 1 .. " + std::to_string(GVL_MAX_DECODE_BATCH - 1) + " (repeat the call for more)");
  const int pos = ctx->seqs[src_seq].pos, V = ctx->cfg.vocab;
  if (max_tokens <= pos || max_tokens > ctx->cfg.max_seq) return fail(ctx, GVL_ERR_ARG, "gvl_seq_fanout: max_tokens must exceed the source's tokens and fit cfg.max_seq");
  if (first_logits >= ctx->d_logits && first_logits < ctx->d_logits + (size_t)GVL_MAX_DECODE_BATCH * V && (first_logits - ctx->d_logits) % V != 0)
    return fail(ctx, GVL_ERR_ARG, "gvl_seq_fanout: first_logits overlaps the library's work rows");
  Sampling followed;                                  // the ctx setting as a sequence's own (the stream is the sibling's)
  { const auto& q = ctx->sample;
    followed.on = q.on; followed.inv_temp = q.inv_temp; followed.top_k = q.top_k; followed.top_p = q.top_p; followed.min_p = q.min_p; followed.typical_p = q.typical_p;
    followed.eps = q.eps; followed.eta = q.eta; followed.seed = q.seed; }
  int ids[GVL_MAX_DECODE_BATCH];
  { const int rc = ctx->fanout(src_seq, n_new, max_tokens, followed, streams, ids); if (rc < 0) return seq_fail(ctx, "gvl_seq_fanout", rc); }
  hipStream_t st = (hipStream_t)stream;
  Seq* sqs[GVL_MAX_DECODE_BATCH]; FanoutArgs fa;
  if (const int rc = bind_copies(ctx, src_seq, pos, ids, n_new, fa, sqs, st)) return rc;
  RUN(GVL_PROF_OTHER, 0, gvl_launch_fanout_rows(first_logits, ctx->d_logits, V, pos, fa, st));
  ArgmaxArgs am; memset(&am, 0, sizeof(am)); am.logits = ctx->d_logits; am.n = V; am.batch = n_new;
  for (int i = 0; i < n_new; ++i) { am.tok_ptrs[i] = sqs[i]->d_tok; am.out_lists[i] = sqs[i]->d_out; am.ngen_ptrs[i] = sqs[i]->d_ngen; }
  RUN(GVL_PROF_OTHER, 0, select_tokens(ctx, am, sqs, st));
  for (int i = 0; i < n_new; ++i) dst_seqs[i] = ids[i];
  return 0;
}
}  // extern "C"

// the bank of `s`: rows for `cap` positions, all or nothing
int gvlm::bank_alloc(gvl_ctx* ctx, Seq& s, int cap) {
  const int Hd = ctx->cfg.hidden;
  if (Hd % 64 || Hd > 8192) return fail(ctx, GVL_ERR_ARG, "gvl_seq_keep_hidden: hidden must be a multiple of 64 and <= 8192");
  ctx->drop_bank(s);
  const size_t row_bytes = al256((size_t)cap * Hd * 2);
  void* p = nullptr;
  if (hipMalloc(&p, row_bytes + (size_t)cap * 4) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, GVL_ERR_OOM, "gvl_seq_keep_hidden: no device memory for the hidden bank"); }
  s.bank = (bf16_t*)p; s.bank_inv = (float*)((char*)p + row_bytes); s.bank_cap = cap; s.bank_rows = 0;
  return 0;
}

int gvlm::seq_clone(gvl_ctx* ctx, int src_seq, int max_tokens, int* dst_seq, hipStream_t stream, bool carry) {
  REQUIRE_READY(ctx->has_llm, "gvl_seq_clone");
  if (!dst_seq) return fail(ctx, GVL_ERR_ARG, "gvl_seq_clone: bad arguments");
  if (const int rc = admit(ctx, carry ? gvl_admit::SEQ_CLONE : gvl_admit::SEQ_CLONE_PLAIN, &src_seq, 1, &max_tokens, 0)) return rc;
  const int pos = ctx->seqs[src_seq].pos;
  const bool carry_generated = carry && ctx->seqs[src_seq].sel.grammar >= 0, carry_bank = carry && ctx->seqs[src_seq].bank;
  const int id = ctx->open(max_tokens, src_seq, pos);
  if (id < 0) return seq_fail(ctx, "gvl_seq_clone", id);
  Seq& s = ctx->seqs[id];
  bind_slot(ctx, s, id);
  hipStream_t st = stream;
  if (carry_bank) {                                   // a keep-hidden source: the clone keeps its own copy of the rows so far
    if (const int rc = bank_alloc(ctx, s, max_tokens)) { ctx->close(id); return rc; }
    const Seq& b = ctx->seqs[src_seq];
    RUN(GVL_PROF_OTHER, 0, gvl_launch_copy_bytes(b.bank, s.bank, (size_t)pos * ctx->cfg.hidden * 2, st));
    RUN(GVL_PROF_OTHER, 0, gvl_launch_copy_bytes(b.bank_inv, s.bank_inv, (size_t)pos * 4, st));
    s.bank_rows = pos;
  }
  { const int rc = upload_table(ctx, s, st); if (rc) return rc; }   // by value, on the clone's stream: ordered behind the source's pending steps there
  if (pos & 63)                                       // the partial last page is private: copy the source's (all layers, K and V^T)
    RUN(GVL_PROF_OTHER, 0, gvl_launch_kv_page_copy(ctx->kpool, ctx->vpool, ctx->layer_stride, (size_t)ctx->cfg.kv_heads * 64 * ctx->l_D, ctx->cfg.layers,
                                                   ctx->seqs[src_seq].pages[pos >> 6], s.pages[pos >> 6], st));
  RUN(GVL_PROF_OTHER, 0, gvl_launch_set_int(s.d_pos, pos, st));
  const Seq& from = ctx->seqs[src_seq];
  const int n = carry_generated ? from.n_gen : 0;
  if (n > 0) {   // the ids generated so far, the one to feed next and, where the source keeps them, their log-probabilities: the clone stands where the source stands
    RUN(GVL_PROF_OTHER, 0, gvl_launch_copy_ints(from.d_out, s.d_out, n, st));
    RUN(GVL_PROF_OTHER, 0, gvl_launch_copy_ints(from.d_tok, s.d_tok, 1, st));
    if (from.sel.top_n >= 0 && from.d_lp && s.d_lp) {   // (floats travel as their 4-byte words)
      RUN(GVL_PROF_OTHER, 0, gvl_launch_copy_ints((const int*)from.d_lp, (int*)s.d_lp, n, st));
      if (from.sel.top_n > 0) {
        RUN(GVL_PROF_OTHER, 0, gvl_launch_copy_ints(from.d_top_ids, s.d_top_ids, n * GVL_MAX_TOP_LOGPROBS, st));
        RUN(GVL_PROF_OTHER, 0, gvl_launch_copy_ints((const int*)from.d_top_lp, (int*)s.d_top_lp, n * GVL_MAX_TOP_LOGPROBS, st));
      }
    }
  }
  RUN(GVL_PROF_OTHER, 0, gvl_launch_set_int(s.d_ngen, n, st));
  s.n_gen = n;
  *dst_seq = id;
  return 0;
}
// n plain clones of `src_seq` at its current length for gvl_contrastive_search's candidates (no bank, empty histories): what n seq_clone calls give, but all or
// nothing -- pages and slots are counted before the first one opens -- and with ONE launch for the n private copies of the partial last page (gvl_seq_fanout's) and ONE
// for the positions and generation counts; the block tables still go up one launch each (page ids travel by value).
__global__ void clone_counters_kernel(const FanoutArgs a, int pos) { if ((int)threadIdx.x < a.n) { *a.pos[threadIdx.x] = pos; *a.ngen[threadIdx.x] = 0; } }
int gvlm::seq_clone_many(gvl_ctx* ctx, int src_seq, int max_tokens, int n, int* dst_seqs, hipStream_t st) {
  REQUIRE_READY(ctx->has_llm, "gvl_seq_clone");
  if (!dst_seqs || n < 1 || n > GVL_MAX_DECODE_BATCH) return fail(ctx, GVL_ERR_ARG, "gvl_seq_clone: bad arguments");
  if (const int rc = admit(ctx, gvl_admit::SEQ_CLONE_PLAIN, &src_seq, 1, &max_tokens, 0)) return rc;
  if (const int rc = ctx->open_many(src_seq, n, max_tokens, dst_seqs)) return seq_fail(ctx, "gvl_seq_clone", rc);
  const int pos = ctx->seqs[src_seq].pos;
  Seq* sqs[GVL_MAX_DECODE_BATCH]; FanoutArgs fa;
  int rc = bind_copies(ctx, src_seq, pos, dst_seqs, n, fa, sqs, st);
  if (!rc) {
    hipLaunchKernelGGL(clone_counters_kernel, dim3(1), dim3(64), 0, st, fa, pos);
    if (hipGetLastError() != hipSuccess) rc = fail(ctx, GVL_ERR_HIP, "gvl_seq_clone: launch failed");
  }
  if (rc) for (int i = 0; i < n; ++i) ctx->close(dst_seqs[i]);   // all or nothing on a failed launch too
  return rc;
}
// The ragged prefill entries: every member's operands are there (`what`: the text behind "bad "; the same text as for a member that is no live sequence), and the walk
// over their groups -- up to `cap` members in call order, as many as the prefill workspace (cfg.max_prefill rows in total) allows; run(first member, B, sqs, embeds, pos0)
static int members_present(gvl_ctx* ctx, const char* fn, const char* what, int n_seqs, const void* const* operands, const void* const* operands2 = nullptr) {
  for (int i = 0; i < n_seqs; ++i) if (!operands[i] || (operands2 && !operands2[i])) return fail(ctx, GVL_ERR_ARG, std::string(fn) + ": bad " + what);
  return 0;
}
template <class Run>
static int prefill_groups(gvl_ctx* ctx, const int* seq_ids, int n_seqs, const uint16_t* const* embeds, const int* lens, int cap, Run&& run) {
  for (int i = 0; i < n_seqs;) {
    const int B = prefill_group_size(lens + i, n_seqs - i, cap, ctx->cfg.max_prefill);
    Seq* sqs[GVL_MAX_PREFILL_BATCH]; const bf16_t* es[GVL_MAX_PREFILL_BATCH]; int pos0[GVL_MAX_PREFILL_BATCH];
    for (int b = 0; b < B; ++b) { sqs[b] = &ctx->seqs[seq_ids[i + b]]; es[b] = embeds[i + b]; pos0[b] = sqs[b]->pos; }
    if (const int rc = run(i, B, sqs, es, pos0)) return rc;
    i += B;
  }
  return 0;
}

extern "C" {

int gvl_prefill_extend(gvl_ctx* ctx, int seq_id, const uint16_t* embeds, int n_new, float* last_logits, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_prefill_extend");
  if (!embeds) return fail(ctx, GVL_ERR_ARG, "gvl_prefill_extend: bad length");
  if (const int rc = admit(ctx, gvl_admit::PREFILL_EXTEND, &seq_id, 1, &n_new, 0)) return rc;
  Seq& sq = ctx->seqs[seq_id];
  hipStream_t st = (hipStream_t)stream;
  Seq* one[1] = {&sq}; const bf16_t* e1[1] = {embeds};
  const int pos0 = sq.pos;
  int rc = llm_prefill(ctx, one, 1, e1, &n_new, st, nullptr, &pos0);
  if (rc) return rc;
  if (last_logits) HIPCHK(ctx, hipMemcpyAsync(last_logits, ctx->d_logits, (size_t)ctx->cfg.vocab * 4, hipMemcpyDeviceToDevice, st));
  return 0;
}

int gvl_forward_loss(gvl_ctx* ctx, int seq_id, const uint16_t* embeds, int S, const int64_t* labels, double* nll_sum, int* n_valid, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_forward_loss");
  if (!embeds || !labels || !nll_sum || !n_valid) return fail(ctx, GVL_ERR_ARG, "gvl_forward_loss: bad arguments / length");
  if (const int rc = admit(ctx, gvl_admit::FORWARD_LOSS, &seq_id, 1, &S, 0)) return rc;
  Seq& sq = ctx->seqs[seq_id];
  // shift (logits[:-1] vs labels[1:]) and drop ignore_index (-100) on the host: integer work
  std::vector<int> rows, tgt;
  for (int t = 0; t + 1 < S; ++t) {
    const int64_t y = labels[t + 1];
    if (y == -100) continue;
    if (y < 0 || y >= ctx->cfg.vocab) return fail(ctx, GVL_ERR_ARG, "gvl_forward_loss: label out of range");   // torch CrossEntropyLoss raises too
    rows.push_back(t); tgt.push_back((int)y);
  }
  std::vector<float> nll(rows.size());
  LossReq lr{(int)rows.size(), rows.data(), tgt.data(), nll.data()};
  hipStream_t st = (hipStream_t)stream;
  Seq* one[1] = {&sq}; const bf16_t* e1[1] = {embeds};
  const int rc = llm_prefill(ctx, one, 1, e1, &S, st, &lr);
  if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(st));                     // host vectors above are the copy endpoints
  double acc = 0;
  for (float v : nll) acc += (double)v;
  *nll_sum = acc; *n_valid = (int)rows.size();
  return 0;
}

int gvl_prefill_varlen(gvl_ctx* ctx, const int* seq_ids, int n_seqs, const uint16_t* const* embeds, const int* seq_lens, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_prefill_varlen");
  if (!seq_ids || !embeds || !seq_lens || n_seqs <= 0 || n_seqs > gvl_ctx::kMaxSeqs) return fail(ctx, GVL_ERR_ARG, "gvl_prefill_varlen: bad arguments");
  if (const int rc = members_present(ctx, "gvl_prefill_varlen", "seq / embeds", n_seqs, (const void* const*)embeds)) return rc;
  if (const int rc = admit(ctx, gvl_admit::PREFILL_VARLEN, seq_ids, n_seqs, seq_lens, 1)) return rc;
  hipStream_t st = (hipStream_t)stream;
  // today's behaviour: groups of up to prefill_group (gvl_debug_set) sequences here, of up to GVL_MAX_PREFILL_BATCH in the extend and score entries
  return prefill_groups(ctx, seq_ids, n_seqs, embeds, seq_lens, ctx->dbg.prefill_group, [&](int i, int B, Seq* const* sqs, const bf16_t* const* es, const int*) {
    return llm_prefill(ctx, sqs, B, es, seq_lens + i, st);
  });
}

// Ragged prefill where every member sits behind its own cached prefix (0 = none).  Everything is checked before the first launch, so an error leaves every sequence
// as it was (the pool is never touched: a sequence owns its pages from gvl_seq_alloc / gvl_seq_fork on).
int gvl_prefill_extend_varlen(gvl_ctx* ctx, const int* seq_ids, int n_seqs, const uint16_t* const* embeds_new, const int* n_new, float* last_logits, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_prefill_extend_varlen");
  if (!seq_ids || !embeds_new || !n_new || n_seqs <= 0 || n_seqs > gvl_ctx::kMaxSeqs) return fail(ctx, GVL_ERR_ARG, "gvl_prefill_extend_varlen: bad arguments");
  if (const int rc = members_present(ctx, "gvl_prefill_extend_varlen", "seq / embeds", n_seqs, (const void* const*)embeds_new)) return rc;
  if (const int rc = admit(ctx, gvl_admit::PREFILL_EXTEND_VARLEN, seq_ids, n_seqs, n_new, 1)) return rc;
  hipStream_t st = (hipStream_t)stream;
  return prefill_groups(ctx, seq_ids, n_seqs, embeds_new, n_new, GVL_MAX_PREFILL_BATCH, [&](int i, int B, Seq* const* sqs, const bf16_t* const* es, const int* pos0) {
    if (const int rc = llm_prefill(ctx, sqs, B, es, n_new + i, st, nullptr, pos0)) return rc;
    if (last_logits) HIPCHK(ctx, hipMemcpyAsync(last_logits + (size_t)i * ctx->cfg.vocab, ctx->d_logits, (size_t)B * ctx->cfg.vocab * 4, hipMemcpyDeviceToDevice, st));
    return 0;
  });
}

// gvl_prefill_extend_varlen that also scores given next ids on the way: the same members, groups, refusals and final states; per group the scored rows' packed indices and
// targets go to llm_prefill as a ScoreReq.  The targets and top_n are checked with everything else, before the first launch.
int gvl_score_extend_varlen(gvl_ctx* ctx, const int* seq_ids, int n_seqs, const uint16_t* const* embeds_new, const int* n_new, const int32_t* const* next_ids_host, int top_n,
                            float* lp_dev, int32_t* rank_dev, int32_t* top_ids_dev, float* top_lp_dev, int* n_scored, float* last_logits, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_score_extend_varlen");
  if (!seq_ids || !embeds_new || !n_new || !next_ids_host || !lp_dev || !rank_dev || n_seqs <= 0 || n_seqs > gvl_ctx::kMaxSeqs)
    return fail(ctx, GVL_ERR_ARG, "gvl_score_extend_varlen: bad arguments");
  if (top_n < 0 || top_n > GVL_MAX_TOP_LOGPROBS || (top_n > 0 && (!top_ids_dev || !top_lp_dev)))
    return fail(ctx, GVL_ERR_ARG, "gvl_score_extend_varlen: top_n must be 0 .. 8 (top lists needed for > 0)");
  if (const int rc = members_present(ctx, "gvl_score_extend_varlen", "seq / embeds / next ids", n_seqs, (const void* const*)embeds_new, (const void* const*)next_ids_host)) return rc;
  if (const int rc = admit(ctx, gvl_admit::SCORE_EXTEND_VARLEN, seq_ids, n_seqs, n_new, 1)) return rc;
  for (int i = 0; i < n_seqs; ++i)
    for (int r = 0; r < n_new[i]; ++r) {
      const int32_t y = next_ids_host[i][r];
      if (y != -100 && (y < 0 || y >= ctx->cfg.vocab)) return fail(ctx, GVL_ERR_ARG, "gvl_score_extend_varlen: next id out of range");
    }
  hipStream_t st = (hipStream_t)stream;
  int done = 0;                                        // scored rows of the groups before this one: where its packed outputs start
  std::vector<int> rows, tgt;
  const int rc = prefill_groups(ctx, seq_ids, n_seqs, embeds_new, n_new, GVL_MAX_PREFILL_BATCH, [&](int i, int B, Seq* const* sqs, const bf16_t* const* es, const int* pos0) {
    rows.clear(); tgt.clear();
    for (int b = 0, off = 0; b < B; off += n_new[i + b], ++b)
      for (int r = 0; r < n_new[i + b]; ++r) if (next_ids_host[i + b][r] != -100) { rows.push_back(off + r); tgt.push_back(next_ids_host[i + b][r]); }
    ScoreReq sr{(int)rows.size(), rows.data(), tgt.data(), top_n, lp_dev + done, rank_dev + done,
                top_n > 0 ? top_ids_dev + (size_t)done * GVL_MAX_TOP_LOGPROBS : nullptr, top_n > 0 ? top_lp_dev + (size_t)done * GVL_MAX_TOP_LOGPROBS : nullptr};
    if (const int rc = llm_prefill(ctx, sqs, B, es, n_new + i, st, nullptr, pos0, &sr)) return rc;
    if (last_logits) HIPCHK(ctx, hipMemcpyAsync(last_logits + (size_t)i * ctx->cfg.vocab, ctx->d_logits, (size_t)B * ctx->cfg.vocab * 4, hipMemcpyDeviceToDevice, st));
    done += sr.n;
    return 0;
  });
  if (rc) return rc;
  if (n_scored) *n_scored = done;
  return 0;
}

int gvl_prefill_batch(gvl_ctx* ctx, const int* seq_ids, int n_seqs, const uint16_t* const* embeds, int S, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (n_seqs <= 0 || n_seqs > gvl_ctx::kMaxSeqs) return fail(ctx, GVL_ERR_ARG, "gvl_prefill_batch: bad arguments");
  int lens[gvl_ctx::kMaxSeqs];
  for (int i = 0; i < n_seqs; ++i) lens[i] = S;
  return gvl_prefill_varlen(ctx, seq_ids, n_seqs, embeds, lens, stream);
}

int gvl_decode_greedy(gvl_ctx* ctx, int seq_id, int max_new, int eos_id, int32_t* out_ids, int* n_out, void* stream) {
  return gvl_decode_greedy_batch(ctx, &seq_id, 1, max_new, eos_id, out_ids, n_out, stream);
}

int gvl_decode_greedy_batch(gvl_ctx* ctx, const int* seq_ids, int n_seqs, int max_new, int eos_id, int32_t* out_ids, int* n_out, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_decode_greedy_batch");
  if (!seq_ids || n_seqs <= 0 || n_seqs > gvl_ctx::kMaxSeqs || !out_ids || !n_out || max_new <= 0 || max_new > ctx->outlist_cap)
    return fail(ctx, GVL_ERR_ARG, "gvl_decode_greedy_batch: bad arguments");
  if (const int rc = admit(ctx, gvl_admit::DECODE_GREEDY_BATCH, seq_ids, n_seqs, nullptr, 0)) return rc;   // members of a group must also be at the SAME step (checked per group)
  hipStream_t st = (hipStream_t)stream;
  // a group streams the weights once per step for all of its members (named_parts)
  Seq* named[gvl_ctx::kMaxSeqs]; int sizes[gvl_ctx::kMaxSeqs];
  for (int i = 0; i < n_seqs; ++i) named[i] = &ctx->seqs[seq_ids[i]];
  for (int k = 0, i = 0, nk = named_parts(ctx, named, n_seqs, sizes); k < nk; ++k) {
    const int B = sizes[k];
    int32_t* outs[GVL_MAX_DECODE_BATCH]; int* nouts[GVL_MAX_DECODE_BATCH];
    for (int b = 0; b < B; ++b) { outs[b] = out_ids + (size_t)(i + b) * max_new; nouts[b] = n_out + i + b; }
    const int rc = decode_group(ctx, named + i, B, max_new, eos_id, outs, nouts, st);
    if (rc) return rc;
    i += B;
  }
  return 0;
}

// ---- building blocks of a continuous-batching scheduler: sequences at DIFFERENT generation steps advance
// together, the host decides between chunks who joins (gvl_prefill*) and who leaves (gvl_seq_free).
int gvl_decode_steps(gvl_ctx* ctx, const int* seq_ids, int n_seqs, int n_steps, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_decode_steps");
  if (!seq_ids || n_seqs <= 0 || n_seqs > gvl_ctx::kMaxSeqs || n_steps <= 0) return fail(ctx, GVL_ERR_ARG, "gvl_decode_steps: bad arguments");
  if (const int rc = admit(ctx, gvl_admit::DECODE_STEPS, seq_ids, n_seqs, &n_steps, 0)) return rc;
  hipStream_t st = (hipStream_t)stream;
  Seq* named[gvl_ctx::kMaxSeqs]; int sizes[gvl_ctx::kMaxSeqs];
  for (int i = 0; i < n_seqs; ++i) named[i] = &ctx->seqs[seq_ids[i]];
  const int nk = named_parts(ctx, named, n_seqs, sizes);   // a guided leader brings its follower's row (bound with at least the leader's capacity left)
  for (int s = 0; s < n_steps; ++s) {
    for (int k = 0, i = 0; k < nk; ++k) {
      Seq* sqs[GVL_MAX_DECODE_BATCH];
      const int rc = decode_step(ctx, sqs, step_rows(ctx, named + i, sizes[k], sqs), st);
      if (rc) return rc;
      i += sizes[k];
    }
  }
  return 0;
}

int gvl_seq_read(gvl_ctx* ctx, int seq_id, int first, int32_t* out_ids, int cap, int* n_gen, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_seq_read");
  if (!ctx->lookup(seq_id) || !n_gen || first < 0 || cap < 0 || (cap > 0 && !out_ids)) return fail(ctx, GVL_ERR_ARG, "gvl_seq_read: bad arguments");
  const Seq& sq = ctx->seqs[seq_id];
  *n_gen = sq.n_gen;
  int n = sq.n_gen - first; if (n > cap) n = cap;
  if (n > 0) {
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));
    memcpy(out_ids, sq.h_out + first, (size_t)n * 4);
  }
  return 0;
}

int gvl_decode_step_logits(gvl_ctx* ctx, int seq_id, int tok, float* logits, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_decode_step_logits");
  if (const int rc = admit(ctx, gvl_admit::DECODE_STEP_LOGITS, &seq_id, 1, &tok, 0)) return rc;
  Seq& sq = ctx->seqs[seq_id];
  hipStream_t st = (hipStream_t)stream;
  RUN(GVL_PROF_OTHER, 0, gvl_launch_set_int(sq.d_tok, tok, st));
  Seq* one[1] = {&sq};
  int rc = decode_step(ctx, one, 1, st);
  if (rc) return rc;
  if (sq.bank) { rc = bank_append(ctx, sq, ctx->d_x, ctx->cfg.hidden, 1, st); if (rc) return rc; }   // the step's residual row behind the last layer
  if (logits) HIPCHK(ctx, hipMemcpyAsync(logits, ctx->d_logits, (size_t)ctx->cfg.vocab * 4, hipMemcpyDeviceToDevice, st));
  return 0;
}

int gvl_decode_step_logits_batch(gvl_ctx* ctx, const int* seq_ids, int n_seqs, const int32_t* toks, float* logits, void* stream) {
  REQUIRE_READY(ctx->has_llm, "gvl_decode_step_logits_batch");
  if (!seq_ids || !toks || !decode_batch_ok(ctx->decode_mfma, n_seqs))
    return fail(ctx, GVL_ERR_ARG, "gvl_decode_step_logits_batch: 1 .. 16 sequences (VALU fallback geometries: 1, 2 or 4)");
  if (const int rc = admit(ctx, gvl_admit::DECODE_STEP_LOGITS_BATCH, seq_ids, n_seqs, toks, 1)) return rc;
  Seq* sqs[GVL_MAX_DECODE_BATCH];
  for (int i = 0; i < n_seqs; ++i) sqs[i] = &ctx->seqs[seq_ids[i]];
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < n_seqs; ++i) RUN(GVL_PROF_OTHER, 0, gvl_launch_set_int(sqs[i]->d_tok, toks[i], st));
  const int rc = decode_step(ctx, sqs, n_seqs, st);       // ONE weight stream for all of them; row i depends on sequence i only (batch-invariant kernels)
  if (rc) return rc;
  for (int i = 0; i < n_seqs; ++i)                        // keep-hidden members: row i of the step's residual rows joins sequence i's bank
    if (sqs[i]->bank) { const int brc = bank_append(ctx, *sqs[i], ctx->d_x + (size_t)i * ctx->cfg.hidden, ctx->cfg.hidden, 1, st); if (brc) return brc; }
  if (logits) HIPCHK(ctx, hipMemcpyAsync(logits, ctx->d_logits, (size_t)n_seqs * ctx->cfg.vocab * 4, hipMemcpyDeviceToDevice, st));
  return 0;
}

int gvl_debug_set(gvl_ctx* ctx, const char* key, int value) {
  if (!ctx || !key) return GVL_ERR_ARG;
  const std::string k = key;
  if (k == "decode_attn_cpb") { if (value < 0 || value > 16) return fail(ctx, GVL_ERR_ARG, "gvl_debug_set: decode_attn_cpb must be 0 (default) .. 16"); ctx->dbg.decode_attn_cpb = value; }
  else if (k == "decode_attn_hpb") { if (value < 0) return fail(ctx, GVL_ERR_ARG, "gvl_debug_set: decode_attn_hpb must be >= 0"); ctx->dbg.decode_attn_hpb = value; }
  else if (k == "decode_graph") ctx->dbg.decode_graph = value != 0;
  else if (k == "attn_ring") { if (value != 0 && value != 2 && value != 3) return fail(ctx, GVL_ERR_ARG, "gvl_debug_set: attn_ring must be 0, 2 or 3"); ctx->dbg.attn_ring = value; }
  else if (k == "prefill_group") { if (value < 1 || value > GVL_MAX_PREFILL_BATCH) return fail(ctx, GVL_ERR_ARG, "gvl_debug_set: prefill_group must be 1 .. 8"); ctx->dbg.prefill_group = value; }
  else if (k == "attn_pipe") { if (value < 0 || value > 2) return fail(ctx, GVL_ERR_ARG, "gvl_debug_set: attn_pipe must be 0, 1 or 2"); ctx->dbg.attn_pipe = value; }
  else if (k == "attn_pipe_rows") { if (value != 128 && value != 256) return fail(ctx, GVL_ERR_ARG, "gvl_debug_set: attn_pipe_rows must be 128 (default) or 256"); ctx->dbg.attn_pipe_rows = value; }
  else if (k == "patch_fused") ctx->dbg.patch_fused = value != 0;
  else if (k == "varlen_attn") ctx->dbg.varlen_attn = value < 0 || value > 2 ? 1 : value;
  else if (k == "varlen_extend") ctx->dbg.varlen_extend = value != 0;
  else if (k == "norm_fused") ctx->dbg.norm_fused = value != 0;
  else if (k == "last_layer_tail") ctx->dbg.last_layer_tail = value != 0;
  else if (k == "gemm_band") { if (value < 0 || value > 64) return fail(ctx, GVL_ERR_ARG, "gvl_debug_set: gemm_band must be 0 (automatic) .. 64"); gvl_gemm_set_band(value); }
  else if (k == "gemm_a4") { if (value < 0 || value > 3) return fail(ctx, GVL_ERR_ARG, "gvl_debug_set: gemm_a4 must be 0 .. 3"); gvl_gemm_set_a4(value); }
  else if (k == "gemm_narrow") gvl_gemm_set_narrow(value < 0 || value > 2 ? 1 : value);
  else if (k == "vision_in_place") { if (value < 0 || value > 2) return fail(ctx, GVL_ERR_ARG, "gvl_debug_set: vision_in_place must be 0, 1 or 2"); ctx->dbg.vision_in_place = value; }
  else return fail(ctx, GVL_ERR_ARG, "gvl_debug_set: unknown key " + k);
  return 0;
}

int gvl_preprocess_frames(gvl_ctx* ctx, const uint8_t* frames, int n, int height, int width, int layout, int size,
                          const float* mean, const float* stdv, float* out, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!frames || !out || !mean || !stdv || n <= 0 || height <= 0 || width <= 0 || size <= 0 || (layout != 0 && layout != 1))
    return fail(ctx, GVL_ERR_ARG, "gvl_preprocess_frames: bad arguments");
  for (int c = 0; c < 3; ++c) if (!(stdv[c] != 0.f)) return fail(ctx, GVL_ERR_ARG, "gvl_preprocess_frames: zero std");
  const int rc = gvl_launch_preprocess(frames, n, height, width, layout, size, mean, stdv, out, &ctx->pre_scratch, &ctx->pre_scratch_bytes, (hipStream_t)stream);
  if (rc == -2) return fail(ctx, GVL_ERR_OOM, "gvl_preprocess_frames: hipMalloc(scratch) failed");
  if (rc) return fail(ctx, rc == -1 ? GVL_ERR_ARG : GVL_ERR_HIP, "gvl_preprocess_frames: launch failed");
  return 0;
}

int gvl_prof_enable(gvl_ctx* ctx, int on) {
  if (!ctx) return GVL_ERR_ARG;
  hipDeviceSynchronize();
  for (auto& r : ctx->recs) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
  ctx->recs.clear();
  for (int i = 0; i < GVL_PROF_NCAT; ++i) { ctx->prof_ms[i] = 0; ctx->prof_work[i] = 0; ctx->prof_n[i] = 0; }
  ctx->prof = on != 0;
  return 0;
}
int gvl_prof_read(gvl_ctx* ctx, int cat, double* total_ms, int64_t* launches, double* work) {
  if (!ctx || cat < 0 || cat >= GVL_PROF_NCAT) return GVL_ERR_ARG;
  hipDeviceSynchronize();
  for (auto& r : ctx->recs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) { ctx->prof_ms[r.cat] += ms; ctx->prof_work[r.cat] += r.work; ctx->prof_n[r.cat] += 1; }
    hipEventDestroy(r.e0); hipEventDestroy(r.e1);
  }
  ctx->recs.clear();
  if (total_ms) *total_ms = ctx->prof_ms[cat];
  if (launches) *launches = ctx->prof_n[cat];
  if (work) *work = ctx->prof_work[cat];
  return 0;
}

// ---- operator-level entry points -------------------------------------------------------------------
int gvl_op_gemm(gvl_ctx* ctx, const uint16_t* A, const uint16_t* W, void* C, int M, int N, int K, const float* bias, const float* gamma,
                const void* resid, int act, int out_f32, int tile_cfg, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  GemmArgs g = gemm(A, K, W, C, act == GVL_ACT_SILU_MUL ? N / 2 : N, M, N, K);
  g.bias = bias; g.gamma = gamma; g.resid = resid; g.ldr = N; g.act = act; g.out_f32 = out_f32; g.round_pre_resid = 1; g.tile_cfg = tile_cfg;
  if (const char* e = gvl_lab_env("GVL_LAB_LD")) { int la = 0, lw = 0; if (sscanf(e, "%d,%d", &la, &lw) == 2) { g.lda = la; g.ldw = lw; } }   // LAB: operand row pitches (tools/gemm_lab.py)
  RUN(GVL_PROF_GEMM, gvl_gemm_flops(g), gvl_launch_gemm(g, st));
  return 0;
}
// The fused-RMSNorm epilogues at operator level (bf16 output): rowscale [M] f32 or null multiplies the accumulator rows before bias / activation; rowsq
// [M][rowsq_ld] f32 or null receives the sums of squares of the rounded outputs per aligned 64-column block (N % 64 == 0).
int gvl_op_gemm_rows(gvl_ctx* ctx, const uint16_t* A, const uint16_t* W, uint16_t* C, int M, int N, int K, const float* bias, const float* gamma,
                     const uint16_t* resid, int act, const float* rowscale, float* rowsq, int rowsq_ld, int tile_cfg, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  GemmArgs g = gemm(A, K, W, C, act == GVL_ACT_SILU_MUL ? N / 2 : N, M, N, K);
  g.bias = bias; g.gamma = gamma; g.resid = resid; g.ldr = N; g.act = act; g.round_pre_resid = 1; g.tile_cfg = tile_cfg;
  g.rowscale = rowscale; g.rowsq = rowsq; g.rowsq_ld = rowsq_ld;
  RUN(GVL_PROF_GEMM, gvl_gemm_flops(g), gvl_launch_gemm(g, st));
  return 0;
}
// The row-remapping store of build_visual at operator level: GEMM row m lands at row (m / grp_rows) * grp_stride + m % grp_rows + row_off of C.
int gvl_op_gemm_grouped(gvl_ctx* ctx, const uint16_t* A, const uint16_t* W, void* C, int M, int N, int K, const float* bias, const float* gamma,
                        const void* resid, int act, int out_f32, float* rowsq, int rowsq_ld, int grp_rows, int grp_stride, int row_off, int tile_cfg,
                        void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!A || !W || !C) return fail(ctx, GVL_ERR_ARG, "gvl_op_gemm_grouped: null operand");
  if (grp_rows < 1 || row_off < 0 || (long)row_off + grp_rows > grp_stride) return fail(ctx, GVL_ERR_ARG, "gvl_op_gemm_grouped: needs grp_rows >= 1, row_off >= 0 and row_off + grp_rows <= grp_stride");
  hipStream_t st = (hipStream_t)stream;
  GemmArgs g = gemm(A, K, W, C, act == GVL_ACT_SILU_MUL ? N / 2 : N, M, N, K);
  g.bias = bias; g.gamma = gamma; g.resid = resid; g.ldr = N; g.act = act; g.out_f32 = out_f32; g.round_pre_resid = 1; g.tile_cfg = tile_cfg;
  g.rowsq = rowsq; g.rowsq_ld = rowsq_ld; g.grp_rows = grp_rows; g.grp_stride = grp_stride; g.row_off = row_off;
  RUN(GVL_PROF_GEMM, gvl_gemm_flops(g), gvl_launch_gemm(g, st));
  return 0;
}
// W' = bf16(W diag(gamma)) and rs = rsqrt(sum of the blocks [b0, b0 + nblk) / cols + eps): the two small kernels around those epilogues
int gvl_op_fold_gamma(gvl_ctx* ctx, const uint16_t* W, const uint16_t* gamma, uint16_t* Wo, int64_t rows, int cols, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  RUN(GVL_PROF_OTHER, 0, gvl_launch_fold_gamma(W, gamma, Wo, (long)rows, cols, st));
  return 0;
}
int gvl_op_rowsq_finish(gvl_ctx* ctx, const float* rowsq, int ld, int b0, int nblk, float* rs, int rows, int cols, float eps, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  RUN(GVL_PROF_OTHER, 0, gvl_launch_rowsq_finish(rowsq, ld, b0, nblk, rs, rows, cols, eps, st));
  return 0;
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
  // non-causal (vision) attention reads v -- and, when no head-dim padding is needed, q and k -- in place, exactly as the towers do
  const int ld = (H + 2 * KV) * Dr;
  const bool v_rows = ctx->dbg.vision_in_place && !causal && D != 128, qk_rows = ctx->dbg.vision_in_place == 1 && v_rows && D == Dr && D == 64;
  if (!qk_rows) { QkvPostArgs p; memset(&p, 0, sizeof(p)); p.qkv = q; p.ld = ld; p.Q = Q; p.Kt = Kt; p.Vt = v_rows ? nullptr : Vt; p.B = B; p.S = S; p.H = H; p.KV = KV; p.Dr = Dr; p.D = D; p.mode = 0;
    RUN(GVL_PROF_OTHER, 0, gvl_launch_qkv_post(p, st)); }
  { AttnArgs a; memset(&a, 0, sizeof(a)); a.Q = Q; a.Kt = Kt; a.Vt = Vt; a.O = out; a.B = B; a.H = H; a.KV = KV; a.S = S; a.D = D; a.Dout = Dr; a.scale = scale; a.causal = causal; a.ring = ctx->dbg.attn_ring;
    if (v_rows) { a.Vrows = v; a.v_ld = ld; }
    if (qk_rows) { a.Qrows = q; a.Krows = k; a.q_ld = a.k_ld = ld; }
    RUN(GVL_PROF_ATTN, gvl_attn_flops(a), gvl_launch_attention(a, st)); }
  return 0;
}
int gvl_op_layernorm(gvl_ctx* ctx, const float* x, const float* w, const float* b, uint16_t* y, int rows, int cols, float eps, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  RUN(GVL_PROF_OTHER, 0, gvl_launch_layernorm_f32(x, w, b, y, rows, cols, eps, st));
  return 0;
}
int gvl_op_rmsnorm(gvl_ctx* ctx, const uint16_t* x, const uint16_t* w, uint16_t* y, int rows, int cols, float eps, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  RUN(GVL_PROF_OTHER, 0, gvl_launch_rmsnorm_bf16(x, w, y, rows, cols, eps, st));
  return 0;
}
// ---- the vision front end and the glue of the visual prefix at operator level (tests/test_gpu_vision_ops.py; fields and geometry: include/gvl.h) ----------------
// The patch embedding of either tower by EITHER path, chosen by the caller: a geometry the fused launcher refuses is an error here, not a fall-back.
int gvl_op_patch_embed(gvl_ctx* ctx, const gvl_patch_embed* p, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!p) return fail(ctx, GVL_ERR_ARG, "gvl_op_patch_embed: null descriptor");
  const char* bad = nullptr;
  if (p->mode != 0 && p->mode != 1) bad = "mode is 0 (CLIP) or 1 (InternVideo2)";
  else if (p->path != 0 && p->path != 1) bad = "path is 0 (fused) or 1 (three passes)";
  else if (p->n <= 0 || p->T <= 0 || p->image <= 0 || p->patch <= 0 || p->C <= 0 || p->Kp <= 0) bad = "n, T, image, patch, C and Kp must be positive";
  else if (p->image % p->patch) bad = "image must be a multiple of patch";
  else if (p->Kp % 8 || p->Kp < 3 * p->patch * p->patch) bad = "Kp must be a multiple of 8 and hold 3 patch^2 columns";
  else if (!p->px || !p->W || !p->cls || !p->pos || !p->out) bad = "px, W, cls, pos and out are required";
  else if (p->mode == 0 && (!p->lnw || !p->lnb)) bad = "CLIP needs lnw and lnb";
  else if (p->mode == 0 && p->T != 1) bad = "CLIP has one frame per image (T = 1)";
  else if (p->mode == 1 && !p->bias) bad = "InternVideo2 needs the conv bias";
  else if (p->path == 0 && p->im2col) bad = "the fused path forms no im2col matrix";
  else if (p->path == 1 && (p->Kp % 64 || p->C % 8 || (p->mode == 0 && p->C > 4096))) bad = "the three passes need Kp % 64 == 0 and C % 8 == 0 (CLIP: C <= 4096)";
  if (bad) return fail(ctx, GVL_ERR_ARG, std::string("gvl_op_patch_embed: ") + bad);
  const int g = p->image / p->patch;
  const long M_l = (long)p->n * p->T * g * g;
  if (M_l > (1l << 30)) return fail(ctx, GVL_ERR_ARG, "gvl_op_patch_embed: too many patch rows");
  const int M = (int)M_l, TL = p->T * g * g, C = p->C;
  hipStream_t st = (hipStream_t)stream;
  ArenaScope arena_scope(ctx->arena_off);
  if (p->path == 0) {
    if (C % 16 || p->patch > 16 || (p->patch & 1)) return fail(ctx, GVL_ERR_ARG, "gvl_op_patch_embed: geometry outside the fused kernel");
    AALLOC(Wt, bf16_t, (size_t)(C / 16) * (3 * p->patch / 2) * 512);
    PatchEmbedArgs e; memset(&e, 0, sizeof(e)); e.px = p->px; e.Wt = Wt; e.n_img = p->n; e.T = p->T; e.image = p->image; e.patch = p->patch; e.C = C;
    e.M = M; e.S = TL + 1; e.mode = p->mode; e.eps = p->eps;
    if (p->mode == 0) { e.cls_f32 = (const float*)p->cls; e.pos_f32 = (const float*)p->pos; e.lnw = p->lnw; e.lnb = p->lnb; e.x_f32 = (float*)p->out; }
    else { e.bias = p->bias; e.cls_bf = (const bf16_t*)p->cls; e.pos_bf = (const bf16_t*)p->pos; e.x_bf = (bf16_t*)p->out; }
    RUN(GVL_PROF_OTHER, 0, gvl_retile_patch_weight(p->W, Wt, C, p->Kp, p->patch, st));
    const int rc = gvl_launch_patch_embed(e, st);
    if (rc) return fail(ctx, rc == -1 ? GVL_ERR_ARG : GVL_ERR_HIP, rc == -1 ? "gvl_op_patch_embed: geometry outside the fused kernel" : "gvl_op_patch_embed: launch failed");
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
  if (!ctx) return GVL_ERR_ARG;
  if (!px || !A || n <= 0 || T <= 0 || image <= 0 || patch <= 0 || Kp <= 0) return fail(ctx, GVL_ERR_ARG, "gvl_op_patchify: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  RUN(GVL_PROF_OTHER, 0, gvl_launch_patchify(px, A, n, T, image, patch, Kp, st));
  return 0;
}
int gvl_op_hd_merge(gvl_ctx* ctx, const float* f, const float* sub_gn, uint16_t* out, int n, int C, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!f || !sub_gn || !out || n <= 0 || C <= 0) return fail(ctx, GVL_ERR_ARG, "gvl_op_hd_merge: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  RUN(GVL_PROF_OTHER, 0, gvl_launch_hd_merge(f, sub_gn, out, n, C, st));
  return 0;
}
int gvl_op_pool_spatial(gvl_ctx* ctx, const float* f, uint16_t* out, int n, int C, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!f || !out || n <= 0 || C <= 0) return fail(ctx, GVL_ERR_ARG, "gvl_op_pool_spatial: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  RUN(GVL_PROF_OTHER, 0, gvl_launch_pool_spatial(f, out, n, C, st));
  return 0;
}
int gvl_op_pool_temporal(gvl_ctx* ctx, const uint16_t* f, uint16_t* out, int n, int T, int C, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!f || !out || n <= 0 || T <= 0 || C <= 0) return fail(ctx, GVL_ERR_ARG, "gvl_op_pool_temporal: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  RUN(GVL_PROF_OTHER, 0, gvl_launch_pool_temporal(f, out, n, T, C, st));
  return 0;
}
int gvl_op_strip_cls(gvl_ctx* ctx, const void* x, void* y, int n, int S, int C, int elem_bytes, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!x || !y || n <= 0 || S < 2 || C <= 0 || (elem_bytes != 2 && elem_bytes != 4)) return fail(ctx, GVL_ERR_ARG, "gvl_op_strip_cls: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  RUN(GVL_PROF_OTHER, 0, gvl_launch_strip_cls(x, y, n, S, C, elem_bytes, st));
  return 0;
}
int gvl_op_bcast_row(gvl_ctx* ctx, const uint16_t* row, uint16_t* dst, int n, int stride_rows, int row_off, int cols, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!row || !dst || n <= 0 || cols <= 0 || row_off < 0 || row_off >= stride_rows) return fail(ctx, GVL_ERR_ARG, "gvl_op_bcast_row: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  RUN(GVL_PROF_OTHER, 0, gvl_launch_bcast_row(row, dst, n, stride_rows, row_off, cols, st));
  return 0;
}
// operator-level entry for the WHOLE GemvArgs surface (tests/test_gpu_decode_proj.py): row-major operands in, private tiled / quantised copies made here, every launcher
// refusal returned as GVL_ERR_ARG before anything is written.  See include/gvl.h for the fields.  gvl_op_decode_proj checks the descriptor, decode_proj_run does the work.
static int decode_proj_run(gvl_ctx* ctx, const gvl_decode_proj* p, hipStream_t st, const char* who);
int gvl_op_decode_proj(gvl_ctx* ctx, const gvl_decode_proj* p, void* stream) {
  if (!ctx) return GVL_ERR_ARG;
  if (!p) return fail(ctx, GVL_ERR_ARG, "gvl_op_decode_proj: null descriptor");
  hipStream_t st = (hipStream_t)stream;
  const char* bad = nullptr;
  const int N = p->N, K = p->K, B = p->batch;
  if (N <= 0 || K <= 0 || !p->W || !p->x) bad = "N, K > 0 and W, x set";
  else if (B < 1 || B > GVL_MAX_DECODE_BATCH) bad = "1 <= batch <= 16";
  else if (p->path < 0 || p->path > 1 || p->w_fmt < 0 || p->w_fmt > 2) bad = "path 0 / 1, w_fmt 0 / 1 / 2";
  else if (K % (p->path == 0 ? 32 : 8)) bad = "K % 32 == 0 (tile order; the VALU GEMV: K % 8 == 0)";
  else if (p->act != GVL_ACT_NONE && p->act != GVL_ACT_SILU_MUL) bad = "act is NONE or SILU_MUL";
  else if (p->x_is_tiled && (p->norm_w || p->path == 1)) bad = "a tiled x feeds the skinny GEMM without norm_w only";
  else if (p->path == 1 && (p->variant || p->w_fmt || p->out_tiled || p->sq_in || p->sq_out || p->out_tiled2)) bad = "the VALU GEMV has no variants, quantised weights, tiled outputs or fused-norm sums";
  else if (p->out_stride < 0 || (p->out_stride && p->out_stride < (p->act == GVL_ACT_SILU_MUL ? N / 2 : N))) bad = "out_stride >= the output row length";
  else if (!p->rope_on && !p->out_bf16 && !p->out_f32) bad = "an output buffer";
  else if (p->path == 0 && B > 1 && !p->rope_on && (p->out_f32 || p->resid || (p->out_bf16 && !p->out_tiled)) && (p->out_stride ? p->out_stride : (p->act == GVL_ACT_SILU_MUL ? N / 2 : N)) % 4) bad = "out_stride % 4 == 0 for batch > 1 (8- and 16-byte epilogue stores)";
  else if (p->rope_on) {
    if (p->H < 1 || p->KV < 1 || p->Dr < 2 || (p->Dr & 1) || p->D < p->Dr || (long)N != (long)(p->H + 2 * p->KV) * p->Dr) bad = "rope: Dr even, D >= Dr, N == (H + 2 KV) Dr";
    else if (!p->cos_s || !p->sin_s || !p->pos || !p->tables || !p->Q || !p->Kt || !p->Vt) bad = "rope: tables, pos, page tables, Q, Kt, Vt set";
    else if (p->rope_switch > 0 && (!p->cos_l || !p->sin_l)) bad = "rope: long tables set when rope_switch > 0";
    else if (p->max_pos < 1 || p->n_pages < 1 || p->table_stride < 1 || p->q_stride < p->H * p->D) bad = "rope: max_pos, n_pages, table_stride >= 1, q_stride >= H D";
    else if (p->act || p->bias || p->resid) bad = "rope: no other epilogue";
  }
  if (bad) return fail(ctx, GVL_ERR_ARG, std::string("gvl_op_decode_proj: ") + bad);
  if (p->rope_on) {                                // the kernel trusts positions and page numbers: check them here, on the host
    std::vector<int> pos(B), tab((size_t)B * p->table_stride);
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, hipMemcpy(pos.data(), p->pos, sizeof(int) * B, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(tab.data(), p->tables, sizeof(int) * tab.size(), hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b) {
      if (pos[b] < 0 || pos[b] >= p->max_pos || (pos[b] >> 6) >= p->table_stride) return fail(ctx, GVL_ERR_ARG, "gvl_op_decode_proj: position outside the tables");
      const int page = tab[(size_t)b * p->table_stride + (pos[b] >> 6)];
      if (page < 0 || page >= p->n_pages) return fail(ctx, GVL_ERR_ARG, "gvl_op_decode_proj: page outside the pools");
    }
  }
  return decode_proj_run(ctx, p, st, "gvl_op_decode_proj");
}
static int decode_proj_run(gvl_ctx* ctx, const gvl_decode_proj* p, hipStream_t st, const char* who) {
  const int N = p->N, K = p->K, B = p->batch;
  struct Bufs { void* v[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; ~Bufs() { for (void* q : v) if (q) hipFree(q); } } bufs;
  void *&wc = bufs.v[0], *&wt = bufs.v[1], *&ws = bufs.v[2], *&xt = bufs.v[3];
  const size_t nb16 = (size_t)((N + 15) / 16);
  const int Dr = p->rope_on ? p->Dr : 0, nqk = p->rope_on ? p->H + p->KV : 0;
  GemvArgs g; memset(&g, 0, sizeof(g));
  int rc = 0;
  if (p->path == 0) {
    if (p->w_fmt) {                                // the quantisers rewrite their row-major source: work on a copy
      if (K % (p->w_fmt == 2 ? 1024 : 512)) return fail(ctx, GVL_ERR_ARG, std::string(who) + ": FP8 needs K % 512 == 0, MXFP4 K % 1024 == 0");
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
  const char* bad = nullptr;
  DecodeAttnLaunch l;
  if (!p->q || !p->Kt || !p->Vt || !p->tables || !p->pos || !p->part || !p->counters || !p->out) bad = "q, Kt, Vt, tables, pos, part, counters, out set";
  else if (B < 1 || B > GVL_MAX_DECODE_BATCH) bad = "1 <= batch <= 16";
  else if (decode_attn_plan(DecodeAttnGeometry{p->H, p->KV, p->D, p->nsplit, B, p->hpb, p->cpb, p->gsplit}, GVL_DECODE_ATTN_KNOBS_DEFAULT, &l) < 0)
    bad = "the launch plan does not serve this geometry (H % KV == 0, D 64 / 96 / 128, 1 <= nsplit <= 16)";
  else if (p->Dout < 1 || p->Dout > p->D) bad = "1 <= Dout <= D";
  else if (p->q_stride < p->H * p->D || (p->q_stride & 7) || ((uintptr_t)p->q & 15)) bad = "q_stride >= H D, q rows 16-byte aligned";
  else if (!p->out_tiled && p->out_stride < p->H * p->Dout) bad = "out_stride >= H Dout";
  else if (p->n_pages < 1 || p->table_stride < 1) bad = "n_pages, table_stride >= 1";
  if (bad) return fail(ctx, GVL_ERR_ARG, std::string("gvl_op_decode_attention: ") + bad);
  std::vector<int> pos(B), tab((size_t)B * p->table_stride);
  HIPCHK(ctx, hipStreamSynchronize(st));
  HIPCHK(ctx, hipMemcpy(pos.data(), p->pos, sizeof(int) * B, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(tab.data(), p->tables, sizeof(int) * tab.size(), hipMemcpyDeviceToHost));
  int longest = 1;                                   // split count of the longest sequence: one per 4 pages of its own length, at most nsplit
  for (int b = 0; b < B; ++b) {
    if (pos[b] < 0 || (long long)pos[b] >= (long long)p->table_stride * 64) return fail(ctx, GVL_ERR_ARG, "gvl_op_decode_attention: position outside the tables");
    const int np = (pos[b] + 1 + 63) >> 6, n4 = (np + 3) >> 2, ns = n4 > p->nsplit ? p->nsplit : n4;
    for (int i = 0; i < np; ++i) {
      const int page = tab[(size_t)b * p->table_stride + i];
      if (page < 0 || page >= p->n_pages) return fail(ctx, GVL_ERR_ARG, "gvl_op_decode_attention: page outside the pools");
    }
    longest = ns > longest ? ns : longest;
  }
  if ((long long)l.gsplit * l.cpb < longest) return fail(ctx, GVL_ERR_ARG, "gvl_op_decode_attention: gsplit * cpb is smaller than the longest sequence's split count (the ticket would never complete)");
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
  const char* bad = nullptr;
  if (!p->qkv || !p->Kt || (!p->Q && !p->q_rs)) bad = "qkv, Kt and Q (or q_rs) set";
  else if (p->mode < 0 || p->mode > 2) bad = "mode 0, 1 or 2";
  else if (p->H < 1 || p->KV < 1 || p->B < 1 || p->n_pages < 1) bad = "H, KV, B, n_pages >= 1";
  else if ((p->Dr & 7) || (p->mode == 2 && (p->Dr & 15)) || (p->D & 7) || p->D < p->Dr || p->Dr < 8 || p->Dr > 128) bad = "Dr % 8 == 0 (mode 2: % 16), 8 <= Dr <= 128, D % 8 == 0, D >= Dr";
  else if ((p->ld & 7) || (long long)p->ld < (long long)(p->H + 2 * p->KV) * p->Dr) bad = "ld % 8 == 0, ld >= (H + 2 KV) Dr";
  else if (p->mode == 1 && (!p->qn || !p->kn)) bad = "mode 1 needs qn and kn";
  else if (p->mode == 2 && (!p->cos || !p->sin || p->max_pos < 1)) bad = "mode 2 needs cos, sin and max_pos";
  else if (p->q_rs && p->mode != 1) bad = "q_rs is a mode 1 form";
  else if (p->q_rs && !p->k_ones) bad = "q_rs needs k_ones";
  else if ((p->ones_row || p->k_ones) && p->D == p->Dr) bad = "ones_row / k_ones need D > Dr";
  else if (n < 0 || n > GVL_MAX_PREFILL_BATCH) bad = "0 <= vl_n <= 8";
  else if (p->ext && (n < 1 || p->q_rs || !p->Vt)) bad = "ext needs a ragged group, Vt and no q_rs";
  else if (n && (p->mode != 2 || p->B != 1 || p->pos0 != 0 || p->block_table)) bad = "a ragged group needs mode 2, B == 1, pos0 == 0 and no block_table";
  else if (!n && (p->S < 1 || p->pos0 < 0)) bad = "S >= 1, pos0 >= 0";
  else if (!n && p->Vt && (p->pos0 & 63)) bad = "Vt needs pos0 % 64 == 0 (V^T pages are written whole)";
  else if (!n && !p->block_table && p->pos0) bad = "pos0 > 0 needs a block table";
  else if (!n && p->block_table && p->max_pages < 1) bad = "max_pages >= 1";
  if (bad) return fail(ctx, GVL_ERR_ARG, std::string("gvl_op_qkv_post: ") + bad);
  HIPCHK(ctx, hipStreamSynchronize(st));
  // per sequence: first position, rows and the table as the launch will index it (null: implicit pages)
  struct Member { long long pos0, rows, page0; std::vector<int> tab; bool has_tab; };
  std::vector<Member> ms;
  if (n) {
    if (p->vl_rows[0] != 0) return fail(ctx, GVL_ERR_ARG, "gvl_op_qkv_post: vl_rows[0] must be 0");
    for (int u = 0; u < n; ++u) {
      const long long rows = (long long)p->vl_rows[u + 1] - p->vl_rows[u];
      if (rows < 1) return fail(ctx, GVL_ERR_ARG, "gvl_op_qkv_post: an empty ragged member");
      if (!p->vl_tables[u] || p->table_len[u] < 1) return fail(ctx, GVL_ERR_ARG, "gvl_op_qkv_post: every ragged member needs a block table");
      const int pos0 = p->ext ? p->vl_pos0[u] : 0;
      if (pos0 < 0 || (pos0 & 63)) return fail(ctx, GVL_ERR_ARG, "gvl_op_qkv_post: vl_pos0 must be a multiple of 64");
      Member m{pos0, rows, 0, std::vector<int>((size_t)p->table_len[u]), true};
      HIPCHK(ctx, hipMemcpy(m.tab.data(), p->vl_tables[u], sizeof(int) * m.tab.size(), hipMemcpyDeviceToHost));
      ms.push_back(std::move(m));
    }
  } else {
    std::vector<int> all;
    if (p->block_table) { all.resize((size_t)p->B * p->max_pages); HIPCHK(ctx, hipMemcpy(all.data(), p->block_table, sizeof(int) * all.size(), hipMemcpyDeviceToHost)); }
    const long long nt = ((long long)p->S + 63) >> 6;
    for (int b = 0; b < p->B; ++b) {
      Member m{p->pos0, p->S, b * nt, {}, p->block_table != nullptr};
      if (p->block_table) m.tab.assign(all.begin() + (size_t)b * p->max_pages, all.begin() + (size_t)(b + 1) * p->max_pages);
      ms.push_back(std::move(m));
    }
  }
  std::vector<char> used((size_t)p->n_pages, 0);
  for (const Member& m : ms) {
    const long long end = m.pos0 + m.rows;                                   // one past the last position written
    if (p->mode == 2 && end > p->max_pos) return fail(ctx, GVL_ERR_ARG, "gvl_op_qkv_post: a position outside the cos / sin tables");
    const long long t0 = m.pos0 >> 6, t1 = (end + 63) >> 6;
    if (m.has_tab && t1 > (long long)m.tab.size()) return fail(ctx, GVL_ERR_ARG, "gvl_op_qkv_post: a block table shorter than ceil((pos0 + S) / 64)");
    for (long long t = t0; t < t1; ++t) {
      const long long page = m.has_tab ? m.tab[(size_t)t] : m.page0 + t;
      if (page < 0 || page >= p->n_pages) return fail(ctx, GVL_ERR_ARG, "gvl_op_qkv_post: page outside the pools");
      if (used[(size_t)page]) return fail(ctx, GVL_ERR_ARG, "gvl_op_qkv_post: a page named twice among the pages the launch writes");
      used[(size_t)page] = 1;
    }
  }
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
  const bool O16 = ((uintptr_t)p->O & 15) == 0;
  const char* bad = nullptr;
  if (!p->Q || !p->Kt || !p->Vt || !p->O) bad = "Q, Kt, Vt, O set";
  else if (p->n_pages < 1) bad = "n_pages >= 1";
  else if (n < 0 || n > GVL_MAX_PREFILL_BATCH) bad = "0 <= vl_n <= 8";
  else if (p->ext && n < 1) bad = "ext needs a ragged group";
  else if (!n && (!p->block_table || p->max_pages < 1)) bad = "the single form needs a block table (implicit pages: gvl_op_attention)";
  else if (p->ring != 0 && p->ring != 2 && p->ring != 3) bad = "ring 0, 2 or 3";
  else if (p->ext) {
    AttnExtGeometry g{};
    g.H = p->H; g.KV = p->KV; g.D = p->D; g.Dout = p->Dout; g.causal = p->causal; g.vl_n = n; g.O16 = O16;
    for (int u = 0; u <= n; ++u) g.vl_rows[u] = p->vl_rows[u];
    for (int u = 0; u < n; ++u) { g.vl_tables[u] = p->vl_tables[u] != nullptr; g.vl_pos0[u] = p->vl_pos0[u]; }
    AttnExtLaunch l;
    if (p->B != 1 || p->Sk || p->qpos0 || p->block_table || attn_ext_plan(g, GVL_ATTN_KNOBS_DEFAULT, &l) < 0)
      bad = "attn_ext_plan does not serve this launch (causal, B == 1, Sk == qpos0 == 0, no block_table, vl_rows[0] == 0, per member a table, >= 1 query, vl_pos0 % 64 == 0)";
  } else {
    AttnGeometry g{};
    g.B = p->B; g.H = p->H; g.KV = p->KV; g.S = p->S; g.D = p->D; g.Dout = p->Dout; g.Sk = p->Sk; g.qpos0 = p->qpos0; g.causal = p->causal; g.ring = p->ring;
    g.max_pages = p->max_pages; g.vl_n = n; g.block_table = p->block_table != nullptr; g.O16 = O16;
    for (int u = 0; u <= n; ++u) g.vl_rows[u] = p->vl_rows[u];
    for (int u = 0; u < n; ++u) g.vl_tables[u] = p->vl_tables[u] != nullptr;
    AttnLaunch l[GVL_ATTN_MAX_LAUNCHES];
    if (attn_plan(g, GVL_ATTN_KNOBS_DEFAULT, l) < 0 || (n && p->vl_rows[0] != 0))
      bad = "attn_plan does not serve this launch (D 64 / 96 / 128, Dout % 8 == 0, H % KV == 0, Sk == 0 or Sk >= qpos0 + S; ragged: causal, B == 1, Sk == qpos0 == 0, no block_table, per member a table and 1 .. S queries)";
  }
  if (bad) return fail(ctx, GVL_ERR_ARG, std::string("gvl_op_prefill_attention: ") + bad);
  HIPCHK(ctx, hipStreamSynchronize(st));
  auto check = [&](const std::vector<int>& tab, long long qpos0, long long S, long long Sk) -> const char* {   // one sequence: the key tiles its blocks read
    const long long tiles = p->causal ? ((qpos0 + S - 1) >> 6) + 1 : (Sk + 63) >> 6;
    if (tiles > (long long)tab.size()) return "a block table shorter than the key tiles the launch reads";
    for (long long t = 0; t < tiles; ++t) if (tab[(size_t)t] < 0 || tab[(size_t)t] >= p->n_pages) return "page outside the pools";
    return nullptr;
  };
  if (n) {
    for (int u = 0; u < n && !bad; ++u) {
      if (p->table_len[u] < 1) { bad = "table_len >= 1"; break; }
      std::vector<int> tab((size_t)p->table_len[u]);
      HIPCHK(ctx, hipMemcpy(tab.data(), p->vl_tables[u], sizeof(int) * tab.size(), hipMemcpyDeviceToHost));
      const long long S = (long long)p->vl_rows[u + 1] - p->vl_rows[u], q0 = p->ext ? p->vl_pos0[u] : 0;
      bad = check(tab, q0, S, q0 + S);
    }
  } else {
    std::vector<int> all((size_t)p->B * p->max_pages);
    HIPCHK(ctx, hipMemcpy(all.data(), p->block_table, sizeof(int) * all.size(), hipMemcpyDeviceToHost));
    for (int b = 0; b < p->B && !bad; ++b)
      bad = check(std::vector<int>(all.begin() + (size_t)b * p->max_pages, all.begin() + (size_t)(b + 1) * p->max_pages), p->qpos0, p->S, p->Sk > 0 ? p->Sk : p->S);
  }
  if (bad) return fail(ctx, GVL_ERR_ARG, std::string("gvl_op_prefill_attention: ") + bad);
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
  const char* bad = nullptr;
  const int f = p->form;
  if (f < 0 || f > 2) bad = "form 0, 1 or 2";
  else if (!p->Kt || !p->out) bad = "Kt and out set";
  else if (f == 0 && (!p->Q || !p->Vt || p->qkv || p->q_rs || p->q_nw)) bad = "form 0 takes Q, Kt, Vt and no qkv, q_rs, q_nw";
  else if (f == 1 && (!p->Q || !p->qkv || p->Vt || p->q_rs || p->q_nw)) bad = "form 1 takes Q, Kt, qkv and no Vt, q_rs, q_nw";
  else if (f == 2 && (!p->qkv || !p->q_rs || !p->q_nw || p->Q || p->Vt)) bad = "form 2 takes qkv, Kt, q_rs, q_nw and no Q, Vt";
  else if (p->B < 1 || p->S < 1 || p->H < 1) bad = "B, S, H >= 1";
  else if ((p->Dr & 7) || p->Dr <= 64 || p->Dr >= 96) bad = "Dr 72, 80 or 88 (a padded head on the D = 96 kernels: the ones row needs D > Dr)";
  else if (f == 2 && p->Dr != 88) bad = "form 2 needs Dr == 88";
  else if (f == 2 && (p->pipe < 0 || p->pipe > 2)) bad = "pipe 0, 1 or 2";
  else if (f == 2 && p->pipe_rows != 0 && p->pipe_rows != 256) bad = "pipe_rows 0 or 256";
  else if (f && ((p->ld & 7) || (long long)p->ld < 3ll * p->H * p->Dr)) bad = "ld % 8 == 0, ld >= 3 H Dr";
  if (bad) return fail(ctx, GVL_ERR_ARG, std::string("gvl_op_iv2_attention: ") + bad);
  AttnArgs a; memset(&a, 0, sizeof(a));
  a.Q = p->Q; a.Kt = p->Kt; a.Vt = p->Vt; a.O = p->out; a.B = p->B; a.H = p->H; a.KV = p->H; a.S = p->S; a.D = pad_head(p->Dr); a.Dout = p->Dr;
  a.scale = p->scale; a.causal = 0; a.ones_row = 1;
  if (f) { a.Vrows = p->qkv + (size_t)2 * p->H * p->Dr; a.v_ld = p->ld; }
  if (f == 2) { a.Qrows = p->qkv; a.q_ld = p->ld; a.q_rs = p->q_rs; a.q_nw = p->q_nw; a.k_ones = 1; a.pipe = p->pipe; a.pipe_rows = p->pipe_rows; }
  {
    auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    AttnGeometry g{};
    g.B = a.B; g.H = a.H; g.KV = a.KV; g.S = a.S; g.D = a.D; g.Dout = a.Dout; g.ones_row = 1; g.k_ones = a.k_ones; g.pipe = a.pipe; g.pipe_rows = a.pipe_rows;
    g.v_ld = a.v_ld; g.q_ld = a.q_ld; g.Vrows = a.Vrows; g.Qrows = a.Qrows; g.q_rs = a.q_rs; g.q_nw = a.q_nw;
    g.O16 = al16(a.O); g.Vrows16 = al16(a.Vrows); g.Qrows16 = al16(a.Qrows); g.Krows16 = true; g.q_nw16 = al16(a.q_nw);
    AttnLaunch l[GVL_ATTN_MAX_LAUNCHES];
    const int n = attn_plan(g, GVL_ATTN_KNOBS_DEFAULT, l);
    if (n < 0) return fail(ctx, GVL_ERR_ARG, "gvl_op_iv2_attention: attn_plan does not serve this launch (at most 256 key tiles, out / qkv / q_nw 16-byte aligned, a 64-row tile of qkv below 4 GiB)");
    if (!l[0].ONES) return fail(ctx, GVL_ERR_ARG, "gvl_op_iv2_attention: the plan chose no ONES kernel for this launch");
  }
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
  if (!ctx) return GVL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  GemvArgs g; memset(&g, 0, sizeof(g)); g.W = W; g.N = N; g.K = K; g.x = x; g.bias = bias; g.out_f32 = y;
  RUN(GVL_PROF_GEMV, 2.0 * N * K, gvl_launch_gemv(g, st));
  return 0;
}

}  // extern "C"
