// gvl_model.hip -- host side of libgvl.so: context, packed weights, workspace arenas, paged KV pool and the C ABI of include/gvl.h except its token-selection part (gvl_select.hip):
// the towers, splice, the sequence / prefill / decode entry points over the sequence table (gvl_seq_table.h); the operator-level entries live in gvl_ops.hip.  The launch sequences behind the ABI live in gvl_vision.hip
// (CLIP, InternVideo2, glue / projectors) and gvl_llm.hip (prefill, decode step, decode loop); gvl_model.h is what the four share.  Restates (file:line in the reference):
//   splice          models/llava_next_video.py:568-596
//   generate()      models/llava_next_video.py:655-661 (greedy; transformers GenerationMixin [ext])
#include "gvl_model.h"
#include "gvl_prefill_plan.h"   // prefill_group_size: how the *_varlen entry points cut their sequences into llm_prefill groups

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

}  // extern "C"
