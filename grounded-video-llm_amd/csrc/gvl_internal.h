// gvl_internal.h -- shared declarations for the libgvl.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gvl_grammar.h"   // decoding grammars: blob header and walk, shared with the host

typedef uint16_t bf16_t;  // raw bf16 bits

// Kernel-selection switches of the A/B history exist only in LAB builds (GVL_BUILD_DEFS=-DGVL_LAB, tools/): the shipped library
// reads no such environment variable -- neither per launch nor per token.  Deployment knobs (GVL_RCCL_LIB, GVL_KV_FRACTION) are documented in
// include/gvl.h; result-neutral launch parameters that tests vary go through gvl_debug_set().
#include <cstdlib>
#ifdef GVL_LAB
inline const char* gvl_lab_env(const char* name) { return getenv(name); }
#else
inline const char* gvl_lab_env(const char*) { return nullptr; }
#endif

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;   // MFMA A/B operand (4 VGPRs)
typedef __attribute__((ext_vector_type(16))) float f32x16_t;   // 32x32 MFMA accumulator
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;

#define GVL_KV_PAGE 64          // tokens per KV page == key tile of the attention kernels
#include "gvl_limits.h"       // GVL_MAX_DECODE_BATCH, GVL_MAX_VALU_BATCH, GVL_MAX_PREFILL_BATCH (shared with the host-only launch plans)
constexpr int GVL_GEMM_ROT_LEN = 64;     // GemmArgs.rot entries (a power of two; longer walks repeat the table)

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE attribute of a kernel: a host may hold one gvl_ctx per device in ONE process
// (include/gvl.h allows it), so "set once" means once per device ordinal -- a process-global flag would leave the second device at the
// 64 KB default and its first big-LDS launch would fail.  One bit per ordinal (mod 64); racing first launches set it twice, harmlessly.
#include <atomic>
#include <vector>
struct GvlDevOnce { std::atomic<unsigned long long> mask{0}; };
inline int gvl_set_max_lds(GvlDevOnce& once, const void* kern, int bytes) {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess) return -3;
  const unsigned long long bit = 1ull << (d & 63);
  if (!(once.mask.load(std::memory_order_acquire) & bit)) {
    if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return -3;
    once.mask.fetch_or(bit, std::memory_order_release);
  }
  return 0;
}

// ---- device helpers ---------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
__device__ __forceinline__ float bf2f(bf16_t h) { return __uint_as_float(((unsigned)h) << 16); }
// float -> bf16 round-to-nearest-even: the (__bf16) cast lowers to v_cvt_pk_bf16_f32 on gfx950
__device__ __forceinline__ bf16_t f2bf(float f) { const __bf16 b = (__bf16)f; return __builtin_bit_cast(unsigned short, b); }
__device__ __forceinline__ unsigned pack2bf(float lo, float hi) {
  const bf16x2_t v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float rbf(float f) { return (float)(__bf16)f; }  // round through bf16
// fast transcendental helpers for epilogues (errors << bf16 resolution)
__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float lo_bf(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float hi_bf(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// global -> LDS DMA, 16 bytes per lane, issued from inline asm so that hipcc does NOT count it in its vmcnt
// bookkeeping (a builtin glds makes the compiler drain vmcnt(0) before the next LDS read: it cannot prove the
// DMA destination and the ds_read source are different ring slots).  The caller owns the waits:
// `s_waitcnt vmcnt(N)` + a barrier before any wave reads the slot.  LDS destination = lds_dst (wave-uniform
// byte address, via M0) + lane*16; gsrc is per lane.  Recipe: cdna_hip_programming.md §5.7.
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_dst)
               : "memory");
}
// Four DMA pieces from ONE wave-uniform 64-bit base (SGPR pair) + per-lane 32-bit byte offsets: no per-piece 64-bit VALU
// address arithmetic in the issuing phase.  lds_dst0 + q*lds_step is piece q's wave-uniform LDS byte address.
__device__ __forceinline__ void glds16x4(const void* sbase, unsigned v0, unsigned v1, unsigned v2, unsigned v3, unsigned lds_dst0, unsigned lds_step) {
  unsigned keep, d;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %7\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %6\n\t"
      "s_add_u32 %1, %7, %8\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %6\n\t"
      "s_add_u32 %1, %1, %8\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, %6\n\t"
      "s_add_u32 %1, %1, %8\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %5, %6\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep), "=&s"(d)
      : "v"(v0), "v"(v1), "v"(v2), "v"(v3), "s"(sbase), "s"(lds_dst0), "s"(lds_step)
      : "memory", "scc");
}
// N pieces (N = 2 or 3) from one SGPR base, LDS destinations lds_dst0 + q*lds_step  (attention K / V^T tiles)
template <int N>
__device__ __forceinline__ void glds16xn(const void* sbase, const unsigned (&v)[N], unsigned lds_dst0, unsigned lds_step) {
  static_assert(N == 2 || N == 3, "2 or 3 pieces");
  unsigned keep, d;
  if constexpr (N == 3) {
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %6\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %5\n\t"
        "s_add_u32 %1, %6, %7\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %5\n\t"
        "s_add_u32 %1, %1, %7\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, %5\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep), "=&s"(d)
        : "v"(v[0]), "v"(v[1]), "v"(v[N - 1]), "s"(sbase), "s"(lds_dst0), "s"(lds_step)
        : "memory", "scc");
  } else {
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %4\n\t"
        "s_add_u32 %1, %5, %6\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %4\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep), "=&s"(d)
        : "v"(v[0]), "v"(v[1]), "s"(sbase), "s"(lds_dst0), "s"(lds_step)
        : "memory", "scc");
  }
}
__device__ __forceinline__ unsigned lds_addr(const void* p) {   // 32-bit LDS byte address of a __shared__ pointer
  return (unsigned)(unsigned long)(__attribute__((address_space(3))) const void*)p;
}

// ---- GEMM ---------------------------------------------------------------------------------------
enum { GVL_ACT_NONE = 0, GVL_ACT_QUICK_GELU = 1, GVL_ACT_GELU = 2, GVL_ACT_SILU_MUL = 3 };

struct GemmArgs {
  const bf16_t* A;  int lda;     // [M,K] bf16
  const bf16_t* W;  int ldw;     // [N,K] bf16 (nn.Linear layout); ldw = row pitch in elements (0: K)
  void* C;          int ldc;     // [M,N'] f32 or bf16
  int M, N, K;
  const float* bias;             // [N] or null
  const float* gamma;            // [N] LayerScale (after bf16 rounding of acc+bias) or null
  const void* resid; int ldr;    // residual stream, same dtype as C, or null (may alias C)
  int act;                       // GVL_ACT_*
  int out_f32;                   // 1: C/resid f32, 0: bf16
  int round_pre_resid;           // 1: round (acc+bias) [and the gamma product] to bf16 before adding resid
  // output row remap: row m -> (m / grp_rows) * grp_stride + (m % grp_rows) + row_off   (grp_rows==0: identity)
  int grp_rows, grp_stride, row_off;
  int tile_cfg;                  // 0 auto; GVL_CFG_* (gvl_gemm_plan.h)
  int band;                      // ping-pong kernel: tile ROWS per rasterisation band (0 = the launcher's choice); any value gives the same result
  unsigned char rot[64];         // pipelined 4-wave kernel: workgroup c of an XCD takes offset (c + rot[round & 63]) mod (workgroups of the XCD) of its XCD's round (0: fixed)
  int narrow;                    // set by gvl_launch_gemm for the pipelined 4-wave kernel: tiles with <= 128 real columns run its narrow statements (gvl_debug_set "gemm_narrow"); result-neutral
  int m_begin;                   // launch covers rows [m_begin, M) -- set internally by the wave-quantisation split
  // Fused RMSNorm (round 5).  CONSUMER side: rowscale[m] (f32, [M]) multiplies row m of the accumulator BEFORE bias / activation -- RMSNorm(x) . W^T =
  // rs[m] * (x . (W diag(gamma))^T): A is the RAW residual stream, W carries the norm weight (gvl_fold_gamma), rs = rsqrt(mean x^2 + eps).
  // PRODUCER side: rowsq[m * rowsq_ld + n / 64] (f32) receives the sum of squares of the bf16-ROUNDED outputs of row m over each aligned block of 64
  // columns -- the statistics the NEXT norm needs, taken while the row piece is in registers (N % 64 == 0; bf16 output; staged epilogue only).
  const float* rowscale;
  float* rowsq; int rowsq_ld;
  const float* act_table;        // set by the launcher: Phi(x) table for the erf-GELU epilogue of the ping-pong kernel (see gvl_gemm.hip)
  unsigned long long* dbg;       // null, or [grid][8 waves][4] s_memtime stamps of the LAST tile (GVL_GEMM_TIMING=1, ping-pong kernel)
};
// Rasterisation band of the 256 x 256 kernels: an XCD's 32 workgroups walk a band of this many tile rows column by column.  4 since round 6: the A panel of a
// band (1 024 rows x K) then fits the XCD's 4 MiB L2 for K <= 1 408 and halves the A re-reads of the wide matrices; same-box A/B of the bench step with the 4-wave
// kernels: 8 -> 4 rows = 701 -> 686 ms per step (-2.1 %), 2 / 3 / 6 / 16 rows: 694 / 688 / 692 / 732 (profiles/r06_ab_gemm_band.json; per shape: iv2.fc2 +3.7 %,
// phi.down +4.9 %, the others within +-1.5 %: profiles/r06_gemm_band_shapes.txt).  (Round 5 had tried 5-row bands for N = 1408 only, on the 8-wave kernel.)
constexpr int GVL_GEMM_BAND = 4;
int gvl_launch_gemm(const GemmArgs& a, hipStream_t st);   // gemm_plan (gvl_gemm_plan.h) + dispatch on the planned forms
int gvl_device_cus();                                     // compute units of the current device, unmasked (see gvl_gemm.hip)
// gvl_gemm4.hip / gvl_gemm4p.hip: the 4-wave / AGPR-accumulator form of the 256 x 256 kernel for the staged bf16 epilogue code `epi` (loop schedule variant `var`), and
// the same kernel with the epilogue software-pipelined into the next tile's main loop.  Template switches only: gemm_plan decides whether they serve a launch.
int gvl_launch_gemm_a4(const GemmArgs& a, int epi, int var, hipStream_t st);
int gvl_launch_gemm_a4p(const GemmArgs& a, int epi, hipStream_t st);
void gvl_gemm_set_a4(int v);     // A/B: 0 = the 256 x 256 launches stay on the 8-wave ping-pong kernel, 1 (default) = the 4-wave kernel where it is faster, 2 = wherever it serves
void gvl_gemm_set_narrow(int v); // A/B: 0 = the pipelined 4-wave kernel runs a half-empty column tile (N = 1408: every sixth) as a full one (rounds <= 6a), 1 (default) = as a narrow tile
void gvl_gemm_set_band(int v);   // A/B: tile rows per rasterisation band of the ping-pong kernel for every later launch of the process (0 = automatic)
double gvl_gemm_flops(const GemmArgs& a);
// GVL_GEMM_TIMING probes (LAB builds): `launch` runs with a zeroed buffer of n 64-bit cycle stamps in GemmArgs.dbg; once it has finished, `report` gets the stamps
template <class Launch, class Report>
inline int gvl_gemm_probe_launch(GemmArgs a, size_t n, hipStream_t st, Launch&& launch, Report&& report) {
  if (hipMalloc((void**)&a.dbg, n * 8) != hipSuccess) return -3;
  hipMemsetAsync(a.dbg, 0, n * 8, st);
  launch(a);
  std::vector<unsigned long long> hbuf(n);
  hipStreamSynchronize(st);
  hipMemcpy(hbuf.data(), a.dbg, n * 8, hipMemcpyDeviceToHost);
  hipFree(a.dbg);
  report(hbuf);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---- attention (prefill / vision) -----------------------------------------------------------------
struct AttnArgs {
  const bf16_t* Q;      // [B][H][S][D] bf16 (D = padded head dim: 64, 96 or 128)
  const bf16_t* Kt;     // key pages  [page][KV][64][D]
  const bf16_t* Vt;     // value pages [page][KV][D][64]  (transposed inside the page)
  const bf16_t* Vrows;  // null, or V as token rows: V[b][s][kv head][0..Dout) = Vrows[(b*S + s)*v_ld + head*Dout + d] (the fused-qkv GEMM output of a
  int v_ld;             //   vision tower, read in place: no V^T pass); then Vt is unused and block_table must be null
  const bf16_t* Qrows; const bf16_t* Krows;   // both null, or (with Vrows; D == Dout == 64) q and k as token rows too: Qrows[(b*S + s)*q_ld + head*D + d], Krows likewise
  int q_ld, k_ld;       //   -- a tower whose q / k need no per-token transform (CLIP) runs no qkv_post pass; then Q / Kt are unused
  int k_ones;           // the K pages' pad column Dout holds 1.0 (QkvPostArgs.k_ones): required by the q_rs mode, which folds the softmax shift into the S^T MFMAs
  const float* q_rs; const bf16_t* q_nw;      // both null, or (Qrows set, Krows null, Vrows set): q needs the full-width RMSNorm of InternVideo2 --
                        //   q'[d] = q_nw[head*Dout + d] * bf16(q[d] * q_rs[token]) applied to the fragments as they are loaded (K stays in pages)
  bf16_t* O;            // [B][S][H*Dout]
  const int* block_table;  // [B][max_pages] page ids, or null: page(b,t) = b*n_tiles + t
  int max_pages;
  int B, H, KV, S, D, Dout;   // S = number of queries; keys: Sk (0 = S, plain self attention)
  int Sk, qpos0;              // extend-prefill (gvl_prefill_extend): query i sits at position qpos0 + i of a context of Sk = qpos0 + S keys (causal: key <= qpos0 + i)
  float scale;
  int causal;
  int ones_row;         // D > Dout only: V^T pad row Dout holds 1.0 for every key (QkvPostArgs.ones_row), so the P.V MFMAs deliver the
                        // softmax row sum in O^T[Dout] for free and the kernel drops its 32 VALU adds per key tile
  int ring;             // K/V LDS ring depth: 0 = launcher's choice, 2 or 3 (paged-KV path only)
  int pipe;             // 1: the q_rs (InternVideo2) mode takes the software-pipelined kernel attn_iv2_pipe_kernel; 0: attn_fwd_kernel (bit-identical); 2: its safe pass only
  int pipe_rows;        // 256: whole 256-row query blocks on the 8-wave form of that kernel, the rest on the 4-wave form; anything else (default): the 4-wave form for every row
  int q_begin, q_rows;  // set by the launcher: the query rows one attn_iv2_pipe_kernel launch covers
  float lazy;           // set by the launcher: the running max (and O) of a wave's rows is only moved when some row's tile max exceeds it by
                        // more than `lazy` (log2 units; 0 = every time it grows)
  // RAGGED causal prefill in one grid (paged K/V, B == 1, Sk == qpos0 == 0): vl_n > 0 sequences packed back to back -- sequence u owns rows
  // [vl_rows[u], vl_rows[u + 1]) of Q ([H][S_u][D] per sequence, at row offset vl_rows[u]) and O, and the block table vl_tables[u]; S = longest sequence
  int vl_n;
  int vl_rows[GVL_MAX_PREFILL_BATCH + 1];
  const int* vl_tables[GVL_MAX_PREFILL_BATCH];
  // ragged EXTEND prefill (gvl_launch_attention_ext only; every other launch ignores it): sequence u already holds vl_pos0[u] tokens (a multiple of 64, 0 = empty) --
  // its query i sits at position vl_pos0[u] + i and sees the vl_pos0[u] + S_u keys of vl_tables[u]
  int vl_pos0[GVL_MAX_PREFILL_BATCH];
};
int gvl_launch_attention(const AttnArgs& a, hipStream_t st);   // attn_plan (gvl_attn_plan.h: operand mode, instantiation, grid, LDS) + dispatch on the planned instantiation
int gvl_launch_attention_ext(const AttnArgs& a, hipStream_t st);   // attn_ext_plan + dispatch: the ragged form (vl_*) with a cached prefix per sequence (vl_pos0)
double gvl_attn_flops(const AttnArgs& a);

// ---- decode attention -----------------------------------------------------------------------------
struct DecodeAttnArgs {
  const bf16_t* q;        // [batch][H][D], q_stride elements apart
  const bf16_t* Kt; const bf16_t* Vt;   // page pools (one layer)
  const int* tables[GVL_MAX_DECODE_BATCH];   // per sequence: [max_pages]
  const int* pos_ptrs[GVL_MAX_DECODE_BATCH]; // per sequence, device: index of the new token (the cache holds *pos + 1 tokens, new one included)
  float* part;            // workspace [batch][H][nsplit][D+2]
  int* counters;          // [batch][H] arrival tickets, zero between launches (the merging block re-arms them)
  bf16_t* out;            // [batch][H*Dout], out_stride elements apart; out_tiled: B-operand tile order (gvl_xt_index) for the skinny decode GEMM
  int H, KV, D, Dout, nsplit, batch, q_stride, out_stride, out_tiled;
  float scale;
  int hpb;                // grouped-query kernel: query heads of a KV head served by one block (0 = all H / KV; must divide it); any value gives the same result
  int cpb;                // consecutive splits per block (0 = 1); any value gives the same result (one partial per split either way)
  int gsplit;             // block slots along the context actually launched (0 = ceil(nsplit / cpb)): the host may pass min(nsplit, ceil(longest context in pages / 4)) -- a
                          // sequence uses ceil(its pages / 4) splits whatever the grid offers, so this only trims blocks that would leave at once
};
int gvl_launch_decode_attention(const DecodeAttnArgs& a, hipStream_t st);   // decode_attn_plan (gvl_attn_plan.h: normalised batch / cpb / gsplit / hpb, instantiation, grid) + dispatch

// ---- elementwise / norm / glue kernels (gvl_elem.hip) ----------------------------------------------
int gvl_launch_layernorm_f32(const float* x, const float* w, const float* b, bf16_t* y, int rows, int cols, float eps, hipStream_t st);
int gvl_launch_rmsnorm_bf16(const bf16_t* x, const bf16_t* w, bf16_t* y, int rows, int cols, float eps, hipStream_t st);
int gvl_launch_copy_bytes(const void* src, void* dst, size_t bytes, hipStream_t st);   // device -> device, 16-byte vectors (falls back to hipMemcpyAsync for odd sizes)
int gvl_launch_fold_gamma(const bf16_t* W, const bf16_t* gamma, bf16_t* Wo, long rows, int cols, hipStream_t st);   // W' = bf16(W diag(gamma)): fused RMSNorm, consumer weights
int gvl_launch_rowsq_finish(const float* sq, int ld, int b0, int nblk, float* rs, int rows, int cols, float eps, hipStream_t st);   // partial sums of squares -> rsqrt(mean + eps)
// im2col for a stride==kernel patch conv.  px f32 [n_img][3][T][HW][HW] (T==1 for CLIP) -> A bf16 [n_img*T*g*g][Kp]
int gvl_launch_patchify(const float* px, bf16_t* A, int n_img, int T, int image, int patch, int Kp, hipStream_t st);
// CLIP embeddings + pre-LN: x[n,0]=cls+pos0, x[n,1+p]=bf16r(patch)+pos -> LN -> f32 [n,1+P,C]
int gvl_launch_clip_embed_ln(const bf16_t* patch, const float* cls, const float* pos, const float* lnw, const float* lnb,
                             float* x, int n_img, int P, int C, float eps, hipStream_t st);
// IV2 embeddings: x[b,0]=bf16(cls+pos0), x[b,1+j]=bf16(patch+pos) (all bf16) -> bf16 [B,1+TL,C]
int gvl_launch_iv2_embed(const bf16_t* patch, const bf16_t* cls, const bf16_t* pos, bf16_t* x, int B, int TL, int C, hipStream_t st);
// ---- fused patch embedding (gvl_patch.hip): im2col in the operand loader + patch GEMM + CLS / position rows (+ CLIP's pre-LayerNorm) as ONE kernel ----
struct PatchEmbedArgs {
  const float* px;        // f32 [n_img][3][T][image][image]
  const bf16_t* Wt;       // tile-order conv weight (gvl_retile_patch_weight): [C / 16][3 * patch / 2][64][8]
  int n_img, T, image, patch, C;
  int M;                  // patch rows = n_img * T * (image / patch)^2
  int S;                  // output rows per image (1 + T * L)
  int mode;               // 0: CLIP (x f32, LayerNorm), 1: InternVideo2 (x bf16, conv bias)
  const float* bias;      // mode 1: conv bias [C]
  const float *cls_f32, *pos_f32, *lnw, *lnb; float eps; float* x_f32;      // mode 0
  const bf16_t *cls_bf, *pos_bf; bf16_t* x_bf;                               // mode 1
};
int gvl_retile_patch_weight(const bf16_t* W, bf16_t* Wt, int C, int Kp, int p, hipStream_t st);
int gvl_launch_patch_embed(const PatchEmbedArgs& a, hipStream_t st);      // -1: geometry outside the fused kernel (caller takes the three-pass path)
// split a fused qkv row into attention operands.
//  mode 0 (CLIP): plain.  mode 1 (IV2): RMS-normalise q and k over the full width with weights qn/kn.
//  mode 2 (LLM): RoPE with cos/sin tables at positions pos0+s.
struct QkvPostArgs {
  const bf16_t* qkv; int ld;       // [B*S][(H+2KV)*Dr]
  bf16_t* Q; bf16_t* Kt; bf16_t* Vt;
  const int* block_table; int max_pages;   // null: page(b,t) = b*n_tiles + t
  int B, S, H, KV, Dr, D;          // Dr = real head dim, D = padded
  int mode;
  const bf16_t* qn; const bf16_t* kn; float eps;     // mode 1
  const float* cos; const float* sin; int pos0;      // mode 2: tables [max_seq][Dr/2] (already bf16-rounded values)
  int ones_row;                    // V^T pad row Dr (needs D > Dr) is filled with 1.0 instead of 0: see AttnArgs.ones_row
  int k_ones;                      // K pad column Dr (needs D > Dr) is 1.0 instead of 0 (harmless while q's pad is 0; see AttnArgs.k_ones)
  float* q_rs;                     // mode 1, or null: [B*S] -- the q rows are NOT written; their RMS factor rsqrt(mean q^2 + eps) is, and the attention
                                   //   kernel normalises the q fragments it loads from the qkv matrix itself (AttnArgs.q_rs / q_nw)
  // RAGGED prefill group in one launch (mode 2, B == 1, pos0 == 0; AttnArgs.vl_* on the attention side): vl_n > 0 sequences packed back to back -- sequence u owns
  // the rows [vl_rows[u], vl_rows[u + 1]) of qkv and of Q ([H][S_u][D] per sequence, at row offset vl_rows[u]) and the block table vl_tables[u]; S is ignored
  int vl_n;
  int vl_rows[GVL_MAX_PREFILL_BATCH + 1];
  const int* vl_tables[GVL_MAX_PREFILL_BATCH];
  // ragged EXTEND group (gvl_launch_qkv_post_ext only; qkv_post_kernel / v_transpose_kernel never read it): sequence u already holds vl_pos0[u] tokens (a multiple
  // of 64) -- RoPE position, page and slot of its row i come from vl_pos0[u] + i, its V^T tile t starts at token vl_pos0[u] + 64 t
  int vl_pos0[GVL_MAX_PREFILL_BATCH];
};
int gvl_launch_qkv_post(const QkvPostArgs& a, hipStream_t st);
int gvl_launch_qkv_post_ext(const QkvPostArgs& a, hipStream_t st);   // mode 2 ragged group with vl_pos0: qkv_post_ext_kernel + v_transpose_ext_kernel, one launch each
// HD 2x2 merge + sub_GN newline (Phi): f32 [n,576,C] -> bf16 [n,156,4C]
int gvl_launch_hd_merge(const float* f, const float* sub_gn, bf16_t* out, int n, int C, hipStream_t st);
// 3x3 block mean (Llama): f32 [n,576,C] -> bf16 [n,64,C]
int gvl_launch_pool_spatial(const float* f, bf16_t* out, int n, int C, hipStream_t st);
// temporal 4x4 block mean: bf16 [n,T*256,C] -> bf16 [n,T*16,C]
int gvl_launch_pool_temporal(const bf16_t* f, bf16_t* out, int n, int T, int C, hipStream_t st);
// broadcast one row to rows row_off + s*stride, s in [0,n)
int gvl_launch_bcast_row(const bf16_t* row, bf16_t* dst, int n, int stride_rows, int row_off, int cols, hipStream_t st);
// embedding gather: ids (device int32) -> rows of dst
int gvl_launch_gather_rows(const bf16_t* table, const int* ids, bf16_t* dst, int n, int cols, hipStream_t st);
int gvl_launch_strip_cls(const void* x, void* y, int n, int S, int C, int elem_bytes, hipStream_t st);
// decode-side
struct GemvArgs {
  const bf16_t* W; int N, K;      // [N][K]
  const bf16_t* x;                // [batch][K] bf16, rows x_stride elements apart
  const bf16_t* norm_w; float eps;  // non-null: x <- rmsnorm(x)*norm_w (bf16 roundings as the reference)
  const float* bias;              // [N] or null
  const bf16_t* resid;            // [batch][N'] or null: out = bf16(resid + bf16(y)); rows out_stride apart
  int act;                        // GVL_ACT_NONE or GVL_ACT_SILU_MUL (interleaved gate/up rows, N' = N/2)
  bf16_t* out_bf16;               // [batch][N'] or null, rows out_stride apart
  float* out_f32;                 // [batch][N'] or null, rows out_stride apart
  int batch, x_stride, out_stride;   // batch 0/1 = one vector (strides ignored)
  // fused decode epilogue of the qkv projection (rope_on): RoPE on q/k at the sequence's position, q -> Q[b][H][D], k/v appended
  // to that sequence's pages.  Rows are visited in (d, d+Dr/2) partner pairs so one lane owns both halves of a rotation.
  int rope_on; const float *cos_s, *sin_s, *cos_l, *sin_l; int rope_switch;
  const int* pos_ptrs[GVL_MAX_DECODE_BATCH]; const int* tables[GVL_MAX_DECODE_BATCH];   // per sequence of the batch
  bf16_t *Q, *Kt, *Vt; int H, KV, Dr, D; int q_stride;
  int variant;                    // skinny-GEMM path: kernel variant (0 = default; tools/decode_bench.py)
  int w_fp8; const float* wscale; // skinny-GEMM path: 1 = W is the FP8 tile copy, wscale[N] its per-row power-of-two scales; 2 = the MXFP4 tile
                                  // copy, wscale = its E8M0 scale words (gvl_mxfp4_quantise_decode_weight)
  int out_tiled;                  // skinny-GEMM path: the SwiGLU epilogue writes out_bf16 in B-operand tile order (it feeds down_proj)
  // Fused RMSNorm on the decode path (round 5; skinny-GEMM path, bf16 weights): rmsnorm(x) W^T = rs[b] * (x (W diag gamma)^T) per sequence b.
  //   PRODUCER (o_proj / down_proj, the residual epilogue; N % 16 == 0): sq_out[b * (N / 16) + block] = sum of squares of the 16 bf16 outputs of that row
  //   block for sequence b, and out_tiled2 = a second copy of the new residual rows in B-operand tile order (the next projection's x);
  //   CONSUMER (qkv_proj / gate_up_proj / lm_head; W = the tile copy of the norm-FOLDED weight, x = that raw tiled stream): sq_in[b * sq_n + j], j < sq_n,
  //   are summed in a fixed order by the epilogue waves while the first weight tiles are in flight; the accumulators are scaled by rsqrt(sum / K + eps).
  // A sequence's sums and scale depend on its own column only: batched decode == single decode still holds bit for bit.
  const float* sq_in; int sq_n;
  float* sq_out; bf16_t* out_tiled2;
};
// B-operand tile order of the decode activations: element (sequence j < 16, column k) of a [16][cols] matrix lives at
// [k / 32][lane = 16 * ((k / 8) % 4) + j][k % 8] -- one k step of the MFMA is 1 KiB of consecutive addresses
__host__ __device__ __forceinline__ size_t gvl_xt_index(int j, int k) { return ((size_t)(k >> 5) * 64 + (size_t)(((k >> 3) & 3) * 16 + j)) * 8 + (k & 7); }
int gvl_retile_decode_weight(const bf16_t* W, bf16_t* Wt, int N, int K, int Dr, int n_qk_heads, hipStream_t st);
// FP8 variant: scale[n] (per logical row, power of two), Wt8 = e4m3 tile copy, and W (row-major bf16) REPLACED by its de-quantised values
int gvl_fp8_quantise_decode_weight(bf16_t* W, unsigned char* Wt8, float* scale, int N, int K, int Dr, int n_qk_heads, hipStream_t st);
// MXFP4 twin: Wt4 [ceil(N/16)][K/128][64][16] bytes, scale [ceil(N/16)][K/128][16] words of four E8M0 bytes; W is replaced by the de-quantised values
int gvl_mxfp4_quantise_decode_weight(bf16_t* W, unsigned char* Wt4, unsigned* scale, int N, int K, int Dr, int n_qk_heads, hipStream_t st);
int gvl_launch_rows_to_tiled(const bf16_t* x, bf16_t* xt, int batch, int cols, int stride, hipStream_t st);
int gvl_launch_gemv(const GemvArgs& a, hipStream_t st);
// the same projection as ONE MFMA skinny GEMM for 1..16 sequences (gvl_decode.hip); -1 when the geometry needs the VALU kernel
int gvl_launch_dgemm(const GemvArgs& a, hipStream_t st);
// greedy sampling for `batch` logit rows (stride n): token -> *tok_ptrs[b] and out_lists[b][steps[b]]
// small host int list passed to kernels by value (stream ordered, no host / staging buffer lifetime)
struct IntList { int v[256]; int n; };
// dst[r] = table[host_ids[r]], ids travel in the kernel arguments (256 per launch)
int gvl_launch_gather_rows_host_ids(const bf16_t* table, const int* host_ids, int n, bf16_t* dst, int cols, hipStream_t st);
// loss tail of the training forward: nll[r] = logsumexp(logits[r]) - logits[r][targets[r]] (f32 on bf16 logits)
int gvl_launch_ce_rows(const bf16_t* logits, int ld, const int* targets, float* nll, int n, int V, hipStream_t st);
// token -> *tok_ptrs[b] and out_lists[b][*ngen_ptrs[b]]; then (*ngen_ptrs[b])++ and, when non-null, (*pos_ptrs[b])++ (the step's
// bookkeeping lives on the device: a decode step's launches carry no host-side counters)
struct ArgmaxArgs { const float* logits; int n, batch; int* tok_ptrs[GVL_MAX_DECODE_BATCH]; int* out_lists[GVL_MAX_DECODE_BATCH];
                    int* ngen_ptrs[GVL_MAX_DECODE_BATCH]; int* pos_ptrs[GVL_MAX_DECODE_BATCH];
                    // sampling (gvl_launch_sample only): scores / temperature -> top-k -> top-p -> one draw per row; the draw of row b is a
                    // pure function of (seed, stream[b], generation step, logits row), i.e. independent of how sequences are grouped
                    // eos watch (gvl_decode_greedy*): when row b's token == eos_id, its generation count is stored (once) into the host-mapped word
                    // eos_flags[b] -- the host reads it two steps behind the GPU instead of draining the stream every 16 steps
                    int eos_id; int* eos_flags[GVL_MAX_DECODE_BATCH];
                    float inv_temp, top_p; int top_k; unsigned seed_lo, seed_hi; unsigned stream[GVL_MAX_DECODE_BATCH];
                    const int* step_override;      // operator tests: generation step of row b when the row has no ngen counter
                    // log-probabilities (after every field above: the kernel-argument offsets of the off instantiations stay put).  Row b is on
                    // when top_n[b] >= 0 and lp_lists[b] is set: lp_lists[b][g] = log-probability of its token under the distribution it was
                    // selected from; top_n[b] = 1 .. GVL_MAX_TOP_LOGPROBS (with top_ids / top_lp set) also stores the best top_n entries at
                    // [g * GVL_MAX_TOP_LOGPROBS ..) and pads the remaining slots with (-1, -inf).  g = *ngen_ptrs[b] (0 without a counter), as for out_lists.
                    int top_n[GVL_MAX_DECODE_BATCH]; float* lp_lists[GVL_MAX_DECODE_BATCH]; int* top_ids[GVL_MAX_DECODE_BATCH]; float* top_lp[GVL_MAX_DECODE_BATCH]; };
constexpr int GVL_MAX_TOP_LOGPROBS = 8;
int gvl_launch_argmax(const ArgmaxArgs& a, hipStream_t st);
int gvl_launch_sample(const ArgmaxArgs& a, hipStream_t st);
// Per-row selection (select_rows_kernel, gvl_pick.hip): every row of one launch is greedy (on = 0) or sampled with its OWN settings, seed and stream.  A sampled row runs HF's
// warpers in HF's order -- scores / T -> top-k -> top-p -> min_p -> typical_p -> epsilon_cutoff -> eta_cutoff (0 = off each; top_p / typical_p also off at 1) -> one Gumbel-max
// draw -- each stage's softmax over what the stage before left.  The kept set is an interval [lo, hi] of smp_key() keys after every stage.  `am` carries the rows'
// pointers and log-probability outputs with ArgmaxArgs' meaning; its inv_temp / top_k / top_p / seed / stream fields are not read.  kept (operator tests, may be null):
// kept[b * n + i] = 1 iff entry i of row b is finite and in the final kept set (a greedy row keeps every finite entry).
struct SelRow { int on; float inv_temp; int top_k; float top_p, min_p, typical_p, eps, eta; unsigned seed_lo, seed_hi, stream; };
struct SelRowsArgs { ArgmaxArgs am; SelRow row[GVL_MAX_DECODE_BATCH]; unsigned char* kept; };
int gvl_launch_select_rows(const SelRowsArgs& a, hipStream_t st);
// Beam search, one step's candidates (beam_rows_kernel + beam_merge_kernel, gvl_pick.hip): rows [k] of n fp32 entries, row b at rows + b * row_stride (0: every beam reads
// row 0 -- the first step); norm != 0: raw logits, log-softmax inside; 0: processed log-probabilities.  row_* [k][2k]: device scratch between the two launches.  vals / idx /
// proc [2k]: the best 2k of the k x n grid in the order (value descending, flat index beam * n + token ascending) -- value = fp32(log-prob + scores[beam]), proc = the log-prob.
struct BeamCandArgs { const float* rows; int n, k, row_stride, norm; float scores[GVL_MAX_DECODE_BATCH]; float* row_v; int* row_i; float* row_lp; float* vals; int* idx; float* proc; };
int gvl_launch_beam_candidates(const BeamCandArgs& a, hipStream_t st);
// One GROUP of diverse beam search (gvl_group_beam_search): c describes the group's s = c.k rows (1 .. 16; n >= 2s), scores and the 2s outputs exactly as above; behind the
// merge the same wave writes the group's choice -- the tokens of the first s candidates that are not `eos` (eos < 0: none; fewer than s: -1 for the rest) -- to
// current[0 .. s), device memory the next group's Hamming stage reads, and to mirror[0 .. s) (may be null).  done != 0: no candidates at all, current / mirror <- pad
// (pad < 0: -1, an id that counts nowhere).
struct BeamGroupArgs { BeamCandArgs c; int* current; int* mirror; int eos, pad, done; };
int gvl_launch_beam_group(const BeamGroupArgs& a, hipStream_t st);
int gvl_launch_beam_normalize(float* rows, int n, int k, hipStream_t st);      // rows [k][n] raw logits -> log-softmax, in place (beam_rows_kernel<true>'s arithmetic)
// Classifier-free guidance (guidance_rows_kernel, gvl_pick.hip): pair p overwrites the n fp32 entries at cond[p] with scale[p] * (lc - lu) + lu, lc / lu the log-softmax
// of cond[p] / neg[p] in beam_normalize_kernel's arithmetic; neg[p] is only read.  The conditional rows of one launch are distinct and none is another pair's negative row.
// follow_commit_kernel: follower p takes the token at lead_tok[p] (its leader's, just selected) into tok[p] and out[p][*ngen[p]], then (*ngen[p])++ and, when non-null,
// (*pos[p])++.  Both launches carry device pointers and by-value constants only: a captured decode step replays them.
constexpr int GVL_MAX_GUIDANCE_PAIRS = GVL_MAX_DECODE_BATCH / 2;
struct GuidanceArgs { int n, n_pairs; float* cond[GVL_MAX_GUIDANCE_PAIRS]; const float* neg[GVL_MAX_GUIDANCE_PAIRS]; float scale[GVL_MAX_GUIDANCE_PAIRS]; };
struct FollowArgs { int n; const int* lead_tok[GVL_MAX_GUIDANCE_PAIRS]; int* tok[GVL_MAX_GUIDANCE_PAIRS]; int* out[GVL_MAX_GUIDANCE_PAIRS]; int* ngen[GVL_MAX_GUIDANCE_PAIRS];
                    int* pos[GVL_MAX_GUIDANCE_PAIRS]; };
struct PairLaunches { GuidanceArgs g; FollowArgs f; };   // what a group with pairs adds around its selection (pick_tokens, gvl_llm.hip)
int gvl_launch_guidance_rows(const GuidanceArgs& a, hipStream_t st);
int gvl_launch_follow_commit(const FollowArgs& a, hipStream_t st);
// Teacher-forced scoring (score_rows_kernel, gvl_pick.hip): `rows` rows of n fp32 logits, ld floats apart, any number of them; targets [rows] on the device.  Per row: lp [rows]
// the target's log-probability under the raw row, rank [rows] how many entries beat it (value descending, lower id first), and with top_n 1 .. 8 the best top_n finite
// entries as top_ids / top_lp [rows][GVL_MAX_TOP_LOGPROBS], padded with (-1, -inf) (top_n == 0: never touched, may be null).
struct ScoreRowsArgs { const float* logits; int n, ld, rows, top_n; const int* targets; float* lp; int* rank; int* top_ids; float* top_lp; };
int gvl_launch_score_rows(const ScoreRowsArgs& a, hipStream_t st);
// fp32 out[r][c0 + j] = x[r] . W[c0 + j] (+ bias[c0 + j]), r < rows, j < nc: the few lm_head columns past the last multiple of 16, which the score tail's GEMM does not take
int gvl_launch_head_cols(const bf16_t* x, int ldx, const bf16_t* W, int K, const float* bias, float* out, int ld, int c0, int nc, int rows, hipStream_t st);
// HF logits processors (repetition penalty -> no-repeat n-gram -> min length) on `batch` fp32 rows (stride ld), in place (gvl_logits.hip).  Row b's
// history is hist[b][0 .. *len_ptrs[b]) (clamped to cap <= GVL_LOGITS_HIST_CAP; a null len_ptrs[b] = empty history); penalty 1 / ngram 0 /
// min_new 0 switch a processor off; eos < 0 switches the min-length ban off.
constexpr int GVL_LOGITS_HIST_CAP = 8192;   // = the sequences' output-list capacity (gvl_ctx::outlist_cap)
// Token rules of a row (gvl_rules_create): sequence_bias -> [penalty -> n-gram] -> bad_words_ids -> [min length] -> forced eos -> suppress ->
// begin suppress.  One immutable device blob of 32-bit words that starts with this header; every off_* is a word offset from the blob's start.
// A bias table (stage 0 = sequence_bias, 1 = bad_words_ids) is grouped BY TARGET TOKEN: targets [n_tgt][3] = (target id, first entry, entries);
// entries [..][3] = (fp32 bias bits, prefix offset into the stage's prefix ids, prefix length 0 .. GVL_RULES_MAX_SEQ_LEN - 1), a target's
// length-1 entry first, then its multi-token entries in the caller's (dict) order.  Targets of one table are distinct.
constexpr int GVL_RULES_MAX_IDS = 1 << 18;     // ids of one single-token list (suppress, begin suppress, forced eos) / length-1 entries of one table
constexpr int GVL_RULES_MAX_SEQS = 1024;       // multi-token entries of one table
constexpr int GVL_RULES_MAX_SEQ_LEN = 16;      // ids of one multi-token entry
struct TokenRulesDev { int n_suppress, off_suppress, n_begin, off_begin, begin_at, n_force, off_force, force_at, n_multi;
                       int n_tgt[2], off_tgt[2], off_ent[2], off_pre[2]; };
// A decoding grammar of a row (gvl_grammar_create; gvl_grammar.h holds the blob's layout and the walk): after the min-length ban, before forced eos -- HF's
// PrefixConstrainedLogitsProcessor.  The mask is a pure function of the blob and the row's history; no state is kept between launches.
using GrammarDev = gvl_grammar::Header;
static_assert(gvl_grammar::HIST_CAP == GVL_LOGITS_HIST_CAP, "the walk covers exactly the staged history");
// rules[b]: null = row b has no token rules; any row non-null selects the kernel's second instantiation (after every field the first one reads)
// grammar[b]: null = row b has no grammar; any row non-null selects the third instantiation (after every field the other two read)
struct LogitsProcArgs { float* logits; int n, ld, batch, cap; const int* hist[GVL_MAX_DECODE_BATCH]; const int* len_ptrs[GVL_MAX_DECODE_BATCH];
                        float penalty[GVL_MAX_DECODE_BATCH]; int ngram[GVL_MAX_DECODE_BATCH], min_new[GVL_MAX_DECODE_BATCH], eos[GVL_MAX_DECODE_BATCH];
                        const TokenRulesDev* rules[GVL_MAX_DECODE_BATCH];
                        const GrammarDev* grammar[GVL_MAX_DECODE_BATCH];
                        // diverse beam search (after every field the other instantiations read): ham_n[b] > 0 in any row selects logits_process_hamming_kernel --
                        // row b loses ham_lambda[b] x (how often the token occurs among the ham_n[b] <= 16 ids at ham_tok[b], DEVICE memory read at run time)
                        const int* ham_tok[GVL_MAX_DECODE_BATCH]; int ham_n[GVL_MAX_DECODE_BATCH]; float ham_lambda[GVL_MAX_DECODE_BATCH]; };
int gvl_launch_logits_process(const LogitsProcArgs& a, hipStream_t st);
// x[b][:] = table[*tok_ptrs[b]][:] for the sequences of the batched decode loop
struct TokPtrs { const int* p[GVL_MAX_DECODE_BATCH]; int n; };
int gvl_launch_gather_tok_rows(const bf16_t* table, const TokPtrs& toks, bf16_t* dst, int cols, hipStream_t st);
// x[b] = table[*toks.p[b]] and xn[b] = bf16(w * bf16(x[b] * rstd)): embedding gather + the first layer's input RMSNorm (gvl_decode.hip)
int gvl_launch_embed_norm(const bf16_t* table, const TokPtrs& toks, bf16_t* x, bf16_t* xn, const bf16_t* w, int cols, float eps, hipStream_t st);
// xn (B-operand tile order) = rmsnorm(x[b]) * w for the row-major residual rows x [batch][cols]: one wave per sequence (gvl_decode.hip)
int gvl_launch_norm_tiled(bf16_t* x, bf16_t* xn, const bf16_t* w, int batch, int cols, float eps, hipStream_t st);
int gvl_launch_kv_page_copy(bf16_t* kpool, bf16_t* vpool, size_t layer_stride, size_t page_elems, int layers, int src_page, int dst_page, hipStream_t st);
// gvl_seq_fanout (gvl_elem.hip): sibling i's private page, position and generation-count words, by value.  kv_page_fanout copies page src_page of every layer's K and V^T
// to every dst_page[i] in ONE launch (pages distinct, none the source, all < n_pages: checked by the launcher); fanout_rows copies the fp32 row src [n] to
// rows + i * n (a row that IS src is left alone) and sets *pos[i] = pos, *ngen[i] = 0, one launch for all siblings.
struct FanoutArgs { int n; int dst_page[GVL_MAX_DECODE_BATCH]; int* pos[GVL_MAX_DECODE_BATCH]; int* ngen[GVL_MAX_DECODE_BATCH]; };
int gvl_launch_kv_page_fanout(bf16_t* kpool, bf16_t* vpool, size_t layer_stride, size_t page_elems, int layers, int n_pages, int src_page, const FanoutArgs& a, hipStream_t st);
int gvl_launch_fanout_rows(const float* src, float* rows, int n, int pos, const FanoutArgs& a, hipStream_t st);
int gvl_launch_set_int(int* p, int v, hipStream_t st);
int gvl_launch_copy_ints(const int* src, int* dst, int n, hipStream_t st);   // n 4-byte words, device -> device, any alignment (a clone's generated ids)

// ---- frame pre-processing (gvl_pre.hip) -------------------------------------------------------------------------
// frames uint8, layout 0 = [n][H][W][3] / 1 = [n][3][H][W] -> out f32 [n][3][size][size]; *scratch grows on demand (caller-owned).
int gvl_launch_preprocess(const unsigned char* frames, int n, int H, int W, int layout, int size, const float* mean, const float* stdv, float* out,
                          void** scratch, size_t* scratch_bytes, hipStream_t st);

