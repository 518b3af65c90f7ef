// gvl_decode_epi.h -- the projection epilogue of the decode step, ONE copy for its two kernels: gemv_kernel (gvl_elem.hip, one lane per row pair) and
// dgemm_kernel (gvl_decode.hip, lane = sequence x 4 consecutive rows).  What is rounded where (rbf) is fixed HERE, so the two kernels -- and batched against single
// decode -- cannot drift apart.  The vector stores of dgemm_kernel (8 and 16 bytes, out_tiled / out_tiled2, the sq_out shuffle) exist once already and stay there.
//
// The stages read GemvArgs through two VIEWS that the kernel fills, inside the branch that needs them, from its by-value argument.  Handing `const GemvArgs&` itself
// to a stage makes hipcc keep a private copy of the whole kernel argument: every field is then fetched at kernel entry, and in dgemm_kernel the sq_in partial sums in
// front of the main loop turn into a load -> wait -> add chain (first MFMA at instruction 225 instead of 178; + 1.6 % per projection launch inside a Llama-3-8B step).
// With the views the stream up to the last MFMA is the written-out kernel's but for one scalar load (H, KV, Dr, D: now fetched in the RoPE branch) and the place of
// one v_and (profiles/decode_refactor_asm.txt).
#pragma once
#include "gvl_internal.h"

// ---- row order of a qkv projection with the fused RoPE epilogue -------------------------------------------------------------------------------------------
// LOGICAL rows (2 j, 2 j + 1) of the q and k heads are the rotate_half partners (d, d + Dr / 2) of head hd = j / (Dr / 2): one lane owns both halves of a
// rotation.  The v rows (j >= n_qk_heads * Dr / 2) and a projection without RoPE (Dr == 0: no pair at all) keep their order.
struct DecodePair { int hd, d; };
__device__ __forceinline__ DecodePair decode_pair(int j, int halfd) { const int hd = j / halfd; return DecodePair{hd, j - hd * halfd}; }
// logical row -> weight row (the tile copies are built through it: retile_weight_kernel and both quantisers; gemv_kernel reads row-major weights through it)
__device__ __forceinline__ int decode_row_perm(int n, int Dr, int n_qk_heads) {
  const int halfd = Dr >> 1, j = n >> 1;
  if (j < n_qk_heads * halfd) { const DecodePair p = decode_pair(j, halfd); return p.hd * Dr + p.d + (n & 1) * halfd; }
  return n;
}

// ---- fused decode epilogue of the qkv projection: RoPE at the sequence's position (apply_rotary_pos_emb modeling_phi3.py:421-445, short / long factors by
// kv length :382-385), q -> Q[b][H][D], k / v appended to the sequence's pages.  THE code that writes into the paged KV pool at q_len = 1. --------------------
struct DecodeRopeView { const float *cos_s, *sin_s, *cos_l, *sin_l; int rope_switch; bf16_t *Q, *Kt, *Vt; int H, KV, Dr, D, q_stride; };
#define GVL_DECODE_ROPE_VIEW(a) DecodeRopeView{(a).cos_s, (a).sin_s, (a).cos_l, (a).sin_l, (a).rope_switch, (a).Q, (a).Kt, (a).Vt, (a).H, (a).KV, (a).Dr, (a).D, (a).q_stride}
struct DecodeRopeRow { int pos, page, slot; const float* cosp; const float* sinp; bf16_t* Qb; };
// sequence b of the batch: pos_ptr = GemvArgs.pos_ptrs[b], table = GemvArgs.tables[b]
__device__ __forceinline__ DecodeRopeRow decode_rope_row(const DecodeRopeView& g, const int* pos_ptr, const int* table, int b) {
  DecodeRopeRow rr;
  rr.pos = *pos_ptr;
  rr.cosp = g.cos_s; rr.sinp = g.sin_s;
  if (g.rope_switch > 0 && rr.pos + 1 > g.rope_switch) { rr.cosp = g.cos_l; rr.sinp = g.sin_l; }
  rr.page = table[rr.pos >> 6]; rr.slot = rr.pos & 63;
  rr.Qb = g.Q + (size_t)b * g.q_stride;
  return rr;
}
// logical rows (n, n + 1), n even, with the fp32 sums (v0, v1): a q / k pair is rotated and lands in Q or the K page [page][KV][64][D]; a v pair is two
// consecutive d of the V^T page [page][KV][D][64]
__device__ __forceinline__ void decode_rope_pair(const DecodeRopeView& g, const DecodeRopeRow& rr, int n, float v0, float v1) {
  const int halfd = g.Dr >> 1, npair_qk = (g.H + g.KV) * halfd;
  const int j = n >> 1;
  if (j < npair_qk) {
    const DecodePair p = decode_pair(j, halfd);
    const int hd = p.hd, d = p.d;
    const float x1 = rbf(v0), x2 = rbf(v1);
    const float c = rr.cosp[(size_t)rr.pos * halfd + d], sn = rr.sinp[(size_t)rr.pos * halfd + d];
    const bf16_t o1 = f2bf(rbf(x1 * c) + rbf(-x2 * sn)), o2 = f2bf(rbf(x2 * c) + rbf(x1 * sn));
    bf16_t* dst = hd < g.H ? rr.Qb + (size_t)hd * g.D + d
                           : g.Kt + (((size_t)rr.page * g.KV + (hd - g.H)) * 64 + rr.slot) * g.D + d;
    dst[0] = o1; dst[halfd] = o2;
  } else {
    const int vi = n - 2 * npair_qk, hv = vi / g.Dr, d = vi - hv * g.Dr;
    bf16_t* dst = g.Vt + (((size_t)rr.page * g.KV + hv) * g.D + d) * 64 + rr.slot;
    dst[0] = f2bf(v0); dst[64] = f2bf(v1);
  }
}

// interleaved (gate, up) rows: up * silu(gate), each op rounded to bf16 (Phi3MLP modeling_phi3.py:458-464); the caller rounds the product when it stores bf16
__device__ __forceinline__ float decode_swiglu_pair(float gate, float up) {
  const float gt = rbf(gate), u = rbf(up);
  return u * rbf(gt * fast_sigmoid(gt));
}

// one (sequence b, row n) element of the plain epilogue: bias, residual (out = resid + bf16(y)), bf16 and / or f32, rows out_stride apart
struct DecodeOutView { const float* bias; const bf16_t* resid; bf16_t* out_bf16; float* out_f32; int out_stride; };
#define GVL_DECODE_OUT_VIEW(a) DecodeOutView{(a).bias, (a).resid, (a).out_bf16, (a).out_f32, (a).out_stride}
__device__ __forceinline__ void decode_store_scalar(const DecodeOutView& o, int b, int n, float v) {
  if (o.bias) v += o.bias[n];
  if (o.resid) v = bf2f(o.resid[(size_t)b * o.out_stride + n]) + rbf(v);
  if (o.out_bf16) o.out_bf16[(size_t)b * o.out_stride + n] = f2bf(v);
  if (o.out_f32) o.out_f32[(size_t)b * o.out_stride + n] = v;
}
