/*
 * gvl.h -- C ABI of libgvl.so, the MI355X-native Grounded-VideoLLM inference hot path.
 *
 * The reference (WHB139426/Grounded-Video-LLM) is pure Python/PyTorch and has no FFI seam; the
 * boundary this library sits behind is the set of Python calls made inside
 * LLAVA_NEXT_VIDEO.generate() (models/llava_next_video.py:616-666).  Each entry point below names
 * the reference call it replaces (paths relative to the reference root).  INTEGRATION.md shows
 * the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only; no torch types.  All tensor arguments are DEVICE pointers owned by the
 *     caller and valid for the duration of the call, unless the parameter says "host".
 *   - every call enqueues its work on the caller's hipStream_t (passed as void*) and returns
 *     without synchronising, except where noted.
 *   - return value: 0 = ok, < 0 = error (gvl_status); text via gvl_last_error().  Nothing throws.
 *   - bf16 tensors are raw uint16 bit patterns; "f32" is IEEE float.
 *   - one gvl_ctx per GPU / rank; a ctx is not thread-safe (the reference is single-threaded too).
 */
#ifndef GVL_H
#define GVL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gvl_ctx gvl_ctx;

typedef enum {
  GVL_OK = 0,
  GVL_ERR_ARG = -1,      /* bad argument / shape */
  GVL_ERR_STATE = -2,    /* call order (weights missing, sequence not allocated ...) */
  GVL_ERR_HIP = -3,      /* HIP runtime error */
  GVL_ERR_OOM = -4,      /* device memory or KV pages exhausted */
  GVL_ERR_NOGPU = -5     /* no gfx950 device */
} gvl_status;

enum { GVL_F32 = 0, GVL_BF16 = 1, GVL_I32 = 2, GVL_I64 = 3 };
enum { GVL_LLM_PHI3 = 0, GVL_LLM_LLAMA = 1 };

/* Geometry of the three towers.  Mirrors the hard-coded / config.json values of the reference:
 * CLIP  models/llava_next_video.py:56-71;  InternVideo2  models/internvideo2.py:1089-1114;
 * Phi-3 / Llama  models/modeling_phi3.py:132-156, models/modeling_llama.py (HF config [ext]). */
typedef struct {
  int32_t llm_kind;            /* GVL_LLM_PHI3 | GVL_LLM_LLAMA */
  /* CLIP ViT */
  int32_t clip_hidden, clip_inter, clip_layers_run, clip_heads, clip_image, clip_patch;
  /* InternVideo2 */
  int32_t iv2_dim, iv2_inter, iv2_blocks_run, iv2_heads, iv2_image, iv2_patch, iv2_frames_per_seg;
  /* LLM */
  int32_t hidden, inter, layers, heads, kv_heads, vocab;
  float rms_eps;
  int32_t lm_head_bias;        /* 1: logits = W h + b (llava_next_video.py:263) */
  int32_t rope_orig_max_pos;   /* LongRoPE switch point (4096); 0 = plain RoPE (one table) */
  int32_t max_seq;             /* rows of the rope tables / largest context of one sequence */
  /* limits */
  int32_t max_segs;            /* largest number of segments per encode call on this rank */
  int32_t kv_pages;            /* pages (64 tokens each, all layers) in the paged KV pool */
  int32_t max_prefill;         /* largest prefill length (rows of the activation workspace) */
  int32_t decode_fp8;          /* quantised weight variants of the LLM, opt-in, NOT the reference's numerics.  0: bf16.
                                  1: FP8 -- every decoder projection and lm_head is quantised at gvl_finalize_weights to OCP e4m3 with a
                                  per-row power-of-two scale; the decode path streams the FP8 copy (half the bytes).  2: MXFP4 (OCP
                                  Microscaling v1.0: E2M1 elements, one E8M0 scale per 32 consecutive k) -- a quarter of the bytes.
                                  In both the prefill path uses the de-quantised bf16 values: ONE model.  Needs hidden / inter /
                                  heads*head_dim multiples of 512 (FP8) / 1024 (MXFP4). */
} gvl_config;

/* ---- lifecycle ------------------------------------------------------------------------------ */
int gvl_create(const gvl_config* cfg, gvl_ctx** out);
int gvl_destroy(gvl_ctx* ctx);
const char* gvl_last_error(const gvl_ctx* ctx);       /* ctx may be NULL: last create() error */
int gvl_device_info(char* arch_out, int arch_len, int* num_cus);

/* Packed weights.  `name` is one of the packed names produced by
 * grounded_video_llm_amd/weights.py from the reference state-dict keys;
 * replaces nn.Module.load_state_dict (inference.py:156-162).  `data` may be a host or device
 * pointer (is_device); the library converts to its internal dtype and keeps its own copy.
 * Synchronous. */
int gvl_load_weight(gvl_ctx* ctx, const char* name, const void* data, int dtype, const int64_t* shape,
                    int ndim, int is_device);
int gvl_finalize_weights(gvl_ctx* ctx);               /* checks every required tensor is present */
/* All packed tensors from ONE file written by tools/pack_checkpoint.py (`gvl-packed-1`: a safetensors container whose tensor
 * names are the packed names above; LoRA merged, q/k/v fused, K padded, pos-embed interpolated, RoPE tables built offline).
 * The C++ twin of `nn.Module.load_state_dict(torch.load(...))` (inference.py:156-162, models/llava_next_video.py:117-151) for a
 * host that has no Python: the file is mapped read-only and every tensor goes through gvl_load_weight.  Synchronous.  Call
 * gvl_finalize_weights afterwards.  *n_loaded (may be NULL) receives the number of tensors. */
int gvl_load_packed(gvl_ctx* ctx, const char* path, int* n_loaded);

/* ---- vision hot path ------------------------------------------------------------------------ */
/* vision_tower(px, output_hidden_states=True).hidden_states[-2][:, 1:]
 * (llava_next_video.py:504-505).  px f32 [n,3,336,336] -> out f32 [n,576,clip_hidden]. */
int gvl_clip_encode(gvl_ctx* ctx, const float* px, int n_images, float* out, void* stream);

/* video_encoder(x, None, False, x_vis_return_idx=-2, x_vis_only=True)[:, 1:, :]
 * (llava_next_video.py:532).  px f32 [n,3,T,224,224] -> out bf16 [n, T*256, iv2_dim]. */
int gvl_iv2_encode(gvl_ctx* ctx, const float* px, int n_segs, uint16_t* out, void* stream);

/* merge/pool + both projectors + newline + concat (llava_next_video.py:507-564) for n_segs
 * segments.  clip_feats f32 [n,576,clip_hidden], iv2_feats bf16 [n,T*256,iv2_dim]
 * -> visual bf16 [n * gvl_tokens_per_seg(), hidden]. */
int gvl_build_visual(gvl_ctx* ctx, const float* clip_feats, const uint16_t* iv2_feats, int n_segs,
                     uint16_t* visual, void* stream);
int gvl_tokens_per_seg(const gvl_ctx* ctx);           /* 285 (Phi-3.5) / 193 (Llama-3) at 8 f/seg */

/* encode_images() for the caller's segments = the three calls above on the ctx workspace.
 * spatial f32 [n,3,336,336], temporal f32 [n,3,T,224,224] (already "(b s) c f h w"). */
int gvl_encode_segments(gvl_ctx* ctx, const float* spatial_px, const float* temporal_px, int n_segs,
                        uint16_t* visual, void* stream);

/* prepare_multimodal_inputs() for one sample (llava_next_video.py:568-596): ids int64 host
 * [n_ids] with exactly one IMAGE_TOKEN_INDEX (-200); embeds bf16 [n_ids-1+n_visual, hidden]. */
int gvl_splice(gvl_ctx* ctx, const int64_t* ids_host, int n_ids, const uint16_t* visual, int n_visual,
               uint16_t* embeds, int* seq_len_out, void* stream);

/* ---- LLM hot path --------------------------------------------------------------------------- */
/* language_model.generate(inputs_embeds=...) (llava_next_video.py:655-661), greedy:
 *   seq_alloc  -> reserves KV pages for up to max_tokens (DynamicCache replacement, paged)
 *   prefill    -> step 0 of generate(): writes KV, returns last-position logits (f32 [vocab],
 *                 device pointer, may be NULL)
 *   decode_greedy -> steps 1..N on the device; out_ids int32 host [max_new]; stops after eos
 *                 (eos < 0 disables).  Synchronises the stream before returning. */
int gvl_seq_alloc(gvl_ctx* ctx, int max_tokens, int* seq_id);
int gvl_seq_free(gvl_ctx* ctx, int seq_id);
/* Paged KV pool of this ctx (replaces transformers' DynamicCache, models/modeling_phi3.py:1291 [ext]): pages of 64 tokens over all
 * layers.  cfg.kv_pages > 0 fixes the pool size at gvl_create; cfg.kv_pages <= 0 sizes it in gvl_finalize_weights from the HBM
 * that is free once the weights are resident (env GVL_KV_FRACTION, default 0.85 of it, minus 4 GiB) -- on a 288 GB MI355X about
 * 670 k Phi-3.5 tokens.  Any out pointer may be NULL.
 * The fused RMSNorm (gvl_debug_set "norm_fused") keeps norm-folded second copies of qkv / fc1 (InternVideo2) and qkv_proj / gate_up_proj / lm_head (LLM;
 * with bf16 decode weights also their decode tile copies): about 1.1 GB + 10 GB (Phi-3.5) / 18 GB (Llama-3-8B).  env GVL_NORM_FOLD=0 skips them (the norms
 * then run as separate passes); a failed allocation does the same by itself -- finalize does not fail for them. */
/* Prefix sharing (the reference asks three questions about ONE video, inference.py:178-182: the prompts share the system prompt and the
 * 3 420 visual tokens).  gvl_seq_fork makes a new sequence whose first n_tokens (a multiple of 64 = whole KV pages, <= the source's
 * tokens) ARE the source's pages -- referenced, not copied; a page returns to the pool when its last holder is freed -- and reserves
 * fresh pages up to max_tokens.  gvl_prefill_extend then runs the decoder over the remaining n_new prompt rows only: they take
 * positions prefix .. prefix + n_new - 1 and attend to the cached prefix plus themselves; last_logits / first token as gvl_prefill.
 * With a prefix that is a multiple of 128 tokens the result is BIT-IDENTICAL to a gvl_prefill of the whole prompt (same query blocks,
 * same page tiles, same k order); any multiple of 64 is within bf16 rounding of it.  LongRoPE models (cfg.rope_orig_max_pos > 0): a prefill
 * picks ONE factor set from the length it sees (short up to the original context, long beyond; modeling_phi3.py:381-385) -- the prefix's
 * cached K carries the choice made when IT was prefilled, so the identity holds only when prefix and whole prompt fall on the same side of
 * rope_orig_max_pos; the host must not share a prefix <= rope_orig_max_pos with a prompt longer than it (model.py falls back to full
 * prefills). */
int gvl_seq_fork(gvl_ctx* ctx, int src_seq, int n_tokens, int max_tokens, int* dst_seq);
int gvl_prefill_extend(gvl_ctx* ctx, int seq_id, const uint16_t* embeds_new, int n_new, float* last_logits, void* stream);
/* The ragged form of gvl_prefill_extend: n_seqs sequences, each behind its OWN cached prefix, in one decoder pass per group (the weights are streamed once
 * for all tails; RoPE / KV append, V^T pages and causal attention are one launch each per layer for the whole group).  Every sequence must hold a multiple of
 * 64 tokens -- 0 is allowed: such a member is prefilled from scratch -- with pos + n_new[i] <= its max_tokens and 1 <= n_new[i] <= cfg.max_prefill; no sequence
 * twice.  Groups of up to 8 sequences (GVL_MAX_PREFILL_BATCH) and cfg.max_prefill rows are formed in call order, as gvl_prefill_varlen forms them.
 * last_logits: [n_seqs][vocab] on the device, or NULL.  Every member ends in exactly the state its own gvl_prefill_extend (or, when empty, gvl_prefill) leaves it
 * in, bit for bit: logits, first token, KV pages, and, with sampling on, the random stream it would get from n_seqs such calls in call order.
 * GVL_ERR_ARG / GVL_ERR_STATE (gvl_last_error says which member rule) are raised before anything runs: every sequence and the pool stay as they were.
 * gvl_debug_set("varlen_extend", 0) (tests, A/B): one launch per sequence of the single-sequence kernels instead, the GEMMs still shared; same results. */
int gvl_prefill_extend_varlen(gvl_ctx* ctx, const int* seq_ids, int n_seqs, const uint16_t* const* embeds_new, const int* n_new,
                              float* last_logits /* [n_seqs][vocab] device, may be NULL */, void* stream);
/* gvl_prefill_extend_varlen that also SCORES given ids on the way (teacher forcing): how likely the model finds a given continuation, without sampling.  Member rules,
 * group formation, the refusals before anything runs and the final state of every member (logits, first token, KV pages, random stream) are gvl_prefill_extend_varlen's; a
 * member holding 0 tokens is scored from scratch.
 * next_ids_host[i][r], r < n_new[i] (host arrays, read before the call returns): the id that new row r of member i must PREDICT -- the next-token convention: row r's target
 * is the token fed at r + 1 (the last row's is whatever follows the rows of this call, if the caller knows it) -- or -100 = row r is not scored.  HF's label convention
 * (labels aligned with the rows and shifted inside) cannot be used: behind a cached prefix the hidden state in front of the first new row is not there to predict it.
 * Per scored row, from the fp32 logits of the row (final norm, lm_head + bias; the raw distribution: no processors, rules or warpers):
 *   lp_dev    log-softmax at the target.  Bit for bit what greedy selection's log-probability reports for such a row when the target is its argmax.
 *   rank_dev  how many entries beat the target in the order (value descending, lower id first); 0 = the target is the greedy choice.
 *   top_n 1 .. 8: top_ids_dev / top_lp_dev [.][8], the best top_n finite entries, padded with (-1, -inf) -- gvl_set_logprobs' lists; top_n = 0: both may be NULL, untouched.
 * The outputs are PACKED device arrays: members in call order, each member's scored rows in row order; *n_scored (may be NULL) = their count, which the caller can also
 * count from next_ids_host and must size the arrays for.  A scored row's values do not depend on the group or the call it travels in.  Its logits come from a GEMM over
 * the scored rows (one stream of the head's weights per 64 rows), so they differ from gvl_prefill's last_logits of the prompt truncated at that row by rounding (a
 * separate bf16 norm pass against the fused one), not bitwise.  Every row of the group runs the last layer's MLP (the default prefill runs it on last rows only).
 * GVL_ERR_ARG also for a target other than -100 outside [0, vocab) and for top_n outside 0 .. 8 -- raised, like every refusal, with every sequence and the pool untouched.
 * All work is enqueued on `stream`; nothing is synchronised. */
int gvl_score_extend_varlen(gvl_ctx* ctx, const int* seq_ids, int n_seqs, const uint16_t* const* embeds_new, const int* n_new, const int32_t* const* next_ids_host,
                            int top_n, float* lp_dev, int32_t* rank_dev, int32_t* top_ids_dev, float* top_lp_dev, int* n_scored,
                            float* last_logits /* [n_seqs][vocab] device, may be NULL */, void* stream);
/* A copy of a sequence AT ITS CURRENT LENGTH (beam search: HF's cache reorder, transformers GenerationMixin._reorder_cache [ext]): whole pages
 * are shared by reference, the partial last page is copied on `stream` (one launch over all layers); the clone then appends to its own pages.
 * Its list of generated ids starts empty -- unless the source has a grammar (gvl_seq_set_grammar): then the clone takes the source's generated ids along, see there. */
int gvl_seq_clone(gvl_ctx* ctx, int src_seq, int max_tokens, int* dst_seq, void* stream);
/* n answers to ONE prompt from one prefill (HF generate(num_return_sequences = n) expands the prompt n times and pays n prefills): n_new SIBLINGS of the freshly prefilled
 * sequence src_seq -- it holds exactly the one token its own prefill selected, as gvl_seq_set_guidance requires -- each with capacity max_tokens; first_logits (device, fp32
 * [vocab]) is the last_logits of that prefill; 1 <= n_new <= 15 (GVL_MAX_DECODE_BATCH - 1); the call may be repeated while the source is still fresh.
 *   copy      a sibling is a gvl_seq_clone of the source at its current length: whole pages shared by reference, the partial last page private.  The siblings' partial pages
 *             are copied in ONE launch for all siblings (all layers, K and V^T); a prompt that ends on a page boundary copies nothing.
 *   settings  the source's processors, rule set, grammar and log-probability setting, and the source's EFFECTIVE sampling -- its own (gvl_seq_set_sampling), else the ctx
 *             setting at the time of the call -- as a setting of the sibling's own with stream = streams[i] (host array [n_new]).
 *   token     sibling i's first token is selected from first_logits with its own draw (seed, streams[i], step 0), one selection launch for all siblings.  A prefill's
 *             last_logits is the row its own selection saw, i.e. the PROCESSED row, and at step 0 every sibling's processed row is that same row (empty history, the same
 *             min-length ban, begin-suppress and grammar start): the call applies warpers and draw only, never processors, rules or grammar a second time.
 * Afterwards every sibling stands where its own prefill would have left it (n_gen 1; output slot 0, the token word, log-probability slot 0 and the top list from its own
 * selection) and the source is untouched (token, lists, pages, random stream).  Sibling i's ids and log-probabilities are bit for bit those of an independent sequence
 * prefilled with the same prompt and settings under gvl_seq_set_sampling(stream = streams[i]), whatever decode group it travels in.  dst_seqs [n_new] receives the ids; free
 * source and siblings in any order.  All work is enqueued on `stream`; nothing is synchronised.
 * All or nothing: GVL_ERR_ARG (NULL arguments, unknown source, n_new / max_tokens out of range), GVL_ERR_STATE (source not fresh, or a member of a guided pair) and
 * GVL_ERR_OOM (KV pages or sequence slots for fewer than n_new siblings) are raised before anything runs, with every sequence and the pool as they were. */
int gvl_seq_fanout(gvl_ctx* ctx, int src_seq, int n_new, int max_tokens, const uint32_t* streams /* [n_new] host */, float* first_logits /* device, fp32 [vocab] */,
                   int* dst_seqs /* [n_new] */, void* stream);
int gvl_kv_info(const gvl_ctx* ctx, int* total_pages, int* free_pages, int64_t* pool_bytes, int* max_live_seqs);
/* Tests: the KV pages of a live sequence in position order (page i holds tokens 64 i .. 64 i + 63; the element offset of page p inside a layer's K or V^T slice is
 * p * kv_heads * 64 * head_dim).  Host-only: reads the sequence table, touches no device memory and enqueues nothing.  *n_pages (may be NULL) = how many pages the
 * sequence holds; the first min(cap, *n_pages) of them are written to pages_host (may be NULL when cap is 0).  GVL_ERR_ARG: no ctx, unknown sequence, cap < 0. */
int gvl_debug_seq_pages(const gvl_ctx* ctx, int seq_id, int32_t* pages_host, int cap, int* n_pages);
/* The group sizes ONE batched decode step takes (gvl_decode_step_logits_batch, and the parts gvl_decode_greedy_batch / gvl_decode_steps
 * step together), valid after gvl_finalize_weights: *max_group = 16 on the skinny-MFMA decode path, 4 on the VALU fallback
 * (geometries whose projection widths are not multiples of 256); *any_size = 1 when every size 1 .. max_group is taken, 0 when only
 * 1, 2 and 4 are.  Hosts that form their own groups (beam search) ask here instead of restating the library's predicate. */
int gvl_decode_group_info(const gvl_ctx* ctx, int* max_group, int* any_size);
int gvl_prefill(gvl_ctx* ctx, int seq_id, const uint16_t* embeds, int seq_len, float* last_logits,
                void* stream);
int gvl_decode_greedy(gvl_ctx* ctx, int seq_id, int max_new, int eos_id, int32_t* out_ids_host,
                      int* n_out, void* stream);
/* Token selection of every later gvl_prefill* / gvl_decode_* call on this ctx, for every sequence without a sampling setting of its own (gvl_seq_set_sampling below).  The reference forwards do_sample / temperature /
 * top_p from generate(**kw) to HF generate (models/llava_next_video.py:655-661; inference.py:45-49 defaults: do_sample True,
 * temperature 0.2, top_p None; HF's GenerationConfig adds top_k 50 [ext]).  do_sample = 0: greedy argmax (the default of a new ctx).
 * do_sample = 1: scores / temperature -> top-k (0 = off; ties with the k-th score are kept) -> top-p (0 or 1 = off; a token is kept
 * iff the probability mass of strictly larger scores is < top_p) -> ONE draw from the softmax of what is left, all on the device
 * inside the decode step.  The draw of a sequence is a pure function of (seed, the order in which sequences were prefilled since
 * this call, generation step, logits): reproducible, and independent of how sequences are grouped into decode batches.  (A call
 * that repeats the current seed while sequences are live continues the numbering instead, so newcomers never share a stream with
 * a running sequence; callers that make several generate() calls per request pass a different seed per call.)
 * torch.multinomial's random stream is not reproduced (parity = same kept set + same distribution).  Beam search (num_beams > 1, do_sample = 0) is
 * gvl_beam_search below: bookkeeping on the host (csrc/gvl_beam.h), every step's log-softmax and top 2 x num_beams candidates in the library's kernels; beam-sample
 * (num_beams > 1, do_sample = 1) stays host bookkeeping over gvl_seq_clone + gvl_decode_step_logits_batch with the candidates of a step DRAWN on the host from the warped
 * beam distributions (grounded_video_llm_amd/beam.py: its draws are torch's). */
int gvl_set_sampling(gvl_ctx* ctx, int do_sample, float temperature, int top_k, float top_p, uint64_t seed);
/* Sampling as one value, with HF's remaining warpers.  A sampled selection runs, in HF's order (transformers _get_logits_processor [ext]), each stage's softmax taken over
 * what the stage before left, min_tokens_to_keep = 1:
 *   scores / temperature -> top_k -> top_p                  as gvl_set_sampling (same arithmetic: with the four fields below off, the same tokens bit for bit)
 *   min_p            MinPLogitsWarper: remove p_i < min_p * p_max
 *   typical_p        TypicalLogitsWarper: with H the entropy and d_i = |-log p_i - H|, keep the smallest d first until their mass reaches typical_p; ties at the cut stay
 *   epsilon_cutoff   EpsilonLogitsWarper: remove p_i < epsilon_cutoff, the largest kept score always stays
 *   eta_cutoff       EtaLogitsWarper: remove p_i < min(eta, sqrt(eta) * exp(-H)), the largest kept score always stays
 * then one draw from the softmax of what is left.  The kept set is an interval of scores after every stage (typical_p alone may drop the maximum).
 * gvl_set_sampling_ex sets the ctx setting (its `stream` field is ignored: followers keep gvl_set_sampling's numbering in prefill order); with the four new fields 0 it is
 * gvl_set_sampling.  gvl_seq_set_sampling gives ONE live sequence its own setting: from then on it is greedy or sampled by that value whatever the ctx setting is and whatever
 * its neighbours in a decode group use, and a sampled draw is a pure function of (seed, stream, generation step, logits) -- not of what else was prefilled or decoded, nor of
 * the group it travels in.  NULL: back to following the ctx setting at every selection (what a new sequence does).  gvl_seq_fork / gvl_seq_clone copy the source's own setting,
 * stream included: a caller that wants distinct draws sets a different `stream` afterwards.
 * Settings are HOST values read when a step is enqueued (or captured: step graphs are built per call, nothing is baked in across calls): a setter takes effect from the next
 * gvl_prefill* / gvl_decode_* call and must not race one in flight on another thread.
 * Errors (GVL_ERR_ARG with a message; nothing is clamped; NaN fails): temperature not > 0, top_k < 0, top_p or min_p outside [0, 1], typical_p / epsilon_cutoff / eta_cutoff
 * outside [0, 1), unknown sequence.  With do_sample = 0 every other field is ignored. */
typedef struct {
  int32_t do_sample;          /* 0: greedy (every other field ignored) */
  float temperature;          /* > 0 */
  int32_t top_k;              /* 0 = off */
  float top_p;                /* 0 or 1 = off */
  float min_p;                /* 0 = off; in [0, 1] */
  float typical_p;            /* 0 = off; the mass to keep, in (0, 1) */
  float epsilon_cutoff;       /* 0 = off; in (0, 1) */
  float eta_cutoff;           /* 0 = off; in (0, 1) */
  uint64_t seed; uint32_t stream;
} gvl_sampling;
int gvl_set_sampling_ex(gvl_ctx* ctx, const gvl_sampling* sampling);
int gvl_seq_set_sampling(gvl_ctx* ctx, int seq_id, const gvl_sampling* sampling);
/* HF generate()'s logits processors, applied on the device to a sequence's fp32 logits row at every token selection (prefill's first
 * token, gvl_decode_greedy*, gvl_decode_steps; greedy and sampling alike), before the warpers / argmax, in HF's order:
 *   penalty != 1   RepetitionPenaltyLogitsProcessor: every DISTINCT generated id t: s[t] = s[t] < 0 ? s[t] * penalty : s[t] / penalty
 *   ngram > 0      NoRepeatNGramLogitsProcessor: an id that would complete an n-gram already generated gets -inf
 *   min_new > 0    MinLength / MinNewTokensLength: s[eos_id] = -inf while fewer than min_new ids were generated (off when eos_id < 0)
 * The history is the sequence's GENERATED ids only (up to 8192): the reference calls generate(inputs_embeds=...) without input_ids, so
 * HF never sees the prompt's ids.  penalty 1, ngram 0, min_new 0 = off (the default): the token selection is then exactly the one without
 * processors.  gvl_set_logits_processors sets the default every sequence allocated AFTER the call starts with (gvl_seq_alloc);
 * gvl_seq_set_processors overrides one live sequence; gvl_seq_fork / gvl_seq_clone copy the source's settings (a clone's history starts
 * empty: its generation count restarts at 0).  Errors: penalty not > 0 (NaN included), ngram < 0, min_new < 0. */
int gvl_set_logits_processors(gvl_ctx* ctx, float penalty, int ngram, int min_new, int eos_id);
int gvl_seq_set_processors(gvl_ctx* ctx, int seq_id, float penalty, int ngram, int min_new, int eos_id);
/* Token rules: HF's other token-level processors (SequenceBias, NoBadWords, ForcedEOSToken, SuppressTokens, SuppressTokensAtBegin), applied by the
 * same launch as the processors above, in HF's order:
 *   sequence_bias -> repetition penalty -> no-repeat n-gram -> bad_words_ids -> min length -> forced eos -> suppress -> begin suppress
 * A rule set is an immutable device-resident object made from host arrays (copied; gvl_rules_create synchronises).  A bias table is grouped
 * BY TARGET TOKEN (the last id of an entry): targets [n_targets][3] = (target id, first entry, number of entries), the targets distinct;
 * entry e has bias entry_bias[e] and the prefix ids prefix[entry_prefix[2e] .. + entry_prefix[2e + 1]) (the entry's ids without its last;
 * length 0 = a single-token entry, which comes first in its group; the multi-token entries follow in the caller's dict order).  For each
 * target the applicable entries' biases are summed in fp32 from 0.0f in that order and the sum is added to the score once; a multi-token entry
 * applies when its prefix equals the last ids of the history and its length does not exceed the history's (HF's rule).  bias[0] runs before
 * the penalty (sequence_bias), bias[1] after the n-gram bans (bad_words_ids: bias -inf).  force_ids (n_force > 0): when the history holds
 * exactly force_at ids every score becomes -inf and the forced ids' scores 0.  suppress: -inf at every step; begin_suppress: -inf when the
 * history holds exactly begin_index ids.  Ids outside the row are ignored.  Limits (GVL_ERR_ARG with a message beyond them, never truncated):
 * 262144 ids per single-token list and single-token entries per table, 1024 multi-token entries per table, 16 ids per entry, 1024 live sets.
 * gvl_set_token_rules sets the default (a rule-set id, or -1 = none) of every sequence allocated AFTER the call; gvl_seq_set_token_rules one
 * live sequence; gvl_seq_fork / gvl_seq_clone copy the source's, gvl_seq_free drops it.  gvl_rules_destroy of a set that a live sequence or
 * the default still references is GVL_ERR_STATE; it synchronises the device before the memory is released.  gvl_destroy frees every set. */
typedef struct {
  int32_t n_targets; const int32_t* targets;
  int32_t n_entries; const float* entry_bias; const int32_t* entry_prefix;
  int32_t n_prefix; const int32_t* prefix;
} gvl_bias_table;
typedef struct {
  int32_t n_suppress; const int32_t* suppress;
  int32_t n_begin_suppress; const int32_t* begin_suppress; int32_t begin_index;
  int32_t n_force; const int32_t* force_ids; int32_t force_at;
  gvl_bias_table bias[2];
} gvl_rules_desc;
int gvl_rules_create(gvl_ctx* ctx, const gvl_rules_desc* desc, int* rules_id);
int gvl_rules_destroy(gvl_ctx* ctx, int rules_id);
int gvl_set_token_rules(gvl_ctx* ctx, int rules_id);
int gvl_seq_set_token_rules(gvl_ctx* ctx, int seq_id, int rules_id);
/* Decoding grammars: HF's PrefixConstrainedLogitsProcessor (prefix_allowed_tokens_fn) as a device-resident object -- a DFA over token classes with
 * one integer register, applied by the same launch as the processors and rules above, in HF's place: ... -> min length -> GRAMMAR -> forced eos ->
 * suppress -> begin suppress.  No state is kept per sequence: every launch recomputes the mask from the grammar and the sequence's generated ids.
 * Walk: start from state = start, reg = 0 and feed the generated ids in order.  The walk turns OFF for good on any of: an id outside [0, vocab), a
 * forbidden transition, a GE transition with ordinal < reg, a history longer than 8192 ids.  A state whose whole row is forbidden is an END state.
 * Mask: in an OFF or END state the logits row is left untouched, bit for bit (tokens after eos inside a multi-step chunk, which the caller discards).
 * Otherwise, for every id t: allowed gives s[t] = s[t] + 0.0f, forbidden gives s[t] = -inf -- HF's `scores + mask`, which turns -0.0 into +0.0.  +inf
 * and NaN logits are outside the contract.  On an edge with both flags GE reads the register before SET overwrites it.
 * gvl_grammar_create checks (GVL_ERR_ARG with a message, nothing is clamped): the limits below; every token's class < n_classes; an ordinal class is
 * exactly a contiguous id range; SET and GE only on ordinal classes; reserved bits clear; next states in range; every non-END state keeps a token
 * allowed whatever reg holds (an edge without GE on a non-empty class, or a GE edge on a class at least as large as every class that has a SET edge).
 * At most 64 live grammars.  The arrays are copied; gvl_grammar_create synchronises.  A grammar bound to sequences (gvl_set_grammar: the default of
 * sequences allocated AFTER the call, -1 none; gvl_seq_set_grammar: one live sequence) must have vocab == cfg.vocab (GVL_ERR_ARG otherwise);
 * gvl_op_logits_process_ex takes any grammar whose vocab equals its row width.  gvl_seq_fork / gvl_seq_clone copy the source's grammar, gvl_seq_free
 * drops it.  Copies taken MID-ANSWER: the mask depends on the generated ids, so a copy must know the ones its tokens contain.
 *   gvl_seq_clone of a source WITH a grammar also copies the source's generated ids, their count, the id to feed next and (where on) their log-probability lists:
 *     the clone stands exactly where the source stands, gvl_decode_steps continues it at once, and gvl_seq_read returns the source's ids followed by the clone's
 *     own -- the answer so far plus a continuation in the language.  (Without a grammar a clone's list starts empty and the caller feeds its next id, as before.)
 *   gvl_seq_fork shares prompt pages: a fork at or before the source's first generated position holds none of its ids, starts its walk at (start, 0) behind its
 *     own gvl_prefill_extend and gives a whole answer.  A fork whose n_tokens would reach past that position is GVL_ERR_STATE while the source has a grammar: the
 *     rows appended behind a fork are embeddings whose ids the library is not told, so the walk could not go on (fork within the prompt, clone, or take the
 *     grammar off the source first).
 * gvl_grammar_destroy of a grammar that a live sequence or the default references is GVL_ERR_STATE, and it synchronises the device before
 * the memory is released.  gvl_destroy frees every grammar.  gvl_beam_search applies the grammar that its seq_id carries to every beam. */
typedef struct {
  int32_t n_states, n_classes, start, vocab;   /* 1..256, 1..64, n_states*n_classes <= 4096, vocab 1 .. 2^23 */
  const uint8_t*  token_class;  /* [vocab]: the class of every id */
  const int32_t*  class_base;   /* [n_classes]: -1 plain; >= 0: ORDINAL class = exactly the ids base .. base+size-1, ordinal(t) = t - base */
  const uint16_t* trans;        /* [n_states][n_classes]: 0xFFFF forbidden; else bits 0-7 next state, bit 8 SET (reg = ordinal), bit 9 GE (allowed iff ordinal >= reg) */
} gvl_grammar_desc;
int gvl_grammar_create(gvl_ctx* ctx, const gvl_grammar_desc* desc, int* grammar_id);
int gvl_grammar_destroy(gvl_ctx* ctx, int grammar_id);
int gvl_set_grammar(gvl_ctx* ctx, int grammar_id);
int gvl_seq_set_grammar(gvl_ctx* ctx, int seq_id, int grammar_id);
/* Classifier-free guidance against a negative sequence: HF generate(guidance_scale=s, negative_prompt_ids=...), i.e. transformers'
 * UnbatchedClassifierFreeGuidanceLogitsProcessor.  Per step, with c = log_softmax(conditional logits) and u = log_softmax(negative logits),
 *     row = s * (c - u) + u                       (fp32; one subtract, one multiply, one add, each rounded; the log-softmax is the fixed-order
 *                                                  one the log-probabilities and beam search use: (l - max) - log(sum exp(l - max)))
 * replaces the conditional row BEFORE everything else the library applies -- processors, token rules, grammar, warpers, selection, log-probabilities
 * (which are then the guided distribution's) -- HF's order, where it is the first processor.  The negative sequence is fed the token the conditional
 * one selected, every step; the first token is guided too.  Raw logits are FINITE by contract (lm_head rows are; a row holding -inf or NaN gives
 * unspecified values, never an out-of-bounds access).
 * gvl_seq_set_guidance binds the freshly prefilled conditional sequence seq_id (the LEADER) to the freshly prefilled negative one neg_seq_id (the
 * FOLLOWER).  Preconditions: both live and distinct, each holding exactly the one token its own prefill selected, neither part of a pair, scale finite,
 * the follower's remaining capacity (max_tokens - tokens held) >= the leader's; cond_logits / neg_logits are the two prefills' last_logits (device,
 * fp32 [vocab], two different buffers) and are scratch for the call.  They must be the RAW rows: a prefill's last_logits are the row its own selection saw, so
 * give the leader its processors, rules and grammar between its prefill and this call (settings that change no row -- sampling, log-probabilities -- may come first).  Otherwise GVL_ERR_ARG / GVL_ERR_STATE with a message, before anything runs.
 * The call re-selects the FIRST token from the guided row with the leader's processors, rules, grammar, sampling and log-probability settings and
 * writes it to both sequences; afterwards both stand exactly where a prefill that had selected from the guided row would have left them: n_gen 1,
 * slot 0 = the guided token, the leader's log-probability slot 0 the guided distribution's, a sampled draw the one of (seed, stream, step 0).
 * From then on the caller names ONLY the leader in gvl_decode_greedy / gvl_decode_greedy_batch / gvl_decode_steps: the follower rides as one more
 * row of the same decode step (the weights stream once for both; a pair is never split across steps: up to 8 pairs, or any mix that fits 16 rows,
 * share a step; on the VALU fallback a pair and a plain sequence run as 2 + 1).  One launch computes the guided rows in front of the processors
 * and one after the selection hands the followers their tokens; a step without pairs takes exactly the launches it took before.  A pair leaves a
 * decode together, when the leader hits eos / max_new / its capacity; the follower's own eos is never looked at and its ids (gvl_seq_read) are the
 * leader's.  A leader's ids do not depend on the sequences it is decoded with.
 * GVL_ERR_STATE, with nothing changed: a bound follower named in any decode, prefill-extend or score call, or freed; either member named in
 * gvl_seq_fork, gvl_seq_clone, gvl_beam_search or gvl_decode_step_logits*.  neg_seq_id = -1 unbinds (the logits pointers and the scale are ignored),
 * and so does gvl_seq_free of the leader; the follower lives on as a plain sequence and the caller frees it. */
int gvl_seq_set_guidance(gvl_ctx* ctx, int seq_id, int neg_seq_id, float scale, float* cond_logits, float* neg_logits, void* stream);
/* Log-probabilities of the selected tokens, computed on the device by the token-selection kernel itself (prefill's first token,
 * gvl_decode_greedy*, gvl_decode_steps; greedy and sampling alike; graph-replayed steps included).  The distribution is the one the token
 * was selected from: greedy, log_softmax of the row after the logits processors, (s_tok - m) - log(sum_i exp(s_i - m)); sampling, the
 * warped distribution HF samples from (temperature -> top-k -> top-p, everything outside the final kept set at -inf),
 * (s_tok - m) / T - log(sum_kept exp((s_i - m) / T)).  fp32, fixed-order reductions: a row's values do not depend on its decode group
 * or path.  top_n: -1 = off (the default; the selection launch is then exactly the one without log-probabilities), 0 = the selected
 * token's only, 1 .. 8 = also the top_n best finite (kept) entries of the same distribution, by value descending,
 * lower id first on ties, padded with (-1, -inf) when fewer exist.  The selected token is the same whatever top_n is.
 * gvl_set_logprobs sets the default of sequences allocated AFTER the call; gvl_seq_set_logprobs one live sequence (fork / clone copy
 * it).  The first setting that needs them allocates the per-slot device lists (top lists: ~134 MB).  Errors: top_n outside -1 .. 8.
 * gvl_seq_read_logprobs follows gvl_seq_read: entries first .. min(n_gen, first + cap) - 1 to host arrays lp [cap] and top_ids /
 * top_lp [cap][8] (slots >= the sequence's top_n hold (-1, -inf)); any of the three may be null; synchronises
 * `stream`.  Asking for lp of a sequence with top_n -1, or for top lists with top_n < 1, is GVL_ERR_STATE. */
int gvl_set_logprobs(gvl_ctx* ctx, int top_n);
int gvl_seq_set_logprobs(gvl_ctx* ctx, int seq_id, int top_n);
int gvl_seq_read_logprobs(gvl_ctx* ctx, int seq_id, int first, int cap, float* lp_host, int32_t* top_ids_host, float* top_lp_host, int* n_gen,
                          void* stream);
/* Prefill of n_seqs sequences together, seq_lens[i] tokens each (ragged: prompts differ in length; the reference left-pads and
 * masks, llava_next_video.py:622-647 -- here the rows are packed back to back, no padding).  Groups of 4 / 2 / 1 sequences whose
 * rows fit cfg.max_prefill: the decoder GEMMs run over all rows of a group at once (better tile fill); RoPE / KV append / causal
 * attention stay per sequence on its own pages (one launch with a batch dimension when the lengths agree, one per sequence
 * otherwise).  Per sequence bit-identical to gvl_prefill.  embeds: host array of n_seqs device pointers (bf16 [len, hidden]). */
int gvl_prefill_varlen(gvl_ctx* ctx, const int* seq_ids, int n_seqs, const uint16_t* const* embeds,
                       const int* seq_lens, void* stream);
/* gvl_prefill_varlen with every length == seq_len. */
int gvl_prefill_batch(gvl_ctx* ctx, const int* seq_ids, int n_seqs, const uint16_t* const* embeds, int seq_len,
                      void* stream);
/* Batched greedy decode of n_seqs freshly prefilled sequences (the reference batches clips in generate() with
 * left padding, llava_next_video.py:622-647 -- here every sequence keeps its own pages and length, no padding).  Groups of
 * up to 16 sequences advance together (skinny MFMA GEMM, gvl_decode.hip; 4 / 2 / 1 on the VALU fallback for K % 256 != 0
 * geometries): every weight matrix is streamed ONCE per step for the whole group, so the HBM cost per
 * sequence falls as 1/group; the per-sequence arithmetic (and therefore the ids) is bit-identical to gvl_decode_greedy.
 * out_ids_host int32 [n_seqs][max_new]; n_out [n_seqs].  A group runs until all of its members hit eos / max_new. */
int gvl_decode_greedy_batch(gvl_ctx* ctx, const int* seq_ids, int n_seqs, int max_new, int eos_id,
                            int32_t* out_ids_host, int* n_out, void* stream);
/* Continuous batching: the two calls a scheduler needs besides prefill / seq_alloc / seq_free.
 * gvl_decode_steps advances every listed sequence by n_steps greedy tokens -- the sequences may be at DIFFERENT generation
 * steps (joined at different times); groups of up to 16 share one weight stream per step; asynchronous on `stream`, no eos
 * test (the host inspects the ids between chunks; tokens after an eos are discarded by the caller).
 * gvl_seq_read copies the ids generated so far, from index `first`, to the host (at most cap), reports the total count in
 * *n_gen and synchronises `stream`.  Free a sequence only after a gvl_seq_read / stream synchronise that follows its last step. */
int gvl_decode_steps(gvl_ctx* ctx, const int* seq_ids, int n_seqs, int n_steps, void* stream);
int gvl_seq_read(gvl_ctx* ctx, int seq_id, int first, int32_t* out_ids_host, int cap, int* n_gen, void* stream);
/* teacher-forced single step (parity tests): appends token `tok`, returns logits f32 [vocab]. */
int gvl_decode_step_logits(gvl_ctx* ctx, int seq_id, int tok, float* logits, void* stream);
/* The same for up to 16 sequences in ONE step (one stream of the weights): sequence i takes toks[i]; logits (may be null) receives
 * [n_seqs][vocab] fp32.  Row i is bit-identical to gvl_decode_step_logits on sequence i alone.  Beam search advances its k beams with it. */
int gvl_decode_step_logits_batch(gvl_ctx* ctx, const int* seq_ids, int n_seqs, const int32_t* toks, float* logits, void* stream);

/* Beam search: HF generate(num_beams = k, do_sample = False) (inference.py:46,170-176 -> models/llava_next_video.py:655-661 -> transformers 4.40.1
 * GenerationMixin._beam_search + BeamSearchScorer [ext]; batch of one, one beam group) inside the library.  seq_id is a PREFILLED sequence and first_logits (device,
 * f32 [vocab]) the last_logits its gvl_prefill* returned.  The sequence is NOT consumed: the k running beams are gvl_seq_clone's of it (capacity min(tokens +
 * max_new_tokens + 1, cfg.max_seq); whole KV pages shared by reference, HF's per-step cache reorder = clone / free), their selection options are switched off so every
 * step yields raw logits, and every sequence the call made is freed on every return path -- on return seq_id is where it was (the KV pool too) and can be decoded or
 * searched again.  Per step: the k beams advance by ONE teacher-forced decode step (one stream of the weights; on the VALU-fallback geometries in parts of 4 / 2 / 1
 * sequences -- a row does not depend on its part), then two launches give the best 2k of the k x vocab grid:
 *     lp = (l - max) - logf(sum exp(l - max))      fp32, the fixed-order sum of gvl_set_logprobs: bit for bit the log-probability greedy selection reports for the token
 *     t  = lp + beam_score                         ONE fp32 add; the beam scores start as [0, -1e9, ...] (the first step expands the prompt's row only)
 *     order: t descending, then flat index beam * vocab + token ascending -- a strict total order over ALL entries, -inf included (torch.topk leaves ties unspecified)
 * With processors (penalty / ngram / min_new / proc_eos_id: gvl_set_logits_processors' meaning, history = the beam's generated ids) or a rule set (gvl_rules_create), HF's
 * order holds: log-softmax -> sequence_bias -> processors -> ... -> + beam score -> top 2k.  A grammar that seq_id carries (gvl_seq_set_grammar) is applied to every
 * beam's row in the same launch, on the beam's own generated ids.  The candidates land in host-mapped memory; after one stream synchronise per
 * step the host bookkeeping (csrc/gvl_beam.h, all score arithmetic in double: sum / pow((double)generated_len, length_penalty)) consumes them: an eos candidate of rank < k
 * closes a hypothesis (generated_len counts the eos), of rank >= k is skipped; done = k hypotheses and (early_stopping 1, or the worst of them >= max candidate /
 * cur_len ** length_penalty); at max_new_tokens the open beams become hypotheses; among equal best scores the last added wins.  Output: the NEW ids of the best hypothesis
 * (eos appended when it ended by eos and there is room) in out_ids_host [cap >= max_new_tokens], their number in *n_out, the hypothesis score in *sequences_score (may be
 * NULL) and per id the processed log-probability it had in its beam's row, before the beam score (HF compute_transition_scores(normalize_logits = False)), in
 * transition_scores_host [cap] (may be NULL).  Synchronises `stream`.
 * Errors (a message via gvl_last_error; nothing is leaked): num_beams outside 2 .. 16, vocab < 2 x num_beams, max_new_tokens < 1 or > 8192, cap < max_new_tokens, an
 * unknown rule set, bad processor values, an unknown or not prefilled sequence (GVL_ERR_STATE), early_stopping 2 ("never") with length_penalty > 0 (it needs a maximum
 * length the reference never passes), KV pages exhausted (GVL_ERR_OOM), fewer than num_beams non-eos candidates among a step's 2 x num_beams (GVL_ERR_STATE).
 * NaN logits are outside the contract: the candidate order is then that of the order-preserving integer keys, not IEEE's (no store goes out of bounds).
 * gvl_beam_search_n returns the num_return (1 .. num_beams) BEST hypotheses (HF num_return_sequences with beams; BeamSearchScorer.finalize with num_beam_hyps_to_keep =
 * num_return): popped from sorted(hypotheses, key = score) best first, among equal scores the later added first.  out_ids_host [num_return][cap], n_out [num_return],
 * sequences_scores [num_return] (non-increasing; may be NULL), transition_scores_host [num_return][cap] (may be NULL).  Everything else -- the search, the errors -- is
 * gvl_beam_search's, which is the num_return = 1 call.  GVL_ERR_ARG for num_return outside 1 .. num_beams.
 * Diverse (group) beams are gvl_group_beam_search below; constrained beams are not supported. */
typedef struct gvl_beam_params {
  int num_beams;            /* 2 .. 16 (GVL_MAX_DECODE_BATCH) */
  int max_new_tokens;       /* >= 1 */
  int eos_id;               /* -1: none */
  double length_penalty;
  int early_stopping;       /* 0 False, 1 True, 2 "never" */
  float penalty; int ngram; int min_new; int proc_eos_id;  /* gvl_set_logits_processors' meaning; 1.0 / 0 / 0 / -1 = off */
  int rules_id;             /* -1: none */
} gvl_beam_params;
int gvl_beam_search(gvl_ctx* ctx, int seq_id, const float* first_logits, const gvl_beam_params* params, int32_t* out_ids_host, int cap, int* n_out,
                    double* sequences_score, float* transition_scores_host, void* stream);
int gvl_beam_search_n(gvl_ctx* ctx, int seq_id, const float* first_logits, const gvl_beam_params* params, int num_return, int32_t* out_ids_host, int cap, int* n_out,
                      double* sequences_scores, float* transition_scores_host, void* stream);
/* Diverse (group) beam search: HF generate(num_beams = k, num_beam_groups = G, diversity_penalty = lambda) (transformers 4.40.1 GenerationMixin._group_beam_search +
 * BeamSearchScorer(num_beam_groups) + HammingDiversityLogitsProcessor [ext]; batch of one).  G groups of s = k / G beams; group g owns the beams g*s .. g*s + s - 1 and
 * is gvl_beam_search's step with k := s (its own hypotheses, its own done flag, its own 2s candidates), beam scores -1e9 except the first beam of every group.  Per step
 * all live beams advance by one decode step, every row is normalised once, and then per group, in order, ONE chain on the stream: the processor launch (for g > 0 with
 * the Hamming stage in HF's place, behind sequence_bias and in front of the repetition penalty: s[t] -= fp32(lambda * count of t among the tokens the earlier groups chose
 * at this step), the product rounded first) -> the group's row candidates -> its merge, which also writes the group's choice -- the tokens of its first s non-eos
 * candidates -- to device memory for the next group's Hamming stage.  One stream synchronise per step; the host bookkeeping (csrc/gvl_beam.h GroupBeamState) must arrive
 * at the tokens the device chose (GVL_ERR_HIP otherwise).  A group that was done when a step began is not processed: its beams are closed at once (their pages go back to
 * the pool), its s entries of the step's tokens are pad_id (which later groups DO count; pad_id < 0: an id that counts nowhere), they never become hypotheses.  The search
 * ends when every group is done or at max_new_tokens; every open group adds its beams, the hypotheses of all groups are pooled in group order and the num_return best leave
 * as from gvl_beam_search_n (outputs, ownership and the remaining errors are that call's: seq_id is never stepped, every clone is closed on every return path).  The
 * transition score of an id includes its Hamming term.  GVL_ERR_ARG: num_beam_groups outside 2 .. num_beams, num_beams % num_beam_groups != 0, diversity_penalty <= 0 or
 * NaN, vocab < 2 x (num_beams / num_beam_groups).
 * gvl_debug_group_beam_tokens: the tokens the DEVICE chose in the last gvl_group_beam_search of this context, step-major [steps][num_beams] (tests compare them with the
 * host bookkeeping's); *n_out = how many exist, at most cap are copied.  gvl_debug_group_beam_pool: behind every step's cache reorder of that search (every step but
 * the last) two numbers -- the clones the search held and the free KV pages: a group that finished has given its beams back by then. */
typedef struct gvl_group_beam_params {
  gvl_beam_params base;
  int   num_beam_groups;    /* 2 .. num_beams, dividing it */
  float diversity_penalty;  /* > 0 */
  int   pad_id;             /* -1: none */
} gvl_group_beam_params;
int gvl_group_beam_search(gvl_ctx* ctx, int seq_id, const float* first_logits, const gvl_group_beam_params* params, int num_return, int32_t* out_ids_host, int cap,
                          int* n_out, double* sequences_scores, float* transition_scores_host, void* stream);
int gvl_debug_group_beam_tokens(gvl_ctx* ctx, int32_t* out_host, int cap, int* n_out);
int gvl_debug_group_beam_pool(gvl_ctx* ctx, int32_t* out_host, int cap, int* n_out);

/* ---- contrastive search (HF generate(penalty_alpha > 0, top_k > 1, do_sample = False, num_beams = 1); transformers 4.40.1 GenerationMixin._contrastive_search and
 * _ranking_fast [ext], restated in tests/contrastive_ref.py; batch of one) -----------------------------------------------------------------------------------------
 * The hidden bank.  gvl_seq_keep_hidden(ctx, seq, 1) on an EMPTY sequence (before its prefill; GVL_ERR_STATE later) gives it a bank of max_tokens rows: per context row
 * the hidden state AFTER the final RMSNorm -- bf16 [hidden], bit for bit gvl_op_rmsnorm of that residual row with the final norm weight (fp32 statistics, bf16 out) --
 * and one fp32 inverse norm 1 / sqrtf(sum h^2) over the bf16 values of the row, summed in fp32 in a fixed order (lane l of one wave adds the squares of its elements
 * 8 (l + 64 i) .. + 7 in index order, i ascending, then the xor butterfly 32, 16, .. 1).  One device allocation, all or nothing (GVL_ERR_OOM), freed with the sequence;
 * on = 0 drops it.  hidden % 64 == 0 and hidden <= 8192, else GVL_ERR_ARG.  gvl_prefill of such a sequence runs the LAST decoder layer on every row (the last-layer
 * tail is off: its MLP output IS the bank) and appends one bank row per prompt row; every gvl_decode_step_logits / gvl_decode_step_logits_batch step appends the row of
 * the token it fed, so bank row j always belongs to position j.  Entries that are not taught the bank refuse a keep-hidden sequence with GVL_ERR_STATE and nothing
 * changed: gvl_prefill_varlen / _batch, gvl_prefill_extend*, gvl_score_extend_varlen, gvl_forward_loss, gvl_seq_fork, gvl_seq_fanout, gvl_seq_set_guidance pairs,
 * gvl_decode_greedy*, gvl_decode_steps, gvl_beam_search*.  gvl_seq_clone of a keep-hidden source gives a keep-hidden clone with its own copy of the rows so far
 * (GVL_ERR_OOM with nothing opened when the copy cannot be allocated).
 * gvl_seq_read_hidden: bank rows [first, first + n) as bf16 into rows_dev [n][hidden] and their inverse norms into inv_dev [n] (device; either may be NULL), on `stream`.
 *
 * gvl_contrastive_search.  seq_id is a PREFILLED keep-hidden sequence, first_logits (device, f32 [vocab]) the last_logits of its gvl_prefill.  Ownership is
 * gvl_beam_search's: seq_id is never stepped, the search runs on clones (capacity min(tokens + max_new_tokens + 1, cfg.max_seq)) and a private copy of the bank, every
 * sequence and buffer the call made is freed on every return path, the pool ends as it began.  Per step, the first token included:
 *     row   = the current context's last logits, behind the processors / rule set / grammar (HF's order, on RAW logits; history = the ids chosen so far).  No warpers.
 *     lp    = (l - max) - logf(sum exp(l - max))       gvl_beam_search's fixed-order log-softmax; candidates = the top_k largest lp, ties to the lower token id
 *     p_i   = expf(lp_i)                               rounded once
 *     the k candidates advance k sequences (the current one and k - 1 clones of it: opened all or nothing, their partial-page copies ONE launch) by ONE teacher-forced decode step on one stream of the weights (VALU-fallback
 *     geometries: parts of 4 / 2 / 1); g_i = candidate i's bank row (the same normalisation code), with its inverse norm
 *     dot_ij = sum_d g_i[d] h_j[d]                     fp32; products of two bf16 values are exact; the order depends on hidden only: lane l of an 8-lane group adds
 *                                                      elements 8 (l + 8 c) .. + 7 in index order with one fma each, c ascending, then the xor butterfly 4, 2, 1
 *     pen_i = max_j (dot_ij * inv_j) * ginv_i          bit-identical whatever k, the context length or the grid (the max is order-free)
 *     score_i = fmaf(-alpha, pen_i, (1 - alpha) * p_i) fp32; the arg-max wins, ties go to the lower candidate rank.  A candidate whose lp is -inf (fewer than k ids
 *                                                      survive a grammar or the token rules; it still fills its place in the trace) scores -inf and is never chosen
 * The winner's sequence lives on and takes over the bank, its row is committed as bank row n_ctx by the ranking launch itself; the losers go back to the pool; the winner's
 * logits are the next step's row.  One stream synchronise per step.  The search ends behind eos_id (appended) or at max_new_tokens.  Output: the new ids in out_ids_host
 * [cap >= max_new_tokens], their number in *n_out.  Trace (each may be NULL; host arrays): trace_ids / trace_p / trace_pen [steps][top_k] -- candidate ids in rank order,
 * their p and pen -- and trace_sel [steps], the selected rank.  trace_rows_dev (may be NULL; device f32 [cap][vocab]): per step the row the candidates were taken from,
 * behind the processors / rule set / grammar -- bit for bit gvl_op_logits_process* of the raw row with the ids chosen so far as history.  final_hidden_dev (may be NULL; device bf16 [n_out][hidden]): the bank rows the search committed.
 * Errors as gvl_beam_search's, and: top_k outside 2 .. 16, penalty_alpha outside [0, 1] or NaN, vocab < max(4, 2 * ((top_k + 1) / 2)) -- the candidate launches' row width --, the candidate rows beyond the ranking kernel's LDS
 * (rows x hidden x 2 bytes <= 128 KiB with rows = top_k rounded up to 4, 8 or 16: top_k <= 8 up to hidden 8192, top_k 9 .. 16 up to hidden 4096) (all GVL_ERR_ARG, before anything runs); a sequence without a bank
 * or whose bank is not in step with its position (GVL_ERR_STATE); device memory for the bank copy or KV pages exhausted (GVL_ERR_OOM). */
typedef struct gvl_contrastive_params {
  int top_k;                /* 2 .. 16 (GVL_MAX_DECODE_BATCH) */
  float penalty_alpha;      /* 0 .. 1 */
  int max_new_tokens;       /* >= 1 */
  int eos_id;               /* -1: none */
  float penalty; int ngram; int min_new; int proc_eos_id;  /* gvl_set_logits_processors' meaning; 1.0 / 0 / 0 / -1 = off */
  int rules_id;             /* -1: none */
} gvl_contrastive_params;
int gvl_seq_keep_hidden(gvl_ctx* ctx, int seq_id, int on);
int gvl_seq_read_hidden(gvl_ctx* ctx, int seq_id, int first, int n, uint16_t* rows_dev, float* inv_dev, void* stream);
int gvl_contrastive_search(gvl_ctx* ctx, int seq_id, const float* first_logits, const gvl_contrastive_params* params, int32_t* out_ids_host, int cap, int* n_out,
                           int32_t* trace_ids, float* trace_p, float* trace_pen, int32_t* trace_sel, float* trace_rows_dev, uint16_t* final_hidden_dev, void* stream);
/* Operator entries (caller-owned device buffers).  gvl_op_hidden_bank_append: residual rows x [n][cols] bf16 (rows ldx elements apart) -> rows_out [n][cols] =
 * gvl_op_rmsnorm(x, w, eps) bit for bit, inv_out [n] = their inverse norms (above).  gvl_op_contrastive_rank: bank [n_ctx][D] + bank_inv [n_ctx], cand [k][D] +
 * cand_inv [k], p [k] -> pen [k], score [k], *sel (all device), in the arithmetic above.  D % 64 == 0, D <= 8192, 2 <= k <= 16, n_ctx >= 1, alpha in [0, 1]. */
int gvl_op_hidden_bank_append(gvl_ctx* ctx, const uint16_t* x, int ldx, const uint16_t* w, float eps, uint16_t* rows_out, float* inv_out, int n, int cols, void* stream);
int gvl_op_contrastive_rank(gvl_ctx* ctx, const uint16_t* bank, const float* bank_inv, int n_ctx, int D, const uint16_t* cand, const float* cand_inv, const float* p, int k,
                            float alpha, float* pen, float* score, int32_t* sel, void* stream);

/* ---- multi-GPU exchange (SURVEY.md §8 e) -------------------------------------------------------------------------------------
 * The reference's inference is single-GPU (inference.py:17); sharding the frame batch over the GPUs of a node is this build's
 * addition: every rank encodes its segments, ONE all-gather moves the per-segment token blocks (llava_next_video.py:563) to
 * every rank.  RCCL is loaded with dlopen("librccl.so.1") on first use; a host without RCCL gets GVL_ERR_STATE.
 *   gvl_comm_unique_id : ncclGetUniqueId on rank 0; the 128 bytes travel to the other ranks by the host's own means
 *   gvl_comm_init      : ncclCommInitRank on the ctx's device (collective over all ranks).  Env GVL_RCCL_LIB overrides the
 *                        library name (default: librccl.so.1, librccl.so, /opt/rocm/lib/librccl.so.1)
 *   gvl_allgather_visual : local bf16 [rows_per_rank, hidden] -> all bf16 [world * rows_per_rank, hidden] (rank order) with
 *                        ncclAllGather on the caller's stream; `comm` = an ncclComm_t the host already owns, or NULL for the
 *                        ctx's communicator; world == 1 degenerates to one device copy. */
int gvl_comm_unique_id(char id_out[128]);
int gvl_comm_init(gvl_ctx* ctx, const char id[128], int rank, int world);
int gvl_comm_destroy(gvl_ctx* ctx);
/* ranks RCCL itself reports for the ctx's communicator (ncclCommCount); 1 when there is none.  bench.py prints it so that a
 * multi-GPU line shows how many ranks the collective really spanned. */
int gvl_comm_count(gvl_ctx* ctx, int* n_ranks);
int gvl_allgather_visual(gvl_ctx* ctx, void* comm, const uint16_t* local, int rows_per_rank, int hidden, uint16_t* all,
                         void* stream);
/* The same exchange for UNEVEN blocks, written straight into the segment-ordered prefix (llava_next_video.py:563: the per-segment blocks in segment
 * order): rank r contributes rows_per_rank[r] rows ([world] ints, host memory, the same on every rank) and they land at row offset
 * sum(rows_per_rank[0..r)) of `all` on every rank -- no padding to the largest block, no re-assembly copy.  One ncclGroup of per-rank broadcasts on
 * the caller's stream; `comm` must be NULL (the ctx's communicator).  Without a communicator: one device copy (or nothing when local == all). */
int gvl_allgatherv_visual(gvl_ctx* ctx, void* comm, const uint16_t* local, const int* rows_per_rank, int hidden, uint16_t* all, void* stream);

/* ---- training forward ---------------------------------------------------------- */
/* LLAVA_NEXT_VIDEO.forward(samples)["loss"] for ONE sample (llava_next_video.py:598-614): the causal-LM loss of
 * language_model(inputs_embeds, labels) -- Phi3ForCausalLM.forward labels branch (modeling_phi3.py:1512-1539; Llama alike):
 * logits[:-1] against labels[1:], ignore_index -100.  embeds bf16 [seq_len, hidden] (device, the spliced prefix WITHOUT the
 * masked right padding); labels int64 [seq_len] (host).  Returns the SUM of the token losses and their count, so that a batch
 * loss is sum(nll_sum) / sum(n_valid) exactly like CrossEntropyLoss(mean) over the flattened padded batch.  Only rows with a
 * label reach the lm_head.  Uses seq_id's KV pages as scratch (allocate >= seq_len tokens, free afterwards).  Forward only. */
int gvl_forward_loss(gvl_ctx* ctx, int seq_id, const uint16_t* embeds, int seq_len, const int64_t* labels_host,
                     double* nll_sum, int* n_valid, void* stream);

/* ---- frame pre-processing ---------------------------------------------------- */
/* frame_transform(image_size = size, mean, std) of the reference (mm_utils/utils.py:153-183, called per frame from
 * inference.py:69-88) for n uint8 RGB frames of one video: torchvision Resize(size, BICUBIC) [shortest edge -> size;
 * = PIL.Image.resize, Pillow Resample.c] -> CenterCrop(size) -> ToTensor -> Normalize, bit-exact to the CPU chain
 * (8-bit two-pass fixed-point resampler; three IEEE f32 operations for ToTensor/Normalize).
 * frames: device uint8, layout 0 = [n][H][W][3] (decoder order, mm_utils/video_utils.py:82) or 1 = [n][3][H][W]
 * (after the reference's permute, :91); out: device f32 [n][3][size][size].  Needs no weights (any ctx). */
int gvl_preprocess_frames(gvl_ctx* ctx, const uint8_t* frames, int n, int height, int width, int layout, int size,
                          const float* mean, const float* std3, float* out, void* stream);

/* ---- measurement ---------------------------------------------------------------------------- */
/* When enabled, every launch of a kernel family is bracketed by hipEvents on the caller's stream
 * (slow; bench.py uses it for ONE profiled step after the timed region). */
enum { GVL_PROF_GEMM = 0, GVL_PROF_ATTN = 1, GVL_PROF_GEMV = 2, GVL_PROF_DECODE_ATTN = 3, GVL_PROF_OTHER = 4,
       GVL_PROF_CS_RANK = 5,    /* gvl_contrastive_search: the ranking launch of a step (rank + finish kernels), one record per step */
       GVL_PROF_CS_CLONE = 6,   /* gvl_contrastive_search: the k - 1 clones of a step as ONE bracket (the launches inside are also booked under OTHER) */
       GVL_PROF_NCAT = 7 };
int gvl_prof_enable(gvl_ctx* ctx, int on);
int gvl_prof_read(gvl_ctx* ctx, int category, double* total_ms, int64_t* launches, double* work);

/* Result-neutral launch parameters, for tests and A/B measurements (the shipped library reads no kernel-selection environment variable):
 *   "decode_attn_cpb"  consecutive context splits one decode-attention block works through (0 = launcher's choice, 1..16)
 *   "decode_attn_hpb"  query heads of a KV head served by one block of the grouped-query decode kernel (0 = launcher's choice)
 *   "decode_graph"     1 (default): a decode group's step is captured once and replayed as a hipGraph for the following tokens; 0: eager
 *   "prefill_group"    sequences whose rows share one pass of the prefill GEMMs in gvl_prefill_varlen / _batch (1 .. 8, default 4: at the bench's 3.5 k-row prompts
 *                      8 measured neutral on clips/s and 0.7 % slower on the GEMM family -- 0.9 GB of activations per projection fall out of the
 *                      Infinity Cache; shorter prompts gain up to 4.7 % from 8, profiles/r03_gemm_prefill_group.txt)
 *   "vision_in_place"  1 (default): non-causal attention (vision towers, gvl_op_attention) reads V -- and Q, K when the head dim needs no padding
 *                      or transform; with InternVideo2's q RMSNorm applied in the kernel prologue -- straight from the fused-qkv matrix;
 *                      2: V only; 0: the round-2 path through Q / K pages and a V^T transpose pass
 *   "attn_pipe_rows"   128 (default): that kernel's 4-wave form (128 query rows per block) for every row; 256: whole 256-row query blocks on its 8-wave form (half
 *                      the DMA pieces per MFMA; measured 12 % slower), the remaining rows on the 4-wave form -- bit-identical (the 8-wave form decides the safe
 *                      re-pass per 128-row half of its block, as the 4-wave form does per block)
 *   "varlen_attn"      1 (default): the causal attention of a ragged prefill group (gvl_prefill_varlen) runs as ONE grid over the query blocks of all its sequences,
 *                      and so do its RoPE / KV-append and V^T-page passes (one launch each per layer); 2: the attention only (round 5), the passes per sequence;
 *                      0: one launch per sequence for all of them (rounds 2-4) -- bit-identical
 *   "varlen_extend"    1 (default): a gvl_prefill_extend_varlen group with a cached prefix runs RoPE / KV append, the V^T pages and causal attention as ONE launch each
 *                      per layer (a prefix per sequence inside the kernels); 0: one launch per sequence of the single-sequence extend kernels, GEMMs still shared -- bit-identical
 *   "norm_fused"       1 (default): RMSNorm in front of qkv / fc1 (InternVideo2) and qkv_proj / gate_up_proj / lm_head (LLM prefill AND, with bf16 decode weights,
 *                      the decode step) is fused into the GEMMs around it
 *                      (row statistics from the producing GEMM's epilogue, norm weight folded into the consuming GEMM's weight, row scale in its epilogue); 0: the
 *                      separate norm pass of rounds 1-4.  NOT bit-neutral -- the third stated exception below: two activation roundings of the reference
 *                      (x * rs and the gamma product, both to bf16) are gone and gamma * W is rounded once per weight instead
 *   "gemm_band"        0 (default): the rasterisation band of the 256 x 256 GEMM kernels (8-wave ping-pong and both 4-wave forms) is 4 tile rows; 1..64: that many
 *                      rows for every later launch of the PROCESS (A/B only) -- bit-identical
 *   "gemm_a4"          which form of the 256 x 256 GEMM kernel a launch takes: 1 (default) per fused epilogue, as measured -- the 4-wave kernel with the epilogue
 *                      pipelined into the next tile's main loop (gvl_gemm4p.hip) for erf-GELU / SwiGLU / residual + row statistics / bias alone, the plain
 *                      4-wave kernel (gvl_gemm4.hip: accumulators in AGPRs, hand-placed k loop) for the store-only epilogues (plain, row scale, SwiGLU without
 *                      row scale, residual alone, row statistics alone), the 8-wave ping-pong kernel for the rest;
 *                      0: always the 8-wave kernel; 2: the plain 4-wave kernel wherever it serves; 3: the pipelined one wherever it serves.  For every later
 *                      launch of the PROCESS -- bit-identical
 *   "gemm_narrow"      1 (default): the pipelined 4-wave kernel runs a column tile with <= 128 real columns (N = 1408 = 5.5 tile columns: every sixth tile of
 *                      InternVideo2's proj / fc2) as a NARROW tile -- 4 waves x (128 rows x 64 columns), no MFMA on the empty half; 0: as a full tile.  For every
 *                      later launch of the PROCESS -- bit-identical
 *   "last_layer_tail"  1 (default): a prefill without a loss request runs the LAST decoder layer's MLP on the sequences' last rows only (nothing else reads its
 *                      output); 0: on every row -- bit-identical
 *   "patch_fused"      1 (default): the patch embedding of a tower whose geometry the fused kernel covers (patch 14, width 1024 / 1408) runs as ONE kernel
 *                      (gvl_patch.hip: im2col in the operand loader + GEMM + CLS / position rows + CLIP's pre-LayerNorm); 0: the three-pass path (patchify, GEMM,
 *                      embed).  NOT bit-neutral: the fp32 accumulation order over k differs (agreement to fp32 rounding before the bf16 round; tests/test_gpu_towers.py)
 *   "attn_pipe"        1 (default): InternVideo2's attention (head dim 88, q in place) runs the software-pipelined key-tile loop
 *                      (attn_iv2_pipe_kernel, round 4); 0: the plain loop of attn_fwd_kernel; 2: the pipelined kernel's SAFE pass alone.  Bit-identical to 0
 *                      WHILE attn_fwd_kernel's lazy rule never fires after a row's first key tile (every golden, the bench: asserted in
 *                      tests/test_gpu_towers.py); the pipelined normal pass keeps the first tile's maximum as the softmax reference for the whole row, so on
 *                      scores where a later tile exceeds it by more than 2^8 the two differ at P-rounding level (bounded at 1.5e-2 of the output scale by
 *                      the sharp-score test there) -- the second stated exception below; mode 2 is bit-identical to 0 on any data
 * None of them may change a single output bit (asserted in tests/test_gpu_llm.py) -- with THREE stated exceptions: "norm_fused" and "attn_pipe" = 1 on
 * peaked scores (above), and "vision_in_place" = 1 on a head
 * dim that is padded (InternVideo2, 88 -> 96) folds the softmax scale and shift into q before its one rounding to bf16, a different (not larger)
 * set of rounding points: modes 0 and 2 are bit-identical to each other, mode 1 is bit-identical to them for CLIP (head dim 64) and agrees within
 * bf16 noise for InternVideo2 (one block 4.1e-3 of the output scale; 39 blocks vs the reference: the same error as the reference's own bf16,
 * tests/test_gpu_towers.py, tests/test_gpu_c0.py). */
int gvl_debug_set(gvl_ctx* ctx, const char* key, int value);

/* ---- operator-level entry points (parity tests call the kernels through these) --------------- */
/* C[M,N] = act(A[M,K] W[N,K]^T + bias) (+ resid); A,W bf16; bias/gamma f32 or NULL.
 * act: 0 none, 1 quick_gelu, 2 gelu(erf), 3 silu(gate)*up on interleaved (gate,up) column pairs
 * (output has N/2 columns).  out_f32: C is f32 else bf16; resid has C's dtype and layout. */
int gvl_op_gemm(gvl_ctx* ctx, const uint16_t* A, const uint16_t* W, void* C, int M, int N, int K,
                const float* bias, const float* gamma, const void* resid, int act, int out_f32,
                int tile_cfg, void* stream);
/* Fused RMSNorm at operator level (round 5; what the towers and the prefill run: models/internvideo2.py:443-448,590-603, modeling_phi3.py:319-324):
 *   RMSNorm(x) W^T  ==  rs[m] * (x (W diag(gamma))^T),   rs[m] = rsqrt(mean_k x[m][k]^2 + eps)
 * gvl_op_gemm_rows: gvl_op_gemm with bf16 output plus rowscale ([M] f32 or NULL: multiplies the accumulator rows before bias / activation) and rowsq
 * ([M][rowsq_ld] f32 or NULL: the GEMM that WRITES the residual stream leaves the sum of squares of its rounded outputs per aligned block of 64 columns;
 * N % 64 == 0).  gvl_op_fold_gamma: Wo = bf16(W diag(gamma)), W [rows][cols], gamma [cols] bf16.  gvl_op_rowsq_finish: rs[m] = rsqrt((sum of the blocks
 * [b0, b0 + nblk) of row m) / cols + eps). */
int gvl_op_gemm_rows(gvl_ctx* ctx, const uint16_t* A, const uint16_t* W, uint16_t* C, int M, int N, int K, const float* bias, const float* gamma,
                     const uint16_t* resid, int act, const float* rowscale, float* rowsq, int rowsq_ld, int tile_cfg, void* stream);
/* gvl_op_gemm with the row-remapping store of the visual prefix (operator tests: tests/test_gpu_vision_ops.py): GEMM row m is stored at row
 *   (m / grp_rows) * grp_stride + m % grp_rows + row_off
 * of C (and read from there in resid), so C and resid hold ceil(M / grp_rows) * grp_stride rows of N columns; the rows between the groups are not touched.
 * grp_rows >= 1, row_off >= 0 and row_off + grp_rows <= grp_stride, else GVL_ERR_ARG.  rowsq / rowsq_ld as in gvl_op_gemm_rows: no kernel serves the row
 * statistics together with a remap, a non-NULL rowsq is refused (GVL_ERR_ARG, nothing written). */
int gvl_op_gemm_grouped(gvl_ctx* ctx, const uint16_t* A, const uint16_t* W, void* C, int M, int N, int K, const float* bias, const float* gamma,
                        const void* resid, int act, int out_f32, float* rowsq, int rowsq_ld, int grp_rows, int grp_stride, int row_off, int tile_cfg,
                        void* stream);
int gvl_op_fold_gamma(gvl_ctx* ctx, const uint16_t* W, const uint16_t* gamma, uint16_t* Wo, int64_t rows, int cols, void* stream);
int gvl_op_rowsq_finish(gvl_ctx* ctx, const float* rowsq, int ld, int b0, int nblk, float* rs, int rows, int cols, float eps, void* stream);
/* attention over q/k/v bf16 [B,S,H|KV,D] (plain layout; the library re-tiles internally).
 * out bf16 [B,S,H*D].  causal: 0/1. */
int gvl_op_attention(gvl_ctx* ctx, const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out,
                     int B, int S, int H, int KV, int D, float scale, int causal, void* stream);
int gvl_op_layernorm(gvl_ctx* ctx, const float* x, const float* w, const float* b, uint16_t* y, int rows,
                     int cols, float eps, void* stream);
int gvl_op_rmsnorm(gvl_ctx* ctx, const uint16_t* x, const uint16_t* w, uint16_t* y, int rows, int cols,
                   float eps, void* stream);
/* The patch embedding of either vision tower on its own (operator tests: tests/test_gpu_vision_ops.py).  All pointers are device memory.
 *   mode 0 = CLIP:         out f32  [n][1 + L][C]    = LayerNorm(cat(cls, bf16(conv(px))) + pos; lnw, lnb, eps), T must be 1
 *   mode 1 = InternVideo2: out bf16 [n][1 + T L][C]  = bf16(cat(cls, bf16(conv(px) + bias)) + pos)
 *   with L = (image / patch)^2 and conv = a convolution of stride = kernel = patch over px f32 [n][3][T][image][image]; W bf16 [C][Kp] row-major,
 *   k = (c * patch + py) * patch + px, columns [3 patch^2, Kp) ignored.  cls [C] and pos [1 + T L][C] are f32 (mode 0) or bf16 (mode 1); bias [C] f32 (mode 1);
 *   lnw, lnb [C] f32 and eps (mode 0).
 *   path 0 = the fused kernel (gvl_patch.hip; patch 14, C 1024 or 1408 -- CLIP: 1024): the call makes its own tile-order copy of W in the workspace arena.
 *            A geometry the fused launcher refuses comes back as GVL_ERR_ARG: there is NO fall-back to path 1 here, the caller knows which kernel ran.
 *   path 1 = the three passes: im2col (patchify), the patch GEMM, the embedding kernel.  Kp % 64 == 0, C % 8 == 0 (mode 0: C <= 4096).  im2col (or NULL)
 *            receives the bf16 im2col matrix [n T L][Kp], zero in the columns [3 patch^2, Kp).  im2col must be NULL on path 0.
 * Refusals (GVL_ERR_ARG; GVL_ERR_OOM when the workspace arena cannot hold the copies) are returned before anything is written to out or im2col. */
typedef struct {
  int32_t mode, path;
  int32_t n, T, image, patch, C, Kp;
  float eps;
  const float* px;
  const uint16_t* W;
  const float* bias;
  const void* cls;
  const void* pos;
  const float* lnw;
  const float* lnb;
  void* out;
  uint16_t* im2col;
} gvl_patch_embed;
int gvl_op_patch_embed(gvl_ctx* ctx, const gvl_patch_embed* p, void* stream);
/* im2col alone (any patch size): px f32 [n][3][T][image][image] -> A bf16 [n T (image / patch)^2][Kp], Kp % 8 == 0, Kp >= 3 patch^2, image % patch == 0. */
int gvl_op_patchify(gvl_ctx* ctx, const float* px, uint16_t* A, int n, int T, int image, int patch, int Kp, void* stream);
/* The glue kernels of the visual prefix on their own.  Their token geometry is FIXED (it is the model's: gvl_build_visual refuses any other tower geometry):
 *   gvl_op_hd_merge      f f32 [n][576 = 24 x 24][C], sub_gn f32 [4 C] -> out bf16 [n][156 = 12 x 13][4 C]: row (h, w < 12) = the 2 x 2 block (2h + dy, 2w + dx) of f,
 *                        channel chunks in (dy, dx) order; row (h, 12) = sub_gn.  C % 4 == 0.
 *   gvl_op_pool_spatial  f f32 [n][576][C] -> out bf16 [n][64 = 8 x 8][C]: the mean of each 3 x 3 window, summed in fp32, divided by 9.  C % 4 == 0.
 *   gvl_op_pool_temporal f bf16 [n][T][256 = 16 x 16][C] -> out bf16 [n][T][16 = 4 x 4][C]: the mean of each 4 x 4 window, summed in fp32, times 2^-4.  C % 8 == 0.
 *   gvl_op_strip_cls     y[n][s][:] = x[n][s + 1][:], x [n][S][C] of elem_bytes 2 or 4, S >= 2, C * elem_bytes % 4 == 0.
 *   gvl_op_bcast_row     dst[(s * stride_rows + row_off)][:] = row[:] for s < n; row, dst bf16, dst [n * stride_rows][cols], 0 <= row_off < stride_rows.
 * n >= 1, T >= 1, C >= 1; anything else is GVL_ERR_ARG before a launch. */
int gvl_op_hd_merge(gvl_ctx* ctx, const float* f, const float* sub_gn, uint16_t* out, int n, int C, void* stream);
int gvl_op_pool_spatial(gvl_ctx* ctx, const float* f, uint16_t* out, int n, int C, void* stream);
int gvl_op_pool_temporal(gvl_ctx* ctx, const uint16_t* f, uint16_t* out, int n, int T, int C, void* stream);
int gvl_op_strip_cls(gvl_ctx* ctx, const void* x, void* y, int n, int S, int C, int elem_bytes, void* stream);
int gvl_op_bcast_row(gvl_ctx* ctx, const uint16_t* row, uint16_t* dst, int n, int stride_rows, int row_off, int cols, void* stream);
/* y[N] = W[N,K] x[K] (+bias) -- the decode GEMV; x,W bf16, y f32. */
int gvl_op_gemv(gvl_ctx* ctx, const uint16_t* W, const uint16_t* x, const float* bias, float* y, int N, int K,
                void* stream);
/* The sampler on its own (operator test): logits f32 device [batch][n] -> tokens_dev int32 device [batch]; row b draws from
 * random stream streams[b] (host array) at generation step steps_dev[b] (device array).  batch <= 16. */
int gvl_op_sample(gvl_ctx* ctx, const float* logits, int n, int batch, float temperature, int top_k, float top_p, uint64_t seed,
                  const uint32_t* streams, const int32_t* steps_dev, int32_t* tokens_dev, void* stream);
/* The logits processors on their own (operator tests; beam search applies them to its log-softmax rows): logits f32 device [batch][n],
 * changed IN PLACE; row b's history is hist_dev[b * hist_stride .. + lens_dev[b]) (int32 device; lengths are clamped to
 * min(hist_stride, 8192)); per-row parameters are host arrays with gvl_set_logits_processors' meaning.  batch <= 16. */
int gvl_op_logits_process(gvl_ctx* ctx, float* logits, int n, int batch, const int32_t* hist_dev, int hist_stride, const int32_t* lens_dev,
                          const float* penalty, const int* ngram, const int* min_new, const int* eos_ids, void* stream);
/* gvl_op_logits_process plus one rule-set id per row (host array; -1 = no rules): the whole ordered pipeline on raw rows. */
int gvl_op_logits_process_rules(gvl_ctx* ctx, float* logits, int n, int batch, const int32_t* hist_dev, int hist_stride, const int32_t* lens_dev,
                                const float* penalty, const int* ngram, const int* min_new, const int* eos_ids, const int* rules_ids, void* stream);
/* ... plus one grammar id per row (host arrays; rules_ids / grammar_ids may be null, -1 = none): a grammar's vocab must equal n. */
int gvl_op_logits_process_ex(gvl_ctx* ctx, float* logits, int n, int batch, const int32_t* hist_dev, int hist_stride, const int32_t* lens_dev,
                             const float* penalty, const int* ngram, const int* min_new, const int* eos_ids, const int* rules_ids, const int* grammar_ids,
                             void* stream);
/* Token selection with log-probabilities on its own (operator tests): greedy (do_sample = 0; streams / steps_dev may be null) or
 * gvl_op_sample's draw; row b with top_n[b] >= 0 (host array) stores its token's log-probability at lp_dev[b], and for top_n[b] >= 1
 * its top list at top_ids_dev / top_lp_dev [b * 8 ..) (gvl_set_logprobs' meaning).  batch <= 16. */
int gvl_op_select_logprobs(gvl_ctx* ctx, const float* logits, int n, int batch, int do_sample, float temperature, int top_k, float top_p,
                           uint64_t seed, const uint32_t* streams, const int32_t* steps_dev, const int* top_n, int32_t* tokens_dev,
                           float* lp_dev, int32_t* top_ids_dev, float* top_lp_dev, void* stream);
/* Per-row token selection on its own (operator tests): row b is greedy or sampled by rows[b] (host array of `batch` <= 16 settings, each with its own seed and stream) at
 * generation step steps_dev[b] (device array; may be null when every row is greedy); tokens / lp / top lists as gvl_op_select_logprobs.  kept_dev (device, batch * n bytes,
 * may be null): 1 where an entry is finite and in the row's final kept set (a greedy row keeps every finite entry), else 0. */
int gvl_op_select_rows(gvl_ctx* ctx, const float* logits, int n, int batch, const gvl_sampling* rows, const int32_t* steps_dev, const int* top_n,
                       int32_t* tokens_dev, float* lp_dev, int32_t* top_ids_dev, float* top_lp_dev, uint8_t* kept_dev, void* stream);
/* The guidance kernel on its own (operator tests): logits f32 device, row r at logits + r * ld (ld >= n); pairs_host [n_pairs][2] = (conditional row, negative row),
 * 1 .. 8 pairs, scales_host [n_pairs] finite.  Pair p's conditional row is overwritten with scales[p] * (c - u) + u as above; every other row is untouched.  A conditional
 * row may not appear in another pair (GVL_ERR_ARG); a negative row may serve several. */
int gvl_op_guidance(gvl_ctx* ctx, float* logits, int n, int ld, const int* pairs_host, int n_pairs, const float* scales_host, void* stream);
/* gvl_score_extend_varlen's row kernel on its own (operator tests): `rows` rows (any number) of n fp32 logits, ld >= n floats apart, targets_dev [rows]; lp_dev / rank_dev
 * [rows] and, top_n 1 .. 8, top_ids_dev / top_lp_dev [rows][8] as described there (top_n = 0: untouched, may be NULL).  A target outside [0, n) never indexes its row:
 * lp = -inf, rank = -1. */
int gvl_op_score_rows(gvl_ctx* ctx, const float* logits_dev, int n, int ld, int rows, const int32_t* targets_dev, int top_n, float* lp_dev, int32_t* rank_dev,
                      int32_t* top_ids_dev, float* top_lp_dev, void* stream);
/* One beam-search step's candidates on their own (operator tests; hosts that keep their own books): rows f32 device, row b of n entries at rows + b * row_stride
 * (row_stride 0: every beam reads row 0, as the first step does; otherwise >= n), k = num_beams 2 .. 16, n >= 2 k; beam_scores_host [k].  rows_are_logprobs = 0: raw
 * logits, the log-softmax runs inside; 1: processed log-probabilities.  vals_dev / idx_dev / proc_dev [2 k] (device): value t, flat index beam * n + token, and the
 * log-probability before the score was added, in gvl_beam_search's order.  gvl_op_beam_normalize: rows [k][n] (k 1 .. 16) raw logits -> log-softmax IN PLACE; normalize
 * followed by candidates with rows_are_logprobs = 1 is bit-identical to candidates with 0.  NaN rows are outside the contract. */
int gvl_op_beam_candidates(gvl_ctx* ctx, const float* rows, int n, int k, int row_stride, const float* beam_scores_host, int rows_are_logprobs, float* vals_dev,
                           int32_t* idx_dev, float* proc_dev, void* stream);
int gvl_op_beam_normalize(gvl_ctx* ctx, float* rows, int n, int k, void* stream);
/* One GROUP of a diverse beam search step on its own (operator tests): gvl_op_beam_candidates for the group's s rows (s 1 .. 16, n >= 2 s; outputs [2 s], flat index
 * local beam * n + token), and the group's choice in chosen_dev [s] (device int32): the tokens of the first s candidates that are not eos_id (-1: none; fewer than s such
 * candidates: -1 for the rest).  group_done != 0: no candidates are computed (rows / scores / outputs may be null), chosen_dev [s] <- pad_id (< 0: -1). */
int gvl_op_beam_group(gvl_ctx* ctx, const float* rows, int n, int s, int row_stride, const float* beam_scores_host, int rows_are_logprobs, int eos_id, int pad_id,
                      int group_done, float* vals_dev, int32_t* idx_dev, float* proc_dev, int32_t* chosen_dev, void* stream);
/* gvl_op_logits_process_ex with HammingDiversityLogitsProcessor in HF's place (behind sequence_bias, in front of the repetition penalty): every row loses
 * fp32(diversity_penalty * count) at each token of ham_tokens_dev [n_ham] (device int32, 0 .. 16 ids, read by the kernel at run time; ids outside [0, n) are ignored),
 * count = how often the token is listed. */
int gvl_op_logits_process_hamming(gvl_ctx* ctx, float* logits, int n, int batch, const int32_t* hist_dev, int hist_stride, const int32_t* lens_dev,
                                  const float* penalty, const int* ngram, const int* min_new, const int* eos_ids, const int* rules_ids, const int* grammar_ids,
                                  const int32_t* ham_tokens_dev, int n_ham, float diversity_penalty, void* stream);
/* y[b][N] = W[N,K] x[b][K] (+bias) for b < batch <= 16 -- the decode projections as ONE skinny MFMA GEMM (the weight stream is
 * read once for all sequences; K % 256 == 0).  x bf16 [batch][K], y f32 [batch][N]. */
int gvl_op_dgemm(gvl_ctx* ctx, const uint16_t* W, const uint16_t* x, const float* bias, float* y, int N, int K, int batch,
                 void* stream);
/* One decode projection with every prologue / epilogue of the two decode kernels (operator tests: tests/test_gpu_decode_proj.py).  All pointers are device
 * memory; W and x arrive ROW-MAJOR and the call tiles / quantises private copies as the chosen path needs (W itself is never written).  Zero / NULL = off.
 *   path 0 = the skinny MFMA GEMM, 1 = the VALU GEMV (serves batch 1, 2, 4 and none of variant, w_fmt, x_is_tiled, out_tiled, sq_in, sq_out, out_tiled2).
 *   variant: 0 = the launcher's default, else rb * 1000 + nw * 100 + u * 10 + nt.   w_fmt: 0 bf16, 1 FP8 (e4m3, power-of-two row scale), 2 MXFP4.
 *   K % 256 == 0 on path 0 (FP8: K % 512, MXFP4: K % 1024), K % 8 == 0 on path 1.  x [batch][K] bf16; x_is_tiled: x is already in the decode activation tile order (16 K elements; a producer's out_tiled2).
 *   act: GVL_ACT_NONE or GVL_ACT_SILU_MUL (interleaved gate / up rows, N / 2 outputs).  out_stride: elements between two sequences' rows of out_bf16 /
 *   out_f32 / resid (0: N, or N / 2 with SILU_MUL); on path 0 with batch > 1 it must be a multiple of 4 (the epilogue stores 8 and 16 bytes at a time).  out_tiled: the SILU_MUL out_bf16 is written in tile order (16 * N / 2 elements).
 *   norm_w [K] bf16 + eps: x is RMS-normalised inside the kernel (batch <= 4; on path 0 also K <= 4096; x rows are K elements apart, so K % 4 == 0 holds).  sq_in [batch][sq_n] f32 + eps: the consumer side of the fused norm (W is
 *   expected to carry the norm weight already: gvl_op_fold_gamma).  sq_out [batch][N / 16] f32 and out_tiled2 (16 N elements): the producer side.
 *   rope_on: the qkv epilogue; N == (H + 2 KV) Dr, W in the model's row order (the rotate-half row permutation is applied to the private copy).  cos / sin
 *   tables [max_pos][Dr / 2] f32 (the _l pair is used when pos + 1 > rope_switch > 0), pos [batch] int32, tables [batch][table_stride] int32 page numbers,
 *   Q [batch][q_stride], Kt / Vt [n_pages][KV][64][D] / [n_pages][KV][D][64].  The call reads pos and tables back and refuses any position >= max_pos,
 *   any page index outside table_stride and any page >= n_pages before it launches.
 *   w_deq [N][K] bf16 (w_fmt != 0, or NULL): receives the de-quantised weight the quantiser leaves behind, in W's row order.  w_scale (or NULL): FP8: [N] f32
 *   row scales by LOGICAL row (pair order with rope_on); MXFP4: the scale words [ceil(N / 16)][K / 128][16] u32, byte j of word (row block, k / 128, row % 16)
 *   = the E8M0 scale of k step 4 (k / 128) + j of that logical row.
 * MXFP4 convention: a block of 32 whose largest magnitude has an fp32 exponent field <= 2 (below 2^-124) gets scale byte 0, and scale byte 0 means "a block
 * of zeros" (2^-127 is not a normal fp32): every element of such a block de-quantises to +0.
 * Whatever the chosen launcher refuses comes back as GVL_ERR_ARG with a message and nothing is written to any output.  Synchronises the stream. */
typedef struct {
  int32_t path, variant, w_fmt;
  int32_t N, K, batch;
  const uint16_t* W;
  const uint16_t* x;
  int32_t x_is_tiled;
  int32_t act;
  const float* bias;
  const uint16_t* resid;
  uint16_t* out_bf16;
  float* out_f32;
  int32_t out_tiled;
  int32_t out_stride;
  const uint16_t* norm_w;
  float eps;
  int32_t sq_n;
  const float* sq_in;
  float* sq_out;
  uint16_t* out_tiled2;
  int32_t rope_on, rope_switch;
  const float* cos_s; const float* sin_s; const float* cos_l; const float* sin_l;
  int32_t max_pos, n_pages;
  const int32_t* pos;
  const int32_t* tables;
  int32_t table_stride, q_stride;
  uint16_t* Q; uint16_t* Kt; uint16_t* Vt;
  int32_t H, KV, Dr, D;
  uint16_t* w_deq;
  void* w_scale;
} gvl_decode_proj;
int gvl_op_decode_proj(gvl_ctx* ctx, const gvl_decode_proj* p, void* stream);
/* One decode-attention launch: one new query per head against a paged cache (operator tests: tests/test_gpu_decode_attn_exact.py).  All pointers are
 * device memory and the caller owns every buffer, the split workspace included.
 *   q        bf16 [batch][H][D], q_stride elements between two sequences (>= H D, a multiple of 8; q 16-byte aligned); columns Dout .. D - 1 of a head are 0
 *   Kt, Vt   the pools of ONE layer: bf16 [n_pages][KV][64][D] (key rows) and [n_pages][KV][D][64] (V transposed); token t of a sequence is slot t % 64 of
 *            page tables[b][t / 64]
 *   tables   int32 [batch][table_stride] page numbers;  pos int32 [batch]: the index of each sequence's newest token (its cache holds pos + 1 tokens)
 *   part     f32 [batch][H][nsplit][D + 2] partial records (D accumulators, running maximum in log2 units, sum), any contents before the launch
 *   counters int32 [batch][H] tickets: ZERO before the launch, zero again after it
 *   out      bf16 [batch][H Dout], out_stride elements between two sequences (>= H Dout), or -- out_tiled -- the decode activation tile order: element
 *            (b, k) at ((k >> 5) * 64 + ((k >> 3) & 3) * 16 + b) * 8 + (k & 7)
 *   D        64, 96 or 128 (the padded head dim), Dout <= D the real one;  H % KV == 0;  1 <= nsplit <= 16;  scale: the softmax scale
 *   A sequence of n = ceil((pos + 1) / 64) pages uses ns = min(nsplit, ceil(n / 4)) context splits of ceil(n / ns) pages and one record per split.
 *   cpb      consecutive splits per block (0 = 1), gsplit  block slots along the context (0 = ceil(nsplit / cpb)), hpb  query heads of a group per block
 *            on the grouped-query kernel (0 or no divisor of H / KV = all): launch shape only, no value may change an output bit.
 * The call reads pos and tables back and returns GVL_ERR_ARG with a message, before anything is launched or written, when the launch plan does not serve
 * the geometry, a position is outside [0, 64 table_stride), one of a sequence's first ceil((pos + 1) / 64) pages is outside [0, n_pages), gsplit * cpb is
 * smaller than the longest sequence's split count (blocks would be missing and the ticket would never complete), Dout > D or a stride is shorter than its
 * row.  Synchronises the stream. */
typedef struct {
  const uint16_t* q;
  const uint16_t* Kt; const uint16_t* Vt;
  const int32_t* tables;
  const int32_t* pos;
  float* part;
  int32_t* counters;
  uint16_t* out;
  int32_t q_stride, n_pages, table_stride, out_stride, out_tiled;
  int32_t batch, H, KV, D, Dout, nsplit, hpb, cpb, gsplit;
  float scale;
} gvl_decode_attn;
int gvl_op_decode_attention(gvl_ctx* ctx, const gvl_decode_attn* p, void* stream);
/* One launch of the pass between the prefill QKV GEMM and attention: a fused qkv matrix -> Q, K pages and V^T pages (operator tests: tests/test_gpu_qkv_post.py).
 * All pointers are device memory and the caller owns every buffer; block tables are device int32.
 *   qkv      bf16 rows of [H Dr | KV Dr | KV Dr] (q, k, v), ld elements apart (>= (H + 2 KV) Dr, a multiple of 8); B S rows, or -- a ragged group -- vl_rows[vl_n]
 *   Q        bf16 [B][H][S][D]; ragged: member u's block [H][S_u][D] starts at element vl_rows[u] H D.  Not written (may be NULL) when q_rs is set
 *   Kt, Vt   page pools bf16 [n_pages][KV][64][D] (key rows) and [n_pages][KV][D][64] (V transposed): the token at position p of a sequence is slot p % 64 of the
 *            sequence's page p / 64.  Vt NULL: keys and queries only (pos0 need not be a multiple of 64 then)
 *   pages    block_table NULL (needs pos0 == 0): page(b, t) = b ceil(S / 64) + t;  else int32 [B][max_pages];  ragged: vl_tables[u], int32 [table_len[u]]
 *   Dr, D    the real and the padded head dim: Dr % 8 == 0 (mode 2: % 16), Dr <= 128, D % 8 == 0, D >= Dr.  Columns Dr .. D - 1 of every Q and K row written are 0,
 *            but K column Dr is 1.0 under k_ones;  of a V^T page that is written ALL 64 slots of all D rows are: rows >= Dr and the slots of tokens behind the
 *            sequence's last new token are 0, but row Dr is 1.0 in every slot under ones_row (both need D > Dr)
 *   mode 0   q, k copied.
 *   mode 1   q' [c] = bf16(qn[c] * bf16(q[c] * rs)), rs = rsqrt(sum of the row's H Dr squares / (H Dr) + eps) in fp32 (InternVideo2's full-width RMSNorm), k likewise
 *            with kn over KV Dr;  q_rs set (f32 [B S]; needs k_ones): q's rs is stored there and Q is not written
 *   mode 2   RoPE at position p = pos0 + i (ragged extend: vl_pos0[u] + i) from cos / sin f32 [max_pos][Dr / 2] holding bf16-representable values, per head with
 *            half = Dr / 2:  d < half: bf16(bf16(x[d] cos[p][d]) + bf16(-x[d + half] sin[p][d]));  d >= half: bf16(bf16(x[d] cos[p][d - half]) + bf16(x[d - half] sin[p][d - half]))
 *   ragged   vl_n in 1 .. 8 (mode 2, B == 1, pos0 == 0, block_table NULL): member u owns rows [vl_rows[u], vl_rows[u + 1]), vl_rows[0] == 0, no member empty
 *   ext      0: gvl_launch_qkv_post;  1: gvl_launch_qkv_post_ext -- the ragged group where member u already holds vl_pos0[u] tokens (a multiple of 64, whole pages):
 *            needs vl_n >= 1, Vt and no q_rs
 * The call reads the tables back and returns GVL_ERR_ARG with a message, before anything is launched or written, for whatever the launcher refuses and for: a page
 * outside [0, n_pages) or named twice among the pages the launch writes, a position >= max_pos in mode 2, a table shorter than ceil((pos0 + S_u) / 64), Vt with
 * pos0 % 64 != 0, pos0 > 0 without a table, vl_rows[0] != 0 or an empty member, q_rs without k_ones, ones_row / k_ones with D == Dr, mode 1 without qn / kn.
 * Synchronises the stream. */
typedef struct {
  const uint16_t* qkv; int32_t ld;
  uint16_t* Q; uint16_t* Kt; uint16_t* Vt;
  const int32_t* block_table; int32_t max_pages;
  int32_t B, S, H, KV, Dr, D;
  int32_t mode;
  const uint16_t* qn; const uint16_t* kn; float eps;
  const float* cos; const float* sin; int32_t pos0;
  int32_t ones_row, k_ones;
  float* q_rs;
  int32_t vl_n;
  int32_t vl_rows[9];
  const int32_t* vl_tables[8];
  int32_t vl_pos0[8];
  int32_t table_len[8];
  int32_t n_pages, max_pos, ext;
} gvl_qkv_post;
int gvl_op_qkv_post(gvl_ctx* ctx, const gvl_qkv_post* p, void* stream);
/* One prefill-attention launch on caller-owned pages: the paged forms of attn_fwd_kernel behind a cached prefix (operator tests: tests/test_gpu_prefill_attn.py).
 * The in-place and InternVideo2 forms and implicit pages stay with gvl_op_attention.  All pointers are device memory; block tables are device int32.
 *   Q        bf16 [B][H][S][D], columns Dout .. D - 1 zero; ragged: member u's block [H][S_u][D] starts at element vl_rows[u] H D
 *   Kt, Vt   the page pools as gvl_op_qkv_post writes them: bf16 [n_pages][KV][64][D] and [n_pages][KV][D][64]; key j of a sequence is slot j % 64 of its page j / 64.
 *            K slots of keys >= Sk may hold anything (the kernel masks by index); V^T slots of keys >= Sk and the pad rows / columns must be FINITE
 *   O        bf16 [B S][H Dout] (ragged: row vl_rows[u] + i), 16-byte aligned
 *   single   vl_n == 0: B sequences of S queries, query i at position qpos0 + i of a context of Sk keys (0 = S; else Sk >= qpos0 + S), pages block_table
 *            [B][max_pages];  causal: query i sees keys 0 .. qpos0 + i, else all Sk.  ring: K / V LDS ring depth 0 (launcher's choice), 2 or 3 -- no value may change a bit
 *   ragged   vl_n in 1 .. 8 (causal, B == 1, Sk == qpos0 == 0, block_table NULL; S = the longest member): member u owns rows [vl_rows[u], vl_rows[u + 1]) and the table
 *            vl_tables[u] (int32 [table_len[u]]);  ext = 1 (gvl_launch_attention_ext): member u's query i sits at position vl_pos0[u] + i (a multiple of 64) and sees
 *            the vl_pos0[u] + S_u keys of its table.  ext = 0: gvl_launch_attention, vl_pos0 ignored
 *   D        64, 96 or 128, Dout <= D a multiple of 8, H % KV == 0, at most 256 key tiles
 * The call reads the tables back and returns GVL_ERR_ARG with a message, before anything is launched or written, for whatever attn_plan / attn_ext_plan refuse, a
 * missing table, a table shorter than the key tiles the launch reads (causal: ceil((qpos0 + S_u) / 64), else ceil(Sk / 64)) and a page outside [0, n_pages) among
 * them.  Synchronises the stream. */
typedef struct {
  const uint16_t* Q; const uint16_t* Kt; const uint16_t* Vt; uint16_t* O;
  const int32_t* block_table; int32_t max_pages;
  int32_t B, H, KV, S, D, Dout, Sk, qpos0;
  float scale;
  int32_t causal, ring;
  int32_t vl_n;
  int32_t vl_rows[9];
  const int32_t* vl_tables[8];
  int32_t vl_pos0[8];
  int32_t table_len[8];
  int32_t ext, n_pages;
} gvl_prefill_attn;
int gvl_op_prefill_attention(gvl_ctx* ctx, const gvl_prefill_attn* p, void* stream);
/* The attention launch of one InternVideo2 block on caller-owned buffers: the ones-row (ONES) forms of attn_fwd_kernel, the q-normalised-on-load operand mode and
 * attn_iv2_pipe_kernel (operator tests: tests/test_gpu_iv2_attn.py).  Non-causal self attention of B sequences of S tokens, H heads of Dr padded to D = 96 (Dr 72, 80 or
 * 88), the softmax row sum taken from a ones row / column of V.  ONE attention launch (two kernels where the plan splits the rows); no workspace, no qkv_post pass: the
 * pages are EXACTLY what gvl_op_qkv_post mode 1 writes on implicit pages (block_table NULL) with ones_row / k_ones / q_rs.  All pointers are device memory.
 *   qkv      bf16 token rows [B S] of [H Dr | H Dr | H Dr] (q, k, v), ld elements apart (>= 3 H Dr, a multiple of 8; wider is legal), 16-byte aligned.  Forms 1 and 2
 *   Q        bf16 [B][H][S][D], pad columns zero.  Forms 0 and 1
 *   Kt       bf16 [B ceil(S / 64)][H][64][D]: key j of sequence b is slot j % 64 of page b ceil(S / 64) + j / 64; column Dr holds 1.0 (k_ones; form 2 needs it, forms 0
 *            and 1 multiply it by Q's zero pad), the other pad columns 0.  Slots of keys >= S may hold anything
 *   Vt       bf16 [B ceil(S / 64)][H][D][64], row Dr = 1.0 in every slot (ones_row), the other pad rows and the slots of keys >= S finite.  Form 0 only
 *   q_rs     f32 [B S] the row scale of q's RMSNorm, q_nw bf16 [H Dr] its weight (16-byte aligned): the kernel forms q'[d] = bf16(q_nw[h Dr + d] * bf16(q[d] * q_rs[token])
 *            * scale * log2(e)) as it loads q.  Form 2 only
 *   out      bf16 [B S][H Dr], 16-byte aligned
 *   form     0: Q, K and V^T pages;  1: Q and K pages, V read in place from qkv;  2: q read in place from qkv and normalised on load, K pages, V in place (Dr == 88 only)
 *   pipe     form 2 only: 0 attn_fwd_kernel, 1 attn_iv2_pipe_kernel, 2 its safe pass only;  pipe_rows  form 2, pipe != 0: 256 = whole 256-row query blocks on the 8-wave
 *            form and the rest on the 4-wave form, 0 = the 4-wave form for every row.  Neither may change an output bit, except that pipe 1 keeps the first key tile's
 *            row maximum as the softmax reference where pipe 0 / 2 move it once a later tile exceeds it by more than 2^8: there the results agree to rounding only
 *   V range  the output is finite for |v| <= 2^27 / S: the pipelined kernel keeps a row whose sum of probabilities (relative to the first tile's maximum) is below
 *            2^100 and its fp32 accumulators are bounded by that sum times max |v|
 * Returns GVL_ERR_ARG with a message that names this entry, before anything is launched or written, for whatever attn_plan refuses (more than 256 key tiles, a
 * misaligned out / qkv / q_nw, ld % 8 != 0 or ld < 3 H Dr), a NULL pointer the form needs, a non-NULL pointer the form does not take, Dr other than 72 / 80 / 88 (form 2: 88),
 * form, pipe or pipe_rows outside their values.  Synchronises the stream. */
typedef struct {
  const uint16_t* qkv; int32_t ld;
  const uint16_t* Q; const uint16_t* Kt; const uint16_t* Vt;
  const float* q_rs; const uint16_t* q_nw;
  uint16_t* out;
  int32_t B, S, H, Dr;
  float scale;
  int32_t form, pipe, pipe_rows;
} gvl_iv2_attn;
int gvl_op_iv2_attention(gvl_ctx* ctx, const gvl_iv2_attn* p, void* stream);
/* measurement only (tools/decode_bench.py): average microseconds per launch of one decode projection [N,K] x `batch` sequences on
 * synthetic operands; mode 0 = skinny MFMA GEMM (variant 0 = default), 1 = VALU GEMV; `rounds` distinct weight copies are cycled. */
int gvl_op_decode_bench(gvl_ctx* ctx, int N, int K, int batch, int mode, int variant, int rounds, int iters, double* us_per_launch,
                        void* stream);

/* measurement only (tools/mfma_probe.py): a register-only kernel that keeps every matrix pipe 100 % busy with
 * v_mfma_f32_32x32x16_bf16 -- mode 0 zero / 1 constant / 2 random operands -- and reports TFLOP/s and s_memtime ticks per ns of wall
 * time: the ceiling the power envelope leaves a PERFECT bf16 GEMM at a given switching activity.  Needs no ctx. */
int gvl_probe_mfma(int mode, int waves_per_simd, int iters, double* tflops, double* ghz, void* stream);
/* One named do-nothing dispatch (gvl_trace_marker_kernel) on `stream`: brackets a region of a rocprofv3 --kernel-trace (tools/rocpd_stats.py --between). */
int gvl_trace_marker(int tag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GVL_H */
