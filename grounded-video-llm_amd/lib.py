"""ctypes binding of libgvl.so (the C ABI declared in include/gvl.h).

There is NO fallback: if the shared library is missing or cannot be loaded, importing callers get a
RuntimeError telling them to run `python __graft_entry__.py build` (hipcc, gfx950).  PyTorch is only
used by callers for device memory and streams; this module has no torch dependency.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GVL_LIB_PATH") or os.path.join(_HERE, "libgvl.so")   # override: A/B of two builds on one GPU box (tools/)

F32, BF16, I32, I64 = 0, 1, 2, 3
LLM_PHI3, LLM_LLAMA = 0, 1
ACT_NONE, ACT_QUICK_GELU, ACT_GELU, ACT_SILU_MUL = 0, 1, 2, 3
PROF_GEMM, PROF_ATTN, PROF_GEMV, PROF_DECODE_ATTN, PROF_OTHER = 0, 1, 2, 3, 4


class GvlConfig(C.Structure):
    _fields_ = [
        ("llm_kind", C.c_int32),
        ("clip_hidden", C.c_int32), ("clip_inter", C.c_int32), ("clip_layers_run", C.c_int32), ("clip_heads", C.c_int32),
        ("clip_image", C.c_int32), ("clip_patch", C.c_int32),
        ("iv2_dim", C.c_int32), ("iv2_inter", C.c_int32), ("iv2_blocks_run", C.c_int32), ("iv2_heads", C.c_int32),
        ("iv2_image", C.c_int32), ("iv2_patch", C.c_int32), ("iv2_frames_per_seg", C.c_int32),
        ("hidden", C.c_int32), ("inter", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32), ("kv_heads", C.c_int32),
        ("vocab", C.c_int32),
        ("rms_eps", C.c_float),
        ("lm_head_bias", C.c_int32), ("rope_orig_max_pos", C.c_int32), ("max_seq", C.c_int32),
        ("max_segs", C.c_int32), ("kv_pages", C.c_int32), ("max_prefill", C.c_int32), ("decode_fp8", C.c_int32),
    ]


class GvlBiasTable(C.Structure):
    """gvl_bias_table (include/gvl.h): one bias stage of a token rule set, grouped by target token."""
    _fields_ = [("n_targets", C.c_int32), ("targets", C.POINTER(C.c_int32)), ("n_entries", C.c_int32), ("entry_bias", C.POINTER(C.c_float)),
                ("entry_prefix", C.POINTER(C.c_int32)), ("n_prefix", C.c_int32), ("prefix", C.POINTER(C.c_int32))]


class GvlRulesDesc(C.Structure):
    """gvl_rules_desc (include/gvl.h)."""
    _fields_ = [("n_suppress", C.c_int32), ("suppress", C.POINTER(C.c_int32)), ("n_begin_suppress", C.c_int32), ("begin_suppress", C.POINTER(C.c_int32)),
                ("begin_index", C.c_int32), ("n_force", C.c_int32), ("force_ids", C.POINTER(C.c_int32)), ("force_at", C.c_int32), ("bias", GvlBiasTable * 2)]


class GvlGrammarDesc(C.Structure):
    """gvl_grammar_desc (include/gvl.h): a DFA over token classes with one register."""
    _fields_ = [("n_states", C.c_int32), ("n_classes", C.c_int32), ("start", C.c_int32), ("vocab", C.c_int32), ("token_class", C.POINTER(C.c_uint8)),
                ("class_base", C.POINTER(C.c_int32)), ("trans", C.POINTER(C.c_uint16))]


class GvlSampling(C.Structure):
    """gvl_sampling (include/gvl.h): one sampling setting, greedy when do_sample is 0."""
    _fields_ = [("do_sample", C.c_int32), ("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("min_p", C.c_float),
                ("typical_p", C.c_float), ("epsilon_cutoff", C.c_float), ("eta_cutoff", C.c_float), ("seed", C.c_uint64), ("stream", C.c_uint32)]


class GvlBeamParams(C.Structure):
    """gvl_beam_params (include/gvl.h)."""
    _fields_ = [("num_beams", C.c_int), ("max_new_tokens", C.c_int), ("eos_id", C.c_int), ("length_penalty", C.c_double), ("early_stopping", C.c_int),
                ("penalty", C.c_float), ("ngram", C.c_int), ("min_new", C.c_int), ("proc_eos_id", C.c_int), ("rules_id", C.c_int)]


class GvlGroupBeamParams(C.Structure):
    """gvl_group_beam_params (include/gvl.h)."""
    _fields_ = [("base", GvlBeamParams), ("num_beam_groups", C.c_int), ("diversity_penalty", C.c_float), ("pad_id", C.c_int)]


class GvlContrastiveParams(C.Structure):
    """gvl_contrastive_params (include/gvl.h)."""
    _fields_ = [("top_k", C.c_int), ("penalty_alpha", C.c_float), ("max_new_tokens", C.c_int), ("eos_id", C.c_int),
                ("penalty", C.c_float), ("ngram", C.c_int), ("min_new", C.c_int), ("proc_eos_id", C.c_int), ("rules_id", C.c_int)]


class GvlDecodeProj(C.Structure):
    """gvl_decode_proj (include/gvl.h): one decode projection with any prologue / epilogue, for the operator tests."""
    _fields_ = [("path", C.c_int32), ("variant", C.c_int32), ("w_fmt", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("batch", C.c_int32),
                ("W", C.c_void_p), ("x", C.c_void_p), ("x_is_tiled", C.c_int32), ("act", C.c_int32), ("bias", C.c_void_p), ("resid", C.c_void_p),
                ("out_bf16", C.c_void_p), ("out_f32", C.c_void_p), ("out_tiled", C.c_int32), ("out_stride", C.c_int32), ("norm_w", C.c_void_p),
                ("eps", C.c_float), ("sq_n", C.c_int32), ("sq_in", C.c_void_p), ("sq_out", C.c_void_p), ("out_tiled2", C.c_void_p),
                ("rope_on", C.c_int32), ("rope_switch", C.c_int32), ("cos_s", C.c_void_p), ("sin_s", C.c_void_p), ("cos_l", C.c_void_p), ("sin_l", C.c_void_p),
                ("max_pos", C.c_int32), ("n_pages", C.c_int32), ("pos", C.c_void_p), ("tables", C.c_void_p), ("table_stride", C.c_int32), ("q_stride", C.c_int32),
                ("Q", C.c_void_p), ("Kt", C.c_void_p), ("Vt", C.c_void_p), ("H", C.c_int32), ("KV", C.c_int32), ("Dr", C.c_int32), ("D", C.c_int32),
                ("w_deq", C.c_void_p), ("w_scale", C.c_void_p)]


class GvlDecodeAttn(C.Structure):
    """gvl_decode_attn (include/gvl.h): one decode-attention launch on caller-owned tensors, for the operator tests."""
    _fields_ = [("q", C.c_void_p), ("Kt", C.c_void_p), ("Vt", C.c_void_p), ("tables", C.c_void_p), ("pos", C.c_void_p), ("part", C.c_void_p),
                ("counters", C.c_void_p), ("out", C.c_void_p), ("q_stride", C.c_int32), ("n_pages", C.c_int32), ("table_stride", C.c_int32),
                ("out_stride", C.c_int32), ("out_tiled", C.c_int32), ("batch", C.c_int32), ("H", C.c_int32), ("KV", C.c_int32), ("D", C.c_int32),
                ("Dout", C.c_int32), ("nsplit", C.c_int32), ("hpb", C.c_int32), ("cpb", C.c_int32), ("gsplit", C.c_int32), ("scale", C.c_float)]


class GvlQkvPost(C.Structure):
    """gvl_qkv_post (include/gvl.h): one launch of gvl_launch_qkv_post / gvl_launch_qkv_post_ext on caller-owned tensors, for the operator tests."""
    _fields_ = [("qkv", C.c_void_p), ("ld", C.c_int32), ("Q", C.c_void_p), ("Kt", C.c_void_p), ("Vt", C.c_void_p), ("block_table", C.c_void_p), ("max_pages", C.c_int32),
                ("B", C.c_int32), ("S", C.c_int32), ("H", C.c_int32), ("KV", C.c_int32), ("Dr", C.c_int32), ("D", C.c_int32), ("mode", C.c_int32),
                ("qn", C.c_void_p), ("kn", C.c_void_p), ("eps", C.c_float), ("cos", C.c_void_p), ("sin", C.c_void_p), ("pos0", C.c_int32),
                ("ones_row", C.c_int32), ("k_ones", C.c_int32), ("q_rs", C.c_void_p), ("vl_n", C.c_int32), ("vl_rows", C.c_int32 * 9), ("vl_tables", C.c_void_p * 8),
                ("vl_pos0", C.c_int32 * 8), ("table_len", C.c_int32 * 8), ("n_pages", C.c_int32), ("max_pos", C.c_int32), ("ext", C.c_int32)]


class GvlPrefillAttn(C.Structure):
    """gvl_prefill_attn (include/gvl.h): one paged prefill-attention launch (block table with qpos0 / Sk, ragged, ragged-extend) on caller-owned pages."""
    _fields_ = [("Q", C.c_void_p), ("Kt", C.c_void_p), ("Vt", C.c_void_p), ("O", C.c_void_p), ("block_table", C.c_void_p), ("max_pages", C.c_int32),
                ("B", C.c_int32), ("H", C.c_int32), ("KV", C.c_int32), ("S", C.c_int32), ("D", C.c_int32), ("Dout", C.c_int32), ("Sk", C.c_int32), ("qpos0", C.c_int32),
                ("scale", C.c_float), ("causal", C.c_int32), ("ring", C.c_int32), ("vl_n", C.c_int32), ("vl_rows", C.c_int32 * 9), ("vl_tables", C.c_void_p * 8),
                ("vl_pos0", C.c_int32 * 8), ("table_len", C.c_int32 * 8), ("ext", C.c_int32), ("n_pages", C.c_int32)]


class GvlIv2Attn(C.Structure):
    """gvl_iv2_attn (include/gvl.h): the attention launch of one InternVideo2 block (ONES forms, q normalised on load, attn_iv2_pipe_kernel) on caller-owned buffers."""
    _fields_ = [("qkv", C.c_void_p), ("ld", C.c_int32), ("Q", C.c_void_p), ("Kt", C.c_void_p), ("Vt", C.c_void_p), ("q_rs", C.c_void_p), ("q_nw", C.c_void_p),
                ("out", C.c_void_p), ("B", C.c_int32), ("S", C.c_int32), ("H", C.c_int32), ("Dr", C.c_int32), ("scale", C.c_float), ("form", C.c_int32),
                ("pipe", C.c_int32), ("pipe_rows", C.c_int32)]


class GvlPatchEmbed(C.Structure):
    """gvl_patch_embed (include/gvl.h): the patch embedding of either vision tower by either path, for the operator tests."""
    _fields_ = [("mode", C.c_int32), ("path", C.c_int32), ("n", C.c_int32), ("T", C.c_int32), ("image", C.c_int32), ("patch", C.c_int32), ("C", C.c_int32),
                ("Kp", C.c_int32), ("eps", C.c_float), ("px", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("cls", C.c_void_p), ("pos", C.c_void_p),
                ("lnw", C.c_void_p), ("lnb", C.c_void_p), ("out", C.c_void_p), ("im2col", C.c_void_p)]


_SIGS = {
    # name: (restype, argtypes)
    "gvl_create": (C.c_int, [C.POINTER(GvlConfig), C.POINTER(C.c_void_p)]),
    "gvl_destroy": (C.c_int, [C.c_void_p]),
    "gvl_last_error": (C.c_char_p, [C.c_void_p]),
    "gvl_device_info": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_int)]),
    "gvl_load_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int, C.c_int]),
    "gvl_finalize_weights": (C.c_int, [C.c_void_p]),
    "gvl_load_packed": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]),
    "gvl_kv_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "gvl_debug_seq_pages": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int)]),
    "gvl_comm_unique_id": (C.c_int, [C.c_char_p]),
    "gvl_comm_init": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int]),
    "gvl_comm_destroy": (C.c_int, [C.c_void_p]),
    "gvl_decode_group_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gvl_comm_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "gvl_allgather_visual": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "gvl_allgatherv_visual": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p]),
    "gvl_clip_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gvl_iv2_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gvl_build_visual": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gvl_tokens_per_seg": (C.c_int, [C.c_void_p]),
    "gvl_encode_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gvl_splice": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "gvl_seq_alloc": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "gvl_seq_free": (C.c_int, [C.c_void_p, C.c_int]),
    "gvl_seq_fork": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "gvl_seq_clone": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p]),
    "gvl_seq_fanout": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "gvl_prefill_extend": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gvl_prefill": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gvl_decode_greedy": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int), C.c_void_p]),
    "gvl_preprocess_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
    "gvl_prefill_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_void_p]),
    "gvl_decode_steps": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p]),
    "gvl_seq_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int), C.c_void_p]),
    "gvl_forward_loss": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p]),
    "gvl_prefill_varlen": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p]),
    "gvl_prefill_extend_varlen": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p, C.c_void_p]),
    "gvl_score_extend_varlen": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.POINTER(C.c_int32)), C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]),
    "gvl_decode_greedy_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int), C.c_void_p]),
    "gvl_decode_step_logits": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "gvl_decode_step_logits_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    "gvl_prof_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "gvl_prof_read": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "gvl_op_gemm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "gvl_op_gemm_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "gvl_op_gemm_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "gvl_op_patch_embed": (C.c_int, [C.c_void_p, C.POINTER(GvlPatchEmbed), C.c_void_p]),
    "gvl_op_patchify": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "gvl_op_hd_merge": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "gvl_op_pool_spatial": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "gvl_op_pool_temporal": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "gvl_op_strip_cls": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "gvl_op_bcast_row": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "gvl_op_fold_gamma": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "gvl_op_rowsq_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "gvl_op_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_float, C.c_int, C.c_void_p]),
    "gvl_op_layernorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "gvl_op_rmsnorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "gvl_debug_set": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "gvl_set_sampling": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_uint64]),
    "gvl_set_sampling_ex": (C.c_int, [C.c_void_p, C.POINTER(GvlSampling)]),
    "gvl_seq_set_sampling": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(GvlSampling)]),
    "gvl_op_select_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(GvlSampling), C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gvl_op_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gvl_set_logits_processors": (C.c_int, [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int]),
    "gvl_seq_set_processors": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int]),
    "gvl_op_logits_process": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float),
                                        C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]),
    "gvl_rules_create": (C.c_int, [C.c_void_p, C.POINTER(GvlRulesDesc), C.POINTER(C.c_int)]),
    "gvl_rules_destroy": (C.c_int, [C.c_void_p, C.c_int]),
    "gvl_set_token_rules": (C.c_int, [C.c_void_p, C.c_int]),
    "gvl_seq_set_token_rules": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "gvl_op_logits_process_rules": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float),
                                              C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]),
    "gvl_grammar_create": (C.c_int, [C.c_void_p, C.POINTER(GvlGrammarDesc), C.POINTER(C.c_int)]),
    "gvl_grammar_destroy": (C.c_int, [C.c_void_p, C.c_int]),
    "gvl_set_grammar": (C.c_int, [C.c_void_p, C.c_int]),
    "gvl_seq_set_grammar": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "gvl_op_logits_process_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float),
                                           C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]),
    "gvl_seq_set_guidance": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gvl_op_guidance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_float), C.c_void_p]),
    "gvl_set_logprobs": (C.c_int, [C.c_void_p, C.c_int]),
    "gvl_seq_set_logprobs": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "gvl_seq_read_logprobs": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "gvl_op_select_logprobs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_uint64, C.c_void_p,
                                         C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gvl_op_score_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gvl_op_dgemm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "gvl_op_decode_proj": (C.c_int, [C.c_void_p, C.POINTER(GvlDecodeProj), C.c_void_p]),
    "gvl_op_decode_attention": (C.c_int, [C.c_void_p, C.POINTER(GvlDecodeAttn), C.c_void_p]),
    "gvl_op_qkv_post": (C.c_int, [C.c_void_p, C.POINTER(GvlQkvPost), C.c_void_p]),
    "gvl_op_prefill_attention": (C.c_int, [C.c_void_p, C.POINTER(GvlPrefillAttn), C.c_void_p]),
    "gvl_op_iv2_attention": (C.c_int, [C.c_void_p, C.POINTER(GvlIv2Attn), C.c_void_p]),
    "gvl_op_decode_bench": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p]),
    "gvl_probe_mfma": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p]),
    "gvl_trace_marker": (C.c_int, [C.c_int, C.c_void_p]),
    "gvl_beam_search": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(GvlBeamParams), C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                  C.POINTER(C.c_float), C.c_void_p]),
    "gvl_beam_search_n": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(GvlBeamParams), C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                    C.POINTER(C.c_float), C.c_void_p]),
    "gvl_op_beam_candidates": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gvl_op_beam_normalize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "gvl_group_beam_search": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(GvlGroupBeamParams), C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int),
                                        C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_void_p]),
    "gvl_debug_group_beam_tokens": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int)]),
    "gvl_debug_group_beam_pool": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int)]),
    "gvl_op_beam_group": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "gvl_op_logits_process_hamming": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float),
                                                C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                C.c_void_p, C.c_int, C.c_float, C.c_void_p]),
    "gvl_op_gemv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "gvl_seq_keep_hidden": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "gvl_seq_read_hidden": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gvl_contrastive_search": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(GvlContrastiveParams), C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p]),
    "gvl_op_hidden_bank_append": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "gvl_op_contrastive_rank": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}
EXPORTS = tuple(_SIGS)

_lib = None


def load():
    """dlopen libgvl.so and bind every symbol of include/gvl.h.  Raises RuntimeError when absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU / PyTorch fallback exists). "
            "Build it with `python __graft_entry__.py build` (hipcc --offload-arch=gfx950).")
    try:
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover
        raise RuntimeError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)   # AttributeError if the .so is stale
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


ERR_ARG, ERR_STATE, ERR_HIP, ERR_OOM, ERR_NOGPU = -1, -2, -3, -4, -5   # include/gvl.h gvl_status


class GvlError(RuntimeError):
    status = 0


def check(lib, ctx, rc, what=""):
    if rc != 0:
        msg = lib.gvl_last_error(ctx)
        err = GvlError(f"{what} failed (status {rc}): {msg.decode() if msg else ''}")
        err.status = rc
        raise err
