"""Engine: one gvl_ctx on one GPU, with torch tensors as the caller-owned I/O buffers.

PyTorch here is plumbing only (device allocations, the current HIP stream); all arithmetic runs
inside libgvl.so.  If the library cannot be loaded this module raises -- there is no eager fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as L
from . import logits as LP
from . import logprobs as LPR

bf = torch.bfloat16


@dataclass
class TowerGeometry:
    """Mirrors gvl_config (include/gvl.h).  Defaults = the reference's Phi-3.5 / 96-frame configuration
    (models/llava_next_video.py:56-71, models/internvideo2.py:1089-1114, HF Phi-3.5 config [ext])."""
    llm: str = "phi3.5"                      # 'phi3.5' | 'llama3' | 'vicuna'
    clip_hidden: int = 1024
    clip_inter: int = 4096
    clip_layers: int = 24                    # layers in the checkpoint; layers-1 are executed (hidden_states[-2])
    clip_heads: int = 16
    clip_image: int = 336
    clip_patch: int = 14
    iv2_dim: int = 1408
    iv2_inter: int = 6144
    iv2_depth: int = 40                      # blocks in the checkpoint; depth-1 are executed (x_vis_return_idx=-2)
    iv2_heads: int = 16
    iv2_image: int = 224
    iv2_patch: int = 14
    frames_per_seg: int = 8
    hidden: int = 3072
    inter: int = 8192
    layers: int = 32
    heads: int = 32
    kv_heads: int = 32
    vocab: int = 32366                       # 32064 + 302 temporal tokens (llava_next_video.py:235-268)
    rms_eps: float = 1e-5
    lm_head_bias: bool = True
    rope_theta: float = 10000.0
    rope_short: Optional[Sequence[float]] = None
    rope_long: Optional[Sequence[float]] = None
    rope_max_pos: int = 131072
    rope_orig_max_pos: int = 4096
    max_seq: int = 8192
    max_segs: int = 12
    kv_pages: int = 128
    max_prefill: int = 4096
    decode_fp8: int = 0                      # quantised weight variant of the LLM (opt-in, not the reference's numerics): 1 / True = FP8 e4m3 with per-row
                                             # power-of-two scales, 2 = MXFP4 (E2M1 elements, E8M0 scale per 32 k); 0 = bf16

    @property
    def kind(self) -> str:
        return "phi3" if self.llm == "phi3.5" else "llama"

    @staticmethod
    def vicuna_7b(**kw) -> "TowerGeometry":
        """LLaVA-Next vicuna-7b-v1.5 base [ext]: Llama-2 architecture -- MHA 32 x 128, inter 11008, theta 1e4, vocab 32000 + 302."""
        base = dict(llm="vicuna", hidden=4096, inter=11008, layers=32, heads=32, kv_heads=32, vocab=32000 + 302, rope_theta=10000.0,
                    rope_short=None, rope_long=None, rope_orig_max_pos=0, max_seq=4096)
        base.update(kw)
        return TowerGeometry(**base)

    def apply_hf_config(self, cfg: dict) -> "TowerGeometry":
        """Fill the LLM fields from an HF config.json dict (the `text`/top-level keys of Phi-3.5(-vision) / Llama configs [ext]):
        hidden sizes, rms_norm_eps, rope_theta and -- for Phi-3.5 -- the LongRoPE short/long factors and both context limits that
        Phi3LongRoPEScaledRotaryEmbedding reads (models/modeling_phi3.py:369-409).  Returns self."""
        cfg = cfg.get("text_config", cfg)
        m = {"hidden_size": "hidden", "intermediate_size": "inter", "num_hidden_layers": "layers", "num_attention_heads": "heads",
             "num_key_value_heads": "kv_heads", "rms_norm_eps": "rms_eps", "rope_theta": "rope_theta"}
        for k, a in m.items():
            if cfg.get(k) is not None:
                setattr(self, a, type(getattr(self, a))(cfg[k]))
        rs = cfg.get("rope_scaling")
        if rs:
            kind = rs.get("type", rs.get("rope_type"))
            # Phi3Config._rope_scaling_adjustment renames the legacy types "su" / "yarn" to "longrope" (modeling_phi3.py:191-202)
            if kind not in ("longrope", "su", "yarn") or "short_factor" not in rs or "long_factor" not in rs:
                raise ValueError(f"unsupported rope_scaling {rs!r}: need type longrope with short_factor and long_factor (modeling_phi3.py:204-240)")
            self.rope_short, self.rope_long = [float(v) for v in rs["short_factor"]], [float(v) for v in rs["long_factor"]]
            self.rope_max_pos = int(cfg.get("max_position_embeddings", self.rope_max_pos))
            self.rope_orig_max_pos = int(cfg.get("original_max_position_embeddings", self.rope_orig_max_pos))
        return self

    @staticmethod
    def llama3_8b(**kw) -> "TowerGeometry":
        base = dict(llm="llama3", hidden=4096, inter=14336, layers=32, heads=32, kv_heads=8, vocab=128558, rope_theta=500000.0,
                    rope_short=None, rope_long=None, rope_orig_max_pos=0, max_seq=8192)
        base.update(kw)
        return TowerGeometry(**base)


def _on(v) -> bool:
    """A warper argument that switches its warper on (None / 0 = off)."""
    return v is not None and float(v) != 0.0


def sampling_struct(do_sample=True, temperature=1.0, top_k=50, top_p=None, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None, seed=0,
                    stream=0) -> "L.GvlSampling":
    """One gvl_sampling (include/gvl.h) from generate()-style arguments: None = off; top_k 50 is HF's GenerationConfig default; typical_p 1.0 (HF's off) = 0."""
    f = lambda v: 0.0 if v is None else float(v)
    tp = f(typical_p)
    return L.GvlSampling(int(bool(do_sample)), float(temperature), int(top_k or 0), f(top_p), f(min_p), 0.0 if tp == 1.0 else tp, f(epsilon_cutoff),
                         f(eta_cutoff), int(seed) & (2 ** 64 - 1), int(stream) & 0xffffffff)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


class Engine:
    def __init__(self, geo: TowerGeometry, device: str = "cuda:0", towers: Sequence[str] = ("clip", "iv2", "llm")):
        self.lib = L.load()
        self.geo = geo
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("grounded_video_llm_amd.Engine needs a HIP device (cuda:N); there is no CPU path")
        torch.cuda.set_device(self.device)
        cfg = L.GvlConfig()
        cfg.llm_kind = L.LLM_PHI3 if geo.kind == "phi3" else L.LLM_LLAMA
        if "clip" in towers:
            cfg.clip_hidden, cfg.clip_inter, cfg.clip_layers_run = geo.clip_hidden, geo.clip_inter, geo.clip_layers - 1
            cfg.clip_heads, cfg.clip_image, cfg.clip_patch = geo.clip_heads, geo.clip_image, geo.clip_patch
        if "iv2" in towers:
            cfg.iv2_dim, cfg.iv2_inter, cfg.iv2_blocks_run = geo.iv2_dim, geo.iv2_inter, geo.iv2_depth - 1
            cfg.iv2_heads, cfg.iv2_image, cfg.iv2_patch, cfg.iv2_frames_per_seg = geo.iv2_heads, geo.iv2_image, geo.iv2_patch, geo.frames_per_seg
        cfg.hidden = geo.hidden if ("llm" in towers or "proj" in towers) else 0
        if "llm" in towers:
            cfg.inter, cfg.layers, cfg.heads, cfg.kv_heads, cfg.vocab = geo.inter, geo.layers, geo.heads, geo.kv_heads, geo.vocab
            cfg.rms_eps = geo.rms_eps
            cfg.lm_head_bias = 1 if geo.lm_head_bias else 0
            cfg.rope_orig_max_pos = geo.rope_orig_max_pos if geo.rope_long is not None else 0
            cfg.max_seq = geo.max_seq
            cfg.kv_pages, cfg.max_prefill = geo.kv_pages, geo.max_prefill
            cfg.decode_fp8 = int(geo.decode_fp8)
        cfg.max_segs = geo.max_segs
        self.cfg = cfg
        self.towers = tuple(towers)
        h = C.c_void_p()
        rc = self.lib.gvl_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise L.GvlError(f"gvl_create failed ({rc}): {self.lib.gvl_last_error(None).decode()}")
        self.ctx = h
        self._finalized = False

    # ---- lifecycle -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "ctx", None):
            self.lib.gvl_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        L.check(self.lib, self.ctx, rc, what)

    @property
    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- weights ---------------------------------------------------------------------------------
    def load_packed(self, packed: Dict[str, torch.Tensor]):
        for name, t in packed.items():
            if t.dtype == torch.float32:
                dt = L.F32
            elif t.dtype == bf:
                dt = L.BF16
            else:
                raise TypeError(f"{name}: packed tensors must be float32 or bfloat16, got {t.dtype}")
            t = t.contiguous()
            shape = (C.c_int64 * max(t.dim(), 1))(*(list(t.shape) or [1]))
            self._chk(self.lib.gvl_load_weight(self.ctx, name.encode(), C.c_void_p(t.data_ptr()), dt, shape, max(t.dim(), 1),
                                               1 if t.is_cuda else 0), f"gvl_load_weight({name})")

    def load_packed_file(self, path: str) -> int:
        """gvl_load_packed: the C++ loader of a `gvl-packed-1` file (tools/pack_checkpoint.py); no torch / safetensors involved."""
        n = C.c_int(0)
        self._chk(self.lib.gvl_load_packed(self.ctx, os.fsencode(path), C.byref(n)), "gvl_load_packed")
        return n.value

    def finalize(self):
        self._chk(self.lib.gvl_finalize_weights(self.ctx), "gvl_finalize_weights")
        self._finalized = True

    def kv_info(self) -> Dict[str, int]:
        t, f, b, m = C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int(0)
        self._chk(self.lib.gvl_kv_info(self.ctx, C.byref(t), C.byref(f), C.byref(b), C.byref(m)), "gvl_kv_info")
        return {"total_pages": t.value, "free_pages": f.value, "pool_bytes": b.value, "max_live_seqs": m.value, "tokens": t.value * 64}

    def seq_pages(self, seq: int) -> List[int]:
        """gvl_debug_seq_pages (tests): the KV pages of a live sequence in position order.  Host-only: no device call."""
        n = C.c_int(0)
        self._chk(self.lib.gvl_debug_seq_pages(self.ctx, int(seq), None, 0, C.byref(n)), "gvl_debug_seq_pages")
        buf = (C.c_int32 * max(n.value, 1))()
        self._chk(self.lib.gvl_debug_seq_pages(self.ctx, int(seq), buf, n.value, C.byref(n)), "gvl_debug_seq_pages")
        return [int(buf[i]) for i in range(n.value)]

    def decode_group_info(self) -> Dict[str, int]:
        """gvl_decode_group_info: the group sizes one batched decode step takes ({max_group: 16, any_size: 1} on the skinny-MFMA path;
        {4, 0} = sizes 1 / 2 / 4 on the VALU fallback)."""
        m, a = C.c_int(0), C.c_int(0)
        self._chk(self.lib.gvl_decode_group_info(self.ctx, C.byref(m), C.byref(a)), "gvl_decode_group_info")
        return {"max_group": m.value, "any_size": a.value}

    # ---- multi-GPU exchange through the C ABI (RCCL dlopen'ed by libgvl) -----------------------------
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        rc = self.lib.gvl_comm_unique_id(buf)
        if rc != 0:
            raise L.GvlError(f"gvl_comm_unique_id failed ({rc}): {self.lib.gvl_last_error(None).decode()}")
        return buf.raw

    def comm_init(self, uid: bytes, rank: int, world: int):
        assert len(uid) == 128
        self._chk(self.lib.gvl_comm_init(self.ctx, uid, int(rank), int(world)), "gvl_comm_init")
        self.comm_world = world

    def comm_count(self) -> int:
        """Ranks RCCL itself reports for the ctx's communicator (ncclCommCount); 1 without a communicator."""
        n = C.c_int(0)
        self._chk(self.lib.gvl_comm_count(self.ctx, C.byref(n)), "gvl_comm_count")
        return n.value

    def allgather_visual(self, local: torch.Tensor) -> torch.Tensor:
        """local bf16 [rows, hidden] (same rows on every rank) -> [world * rows, hidden] in rank order (ncclAllGather on the current stream)."""
        local = local.contiguous()
        world = getattr(self, "comm_world", 1)
        out = torch.empty((world * local.shape[0], local.shape[1]), dtype=bf, device=self.device)
        self._chk(self.lib.gvl_allgather_visual(self.ctx, None, _ptr(local), local.shape[0], local.shape[1], _ptr(out), self.stream), "gvl_allgather_visual")
        return out

    def allgatherv_visual(self, local: torch.Tensor, rows_per_rank, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Uneven blocks straight into the segment-ordered prefix: rank r's `rows_per_rank[r]` rows land at row offset sum(rows_per_rank[:r]) of the result on
        every rank (gvl_allgatherv_visual: one ncclGroup of per-rank broadcasts on the current stream; no padding, no re-assembly copy).  `out`: a
        preallocated [sum(rows), hidden] bf16 buffer (the step's prefix) to gather into."""
        local = local.contiguous()
        rows = [int(r) for r in rows_per_rank]
        hidden = local.shape[1]
        if out is None:
            out = torch.empty((sum(rows), hidden), dtype=bf, device=self.device)
        assert out.is_contiguous() and out.shape == (sum(rows), hidden) and out.dtype == bf
        arr = (C.c_int * len(rows))(*rows)
        self._chk(self.lib.gvl_allgatherv_visual(self.ctx, None, _ptr(local) if local.numel() else None, arr, hidden, _ptr(out), self.stream), "gvl_allgatherv_visual")
        return out

    # ---- vision ----------------------------------------------------------------------------------
    def clip_encode(self, px: torch.Tensor) -> torch.Tensor:
        """vision_tower(px, output_hidden_states=True).hidden_states[-2][:, 1:] (llava_next_video.py:504-505)."""
        px = px.to(self.device, torch.float32).contiguous()
        n = px.shape[0]
        P = (self.geo.clip_image // self.geo.clip_patch) ** 2
        out = torch.empty((n, P, self.geo.clip_hidden), dtype=torch.float32, device=self.device)
        self._chk(self.lib.gvl_clip_encode(self.ctx, _ptr(px), n, _ptr(out), self.stream), "gvl_clip_encode")
        return out

    def iv2_encode(self, px: torch.Tensor) -> torch.Tensor:
        """video_encoder(x, None, False, x_vis_return_idx=-2, x_vis_only=True)[:, 1:, :] (llava_next_video.py:532).
        px [n,3,T,H,W]."""
        px = px.to(self.device, torch.float32).contiguous()
        n, T = px.shape[0], px.shape[2]
        assert T == self.geo.frames_per_seg
        Lp = (self.geo.iv2_image // self.geo.iv2_patch) ** 2
        out = torch.empty((n, T * Lp, self.geo.iv2_dim), dtype=bf, device=self.device)
        self._chk(self.lib.gvl_iv2_encode(self.ctx, _ptr(px), n, _ptr(out), self.stream), "gvl_iv2_encode")
        return out

    @property
    def tokens_per_seg(self) -> int:
        return int(self.lib.gvl_tokens_per_seg(self.ctx))

    def build_visual(self, clip_feats: torch.Tensor, iv2_feats: torch.Tensor) -> torch.Tensor:
        n = clip_feats.shape[0]
        out = torch.empty((n * self.tokens_per_seg, self.geo.hidden), dtype=bf, device=self.device)
        self._chk(self.lib.gvl_build_visual(self.ctx, _ptr(clip_feats.contiguous()), _ptr(iv2_feats.contiguous()), n, _ptr(out), self.stream),
                  "gvl_build_visual")
        return out

    def encode_segments(self, spatial_px: torch.Tensor, temporal_px: torch.Tensor) -> torch.Tensor:
        """encode_images() for n segments: spatial [n,3,336,336], temporal [n,3,T,224,224] -> [n*L, hidden] bf16."""
        sp = spatial_px.to(self.device, torch.float32).contiguous()
        tp = temporal_px.to(self.device, torch.float32).contiguous()
        n = sp.shape[0]
        out = torch.empty((n * self.tokens_per_seg, self.geo.hidden), dtype=bf, device=self.device)
        self._chk(self.lib.gvl_encode_segments(self.ctx, _ptr(sp), _ptr(tp), n, _ptr(out), self.stream), "gvl_encode_segments")
        return out

    def preprocess_frames(self, frames_u8: torch.Tensor, size: int, mean, std) -> torch.Tensor:
        """frame_transform of the reference on the GPU (bit-exact to PIL bicubic + torchvision glue): uint8 frames [n,H,W,3]
        (decoder order) or [n,3,H,W] -> f32 [n,3,size,size].  mm_utils/utils.py:153-183."""
        assert frames_u8.dtype == torch.uint8 and frames_u8.dim() == 4
        if frames_u8.shape[-1] == 3 and frames_u8.shape[1] != 3:
            layout, (n, H, W) = 0, (frames_u8.shape[0], frames_u8.shape[1], frames_u8.shape[2])
        else:
            layout, (n, H, W) = 1, (frames_u8.shape[0], frames_u8.shape[2], frames_u8.shape[3])
        fr = frames_u8.to(self.device).contiguous()
        out = torch.empty((n, 3, size, size), dtype=torch.float32, device=self.device)
        m = (C.c_float * 3)(*[float(v) for v in mean]); s = (C.c_float * 3)(*[float(v) for v in std])
        self._chk(self.lib.gvl_preprocess_frames(self.ctx, _ptr(fr), n, H, W, layout, int(size), m, s, _ptr(out), self.stream), "gvl_preprocess_frames")
        return out

    # ---- LLM -------------------------------------------------------------------------------------
    def splice(self, input_ids: Sequence[int], visual: torch.Tensor) -> torch.Tensor:
        ids = (C.c_int64 * len(input_ids))(*[int(i) for i in input_ids])
        nv = visual.shape[0]
        out = torch.empty((len(input_ids) - 1 + nv, self.geo.hidden), dtype=bf, device=self.device)
        S = C.c_int(0)
        self._chk(self.lib.gvl_splice(self.ctx, ids, len(input_ids), _ptr(visual.contiguous()), nv, _ptr(out), C.byref(S), self.stream), "gvl_splice")
        assert S.value == out.shape[0]
        return out

    def embed_ids(self, input_ids: Sequence[int]) -> torch.Tensor:
        """The embedding rows of plain token ids [len, hidden] -- a text-only prompt (no image slot): gvl_splice with the slot behind the last id and no visual rows."""
        if len(input_ids) == 0 or any(int(i) < 0 for i in input_ids):
            raise ValueError("embed_ids: a non-empty list of token ids >= 0 (no image slot)")
        return self.splice(list(input_ids) + [-200], torch.empty((0, self.geo.hidden), dtype=bf, device=self.device))

    def seq_alloc(self, max_tokens: int) -> int:
        s = C.c_int(-1)
        self._chk(self.lib.gvl_seq_alloc(self.ctx, int(max_tokens), C.byref(s)), "gvl_seq_alloc")
        return s.value

    def seq_free(self, seq: int):
        self._chk(self.lib.gvl_seq_free(self.ctx, int(seq)), "gvl_seq_free")

    def seq_fork(self, src: int, n_tokens: int, max_tokens: int) -> int:
        """A new sequence that SHARES the first n_tokens (multiple of 64) of `src` -- whole KV pages, referenced not copied (gvl_seq_fork)."""
        sid = C.c_int(-1)
        self._chk(self.lib.gvl_seq_fork(self.ctx, int(src), int(n_tokens), int(max_tokens), C.byref(sid)), "gvl_seq_fork")
        return sid.value

    def seq_clone(self, src: int, max_tokens: int) -> int:
        """A copy of `src` at its current length: whole pages shared by reference, the partial last page copied (gvl_seq_clone; beam search).
        Its generated ids (seq_read) start empty; a clone of a sequence WITH a grammar takes the source's generated ids along and continues its answer."""
        sid = C.c_int(-1)
        self._chk(self.lib.gvl_seq_clone(self.ctx, int(src), int(max_tokens), C.byref(sid), self.stream), "gvl_seq_clone")
        return sid.value

    def seq_fanout(self, seq: int, n_new: int, max_tokens: int, streams: Sequence[int], first_logits: torch.Tensor) -> List[int]:
        """n_new siblings of the freshly prefilled `seq` (gvl_seq_fanout): n answers to one prompt from ONE prefill.  first_logits: that prefill's logits
        (prefill(..., want_logits=True)); streams: the random stream of every sibling.  A sibling shares the prompt's whole KV pages, copies the source's settings with the
        source's effective sampling as its own on stream streams[i], and holds its own first token, drawn from first_logits: decode source and siblings together.
        All or nothing: a refusal (GvlError) leaves every sequence and the pool as they were."""
        n_new = int(n_new)
        if len(streams) != n_new:
            raise ValueError("seq_fanout: one stream per sibling")
        assert first_logits.dtype == torch.float32 and first_logits.is_contiguous() and first_logits.numel() == self.geo.vocab and first_logits.device == self.device
        st = (C.c_uint32 * max(n_new, 1))(*[int(x) & 0xFFFFFFFF for x in streams])
        out = (C.c_int * max(n_new, 1))()
        self._chk(self.lib.gvl_seq_fanout(self.ctx, int(seq), n_new, int(max_tokens), st, _ptr(first_logits), out, self.stream), "gvl_seq_fanout")
        return [int(out[i]) for i in range(n_new)]

    def prefill_extend(self, seq: int, embeds_new: torch.Tensor, want_logits: bool = False) -> Optional[torch.Tensor]:
        """Prefill of the rows that FOLLOW a forked prefix (gvl_prefill_extend): positions prefix .. prefix + n - 1, attention over prefix + new rows."""
        embeds_new = embeds_new.contiguous()
        assert embeds_new.dtype == bf and embeds_new.dim() == 2
        lg = torch.empty((self.geo.vocab,), dtype=torch.float32, device=self.device) if want_logits else None
        self._chk(self.lib.gvl_prefill_extend(self.ctx, int(seq), _ptr(embeds_new), embeds_new.shape[0], _ptr(lg), self.stream), "gvl_prefill_extend")
        return lg

    def prefill_extend_batch(self, seqs: Sequence[int], embeds_new: Sequence[torch.Tensor], want_logits: bool = False) -> Optional[torch.Tensor]:
        """Ragged prefill where every sequence sits behind its own cached prefix (gvl_prefill_extend_varlen): each holds a multiple of 64 tokens (0 = empty) and gets
        its own new rows; one decoder pass per group of up to 8.  Every member ends exactly as after its own prefill_extend / prefill.  -> [n][vocab] logits if asked."""
        es = [e.contiguous() for e in embeds_new]
        assert all(e.dtype == bf and e.dim() == 2 for e in es) and len(es) == len(seqs)
        n = len(seqs)
        ids = (C.c_int * n)(*[int(s) for s in seqs])
        ptrs = (C.c_void_p * n)(*[e.data_ptr() for e in es])
        lens = (C.c_int * n)(*[int(e.shape[0]) for e in es])
        lg = torch.empty((n, self.geo.vocab), dtype=torch.float32, device=self.device) if want_logits else None
        self._chk(self.lib.gvl_prefill_extend_varlen(self.ctx, ids, n, ptrs, lens, _ptr(lg), self.stream), "gvl_prefill_extend_varlen")
        return lg

    def score_extend_batch(self, seqs: Sequence[int], embeds_new: Sequence[torch.Tensor], next_ids: Sequence[Sequence[int]], top_n: int = 0, want_logits: bool = False):
        """prefill_extend_batch that also scores given ids (gvl_score_extend_varlen): next_ids[i][r] is the id that new row r of member i must predict (the token fed at
        r + 1), -100 = not scored.  -> (lp f32 [n], rank int32 [n], top_ids int32 [n, 8] | None, top_lp f32 [n, 8] | None) on the device, packed: members in call
        order, scored rows in row order (top lists with top_n 1 .. 8 only); with want_logits also the members' last-row logits [len(seqs), vocab].  Asynchronous.
        Every member ends as after prefill_extend_batch of the same rows."""
        es = [e.contiguous() for e in embeds_new]
        assert all(e.dtype == bf and e.dim() == 2 for e in es) and len(es) == len(seqs) == len(next_ids)
        assert all(len(t) == e.shape[0] for t, e in zip(next_ids, es)), "next_ids must cover every new row"
        n = len(seqs)
        ids = (C.c_int * n)(*[int(s) for s in seqs])
        ptrs = (C.c_void_p * n)(*[e.data_ptr() for e in es])
        lens = (C.c_int * n)(*[int(e.shape[0]) for e in es])
        tg = [(C.c_int32 * max(len(t), 1))(*[int(v) for v in t]) for t in next_ids]
        tgp = (C.POINTER(C.c_int32) * n)(*[C.cast(t, C.POINTER(C.c_int32)) for t in tg])
        ns = sum(1 for t in next_ids for v in t if int(v) != -100)
        cap = max(ns, 1)                                    # (an empty tensor has no address to hand over)
        lp = torch.empty((cap,), dtype=torch.float32, device=self.device)[:ns]
        rank = torch.empty((cap,), dtype=torch.int32, device=self.device)[:ns]
        ti = torch.empty((cap, LPR.MAX_TOP), dtype=torch.int32, device=self.device)[:ns] if top_n else None
        tv = torch.empty((cap, LPR.MAX_TOP), dtype=torch.float32, device=self.device)[:ns] if top_n else None
        lg = torch.empty((n, self.geo.vocab), dtype=torch.float32, device=self.device) if want_logits else None
        got = C.c_int(-1)
        self._chk(self.lib.gvl_score_extend_varlen(self.ctx, ids, n, ptrs, lens, tgp, int(top_n), _ptr(lp), _ptr(rank), _ptr(ti), _ptr(tv), C.byref(got), _ptr(lg),
                                                   self.stream), "gvl_score_extend_varlen")
        assert got.value == ns
        return (lp, rank, ti, tv, lg) if want_logits else (lp, rank, ti, tv)

    def op_score_rows(self, logits: torch.Tensor, targets, top_n: int = 0, out=None):
        """gvl_op_score_rows on fp32 rows [R, n] (any R; the row stride is taken from the tensor): (lp f32 [R], rank int32 [R], top_ids int32 [R, 8], top_lp f32 [R, 8]) on
        the device.  targets: a host sequence -- one outside [0, n) raises ValueError before anything runs -- or an int32 device tensor, taken as it is (the kernel scores
        such a target lp = -inf, rank = -1 and never indexes its row).  out: the four output tensors to write into (default: fresh ones filled with NaN / -2; what a call
        does not produce keeps its fill -- with top_n = 0 both lists)."""
        assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.device.type == "cuda"
        R, n = logits.shape
        if isinstance(targets, torch.Tensor) and targets.device.type == "cuda":
            tg = targets.to(torch.int32).contiguous()
        else:
            tl = [int(t) for t in targets]
            if any(t < 0 or t >= n for t in tl):
                raise ValueError(f"op_score_rows: a target outside [0, {n})")
            tg = torch.tensor(tl, dtype=torch.int32, device=self.device)
        assert tg.shape == (R,)
        if out is None:
            out = (torch.full((R,), float("nan"), dtype=torch.float32, device=self.device), torch.full((R,), -2, dtype=torch.int32, device=self.device),
                   torch.full((R, LPR.MAX_TOP), -2, dtype=torch.int32, device=self.device), torch.full((R, LPR.MAX_TOP), float("nan"), dtype=torch.float32, device=self.device))
        lp, rank, ti, tv = out
        self._chk(self.lib.gvl_op_score_rows(self.ctx, _ptr(logits), n, int(logits.stride(0)) if R > 1 else n, R, _ptr(tg), int(top_n), _ptr(lp), _ptr(rank), _ptr(ti), _ptr(tv),
                                             self.stream), "gvl_op_score_rows")
        return lp, rank, ti, tv

    def prefill(self, seq: int, embeds: torch.Tensor, want_logits: bool = False) -> Optional[torch.Tensor]:
        embeds = embeds.contiguous()
        logits = torch.empty((self.geo.vocab,), dtype=torch.float32, device=self.device) if want_logits else None
        self._chk(self.lib.gvl_prefill(self.ctx, seq, _ptr(embeds), embeds.shape[0], _ptr(logits), self.stream), "gvl_prefill")
        return logits

    def decode_greedy(self, seq: int, max_new: int, eos_id: Optional[int]) -> List[int]:
        buf = (C.c_int32 * max_new)()
        n = C.c_int(0)
        self._chk(self.lib.gvl_decode_greedy(self.ctx, seq, int(max_new), -1 if eos_id is None else int(eos_id), buf, C.byref(n), self.stream),
                  "gvl_decode_greedy")
        return [int(buf[i]) for i in range(n.value)]

    def prefill_batch(self, seqs: Sequence[int], embeds: Sequence[torch.Tensor]) -> None:
        """Prefill several sequences together -- equal or ragged lengths (one pass of the decoder GEMMs over all their rows)."""
        es = [e.contiguous() for e in embeds]
        n = len(seqs)
        ids = (C.c_int * n)(*[int(s) for s in seqs])
        ptrs = (C.c_void_p * n)(*[e.data_ptr() for e in es])
        lens = (C.c_int * n)(*[int(e.shape[0]) for e in es])
        self._chk(self.lib.gvl_prefill_varlen(self.ctx, ids, n, ptrs, lens, self.stream), "gvl_prefill_varlen")

    def decode_greedy_batch(self, seqs: Sequence[int], max_new: int, eos_id: Optional[int]) -> List[List[int]]:
        """Greedy decode of several freshly prefilled sequences together (weights streamed once per step per group of up to 16 sequences)."""
        n = len(seqs)
        ids = (C.c_int * n)(*[int(s) for s in seqs])
        buf = (C.c_int32 * (n * max_new))()
        nout = (C.c_int * n)()
        self._chk(self.lib.gvl_decode_greedy_batch(self.ctx, ids, n, int(max_new), -1 if eos_id is None else int(eos_id), buf, nout, self.stream),
                  "gvl_decode_greedy_batch")
        return [[int(buf[i * max_new + j]) for j in range(nout[i])] for i in range(n)]

    def forward_loss(self, embeds: torch.Tensor, labels: Sequence[int]) -> Tuple[float, int]:
        """Causal-LM loss terms of one sample: (sum of token nll, number of labelled tokens); labels use -100 = ignore."""
        embeds = embeds.contiguous()
        S = embeds.shape[0]
        assert len(labels) == S, "labels must cover every row of inputs_embeds"
        lab = (C.c_int64 * S)(*[int(v) for v in labels])
        nll, n = C.c_double(0.0), C.c_int(0)
        seq = self.seq_alloc(S)
        try:
            self._chk(self.lib.gvl_forward_loss(self.ctx, seq, _ptr(embeds), S, lab, C.byref(nll), C.byref(n), self.stream), "gvl_forward_loss")
        finally:
            self.seq_free(seq)
        return nll.value, n.value

    def decode_steps(self, seqs: Sequence[int], n_steps: int) -> None:
        """Advance every listed sequence by n_steps greedy tokens (mixed generation steps allowed; asynchronous)."""
        n = len(seqs)
        ids = (C.c_int * n)(*[int(s) for s in seqs])
        self._chk(self.lib.gvl_decode_steps(self.ctx, ids, n, int(n_steps), self.stream), "gvl_decode_steps")

    def seq_read(self, seq: int, first: int = 0, cap: int = 4096) -> List[int]:
        """Ids generated so far by `seq`, from generation index `first` (synchronises the stream)."""
        buf = (C.c_int32 * max(cap, 1))()
        n = C.c_int(0)
        self._chk(self.lib.gvl_seq_read(self.ctx, int(seq), int(first), buf, int(cap), C.byref(n), self.stream), "gvl_seq_read")
        return [int(buf[i]) for i in range(max(0, min(n.value - first, cap)))]

    def decode_step_logits(self, seq: int, tok: int) -> torch.Tensor:
        logits = torch.empty((self.geo.vocab,), dtype=torch.float32, device=self.device)
        self._chk(self.lib.gvl_decode_step_logits(self.ctx, seq, int(tok), _ptr(logits), self.stream), "gvl_decode_step_logits")
        return logits

    def decode_step_logits_batch(self, seqs: Sequence[int], toks: Sequence[int]) -> torch.Tensor:
        """One teacher-forced decode step for several sequences together (one stream of the weights): [n, vocab] fp32 logits."""
        n = len(seqs)
        logits = torch.empty((n, self.geo.vocab), dtype=torch.float32, device=self.device)
        ids = (C.c_int * n)(*[int(s) for s in seqs]); tk = (C.c_int32 * n)(*[int(t) for t in toks])
        self._chk(self.lib.gvl_decode_step_logits_batch(self.ctx, ids, n, tk, _ptr(logits), self.stream), "gvl_decode_step_logits_batch")
        return logits

    # ---- classifier-free guidance against a negative sequence (gvl_seq_set_guidance; the guidance / follow kernels of csrc/gvl_pick.hip) ----
    def seq_set_guidance(self, seq: int, neg_seq: Optional[int], scale: float = 1.0, cond_logits: Optional[torch.Tensor] = None,
                         neg_logits: Optional[torch.Tensor] = None) -> None:
        """gvl_seq_set_guidance: bind the freshly prefilled sequence `seq` (the leader) to the freshly prefilled negative sequence `neg_seq` (its follower); HF
        generate(guidance_scale=scale, negative_prompt_ids=...).  cond_logits / neg_logits: the two prefills' last-row logits (prefill(..., want_logits=True)); they are
        scratch for the call, which re-selects the first token from the guided row and writes it to both sequences; they must be RAW rows -- set the leader's processors,
        rules and grammar between its prefill and this call.  From then on only `seq` is named in decode_greedy /
        decode_greedy_batch / decode_steps; the follower rides as one more row of the same step.  neg_seq None: unbind."""
        if neg_seq is None:
            self._chk(self.lib.gvl_seq_set_guidance(self.ctx, int(seq), -1, 1.0, None, None, self.stream), "gvl_seq_set_guidance")
            return
        for t in (cond_logits, neg_logits):
            if t is None or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != self.geo.vocab or t.device != self.device:
                raise ValueError("seq_set_guidance: cond_logits / neg_logits must be contiguous fp32 [vocab] device tensors (the prefills' last logits)")
        self._chk(self.lib.gvl_seq_set_guidance(self.ctx, int(seq), int(neg_seq), float(scale), _ptr(cond_logits), _ptr(neg_logits), self.stream), "gvl_seq_set_guidance")

    def op_guidance(self, logits: torch.Tensor, pairs, scales) -> torch.Tensor:
        """gvl_op_guidance on fp32 rows [R, n] IN PLACE (the row stride is taken from the tensor): pairs = [(conditional row, negative row), ...] (1 .. 8), one scale per
        pair; a pair's conditional row becomes scale * (log_softmax(cond) - log_softmax(neg)) + log_softmax(neg), every other row is untouched.  Returns logits."""
        assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.device.type == "cuda"
        R, n = logits.shape
        pr = [(int(c), int(u)) for c, u in pairs]
        sc = [float(s) for s in scales]
        if len(sc) != len(pr) or any(not (0 <= r < R) for p in pr for r in p):
            raise ValueError(f"op_guidance: one scale per pair and rows inside [0, {R})")
        flat = (C.c_int * (2 * len(pr)))(*[r for p in pr for r in p])
        self._chk(self.lib.gvl_op_guidance(self.ctx, _ptr(logits), n, int(logits.stride(0)) if R > 1 else n, flat, len(pr), (C.c_float * len(sc))(*sc), self.stream),
                  "gvl_op_guidance")
        return logits

    # ---- beam search in the library (gvl_beam_search; csrc/gvl_beam.h + the candidate kernels) -------------------
    def op_beam_candidates(self, rows: torch.Tensor, scores, logprobs: bool = False, stride0: bool = False):
        """gvl_op_beam_candidates: one beam-search step's 2k candidates of fp32 rows [k, n] with beam scores [k] -> (vals f32 [2k], idx int32 [2k] flat
        beam * n + token, proc f32 [2k]) on the device, ordered by (value descending, flat index ascending).  logprobs: the rows are processed
        log-probabilities already (otherwise raw logits: the log-softmax runs inside).  stride0: rows is ONE row [n] every beam reads (the first step)."""
        assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.device == self.device
        sc = [float(x) for x in (scores.tolist() if isinstance(scores, torch.Tensor) else scores)]
        k = len(sc)
        n = rows.shape[-1]
        if not stride0 and (rows.dim() != 2 or rows.shape[0] != k):
            raise ValueError(f"op_beam_candidates: {k} scores for rows of shape {tuple(rows.shape)}")
        vals = torch.full((2 * k,), float("nan"), dtype=torch.float32, device=self.device)
        idx = torch.full((2 * k,), -1, dtype=torch.int32, device=self.device)
        proc = torch.full((2 * k,), float("nan"), dtype=torch.float32, device=self.device)
        self._chk(self.lib.gvl_op_beam_candidates(self.ctx, _ptr(rows), n, k, 0 if stride0 else n, (C.c_float * k)(*sc), int(bool(logprobs)), _ptr(vals), _ptr(idx),
                                                  _ptr(proc), self.stream), "gvl_op_beam_candidates")
        return vals, idx, proc

    def op_beam_normalize(self, rows: torch.Tensor) -> torch.Tensor:
        """gvl_op_beam_normalize: fp32 rows [k, n] of raw logits -> their log-softmax IN PLACE (the candidate kernel's own arithmetic); returns rows."""
        assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.dim() == 2 and rows.device == self.device
        self._chk(self.lib.gvl_op_beam_normalize(self.ctx, _ptr(rows), rows.shape[1], rows.shape[0], self.stream), "gvl_op_beam_normalize")
        return rows

    def _beam_params(self, first_logits: torch.Tensor, num_beams: int, max_new: int, eos: Optional[int], length_penalty: float, early_stopping, processors,
                     rules: Optional[int]) -> "L.GvlBeamParams":
        """what the two beam entries share of their arguments"""
        if early_stopping not in (False, True, "never"):
            raise ValueError("early_stopping must be False, True or 'never'")
        assert first_logits.dtype == torch.float32 and first_logits.is_contiguous() and first_logits.device == self.device
        pe, ng, mn, pe_eos = processors.args() if processors is not None else (1.0, 0, 0, None)
        return L.GvlBeamParams(int(num_beams), int(max_new), -1 if eos is None else int(eos), float(length_penalty), {False: 0, True: 1, "never": 2}[early_stopping],
                               float(pe), int(ng), int(mn), -1 if pe_eos is None else int(pe_eos), -1 if rules is None else int(rules))

    def _run_beam_entry(self, entry, num_beams: int, max_new: int, num_return: int, with_scores: bool):
        """entry(nr, ids, cap, n, score, ts) -> (status, name): one beam entry over result buffers for num_return hypotheses, unpacked as beam_search documents"""
        cap, nr = max(int(max_new), 1), int(num_return)
        if nr < 1 or nr > int(num_beams):
            raise ValueError("num_return must be 1 .. num_beams")
        ids = (C.c_int32 * (cap * nr))()
        ts = (C.c_float * (cap * nr))()
        n, score = (C.c_int * nr)(), (C.c_double * nr)()
        self._chk(*entry(nr, ids, cap, n, score, ts))
        res = []
        for r in range(nr):
            out = [int(ids[r * cap + i]) for i in range(n[r])]
            res.append((out, score[r], [float(ts[r * cap + i]) for i in range(n[r])]) if with_scores else out)
        return res[0] if nr == 1 else res

    def beam_search(self, seq: int, first_logits: torch.Tensor, num_beams: int, max_new: int, eos: Optional[int], length_penalty: float = 1.0, early_stopping=False,
                    processors=None, rules: Optional[int] = None, with_scores: bool = False, num_return: int = 1):
        """gvl_beam_search: HF beam search (num_beams = k, do_sample = False) from the PREFILLED sequence `seq` and its prefill logits, inside the library; `seq` is not
        consumed.  processors: a logits.Processors (None = off); rules: a rule-set id (None = none); early_stopping: False / True / "never".  Returns the new ids, or with
        with_scores (ids, sequences_score, transition_scores) as beam.beam_search does.  num_return > 1 (gvl_beam_search_n): a list of such results, the num_return best
        hypotheses, best first."""
        prm = self._beam_params(first_logits, num_beams, max_new, eos, length_penalty, early_stopping, processors, rules)

        def entry(nr, ids, cap, n, score, ts):
            if nr == 1:
                return self.lib.gvl_beam_search(self.ctx, int(seq), _ptr(first_logits), C.byref(prm), ids, cap, n, score, ts, self.stream), "gvl_beam_search"
            return self.lib.gvl_beam_search_n(self.ctx, int(seq), _ptr(first_logits), C.byref(prm), nr, ids, cap, n, score, ts, self.stream), "gvl_beam_search_n"
        return self._run_beam_entry(entry, num_beams, max_new, num_return, with_scores)

    def op_beam_group(self, rows: Optional[torch.Tensor], scores, eos: Optional[int] = None, pad: Optional[int] = None, logprobs: bool = True, stride0: bool = False,
                      done: bool = False, s: Optional[int] = None):
        """gvl_op_beam_group: ONE group of a diverse beam search step -- op_beam_candidates for the group's s rows [s, n] (s = len(scores), 1 .. 16) -> (vals [2s], idx
        int32 [2s] local beam * n + token, proc [2s], chosen int32 [s]) on the device; chosen = the tokens of the first s candidates that are not eos (-1 where there are
        fewer).  done: the group is finished -- no candidates (the first three are None), chosen [s] = pad (None: -1); give s."""
        if done:
            chosen = torch.full((int(s),), -7, dtype=torch.int32, device=self.device)
            self._chk(self.lib.gvl_op_beam_group(self.ctx, None, 0, int(s), 0, None, 1, -1 if eos is None else int(eos), -1 if pad is None else int(pad), 1, None, None, None,
                                                 _ptr(chosen), self.stream), "gvl_op_beam_group")
            return None, None, None, chosen
        assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.device == self.device
        sc = [float(x) for x in (scores.tolist() if isinstance(scores, torch.Tensor) else scores)]
        s_, n = len(sc), rows.shape[-1]
        if not stride0 and (rows.dim() != 2 or rows.shape[0] != s_):
            raise ValueError(f"op_beam_group: {s_} scores for rows of shape {tuple(rows.shape)}")
        vals = torch.full((2 * s_,), float("nan"), dtype=torch.float32, device=self.device)
        idx = torch.full((2 * s_,), -1, dtype=torch.int32, device=self.device)
        proc = torch.full((2 * s_,), float("nan"), dtype=torch.float32, device=self.device)
        chosen = torch.full((s_,), -7, dtype=torch.int32, device=self.device)
        self._chk(self.lib.gvl_op_beam_group(self.ctx, _ptr(rows), n, s_, 0 if stride0 else n, (C.c_float * s_)(*sc), int(bool(logprobs)), -1 if eos is None else int(eos),
                                             -1 if pad is None else int(pad), 0, _ptr(vals), _ptr(idx), _ptr(proc), _ptr(chosen), self.stream), "gvl_op_beam_group")
        return vals, idx, proc, chosen

    def group_beam_search(self, seq: int, first_logits: torch.Tensor, num_beams: int, num_beam_groups: int, diversity_penalty: float, max_new: int, eos: Optional[int],
                          pad: Optional[int] = None, length_penalty: float = 1.0, early_stopping=False, processors=None, rules: Optional[int] = None,
                          with_scores: bool = False, num_return: int = 1):
        """gvl_group_beam_search: HF diverse (group) beam search (num_beams = k, num_beam_groups = G, diversity_penalty) from the PREFILLED sequence `seq`, inside the
        library; everything else as beam_search.  pad: the token of a finished group's beams (None: an id no later group counts)."""
        base = self._beam_params(first_logits, num_beams, max_new, eos, length_penalty, early_stopping, processors, rules)
        prm = L.GvlGroupBeamParams(base, int(num_beam_groups), float(diversity_penalty), -1 if pad is None else int(pad))
        return self._run_beam_entry(lambda nr, ids, cap, n, score, ts: (self.lib.gvl_group_beam_search(
            self.ctx, int(seq), _ptr(first_logits), C.byref(prm), nr, ids, cap, n, score, ts, self.stream), "gvl_group_beam_search"), num_beams, max_new, num_return, with_scores)

    # ---- contrastive search (gvl_contrastive.hip) --------------------------------------------------
    def seq_keep_hidden(self, seq: int, on: bool = True):
        """gvl_seq_keep_hidden: the EMPTY sequence `seq` gets a hidden bank -- per context row the post-final-norm hidden state (bf16) and its inverse norm --
        filled by prefill() and by every decode_step_logits* step.  Call it before the prefill; contrastive_search needs it."""
        self._chk(self.lib.gvl_seq_keep_hidden(self.ctx, int(seq), int(bool(on))), "gvl_seq_keep_hidden")

    def seq_read_hidden(self, seq: int, first: int, n: int):
        """gvl_seq_read_hidden: bank rows [first, first + n) of a keep-hidden sequence -> (bf16 [n, hidden], fp32 inverse norms [n]) on the device."""
        rows = torch.empty((int(n), self.geo.hidden), dtype=bf, device=self.device)
        inv = torch.empty((int(n),), dtype=torch.float32, device=self.device)
        self._chk(self.lib.gvl_seq_read_hidden(self.ctx, int(seq), int(first), int(n), _ptr(rows), _ptr(inv), self.stream), "gvl_seq_read_hidden")
        return rows, inv

    def op_hidden_bank_append(self, x: torch.Tensor, w: torch.Tensor, eps: float):
        """gvl_op_hidden_bank_append: residual rows x bf16 [n, cols] (any row pitch) -> (rows bf16 [n, cols] = op_rmsnorm(x, w, eps) bit for bit, inverse norms fp32 [n])."""
        assert x.dtype == bf and x.dim() == 2 and x.stride(1) == 1 and w.dtype == bf and w.is_contiguous() and x.device == self.device
        n, cols = x.shape
        rows = torch.empty((n, cols), dtype=bf, device=self.device)
        inv = torch.empty((n,), dtype=torch.float32, device=self.device)
        self._chk(self.lib.gvl_op_hidden_bank_append(self.ctx, _ptr(x), int(x.stride(0)), _ptr(w), float(eps), _ptr(rows), _ptr(inv), n, cols, self.stream),
                  "gvl_op_hidden_bank_append")
        return rows, inv

    def op_contrastive_rank(self, bank: torch.Tensor, bank_inv: torch.Tensor, cand: torch.Tensor, cand_inv: torch.Tensor, p: torch.Tensor, alpha: float):
        """gvl_op_contrastive_rank: bank bf16 [n_ctx, D] + inverse norms, candidates bf16 [k, D] + inverse norms, p fp32 [k] -> (pen fp32 [k], score fp32 [k],
        selected rank int32 [1]) on the device: pen_i = max_j cos(g_i, h_j), score_i = (1 - alpha) p_i - alpha pen_i, ties to the lower rank."""
        for t in (bank, bank_inv, cand, cand_inv, p):
            assert t.is_contiguous() and t.device == self.device
        assert bank.dtype == bf and cand.dtype == bf and bank_inv.dtype == cand_inv.dtype == p.dtype == torch.float32
        n_ctx, D = bank.shape
        k = cand.shape[0]
        assert cand.shape[1] == D and bank_inv.numel() == n_ctx and cand_inv.numel() == k and p.numel() == k
        pen = torch.full((k,), float("nan"), dtype=torch.float32, device=self.device)
        score = torch.full((k,), float("nan"), dtype=torch.float32, device=self.device)
        sel = torch.full((1,), -1, dtype=torch.int32, device=self.device)
        self._chk(self.lib.gvl_op_contrastive_rank(self.ctx, _ptr(bank), _ptr(bank_inv), n_ctx, D, _ptr(cand), _ptr(cand_inv), _ptr(p), k, float(alpha),
                                                   _ptr(pen), _ptr(score), _ptr(sel), self.stream), "gvl_op_contrastive_rank")
        return pen, score, sel

    def contrastive_search(self, seq: int, first_logits: torch.Tensor, top_k: int, penalty_alpha: float, max_new: int, eos: Optional[int], processors=None,
                           rules: Optional[int] = None, with_trace: bool = False):
        """gvl_contrastive_search: HF contrastive search (penalty_alpha, top_k) from the PREFILLED keep-hidden sequence `seq` and its prefill logits, inside the
        library; `seq` is not consumed.  processors / rules as beam_search; the sequence's grammar applies.  Returns the new ids, or with with_trace (ids, trace):
        trace = {"ids": [steps][k] candidate ids in rank order, "p": [steps][k], "pen": [steps][k], "sel": [steps] selected ranks, "hidden": bf16 [steps, hidden] the
        rows the search committed to its bank, "rows": fp32 [steps, vocab] the processed row every step's candidates were taken from}."""
        assert first_logits.dtype == torch.float32 and first_logits.is_contiguous() and first_logits.device == self.device
        pe, ng, mn, pe_eos = processors.args() if processors is not None else (1.0, 0, 0, None)
        k = int(top_k)
        prm = L.GvlContrastiveParams(k, float(penalty_alpha), int(max_new), -1 if eos is None else int(eos), float(pe), int(ng), int(mn),
                                     -1 if pe_eos is None else int(pe_eos), -1 if rules is None else int(rules))
        cap = max(int(max_new), 1)
        ids, n = (C.c_int32 * cap)(), C.c_int(0)
        if not with_trace:
            self._chk(self.lib.gvl_contrastive_search(self.ctx, int(seq), _ptr(first_logits), C.byref(prm), ids, cap, C.byref(n), None, None, None, None, None, None,
                                                      self.stream), "gvl_contrastive_search")
            return [int(ids[i]) for i in range(n.value)]
        kk = max(k, 1)
        t_ids, t_p, t_pen, t_sel = (C.c_int32 * (cap * kk))(), (C.c_float * (cap * kk))(), (C.c_float * (cap * kk))(), (C.c_int32 * cap)()
        hid = torch.zeros((cap, self.geo.hidden), dtype=bf, device=self.device)
        rows = torch.zeros((cap, self.geo.vocab), dtype=torch.float32, device=self.device)
        self._chk(self.lib.gvl_contrastive_search(self.ctx, int(seq), _ptr(first_logits), C.byref(prm), ids, cap, C.byref(n), t_ids, t_p, t_pen, t_sel, _ptr(rows), _ptr(hid),
                                                  self.stream), "gvl_contrastive_search")
        steps = n.value
        trace = {"ids": [[int(t_ids[s * k + i]) for i in range(k)] for s in range(steps)], "p": [[float(t_p[s * k + i]) for i in range(k)] for s in range(steps)],
                 "pen": [[float(t_pen[s * k + i]) for i in range(k)] for s in range(steps)], "sel": [int(t_sel[s]) for s in range(steps)], "hidden": hid[:steps], "rows": rows[:steps]}
        return [int(ids[i]) for i in range(steps)], trace

    def group_beam_tokens(self, num_beams: int) -> List[List[int]]:
        """gvl_debug_group_beam_tokens: per step of the last group_beam_search, the num_beams tokens the DEVICE chose (a finished group's: its pad)."""
        n = C.c_int(0)
        self._chk(self.lib.gvl_debug_group_beam_tokens(self.ctx, None, 0, C.byref(n)), "gvl_debug_group_beam_tokens")
        buf = (C.c_int32 * max(n.value, 1))()
        self._chk(self.lib.gvl_debug_group_beam_tokens(self.ctx, buf, n.value, C.byref(n)), "gvl_debug_group_beam_tokens")
        k = int(num_beams)
        return [[int(buf[i * k + j]) for j in range(k)] for i in range(n.value // k)]

    def group_beam_pool(self) -> List[Tuple[int, int]]:
        """gvl_debug_group_beam_pool: behind every step's cache reorder of the last group_beam_search (every step but the last), (clones the search held, free KV pages)."""
        n = C.c_int(0)
        self._chk(self.lib.gvl_debug_group_beam_pool(self.ctx, None, 0, C.byref(n)), "gvl_debug_group_beam_pool")
        buf = (C.c_int32 * max(n.value, 1))()
        self._chk(self.lib.gvl_debug_group_beam_pool(self.ctx, buf, n.value, C.byref(n)), "gvl_debug_group_beam_pool")
        return [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(n.value // 2)]

    def generate_ids(self, embeds: torch.Tensor, max_new_tokens: int, eos_id: Optional[int], processors=None, logprobs: Optional[int] = None,
                     rules: Optional[int] = None, grammar: Optional[int] = None):
        """language_model.generate(inputs_embeds=..., greedy): returns only the NEW ids (eos included).  grammar: a grammar_create id for this sequence (None: the
        default of set_grammar).  processors: a logits.Processors for this
        sequence (None: the default of set_logits_processors).  rules: a rule-set id for this sequence (None: the default of set_token_rules).  logprobs: None = ids only; -1 .. 8 = this sequence's seq_set_logprobs setting, and
        the return value is (ids, (lp, top)) as seq_read_logprobs gives them for the ids (read before the sequence is freed)."""
        opts = LP.SeqOptions(processors, logprobs, ... if rules is None else rules, grammar=... if grammar is None else grammar)
        seq = self.seq_alloc(min(embeds.shape[0] + max_new_tokens, self.geo.max_seq))
        try:
            LP.apply_seq_options(self, seq, opts)
            self.prefill(seq, embeds)
            ids = self.decode_greedy(seq, max_new_tokens, eos_id)
            return ids if logprobs is None else (ids, LP.read_seq_logprobs(self, seq, ids, opts))
        finally:
            self.seq_free(seq)

    # ---- measurement -----------------------------------------------------------------------------
    def trace_marker(self, tag: int = 0, stream=None):
        """gvl_trace_marker on `stream` (a torch stream; default: the current one): a named empty dispatch that brackets a region of a kernel trace."""
        st = C.c_void_p(stream.cuda_stream) if stream is not None else self.stream
        self._chk(self.lib.gvl_trace_marker(int(tag), st), "gvl_trace_marker")

    def prof_enable(self, on: bool):
        self._chk(self.lib.gvl_prof_enable(self.ctx, 1 if on else 0), "gvl_prof_enable")

    def prof_read(self, cat: int):
        ms, n, w = C.c_double(0), C.c_int64(0), C.c_double(0)
        self._chk(self.lib.gvl_prof_read(self.ctx, cat, C.byref(ms), C.byref(n), C.byref(w)), "gvl_prof_read")
        return ms.value, n.value, w.value

    # ---- operator-level (parity tests) -------------------------------------------------------------
    def op_gemm(self, A, W, bias=None, gamma=None, resid=None, act=L.ACT_NONE, out_f32=False, tile_cfg=0):
        M, K = A.shape
        N = W.shape[0]
        n_out = N // 2 if act == L.ACT_SILU_MUL else N
        Cc = torch.empty((M, n_out), dtype=torch.float32 if out_f32 else bf, device=self.device)
        self._chk(self.lib.gvl_op_gemm(self.ctx, _ptr(A.contiguous()), _ptr(W.contiguous()), _ptr(Cc), M, N, K, _ptr(bias), _ptr(gamma),
                                       _ptr(resid), act, 1 if out_f32 else 0, tile_cfg, self.stream), "gvl_op_gemm")
        return Cc

    def op_gemm_rows(self, A, W, bias=None, gamma=None, resid=None, act=L.ACT_NONE, rowscale=None, want_rowsq=False, tile_cfg=0):
        """gvl_op_gemm_rows: the fused-RMSNorm epilogues.  rowscale [M] f32 multiplies the accumulator rows; want_rowsq: also returns the sums of squares of the
        bf16 outputs per aligned 64-column block, [M, N // 64] f32 (NaN-filled first: every slot must be written)."""
        M, K = A.shape
        N = W.shape[0]
        n_out = N // 2 if act == L.ACT_SILU_MUL else N
        Cc = torch.empty((M, n_out), dtype=bf, device=self.device)
        sq = torch.full((M, N // 64), float("nan"), dtype=torch.float32, device=self.device) if want_rowsq else None
        self._chk(self.lib.gvl_op_gemm_rows(self.ctx, _ptr(A.contiguous()), _ptr(W.contiguous()), _ptr(Cc), M, N, K, _ptr(bias), _ptr(gamma), _ptr(resid), act,
                                            _ptr(rowscale), _ptr(sq), N // 64 if want_rowsq else 0, tile_cfg, self.stream), "gvl_op_gemm_rows")
        return (Cc, sq) if want_rowsq else Cc

    def op_gemm_grouped(self, A, W, out, grp_rows, grp_stride, row_off, bias=None, gamma=None, resid=None, act=L.ACT_NONE, rowsq=None, tile_cfg=0):
        """gvl_op_gemm_grouped: GEMM row m is stored at row (m / grp_rows) * grp_stride + m % grp_rows + row_off of `out` (bf16 or f32, contiguous,
        ceil(M / grp_rows) * grp_stride rows, written in place: the caller pre-fills it).  rowsq [M, N // 64] f32: refused by the library."""
        M, K = A.shape
        N = W.shape[0]
        assert out.is_contiguous() and out.dtype in (bf, torch.float32)
        self._chk(self.lib.gvl_op_gemm_grouped(self.ctx, _ptr(A.contiguous()), _ptr(W.contiguous()), _ptr(out), M, N, K, _ptr(bias), _ptr(gamma), _ptr(resid), act,
                                               1 if out.dtype == torch.float32 else 0, _ptr(rowsq), N // 64 if rowsq is not None else 0, int(grp_rows),
                                               int(grp_stride), int(row_off), tile_cfg, self.stream), "gvl_op_gemm_grouped")
        return out

    def op_patch_embed(self, mode, path, px, W, cls, pos, out, patch, bias=None, lnw=None, lnb=None, eps=1e-5, im2col=None):
        """gvl_op_patch_embed (include/gvl.h): mode 0 CLIP / 1 InternVideo2, path 0 fused / 1 three passes.  px f32 [n, 3, T, image, image], W bf16 [C, Kp];
        `out` (and `im2col`, path 1) are written in place: the caller allocates and pre-fills them.  Raises GvlError (status ERR_ARG) on a refusal."""
        d = L.GvlPatchEmbed()
        n, _, T, image, _ = px.shape
        keep = [t if t is None else t.contiguous() for t in (px, W, bias, cls, pos, lnw, lnb)]
        assert out.is_contiguous() and (im2col is None or im2col.is_contiguous())
        d.mode, d.path, d.n, d.T, d.image, d.patch, d.C, d.Kp, d.eps = mode, path, n, T, image, patch, W.shape[0], W.shape[1], float(eps)
        for name, t in zip(("px", "W", "bias", "cls", "pos", "lnw", "lnb"), keep):
            setattr(d, name, None if t is None else t.data_ptr())
        d.out, d.im2col = out.data_ptr(), None if im2col is None else im2col.data_ptr()
        self._chk(self.lib.gvl_op_patch_embed(self.ctx, C.byref(d), self.stream), "gvl_op_patch_embed")
        return out

    def op_patchify(self, px, out, patch):
        """px f32 [n, 3, T, image, image] -> out bf16 [n T (image / patch)^2, Kp] (in place)."""
        n, _, T, image, _ = px.shape
        self._chk(self.lib.gvl_op_patchify(self.ctx, _ptr(px.contiguous()), _ptr(out), n, T, image, patch, out.shape[-1], self.stream), "gvl_op_patchify")
        return out

    def op_hd_merge(self, f, sub_gn, out):
        """f f32 [n, 576, C], sub_gn f32 [4 C] -> out bf16 [n, 156, 4 C] (in place)."""
        self._chk(self.lib.gvl_op_hd_merge(self.ctx, _ptr(f.contiguous()), _ptr(sub_gn.contiguous()), _ptr(out), f.shape[0], f.shape[2], self.stream), "gvl_op_hd_merge")
        return out

    def op_pool_spatial(self, f, out):
        """f f32 [n, 576, C] -> out bf16 [n, 64, C] (in place)."""
        self._chk(self.lib.gvl_op_pool_spatial(self.ctx, _ptr(f.contiguous()), _ptr(out), f.shape[0], f.shape[2], self.stream), "gvl_op_pool_spatial")
        return out

    def op_pool_temporal(self, f, out):
        """f bf16 [n, T, 256, C] -> out bf16 [n, T, 16, C] (in place)."""
        self._chk(self.lib.gvl_op_pool_temporal(self.ctx, _ptr(f.contiguous()), _ptr(out), f.shape[0], f.shape[1], f.shape[3], self.stream), "gvl_op_pool_temporal")
        return out

    def op_strip_cls(self, x, out):
        """x [n, S, C] f32 or bf16 -> out [n, S - 1, C] (in place)."""
        self._chk(self.lib.gvl_op_strip_cls(self.ctx, _ptr(x.contiguous()), _ptr(out), x.shape[0], x.shape[1], x.shape[2], x.element_size(), self.stream),
                  "gvl_op_strip_cls")
        return out

    def op_bcast_row(self, row, dst, n, stride_rows, row_off):
        """dst bf16 [n * stride_rows, cols]: rows s * stride_rows + row_off receive `row` (in place)."""
        self._chk(self.lib.gvl_op_bcast_row(self.ctx, _ptr(row.contiguous()), _ptr(dst), n, stride_rows, row_off, row.shape[-1], self.stream), "gvl_op_bcast_row")
        return dst

    def op_fold_gamma(self, W, gamma):
        W = W.contiguous()
        out = torch.empty_like(W)
        self._chk(self.lib.gvl_op_fold_gamma(self.ctx, _ptr(W), _ptr(gamma.contiguous()), _ptr(out), W.shape[0], W.shape[1], self.stream), "gvl_op_fold_gamma")
        return out

    def op_rowsq_finish(self, sq, cols, eps, b0=0, nblk=None):
        sq = sq.contiguous()
        nblk = sq.shape[1] - b0 if nblk is None else nblk
        rs = torch.empty((sq.shape[0],), dtype=torch.float32, device=self.device)
        self._chk(self.lib.gvl_op_rowsq_finish(self.ctx, _ptr(sq), sq.shape[1], b0, nblk, _ptr(rs), sq.shape[0], cols, float(eps), self.stream), "gvl_op_rowsq_finish")
        return rs

    def op_attention(self, qkv: torch.Tensor, B, S, H, KV, Dr, scale, causal):
        """qkv bf16 [B*S, (H+2KV)*Dr] fused rows -> out bf16 [B*S, H*Dr]."""
        qkv = qkv.contiguous()
        out = torch.empty((B * S, H * Dr), dtype=bf, device=self.device)
        base = qkv.data_ptr()
        self._chk(self.lib.gvl_op_attention(self.ctx, C.c_void_p(base), C.c_void_p(base + 2 * H * Dr), C.c_void_p(base + 2 * (H + KV) * Dr),
                                            _ptr(out), B, S, H, KV, Dr, float(scale), int(causal), self.stream), "gvl_op_attention")
        return out

    def op_layernorm(self, x, w, b, eps):
        y = torch.empty(x.shape, dtype=bf, device=self.device)
        self._chk(self.lib.gvl_op_layernorm(self.ctx, _ptr(x.contiguous()), _ptr(w), _ptr(b), _ptr(y), x.shape[0], x.shape[1], float(eps), self.stream),
                  "gvl_op_layernorm")
        return y

    def op_rmsnorm(self, x, w, eps):
        y = torch.empty(x.shape, dtype=bf, device=self.device)
        self._chk(self.lib.gvl_op_rmsnorm(self.ctx, _ptr(x.contiguous()), _ptr(w), _ptr(y), x.shape[0], x.shape[1], float(eps), self.stream),
                  "gvl_op_rmsnorm")
        return y

    def debug_set(self, key: str, value: int):
        """gvl_debug_set: result-neutral launch parameters ("decode_attn_cpb", "decode_attn_hpb", "decode_graph"); 0 = the launcher's choice."""
        self._chk(self.lib.gvl_debug_set(self.ctx, key.encode(), int(value)), "gvl_debug_set")

    def set_sampling(self, do_sample, temperature=1.0, top_k=50, top_p=None, seed=0, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
        """Token selection of every later prefill / decode call, for the sequences without a setting of their own: greedy argmax (do_sample False) or
        temperature / top-k / top-p sampling on the device (HF generate's do_sample=True; `top_k` 50 is HF's GenerationConfig default, `top_p` None / 1.0 =
        off), then HF's min_p / typical_p / epsilon_cutoff / eta_cutoff warpers (None / 0 = off; typical_p 1.0 = off) -- gvl_set_sampling_ex when one is on."""
        if not do_sample or not any(_on(v) for v in (min_p, typical_p, epsilon_cutoff, eta_cutoff)):
            self._chk(self.lib.gvl_set_sampling(self.ctx, int(bool(do_sample)), float(temperature), int(top_k or 0),
                                                float(top_p) if top_p is not None else 0.0, int(seed) & (2 ** 64 - 1)), "gvl_set_sampling")
            return
        g = sampling_struct(True, temperature, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff, seed, 0)
        self._chk(self.lib.gvl_set_sampling_ex(self.ctx, C.byref(g)), "gvl_set_sampling_ex")

    def seq_set_sampling(self, seq: int, sampling: Optional[dict] = None, **kw):
        """gvl_seq_set_sampling: one live sequence's OWN setting -- a dict / keywords of do_sample, temperature, top_k, top_p, min_p, typical_p, epsilon_cutoff,
        eta_cutoff, seed, stream (sampling_struct's defaults) -- from the next prefill / decode call on: the sequence is greedy or sampled by it whatever the
        engine's setting and its neighbours in a decode group are, and its draws depend on (seed, stream, step, logits) alone.  None (and no keywords): back to
        following the engine's setting.  Forks and clones copy it, stream included."""
        if sampling is None and not kw:
            self._chk(self.lib.gvl_seq_set_sampling(self.ctx, int(seq), None), "gvl_seq_set_sampling")
            return
        g = sampling_struct(**{**(sampling or {}), **kw})
        self._chk(self.lib.gvl_seq_set_sampling(self.ctx, int(seq), C.byref(g)), "gvl_seq_set_sampling")

    def op_select_rows(self, logits: torch.Tensor, rows, top_n=-1, steps=None, kept: bool = False):
        """gvl_op_select_rows on fp32 rows [B, n] (B <= 16): row b is selected by rows[b] (a dict as seq_set_sampling takes it; None = greedy) at generation
        step steps[b].  Returns op_select_logprobs' (tokens, lp, top_ids, top_lp), and with kept=True also the uint8 [B, n] mask of each row's final kept set."""
        B, n = logits.shape
        if len(rows) != B:
            raise ValueError(f"op_select_rows: {len(rows)} settings for {B} rows")
        tn = [int(x) for x in (top_n if isinstance(top_n, (list, tuple)) else [top_n] * B)]
        arr = (L.GvlSampling * B)(*[sampling_struct(**(r or {"do_sample": False})) for r in rows])
        toks = torch.full((B,), -1, dtype=torch.int32, device=self.device)
        lp = torch.full((B,), float("nan"), dtype=torch.float32, device=self.device)
        ti = torch.full((B, LPR.MAX_TOP), -2, dtype=torch.int32, device=self.device)
        tv = torch.full((B, LPR.MAX_TOP), float("nan"), dtype=torch.float32, device=self.device)
        km = torch.full((B, n), 255, dtype=torch.uint8, device=self.device) if kept else None
        steps_d = torch.tensor(list(steps) if steps is not None else [0] * B, dtype=torch.int32, device=self.device)
        self._chk(self.lib.gvl_op_select_rows(self.ctx, _ptr(logits.contiguous()), n, B, arr, _ptr(steps_d), (C.c_int * B)(*tn), _ptr(toks), _ptr(lp),
                                              _ptr(ti), _ptr(tv), _ptr(km), self.stream), "gvl_op_select_rows")
        return (toks, lp, ti, tv, km) if kept else (toks, lp, ti, tv)

    def op_sample(self, logits, temperature, top_k, top_p, seed, streams, steps):
        """logits f32 [B, n] -> int32 [B] drawn tokens (row b: random stream streams[b], generation step steps[b])."""
        import ctypes as C
        B, n = logits.shape
        st = (C.c_uint32 * B)(*[int(x) for x in streams])
        steps_d = torch.tensor(list(steps), dtype=torch.int32, device=self.device)
        out = torch.empty((B,), dtype=torch.int32, device=self.device)
        self._chk(self.lib.gvl_op_sample(self.ctx, _ptr(logits.contiguous()), n, B, float(temperature), int(top_k or 0), float(top_p or 0.0),
                                         int(seed) & (2 ** 64 - 1), st, _ptr(steps_d), _ptr(out), self.stream), "gvl_op_sample")
        return out

    def set_logits_processors(self, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, min_new_tokens: int = 0, eos_id: Optional[int] = None):
        """gvl_set_logits_processors: HF's repetition penalty / no-repeat n-gram / min-length processors for every sequence allocated AFTER this call
        (the history is each sequence's generated ids only).  1.0 / 0 / 0 = off; min_new_tokens needs an eos id."""
        self._chk(self.lib.gvl_set_logits_processors(self.ctx, float(repetition_penalty), int(no_repeat_ngram_size), int(min_new_tokens),
                                                     -1 if eos_id is None else int(eos_id)), "gvl_set_logits_processors")

    def seq_set_processors(self, seq: int, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, min_new_tokens: int = 0,
                           eos_id: Optional[int] = None):
        """gvl_seq_set_processors: the processors of one live sequence (overrides the default it was allocated with)."""
        self._chk(self.lib.gvl_seq_set_processors(self.ctx, int(seq), float(repetition_penalty), int(no_repeat_ngram_size), int(min_new_tokens),
                                                  -1 if eos_id is None else int(eos_id)), "gvl_seq_set_processors")

    def op_logits_process(self, logits: torch.Tensor, histories: Sequence[Sequence[int]], penalty, ngram, min_new, eos, rules=None, grammar=None, hamming=None):
        """gvl_op_logits_process on fp32 rows [B, n] (any B; 16 rows per launch): row b gets the processors (penalty[b], ngram[b], min_new[b],
        eos[b]) over the history histories[b].  `logits` must be a contiguous fp32 device tensor: it is changed IN PLACE and returned.
        rules: None, one rule-set id (rules_create) for every row, or a list with an id or None per row -- then gvl_op_logits_process_rules
        runs the whole ordered pipeline (token rules around the processors).  grammar: the same for grammar ids (grammar_create; the grammar's
        vocab must equal n) -- then gvl_op_logits_process_ex runs the pipeline with the grammar stage in HF's place.
        hamming: (tokens, diversity_penalty) -- gvl_op_logits_process_hamming: HF's HammingDiversityLogitsProcessor in its place (behind sequence_bias, in front of the
        repetition penalty) on every row; tokens = 0 .. 16 ids, a list (uploaded here) or an int32 device tensor (what the group candidate launch left)."""
        assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2 and logits.device == self.device
        B, n = logits.shape
        assert len(histories) == B
        width = max([len(h) for h in histories] + [1])
        hist = torch.zeros((B, width), dtype=torch.int32)
        for b, h in enumerate(histories):
            if len(h):
                hist[b, :len(h)] = torch.as_tensor(list(h), dtype=torch.int32)
        hist = hist.to(self.device)
        lens = torch.tensor([len(h) for h in histories], dtype=torch.int32, device=self.device)
        per_row = lambda v, t: [t(x) for x in (v if isinstance(v, (list, tuple)) else [v] * B)]
        pe, ng, mn, eo = per_row(penalty, float), per_row(ngram, int), per_row(min_new, int), per_row(eos, lambda x: -1 if x is None else int(x))
        ru = None if rules is None else per_row(rules, lambda x: -1 if x is None else int(x))
        gr = None if grammar is None else per_row(grammar, lambda x: -1 if x is None else int(x))
        ham = None
        if hamming is not None:
            ham = hamming[0] if isinstance(hamming[0], torch.Tensor) else torch.tensor([int(t) for t in hamming[0]], dtype=torch.int32, device=self.device)
            assert ham.dtype == torch.int32 and ham.is_contiguous() and ham.device == self.device and ham.numel() <= 16
        for b0 in range(0, B, 16):
            nb = min(16, B - b0)
            args = (self.ctx, C.c_void_p(logits.data_ptr() + b0 * n * 4), n, nb, C.c_void_p(hist.data_ptr() + b0 * width * 4),
                    width, C.c_void_p(lens.data_ptr() + b0 * 4), (C.c_float * nb)(*pe[b0:b0 + nb]), (C.c_int * nb)(*ng[b0:b0 + nb]),
                    (C.c_int * nb)(*mn[b0:b0 + nb]), (C.c_int * nb)(*eo[b0:b0 + nb]))
            if ham is not None:
                rr = None if ru is None else (C.c_int * nb)(*ru[b0:b0 + nb])
                gg = None if gr is None else (C.c_int * nb)(*gr[b0:b0 + nb])
                self._chk(self.lib.gvl_op_logits_process_hamming(*args, rr, gg, C.c_void_p(ham.data_ptr()) if ham.numel() else None, int(ham.numel()),
                                                                 float(hamming[1]), self.stream), "gvl_op_logits_process_hamming")
            elif gr is not None:
                rr = None if ru is None else (C.c_int * nb)(*ru[b0:b0 + nb])
                self._chk(self.lib.gvl_op_logits_process_ex(*args, rr, (C.c_int * nb)(*gr[b0:b0 + nb]), self.stream), "gvl_op_logits_process_ex")
            elif ru is None:
                self._chk(self.lib.gvl_op_logits_process(*args, self.stream), "gvl_op_logits_process")
            else:
                self._chk(self.lib.gvl_op_logits_process_rules(*args, (C.c_int * nb)(*ru[b0:b0 + nb]), self.stream), "gvl_op_logits_process_rules")
        return logits

    # ---- token rules (logits.TokenRules -> a device rule set) ---------------------------------------------------
    def rules_create(self, rules) -> int:
        """gvl_rules_create: a logits.TokenRules (or anything with its fields) as an immutable device rule set; returns its id.  Raises GvlError
        (status ERR_ARG, with the library's message) for a set beyond the library's capacities."""
        keep = []

        def ints(v):
            a = np.ascontiguousarray(np.asarray(v, dtype=np.int32).reshape(-1))
            keep.append(a)
            return len(a), a.ctypes.data_as(C.POINTER(C.c_int32))
        d = L.GvlRulesDesc()
        d.n_suppress, d.suppress = ints(rules.suppress)
        d.n_begin_suppress, d.begin_suppress = ints(rules.begin_suppress)
        d.begin_index = int(rules.begin_index)
        d.n_force, d.force_ids = ints(rules.force_ids)
        d.force_at = int(rules.force_at)
        for st, t in enumerate((rules.sequence_bias, rules.bad_words)):
            bt = d.bias[st]
            n3, bt.targets = ints(t.targets)
            bt.n_targets = n3 // 3
            eb = np.ascontiguousarray(np.asarray(t.entry_bias, dtype=np.float32).reshape(-1))
            keep.append(eb)
            bt.n_entries, bt.entry_bias = len(eb), eb.ctypes.data_as(C.POINTER(C.c_float))
            _, bt.entry_prefix = ints(t.entry_prefix)
            bt.n_prefix, bt.prefix = ints(t.prefix)
        rid = C.c_int(-1)
        self._chk(self.lib.gvl_rules_create(self.ctx, C.byref(d), C.byref(rid)), "gvl_rules_create")
        return rid.value

    def rules_destroy(self, rules_id: int):
        """gvl_rules_destroy: GvlError (ERR_STATE) while a live sequence or the default still references the set."""
        self._chk(self.lib.gvl_rules_destroy(self.ctx, int(rules_id)), "gvl_rules_destroy")

    def set_token_rules(self, rules_id: Optional[int] = None):
        """gvl_set_token_rules: the rule set of every sequence allocated AFTER this call (None / -1: none)."""
        self._chk(self.lib.gvl_set_token_rules(self.ctx, -1 if rules_id is None else int(rules_id)), "gvl_set_token_rules")

    def seq_set_token_rules(self, seq: int, rules_id: Optional[int]):
        """gvl_seq_set_token_rules: the rule set of one live sequence (None / -1: none)."""
        self._chk(self.lib.gvl_seq_set_token_rules(self.ctx, int(seq), -1 if rules_id is None else int(rules_id)), "gvl_seq_set_token_rules")

    # ---- decoding grammars (grammar.Grammar -> a device grammar) ---------------------------------------------------
    def grammar_create(self, grammar) -> int:
        """gvl_grammar_create: a grammar.Grammar (or anything with its fields) as an immutable device grammar; returns its id.  Raises GvlError
        (status ERR_ARG, with the library's message) for a description the library's checker refuses."""
        tc = np.ascontiguousarray(np.asarray(grammar.token_class, dtype=np.uint8).reshape(-1))
        cb = np.ascontiguousarray(np.asarray(grammar.class_base, dtype=np.int32).reshape(-1))
        tr = np.ascontiguousarray(np.asarray(grammar.trans, dtype=np.uint16).reshape(-1))
        d = L.GvlGrammarDesc(int(grammar.n_states), int(grammar.n_classes), int(grammar.start), int(grammar.vocab), tc.ctypes.data_as(C.POINTER(C.c_uint8)),
                             cb.ctypes.data_as(C.POINTER(C.c_int32)), tr.ctypes.data_as(C.POINTER(C.c_uint16)))
        gid = C.c_int(-1)
        self._chk(self.lib.gvl_grammar_create(self.ctx, C.byref(d), C.byref(gid)), "gvl_grammar_create")
        return gid.value

    def grammar_destroy(self, grammar_id: int):
        """gvl_grammar_destroy: GvlError (ERR_STATE) while a live sequence or the default still references the grammar."""
        self._chk(self.lib.gvl_grammar_destroy(self.ctx, int(grammar_id)), "gvl_grammar_destroy")

    def set_grammar(self, grammar_id: Optional[int] = None):
        """gvl_set_grammar: the grammar of every sequence allocated AFTER this call (None / -1: none)."""
        self._chk(self.lib.gvl_set_grammar(self.ctx, -1 if grammar_id is None else int(grammar_id)), "gvl_set_grammar")

    def seq_set_grammar(self, seq: int, grammar_id: Optional[int]):
        """gvl_seq_set_grammar: the grammar of one live sequence (None / -1: none)."""
        self._chk(self.lib.gvl_seq_set_grammar(self.ctx, int(seq), -1 if grammar_id is None else int(grammar_id)), "gvl_seq_set_grammar")

    def set_logprobs(self, top_n: Optional[int] = -1):
        """gvl_set_logprobs: log-probabilities of the selected tokens for every sequence allocated AFTER this call.  None / -1 = off, 0 = the selected
        token's, 1 .. 8 = also the top N of the same distribution (include/gvl.h)."""
        self._chk(self.lib.gvl_set_logprobs(self.ctx, -1 if top_n is None else int(top_n)), "gvl_set_logprobs")

    def seq_set_logprobs(self, seq: int, top_n: Optional[int]):
        """gvl_seq_set_logprobs: the setting of one live sequence (overrides the default it was allocated with)."""
        self._chk(self.lib.gvl_seq_set_logprobs(self.ctx, int(seq), -1 if top_n is None else int(top_n)), "gvl_seq_set_logprobs")

    def seq_read_logprobs(self, seq: int, first: int = 0, cap: int = 4096, top: bool = False):
        """gvl_seq_read_logprobs (synchronises the stream): (lp, top_list) of the ids generated by `seq` from index `first` (at most cap); lp: one
        float per id; top_list (top=True; the sequence's top_n >= 1): per id its top_n (id, log-probability) pairs without padding, else None."""
        cap = max(int(cap), 0)
        lp = (C.c_float * max(cap, 1))()
        K = LPR.MAX_TOP
        ti = (C.c_int32 * max(cap * K, 1))() if top else None
        tv = (C.c_float * max(cap * K, 1))() if top else None
        n = C.c_int(0)
        self._chk(self.lib.gvl_seq_read_logprobs(self.ctx, int(seq), int(first), cap, lp, ti, tv, C.byref(n), self.stream), "gvl_seq_read_logprobs")
        m = max(0, min(n.value - first, cap))
        lps = [float(lp[i]) for i in range(m)]
        if not top:
            return lps, None
        return lps, [LPR.top_pairs(ti[i * K:(i + 1) * K], tv[i * K:(i + 1) * K], K) for i in range(m)]

    def op_select_logprobs(self, logits: torch.Tensor, top_n, do_sample: bool = False, temperature: float = 1.0, top_k: int = 0, top_p=None,
                           seed: int = 0, streams=None, steps=None):
        """gvl_op_select_logprobs on fp32 rows [B, n] (B <= 16): (tokens int32 [B], lp f32 [B], top_ids int32 [B, 8], top_lp f32 [B, 8]) on the
        device; row b's setting is top_n[b] (an int applies to every row).  Entries a row does not produce keep their fill (token -1, lp NaN,
        top (-2, NaN))."""
        B, n = logits.shape
        tn = [int(x) for x in (top_n if isinstance(top_n, (list, tuple)) else [top_n] * B)]
        toks = torch.full((B,), -1, dtype=torch.int32, device=self.device)
        lp = torch.full((B,), float("nan"), dtype=torch.float32, device=self.device)
        ti = torch.full((B, LPR.MAX_TOP), -2, dtype=torch.int32, device=self.device)
        tv = torch.full((B, LPR.MAX_TOP), float("nan"), dtype=torch.float32, device=self.device)
        st = (C.c_uint32 * B)(*[int(x) for x in (streams if streams is not None else [0] * B)])
        steps_d = torch.tensor(list(steps) if steps is not None else [0] * B, dtype=torch.int32, device=self.device)
        self._chk(self.lib.gvl_op_select_logprobs(self.ctx, _ptr(logits.contiguous()), n, B, int(bool(do_sample)), float(temperature), int(top_k or 0),
                                                  float(top_p or 0.0), int(seed) & (2 ** 64 - 1), st, _ptr(steps_d), (C.c_int * B)(*tn), _ptr(toks),
                                                  _ptr(lp), _ptr(ti), _ptr(tv), self.stream), "gvl_op_select_logprobs")
        return toks, lp, ti, tv

    def op_dgemm(self, W, x, bias=None):
        """x bf16 [B, K] (B <= 16) -> y f32 [B, N]: the skinny MFMA decode GEMM."""
        N, K = W.shape
        B = x.shape[0]
        y = torch.empty((B, N), dtype=torch.float32, device=self.device)
        self._chk(self.lib.gvl_op_dgemm(self.ctx, _ptr(W.contiguous()), _ptr(x.contiguous()), _ptr(bias), _ptr(y), N, K, B, self.stream), "gvl_op_dgemm")
        return y

    def op_decode_proj(self, W, x, **kw):
        """gvl_op_decode_proj (include/gvl.h): one decode projection with any prologue / epilogue.  W bf16 [N, K], x bf16 [B, K] (or the tiled
        stream with x_is_tiled=1); every other field of gvl_decode_proj by keyword -- tensors for the pointer fields (outputs are written in
        place, the caller allocates and pre-fills them), ints / floats for the rest.  Raises GvlError (status ERR_ARG) on a refusal."""
        for k in ("W", "x", "N", "K"):
            if k in kw:
                raise TypeError(f"gvl_op_decode_proj: unknown field {k}")
        kw = dict(kw, N=W.shape[0], K=W.shape[1], W=W.contiguous(), x=x.contiguous(), batch=int(kw.get("batch", x.shape[0])))
        self._op_desc(L.GvlDecodeProj, self.lib.gvl_op_decode_proj, "gvl_op_decode_proj", kw)

    def op_decode_attention(self, **kw):
        """gvl_op_decode_attention (include/gvl.h): one decode-attention launch.  Every field of gvl_decode_attn by keyword -- device tensors for the
        pointer fields (out, part and counters are written in place: the caller allocates and pre-fills them), ints / floats for the rest.  Raises
        GvlError (status ERR_ARG) on a refusal."""
        self._op_desc(L.GvlDecodeAttn, self.lib.gvl_op_decode_attention, "gvl_op_decode_attention", kw)

    def _op_desc(self, struct, fn, what, kw):
        """fill a descriptor from keywords and call fn: an unknown field raises TypeError, None is skipped, a pointer field takes a contiguous device tensor (kept alive
        over the call); the arrays of a ragged group -- vl_rows / vl_pos0 / table_len: lists of ints, vl_tables: a list of device int32 tensors"""
        d = struct()
        names = {n: t for n, t in struct._fields_}
        keep = []
        if kw.get("vl_tables") is not None and "table_len" not in kw:
            kw = dict(kw, table_len=[int(t.numel()) for t in kw["vl_tables"]])
        for k, v in kw.items():
            if k not in names:
                raise TypeError(f"{what}: unknown field {k}")
            if v is None:
                continue
            if k == "vl_tables":
                for u, t in enumerate(v):
                    if t is not None:
                        assert t.is_contiguous() and t.device.type == "cuda" and t.dtype == torch.int32, k
                        keep.append(t)
                        d.vl_tables[u] = t.data_ptr()
            elif k in ("vl_rows", "vl_pos0", "table_len"):
                for u, x in enumerate(v):
                    getattr(d, k)[u] = int(x)
            elif names[k] is C.c_void_p:
                assert v.is_contiguous() and v.device.type == "cuda", k
                keep.append(v)
                setattr(d, k, v.data_ptr())
            else:
                setattr(d, k, v)
        self._chk(fn(self.ctx, C.byref(d), self.stream), what)

    def op_qkv_post(self, **kw):
        """gvl_op_qkv_post (include/gvl.h): one launch of the qkv_post pass.  Every field of gvl_qkv_post by keyword -- device tensors for the pointer fields (Q, Kt,
        Vt and q_rs are written in place: the caller allocates and pre-fills them), ints / floats for the rest; vl_rows, vl_pos0 and table_len take lists of ints,
        vl_tables a list of device int32 tensors (table_len defaults to their lengths).  Raises GvlError (status ERR_ARG) on a refusal."""
        self._op_desc(L.GvlQkvPost, self.lib.gvl_op_qkv_post, "gvl_op_qkv_post", kw)

    def op_prefill_attention(self, **kw):
        """gvl_op_prefill_attention (include/gvl.h): one paged prefill-attention launch on caller-owned pages.  Every field of gvl_prefill_attn by keyword, as
        op_qkv_post takes them (O is written in place).  Raises GvlError (status ERR_ARG) on a refusal."""
        self._op_desc(L.GvlPrefillAttn, self.lib.gvl_op_prefill_attention, "gvl_op_prefill_attention", kw)

    def op_iv2_attention(self, **kw):
        """gvl_op_iv2_attention (include/gvl.h): the attention launch of one InternVideo2 block on caller-owned buffers.  Every field of gvl_iv2_attn by keyword, as
        op_qkv_post takes them (out is written in place; a pointer field may be a view into a larger allocation).  Raises GvlError (status ERR_ARG) on a refusal."""
        self._op_desc(L.GvlIv2Attn, self.lib.gvl_op_iv2_attention, "gvl_op_iv2_attention", kw)

    def op_gemv(self, W, x, bias=None):
        N, K = W.shape
        y = torch.empty((N,), dtype=torch.float32, device=self.device)
        self._chk(self.lib.gvl_op_gemv(self.ctx, _ptr(W.contiguous()), _ptr(x.contiguous()), _ptr(bias), _ptr(y), N, K, self.stream), "gvl_op_gemv")
        return y
