"""Host-side mirror of the reference's model surface:  LLAVA_NEXT_VIDEO(...).generate(samples, **kw).

Same constructor arguments and `generate()` contract as models/llava_next_video.py:73-89,616-666:
`samples` = {"prompts": [str], "temporal_pixel_values": [bs,F,3,224,224], "spatial_pixel_values":
[bs,S,3,336,336], "video_ids": [...]}; returns List[str].  Everything numeric runs in libgvl.so
(grounded_video_llm_amd.engine); this file only does the text plumbing and the call order.

Differences that are deliberate and documented: 23 CLIP layers instead of 24
(#2), last-row lm_head (#7), paged KV instead of DynamicCache (#8), glb_GN projected once (#5), LoRA
merged at load (#16).  Decoding covers HF generate's modes as the reference forwards them -- greedy, sampling, beam / beam-sample / group beam search, contrastive
search, classifier-free guidance, num_return_sequences --, each on the device; call.py resolves a call's kwargs into its mode once.
"""
from __future__ import annotations

import contextlib
import dataclasses
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import call as C
from . import dist as gdist
from . import logits as LP
from . import logprobs as LPR
from . import prompts as P
from . import weights as Wt
from .call import Mode, beam_groups, fanout_stream, num_return_sequences  # noqa: F401  (the resolvers live in call.py; these names are part of this module's surface)
from .engine import Engine, TowerGeometry

bf = torch.bfloat16


def _row(ids_arr, mask, i: int) -> List[int]:
    """Row i of a padded id batch without its padding."""
    return [int(t) for t, m in zip(ids_arr[i], mask[i]) if m]


class SyntheticTokenizer:
    """Stand-in for the HF tokenizer (tokenizer files are not available offline): whitespace words -> ids by a
    stable hash; the 302 temporal tokens map to the last 302 rows of the vocabulary like `add_tokens` does."""

    def __init__(self, vocab: int, num_temporal_tokens: int = 300, bos_token_id: Optional[int] = 1, eos_token_id: int = 2, pad_token_id: int = 0):
        self.vocab, self.bos_token_id, self.eos_token_id, self.pad_token_id = vocab, bos_token_id, eos_token_id, pad_token_id
        self.added = P.temporal_token_strings(num_temporal_tokens)
        self.base = vocab - len(self.added)
        self.tok2id = {t: self.base + i for i, t in enumerate(self.added)}
        self.id2tok = {v: k for k, v in self.tok2id.items()}

    def __len__(self):
        return self.vocab

    def _word(self, w: str) -> int:
        if w in self.tok2id:
            return self.tok2id[w]
        h = 2166136261
        for ch in w.encode():
            h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
        return 3 + h % (self.base - 3)

    def __call__(self, text: str) -> List[int]:
        import re
        words = re.findall(r"<\d+>|<timestamp_grounding>|\S+", text)
        ids = [self._word(w) for w in words]
        return ([self.bos_token_id] if self.bos_token_id is not None else []) + ids

    def batch_decode(self, batch: Sequence[Sequence[int]], skip_special_tokens: bool = True) -> List[str]:
        out = []
        for ids in batch:
            toks = []
            for i in ids:
                if skip_special_tokens and i in (self.bos_token_id, self.eos_token_id, self.pad_token_id):
                    continue
                toks.append(self.id2tok.get(int(i), f"w{int(i)}"))
            out.append(" ".join(toks))
        return out


def fit_geometry(geometry: TowerGeometry, llm: str, num_frames: int, num_segs: int, max_txt_len: int) -> TowerGeometry:
    """A copy of `geometry` whose limits hold the reference's configuration (frames / segments / max_txt_len): the prefill workspace and
    the RoPE tables must cover the visual prefix plus the longest prompt the reference accepts (llava_next_video.py:622-647).  Shared by
    the model constructor and tools/pack_checkpoint.py, so a packed file's RoPE tables have the max_seq the loader will ask for.
    The paged KV pool is sized from the free HBM (kv_pages = 0) only when the caller left kv_pages at the dataclass default or passed 0;
    an explicit pool that cannot hold one full-length sequence is an error, never silently replaced by "all of the HBM"."""
    g = dataclasses.replace(geometry)
    g.frames_per_seg = num_frames // num_segs
    g.max_segs = max(g.max_segs, num_segs)
    tok_seg = (156 if llm == "phi3.5" else 64) + 16 * g.frames_per_seg + 1
    need = num_segs * tok_seg + max_txt_len
    g.max_prefill = max(g.max_prefill, need)
    g.max_seq = max(g.max_seq, min(need + 256, 131072))
    if g.kv_pages * 64 < need + 256:
        default_pages = TowerGeometry.__dataclass_fields__["kv_pages"].default
        if g.kv_pages in (0, default_pages):
            g.kv_pages = 0                            # 0 = size the paged KV pool from the free HBM (gvl_finalize_weights)
        else:
            raise ValueError(f"kv_pages = {g.kv_pages} ({g.kv_pages * 64} tokens) cannot hold one sequence of {need + 256} tokens "
                             f"({num_segs} segments x {tok_seg} visual tokens + max_txt_len {max_txt_len} + 256 new): pass a larger pool, "
                             "a smaller max_txt_len, or kv_pages = 0 to size the pool from the free HBM")
    return g


def packed_file_metadata(path: str) -> Dict[str, str]:
    """The __metadata__ dict of a `gvl-packed-1` safetensors file (8-byte little-endian header length + JSON header)."""
    import json
    import struct
    with open(path, "rb") as f:
        (n,) = struct.unpack("<Q", f.read(8))
        hdr = json.loads(f.read(n))
    meta = hdr.get("__metadata__") or {}
    if meta.get("format") != "gvl-packed-1":
        raise ValueError(f"{path}: not a gvl packed weight file")
    return meta


class LLAVA_NEXT_VIDEO:
    def __init__(self, dtype=torch.bfloat16, stage="pretrain", max_txt_len=2048, num_frames=96, num_segs=12, lora=False,
                 num_temporal_tokens=300, llm="llama3", attn_implementation="flash_attention_2",
                 config_path="weight_path/Phi-3.5-vision-instruct", tokenizer_path="weight_path/Phi-3.5-mini-instruct",
                 pretrained_video_path="weight_path/internvideo/vision-encoder-InternVideo2-stage2_1b-224p-f4.pt",
                 pretrained_vision_proj_llm_path="weight_path/Phi-3.5-vision-instruct-seperated/",
                 *, geometry: Optional[TowerGeometry] = None, tokenizer=None, state_dicts: Optional[Dict[str, Dict[str, torch.Tensor]]] = None,
                 device: str = "cuda:0", group=None, packed_weights: Optional[str] = None, ckpt_path: Optional[str] = None,
                 exchange: str = "torch"):
        if dtype not in (torch.bfloat16,):
            raise ValueError("the MI355X path computes in bfloat16 (the reference's recommended dtype, README.md:57)")
        if num_frames % num_segs != 0:
            raise ValueError("num_frames must be a multiple of num_segs (einops rearrange at models/llava_next_video.py:530)")
        self.dtype, self.stage, self.max_txt_len = dtype, stage, max_txt_len
        self.num_frames, self.num_segs, self.lora, self.num_temporal_tokens, self.llm = num_frames, num_segs, lora, num_temporal_tokens, llm
        self.group = group
        if exchange not in ("torch", "gvl"):
            raise ValueError("exchange: 'torch' (torch.distributed all_gather_into_tensor) or 'gvl' (libgvl's own RCCL communicator through the C ABI)")
        self.exchange = exchange         # the all-gather of the visual tokens when the segments are sharded over a process group (encode_images)
        if geometry is None:
            geometry = geometry_from_checkpoint_dirs(llm, config_path, pretrained_vision_proj_llm_path, stage, num_temporal_tokens)
        geometry = fit_geometry(geometry, llm, num_frames, num_segs, max_txt_len)     # a COPY: the caller's object is never edited
        if llm == "phi3.5" and geometry.rope_short is None and geometry.rope_orig_max_pos > 0:
            raise ValueError("Phi-3.5 needs its LongRoPE short_factor / long_factor (config.json rope_scaling): Phi3LongRoPEScaledRotaryEmbedding "
                             "applies the short factors and the sqrt(1 + ln(s)/ln(4096)) scale even below 4096 tokens (modeling_phi3.py:380-409); "
                             "pass geometry=TowerGeometry().apply_hf_config(cfg) or a config_path that holds config.json")
        self.geo = geometry
        self.tokenizer = tokenizer
        if self.tokenizer is None:
            try:
                from transformers import AutoTokenizer
                self.tokenizer = AutoTokenizer.from_pretrained(tokenizer_path)
            except Exception as e:   # no network / no files: the caller must inject one
                raise RuntimeError(f"cannot load a tokenizer from {tokenizer_path!r} ({e}); pass tokenizer=...") from e
            if llm == "llama3":
                self.tokenizer.eos_token_id, self.tokenizer.pad_token_id = 128009, 128001   # llava_next_video.py:103-104
            elif llm == "phi3.5":
                self.tokenizer.pad_token = "<|end|>"                                       # :114
            if stage in ("grounded", "sft"):
                self.tokenizer.add_tokens(P.temporal_token_strings(num_temporal_tokens))   # :235-236
        self.engine = Engine(geometry, device)
        self._base_sd = None
        if packed_weights is not None:                    # file written by tools/pack_checkpoint.py: no per-start packing / LoRA merge;
            meta = packed_file_metadata(packed_weights)
            for key, have in (("max_seq", geometry.max_seq), ("frames_per_seg", geometry.frames_per_seg)):
                if key in meta and int(meta[key]) != int(have):
                    raise ValueError(f"{packed_weights}: packed for {key} = {meta[key]} but this model needs {key} = {have} (num_frames / num_segs / "
                                     "max_txt_len differ from the ones given to tools/pack_checkpoint.py: re-pack, or pass the same values)")
            self.engine.load_packed_file(packed_weights)  # read by libgvl itself (gvl_load_packed: mmap + one upload per tensor)
            self.engine.finalize()
            return
        if state_dicts is None:
            state_dicts = load_reference_checkpoints(llm, pretrained_video_path, pretrained_vision_proj_llm_path)
        self._base_sd = state_dicts
        if ckpt_path is not None:                         # inference.py:156-162 in one pass: base + fine-tuned overlay, packed ONCE
            ckpt = torch.load(ckpt_path, map_location="cpu")
            self.load_ckpt(ckpt.get("model", ckpt))
        else:
            self.load_state_dicts(state_dicts)

    # weights -------------------------------------------------------------------------------------------
    def load_state_dicts(self, sd: Dict[str, Dict[str, torch.Tensor]], ckpt_frames: Optional[int] = None):
        g = self.geo
        lm = sd["language_model"]
        if self.stage in ("grounded", "sft"):
            # the constructor of the reference grows the vocabulary BEFORE any fine-tuned weights arrive (reset_embeddings, :231-268)
            ek = next(k for k in lm if k.endswith("embed_tokens.weight"))
            n_new = g.vocab - lm[ek].shape[0]
            if n_new > 0:
                lm = Wt.reset_embeddings(lm, n_new, g.lm_head_bias)
        self.engine.load_packed(Wt.pack_clip(sd["vision_tower"], g.clip_layers - 1))
        self.engine.load_packed(Wt.pack_iv2(sd["video_encoder"], g.iv2_depth - 1, g.frames_per_seg, ckpt_frames,
                                            tokens_per_frame=(g.iv2_image // g.iv2_patch) ** 2))
        self.engine.load_packed(Wt.pack_projectors(sd["projectors"], self.llm))
        self.engine.load_packed(Wt.pack_llm(lm, g.kind, g.layers, g.heads, g.kv_heads, g.max_seq, g.rope_theta,
                                            g.rope_short, g.rope_long, g.rope_max_pos, g.rope_orig_max_pos))
        self.engine.finalize()

    def load_ckpt(self, ckpt: Dict[str, Dict[str, torch.Tensor]], base: Optional[Dict[str, Dict[str, torch.Tensor]]] = None):
        """inference.py:156-162: overlay the fine-tuned groups {multi_modal_projector, video_projecter, language_model} on the base
        state dicts this object was built from (kept in memory: nothing is read from disk twice)."""
        base = base if base is not None else self._base_sd
        if base is None:
            raise RuntimeError("load_ckpt: this model was started from a packed weight file, which holds no base state dicts to overlay; "
                               "pass base=..., or overlay the checkpoint when packing (tools/pack_checkpoint.py --ckpt_path)")
        proj = dict(base["projectors"])
        for grp in ("multi_modal_projector", "video_projecter"):
            for k, v in ckpt.get(grp, {}).items():
                proj[f"{grp}.{k}"] = v
        sd = dict(base)
        sd["projectors"] = proj
        if "language_model" in ckpt:
            sd["language_model"] = ckpt["language_model"]
        self.load_state_dicts(sd)

    # text plumbing ----------------------------------------------------------------------------------------
    def tokenizer_image_token(self, prompt: str) -> List[int]:
        tok = (lambda s: self.tokenizer(s).input_ids) if hasattr(self.tokenizer("x"), "input_ids") else self.tokenizer
        return P.tokenize_with_image(prompt, tok, getattr(self.tokenizer, "bos_token_id", None))

    # vision -------------------------------------------------------------------------------------------------
    def encode_images(self, samples) -> torch.Tensor:
        """[bs, num_segs*L, hidden] bf16.  With a process group, segments are sharded over the ranks and the
        token blocks all-gathered (dist.py)."""
        sp, tp = samples["spatial_pixel_values"], samples["temporal_pixel_values"]
        bs, S = sp.shape[:2]
        fps = tp.shape[1] // S
        sp = sp.reshape(bs * S, *sp.shape[2:])
        tp = tp.reshape(bs, S, fps, *tp.shape[2:]).permute(0, 1, 3, 2, 4, 5).reshape(bs * S, tp.shape[2], fps, *tp.shape[3:])
        n = bs * S
        L = self.engine.tokens_per_seg
        if self.group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1):
            world, rank = torch.distributed.get_world_size(self.group), torch.distributed.get_rank(self.group)
            lo, hi = gdist.my_shard(n, rank, world)
            ms = max(1, self.geo.max_segs)
            parts = [self.engine.encode_segments(sp[i:min(i + ms, hi)], tp[i:min(i + ms, hi)]) for i in range(lo, hi, ms)]   # bs > 1: the shard may exceed max_segs
            local = (torch.cat(parts, 0) if len(parts) > 1 else parts[0]) if parts else torch.empty((0, self.geo.hidden), dtype=bf, device=self.engine.device)
            # the ONE collective of the sharded plan: torch.distributed's all_gather_into_tensor (RCCL), or -- exchange="gvl" -- libgvl's own
            # communicator through the C ABI (gvl_comm_init / gvl_allgather_visual), what a non-Python host of the library calls
            if self.exchange == "gvl" and getattr(self.engine, "comm_world", 0) != world:
                gdist.init_gvl_comm(self.engine, self.group)
            vis = gdist.allgather_visual(local, n, L, self.group, gatherv=self.engine.allgatherv_visual if self.exchange == "gvl" else None)
        else:
            ms = self.geo.max_segs
            if bs > 1 and S <= ms:
                # several samples: the CLIP tower takes as many key frames per call as the workspace allows (its GEMMs are small:
                # +1.6 % clips/s in bench.py), InternVideo2 + projectors run per sample (batching them further is slower).
                # Every kernel is batch-invariant, so the tokens are bit-identical to per-sample encodes.
                cf = torch.cat([self.engine.clip_encode(sp[i:i + ms]) for i in range(0, n, ms)], 0)
                chunks = [self.engine.build_visual(cf[i:i + S], self.engine.iv2_encode(tp[i:i + S])) for i in range(0, n, S)]
            else:
                chunks = [self.engine.encode_segments(sp[i:i + ms], tp[i:i + ms]) for i in range(0, n, ms)]
            vis = torch.cat(chunks, 0) if len(chunks) > 1 else chunks[0]
        return vis.view(bs, S * L, self.geo.hidden)

    # generate -----------------------------------------------------------------------------------------------
    def _resolve(self, kw, entry: str, n: int) -> "C.Call":
        tk = getattr(self, "tokenizer", None)     # the argument errors need none; an unseeded call draws from torch's CPU generator: torch.manual_seed governs it, as HF's
        return C.resolve_call(kw, entry=entry, n_samples=n, eos_id=getattr(tk, "eos_token_id", None), pad_id=getattr(tk, "pad_token_id", 0) or 0,
                              vocab=self.geo.vocab, draw_seed=lambda: int(torch.randint(0, 2 ** 62, (1,)).item()))

    def _check_guidance(self, kw, n: int) -> Optional[float]:     # the scale of a guided call of n samples (None: off), after call.check_guidance's checks
        return C.check_guidance(kw, n, self.geo.vocab)[0]

    @contextlib.contextmanager
    def _settings(self, call: "C.Call", procs: "LP.Processors" = LP.OFF):
        """The engine's settings for the length of one call: writes the five defaults on EVERY call -- log-probabilities, processors (`procs`), sampling, token rules,
        grammar; off where the call leaves them out, so nothing carries over from one call to the next -- and creates the call's device rule set and grammar; yields
        their two ids (None: none); clears the two defaults and destroys the two objects on the way out.  A search (not call.device_selects) gets every default off:
        it hands the processors and the two ids to its own processing of the rows.  A rule set beyond the device's capacities is refused by Engine.rules_create."""
        eng, on = self.engine, call.device_selects
        eng.set_logprobs(call.logprobs.top_n if on else -1)
        eng.set_logits_processors(*(procs if on else LP.OFF).args())
        eng.set_sampling(*call.sampling_args, **call.warpers)
        eng.set_token_rules(None)
        rid = gid = None
        if call.rules.active:
            rid = eng.rules_create(call.rules)
            if on:
                eng.set_token_rules(rid)
        try:
            eng.set_grammar(None)
            if call.grammar is not None:
                gid = eng.grammar_create(call.grammar)
                if on:
                    eng.set_grammar(gid)
            yield rid, gid
        finally:
            eng.set_grammar(None)
            if gid is not None:
                eng.grammar_destroy(gid)
            eng.set_token_rules(None)
            if rid is not None:
                eng.rules_destroy(rid)

    def _negative_embeds(self, call: "C.Call", feats) -> List[torch.Tensor]:
        """The negative prompts of a guided call as embedding rows, one tensor per sample.  negative_ids: the ids' embedding rows (what HF runs as the unconditional
        branch of an inputs_embeds prompt).  negative_texts: tokenised and truncated like the prompts; a string with the <image> slot is spliced with the sample's own
        visual rows (a negative instruction about the same video), one without is text-only (the video-free contrast)."""
        eng = self.engine
        if call.negative_ids is not None:
            return [eng.embed_ids(r) for r in call.negative_ids]
        out = []
        for b, t in enumerate(call.negative_texts):
            row = _row(*P.left_pad_truncate([self.tokenizer_image_token(t)], call.pad_id, self.max_txt_len), 0)
            if sum(1 for x in row if x == P.IMAGE_TOKEN_INDEX) > 1 or not row:
                raise ValueError("generate(): a negative prompt holds at most one <image> slot and at least one token")
            out.append(eng.splice(row, feats[b]) if P.IMAGE_TOKEN_INDEX in row else eng.embed_ids(row))
        return out

    def _decode_in_pool_groups(self, n: int, plan, max_new: int, logprobs: Optional[int], launch=None):
        """Items 0 .. n - 1, as many at once as the KV pool holds.  plan(i) -> (capacities, begin): item i needs one sequence per capacity -- a single one, or a
        leader and its follower --, allocated in that order; begin(seqs) then sets them up.  An item the pool has no room for (ERR_OOM from seq_alloc) closes the
        group once at least one item is in: what fits runs, the rest in the next group.  A closed group: launch(firsts, what every begin returned), if given; the
        items' first sequences decode together; all are freed, the first sequences first -- freeing a leader unbinds its pair.  Returns what generate_ids returns."""
        from .lib import GvlError, ERR_OOM
        eng, eos = self.engine, getattr(self.tokenizer, "eos_token_id", None)
        out, lps, b = [], [], 0
        while b < n:
            live, begun = [], []                         # per admitted item: its sequences; what its begin returned
            try:
                while b + len(live) < n:
                    caps, begin = plan(b + len(live))
                    seqs: List[int] = []
                    try:
                        for cap in caps:
                            seqs.append(eng.seq_alloc(cap))
                    except GvlError as e:
                        for s in seqs:
                            eng.seq_free(s)
                        if e.status == ERR_OOM and live:
                            break
                        raise
                    live.append(seqs)
                    begun.append(begin(seqs))
                firsts = [seqs[0] for seqs in live]
                if launch is not None:
                    launch(firsts, begun)
                got = eng.decode_greedy_batch(firsts, max_new, eos)
                if logprobs is not None:
                    lps += [eng.seq_read_logprobs(s, 0, len(g), top=logprobs > 0) for s, g in zip(firsts, got)]
                out += got
            finally:
                for s in [seqs[0] for seqs in live] + [s for seqs in live for s in seqs[1:]]:
                    eng.seq_free(s)
            b += len(live)
        return out if logprobs is None else (out, lps)

    def guided_generate_ids(self, ids_arr, mask, feats, negatives: Sequence[torch.Tensor], scale: float, max_new: int, processors=None, logprobs: Optional[int] = None,
                            rules: Optional[int] = None, grammar: Optional[int] = None):
        """generate_ids with classifier-free guidance: sample i is decoded against negatives[i] (embedding rows) at `scale`.  Each sample becomes a PAIR of sequences:
        both are prefilled, Engine.seq_set_guidance binds them and re-selects the first token from the guided row, and the pairs decode together -- the negative
        sequence is one more row of the leader's decode step (one weight stream for both).  Processors, rules, grammar, sampling and log-probabilities are the
        conditional sequence's and apply to the guided row: both prefills run with every setting off (a prefill's last logits are the row its own selection saw, and guidance
        needs the RAW rows), then the leader takes the call's processors, rule set `rules` and grammar `grammar`.  Returns what generate_ids returns."""
        eng = self.engine
        n = ids_arr.shape[0]
        opts = [LP.SeqOptions(p if p is not None else LP.OFF, -1 if logprobs is None else logprobs, rules, grammar=grammar)
                for p in (processors if isinstance(processors, (list, tuple)) else [processors] * n)]

        def plan(i):
            emb = eng.splice(_row(ids_arr, mask, i), feats[i])
            room = min(max_new, self.geo.max_seq - max(emb.shape[0], negatives[i].shape[0]))
            if room < 1:
                raise ValueError(f"generate(): sample {i}: the prompt (or its negative) leaves no room below max_seq {self.geo.max_seq}")

            def begin(pair):
                s, f = pair
                LP.apply_seq_options(eng, s, LP.SeqOptions.OFF)
                LP.apply_seq_options(eng, f, LP.SeqOptions.OFF)     # the follower selects nothing: it is handed the leader's tokens
                lc, lu = eng.prefill(s, emb, want_logits=True), eng.prefill(f, negatives[i], want_logits=True)
                LP.apply_seq_options(eng, s, opts[i])
                eng.seq_set_guidance(s, f, scale, lc, lu)
            return (emb.shape[0] + room, negatives[i].shape[0] + room), begin
        return self._decode_in_pool_groups(n, plan, max_new, logprobs)

    def fanout_generate_ids(self, ids_arr, mask, feats, max_new: int, n: int, sampling: dict, processors=None, logprobs: Optional[int] = None, prompt_index=None):
        """n sampled answers per row from ONE prefill per row: the row is spliced and prefilled once, Engine.seq_fanout makes n - 1 siblings that share the prompt's KV
        pages (in parts of at most 15 siblings), and source and siblings decode together (decode_greedy_batch groups them: one weight stream per token for up to 16 answers).
        Answer j of row p draws from stream fanout_stream(p, j) of sampling["seed"], whatever n is and whatever fits the KV pool at once: when the pool cannot hold all
        siblings the remaining answers start from another prefill of the same prompt -- a sibling is bit for bit an independent sequence on its stream, so the answers
        do not change.  prompt_index: the p of every row (default: its position).  Processors, rules, grammar and log-probabilities apply per answer.
        Returns the ids prompt-major (n per row); with logprobs (ids, lps) as generate_ids.  (Not _decode_in_pool_groups: a full pool halves the part, then re-prefills the row.)"""
        from .lib import GvlError, ERR_OOM
        eos = getattr(self.tokenizer, "eos_token_id", None)
        eng = self.engine
        rows = ids_arr.shape[0]
        procs = processors if isinstance(processors, (list, tuple)) else [processors] * rows
        out: List[List[int]] = []
        lps = []
        for i in range(rows):
            p = i if prompt_index is None else int(prompt_index[i])
            emb = eng.splice(_row(ids_arr, mask, i), feats[i])
            cap = min(emb.shape[0] + max_new, self.geo.max_seq)
            done = 0
            while done < n:
                opts = LP.SeqOptions(procs[i], logprobs, sampling=dict(sampling, stream=fanout_stream(p, done)))
                group: List[int] = []
                try:
                    group.append(eng.seq_alloc(cap))
                    LP.apply_seq_options(eng, group[0], opts)
                    first = eng.prefill(group[0], emb, want_logits=True)
                    while done + len(group) < n:
                        part = min(15, n - done - len(group))
                        while part >= 1:                   # all or nothing per call: halve until it fits
                            try:
                                group += eng.seq_fanout(group[0], part, cap, [fanout_stream(p, done + len(group) + j) for j in range(part)], first)
                                break
                            except GvlError as e:
                                if e.status != ERR_OOM:
                                    raise
                                part //= 2
                        if part < 1:
                            break                          # pool (or slots) full: decode what fits, the rest behind another prefill
                    got = eng.decode_greedy_batch(group, max_new, eos)
                    if logprobs is not None:
                        lps += [LP.read_seq_logprobs(eng, s_, g, opts) for s_, g in zip(group, got)]
                    out += got
                finally:
                    for s_ in group:
                        eng.seq_free(s_)
                done += len(group)
        return out if logprobs is None else (out, lps)

    def _n_visual(self, samples) -> int:
        return int(samples["spatial_pixel_values"].shape[1]) * self.engine.tokens_per_seg

    @torch.inference_mode()
    def generate(self, samples, **generate_kwargs):
        """The reference's generate(samples, **generate_kwargs) -> the answers' texts, or with return_dict_in_generate=True a logprobs.GenerateOutput (texts,
        sequences and, with output_scores / top_logprobs, per-token log-probabilities).  call.resolve_call turns the kwargs into one call.Call -- raising every
        argument error before any work -- and the call's mode decides what runs:

          mode          kwargs (HF's unless marked extra)                       runs                         Call fields
          greedy        (none)                                                  generate_ids                 --
          sample        do_sample, temperature, top_k, top_p, min_p, typical_p, generate_ids                 sampling_args, warpers
                        epsilon_cutoff, eta_cutoff, seed (extra)
          fan-out       do_sample with num_return_sequences = n                 fanout_generate_ids          n_return, seq_sampling
          guided        guidance_scale != 1 with negative_prompt_ids (+ mask)   guided_generate_ids          guidance, negative_ids / negative_texts
                        or negative_prompts (extra); greedy or sampled
          beam          num_beams = k > 1, length_penalty, early_stopping,      beam_generate_ids            num_beams, beam_impl, length_penalty,
                        num_return_sequences <= k, beam_impl (extra)                                         early_stopping, n_return
          beam-sample   ... with do_sample; beam_impl "host" only               beam_generate_ids            beam_sample
          group-beam    ... with num_beam_groups = G > 1, diversity_penalty > 0 beam_generate_ids            groups
          contrastive   penalty_alpha in (0, 1] with top_k in 2 .. 16           contrastive_generate_ids     contrastive

        In every mode, on the device and in HF's order (logits.py), guidance in front: repetition_penalty, no_repeat_ngram_size, min_new_tokens / min_length
        (Call.processors); sequence_bias, bad_words_ids, forced_eos_token_id, suppress_tokens, begin_suppress_tokens (Call.rules); grammar (extra: a grammar.Grammar in
        the place of HF's prefix_allowed_tokens_fn, which itself is refused); max_new_tokens; return_dict_in_generate, output_scores, top_logprobs (extra;
        Call.logprobs).  The first four modes let the device's own selection apply them (Call.device_selects), a search applies them to its own rows; the method
        that runs a mode says what it returns as scores.  Combinations that are not built raise ValueError.  Other HF kwargs are ignored."""
        if any(v == "text" for v in samples.get("video_ids", [])):
            # prepare_multimodal_inputs' `video_ids == 'text'` branch (llava_next_video.py:583-586) is a TRAINING device (dummy visual
            # rows appended with mask 0 so FSDP sees every parameter); the reference's inference never produces it.  forward() handles it.
            raise ValueError("generate(): 'text' samples are a training-only construct of the reference; use forward() for them")
        call = self._resolve(generate_kwargs, "generate", len(samples["prompts"]))
        ids_arr, mask = P.left_pad_truncate([self.tokenizer_image_token(t) for t in samples["prompts"]], call.pad_id, self.max_txt_len)
        procs = call.processors(LP.padded_embed_len(ids_arr.shape[1], self._n_visual(samples)))
        with self._settings(call, procs) as (rid, gid):
            return self._generate(call, samples, ids_arr, mask, procs, rid, gid)

    def _generate(self, call: "C.Call", samples, ids_arr, mask, procs, rid: Optional[int], gid: Optional[int]):
        feats = self.encode_images(samples)
        n, max_new, want = ids_arr.shape[0], call.max_new, call.want_logprobs
        scored = call.logprobs.return_dict and call.logprobs.output_scores
        if call.mode is Mode.CONTRASTIVE:                 # one sample at a time, like beams
            res = [self.contrastive_generate_ids(_row(ids_arr, mask, b), feats[b], *call.contrastive, max_new, processors=procs, rules=rid, grammar=gid, with_scores=scored)
                   for b in range(n)]
            if not scored:
                return self._output(call, res)
            out = self._output(call, [r[0] for r in res], [(r[1], None) for r in res])
            out.degeneration_penalties = [list(r[2]) for r in res]
            return out
        if not call.device_selects:                       # beam, beam-sample, group-beam: one sample at a time
            sample = call.beam_sample                     # HF _beam_sample: the warpers' arguments as generate() takes them; one generator per call
            if sample is not None:
                sample = dict(sample, generator=torch.Generator(device=self.engine.device).manual_seed(sample["seed"]))
            G, lam = call.groups or (1, 0.0)
            out_ids = [self.beam_generate_ids(_row(ids_arr, mask, b), feats[b], call.num_beams, max_new, call.length_penalty, call.early_stopping, sample,
                                              processors=procs, with_scores=scored, rules=rid, impl=call.beam_impl, grammar=gid, num_return=call.n_return,
                                              num_beam_groups=G, diversity_penalty=lam)
                       for b in range(n)]
            if call.n_return > 1:                         # the n best hypotheses of every prompt, prompt-major
                out_ids = [r for per_prompt in out_ids for r in per_prompt]
            if scored:                                    # (ids, sequences_score, transition_scores) per hypothesis
                return self._output(call, [r[0] for r in out_ids], [(r[2], None) for r in out_ids], [r[1] for r in out_ids])
            return self._output(call, out_ids)
        if call.mode is Mode.GUIDED:                      # every sample decodes as a pair with its negative
            res = self.guided_generate_ids(ids_arr, mask, feats, self._negative_embeds(call, feats), call.guidance, max_new, processors=procs, logprobs=want,
                                           rules=rid, grammar=gid)
        elif call.mode is Mode.FANOUT:                    # n sampled answers per prompt from ONE prefill each (gvl_seq_fanout), prompt-major
            res = self.fanout_generate_ids(ids_arr, mask, feats, max_new, call.n_return, call.seq_sampling, processors=procs, logprobs=want)
        else:
            res = self.generate_ids(ids_arr, mask, feats, max_new, processors=procs, logprobs=want)
        return self._output(call, *(res if want is not None else (res, None)))

    def _output(self, call: "C.Call", out_ids, lps=None, beam_scores=None):      # the new ids of every answer -> generate()'s return value
        texts = [t.strip() for t in self.tokenizer.batch_decode(out_ids, skip_special_tokens=True)]
        return LPR.build_output(texts, [list(x) for x in out_ids], call.logprobs, lps, beam_scores) if call.logprobs.return_dict else texts

    @contextlib.contextmanager
    def _search_seq(self, row: List[int], vis: torch.Tensor, grammar: Optional[int], keep_hidden: bool = False):
        """(seq, first logits): the prompt prefilled once into a sequence of its own for a search inside the library -- every option off but the grammar, which the
        search reads from it -- and freed on the way out."""
        eng = self.engine
        emb = eng.splice(row, vis)
        seq = eng.seq_alloc(min(emb.shape[0], self.geo.max_seq))
        try:
            LP.apply_seq_options(eng, seq, dataclasses.replace(LP.SeqOptions.OFF, grammar=grammar))
            if keep_hidden:
                eng.seq_keep_hidden(seq)
            yield seq, eng.prefill(seq, emb, want_logits=True)
        finally:
            eng.seq_free(seq)

    def contrastive_generate_ids(self, row: List[int], vis: torch.Tensor, top_k: int, penalty_alpha: float, max_new: int, processors: Optional["LP.Processors"] = None,
                                 rules: Optional[int] = None, grammar: Optional[int] = None, with_scores: bool = False):
        """generate(penalty_alpha = a, top_k = k): HF contrastive search (tests/contrastive_ref.py restates transformers 4.40.1's) inside the library
        (Engine.contrastive_search = gvl_contrastive_search).  The prompt is prefilled once into a keep-hidden sequence -- its bank holds the post-final-norm hidden state
        of every prompt row, the visual ones included --; per token the k most probable ids advance k sequences (the current one and k - 1 clones sharing its KV pages)
        by one batched decode step, and the device ranks score = (1 - a) p - a max_j cos(h, h_j) over the bank.  Deterministic: no seed, one answer.  processors / rules:
        applied to every step's raw logits row before the softmax (HF's order), history = the ids chosen so far; grammar: the search sequence carries it.  No warpers.
        with_scores: (ids, p per id, degeneration penalty per id)."""
        eng = self.engine
        eos = getattr(self.tokenizer, "eos_token_id", None)
        procs = processors if processors is not None and processors.active else None
        with self._search_seq(row, vis, grammar, keep_hidden=True) as (seq, first):
            if not with_scores:
                return eng.contrastive_search(seq, first, top_k, penalty_alpha, max_new, eos, procs, rules)
            ids, tr = eng.contrastive_search(seq, first, top_k, penalty_alpha, max_new, eos, procs, rules, with_trace=True)
            return ids, [tr["p"][s][r] for s, r in enumerate(tr["sel"])], [tr["pen"][s][r] for s, r in enumerate(tr["sel"])]

    def beam_generate_ids(self, row: List[int], vis: torch.Tensor, num_beams: int, max_new: int, length_penalty: float = 1.0, early_stopping=False,
                          sample: Optional[dict] = None, processors: Optional["LP.Processors"] = None, with_scores: bool = False,
                          rules: Optional[int] = None, impl: str = "host", grammar: Optional[int] = None, num_return: int = 1,
                          num_beam_groups: int = 1, diversity_penalty: float = 0.0):
        """num_beam_groups / diversity_penalty: anything but (1, 0.0) is diverse (group) beam search (beam.group_beam_search / gvl_group_beam_search) with the
        tokenizer's pad_token_id as the token of a finished group's beams; on the host path the Hamming term is subtracted in torch, or -- when processors, rules or a
        grammar are active -- inside the processor launch, in HF's place.
        num_return > 1: a list of results, the num_return best hypotheses, best first (beam.beam_search's num_return / gvl_beam_search_n).
        generate(num_beams = k, do_sample = False): HF beam search (beam.py restates transformers 4.40.1's scorer) on the paged KV cache.  The k running
        beams are k sequences; HF's per-step cache reorder becomes gvl_seq_clone -- a beam that continues another one shares its whole KV pages by
        reference and copies only the partial last page; the first child of a parent simply keeps the parent's sequence.  All beams advance by ONE
        teacher-forced batched decode step per token (gvl_decode_step_logits_batch: one stream of the weights for the k beams); log-softmax / top-2k of the step run on the device (torch), the bookkeeping on
        the host.  processors: HF's logits processors, applied by gvl_op_logits_process to every step's log-softmax rows before the beam scores
        are added (HF _beam_search / _beam_sample); the beams' own sequences select their tokens without them (their raw logits are what the
        steps return).  rules: a rule-set id (Engine.rules_create) applied in the same pass, in HF's order; grammar: a grammar id (Engine.grammar_create), likewise --
        every beam's row is masked by the walk over that beam's own ids (impl = "device": the search sequence carries the grammar, gvl_beam_search reads it).  with_scores: (ids, sequences_score, transition_scores) as beam.beam_search returns them.
        impl = "device": the same search inside the library (Engine.beam_search = gvl_beam_search: bookkeeping in C++, every step's log-softmax and top-2k in the
        library's kernels, the processors / rules by the same launch); beam search only (sample must be None)."""
        from . import beam as B
        eng = self.engine
        if impl not in ("host", "device"):
            raise ValueError(f"beam search: impl must be 'host' or 'device', not {impl!r}")
        grouped = B.check_groups(num_beams, num_beam_groups, diversity_penalty, sample is not None)
        pad = getattr(self.tokenizer, "pad_token_id", None)
        if impl == "device":
            if sample is not None:
                raise ValueError("beam-sample runs on the host path only (its draws are torch's): impl='device' needs sample=None")
            eos = getattr(self.tokenizer, "eos_token_id", None)
            procs = processors if processors is not None and processors.active else None
            with self._search_seq(row, vis, grammar) as (seq, first):
                if grouped:
                    return eng.group_beam_search(seq, first, num_beams, num_beam_groups, diversity_penalty, max_new, eos, pad, length_penalty, early_stopping,
                                                 procs, rules, with_scores, num_return=num_return)
                return eng.beam_search(seq, first, num_beams, max_new, eos, length_penalty, early_stopping, procs, rules, with_scores, num_return=num_return)
        gi = eng.decode_group_info()                     # which group sizes ONE batched step takes: asked from the library, not restated here
        eos = getattr(self.tokenizer, "eos_token_id", None)
        emb = eng.splice(row, vis)
        cap = min(emb.shape[0] + max_new + 1, self.geo.max_seq)
        beams: List[Optional[int]] = [eng.seq_alloc(cap)]
        fresh: List[int] = []                            # clones of the step in progress: owned here until they are installed in `beams`
        process = None
        if (processors is not None and processors.active) or rules is not None or grammar is not None:
            pa = (processors if processors is not None else LP.OFF).args()

            opt = {name: v for name, v in (("rules", rules), ("grammar", grammar)) if v is not None}     # only what is set: op_logits_process defaults the rest

            def process(histories: List[List[int]], logprobs: torch.Tensor, group: int = 0, prev_tokens=(), diversity_penalty: float = 0.0) -> torch.Tensor:
                # a later group of diverse beam search: the Hamming term rides in the same launch, in HF's place
                ham = {"hamming": (list(prev_tokens), float(diversity_penalty))} if group > 0 else {}
                return eng.op_logits_process(logprobs.float().contiguous(), histories, *pa, **opt, **ham)
        try:
            LP.apply_seq_options(eng, beams[0], LP.SeqOptions.OFF)    # the steps must hand back raw logits, the scores come from the host rows (beam.py); clones copy these settings
            first = eng.prefill(beams[0], emb, want_logits=True)

            def step(parents: List[Optional[int]], toks: List[int]) -> torch.Tensor:
                # beam.reorder's plan over the sequences; a finished group's beams (parent None) are freed and their rows stay zero -- nothing reads them
                src, clones, closed = B.reorder(beams, parents)
                new: List[Optional[int]] = [None] * len(parents)
                for j in clones:                             # clones first: every parent is still at the length the children continue from
                    new[j] = eng.seq_clone(beams[src[j]], cap)
                    fresh.append(new[j])                     # if a later clone raises (pool exhausted, kMaxSeqs), `finally` frees these
                for j, p_ in enumerate(src):
                    if p_ is not None and new[j] is None:
                        new[j] = beams[p_]
                losers = [beams[q] for q in closed]
                beams[:] = new                               # install before freeing: `finally` never sees an id twice or a freed id
                del fresh[:]
                for s_ in losers:
                    eng.seq_free(s_)
                live = [j for j, s_ in enumerate(beams) if s_ is not None]
                ls, lt = [beams[j] for j in live], [toks[j] for j in live]
                if len(ls) <= gi["max_group"] and (gi["any_size"] or len(ls) in (1, 2, 4)):
                    got = eng.decode_step_logits_batch(ls, lt)              # the live beams share ONE stream of the weights
                else:
                    got = torch.stack([eng.decode_step_logits(s_, t) for s_, t in zip(ls, lt)])
                if len(live) == len(beams):
                    return got
                out = torch.zeros((len(parents), got.shape[-1]), dtype=torch.float32, device=got.device)
                out[torch.as_tensor(live, device=got.device)] = got
                return out

            return B.beam_search(step, first, num_beams, max_new, eos, length_penalty, early_stopping, sample, process=process, with_scores=with_scores, num_return=num_return,
                                 num_beam_groups=num_beam_groups, diversity_penalty=diversity_penalty, pad_id=pad)
        finally:
            for s_ in set(x for x in list(beams) + fresh if x is not None):
                try:
                    eng.seq_free(s_)
                except Exception:                            # never mask the original error with a cleanup error
                    pass

    @torch.inference_mode()
    def generate_shared(self, samples, prompts: Sequence[str], **generate_kwargs):
        """Several prompts about ONE video.  The reference's inference.py calls generate() once per prompt (grounding / QA /
        referring, inference.py:178-182) and re-runs both vision towers every time; here the video is encoded once and the prompts
        are prefilled and decoded together.  Texts are identical to one generate() call per prompt (batch-invariant kernels) -- the logits
        processors included: each prompt gets its own (its min_length is lowered by its own embedding length, as its own reference call would).
        Modes greedy, sample and fan-out (call.resolve_call, entry "generate_shared"); return_dict_in_generate / output_scores / top_logprobs as in generate()."""
        if samples["spatial_pixel_values"].shape[0] != 1:
            raise ValueError("generate_shared takes the pixel tensors of one video")
        call = self._resolve(generate_kwargs, "generate_shared", len(prompts))
        ids_arr, mask = P.left_pad_truncate([self.tokenizer_image_token(t) for t in prompts], call.pad_id, self.max_txt_len)
        rows = [_row(ids_arr, mask, i) for i in range(len(prompts))]
        n_vis = self._n_visual(samples)
        procs = [call.processors(LP.padded_embed_len(len(r), n_vis)) for r in rows]
        max_new, want = call.max_new, call.want_logprobs
        with self._settings(call, procs[0] if procs else call.processors(0)):       # rules and grammar: every sequence allocated below starts with them
            feats = self.encode_images(samples)
            # num_return_sequences = n: every prompt's sequence is fanned out behind its own (extend-)prefill.  Every prompt stands for a generate() call of its own,
            # so each draws from the streams of prompt index 0: the n answers of a prompt equal generate(num_return_sequences=n) on that prompt alone
            fan = (call.n_return, call.seq_sampling) if call.mode is Mode.FANOUT else None
            res = self._generate_shared_prefix(rows, feats[0], max_new, procs, logprobs=want, fanout=fan)
            if res is None and fan is not None:
                res = self.fanout_generate_ids(ids_arr, mask, feats.expand(len(prompts), -1, -1), max_new, fan[0], fan[1], processors=procs, logprobs=want,
                                               prompt_index=[0] * len(prompts))
            elif res is None:                            # nothing worth sharing (one prompt, or the prompts part ways before 128 tokens)
                res = self.generate_ids(ids_arr, mask, feats.expand(len(prompts), -1, -1), max_new, processors=procs, logprobs=want)
        return self._output(call, *(res if want is not None else (res, None)))


    def _shared_prefix(self, rows: Sequence[Sequence[int]], n_vis: int, lens: Sequence[int], limit: int) -> int:
        """THE shared-prefix rule of generate_shared and score: how many leading EMBEDDING rows the id rows `rows` (one image slot each, n_vis visual rows) have in
        common, at most `limit`, rounded down to 128 (whole KV pages AND whole query blocks, so that every later row is computed exactly as in a full prefill); 0 =
        nothing worth sharing (one row, rows that part ways before 128, or the LongRoPE condition below).  lens: the rows each sequence will hold in the end."""
        if len(rows) < 2:
            return 0
        # common prefix in EMBEDDING rows: ids before the image slot must agree, then the visual rows, then the ids after it
        k = list(rows[0]).index(P.IMAGE_TOKEN_INDEX)
        if any(list(r[:k + 1]) != list(rows[0][:k + 1]) for r in rows):
            return 0
        tail = 0
        while all(k + 1 + tail < len(r) for r in rows) and len({r[k + 1 + tail] for r in rows}) == 1:
            tail += 1
        prefix = min(k + n_vis + tail, limit) // 128 * 128
        if prefix < 128:
            return 0
        # LongRoPE (modeling_phi3.py:381-385) picks ONE factor set per forward from the TOTAL length: a full prefill of a prompt longer than
        # original_max_position_embeddings ropes every row -- the shared ones too -- with the long factors, while a base prefill of a prefix
        # that still fits the original context would cache its K with the short ones.  Share only when base and forks agree.
        omax = self.geo.rope_orig_max_pos if self.geo.rope_long is not None else 0
        if omax > 0 and prefix <= omax and any(n > omax for n in lens):
            return 0
        return prefix

    def _generate_shared_prefix(self, rows: List[List[int]], vis: torch.Tensor, max_new: int,
                                processors: Optional[List["LP.Processors"]] = None, logprobs: Optional[int] = None, fanout=None):
        """Prompts about one video share the system prompt and the visual tokens: the common prefix (rounded down to 128 tokens = whole KV pages AND
        whole query blocks, so that every later row is computed exactly as in a full prefill) is prefilled ONCE; every prompt forks it
        (gvl_seq_fork: pages referenced, not copied) and only its own tail is prefilled -- the tails of up to 8 prompts in one ragged decoder pass
        (gvl_prefill_extend_varlen: the weights are streamed once per group, not once per prompt); the answers are decoded together.
        Ids are bit-identical to one full prefill per prompt.  logprobs: as in generate_ids (then (ids, lps) is returned).
        fanout: None, or (n, sampling) -- n sampled answers per prompt: every fork takes `sampling` (fanout_generate_ids') on stream fanout_stream(0, 0) and, behind its
        tail's prefill, n - 1 siblings (Engine.seq_fanout) on the streams fanout_stream(0, j); the answers come back prompt-major.  When the KV pool cannot hold all of
        them at once: None, and the caller takes the per-prompt path."""
        eng = self.engine
        self.last_shared_prefix = 0                      # tokens prefilled once for all prompts in the last generate_shared call (0 = not shared)
        if len(rows) < 2:
            return None
        embs = [eng.splice(r, vis) for r in rows]
        lens = [e.shape[0] for e in embs]
        prefix = self._shared_prefix(rows, vis.shape[0], lens, min(lens) - 1)     # every prompt keeps at least one row of its own (its last row feeds the first token)
        if not prefix:
            return None
        self.last_shared_prefix = prefix
        eos = getattr(self.tokenizer, "eos_token_id", None)
        from .lib import GvlError, ERR_OOM
        n = fanout[0] if fanout else 1
        own = dict(sampling=dict(fanout[1], stream=fanout_stream(0, 0))) if fanout else {}
        opts = [LP.SeqOptions(p, logprobs, **own) for p in (processors or [None] * len(rows))]
        base, seqs, sibs = None, [], []
        try:
            base = eng.seq_alloc(prefix)
            eng.prefill(base, embs[0][:prefix])
            for o, e in zip(opts, embs):
                seqs.append(eng.seq_fork(base, prefix, min(e.shape[0] + max_new, self.geo.max_seq)))
                LP.apply_seq_options(eng, seqs[-1], o)
            firsts = []
            for g in range(0, len(seqs), 8):                 # all tails of a group in ONE decoder pass (each exactly as its own gvl_prefill_extend)
                firsts.append(eng.prefill_extend_batch(seqs[g:g + 8], [e[prefix:] for e in embs[g:g + 8]], want_logits=n > 1))
            order = list(seqs)
            if n > 1:
                try:
                    order = []
                    for i, (s_, e) in enumerate(zip(seqs, embs)):
                        order.append(s_)
                        first = firsts[i // 8][i % 8].contiguous()
                        for j0 in range(1, n, 15):
                            new = eng.seq_fanout(s_, min(15, n - j0), min(e.shape[0] + max_new, self.geo.max_seq), [fanout_stream(0, j) for j in range(j0, min(n, j0 + 15))], first)
                            sibs += new
                            order += new
                except GvlError as e:
                    if e.status == ERR_OOM:
                        self.last_shared_prefix = 0
                        return None
                    raise
            got = eng.decode_greedy_batch(order, max_new, eos)
            if logprobs is None:
                return got
            return got, [LP.read_seq_logprobs(eng, s_, g, opts[0]) for s_, g in zip(order, got)]
        finally:
            for s_ in sibs + seqs:
                eng.seq_free(s_)
            if base is not None:
                eng.seq_free(base)

    @torch.inference_mode()
    def score(self, samples, prompts: Sequence[str], continuations: Optional[Sequence[str]] = None, continuation_ids: Optional[Sequence[Sequence[int]]] = None,
              top_logprobs: Optional[int] = None, append_eos: bool = False, *, share_prefix: bool = True) -> List["SC.ScoreOutput"]:
        """How likely the model finds GIVEN answers about ONE video: pair i = (prompts[i], continuations[i]) -> a scoring.ScoreOutput (per-token log-probabilities
        and ranks of the continuation's ids under teacher forcing, their sum and mean, and with top_logprobs = N the N best alternatives per position).  A
        multiple-choice question passes the same prompt k times with the k options; ranking needs no sampling.  continuations are tokenised without BOS (or pass
        continuation_ids); append_eos also scores the closing EOS.  The distribution is the raw model's: no logits processors, token rules or warpers.
        One vision encode; the pairs share their common prefix as generate_shared's prompts do (_shared_prefix: one base prefill, forks), then up to 8 pairs run
        their remaining rows in ONE ragged decoder pass that scores on the way (Engine.score_extend_batch); with nothing to share the same call runs on empty
        sequences.  A pair's numbers do not depend on the other pairs or on sharing (share_prefix=False: never share; same numbers).  prompt + continuation beyond
        max_seq (or the prefill workspace) raises ValueError: truncation is never applied, it would score another text."""
        from . import scoring as SC
        if samples["spatial_pixel_values"].shape[0] != 1:
            raise ValueError("score takes the pixel tensors of one video")
        if (continuations is None) == (continuation_ids is None):
            raise ValueError("score: pass exactly one of continuations and continuation_ids")
        top_n = SC.resolve_top(top_logprobs)
        tk = self.tokenizer
        eos, bos = getattr(tk, "eos_token_id", None), getattr(tk, "bos_token_id", None)
        if continuations is not None:
            tok = (lambda s: tk(s).input_ids) if hasattr(tk("x"), "input_ids") else tk
            conts = [SC.continuation_ids(tok, c, bos, append_eos, eos) for c in continuations]
        else:
            conts = [SC.with_eos(c, append_eos, eos) for c in continuation_ids]
        if len(conts) != len(prompts) or not conts:
            raise ValueError("score: one continuation per prompt, at least one pair")
        if any(t < 0 or t >= self.geo.vocab for c in conts for t in c):
            raise ValueError("score: a continuation id outside the vocabulary")
        rows = [self.tokenizer_image_token(t) for t in prompts]          # never truncated
        n_vis = self._n_visual(samples)
        n_prompt = [len(r) - 1 + n_vis for r in rows]
        for p_, c in zip(n_prompt, conts):                               # the over-length error comes before any device work
            SC.assemble(p_, c, 0, self.geo.max_seq)
        full = [list(r) + c for r, c in zip(rows, conts)]
        lens = [p_ + len(c) for p_, c in zip(n_prompt, conts)]
        prefix = self._shared_prefix(full, n_vis, lens, min(n_prompt) - 1) if share_prefix else 0
        if max(lens) - prefix > self.geo.max_prefill:
            raise ValueError(f"score: {max(lens) - prefix} rows of one pair exceed the prefill workspace (max_prefill = {self.geo.max_prefill})")
        self.last_shared_prefix = prefix
        eng = self.engine
        eng.set_sampling(False)                                          # the members' first tokens (never read here) are picked by the defaults: all off
        eng.set_logits_processors(*LP.OFF.args())
        eng.set_token_rules(None)
        eng.set_grammar(None)
        eng.set_logprobs(-1)
        vis = self.encode_images(samples)[0]
        parts, base = [], None
        try:
            if prefix:
                base = eng.seq_alloc(prefix)
                eng.prefill(base, eng.splice(full[0], vis)[:prefix])
            for g in range(0, len(full), 8):                             # a group: its remaining rows in ONE decoder pass, scored on the way
                seqs = []
                try:
                    embs, nxt = [], []
                    for i in range(g, min(g + 8, len(full))):
                        sl, ids = SC.assemble(n_prompt[i], conts[i], prefix, self.geo.max_seq)
                        embs.append(eng.splice(full[i], vis)[sl])
                        nxt.append(ids)
                        seqs.append(eng.seq_fork(base, prefix, lens[i]) if prefix else eng.seq_alloc(lens[i]))
                    parts.append(eng.score_extend_batch(seqs, embs, nxt, top_n))
                finally:
                    for s_ in seqs:
                        eng.seq_free(s_)
        finally:
            if base is not None:
                eng.seq_free(base)
        cat = lambda j: torch.cat([p_[j] for p_ in parts]).cpu().tolist()    # (the copy synchronises)
        return SC.fold(conts, cat(0), cat(1), cat(2) if top_n else None, cat(3) if top_n else None, top_n)

    # training forward --------------------------------------------------------------------------
    @torch.inference_mode()
    def forward(self, samples) -> Dict[str, torch.Tensor]:
        """LLAVA_NEXT_VIDEO.forward(samples) -> {"loss"} (models/llava_next_video.py:598-614), forward only: prepare_batch
        (labels / right padding / truncation), encode_images, label + mask splice, then the causal-LM loss of the language model.
        The padded batch is never materialised: the masked rows of every sample sit at its END (right padding; the dummy visual
        rows of a 'text' sample), so dropping them leaves positions and causal attention of the kept rows unchanged, and
        CrossEntropyLoss(mean) over the flattened batch == sum of token losses / number of labelled tokens over the samples."""
        tk = self.tokenizer
        tok = (lambda s: tk(s).input_ids) if hasattr(tk("x"), "input_ids") else tk
        ids, labels, mask = P.prepare_batch(self.llm, samples["text_inputs"], tok, getattr(tk, "bos_token_id", None),
                                            tk.pad_token_id, tk.eos_token_id, self.max_txt_len)
        feats = self.encode_images(samples)
        total, count = 0.0, 0
        for b, vid in enumerate(samples["video_ids"]):
            is_text = vid == "text"
            ml, mm = P.splice_labels(ids[b], labels[b], mask[b], feats.shape[1], is_text)
            n = int(mm.sum())
            assert bool((mm[:n] == 1).all()), "attention mask is not a prefix of ones"
            if bool((ml[n:] != P.IGNORE_INDEX).any()) and not getattr(self, "_warned_pad_label", False):
                # reference quirk: after truncation `batch_labels[:, -1] = eos` also labels the PAD slot of shorter rows, whose
                # logits come from a masked pad row; that term is dropped here (it trains nothing but the pad embedding)
                print("WARNING: label on a masked (padding) position ignored")
                self._warned_pad_label = True
            emb = self.engine.splice(_row(ids, mask, b), feats[b][:0] if is_text else feats[b])
            assert emb.shape[0] == n
            s, c = self.engine.forward_loss(emb, ml[:n].tolist())
            total, count = total + s, count + c
        loss = total / count if count else float("nan")         # CrossEntropyLoss over zero targets is nan in torch too
        return {"loss": torch.tensor(loss, dtype=torch.float32, device=self.engine.device)}

    __call__ = forward

    def generate_ids(self, ids_arr, mask, feats, max_new: int, processors=None, logprobs: Optional[int] = None):
        """Greedy / sampled ids of every row.  processors: one logits.Processors for all rows, a list with one per row, or None (the engine's
        default, set_logits_processors).  logprobs: None = the ids only; -1 .. 8 = every row's gvl_seq_set_logprobs setting, and the return value
        is (ids, lps) with lps[i] = (lp, top) of row i as Engine.seq_read_logprobs reads them back before the sequence is freed."""
        eng = self.engine
        opts = [LP.SeqOptions(p, logprobs) for p in (processors if isinstance(processors, (list, tuple)) else [processors] * ids_arr.shape[0])]
        if ids_arr.shape[0] == 1:
            got = eng.generate_ids(eng.splice(_row(ids_arr, mask, 0), feats[0]), max_new, getattr(self.tokenizer, "eos_token_id", None),
                                   processors=opts[0].processors, logprobs=logprobs)
            return [got] if logprobs is None else ([got[0]], [got[1]])
        # bs > 1 (the reference left-pads the batch, llava_next_video.py:622-647): every sample keeps its own paged KV and its
        # un-padded length -- identical maths to the masked left-padded batch.  Prefill runs over the packed rows of a group
        # (gvl_prefill_varlen) and the greedy decode of the whole group runs together (gvl_decode_greedy_batch: one weight stream
        # per token for groups of up to 16 sequences)

        def plan(i):
            emb = eng.splice(_row(ids_arr, mask, i), feats[i])

            def begin(seqs):
                LP.apply_seq_options(eng, seqs[0], opts[i])
                return emb
            return (min(emb.shape[0] + max_new, self.geo.max_seq),), begin
        return self._decode_in_pool_groups(ids_arr.shape[0], plan, max_new, logprobs, launch=eng.prefill_batch)


BASE_VOCAB = {"phi3.5": 32064, "llama3": 128256, "vicuna": 32000}     # tokenizer sizes before reset_embeddings [ext]


def geometry_from_checkpoint_dirs(llm: str, config_path: Optional[str], pretrained_vision_proj_llm_path: Optional[str],
                                  stage: str = "sft", num_temporal_tokens: int = 300) -> TowerGeometry:
    """Default geometry of an LLM family, completed from the HF config.json next to the weights: the reference builds its language
    model from `<pretrained_vision_proj_llm_path>/language_model_seperated` (models/llava_next_video.py:149-151), whose config.json
    carries rope_scaling.{short,long}_factor, both context limits, rope_theta, rms_norm_eps and the base vocab_size.
    Vocabulary: stages 'grounded' / 'sft' run reset_embeddings (:153-154, :231-268): num_temporal_tokens + 2 new rows and an lm_head
    WITH bias; stage 'pretrain' keeps the base vocabulary and the bias-free lm_head."""
    import json
    geo = {"phi3.5": TowerGeometry, "llama3": TowerGeometry.llama3_8b, "vicuna": TowerGeometry.vicuna_7b}[llm]()
    geo.kv_pages = 0                   # production default: the paged KV pool takes the HBM left once the weights are resident
    base_vocab = BASE_VOCAB[llm]
    cands = []
    if pretrained_vision_proj_llm_path:
        cands.append(os.path.join(pretrained_vision_proj_llm_path, "language_model_seperated", "config.json"))
    if config_path:
        cands.append(os.path.join(config_path, "config.json"))
    for c in cands:
        if os.path.exists(c):
            with open(c) as f:
                cfg = json.load(f)
            geo.apply_hf_config(cfg)
            base_vocab = int(cfg.get("text_config", cfg).get("vocab_size", base_vocab))
            break
    grown = stage in ("grounded", "sft")
    geo.vocab = base_vocab + (num_temporal_tokens + 2 if grown else 0)
    geo.lm_head_bias = grown
    return geo


def load_reference_checkpoints(llm: str, pretrained_video_path: str, pretrained_vision_proj_llm_path: str):
    """The reference's on-disk layout (models/llava_next_video.py:117-151): vision_model.pth, image_newline(s).pth,
    multi_modal_projector.pth, language_model_seperated/ (HF safetensors), InternVideo2 .pt."""
    d = pretrained_vision_proj_llm_path
    need = [os.path.join(d, "vision_model.pth"), pretrained_video_path]
    missing = [p for p in need if not os.path.exists(p)]
    if missing:
        raise FileNotFoundError(f"reference checkpoints not found: {missing}; pass state_dicts=... (e.g. synthetic weights from grounded_video_llm_amd.synth)")
    sd = {"vision_tower": torch.load(os.path.join(d, "vision_model.pth"), map_location="cpu"),
          "video_encoder": torch.load(pretrained_video_path, map_location="cpu")}
    proj = {f"multi_modal_projector.{k}": v for k, v in torch.load(os.path.join(d, "multi_modal_projector.pth"), map_location="cpu").items()}
    if llm == "phi3.5":
        nl = torch.load(os.path.join(d, "image_newlines.pth"), map_location="cpu")
        proj["glb_GN"], proj["sub_GN"] = nl["glb_GN"], nl["sub_GN"]
    else:
        proj["image_newline"] = torch.load(os.path.join(d, "image_newline.pth"), map_location="cpu")["image_newline"]
    sd["projectors"] = proj
    from safetensors.torch import load_file
    lm = {}
    lmdir = os.path.join(d, "language_model_seperated")
    for f in sorted(os.listdir(lmdir)):
        if f.endswith(".safetensors"):
            lm.update(load_file(os.path.join(lmdir, f)))
    sd["language_model"] = lm
    if "video_projecter.up_proj.weight" not in proj:   # trained group: arrives with the fine-tuned ckpt (inference.py:159-160)
        emb = next(v for k, v in lm.items() if k.endswith("embed_tokens.weight"))
        hid, vd = emb.shape[1], sd["video_encoder"]["cls_token"].shape[-1]
        proj.update({"video_projecter.up_proj.weight": torch.zeros(hid, vd), "video_projecter.up_proj.bias": torch.zeros(hid),
                     "video_projecter.down_proj.weight": torch.zeros(hid, hid), "video_projecter.down_proj.bias": torch.zeros(hid)})
    return sd
