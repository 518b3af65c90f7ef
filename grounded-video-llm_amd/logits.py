"""HF generate()'s logits processors as the reference gets them: `repetition_penalty`, `no_repeat_ngram_size`, `min_new_tokens` / `min_length`
forwarded through **generate_kwargs (models/llava_next_video.py:655-661) into transformers' `_get_logits_processor` [ext].  This module only turns
those kwargs into the per-sequence parameters of the device kernel (gvl_set_logits_processors / gvl_seq_set_processors, csrc/gvl_logits.hip) and
raises HF's validation errors; the arithmetic runs on the device.

Semantics (transformers 4.40.1 as the reference pins; the installed 5.x agrees on every point used here):
  * the history every processor sees is the GENERATED ids only -- the reference passes inputs_embeds and no input_ids, so HF's input_ids start
    empty (5.x additionally warns about it).  Prompt tokens are never penalised.
  * order: repetition penalty -> no-repeat n-gram -> min_length -> min_new_tokens; then the warpers (temperature -> top-k -> top-p).
  * a processor exists only when its argument is "on": repetition_penalty not None and != 1.0; no_repeat_ngram_size not None and > 0 (so a
    negative value is silently off, as in HF); min_length / min_new_tokens > 0 AND an eos id exists.  Validation runs only for processors
    that exist, with HF's messages.
  * min_length with inputs_embeds is lowered by the embedding length: max(min_length - inputs_embeds.shape[1], 0); min_new_tokens, when given,
    takes precedence (min_length = min_new_tokens + 0).  For a batch the embedding length is the reference's PADDED batch length (its rows are
    stacked at one length, llava_next_video.py:568-594): left-padded id length - 1 + visual rows.

Token rules (`sequence_bias`, `bad_words_ids`, `forced_eos_token_id`, `suppress_tokens`, `begin_suppress_tokens`) are the other token-level
processors of `_get_logits_processor`; `resolve_rules` validates them as HF does and flattens them into the arrays of a device rule set
(gvl_rules_create).  The whole order is
  sequence_bias -> repetition penalty -> no-repeat n-gram -> bad_words_ids -> min_length / min_new_tokens -> forced_eos_token_id
    -> suppress_tokens -> begin_suppress_tokens -> warpers.
As the installed transformers computes them with inputs_embeds and no input_ids:
  * sequence_bias / bad_words_ids: per target token (an entry's last id) an fp32 sum from 0.0: the length-1 entry, then, in dict order, the
    multi-token entries whose first len - 1 ids equal the last len - 1 generated ids; the sum is added to the score once.  An entry is skipped
    while it is LONGER THAN THE HISTORY (`len(sequence_ids) > input_ids.shape[1]`): a 2-token entry first applies at the third new token.
    bad_words_ids is the same mechanism with bias -inf, entries equal to [eos] dropped.
  * forced_eos_token_id: when max_new_tokens - 1 ids were generated every score becomes -inf and the forced ids' scores 0.
  * suppress_tokens: -inf at every step; begin_suppress_tokens: -inf only while nothing was generated yet (begin_index 0).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np

RULE_KWARGS = ("sequence_bias", "bad_words_ids", "forced_eos_token_id", "suppress_tokens", "begin_suppress_tokens")
KWARGS = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "min_length") + RULE_KWARGS


@dataclass(frozen=True)
class Processors:
    """Per-sequence parameters of the device kernel; the defaults switch every processor off."""
    penalty: float = 1.0
    ngram: int = 0
    min_new: int = 0            # eos is banned while fewer ids than this were generated
    eos: int = -1               # -1: no eos id -> the min-length ban is off

    @property
    def active(self) -> bool:
        return self.penalty != 1.0 or self.ngram > 0 or (self.min_new > 0 and self.eos >= 0)

    def args(self):
        """(penalty, ngram, min_new, eos_id) in the order of the C ABI."""
        return float(self.penalty), int(self.ngram), int(self.min_new), int(self.eos)


OFF = Processors()


def resolve(kw: dict, eos_id: Optional[int], embed_len: int = 0) -> Processors:
    """HF kwargs -> Processors for one reference generate() call whose inputs_embeds have `embed_len` rows.  Raises HF's ValueErrors."""
    penalty, ngram, min_new = 1.0, 0, 0
    p = kw.get("repetition_penalty")
    if p is not None and p != 1.0:
        if not isinstance(p, float) or not (p > 0):                          # RepetitionPenaltyLogitsProcessor.__init__
            raise ValueError(f"`penalty` has to be a strictly positive float, but is {p}")
        penalty = float(p)
    n = kw.get("no_repeat_ngram_size")
    if n is not None and n > 0:
        if not isinstance(n, int) or n <= 0:                                 # NoRepeatNGramLogitsProcessor.__init__
            raise ValueError(f"`ngram_size` has to be a strictly positive integer, but is {n}")
        ngram = int(n)
    if eos_id is not None and eos_id >= 0:
        # GenerationMixin._prepare_generated_length: min_new_tokens wins; otherwise min_length loses the embedding rows
        mnt, ml = kw.get("min_new_tokens"), kw.get("min_length")
        if mnt is not None:
            m = mnt + 0
        elif ml is not None:
            m = max(ml - int(embed_len), 0) if embed_len > 0 else ml
        else:
            m = 0
        if m > 0:
            if not isinstance(m, int) or m < 0:                              # MinLengthLogitsProcessor.__init__ (min_new_tokens reaches it first)
                raise ValueError(f"`min_length` has to be a non-negative integer, but is {m}")
            min_new = int(m)
        return Processors(penalty, ngram, min_new, int(eos_id))
    return Processors(penalty, ngram, 0, -1)


WARPER_KWARGS = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")


def resolve_sampling(kw: dict) -> dict:
    """HF's warpers past top-p among generate()'s kwargs -> {min_p, typical_p, epsilon_cutoff, eta_cutoff}, None where a warper is off (absent, None, 0; typical_p
    1.0), as Engine.set_sampling / seq_set_sampling take them.  Raises the ValueErrors of HF's MinP / Typical / Epsilon / Eta warpers for values outside their ranges."""
    out = dict.fromkeys(WARPER_KWARGS)
    v = kw.get("min_p")
    if v is not None:
        if not (0 <= v <= 1.0):                                              # MinPLogitsWarper.__init__
            raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {v}")
        out["min_p"] = float(v) or None
    v = kw.get("typical_p")
    if v is not None and float(v) != 1.0:
        v = float(v)
        if not (v > 0 and v < 1):                                            # TypicalLogitsWarper.__init__
            raise ValueError(f"`typical_p` has to be a float > 0 and < 1, but is {v}")
        out["typical_p"] = v
    for name in ("epsilon_cutoff", "eta_cutoff"):
        v = kw.get(name)
        if v is not None and float(v) != 0.0:
            v = float(v)
            if v <= 0 or v >= 1:                                             # EpsilonLogitsWarper / EtaLogitsWarper.__init__
                raise ValueError(f"`{name}` has to be a float > 0 and < 1, but is {v}")
            out[name] = v
    return out


GUIDANCE_KWARGS = ("guidance_scale", "negative_prompt_ids", "negative_prompt_attention_mask", "negative_prompts")


def resolve_guidance(kw: dict) -> Optional[float]:
    """HF's `guidance_scale` among generate()'s kwargs -> the scale of classifier-free guidance, or None when it is off.  HF's rule (`_get_logits_processor`): the
    processor exists only when guidance_scale is not None and != 1.  HF itself checks nothing else and would compute with whatever it is given; here the value must
    be a finite real number (an int is taken as its float), since it travels to the device as one fp32 constant."""
    s = kw.get("guidance_scale")
    if s is None:
        return None
    if isinstance(s, bool) or not isinstance(s, (int, float, np.integer, np.floating)) or not np.isfinite(float(s)):
        raise ValueError(f"`guidance_scale` has to be a finite float, but is {s!r}")
    return None if s == 1 else float(s)


MAX_CONTRASTIVE_TOP_K = 16   # = GVL_MAX_DECODE_BATCH (csrc/gvl_limits.h): a step's candidates advance in ONE decode batch


def resolve_contrastive(kw: dict) -> Optional[tuple]:
    """HF's contrastive search among generate()'s kwargs -> (top_k, penalty_alpha), or None when the call is another mode.  HF's rule (GenerationMixin
    ._get_generation_mode, transformers 4.40.1 [ext]): num_beams == 1, do_sample false, top_k not None and > 1, penalty_alpha not None and > 0.  penalty_alpha must be a
    real number in [0, 1] whatever the mode (HF validates nothing and would compute with any value; here it travels to the device as one fp32 constant), and in the mode
    top_k is an integer of at most MAX_CONTRASTIVE_TOP_K: the candidates of a step share one decode batch."""
    a = kw.get("penalty_alpha")
    if a is None:
        return None
    if isinstance(a, bool) or not isinstance(a, (int, float, np.integer, np.floating)) or not 0.0 <= float(a) <= 1.0:
        raise ValueError(f"`penalty_alpha` has to be a float in [0, 1], but is {a!r}")
    k = kw.get("top_k")
    if not float(a) > 0 or k is None or kw.get("do_sample", False) or (kw.get("num_beams", 1) or 1) != 1:
        return None
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"`top_k` has to be an integer, but is {k!r}")
    if int(k) <= 1:
        return None
    if int(k) > MAX_CONTRASTIVE_TOP_K:
        raise ValueError(f"contrastive search (penalty_alpha > 0): `top_k` is at most {MAX_CONTRASTIVE_TOP_K} (the candidates of a step share one decode batch), but is {k}")
    return int(k), float(a)


def negative_id_rows(ids, mask=None) -> list:
    """HF's negative_prompt_ids (+ negative_prompt_attention_mask) -> one plain list of token ids per row: a tensor / array / list of rows (or one flat row), the ids
    whose mask is 0 (padding) dropped.  Raises ValueError for an empty row, a negative id or a mask of another shape."""
    rows = ids.tolist() if hasattr(ids, "tolist") else list(ids)
    if rows and not isinstance(rows[0], (list, tuple)):
        rows = [rows]
    mrows = None
    if mask is not None:
        mrows = mask.tolist() if hasattr(mask, "tolist") else list(mask)
        if mrows and not isinstance(mrows[0], (list, tuple)):
            mrows = [mrows]
        if len(mrows) != len(rows) or any(len(m) != len(r) for m, r in zip(mrows, rows)):
            raise ValueError("`negative_prompt_attention_mask` must have the shape of `negative_prompt_ids`")
    out = []
    for i, r in enumerate(rows):
        keep = [int(t) for j, t in enumerate(r) if mrows is None or mrows[i][j]]
        if not keep or any(t < 0 for t in keep):
            raise ValueError("`negative_prompt_ids`: every row needs at least one (unmasked) token id, all >= 0")
        out.append(keep)
    return out


def request_sampling(do_sample=None, temperature=None, top_k=None, top_p=None, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None, seed=None):
    """One request's OWN sampling setting for SeqOptions.sampling: ... when every argument is None (the request follows the engine's setting), else a dict for
    Engine.seq_set_sampling with stream 0 -- greedy for do_sample=False; otherwise sampled (do_sample None counts as True once another argument is given) with HF's
    defaults for what is absent (temperature 1.0, top_k 50, seed 0).  Raises HF's ValueErrors."""
    given = dict(temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff, seed=seed)
    if do_sample is None and all(v is None for v in given.values()):
        return ...
    warp = resolve_sampling(given)
    if do_sample is not None and not do_sample:
        return dict(do_sample=False)
    t = 1.0 if temperature is None else temperature
    if isinstance(t, bool) or not isinstance(t, (int, float)) or not t > 0:      # TemperatureLogitsWarper.__init__
        raise ValueError(f"`temperature` (={t}) has to be a strictly positive float, otherwise your next token scores will be invalid.")
    k = 50 if top_k is None else top_k
    if isinstance(k, bool) or not isinstance(k, int) or k < 0:                   # 0 = off, as GenerationConfig takes it; TopKLogitsWarper rejects the rest
        raise ValueError(f"`top_k` has to be a strictly positive integer, but is {k}")
    if top_p is not None and not (0 <= float(top_p) <= 1.0):                     # TopPLogitsWarper.__init__
        raise ValueError(f"`top_p` has to be a float > 0 and < 1, but is {top_p}")
    return dict(do_sample=True, temperature=float(t), top_k=int(k), top_p=None if top_p is None else float(top_p), seed=0 if seed is None else int(seed), stream=0, **warp)


@dataclass(frozen=True)
class SeqOptions:
    """One sequence's settings; per field leave what it was allocated with | off | set: processors None | OFF | a Processors; logprobs None | -1 | 0 .. 8; rules ... | None | a rules_create id;
    sampling ... | None (follow the engine's setting) | a dict as Engine.seq_set_sampling takes it (the sequence's own setting); grammar ... | None | a grammar_create id"""
    processors: Optional[Processors] = None
    logprobs: Optional[int] = None
    rules: object = ...
    sampling: object = ...
    grammar: object = ...


SeqOptions.OFF = SeqOptions(OFF, -1, None, grammar=None)


def apply_seq_options(eng, seq: int, opts: SeqOptions) -> None:
    """Set what `opts` does not leave alone on the live sequence `seq` (right after its seq_alloc / seq_fork, before its prefill)."""
    if opts.processors is not None:
        eng.seq_set_processors(seq, *opts.processors.args())
    if opts.logprobs is not None:
        eng.seq_set_logprobs(seq, opts.logprobs)
    if opts.rules is not ...:
        eng.seq_set_token_rules(seq, opts.rules)
    if opts.sampling is not ...:
        eng.seq_set_sampling(seq, opts.sampling)
    if opts.grammar is not ...:
        eng.seq_set_grammar(seq, opts.grammar)


def read_seq_logprobs(eng, seq: int, ids, opts: SeqOptions):
    """(lp, top) of the generated `ids` of `seq` (Engine.seq_read_logprobs; before the sequence is freed); None when opts.logprobs left the engine's default."""
    return None if opts.logprobs is None else eng.seq_read_logprobs(seq, 0, len(ids), top=opts.logprobs > 0)


def padded_embed_len(ids_width: int, n_visual: int) -> int:
    """Rows of the reference's inputs_embeds for a batch whose left-padded id rows are `ids_width` wide (one image slot -> n_visual rows)."""
    return int(ids_width) - 1 + int(n_visual)


# ---- token rules -----------------------------------------------------------------------------------------------------------------
MAX_IDS = 1 << 18        # ids of one single-token list / single-token entries of one bias table (GVL_RULES_MAX_IDS)
MAX_SEQS = 1024          # multi-token entries of one bias table (GVL_RULES_MAX_SEQS)
MAX_SEQ_LEN = 16         # ids of one multi-token entry (GVL_RULES_MAX_SEQ_LEN)


@dataclass(frozen=True)
class BiasTable:
    """{ids: bias} grouped by target token (an entry's last id) for the device: one thread owns one target and sums its entries in order.
    targets: (target, first_entry, n_entries); entry e: bias entry_bias[e] (fp32 value) and the prefix ids prefix[off : off + len] with
    (off, len) = entry_prefix[e].  Within a group the length-1 entry comes first, then the multi-token entries in dict order."""
    targets: tuple = ()
    entry_bias: tuple = ()
    entry_prefix: tuple = ()
    prefix: tuple = ()

    def to_dict(self) -> dict:
        out = {}
        for t, e0, ne in self.targets:
            for e in range(e0, e0 + ne):
                off, ln = self.entry_prefix[e]
                out[tuple(self.prefix[off:off + ln]) + (t,)] = self.entry_bias[e]
        return out


def group_by_target(bias: dict, what: str = "sequence_bias") -> BiasTable:
    """dict {tuple of ids: float} -> BiasTable.  Raises ValueError beyond the capacities of the device rule set (nothing is truncated)."""
    groups: dict = {}
    n_multi = 0
    for ids, b in bias.items():
        ids = tuple(int(t) for t in ids)
        if len(ids) > MAX_SEQ_LEN:
            raise ValueError(f"`{what}`: an entry of {len(ids)} ids exceeds the limit of {MAX_SEQ_LEN} ids per entry")
        n_multi += len(ids) > 1
        g = groups.setdefault(ids[-1], [[], []])
        g[0 if len(ids) == 1 else 1].append((ids[:-1], float(np.float32(b))))
    if n_multi > MAX_SEQS:
        raise ValueError(f"`{what}`: {n_multi} multi-token entries exceed the limit of {MAX_SEQS}")
    if len(bias) - n_multi > MAX_IDS:
        raise ValueError(f"`{what}`: {len(bias) - n_multi} single-token entries exceed the limit of {MAX_IDS}")
    targets, eb, ep, pre = [], [], [], []
    for t, (single, multi) in groups.items():
        targets.append((t, len(eb), len(single) + len(multi)))
        for ids, b in single + multi:
            eb.append(b)
            ep.append((len(pre), len(ids)))
            pre.extend(ids)
    return BiasTable(tuple(targets), tuple(eb), tuple(ep), tuple(pre))


@dataclass(frozen=True)
class TokenRules:
    """One generate() call's token rules as the device takes them (gvl_rules_create); the defaults switch every rule off."""
    suppress: tuple = ()
    begin_suppress: tuple = ()
    begin_index: int = 0
    force_ids: tuple = ()          # forced_eos_token_id(s); applied when exactly force_at ids were generated
    force_at: int = 0
    sequence_bias: BiasTable = field(default_factory=BiasTable)
    bad_words: BiasTable = field(default_factory=BiasTable)

    @property
    def active(self) -> bool:
        return bool(self.suppress or self.begin_suppress or self.force_ids or self.sequence_bias.targets or self.bad_words.targets)


NO_RULES = TokenRules()


def _validate_sequence_bias(sequence_bias):
    """SequenceBiasLogitsProcessor._validate_arguments + _convert_list_arguments_into_dict, with HF's messages."""
    if not isinstance(sequence_bias, dict) and not isinstance(sequence_bias, list) or len(sequence_bias) == 0:
        raise ValueError(f"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is {sequence_bias}.")
    if isinstance(sequence_bias, dict) and any(not isinstance(ids, tuple) for ids in sequence_bias):
        raise ValueError(f"`sequence_bias` has to be a dict with tuples as keys, but is {sequence_bias}.")
    if isinstance(sequence_bias, dict) and any(
            any((not isinstance(t, (int, np.integer)) or t < 0) for t in ids) or len(ids) == 0 for ids in sequence_bias):
        raise ValueError(f"Each key in `sequence_bias` has to be a non-empty tuple of positive integers, but is {sequence_bias}.")

    def pair_ok(seq):
        return isinstance(seq[0], list) and all(isinstance(t, (int, np.integer)) and t > 0 for t in seq[0]) and isinstance(seq[1], float)
    if isinstance(sequence_bias, list) and any((not pair_ok(seq)) or len(seq) == 0 for seq in sequence_bias):
        raise ValueError(f"Each element in `sequence_bias` has to be a non-empty list of lists of positive integers and float, but is {sequence_bias}.")
    if isinstance(sequence_bias, dict) and any(not isinstance(b, float) for b in sequence_bias.values()):
        raise ValueError(f"`sequence_bias` has to be a dict with floats as values, but is {sequence_bias}.")
    if isinstance(sequence_bias, list):
        return {tuple(seq[0]): seq[1] for seq in sequence_bias}
    return dict(sequence_bias)


def _validate_bad_words(bad_words_ids, eos_id):
    """NoBadWordsLogitsProcessor.__init__: HF's messages, [eos] entries dropped, every sequence -> bias -inf."""
    if not isinstance(bad_words_ids, list) or len(bad_words_ids) == 0:
        raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bad_words_ids}.")
    if any(not isinstance(w, list) for w in bad_words_ids):
        raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bad_words_ids}.")
    if any(any((not isinstance(t, (int, np.integer)) or t < 0) for t in w) for w in bad_words_ids):
        raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bad_words_ids}.")
    if any(len(w) == 0 for w in bad_words_ids):                                # HF: an IndexError at the first call
        raise ValueError(f"Each list in `bad_words_ids` has to be non-empty, but is {bad_words_ids}.")
    if eos_id is not None and eos_id >= 0:
        bad_words_ids = [w for w in bad_words_ids if w != [eos_id]]
    return {tuple(w): float("-inf") for w in bad_words_ids}                    # may be empty (only [eos] given): HF then bans nothing


def _id_list(ids, what: str, vocab: Optional[int]) -> tuple:
    """suppress lists: HF builds torch.tensor(list(ids)) and masks with isin, so ids outside the vocabulary never match; they are dropped here."""
    out = []
    for t in list(ids):
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)):
            raise ValueError(f"`{what}` has to be a list of integers, but is {ids}.")
        if t >= 0 and (vocab is None or t < vocab):
            out.append(int(t))
    out = tuple(dict.fromkeys(out))
    if len(out) > MAX_IDS:
        raise ValueError(f"`{what}`: {len(out)} ids exceed the limit of {MAX_IDS}")
    return out


def resolve_rules(kw: dict, eos_id: Optional[int], max_new: int, vocab: Optional[int] = None) -> TokenRules:
    """HF kwargs -> TokenRules for one reference generate(inputs_embeds=..., max_new_tokens=max_new) call.  Raises HF's ValueErrors with HF's
    messages, and ValueError for a rule set beyond the device capacities.  vocab (when known) enables HF's vocabulary check of the biased ids."""
    sb, bw = BiasTable(), BiasTable()
    if kw.get("sequence_bias") is not None:
        d = _validate_sequence_bias(kw["sequence_bias"])
        if vocab is not None:                                                 # SequenceBiasLogitsProcessor._prepare_bias_variables
            bad = [t for ids in d for t in ids if t >= vocab]
            if bad:
                raise ValueError(f"The model vocabulary size is {vocab}, but the following tokens were being biased: {bad}")
        sb = group_by_target(d, "sequence_bias")
    if kw.get("bad_words_ids") is not None:
        d = _validate_bad_words(kw["bad_words_ids"], eos_id)
        if vocab is not None:
            bad = [t for ids in d for t in ids if t >= vocab]
            if bad:
                raise ValueError(f"The model vocabulary size is {vocab}, but the following tokens were being biased: {bad}")
        bw = group_by_target(d, "bad_words_ids")
    force, force_at = (), 0
    fe = kw.get("forced_eos_token_id")
    if fe is not None:
        ids = [fe] if isinstance(fe, (int, np.integer)) and not isinstance(fe, bool) else list(fe)
        if any(isinstance(t, bool) or not isinstance(t, (int, np.integer)) or t < 0 for t in ids):    # ForcedEOSTokenLogitsProcessor.__init__
            import torch
            raise ValueError(f"`eos_token_id` has to be a list of positive integers, but is {torch.tensor(ids)}")
        if vocab is not None and any(t >= vocab for t in ids):
            raise ValueError(f"`forced_eos_token_id` {ids} outside the vocabulary of {vocab} tokens")   # HF: an IndexError at the forced step
        force = tuple(dict.fromkeys(int(t) for t in ids))
        if len(force) > MAX_IDS:
            raise ValueError(f"`forced_eos_token_id`: {len(force)} ids exceed the limit of {MAX_IDS}")
        force_at = int(max_new) - 1
        if force_at < 0:
            force = ()
    sup = _id_list(kw["suppress_tokens"], "suppress_tokens", vocab) if kw.get("suppress_tokens") is not None else ()
    beg = _id_list(kw["begin_suppress_tokens"], "begin_suppress_tokens", vocab) if kw.get("begin_suppress_tokens") is not None else ()
    return TokenRules(sup, beg, 0, force, force_at, sb, bw)
