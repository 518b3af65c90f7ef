"""One generate() / generate_shared() call, resolved once: `resolve_call` turns the kwargs into a frozen `Call` -- the decoding mode and every value the mode needs --
and raises every ValueError that depends only on the kwargs, the tokenizer's ids and the vocabulary size, before the model touches its engine.  It is made of the
resolvers the features came with (logits.resolve*, logprobs.resolve, beam.check_groups and the ones below); nothing here imports torch."""
from __future__ import annotations

import dataclasses
import enum
from typing import Callable, Optional, Tuple

from . import grammar as GR
from . import logits as LP
from . import logprobs as LPR


Mode = enum.Enum("Mode", dict(GREEDY="greedy", SAMPLE="sample", BEAM="beam", BEAM_SAMPLE="beam-sample", GROUP_BEAM="group-beam", CONTRASTIVE="contrastive",
                              GUIDED="guided", FANOUT="fan-out"))       # guided: greedy or sampled, every sequence paired with its negative; fan-out: n samples per prompt


def _sampling_args(kw, draw_seed: Callable[[], int]):
    """(temperature, top_p, seed) of a do_sample call, validated as HF's warpers do; without `seed` one is drawn (draw_seed: from torch's CPU generator)."""
    t = kw.get("temperature", 1.0)
    t = 1.0 if t is None else float(t)
    if not t > 0:
        raise ValueError("`temperature` has to be a strictly positive float")      # HF's TemperatureLogitsWarper check
    top_p = kw.get("top_p")
    if top_p is not None and not (0 < float(top_p) <= 1.0):
        raise ValueError("`top_p` has to be a float > 0 and <= 1")
    seed = kw.get("seed")
    return t, top_p, int(seed) if seed is not None else int(draw_seed())


def _beam_impl(kw) -> str:
    """generate()'s beam_impl: "host" (default) or "device"; "device" is beam search only."""
    impl = kw.get("beam_impl", "host")
    if impl not in ("host", "device"):
        raise ValueError(f"beam_impl must be 'host' or 'device', not {impl!r}")
    if impl == "device" and kw.get("do_sample", False) and kw.get("num_beams", 1) not in (1, None):
        raise ValueError("beam_impl='device' is beam search (do_sample=False); beam-sample runs on the host path: its draws are torch's")
    return impl


def check_guidance(kw, n: int, vocab: int):
    """generate(guidance_scale=s, ...): HF's classifier-free guidance against a negative prompt (logits.resolve_guidance: off for None / 1).  Returns (scale, negative id
    rows, negative texts) -- (None, None, None) when off -- after checking that the call names one negative per sample -- negative_prompt_ids (HF's; plain ids, text-only)
    or negative_prompts (extra; strings through the model's own prompt path) -- and combines guidance with nothing it is not built for."""
    scale = LP.resolve_guidance(kw)
    if scale is None:
        return None, None, None
    if kw.get("num_beams", 1) not in (1, None):
        raise ValueError("generate(): guidance_scale with num_beams > 1 is not supported yet")
    ids, texts = kw.get("negative_prompt_ids"), kw.get("negative_prompts")
    if (ids is None) == (texts is None):
        raise ValueError("generate(): guidance_scale != 1 needs the negative prompt of every sample: pass negative_prompt_ids (token ids, text-only) or "
                         "negative_prompts (strings; with the <image> slot they see the same video) -- exactly one of them.  (HF's fallback, the prompt's last "
                         "id, does not exist for an embeddings prompt.)")
    if ids is not None:
        ids = LP.negative_id_rows(ids, kw.get("negative_prompt_attention_mask"))
        if any(t >= vocab for r in ids for t in r):
            raise ValueError(f"generate(): negative_prompt_ids holds an id outside the vocabulary of {vocab} tokens")
    elif isinstance(texts, str) or any(not isinstance(t, str) for t in texts):
        raise ValueError("generate(): negative_prompts must be a list of strings, one per sample")
    if len(ids if ids is not None else texts) != n:
        raise ValueError(f"generate(): {n} samples need {n} negative prompts, not {len(ids if ids is not None else texts)}")
    return scale, ids, None if texts is None else list(texts)


def num_return_sequences(kw) -> int:
    """generate()'s num_return_sequences (None = 1), with HF's validation (GenerationConfig.validate / GenerationMixin._validate_generated_length [ext]) as ValueError, and
    the one combination that is not built yet -- guidance_scale with several answers -- refused instead of ignored."""
    n = kw.get("num_return_sequences")
    n = 1 if n is None else int(n)
    if n < 1:
        raise ValueError(f"`num_return_sequences` has to be a strictly positive integer, but is {n}")
    if n == 1:
        return 1
    k = kw.get("num_beams", 1) or 1
    if k == 1 and not kw.get("do_sample", False):
        raise ValueError(f"Greedy methods without beam search do not support `num_return_sequences` different than 1 (got {n}).")
    if k > 1 and n > k:
        raise ValueError(f"`num_return_sequences` ({n}) has to be smaller or equal to `num_beams` ({k}).")
    if LP.resolve_guidance(kw) is not None:
        raise ValueError("generate(): guidance_scale with num_return_sequences > 1 is not supported yet")
    return n


def beam_groups(kw) -> Optional[Tuple[int, float]]:
    """generate()'s num_beam_groups / diversity_penalty: None for plain decoding (1 / 0.0 / absent), else (G, lambda) after HF's validation (beam.check_groups) as
    ValueError; the combinations that are not built -- groups with guidance_scale, groups with constrained beams -- are refused, never ignored."""
    from . import beam as B
    if not B.check_groups(kw.get("num_beams", 1) or 1, kw.get("num_beam_groups"), kw.get("diversity_penalty"), bool(kw.get("do_sample", False))):
        return None
    if LP.resolve_guidance(kw) is not None:
        raise ValueError("generate(): num_beam_groups > 1 with guidance_scale is not supported")
    if kw.get("constraints") or kw.get("force_words_ids"):
        raise ValueError("generate(): constrained beams (constraints / force_words_ids) with num_beam_groups > 1 are not supported")
    return int(kw["num_beam_groups"]), float(kw["diversity_penalty"])


def fanout_stream(prompt: int, member: int) -> int:
    """The random stream of answer `member` of prompt `prompt` in a generate(do_sample=True, num_return_sequences=n) call: member * 65536 + prompt.  It does not depend on
    n, so under a fixed seed the answers for n' < n are a prefix of the answers for n, per prompt."""
    if not 0 <= prompt < 65536 or not 0 <= member < 65536:
        raise ValueError("num_return_sequences: at most 65536 prompts per call and 65536 answers per prompt")
    return member * 65536 + prompt


@dataclasses.dataclass(frozen=True)
class Call:
    """What one call decodes with.  The defaults are the all-off call: greedy, nothing set."""
    mode: Mode = Mode.GREEDY
    max_new: int = 2048
    eos_id: Optional[int] = None
    pad_id: int = 0
    num_beams: int = 1                                    # > 1 in the three beam modes
    beam_impl: str = "host"
    length_penalty: float = 1.0
    early_stopping: object = False
    n_return: int = 1                                     # answers per prompt: the n best beams, or in fan-out mode n samples
    groups: Optional[Tuple[int, float]] = None            # group-beam: (G, lambda)
    contrastive: Optional[Tuple[int, float]] = None       # contrastive: (top_k, penalty_alpha)
    beam_sample: Optional[dict] = None                    # beam-sample: temperature, top_k, top_p, the four later warpers and the seed of the call's generator
    guidance: Optional[float] = None                      # guided: the scale, and the validated negatives, one per sample -- id rows or texts
    negative_ids: Optional[list] = None
    negative_texts: Optional[list] = None
    sampling_args: tuple = (False,)                       # Engine.set_sampling's positional arguments: (False,) or (True, temperature, top_k, top_p, seed)
    warpers: dict = dataclasses.field(default_factory=dict)      # ... and its keywords: the warpers past top-p that are on
    seq_sampling: Optional[dict] = None                   # fan-out: every sequence's own setting (Engine.seq_set_sampling's dict without the stream)
    rules: "LP.TokenRules" = LP.NO_RULES
    grammar: Optional["GR.Grammar"] = None
    logprobs: "LPR.Options" = LPR.Options()
    processor_kwargs: dict = dataclasses.field(default_factory=dict)

    @property
    def device_selects(self) -> bool:
        """Whether the device's own selection picks the tokens.  A search applies processors, rules and grammar to its own rows: the engine's defaults are off for it."""
        return self.mode not in (Mode.BEAM, Mode.BEAM_SAMPLE, Mode.GROUP_BEAM, Mode.CONTRASTIVE)

    @property
    def want_logprobs(self) -> Optional[int]:             # the logprobs argument of the id-level methods: None = ids only
        return self.logprobs.top_n if self.logprobs.top_n >= 0 else None

    def processors(self, embed_len: int) -> "LP.Processors":
        """The logits processors for inputs_embeds of `embed_len` rows, which lower min_length; only a min_length left positive that is no integer still raises here."""
        return LP.resolve(self.processor_kwargs, self.eos_id, embed_len)


def resolve_call(kw, *, entry: str, n_samples: int, eos_id: Optional[int], pad_id: int, vocab: int, draw_seed: Callable[[], int]) -> Call:
    """The kwargs of generate(samples, **kw) (entry "generate", n_samples samples) or generate_shared(samples, prompts, **kw) (entry "generate_shared") -> Call.
    generate_shared decodes greedily or sampled, with fan-out: it refuses guidance, groups and contrastive search, and takes num_beams > 1 as greedy, n-best refused.
    The checks run in a fixed order, because a call that is wrong in two ways reports the first: beam_impl, guidance, num_return_sequences, beam groups, contrastive
    search (generate_shared: its own refusals instead), log-probabilities, processors, warpers / temperature / top_p, token rules, grammar."""
    if entry not in ("generate", "generate_shared"):
        raise ValueError(f"resolve_call: entry must be 'generate' or 'generate_shared', not {entry!r}")
    shared = entry == "generate_shared"
    num_beams, do_sample = kw.get("num_beams", 1) or 1, bool(kw.get("do_sample", False))
    impl, scale, neg_ids, neg_texts, groups, cs = "host", None, None, None, None, None
    if shared:
        for what, msg in ((LP.resolve_guidance, "guidance_scale != 1 is not supported yet"), (beam_groups, "num_beam_groups > 1 (diverse beam search) is not supported"),
                          (LP.resolve_contrastive, "contrastive search (penalty_alpha > 0 with top_k > 1) is not supported")):
            if what(kw) is not None:
                raise ValueError(f"generate_shared(): {msg} (generate() takes it)")
        n_ret = num_return_sequences(kw)
        if n_ret > 1 and num_beams > 1:
            raise ValueError("generate_shared(): num_return_sequences > 1 is built for sampling (do_sample=True, num_beams=1); generate() returns the n best beams")
    else:
        impl = _beam_impl(kw)
        scale, neg_ids, neg_texts = check_guidance(kw, n_samples, vocab)
        n_ret = num_return_sequences(kw)
        groups = beam_groups(kw)
        cs = LP.resolve_contrastive(kw)                   # penalty_alpha is validated whatever the mode; what is not built is refused, never ignored
        if cs is not None and scale is not None:
            raise ValueError("generate(): contrastive search (penalty_alpha, top_k) with guidance_scale is not supported")
        if cs is not None and n_ret > 1:
            raise ValueError("generate(): contrastive search (penalty_alpha, top_k) is deterministic and returns one answer: num_return_sequences > 1 is not supported")
        if cs is not None and kw.get("top_logprobs") is not None:
            raise ValueError("generate(): `top_logprobs` is not supported with contrastive search (penalty_alpha, top_k); output_scores gives p and the degeneration penalty")
    opts = LPR.resolve(kw)
    proc_kw = {k: kw[k] for k in ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "min_length") if k in kw}
    LP.resolve({k: v for k, v in proc_kw.items() if k != "min_length"}, eos_id)       # min_length needs the embedding length: Call.processors
    warp = LP.resolve_sampling(kw)                        # HF validates the warpers' arguments whether or not the call samples
    sampling_args, warpers, seq_sampling, beam_sample = (False,), {}, None, None
    if do_sample and not (shared and num_beams > 1):
        # An unseeded call takes its seed from draw_seed, as often as it always did, so that torch.manual_seed reproduces it: once -- except in fan-out mode, where
        # the first draw goes to the engine's default (no sequence of the call follows it) and a second one to the sequences, which is the one the answers come from.
        t, top_p, seed = _sampling_args(kw, draw_seed)
        top_k = kw.get("top_k", 50)
        if num_beams > 1:
            beam_sample = dict(temperature=t, top_k=top_k, top_p=top_p, seed=seed, **warp)
        else:
            top_k = 0 if top_k is None else int(top_k)
            warpers = {k: v for k, v in warp.items() if v is not None}
            sampling_args = (True, t, top_k, top_p, seed)
            if n_ret > 1:
                seq_seed = seed if kw.get("seed") is not None else int(draw_seed())
                seq_sampling = dict(do_sample=True, temperature=t, top_k=top_k, top_p=top_p, seed=seq_seed, **warpers)
    max_new = int(kw.get("max_new_tokens", 2048))
    rules = LP.resolve_rules(kw, eos_id, max_new, vocab)
    if kw.get("prefix_allowed_tokens_fn") is not None:
        raise ValueError("generate(): prefix_allowed_tokens_fn is a Python callback and cannot run inside the device's decode loop; pass grammar= "
                         "(grounded_video_llm_amd.grammar: GrammarBuilder / grounding_grammar; Grammar.as_prefix_allowed_tokens_fn gives HF the same language)")
    grammar = kw.get("grammar")                           # a grammar.Grammar constrains every answer of the call: HF's prefix_allowed_tokens_fn as a device object
    if grammar is not None and not isinstance(grammar, GR.Grammar):
        raise ValueError(f"generate(): grammar must be a grounded_video_llm_amd.grammar.Grammar, not {type(grammar).__name__}")
    if grammar is not None and grammar.vocab != vocab:
        raise ValueError(f"generate(): the grammar classifies {grammar.vocab} ids, the model's vocabulary holds {vocab}")
    if cs is not None:
        mode = Mode.CONTRASTIVE
    elif num_beams > 1 and not shared:
        mode = Mode.GROUP_BEAM if groups else Mode.BEAM_SAMPLE if do_sample else Mode.BEAM
    else:
        mode = Mode.GUIDED if scale is not None else Mode.FANOUT if n_ret > 1 else Mode.SAMPLE if sampling_args[0] else Mode.GREEDY
    return Call(mode, max_new, eos_id, pad_id, num_beams, impl, float(kw.get("length_penalty", 1.0)) if num_beams > 1 else 1.0, kw.get("early_stopping", False), n_ret,
                groups, cs, beam_sample, scale, neg_ids, neg_texts, sampling_args, warpers, seq_sampling, rules, grammar, opts, proc_kw)
