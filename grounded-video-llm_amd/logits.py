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
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

KWARGS = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "min_length")


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


def padded_embed_len(ids_width: int, n_visual: int) -> int:
    """Rows of the reference's inputs_embeds for a batch whose left-padded id rows are `ids_width` wide (one image slot -> n_visual rows)."""
    return int(ids_width) - 1 + int(n_visual)
