"""Per-token log-probabilities of generate(): the confidence a caller can get for an answer (the spread over the temporal tokens <0> .. <299>
of a grounding answer, the probabilities of the option letters of a multiple-choice one).  HF users get it through
generate(..., output_scores=True, return_dict_in_generate=True) and compute_transition_scores [ext]; the reference cannot return it (its
generate() batch-decodes whatever language_model.generate hands back).  This module resolves those kwargs and shapes the result; the
numbers come from the device (the token-selection kernels, include/gvl.h gvl_seq_set_logprobs) or, for beam search, from beam.py.

  return_dict_in_generate=True    generate() returns a GenerateOutput instead of a list of texts
  output_scores=True              GenerateOutput.transition_scores: per row, one log-probability per new id -- HF's
                                  compute_transition_scores(out.sequences, out.scores, normalize_logits=True) for greedy / sampling (the
                                  processed row, or the warped distribution the token was drawn from), and compute_transition_scores(...,
                                  beam_indices) with sequences_scores for beam search
  top_logprobs=N (extra, 0 .. 8)  GenerateOutput.top_logprobs: per row, per new id, the N best (id, log-probability) of the same distribution
                                  (fewer when fewer are finite / kept); not with num_beams > 1
HF's full per-step vocabulary rows (`scores` / `logits`) are not returned: output_logits=True with return_dict_in_generate raises.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

MAX_TOP = 8            # = GVL_MAX_TOP_LOGPROBS (csrc/gvl_internal.h): slots per generation step of a sequence's top lists


@dataclass
class GenerateOutput:
    """generate(..., return_dict_in_generate=True).  sequences: the new ids of every row (what generate() decodes into texts)."""
    texts: List[str]
    sequences: List[List[int]]
    transition_scores: Optional[List[List[float]]] = None
    top_logprobs: Optional[List[List[List[Tuple[int, float]]]]] = None
    sequences_scores: Optional[List[float]] = None
    # contrastive search (penalty_alpha, top_k) with output_scores: per token the degeneration penalty max_j cos(h, h_j) it was selected with; transition_scores are
    # then the tokens' PROBABILITIES p (the model confidence of the score (1 - alpha) p - alpha pen), not log-probabilities
    degeneration_penalties: Optional[List[List[float]]] = None


@dataclass(frozen=True)
class Options:
    return_dict: bool = False
    output_scores: bool = False
    top: Optional[int] = None             # the top_logprobs kwarg

    @property
    def top_n(self) -> int:
        """The device setting of the call's sequences (gvl_seq_set_logprobs): -1 off, 0 the selected token's, N also the top N."""
        if not self.return_dict:
            return -1
        if self.top is not None:
            return self.top
        return 0 if self.output_scores else -1


def resolve(kw: dict) -> Options:
    """generate() kwargs -> Options.  Raises ValueError for a top_logprobs outside 0 .. 8, top_logprobs with beam search, and output_logits with
    return_dict_in_generate (the full rows are not returned)."""
    rd, osc = bool(kw.get("return_dict_in_generate", False)), bool(kw.get("output_scores", False))
    top = kw.get("top_logprobs")
    if top is not None:
        if isinstance(top, bool) or not isinstance(top, int) or not 0 <= top <= MAX_TOP:
            raise ValueError(f"`top_logprobs` has to be an integer in 0 .. {MAX_TOP}, but is {top!r}")
        if (kw.get("num_beams", 1) or 1) > 1:
            raise ValueError("`top_logprobs` is not supported with num_beams > 1")
    if rd and kw.get("output_logits", False):
        raise ValueError("output_logits=True is not supported: the full per-step logits rows are not returned (use output_scores / top_logprobs)")
    return Options(rd, osc, top)


def top_pairs(ids: Sequence[int], vals: Sequence[float], n: int) -> List[Tuple[int, float]]:
    """One generation step's top list (MAX_TOP slots) -> its first n (id, log-probability) pairs, without the (-1, -inf) padding."""
    return [(int(i), float(v)) for i, v in zip(list(ids)[:n], list(vals)[:n]) if int(i) >= 0]


def build_output(texts: List[str], sequences: List[List[int]], opts: Options, lps=None, beam_scores: Optional[List[float]] = None) -> GenerateOutput:
    """lps: per row (lp, top) as the engine reads them back (top: per token a list of pairs, or None); None when logprobs were off."""
    out = GenerateOutput(texts, sequences)
    if lps is not None:
        if opts.output_scores:
            out.transition_scores = [list(lp[:len(s)]) for (lp, _), s in zip(lps, sequences)]
        if opts.top is not None:
            out.top_logprobs = [[list(t) for t in (top or [[] for _ in s])[:len(s)]] for (_, top), s in zip(lps, sequences)]
    if beam_scores is not None:
        out.sequences_scores = list(beam_scores)
    return out
