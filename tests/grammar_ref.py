"""CPU torch restatement of the device's whole token-selection pipeline on ONE fp32 row (csrc/gvl_logits.hip) with the grammar stage in HF's place:
sequence_bias -> repetition penalty -> no-repeat n-gram -> bad_words_ids -> min length -> GRAMMAR -> forced eos -> suppress -> begin suppress.
Everything around the grammar is tests/token_rules_ref.py's restate_rules, run in two halves.  The grammar stage is HF's
PrefixConstrainedLogitsProcessor: `scores + mask`, mask 0.0 on the allowed ids and -inf elsewhere (so an allowed -0.0 becomes +0.0); where the
device's walk is OFF or in an END state (Grammar.allowed -> None) the row is left as it is, bit for bit."""
import dataclasses
import math

import torch

from token_rules_ref import restate_rules


def grammar_stage(s: torch.Tensor, hist, grammar) -> torch.Tensor:
    """The grammar stage alone, on a copy of the fp32 row `s`."""
    s = s.clone()
    m = grammar.allowed(list(hist))
    if m is None:
        return s
    mask = torch.full_like(s, -math.inf)
    mask[torch.from_numpy(m.copy())] = 0.0
    return s + mask


def restate(scores: torch.Tensor, hist, grammar=None, rules=None, penalty=1.0, ngram=0, min_new=0, eos=-1) -> torch.Tensor:
    """grammar: a grounded_video_llm_amd.grammar.Grammar or None; rules: a logits.TokenRules or None.  Returns the processed copy of the row."""
    hist = list(hist)
    head = None if rules is None else dataclasses.replace(rules, force_ids=(), suppress=(), begin_suppress=())          # up to the min-length ban
    s = restate_rules(scores, hist, head, penalty, ngram, min_new, eos)
    if grammar is not None:
        s = grammar_stage(s, hist, grammar)
    if rules is not None:                                                                                                # forced eos and the suppress lists
        s = restate_rules(s, hist, dataclasses.replace(rules, sequence_bias=type(rules.sequence_bias)(), bad_words=type(rules.bad_words)()))
    return s


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """equal as bit patterns: -0.0 and +0.0 differ"""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
