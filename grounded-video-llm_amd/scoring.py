"""Teacher-forced scoring of GIVEN answers: how likely the model finds a continuation of a prompt -- option (A) against (B) / (C) / (D) of a multiple-choice
question (the reference's inference.py --prompt_videoqa), one candidate interval `From <12> to <45>` against another, a caption's perplexity.  generate() reports
log-probabilities only for the ids the model chose itself; this is the path for ids the caller chose.  The numbers come from the device (include/gvl.h
gvl_score_extend_varlen: one ragged decoder pass per group of up to 8 continuations behind a shared cached prefix); this module is the host side and does no device work:

  continuation_ids   a continuation's token ids: no BOS, optionally a closing EOS
  assemble           prompt rows + continuation ids + prefix length -> the rows a pair still has to run and the id each of them must predict
  fold               the packed device outputs -> one ScoreOutput per pair

Row / target convention (next token): with P prompt rows (embedding rows: text ids and the visual rows) and a continuation c[0 .. C), the sequence fed is the P + C rows
prompt ++ c.  Row P - 1 (the last prompt row) predicts c[0], row P + j predicts c[j + 1], and row P + C - 1 (the last continuation token) is fed but not scored -- what
follows it is not given.  Behind a cached prefix of `prefix` rows only rows prefix .. P + C - 1 run; the prefix never reaches the last prompt row (prefix <= P - 1)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

from .logprobs import MAX_TOP, top_pairs

NOT_SCORED = -100          # include/gvl.h gvl_score_extend_varlen: a row whose prediction is not scored


@dataclass
class ScoreOutput:
    """One (prompt, continuation) pair.  token_logprobs[j] = log p(token_ids[j] | prompt, token_ids[:j]) under the raw model distribution (no processors, rules or
    warpers); ranks[j] = how many ids the model finds more likely there (0: greedy decoding would have chosen token_ids[j]); top_logprobs[j] (top_logprobs=N only)
    = the N best (id, log-probability) pairs at that position."""
    token_ids: List[int]
    token_logprobs: List[float]
    ranks: List[int]
    top_logprobs: Optional[List[List[Tuple[int, float]]]]
    sum_logprob: float
    mean_logprob: float


def resolve_top(top_logprobs) -> int:
    """the top_logprobs argument -> the device's top_n (None = 0: no lists)"""
    if top_logprobs is None:
        return 0
    if isinstance(top_logprobs, bool) or not isinstance(top_logprobs, int) or not 0 <= top_logprobs <= MAX_TOP:
        raise ValueError(f"`top_logprobs` has to be an integer in 0 .. {MAX_TOP}, but is {top_logprobs!r}")
    return top_logprobs


def continuation_ids(tokenize: Callable[[str], Sequence[int]], text: str, bos_token_id: Optional[int], append_eos: bool = False, eos_token_id: Optional[int] = None) -> List[int]:
    """A continuation's ids: tokenised WITHOUT BOS (it continues a prompt), with the EOS appended on request (scores "and the answer ends here")."""
    ids = [int(t) for t in tokenize(text)]
    if ids and bos_token_id is not None and ids[0] == bos_token_id:
        ids = ids[1:]
    return with_eos(ids, append_eos, eos_token_id)


def with_eos(ids: Sequence[int], append_eos: bool, eos_token_id: Optional[int]) -> List[int]:
    ids = [int(t) for t in ids]
    if append_eos:
        if eos_token_id is None:
            raise ValueError("append_eos needs a tokenizer with an eos_token_id")
        ids.append(int(eos_token_id))
    if not ids:
        raise ValueError("a continuation needs at least one token")
    return ids


def assemble(n_prompt_rows: int, cont_ids: Sequence[int], prefix: int, max_seq: int) -> Tuple[slice, List[int]]:
    """-> (the slice of the pair's P + C rows that still has to run, the id each of those rows must predict or NOT_SCORED).  Raises ValueError when prompt +
    continuation exceed max_seq: nothing is ever truncated, that would score another text."""
    P, C = int(n_prompt_rows), len(cont_ids)
    if P < 1 or C < 1:
        raise ValueError("a pair needs at least one prompt row and one continuation token")
    if P + C > max_seq:
        raise ValueError(f"prompt ({P} rows) + continuation ({C} tokens) exceed max_seq = {max_seq}; scoring never truncates")
    if prefix < 0 or prefix > P - 1:
        raise ValueError(f"a cached prefix ({prefix} rows) must leave the last prompt row (row {P - 1}) to this pair: it predicts the first continuation token")
    nxt = [int(cont_ids[g - (P - 1)]) if P - 1 <= g < P + C - 1 else NOT_SCORED for g in range(prefix, P + C)]
    return slice(prefix, P + C), nxt


def fold(conts: Sequence[Sequence[int]], lp: Sequence[float], rank: Sequence[int], top_ids=None, top_lp=None, top_n: int = 0) -> List[ScoreOutput]:
    """The packed outputs of the device (pairs in call order, each pair's scored rows in row order = its continuation tokens in order; top lists [n][MAX_TOP]) ->
    one ScoreOutput per pair."""
    if len(lp) != sum(len(c) for c in conts) or len(rank) != len(lp):
        raise ValueError(f"{len(lp)} scored rows for {sum(len(c) for c in conts)} continuation tokens")
    out, at = [], 0
    for c in conts:
        n = len(c)
        lps = [float(v) for v in lp[at:at + n]]
        tops = [top_pairs(top_ids[at + j], top_lp[at + j], top_n) for j in range(n)] if top_n > 0 else None
        total = float(sum(lps))
        out.append(ScoreOutput([int(t) for t in c], lps, [int(r) for r in rank[at:at + n]], tops, total, total / n))
        at += n
    return out
