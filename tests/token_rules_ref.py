"""CPU torch restatement of the device's whole token-selection pipeline on ONE fp32 row (csrc/gvl_logits.hip), in HF's order:
sequence_bias -> repetition penalty -> no-repeat n-gram -> bad_words_ids -> min length -> forced eos -> suppress -> begin suppress.
The penalty / n-gram / min-length part has the semantics of `restate` in tests/test_gpu_logits_processors.py; every operation is one IEEE fp32
add, multiply, divide or store, so the device must reproduce it exactly (`torch.equal`: float equality, -0.0 == 0.0 -- HF adds a zero bias
to every token, which only turns -0.0 into +0.0)."""
import math

import torch


def _bias_stage(s: torch.Tensor, hist, table: dict) -> None:
    """s[t] += fp32 sum from 0.0 of t's length-1 bias, then of the multi-token entries (dict order) that end in t, are not longer than the
    history and whose first len - 1 ids equal the last len - 1 history ids (SequenceBiasLogitsProcessor.__call__)."""
    L = len(hist)
    zero = torch.zeros((), dtype=torch.float32)
    sums = {}
    for ids, b in table.items():
        if len(ids) == 1:
            sums[ids[0]] = zero + torch.tensor(b, dtype=torch.float32)
    for ids, b in table.items():
        if len(ids) == 1 or len(ids) > L:
            continue
        if list(hist[L - (len(ids) - 1):]) == list(ids[:-1]):
            sums[ids[-1]] = sums.get(ids[-1], zero) + torch.tensor(b, dtype=torch.float32)
    for t, v in sums.items():
        if 0 <= t < s.shape[0]:
            s[t] = s[t] + v


def restate_rules(scores: torch.Tensor, hist, rules=None, penalty=1.0, ngram=0, min_new=0, eos=-1) -> torch.Tensor:
    """rules: a grounded_video_llm_amd.logits.TokenRules or None.  Returns the processed copy of the row."""
    s = scores.detach().float().cpu().clone()
    hist = list(hist)
    L, V = len(hist), s.shape[0]
    if rules is not None and rules.sequence_bias.targets:
        _bias_stage(s, hist, rules.sequence_bias.to_dict())
    if penalty != 1.0 and L:
        h = torch.tensor(hist, dtype=torch.long)
        g = s.gather(0, h)
        s.scatter_(0, h, torch.where(g < 0, g * penalty, g / penalty))
    if ngram > 0 and L >= ngram:
        suf = hist[L - ngram + 1:]
        for i in range(L - ngram + 1):
            if hist[i:i + ngram - 1] == suf:
                s[hist[i + ngram - 1]] = -math.inf
    if rules is not None and rules.bad_words.targets:
        _bias_stage(s, hist, rules.bad_words.to_dict())
    if eos >= 0 and L < min_new:
        s[eos] = -math.inf
    if rules is not None:
        if rules.force_ids and L == rules.force_at:
            s[:] = -math.inf
            for t in rules.force_ids:
                if 0 <= t < V:
                    s[t] = 0.0
        if rules.suppress:
            _ban(s, rules.suppress)
        if rules.begin_suppress and L == rules.begin_index:
            _ban(s, rules.begin_suppress)
    return s


def _ban(s: torch.Tensor, ids) -> None:
    t = torch.tensor(list(ids), dtype=torch.long)
    s[t[(t >= 0) & (t < s.shape[0])]] = -math.inf


def has_subsequence(ids, seq) -> bool:
    ids, seq = list(ids), list(seq)
    return any(ids[i:i + len(seq)] == seq for i in range(len(ids) - len(seq) + 1))
