"""Beam search as the reference gets it from HF `generate(num_beams=k, do_sample=False)` (inference.py:46,170-176 ->
models/llava_next_video.py:655-661 -> transformers 4.40.1 GenerationMixin._beam_search + BeamSearchScorer / BeamHypotheses [ext],
the version requirements.txt pins): host-side bookkeeping only -- the log-softmax / top-2k of every step and the KV cache
live with the caller (`step`).  Restated, not imported: the installed transformers (5.x) no longer ships BeamSearchScorer; the
CPU test drives this function and the installed `generate()` with the same tiny HF model and compares the sequences.

Semantics kept from 4.40.1 (batch of one, one beam group):
  * beam_scores start as [0, -1e9, ...]; per step the log-softmax of every running beam plus its score is flattened, the best
    2k (token, beam) pairs are visited in order: an eos candidate of rank < k closes a hypothesis (score = sum of log-probs /
    generated_len ** length_penalty, generated_len counting the eos), of rank >= k is skipped; the first k non-eos candidates are the
    next running beams;
  * the search is done when k hypotheses exist and (early_stopping, or the worst of them is at least the best running
    sum-log-prob / cur_len ** length_penalty); at max_new_tokens the running beams are added as hypotheses;
  * the answer is the best hypothesis (num_return > 1: the num_return best, best first), with eos appended when it ended by eos.

Beam-SAMPLE (`generate(num_beams=k, do_sample=True)`; reachable from inference.py:45-49,170-176; 4.40.1 GenerationMixin._beam_sample): the same
bookkeeping, but the 2k candidates of a step are DRAWN: every running beam's log-softmax goes through the warpers (temperature -> top-k ->
top-p, min_tokens_to_keep = 2 as HF sets it for num_beams > 1), the beam scores are added, and 2k (token, beam) pairs are sampled without
replacement from softmax over the k x V grid, then visited in order of their score.  torch.multinomial's random stream cannot be reproduced
across implementations (the same caveat as plain sampling, include/gvl.h): parity = same candidate distribution; draws come from a seeded
torch.Generator, so a run is reproducible under `seed`.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import torch


class _Hyps:
    """BeamHypotheses of transformers 4.40.1 (generation/beam_search.py) for one batch item."""

    def __init__(self, num_beams: int, length_penalty: float, early_stopping):
        self.k, self.lp, self.early = num_beams, length_penalty, early_stopping
        self.beams: List[Tuple[float, List[int], bool, List[float]]] = []   # (score, ids, ended by eos, per-token scores)
        self.worst = 1e9

    def add(self, toks: Sequence[int], sum_logprobs: float, generated_len: int, by_eos: bool, token_scores: Sequence[float] = ()):
        score = sum_logprobs / (generated_len ** self.lp)
        if len(self.beams) < self.k or score > self.worst:
            self.beams.append((score, list(toks), by_eos, list(token_scores)))
            if len(self.beams) > self.k:
                order = sorted((s, i) for i, (s, _, _, _) in enumerate(self.beams))
                del self.beams[order[0][1]]
                self.worst = order[1][0]
            else:
                self.worst = min(score, self.worst)

    def is_done(self, best_sum_logprobs: float, cur_len: int) -> bool:
        if len(self.beams) < self.k:
            return False
        if self.early is True:
            return True
        if self.early is False:
            return self.worst >= best_sum_logprobs / (cur_len ** self.lp)
        # "never": a heuristic-free upper bound on what a running beam can still reach
        if self.lp > 0.0:
            raise ValueError("early_stopping='never' with length_penalty > 0 needs max_length; not used by the reference")
        return self.worst >= best_sum_logprobs / (cur_len ** self.lp)


def warp_scores(scores: torch.Tensor, temperature: float = 1.0, top_k: Optional[int] = 50, top_p: Optional[float] = None, min_keep: int = 2,
                min_p: Optional[float] = None, typical_p: Optional[float] = None, epsilon_cutoff: Optional[float] = None,
                eta_cutoff: Optional[float] = None) -> torch.Tensor:
    """transformers 4.40.1 logits warpers in generate()'s order on `scores` [rows, V] (here: log-probabilities): TemperatureLogitsWarper (scores / T),
    TopKLogitsWarper (everything below the k-th largest -> -inf; k = max(top_k, min_keep)), TopPLogitsWarper (ascending sort, drop the tokens whose
    cumulative probability stays <= 1 - top_p, never the last min_keep); then HF's MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper and
    EtaLogitsWarper in that order (None / 0 = off; typical_p 1.0 = off), each on the rows the stage before left, each keeping at least min_keep."""
    s = scores.float()
    if temperature is not None and temperature != 1.0:
        s = s / float(temperature)
    if top_k is not None and top_k > 0:
        kk = min(max(int(top_k), min_keep), s.shape[-1])
        s = s.masked_fill(s < torch.topk(s, kk).values[..., -1, None], float("-inf"))
    if top_p is not None and top_p < 1.0:
        srt, idx = torch.sort(s, descending=False)
        remove = srt.softmax(dim=-1).cumsum(dim=-1) <= (1.0 - float(top_p))
        remove[..., -min_keep:] = False
        s = s.masked_fill(remove.scatter(-1, idx, remove), float("-inf"))
    V = s.shape[-1]
    if min_p:                                                # p < min_p * p_max goes, never the min_keep most probable
        probs = torch.softmax(s, dim=-1)
        remove = probs < float(min_p) * probs.amax(dim=-1, keepdim=True)
        remove.scatter_(-1, torch.topk(probs, min(min_keep, V), dim=-1).indices, False)
        s = s.masked_fill(remove, float("-inf"))
    if typical_p and typical_p < 1.0:                        # ascending |-log p - H|: keep up to and including the first whose cumulative mass reaches typical_p
        norm = torch.log_softmax(s, dim=-1)
        ent = -(norm * norm.exp()).nansum(-1, keepdim=True)
        srt, idx = torch.sort(torch.abs(-norm - ent), descending=False)
        cum = s.gather(-1, idx).softmax(dim=-1).cumsum(dim=-1)
        last = (cum < float(typical_p)).sum(dim=-1).clamp_(max=V - 1)
        remove = srt > srt.gather(-1, last[..., None])
        remove[..., :min_keep] = False
        s = s.masked_fill(remove.scatter(-1, idx, remove), float("-inf"))
    for cut, eta in ((epsilon_cutoff, False), (eta_cutoff, True)):
        if not cut:
            continue
        c = torch.tensor(float(cut), device=s.device)
        if eta:                                              # min(eta, sqrt(eta) * exp(-H))
            c = torch.min(c, torch.sqrt(c) * torch.exp(-torch.distributions.Categorical(logits=s).entropy()))[..., None]
        remove = (s.softmax(dim=-1) < c) & (s < torch.topk(s, min(min_keep, V)).values[..., -1, None])
        s = s.masked_fill(remove, float("-inf"))
    return s


def reorder(beams: Sequence[Optional[int]], parents: Sequence[Optional[int]]) -> Tuple[List[Optional[int]], List[int], List[int]]:
    """HF's cache reorder as a plan over beam slots (csrc/gvl_beam.h's reorder, the one definition every stepper follows): new beam j continues old slot parents[j]
    (None: slot j dies); beams[q] None: slot q is closed already.  Returns (src, clones, closed): src[j] the slot beam j continues or None; clones the j that need a
    clone of beams[src[j]] -- every child of a parent but its first, made before anything is closed --; closed the live slots nobody continues.  Both ascending."""
    src: List[Optional[int]] = [None] * len(parents)
    kept, clones = set(), []
    for j, p in enumerate(parents):
        if p is None or p < 0:
            continue
        if p >= len(beams) or beams[p] is None:
            raise ValueError("a beam continues a closed beam")
        src[j] = p
        if p in kept:
            clones.append(j)
        kept.add(p)
    return src, clones, [q for q, b in enumerate(beams) if b is not None and q not in kept]


def beam_search(step: Callable[[List[int], List[int]], torch.Tensor], first_logits: torch.Tensor, num_beams: int, max_new_tokens: int,
                eos_id: Optional[int], length_penalty: float = 1.0, early_stopping=False, sample: Optional[dict] = None,
                process: Optional[Callable[[List[List[int]], torch.Tensor], torch.Tensor]] = None, with_scores: bool = False,
                candidates: Optional[Callable[[torch.Tensor, torch.Tensor], Tuple[Sequence[float], Sequence[int], Sequence[float]]]] = None,
                num_return: int = 1, num_beam_groups: int = 1, diversity_penalty: float = 0.0, pad_id: Optional[int] = None):
    """first_logits [vocab]: logits after the prompt.  step(parents, tokens) -> logits [k, vocab] of the k new running beams, where new beam j
    continues old beam parents[j] with tokens[j] (the caller reorders its KV cache accordingly; at the first call every parent is 0 = the
    prompt).  Returns the NEW ids of the best hypothesis (eos included when it ended by eos), as HF does for inputs_embeds prompts.
    sample: None = beam search; dict(temperature, top_k, top_p, generator[, min_p, typical_p, epsilon_cutoff, eta_cutoff]) = beam-sample (module docstring).
    process(histories, logprobs) -> logprobs: HF's logits processors (repetition penalty, no-repeat n-gram, min length; grounded_video_llm_amd/logits.py)
    on the [k, vocab] log-softmax rows of the running beams, histories[j] = the ids beam j generated so far; applied before the warpers and before
    the beam scores are added, as HF's _beam_search / _beam_sample do.
    with_scores: return (ids, sequences_score, transition_scores) instead -- HF's definitions: sequences_score = the hypothesis score (sum of the
    processed log-probabilities / generated_len ** length_penalty), transition_scores = compute_transition_scores(seq, scores, beam_indices,
    normalize_logits=False), i.e. per new id the processed (beam-sample: warped) log-probability it had in the row of the beam it extended, before
    the beam score was added -- tracked per running beam through the parent chain.
    candidates (beam search only): a callable (processed rows [k, vocab], beam scores [k]) -> (vals, idxs, proc_vals), the step's 2k candidates best first -- value
    (processed log-probability + beam score), flat index beam * vocab + token, the processed log-probability alone.  It replaces the torch top-2k below and the
    gather of the transition scores: Engine.op_beam_candidates (the library's own kernels) plugs in here, and tests record every step's list through it.
    num_return (1 .. num_beams; HF num_return_sequences with beams, BeamSearchScorer.finalize's num_beam_hyps_to_keep): > 1 returns a LIST of results, the num_return
    best hypotheses, best first -- among equal scores the later added first; beam search and beam-sample alike.  1 returns the one result, as ever.
    num_beam_groups / diversity_penalty / pad_id: anything but (1, 0.0) is diverse (group) beam search -- group_beam_search below, whose hooks take the group; (1, 0.0) is
    this function as it always was."""
    if check_groups(num_beams, num_beam_groups, diversity_penalty, sample is not None):
        return group_beam_search(step, first_logits, num_beams, num_beam_groups, diversity_penalty, max_new_tokens, eos_id, length_penalty, early_stopping,
                                 process=process, with_scores=with_scores, candidates=candidates, num_return=num_return, pad_id=pad_id)
    k = int(num_beams)
    if k < 2:
        raise ValueError("beam_search needs num_beams >= 2")
    n_ret = int(num_return)
    if n_ret < 1 or n_ret > k:
        raise ValueError("num_return must be 1 .. num_beams")
    V = first_logits.shape[-1]
    if V < 2 * k:
        raise ValueError("vocabulary smaller than 2 x num_beams")
    seqs: List[List[int]] = [[] for _ in range(k)]
    tsc: List[List[float]] = [[] for _ in range(k)]             # per running beam: the transition score of each of its ids
    # transformers 4.40.1: _beam_search starts beams 1..k-1 at -1e9 (the first step expands beam 0 only); _beam_sample starts EVERY beam at 0 -- its
    # first draw is over k identical rows, so the same token may be drawn from two rows and the running beams may start as duplicates
    scores = torch.zeros((k,), dtype=torch.float32, device=first_logits.device)
    if sample is None:
        scores[1:] = -1e9
    logits = first_logits.float().unsqueeze(0).expand(k, V)
    hyps = _Hyps(k, length_penalty, early_stopping)
    done = False
    while True:
        lp = torch.log_softmax(logits.float(), dim=-1)
        if process is not None:
            lp = process([list(q) for q in seqs], lp)
        proc = lp                                        # (beam-sample: warped below) the rows HF reports as `scores`
        hooked = None
        if sample is None and candidates is not None:
            vals, idxs, hooked = (list(x) for x in candidates(lp, scores))
        elif sample is None:
            lp = lp + scores[:, None]
            top = torch.topk(lp.reshape(-1), 2 * k, largest=True, sorted=True)
            vals, idxs = top.values.tolist(), top.indices.tolist()
        else:
            proc = warp_scores(lp, sample.get("temperature", 1.0), sample.get("top_k", 50), sample.get("top_p"), min_p=sample.get("min_p"),
                               typical_p=sample.get("typical_p"), epsilon_cutoff=sample.get("epsilon_cutoff"), eta_cutoff=sample.get("eta_cutoff"))
            lp = proc + scores[:, None]
            flat = lp.reshape(-1)
            n_fin = int(torch.isfinite(flat).sum())
            if n_fin < 2 * k:                                # torch.multinomial(replacement=False) would silently hand back zero-probability indices
                raise ValueError(f"beam-sample: only {n_fin} tokens survive the warpers but 2 x num_beams = {2 * k} draws are needed "
                                 "(raise top_p / top_k / temperature, or lower num_beams)")
            picks = torch.multinomial(torch.softmax(flat, dim=-1), 2 * k, replacement=False, generator=sample.get("generator"))
            pv, order = torch.sort(flat[picks], descending=True)
            vals, idxs = pv.tolist(), picks[order].tolist()
        cur_len = len(seqs[0]) + 1
        if hooked is not None:
            pv_tok = hooked
        else:
            pv_tok = proc.reshape(-1)[torch.as_tensor(idxs, device=proc.device)].tolist() if with_scores else [0.0] * len(idxs)
        nxt: List[Tuple[float, int, int, float]] = []
        for rank, (v, ix, t_sc) in enumerate(zip(vals, idxs, pv_tok)):
            b, tok = ix // V, ix % V
            if eos_id is not None and tok == eos_id:
                if rank >= k:
                    continue
                hyps.add(seqs[b], v, cur_len, True, tsc[b] + [t_sc])
            else:
                nxt.append((v, tok, b, t_sc))
            if len(nxt) == k:
                break
        if len(nxt) < k:
            raise ValueError("fewer than num_beams non-eos candidates among the top 2 x num_beams")
        done = done or hyps.is_done(max(vals), cur_len)
        # first step: every row is the prompt itself (beam-sample may have drawn from rows >= 1 of its k identical rows) -> parent 0
        parents, toks = [0 if cur_len == 1 else b for _, _, b, _ in nxt], [t for _, t, _, _ in nxt]
        seqs = [seqs[b] + [t] for _, t, b, _ in nxt]
        tsc = [tsc[b] + [t_sc] for _, _, b, t_sc in nxt]
        scores = torch.tensor([v for v, _, _, _ in nxt], dtype=torch.float32, device=first_logits.device)
        if done or len(seqs[0]) >= max_new_tokens:
            break
        logits = step(parents, toks)
    if not done:
        for j in range(k):                                   # finalize(): the open beams become hypotheses
            hyps.add(seqs[j], float(scores[j]), len(seqs[j]), False, tsc[j])
    # HF's finalize: sorted(beams, key=score) is stable and hypotheses are popped from its end -- best first, among equal scores the LATER added first
    ranked = sorted(hyps.beams, key=lambda x: x[0])[::-1] if hyps.beams else [(0.0, seqs[0], False, tsc[0])]
    results = []
    for best in ranked[:n_ret]:
        out = list(best[1])
        if best[2] and eos_id is not None and len(out) < max_new_tokens:
            out.append(eos_id)
        results.append((out, float(best[0]), list(best[3])[:len(out)]) if with_scores else out)
    return results[0] if n_ret == 1 else results


# ---- diverse (group) beam search: transformers 4.40.1 GenerationMixin._group_beam_search + BeamSearchScorer(num_beam_groups = G) + HammingDiversityLogitsProcessor [ext] ----
def check_groups(num_beams, num_beam_groups, diversity_penalty, do_sample: bool = False) -> bool:
    """HF's validation of num_beam_groups / diversity_penalty (GenerationConfig.validate, BeamSearchScorer and HammingDiversityLogitsProcessor's constructors) as
    ValueError.  Returns whether the arguments ask for group beam search; (1, 0.0) -- and None for either -- is plain beam search."""
    G = 1 if num_beam_groups is None else num_beam_groups
    lam = 0.0 if diversity_penalty is None else diversity_penalty
    if isinstance(G, bool) or not isinstance(G, int) or G < 1:
        raise ValueError(f"`num_beam_groups` has to be a strictly positive integer, but is {G!r}")
    if isinstance(lam, bool) or not isinstance(lam, (int, float)) or lam != lam:
        raise ValueError(f"`diversity_penalty` should be a float strictly larger than 0., but is {lam!r}")
    if G == 1 and lam == 0:
        return False
    prefix = "`diversity_penalty` is not 0.0 or `num_beam_groups` is not 1, triggering group beam search. In this generation mode, "
    if do_sample:
        raise ValueError(prefix + "`do_sample` must be set to `False`")
    k = 1 if num_beams is None else int(num_beams)
    if G > k or k % G != 0:
        raise ValueError(f"`num_beam_groups` ({G}) has to be an integer smaller or equal than `num_beams` ({k}) and `num_beams` has to be divisible by `num_beam_groups`")
    if G > 1 and lam == 0:
        raise ValueError(prefix + "`diversity_penalty` should be greater than `0.0`, otherwise your groups will be identical.")
    if not isinstance(lam, float) or not lam > 0.0:
        raise ValueError(f"`diversity_penalty` should be a float strictly larger than 0., but is {lam!r}")
    if G == 1:
        raise ValueError(prefix + "`num_beam_groups` should be greater than 1: a diversity penalty needs a second group to act on")
    return True


def hamming_penalty(rows: torch.Tensor, prev_tokens: Sequence[int], diversity_penalty: float) -> torch.Tensor:
    """HammingDiversityLogitsProcessor on one group's rows [s, V]: every row loses fp32(fp32(lambda) * fp32(c[t])) at token t, c = how often t occurs among the
    tokens the earlier groups chose at this step (`scores -= lambda * bincount`); ids outside [0, V) count nowhere."""
    V = rows.shape[-1]
    ids = [int(t) for t in prev_tokens if 0 <= int(t) < V]
    if not ids:
        return rows
    c = torch.bincount(torch.as_tensor(ids, dtype=torch.long), minlength=V).to(device=rows.device, dtype=torch.float32)
    return rows.float() - torch.tensor(float(diversity_penalty), dtype=torch.float32, device=rows.device) * c


def group_beam_search(step: Callable[[List[Optional[int]], List[int]], torch.Tensor], first_logits: torch.Tensor, num_beams: int, num_beam_groups: int,
                      diversity_penalty: float, max_new_tokens: int, eos_id: Optional[int], length_penalty: float = 1.0, early_stopping=False,
                      process: Optional[Callable] = None, with_scores: bool = False, candidates: Optional[Callable] = None, num_return: int = 1,
                      pad_id: Optional[int] = None):
    """generate(num_beams = k, num_beam_groups = G, diversity_penalty = lambda): G groups of s = k / G beams, group g owning the running beams g*s .. g*s + s - 1.  Every
    step advances all k beams once; then the groups are visited in order, each one beam_search's own step with k := s (its own _Hyps(s), its own done flag, its 2s
    candidates from its s x vocab grid).  Two things couple them: group g > 0's processed rows lose lambda x (how often the earlier groups chose the token at this step)
    -- HammingDiversityLogitsProcessor, in HF's list after sequence_bias and before the repetition penalty -- and the tokens a group chose (its first s non-eos candidates)
    are what the later groups count.  The beam scores start at -1e9 except the first beam of every group.  A group that was done when the step began is not processed: its
    beams get score 0 and pad_id as their token (which the later groups DO count; None: an id that counts nowhere), and they never become hypotheses.  At the end every
    open group adds its beams, the hypotheses of all groups are pooled in group order and ranked as beam_search ranks them.
    step(parents, tokens): as beam_search's, over all k beams -- parents are global (g*s + the local parent; 0 at the first call); the beams of a done group come with
    parent None (nothing of theirs is read again: the caller may free them) and their rows of the returned [k, vocab] logits are ignored.
    process(histories, logprobs, group=g, prev_tokens=[...], diversity_penalty=lambda) -> the processed rows [s, vocab] of group g: the whole chain INCLUDING the Hamming
    term in its place (Engine.op_logits_process(..., hamming=...)); None: the Hamming term alone, in torch.
    candidates(rows [s, vocab], scores [s], group=g) -> (vals, idxs, proc_vals), the group's 2s candidates, flat index = local beam * vocab + token.
    with_scores / num_return: as beam_search (the transition score of an id includes its Hamming term, as HF's `scores` do)."""
    if not check_groups(num_beams, num_beam_groups, diversity_penalty, False):
        raise ValueError("group_beam_search needs num_beam_groups > 1 and diversity_penalty > 0")
    k, G, lam = int(num_beams), int(num_beam_groups), float(diversity_penalty)
    s = k // G
    n_ret = int(num_return)
    if n_ret < 1 or n_ret > k:
        raise ValueError("num_return must be 1 .. num_beams")
    V = first_logits.shape[-1]
    if V < 2 * s:
        raise ValueError("vocabulary smaller than 2 x the beams of a group")
    pad = -1 if pad_id is None or int(pad_id) < 0 else int(pad_id)
    dev = first_logits.device
    seqs: List[List[int]] = [[] for _ in range(k)]
    tsc: List[List[float]] = [[] for _ in range(k)]
    scores = torch.full((k,), -1e9, dtype=torch.float32, device=dev)
    scores[::s] = 0.0
    hyps = [_Hyps(s, length_penalty, early_stopping) for _ in range(G)]
    done = [False] * G
    logits = first_logits.float().unsqueeze(0).expand(k, V)
    n_gen = 0
    while True:
        lp_all = torch.log_softmax(logits.float(), dim=-1)
        cur_len = n_gen + 1
        current: List[int] = [pad] * k                        # the tokens chosen at THIS step, filled group by group
        parents: List[Optional[int]] = [None] * k
        new_seqs, new_tsc, new_scores = list(seqs), list(tsc), [0.0] * k
        for g in range(G):
            lo = g * s
            if done[g]:                                       # BeamSearchScorer.process: a done group is padded -- score 0, token pad
                for j in range(s):
                    new_seqs[lo + j], new_tsc[lo + j] = seqs[lo] + [pad], tsc[lo] + [0.0]
                continue
            rows, sc, prev = lp_all[lo:lo + s], scores[lo:lo + s], current[:lo]
            if process is not None:
                rows = process([list(q) for q in seqs[lo:lo + s]], rows, group=g, prev_tokens=list(prev), diversity_penalty=lam)
            elif g > 0:
                rows = hamming_penalty(rows, prev, lam)
            if candidates is not None:
                vals, idxs, pv_tok = (list(x) for x in candidates(rows, sc, group=g))
            else:
                top = torch.topk((rows + sc[:, None]).reshape(-1), 2 * s, largest=True, sorted=True)
                vals, idxs = top.values.tolist(), top.indices.tolist()
                pv_tok = rows.reshape(-1)[top.indices].tolist() if with_scores else [0.0] * len(idxs)
            nxt: List[Tuple[float, int, int, float]] = []
            for rank, (v, ix, t_sc) in enumerate(zip(vals, idxs, pv_tok)):
                b, tok = lo + ix // V, ix % V
                if eos_id is not None and tok == eos_id:
                    if rank >= s:
                        continue
                    hyps[g].add(seqs[b], v, cur_len, True, tsc[b] + [t_sc])
                else:
                    nxt.append((v, tok, b, t_sc))
                if len(nxt) == s:
                    break
            if len(nxt) < s:
                raise ValueError("fewer than num_beams non-eos candidates among the top 2 x num_beams")
            done[g] = hyps[g].is_done(max(vals), cur_len)
            for j, (v, tok, b, t_sc) in enumerate(nxt):
                parents[lo + j], current[lo + j] = (0 if cur_len == 1 else b), tok
                new_seqs[lo + j], new_tsc[lo + j], new_scores[lo + j] = seqs[b] + [tok], tsc[b] + [t_sc], v
        seqs, tsc = new_seqs, new_tsc
        scores = torch.tensor(new_scores, dtype=torch.float32, device=dev)
        n_gen += 1
        if all(done) or n_gen >= max_new_tokens:
            break
        logits = step(parents, list(current))
    pool = []
    for g in range(G):
        if not done[g]:
            for j in range(g * s, g * s + s):
                hyps[g].add(seqs[j], float(scores[j]), len(seqs[j]), False, tsc[j])
        pool += hyps[g].beams
    ranked = sorted(pool, key=lambda x: x[0])[::-1]
    results = []
    for best in ranked[:n_ret]:
        out = list(best[1])
        if best[2] and eos_id is not None and len(out) < max_new_tokens:
            out.append(eos_id)
        results.append((out, float(best[0]), list(best[3])[:len(out)]) if with_scores else out)
    return results[0] if n_ret == 1 else results
