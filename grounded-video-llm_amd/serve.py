"""Continuous batching of clips on the LLM.

The reference answers a batch of clips with ONE `language_model.generate(inputs_embeds=...)` over a left-padded batch
(models/llava_next_video.py:622-661): all members start together and the call returns when the LAST one has produced its
eos.  `ClipScheduler` keeps the same per-request result (greedy ids up to and including eos, at most max_new_tokens) but
lets requests join and leave between decode chunks:

  admit    queued requests take a free slot: splice -> KV pages (gvl_seq_alloc) -> ONE ragged prefill for all newcomers
           (gvl_prefill_varlen: packed rows through the decoder GEMMs)
  prefix   another question about a clip that is already resident: add_prefix() prefills the clip's rows once into a holder
           sequence; a request submitted with prefix=pid forks the holder (gvl_seq_fork: pages referenced, not copied) and
           prefills only the rows behind it -- newcomers with and without a prefix share ONE ragged pass
           (gvl_prefill_extend_varlen).  Same ids as without the prefix.
  decode   every active sequence advances `chunk` tokens (gvl_decode_steps: members at different generation steps share
           one weight stream per step in groups of up to 16)
  retire   ids are read back (gvl_seq_read), sequences that produced eos / reached max_new free their pages at once

All arithmetic is per sequence and batch-invariant, so the ids equal `Engine.generate_ids` of each request on its own
(tests/test_gpu_llm.py::test_scheduler_matches_one_at_a_time).  The scheduler itself is plain host logic and is tested
on CPU against a scripted engine (tests/test_host_logic.py).
"""
from __future__ import annotations

from collections import deque
from dataclasses import dataclass, field, replace
from typing import Deque, Dict, List, Optional, Sequence

from . import lib as L
from . import logits as LP


@dataclass
class _Request:
    rid: int
    embeds: object               # bf16 [S, hidden] device tensor (output of Engine.splice)
    max_new: int
    seq: int = -1
    ids: List[int] = field(default_factory=list)
    n_gen: int = 0               # tokens generated on the device so far (>= len(ids) once eos was seen)
    opts: LP.SeqOptions = LP.SeqOptions()   # this request's settings (a field left alone: the engine's default); opts.rules holds its logits.TokenRules ...
    rules_id: Optional[int] = None   # ... and this their device rule set: created when the request is admitted, destroyed when it retires
    prefix: Optional[int] = None     # add_prefix() id whose rows are the first rows of embeds (None: prefill everything)
    guidance: Optional[float] = None # classifier-free guidance scale (None: off) against ...
    negative: object = None          # ... the negative prompt's embedding rows; neg_seq: its sequence, the follower of `seq` (Engine.seq_set_guidance)
    neg_seq: int = -1
    fan: int = 1                     # answers wanted from ONE prefill (num_return_sequences); back to 1 once admitted: its siblings are requests of their own then
    fan_rids: List[int] = field(default_factory=list)   # ... and the request ids reserved for the siblings

    @property
    def slots(self) -> int:          # a guided request holds two sequences, and two rows of every decode step; a queued fan-out needs room for all its answers
        return 2 if self.guidance is not None else self.fan


@dataclass
class _Prefix:
    seq: int                     # the holder sequence: owns the prefix's KV pages until drop_prefix and the last queued request that names it
    rows: int                    # P, a multiple of 128
    queued: int = 0              # requests in the queue that name it
    dropped: bool = False


class _Guided(Exception):
    """_admit: a guided request's settings are applied after its prefill"""


class ClipScheduler:
    """engine: anything with seq_alloc / seq_free / prefill_batch / decode_steps / seq_read (grounded_video_llm_amd.engine.Engine); requests that
    name a prefix also need seq_fork / prefill_extend_batch -- neither is called while no request does."""

    def __init__(self, engine, eos_id: Optional[int], max_active: int = 8, chunk: int = 8, max_prefill_rows: Optional[int] = None):
        if max_active < 1 or chunk < 1:
            raise ValueError("max_active and chunk must be >= 1")
        self.eng, self.eos, self.max_active, self.chunk = engine, eos_id, int(max_active), int(chunk)
        self.max_prefill_rows = max_prefill_rows
        self.queue: Deque[_Request] = deque()
        self.active: List[_Request] = []
        self.done: Dict[int, List[int]] = {}
        self.done_logprobs: Dict[int, tuple] = {}    # rid -> (lp, top) of a finished request that asked for them (logprobs())
        self._next = 0
        self.prefixes: Dict[int, _Prefix] = {}
        self._next_prefix = 0
        self._rule_holders: Dict[int, int] = {}      # device rule set -> requests that still hold it (the answers of one fan-out share their request's set)
        self.stats = {"prefill_calls": 0, "decode_chunks": 0, "decode_seq_steps": 0, "wasted_seq_steps": 0, "max_concurrent": 0, "prefix_rows_saved": 0}

    # ---- public ------------------------------------------------------------------------------------------
    def add_prefix(self, embeds) -> int:
        """Prefill the first P = len(embeds) // 128 * 128 rows of `embeds` (a clip's system prompt + visual rows, or a whole spliced prompt about it) once, into a
        holder sequence, and return an id for submit(..., prefix=).  128 rather than the 64 of a KV page: whole query blocks too, so that the rows behind the
        prefix are computed exactly as in a full prefill and a request's ids do not depend on whether it named the prefix (generate_shared's rule).
        The holder's pages stay resident until drop_prefix."""
        P = int(embeds.shape[0]) // 128 * 128
        if P < 128:
            raise ValueError(f"a shared prefix needs at least 128 rows, not {int(embeds.shape[0])}")
        seq = self.eng.seq_alloc(P)
        try:
            self.eng.prefill_batch([seq], [embeds[:P]])
        except Exception:
            self.eng.seq_free(seq)
            raise
        self.prefixes[self._next_prefix] = _Prefix(seq, P)
        self._next_prefix += 1
        return self._next_prefix - 1

    def drop_prefix(self, pid: int):
        """No new request may name `pid`.  Its holder is freed as soon as no QUEUED request names it (now, if none does); requests already admitted keep the
        pages alive through their own references."""
        p = self.prefixes.get(pid)
        if p is None or p.dropped:
            raise KeyError(f"prefix {pid}: unknown or already dropped")
        p.dropped = True
        self._release_prefix(pid)

    def submit(self, embeds, max_new_tokens: int, repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
               min_new_tokens: Optional[int] = None, logprobs: Optional[int] = None, bad_words_ids=None, sequence_bias=None, suppress_tokens=None,
               begin_suppress_tokens=None, forced_eos_token_id=None, do_sample: Optional[bool] = None, temperature: Optional[float] = None,
               top_k: Optional[int] = None, top_p: Optional[float] = None, min_p: Optional[float] = None, typical_p: Optional[float] = None,
               epsilon_cutoff: Optional[float] = None, eta_cutoff: Optional[float] = None, seed: Optional[int] = None, prefix: Optional[int] = None,
               grammar: Optional[int] = None, guidance_scale: Optional[float] = None, negative=None, num_return_sequences: Optional[int] = None,
               num_beam_groups: Optional[int] = None, diversity_penalty: Optional[float] = None, penalty_alpha: Optional[float] = None):
        """Queue one request.  embeds: the full spliced prompt.  prefix: an add_prefix() id -- the caller promises that the prompt's first P rows ARE the registered
        ones; only embeds[P:] (at least one row) is then prefilled.  An optimisation only: the result is the same without it.  (It is ignored for a request that
        LongRoPE forbids to share: P <= rope_orig_max_pos < len(embeds) -- a full prefill of that prompt ropes the shared rows with the long factors.)
        repetition_penalty / no_repeat_ngram_size / min_new_tokens: HF's logits processors for THIS request (HF's validation;
        applied on the device to its generated ids; min_new_tokens needs the scheduler's eos id).  Requests with different settings share one
        decode group.  None for all three: the sequence keeps the engine's default (Engine.set_logits_processors).
        logprobs: 0 = the log-probability of every generated id, 1 .. 8 = also its top N alternatives (Engine.seq_set_logprobs); read back
        with logprobs(rid) once the request finished.
        bad_words_ids / sequence_bias / suppress_tokens / begin_suppress_tokens / forced_eos_token_id: HF's token rules for THIS request
        (logits.resolve_rules: HF's validation; forced eos at this request's max_new_tokens); its device rule set lives from admission to
        retirement.  None for all five: the sequence keeps the engine's default (Engine.set_token_rules).
        do_sample / temperature / top_k / top_p / min_p / typical_p / epsilon_cutoff / eta_cutoff / seed: THIS request's own token selection
        (logits.request_sampling: HF's validation and defaults; Engine.seq_set_sampling at admission, random stream 0 of `seed`): greedy next to
        sampled neighbours, or sampled with its own warpers.  Its ids are a function of its own settings and logits alone -- not of max_active,
        chunk, or the other requests.  None for all nine: the request follows the engine's setting (Engine.set_sampling).
        grammar: an Engine.grammar_create id that constrains THIS request's answer (the caller owns the grammar and destroys it after the request
        retired); None: the sequence keeps the engine's default (Engine.set_grammar).
        guidance_scale / negative: HF's classifier-free guidance for THIS request (logits.resolve_guidance: None or 1 = off) against the negative prompt whose
        embedding rows `negative` holds.  The request runs as a pair of sequences -- the negative one follows it as one more row of every decode step
        (Engine.seq_set_guidance) -- so it counts as TWO toward max_active; its ids do not depend on its neighbours, max_active or chunk.  Not with prefix=.  Its own
        settings are applied behind its prefill (guidance works on the raw first rows): engine-wide default processors, rules or a grammar must be off for it.
        num_return_sequences = n > 1 (HF's; needs a sampled setting of the request's own): n sampled answers to this ONE prompt -- a LIST of n request ids is returned, one per answer.  The
        prompt is prefilled once; at admission the sequence is fanned out into its n - 1 siblings (Engine.seq_fanout: the prompt's KV pages are shared), answer j drawing
        from random stream j of `seed`.  The request counts as n toward max_active and is admitted only when n slots (and the KV pages of all answers) are free; from
        then on every answer is a request of its own that retires on its own eos.  Each answer's ids depend on its settings, its stream and its logits alone -- not on
        max_active, chunk or its neighbours.  Not with guidance_scale.
        num_beam_groups / diversity_penalty: the scheduler decodes greedily or by sampling, never by beams -- anything but (None / 1, None / 0) raises ValueError
        (generate() runs diverse beam search).
        penalty_alpha: with top_k it would select HF's contrastive search (logits.resolve_contrastive), which the scheduler does not run -- ValueError
        (generate() takes it); a penalty_alpha that selects nothing (None, 0, or with do_sample) is accepted and has no effect, as in HF."""
        if LP.resolve_contrastive(dict(penalty_alpha=penalty_alpha, top_k=top_k, do_sample=bool(do_sample))) is not None:
            raise ValueError("ClipScheduler: contrastive search (penalty_alpha > 0 with top_k > 1) is not supported; generate() takes it")
        if num_beam_groups not in (None, 1) or diversity_penalty not in (None, 0, 0.0):
            raise ValueError("ClipScheduler: num_beam_groups / diversity_penalty (diverse beam search) are not supported; generate() takes them")
        n_fan = 1 if num_return_sequences is None else int(num_return_sequences)
        if n_fan < 1:
            raise ValueError(f"`num_return_sequences` has to be a strictly positive integer, but is {n_fan}")
        if n_fan > 1:
            if LP.resolve_guidance(dict(guidance_scale=guidance_scale)) is not None:
                raise ValueError("guidance_scale with num_return_sequences > 1 is not supported yet")
            if n_fan > self.max_active:
                raise ValueError(f"a request with num_return_sequences={n_fan} counts as {n_fan} toward max_active, which is {self.max_active}")
        guidance = LP.resolve_guidance(dict(guidance_scale=guidance_scale))
        if guidance is not None:
            if negative is None:
                raise ValueError("guidance_scale != 1 needs `negative`: the embedding rows of the negative prompt")
            if prefix is not None:
                raise ValueError("a guided request cannot name a prefix")
            if self.max_active < 2:
                raise ValueError("a guided request counts as two toward max_active, which is 1")
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        if logprobs is not None and (isinstance(logprobs, bool) or not isinstance(logprobs, int) or not 0 <= logprobs <= 8):
            raise ValueError(f"logprobs must be None or an integer in 0 .. 8, not {logprobs!r}")
        pkw = dict(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_new_tokens=min_new_tokens)
        procs = LP.resolve(pkw, self.eos) if any(v is not None for v in pkw.values()) else None
        rules = ...
        rkw = dict(bad_words_ids=bad_words_ids, sequence_bias=sequence_bias, suppress_tokens=suppress_tokens,
                   begin_suppress_tokens=begin_suppress_tokens, forced_eos_token_id=forced_eos_token_id)
        if any(v is not None for v in rkw.values()):
            rules = LP.resolve_rules(rkw, self.eos, int(max_new_tokens), getattr(getattr(self.eng, "geo", None), "vocab", None))
        sampling = LP.request_sampling(do_sample, temperature, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff, seed)
        if n_fan > 1 and (sampling is ... or not sampling.get("do_sample")):      # the answers differ by their random streams only: the request's own sampled setting
            raise ValueError(f"Greedy methods without beam search do not support `num_return_sequences` different than 1 (got {n_fan}): give the request its own "
                             "sampling (do_sample=True, or any of temperature / top_k / top_p / ... / seed)")
        if prefix is not None:
            p = self.prefixes.get(prefix)
            if p is None or p.dropped:
                raise KeyError(f"prefix {prefix}: unknown or dropped")
            S = int(embeds.shape[0])
            if S <= p.rows:
                raise ValueError(f"a request behind a prefix of {p.rows} rows needs at least one row of its own, not {S} in all")
            geo = getattr(self.eng, "geo", None)
            omax = getattr(geo, "rope_orig_max_pos", 0) if getattr(geo, "rope_long", None) is not None else 0
            if omax > 0 and p.rows <= omax < S:
                prefix = None
            else:
                p.queued += 1
        r = _Request(self._next, embeds, int(max_new_tokens), opts=LP.SeqOptions(procs, logprobs, rules, sampling, ... if grammar is None else int(grammar)), prefix=prefix,
                     guidance=guidance, negative=negative if guidance is not None else None, fan=n_fan)
        self._next += 1
        if n_fan > 1:
            r.fan_rids = list(range(self._next, self._next + n_fan - 1))
            self._next += n_fan - 1
        self.queue.append(r)
        return r.rid if n_fan == 1 else [r.rid] + r.fan_rids

    def logprobs(self, rid: int):
        """(lp, top) of a finished request submitted with logprobs: lp[i] = the log-probability of its i-th id, top[i] = its top N (id,
        log-probability) pairs (None for logprobs=0); truncated exactly like its ids."""
        if rid not in self.done_logprobs:
            raise KeyError(f"request {rid}: not finished, or submitted without logprobs")
        return self.done_logprobs[rid]

    def pending(self) -> int:
        return len(self.queue) + len(self.active)

    def step(self) -> List[int]:
        """One scheduler iteration: admit -> decode chunk -> retire.  Returns the ids of the requests that finished."""
        self._admit()
        finished = self._retire()                # a request can finish on its prefill token (eos first, or max_new == 1)
        if self.active:
            k = min([self.chunk] + [r.max_new - r.n_gen for r in self.active])
            self.eng.decode_steps([r.seq for r in self.active], k)          # (a guided request's follower is stepped with it: only leaders are named)
            self.stats["decode_chunks"] += 1
            self.stats["decode_seq_steps"] += k * len(self.active)
            for r in self.active:
                r.n_gen += k
            finished += self._retire()
        return finished

    def run(self) -> Dict[int, List[int]]:
        while self.pending():
            before = (len(self.queue), len(self.active))
            self.step()
            if not self.active and self.queue and before == (len(self.queue), 0):
                raise L.GvlError("scheduler: the head request does not fit the KV pool / prefill workspace even on an idle engine")
        out, self.done = self.done, {}
        return out

    # ---- internals ---------------------------------------------------------------------------------------
    def _admit(self):
        new: List[_Request] = []
        fanned: List[_Request] = []                          # fan-out requests (prefilled on admission) and their siblings
        rows = 0
        while self.queue and sum(q.slots for q in self.active + new) + sum(q not in new for q in fanned) + self.queue[0].slots <= self.max_active:
            r = self.queue[0]
            S = int(r.embeds.shape[0])
            P = self.prefixes[r.prefix].rows if r.prefix is not None else 0     # rows the request does not prefill
            if self.max_prefill_rows is not None and new and rows + S - P > self.max_prefill_rows:
                break                                        # next iteration: keep the newcomers' prefill inside the workspace
            max_seq = getattr(getattr(self.eng, "geo", None), "max_seq", None)
            cap = S + r.max_new if max_seq is None else min(S + r.max_new, int(max_seq))
            Sn = int(r.negative.shape[0]) if r.guidance is not None else 0
            if max_seq is not None and Sn:                   # the follower needs as much room behind its prompt as the leader keeps
                cap = min(cap, S + int(max_seq) - Sn)
            if cap < S:
                raise ValueError(f"request {r.rid}: {S} prefill tokens exceed the engine's max_seq {max_seq}")
            try:
                r.seq = self.eng.seq_fork(self.prefixes[r.prefix].seq, P, cap) if P else self.eng.seq_alloc(cap)
            except L.GvlError as e:
                if getattr(e, "status", 0) == L.ERR_OOM:     # KV pages exhausted: wait for a retirement (FIFO, no overtaking)
                    break
                raise
            if r.guidance is not None:
                try:
                    r.neg_seq = self.eng.seq_alloc(Sn + cap - S)
                except L.GvlError as e:
                    self.eng.seq_free(r.seq)
                    if getattr(e, "status", 0) == L.ERR_OOM:
                        break
                    raise
            try:
                if r.guidance is not None:                   # its settings follow its prefill (below): guidance needs the raw first rows
                    raise _Guided()
                if r.opts.rules is not ... and r.opts.rules.active:    # an inactive set still overrides the engine's default: this request runs without rules
                    r.rules_id = self.eng.rules_create(r.opts.rules)
                LP.apply_seq_options(self.eng, r.seq, r.opts if r.opts.rules is ... else replace(r.opts, rules=r.rules_id))
            except _Guided:
                pass
            except Exception:
                self._free(r)
                self._drop_rules(r)
                raise
            r.max_new = min(r.max_new, cap - S + 1)          # generate() stops at the context limit (Engine.generate_ids does too)
            if r.fan > 1:                                    # n answers from one prefill: prefill now, with its logits, and fan out -- all siblings or none
                try:
                    sibs = self._fan_out(r, cap, P)
                except Exception as e:
                    self._free(r)
                    self._drop_rules(r)
                    if getattr(e, "status", 0) == L.ERR_OOM and isinstance(e, L.GvlError):
                        break                                # KV pages for all n answers: wait for a retirement
                    raise
                fanned += [r] + sibs
            self.queue.popleft()
            new.append(r)
            rows += S - P
            if P:                                            # the fork holds the pages now
                self.prefixes[r.prefix].queued -= 1
                self._release_prefix(r.prefix)
                self.stats["prefix_rows_saved"] += P
                r.embeds = r.embeds[P:]
        plain = [r for r in new if r.guidance is None and r not in fanned]
        for r in new:                                        # a guided request: both prompts prefilled with their logits, then bound -- the first token is guided too
            if r.guidance is not None:
                lc, lu = self.eng.prefill(r.seq, r.embeds, want_logits=True), self.eng.prefill(r.neg_seq, r.negative, want_logits=True)
                if r.opts.rules is not ... and r.opts.rules.active:
                    r.rules_id = self.eng.rules_create(r.opts.rules)
                LP.apply_seq_options(self.eng, r.seq, r.opts if r.opts.rules is ... else replace(r.opts, rules=r.rules_id))
                self.eng.seq_set_guidance(r.seq, r.neg_seq, r.guidance, lc, lu)
                r.negative = None
                self.stats["prefill_calls"] += 1
        if new:
            self._prefill(plain)
            for r in new:
                r.n_gen = 1
                r.embeds = None                              # the KV cache holds it now
            for r in new:                                    # a fan-out's answers stand together, in the order of their request ids
                self.active += [q for q in fanned if q is r or q.rid in r.fan_rids] if r.fan_rids else [r]
                r.fan_rids = []
            self.stats["max_concurrent"] = max(self.stats["max_concurrent"], sum(r.slots for r in self.active))

    def _fan_out(self, r: _Request, cap: int, P: int) -> List[_Request]:
        """Prefill `r` (behind its prefix, when it names one) and make its r.fan - 1 siblings, each a request of its own: answer j draws from stream j of the request's
        seed (the source, answer 0, from stream 0 -- what a plain sampled request does).  A failure leaves no sibling behind."""
        first = self.eng.prefill_extend(r.seq, r.embeds[P:], want_logits=True) if P else self.eng.prefill(r.seq, r.embeds, want_logits=True)   # (the fork holds the first P rows)
        self.stats["prefill_calls"] += 1
        seqs: List[int] = []
        try:
            for j0 in range(1, r.fan, 15):
                seqs += self.eng.seq_fanout(r.seq, min(15, r.fan - j0), cap, list(range(j0, min(r.fan, j0 + 15))), first)
        except Exception:
            for s_ in seqs:
                self.eng.seq_free(s_)
            raise
        if r.rules_id is not None:
            self._rule_holders[r.rules_id] = r.fan
        sibs = [_Request(rid, None, r.max_new, seq=s_, n_gen=1, opts=r.opts, rules_id=r.rules_id) for rid, s_ in zip(r.fan_rids, seqs)]
        r.fan = 1
        return sibs

    def _free(self, r: _Request):
        self.eng.seq_free(r.seq)                             # the leader first: freeing it unbinds the pair
        if r.neg_seq >= 0:
            self.eng.seq_free(r.neg_seq)
            r.neg_seq = -1

    def _prefill(self, new: List[_Request]):
        if new:
            if any(r.prefix is not None for r in new):       # one ragged pass for all newcomers, each behind its own prefix (none = empty)
                self.eng.prefill_extend_batch([r.seq for r in new], [r.embeds for r in new])
            else:
                self.eng.prefill_batch([r.seq for r in new], [r.embeds for r in new])
            self.stats["prefill_calls"] += 1

    def _release_prefix(self, pid: int):
        p = self.prefixes[pid]
        if p.dropped and p.queued == 0:
            del self.prefixes[pid]
            self.eng.seq_free(p.seq)

    def _drop_rules(self, r: _Request):
        if r.rules_id is not None:
            rid, r.rules_id = r.rules_id, None
            left = self._rule_holders.get(rid, 1) - 1        # the answers of one fan-out share the set: the last one to retire destroys it
            if left > 0:
                self._rule_holders[rid] = left
                return
            self._rule_holders.pop(rid, None)
            self.eng.rules_destroy(rid)

    def _retire(self) -> List[int]:
        finished, keep = [], []
        for r in self.active:
            fresh = self.eng.seq_read(r.seq, len(r.ids), r.n_gen - len(r.ids)) if r.n_gen > len(r.ids) else []
            stop = False
            for i, t in enumerate(fresh):
                r.ids.append(t)
                if self.eos is not None and t == self.eos:
                    self.stats["wasted_seq_steps"] += len(fresh) - 1 - i
                    stop = True
                    break
            if stop or len(r.ids) >= r.max_new:
                if r.opts.logprobs is not None:              # before the slot is freed: its lists are reused by the next sequence
                    self.done_logprobs[r.rid] = LP.read_seq_logprobs(self.eng, r.seq, r.ids, r.opts)
                self._free(r)                                # seq_read synchronised the stream: no step of r is in flight
                self._drop_rules(r)
                self.done[r.rid] = r.ids
                finished.append(r.rid)
            else:
                keep.append(r)
        self.active = keep
        return finished


def generate_many(engine, embeds_list: Sequence, max_new_tokens: int, eos_id: Optional[int], max_active: int = 8, chunk: int = 8,
                  max_prefill_rows: Optional[int] = None) -> List[List[int]]:
    """Greedy ids of every request, in submission order (== [engine.generate_ids(e, max_new_tokens, eos_id) for e in embeds_list])."""
    sch = ClipScheduler(engine, eos_id, max_active, chunk, max_prefill_rows)
    rids = [sch.submit(e, max_new_tokens) for e in embeds_list]
    out = sch.run()
    return [out[r] for r in rids]
