"""HF generate()'s token rules (sequence_bias, bad_words_ids, forced_eos_token_id, suppress_tokens, begin_suppress_tokens) as the product
resolves them (grounded_video_llm_amd/logits.py) and as the device kernel applies them (csrc/gvl_logits.hip, restated in tests/token_rules_ref.py)
-- pinned against the installed transformers: its processor classes chained in `_get_logits_processor`'s order on CPU fp32 rows, and its own
generate(inputs_embeds=...) on a tiny LlamaForCausalLM, greedy and beam search.  No GPU.

What HF shows (and the product follows): begin_index is 0 and the forced-eos step is history length == max_new_tokens - 1, as expected; but a
multi-token sequence_bias / bad_words_ids entry is skipped while it is longer than the HISTORY (`len(sequence_ids) > input_ids.shape[1]`), not
while it is longer than the history plus one -- with inputs_embeds a 2-token entry first applies at the third new token."""
import math
import warnings

import pytest
import torch

from grounded_video_llm_amd import logits as LP
from grounded_video_llm_amd.beam import beam_search
from test_logits_processors_cpu import _fwd, _hf, _tiny
from token_rules_ref import restate_rules

V = 64


def _hf_chain(kw, eos, max_new, penalty=1.0, ngram=0, min_new=0):
    """HF's own processor objects in _get_logits_processor's order (input_ids = the generated ids: no prompt ids with inputs_embeds)."""
    from transformers.generation import logits_process as H
    ps = []
    if kw.get("sequence_bias") is not None:
        ps.append(H.SequenceBiasLogitsProcessor(sequence_bias=kw["sequence_bias"]))
    if penalty != 1.0:
        ps.append(H.RepetitionPenaltyLogitsProcessor(penalty=penalty))
    if ngram > 0:
        ps.append(H.NoRepeatNGramLogitsProcessor(ngram))
    if kw.get("bad_words_ids") is not None:
        ps.append(H.NoBadWordsLogitsProcessor(kw["bad_words_ids"], torch.tensor([eos])))
    if min_new > 0:
        ps.append(H.MinLengthLogitsProcessor(min_new, torch.tensor([eos])))
    if kw.get("forced_eos_token_id") is not None:
        ps.append(H.ForcedEOSTokenLogitsProcessor(max_new, kw["forced_eos_token_id"]))
    if kw.get("suppress_tokens") is not None:
        ps.append(H.SuppressTokensLogitsProcessor(kw["suppress_tokens"]))
    if kw.get("begin_suppress_tokens") is not None:
        ps.append(H.SuppressTokensAtBeginLogitsProcessor(kw["begin_suppress_tokens"], 0))
    return ps


def _rows():
    g = torch.Generator().manual_seed(5)
    x = torch.randn((3, V), generator=g) * 4.0
    x[:, ::7] = 0.0
    x[:, 3::11] = -0.0
    x[1, 5::13] = -math.inf
    return x


def test_restatement_equals_hf_processor_classes():
    eos = 2
    long_hist = [int(t) for t in torch.randint(0, V, (300,), generator=torch.Generator().manual_seed(1))] + [9, 8, 7]
    hists = [[], [7], [8, 7], [4, 9, 8, 7], [7, 7, 7, 30, 8, 7], long_hist]
    cases = [
        # a target hit by a length-1 bias plus two matching multi-token entries (different lengths): the sum order ((0 + a) + b) + c
        (dict(sequence_bias={(9, 8, 7, 11): 0.1, (11,): 1e8, (7, 11): -1e8, (8, 7, 12): 3.5, (13,): -2.25}), {}),
        (dict(sequence_bias=[[[7, 11], 0.3], [[11], 0.7], [[8, 7, 11], 1e-3]]), {}),
        # a biased token that is also in the history, with the penalty on: the bias lands BEFORE the penalty
        (dict(sequence_bias={(7,): 5.0, (30,): -3.0, (8, 7): 2.0}), dict(penalty=1.7)),
        (dict(sequence_bias={(7,): -5.0}), dict(penalty=0.6, ngram=2)),
        # an entry longer than the history; [eos] among the bad words (dropped); a bad word ending in a history token
        (dict(bad_words_ids=[[5], [8, 7, 21], [4, 9, 8, 7, 22], [eos], [7, 23], [7, 7]]), dict(penalty=1.3, ngram=2)),
        (dict(bad_words_ids=[[eos], [6]], sequence_bias={(6,): 100.0}), {}),
        # forced eos together with a suppressed eos: everything ends at -inf
        (dict(forced_eos_token_id=eos, suppress_tokens=[eos, 3, 63], begin_suppress_tokens=[1, 0]), dict(min_new=3)),
        (dict(forced_eos_token_id=[eos, 40]), dict(min_new=7, penalty=1.2)),
        (dict(suppress_tokens=list(range(10, 50)), begin_suppress_tokens=[eos, 9], bad_words_ids=[[9, 8, 7, 1]], sequence_bias={(8, 7, 1): 9.0}), dict(ngram=3)),
    ]
    checked = 0
    for kw, pk in cases:
        for hist in hists:
            for max_new in (len(hist) + 1, len(hist) + 2):                       # the forced step and a step before it
                rules = LP.resolve_rules(kw, eos, max_new, V)
                for row in _rows():
                    ref = row.clone()[None]
                    ids = torch.tensor([hist], dtype=torch.long)
                    for p in _hf_chain(kw, eos, max_new, **pk):
                        ref = p(ids, ref)
                    got = restate_rules(row, hist, rules, pk.get("penalty", 1.0), pk.get("ngram", 0), pk.get("min_new", 0), eos)
                    assert not torch.isnan(ref).any()
                    assert torch.equal(got, ref[0]), (kw, pk, hist[-6:], max_new)
                    checked += 1
    assert checked == len(cases) * len(hists) * 2 * 3
    # the points above, spelled out
    r = LP.resolve_rules(cases[0][0], eos, 99, V)
    z = torch.zeros(V)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    assert restate_rules(z, [9, 8, 7], r)[11] == ((f32(0.0) + f32(1e8)) + f32(0.1)) + f32(-1e8)      # length-1 first, then dict order
    assert restate_rules(z, [8, 7], r)[11] == 0.0 and restate_rules(z, [8, 7], r)[12] == 0.0         # (7, 11) applies; (8, 7, 12) is longer than the history
    assert restate_rules(z, [7], r)[11] == 1e8                                                         # (7, 11) is longer than a history of 1: skipped (HF)
    r = LP.resolve_rules(dict(sequence_bias={(7,): 5.0}), eos, 99, V)
    assert restate_rules(torch.full((V,), 1.0), [7], r, penalty=2.0)[7] == 3.0                         # (1 + 5) / 2, not 1 / 2 + 5
    r = LP.resolve_rules(dict(forced_eos_token_id=eos, suppress_tokens=[eos]), eos, 4, V)
    assert bool(torch.isinf(restate_rules(z, [1, 2, 3], r)).all()) and restate_rules(z, [1, 2], r)[5] == 0.0


def _greedy(m, E, emb, mx, eos, kw, procs=LP.OFF):
    rules = LP.resolve_rules(kw, eos, mx, m.config.vocab_size)
    ids = []
    while len(ids) < mx:
        t = int(torch.argmax(restate_rules(_fwd(m, E, emb, ids), ids, rules, *procs.args())))
        ids.append(t)
        if eos is not None and t == eos:
            break
    return ids


def _rule_cases(p, eos):
    """kwargs built from a plain run's ids p (vocabulary 50)."""
    unused = [t for t in range(1, 50) if t not in p and t != eos]
    return [dict(bad_words_ids=[[p[0]], p[2:4]]), dict(bad_words_ids=[p[1:3], [eos]], begin_suppress_tokens=[p[0], unused[0]]),
            dict(suppress_tokens=sorted(set(p[:3]))), dict(sequence_bias={(unused[1],): 50.0, (unused[1], unused[2]): 80.0, (p[0],): -1.0}),
            dict(sequence_bias=[[[p[1], unused[3]], 90.0]], repetition_penalty=1.4), dict(forced_eos_token_id=eos),
            dict(forced_eos_token_id=eos, suppress_tokens=[p[0]], begin_suppress_tokens=[p[1]], bad_words_ids=[p[2:5]],
                 sequence_bias={(unused[4],): 4.0}, no_repeat_ngram_size=2, min_new_tokens=3)]


def test_greedy_with_rules_equals_hf_generate():
    m, E = _tiny()
    changed = forced = 0
    for seed in range(3):
        emb = torch.randn((1, 7, 32), generator=torch.Generator().manual_seed(seed)) * 2.0
        p = _hf(m, emb, do_sample=False, max_new_tokens=12, eos_token_id=None)
        p = [t if t else 1 for t in p]                                        # list-form sequence_bias wants ids > 0
        for eos in (p[5], 49):
            for kw in _rule_cases(p, eos):
                ref = _hf(m, emb, do_sample=False, max_new_tokens=10, eos_token_id=eos, **kw)
                got = _greedy(m, E, emb, 10, eos, kw, LP.resolve(kw, eos, emb.shape[1]))
                assert got == ref, (seed, eos, kw, got, ref)
                changed += got != _hf(m, emb, do_sample=False, max_new_tokens=10, eos_token_id=eos)
                if "forced_eos_token_id" in kw and len(got) == 10:
                    assert got[-1] == eos                                     # pins the forced step: history length == max_new_tokens - 1
                    forced += 1
                if "begin_suppress_tokens" in kw:
                    assert got[0] not in kw["begin_suppress_tokens"]          # pins begin_index == 0
    assert changed > 10 and forced > 0


def test_beam_search_with_rules_equals_hf_generate():
    m, E = _tiny()
    checked = 0
    for seed in range(2):
        emb = torch.randn((1, 7, 32), generator=torch.Generator().manual_seed(seed)) * 2.0
        p = _hf(m, emb, num_beams=3, do_sample=False, max_new_tokens=8, eos_token_id=None)
        p = [t if t else 1 for t in p]
        eos = 49
        for kw in _rule_cases(p + p, eos):
            ref = _hf(m, emb, num_beams=3, do_sample=False, max_new_tokens=8, eos_token_id=eos, length_penalty=1.0, early_stopping=False, **kw)
            procs = LP.resolve(kw, eos, emb.shape[1])
            rules = LP.resolve_rules(kw, eos, 8, 50)
            beams = [[] for _ in range(3)]

            def step(parents, toks):
                beams[:] = [beams[p_] + [t] for p_, t in zip(parents, toks)]
                return torch.stack([_fwd(m, E, emb, b) for b in beams])

            def process(hists, lp):
                return torch.stack([restate_rules(lp[j], hists[j], rules, *procs.args()) for j in range(lp.shape[0])])
            got = beam_search(step, _fwd(m, E, emb, []), 3, 8, eos, 1.0, False, process=process)
            while ref and ref[-1] == 0 and len(ref) > len(got):
                ref = ref[:-1]
            assert got == ref, (seed, kw, got, ref)
            checked += 1
    assert checked == 14


def _hf_error(make):
    with pytest.raises(ValueError) as e:
        make()
    return str(e.value)


def test_kwarg_validation_raises_hf_messages():
    from transformers.generation import logits_process as H
    for sb in ({}, [], "x", {(1, 2): 1.0, 3: 2.0}, {(1, -2): 1.0}, {(): 1.0}, {(1, 2.5): 1.0}, {(1,): 1}, [[[0, 2], 1.0]], [[[1, 2], 1]], [[(1, 2), 1.0]]):
        want = _hf_error(lambda: H.SequenceBiasLogitsProcessor(sequence_bias=sb))
        with pytest.raises(ValueError) as e:
            LP.resolve_rules(dict(sequence_bias=sb), 2, 8, 50)
        assert str(e.value) == want, sb
    for bw in ([], "x", [3], [[1], 2], [[-1]], [[1.5]]):
        want = _hf_error(lambda: H.NoBadWordsLogitsProcessor(bw, torch.tensor([2])))
        with pytest.raises(ValueError) as e:
            LP.resolve_rules(dict(bad_words_ids=bw), 2, 8, 50)
        assert str(e.value) == want, bw
    assert not LP.resolve_rules(dict(bad_words_ids=[[2]]), 2, 8, 50).active      # only [eos]: HF builds a processor that bans nothing
    with pytest.raises(ValueError, match="non-empty"):
        LP.resolve_rules(dict(bad_words_ids=[[]]), 2, 8, 50)                     # HF: an IndexError at the first call
    for fe in (-1, [3, -2], [1.5]):
        want = _hf_error(lambda: H.ForcedEOSTokenLogitsProcessor(8, fe))
        with pytest.raises(ValueError) as e:
            LP.resolve_rules(dict(forced_eos_token_id=fe), 2, 8, 50)
        assert str(e.value) == want, fe
    # the vocabulary check HF makes at the first call
    p = H.SequenceBiasLogitsProcessor(sequence_bias={(3, 70): 1.0, (50,): 2.0})
    want = _hf_error(lambda: p(torch.zeros((1, 0), dtype=torch.long), torch.zeros((1, 50))))
    with pytest.raises(ValueError) as e:
        LP.resolve_rules(dict(sequence_bias={(3, 70): 1.0, (50,): 2.0}), 2, 8, 50)
    assert str(e.value) == want
    # what stays off: nothing given, None values
    assert not LP.resolve_rules({}, 2, 8, 50).active
    assert not LP.resolve_rules(dict(bad_words_ids=None, sequence_bias=None, suppress_tokens=None, forced_eos_token_id=None), 2, 8, 50).active
    assert LP.resolve_rules({}, 2, 8) == LP.NO_RULES
    assert set(LP.RULE_KWARGS) <= set(LP.KWARGS)
    # duplicate keys of the list form collapse as a dict does (the last bias wins, the first position stays)
    r = LP.resolve_rules(dict(sequence_bias=[[[4], 1.0], [[5], 2.0], [[4], 3.0]]), 2, 8, 50)
    assert r.sequence_bias.to_dict() == {(4,): 3.0, (5,): 2.0}
    r = LP.resolve_rules(dict(forced_eos_token_id=7, suppress_tokens=[3, 3, 99, -1], begin_suppress_tokens=(4,)), 2, 8, 50)
    assert (r.force_ids, r.force_at, r.suppress, r.begin_suppress, r.begin_index) == ((7,), 7, (3,), (4,), 0)


def test_grouping_by_target_round_trips():
    g = torch.Generator().manual_seed(3)
    d = {}
    for _ in range(400):
        n = int(torch.randint(1, 17, (1,), generator=g))
        ids = tuple(int(t) for t in torch.randint(0, 40, (n,), generator=g))
        d[ids] = float(torch.randn((), generator=g))
    t = LP.group_by_target(d)
    assert t.to_dict() == {k: float(torch.tensor(v, dtype=torch.float32)) for k, v in d.items()}
    assert len({x[0] for x in t.targets}) == len(t.targets) == len({k[-1] for k in d})       # one group per target token
    assert sum(x[2] for x in t.targets) == len(d) == len(t.entry_bias) == len(t.entry_prefix)
    order = list(d)
    for tk, e0, ne in t.targets:                                                               # length-1 first, then dict order
        keys = [tuple(t.prefix[o:o + n]) + (tk,) for o, n in t.entry_prefix[e0:e0 + ne]]
        multi = [k for k in keys if len(k) > 1]
        assert all(len(k) == 1 for k in keys[:len(keys) - len(multi)]) and len(keys) - len(multi) <= 1
        assert [order.index(k) for k in multi] == sorted(order.index(k) for k in multi)
    r = LP.resolve_rules(dict(bad_words_ids=[[1, 2], [3], [2], [9, 2]]), 3, 8, 50)              # [eos] dropped, bias -inf
    assert r.bad_words.to_dict() == {(1, 2): -math.inf, (2,): -math.inf, (9, 2): -math.inf}
    assert r.bad_words.targets == ((2, 0, 3),) and r.bad_words.entry_prefix == ((0, 0), (0, 1), (1, 1)) and r.bad_words.prefix == (1, 9)


def test_capacity_overflows_raise():
    ok = {(i, i + 1): 1.0 for i in range(LP.MAX_SEQS)}
    assert len(LP.group_by_target(ok).entry_bias) == LP.MAX_SEQS
    with pytest.raises(ValueError, match="multi-token entries exceed the limit of 1024"):
        LP.resolve_rules(dict(sequence_bias={**ok, (5000, 1): 1.0}), 2, 8)
    with pytest.raises(ValueError, match="exceeds the limit of 16 ids per entry"):
        LP.resolve_rules(dict(bad_words_ids=[list(range(1, 18))]), 2, 8)
    assert LP.resolve_rules(dict(bad_words_ids=[list(range(1, 17))]), 2, 8).bad_words.entry_prefix == ((0, 15),)
    with pytest.raises(ValueError, match="ids exceed the limit of 262144"):
        LP.resolve_rules(dict(suppress_tokens=range(LP.MAX_IDS + 1)), 2, 8)
    with pytest.raises(ValueError, match="single-token entries exceed the limit"):
        LP.group_by_target({(i,): 1.0 for i in range(LP.MAX_IDS + 1)})
    assert len(LP.resolve_rules(dict(suppress_tokens=range(128558 - 300)), 2, 8).suppress) == 128558 - 300   # a vocabulary-sized list fits


class _ScriptedEngine:
    """The ClipScheduler's engine surface on the CPU: every sequence emits its own seq id forever; records rule sets and their lifetime."""

    def __init__(self):
        self.n, self.live, self.gen, self.sets, self.seq_rules, self.log = 0, set(), {}, {}, {}, []

    def seq_alloc(self, cap):
        self.n += 1
        self.live.add(self.n)
        self.gen[self.n] = 0
        return self.n

    def seq_free(self, s):
        self.live.discard(s)
        self.log.append(("free", s))

    def rules_create(self, rules):
        rid = 10 + len(self.log)
        self.sets[rid] = rules
        self.log.append(("create", rid))
        return rid

    def rules_destroy(self, rid):
        assert rid in self.sets and not any(v == rid and s in self.live for s, v in self.seq_rules.items()), "destroyed while referenced"
        del self.sets[rid]
        self.log.append(("destroy", rid))

    def seq_set_token_rules(self, s, rid):
        assert s in self.live and (rid is None or rid in self.sets)
        self.seq_rules[s] = rid

    def prefill_batch(self, seqs, embeds):
        for s in seqs:
            self.gen[s] = 1

    def decode_steps(self, seqs, k):
        for s in seqs:
            self.gen[s] += k

    def seq_read(self, s, first, cap):
        return [100 + s] * max(0, min(self.gen[s] - first, cap))


def test_scheduler_sets_and_frees_per_request_rules():
    from grounded_video_llm_amd.serve import ClipScheduler
    eng = _ScriptedEngine()
    sch = ClipScheduler(eng, eos_id=2, max_active=4, chunk=3)
    emb = torch.zeros((5, 4))
    a = sch.submit(emb, 6, bad_words_ids=[[7], [8, 9], [2]], forced_eos_token_id=2)
    b = sch.submit(emb, 4)
    c = sch.submit(emb, 9, sequence_bias={(5,): 2.0}, suppress_tokens=[1, 3], begin_suppress_tokens=[4])
    sch.step()
    assert set(eng.seq_rules) == {1, 3} and len(eng.sets) == 2                  # request b keeps the engine's default: no call
    ra, rc = eng.sets[eng.seq_rules[1]], eng.sets[eng.seq_rules[3]]
    assert ra == LP.resolve_rules(dict(bad_words_ids=[[7], [8, 9], [2]], forced_eos_token_id=2), 2, 6) and ra.force_at == 5
    assert ra.bad_words.to_dict() == {(7,): -math.inf, (8, 9): -math.inf}
    assert rc.sequence_bias.to_dict() == {(5,): 2.0} and rc.suppress == (1, 3) and rc.begin_suppress == (4,) and not rc.force_ids
    out = sch.run()
    assert [len(out[r]) for r in (a, b, c)] == [6, 4, 9]
    assert eng.sets == {} and not eng.live                                      # every set is freed when its request retires ...
    for s_, rid in eng.seq_rules.items():
        assert eng.log.index(("free", s_)) < eng.log.index(("destroy", rid))    # ... after its sequence
    with pytest.raises(ValueError):
        sch.submit(emb, 4, bad_words_ids=[])
    with pytest.raises(ValueError):
        sch.submit(emb, 4, sequence_bias={(1,): 1})
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert sch.pending() == 0
