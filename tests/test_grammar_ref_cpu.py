"""The torch restatement of the token-selection pipeline with the grammar stage (tests/grammar_ref.py) pinned to the installed transformers: its own processor
classes, PrefixConstrainedLogitsProcessor included, chained in `_get_logits_processor`'s order on CPU fp32 rows, with the grammar handed to HF as
Grammar.as_prefix_allowed_tokens_fn().  And the grounding grammars themselves: the "interval" language is exactly `From <s> to <e>.` + eos with s <= e -- all
301 * 302 / 2 pairs are walked through Grammar.allowed.  No GPU."""
import inspect
import math

import numpy as np
import pytest
import torch

from grammar_ref import grammar_stage, restate, same_bits
from grounded_video_llm_amd import grammar as GR, logits as LP
from grounded_video_llm_amd.model import SyntheticTokenizer
from test_token_rules_cpu import _hf_chain

V, N, EOS = 640, 300, 2
TOK = SyntheticTokenizer(V, N)
T0 = TOK.tok2id["<0>"]                                                           # <k> = T0 + k
FROM, TO, DOT = (TOK._word(w) for w in ("From", "to", "."))


@pytest.fixture(scope="module")
def interval():
    return GR.grounding_grammar(TOK, N, EOS, "interval")


@pytest.fixture(scope="module")
def ordered():
    return GR.grounding_grammar(TOK, N, EOS, "ordered")


def _hf_pipeline(grammar, kw, max_new, penalty=1.0, ngram=0, min_new=0):
    """_hf_chain with PrefixConstrainedLogitsProcessor where the installed _get_logits_processor puts it: after MinLength / MinNewTokens, before ForcedEOS"""
    from transformers.generation import logits_process as H
    ps = _hf_chain(kw, EOS, max_new, penalty, ngram, min_new)
    at = next((i for i, p in enumerate(ps) if isinstance(p, (H.ForcedEOSTokenLogitsProcessor, H.SuppressTokensLogitsProcessor, H.SuppressTokensAtBeginLogitsProcessor))), len(ps))
    ps.insert(at, H.PrefixConstrainedLogitsProcessor(grammar.as_prefix_allowed_tokens_fn(), 1))
    return ps


def test_hf_puts_the_prefix_constraint_after_min_length_and_before_forced_eos():
    from transformers.generation.utils import GenerationMixin
    src = inspect.getsource(GenerationMixin._get_logits_processor)
    order = [src.index(name + "(") for name in ("NoBadWordsLogitsProcessor", "MinLengthLogitsProcessor", "MinNewTokensLengthLogitsProcessor", "PrefixConstrainedLogitsProcessor",
                                                "ForcedEOSTokenLogitsProcessor", "SuppressTokensLogitsProcessor")]
    assert order == sorted(order), order


def _rows(n=3):
    g = torch.Generator().manual_seed(7)
    x = torch.randn((n, V), generator=g) * 4.0
    x[:, ::7] = 0.0
    x[:, 3::11] = -0.0
    x[1, 5::13] = -math.inf
    x[:, T0 + 150] = -0.0                                                        # an ALLOWED -0.0: HF's `scores + mask` turns it into +0.0
    return x


# (name, history, masked?): empty, mid-literal, just after SET, reg at 0 / 150 / 300, END, OFF by a forbidden id, OFF by an out-of-range id
HISTORIES = [("empty", [], True), ("mid-literal", [FROM], True), ("after SET", [FROM, T0 + 36], True), ("reg 0", [FROM, T0, TO], True),
             ("reg 150", [FROM, T0 + 150, TO], True), ("reg 300", [FROM, T0 + 300, TO], True), ("before eos", [FROM, T0 + 36, TO, T0 + 64, DOT], True),
             ("END", [FROM, T0 + 36, TO, T0 + 64, DOT, EOS], False), ("OFF forbidden", [FROM, 17], False), ("OFF GE", [FROM, T0 + 64, TO, T0 + 36], False),
             ("OFF out of range", [FROM, V], False)]


def test_restatement_equals_hf_processor_classes(interval, ordered):
    cases = [({}, {}),
             ({}, dict(min_new=40)),                                              # min-length ban and grammar both hit eos
             (dict(forced_eos_token_id=EOS), {}),                                 # forced eos overrides the grammar (at history length max_new - 1)
             (dict(suppress_tokens=[FROM, T0 + 200, DOT], begin_suppress_tokens=[TO]), dict(penalty=1.3)),       # a suppress list after it
             (dict(sequence_bias={(T0 + 10,): 5.0, (FROM, T0 + 11): 2.0}, bad_words_ids=[[T0 + 12], [TO, T0 + 13]]), dict(ngram=2, min_new=3))]
    checked = 0
    for grammar in (interval, ordered):
        for kw, pk in cases:
            for name, hist, _ in HISTORIES:
                if max(hist, default=0) >= V and (pk.get("penalty", 1.0) != 1.0 or pk.get("ngram", 0)):
                    continue                                                      # HF's penalty / n-gram processors index the row with the history: no id outside it for them
                for max_new in (len(hist) + 1, len(hist) + 3):
                    rules = LP.resolve_rules(kw, EOS, max_new, V) if kw else None
                    ids = torch.tensor([hist], dtype=torch.long)
                    for row in _rows():
                        ref = row.clone()[None]
                        for p in _hf_pipeline(grammar, kw, max_new, **pk):
                            ref = p(ids, ref)
                        got = restate(row, hist, grammar, rules, pk.get("penalty", 1.0), pk.get("ngram", 0), pk.get("min_new", 0), EOS)
                        assert not torch.isnan(ref).any()
                        assert torch.equal(got, ref[0]), (name, kw, pk, max_new)
                        checked += 1
    assert checked > 500


def test_the_interplay_spelled_out(interval):
    row = _rows()[0]
    h = [FROM, T0 + 36, TO, T0 + 64, DOT]                                        # only eos is allowed now
    assert np.nonzero(interval.allowed(h))[0].tolist() == [EOS]
    s = restate(row, h, interval)
    assert s[EOS] == row[EOS] and bool(torch.isinf(s[torch.arange(V) != EOS]).all())
    assert bool(torch.isinf(restate(row, h, interval, min_new=40, eos=EOS)).all())                      # the min-length ban lands first: nothing is left
    r = LP.resolve_rules(dict(forced_eos_token_id=EOS), EOS, 3, V)
    s = restate(row, [FROM, T0 + 5], interval, r)                                                        # forced eos at history length 2 overrides the grammar
    assert s[EOS] == 0.0 and bool(torch.isinf(s[torch.arange(V) != EOS]).all())
    r = LP.resolve_rules(dict(suppress_tokens=[T0 + 7]), EOS, 99, V)
    s = restate(row, [FROM], interval, r)
    assert math.isinf(float(s[T0 + 7])) and s[T0 + 8] == row[T0 + 8] and math.isinf(float(s[FROM]))     # a suppress list after it
    # an allowed -0.0 becomes +0.0 (HF's add); OFF and END rows keep every bit
    s = grammar_stage(row, [FROM], interval)
    assert float(row[T0 + 150]) == 0.0 and math.copysign(1.0, float(row[T0 + 150])) < 0 < math.copysign(1.0, float(s[T0 + 150]))
    for name, hist, masked in HISTORIES:
        assert same_bits(grammar_stage(row, hist, interval), row) == (not masked), name


def test_interval_language_is_exactly_from_s_to_e_dot_eos(interval):
    g = interval
    assert g.vocab == V and np.nonzero(g.allowed([]))[0].tolist() == [FROM]
    assert np.nonzero(g.allowed([FROM]))[0].tolist() == list(range(T0, T0 + N + 1))                     # <0> .. <300>, not <timestamp_grounding>
    assert TOK.tok2id["<timestamp_grounding>"] == T0 + N + 1 and all(not g.allowed(h)[T0 + N + 1] for h in ([], [FROM], [FROM, T0, TO]))
    pairs = 0
    for s in range(N + 1):
        assert np.nonzero(g.allowed([FROM, T0 + s]))[0].tolist() == [TO]
        assert np.nonzero(g.allowed([FROM, T0 + s, TO]))[0].tolist() == list(range(T0 + s, T0 + N + 1))    # exactly the e >= s
        for e in range(s, N + 1):
            h = [FROM, T0 + s, TO, T0 + e]
            assert np.nonzero(g.allowed(h))[0].tolist() == [DOT] and np.nonzero(g.allowed(h + [DOT]))[0].tolist() == [EOS]
            pairs += 1
    assert pairs == 301 * 302 // 2
    # the accepted sentences are the tokenisations of the answers, and nothing else of that shape
    for s, e in ((0, 0), (36, 64), (0, 300), (300, 300), (150, 151)):
        assert g.accepts(TOK(f"From <{s}> to <{e}>.")[1:] + [EOS])
    for bad in ([FROM, T0 + 64, TO, T0 + 36, DOT, EOS], [FROM, T0 + 36, TO, T0 + 64, DOT], [FROM, T0 + 36, DOT, EOS], [T0 + 36, TO, T0 + 64, DOT, EOS],
                [FROM, T0 + 36, TO, T0 + 64, EOS], [FROM, T0 + 36, TO, T0 + 64, DOT, EOS, EOS], [FROM, T0 + N + 1, TO, T0 + 64, DOT, EOS]):
        assert not g.accepts(bad), bad


def test_ordered_language(ordered):
    g = ordered
    w = [TOK._word(x) for x in ("the", "person", "opens")]
    ok = [w[0], T0 + 5, w[1], T0 + 5, w[2], T0 + 100, T0 + 300, EOS]
    assert g.accepts(ok) and g.accepts([EOS]) and g.accepts(w + [EOS])
    assert not g.accepts([w[0], T0 + 5, EOS])                                    # eos only between pairs
    assert not g.accepts([T0 + 64, w[0], T0 + 36, EOS])                          # the pair's end before its start
    m = g.allowed([T0 + 64, w[0]])
    assert not m[EOS] and not m[T0 + 63] and m[T0 + 64] and m[w[1]] and m[T0 + N + 1]
    assert g.allowed([T0 + 64, T0 + 70])[EOS] and g.allowed([T0 + 64, T0 + 70])[T0]                     # a new pair starts anywhere


def test_grounding_grammar_errors():
    with pytest.raises(ValueError, match="mode must be"):
        GR.grounding_grammar(TOK, N, EOS, "free")
    with pytest.raises(ValueError, match="is not one token|not one contiguous"):
        GR.grounding_grammar(TOK, N + 5, EOS)                                     # <301> .. are not temporal tokens of this tokenizer


def test_grounding_grammar_over_a_vocabulary_larger_than_the_tokenizer(interval, ordered):
    """A model's vocabulary (its embedding rows) may outnumber its tokenizer's entries (Phi-3.5: 32 064 rows, about 32 011 tokens, both plus the added ones): the
    grammar classifies the MODEL's ids; the rows past the tokenizer are class 0 -- never allowed in "interval", other-tokens in "ordered" -- and the language over
    the tokenizer's ids is the one of the tokenizer-sized grammar."""
    W = V + 53
    assert len(TOK) == V
    for small, mode in ((interval, "interval"), (ordered, "ordered")):
        g = GR.grounding_grammar(TOK, N, EOS, mode, vocab=W)
        assert g.vocab == W and small.vocab == V and not g.token_class[V:].any()
        assert (g.token_class[:V] == small.token_class).all() and (g.trans == small.trans).all() and (g.class_base == small.class_base).all()
        for h in ([], [FROM], [FROM, T0 + 36], [FROM, T0 + 36, TO], [FROM, T0 + 36, TO, T0 + 64], [FROM, T0 + 36, TO, T0 + 64, DOT], [T0 + 64, TOK._word("the")]):
            a, b = g.allowed(h), small.allowed(h)
            assert (a is None) == (b is None)
            if a is not None:
                assert (a[:V] == b).all() and a[V:].tolist() == [mode == "ordered"] * 53, (mode, h)
    g = GR.grounding_grammar(TOK, N, EOS, "interval", vocab=W)
    assert g.accepts(TOK("From <36> to <64>.")[1:] + [EOS]) and not g.accepts([FROM, T0 + 36, TO, T0 + 64, DOT, V + 1])
    assert GR.grounding_grammar(TOK, N, EOS, "ordered", vocab=W).accepts([V + 1, T0 + 5, W - 1, T0 + 5, EOS])
    with pytest.raises(ValueError, match=f"vocab is {V - 1}, the tokenizer holds {V}"):
        GR.grounding_grammar(TOK, N, EOS, "interval", vocab=V - 1)


def test_cli_constrain_grounding_builds_the_grammar_over_the_models_vocabulary(capsys):
    """inference.py --constrain_grounding: the grounding call gets the "interval" grammar over model.geo.vocab (not len(tokenizer)), the flag is off by default,
    and its clash with --share_visual is an argument error -- raised while parsing, before any model is built."""
    import os
    import sys
    import types
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import inference
    model = types.SimpleNamespace(tokenizer=TOK, geo=types.SimpleNamespace(vocab=V + 53))
    assert inference.grounding_constraint(inference.parse_args(["--synthetic"]), model) == {}
    kw = inference.grounding_constraint(inference.parse_args(["--synthetic", "--constrain_grounding"]), model)
    g = kw["grammar"]
    assert list(kw) == ["grammar"] and g.vocab == V + 53 and g.accepts(TOK("From <36> to <64>.")[1:] + [TOK.eos_token_id])
    assert not g.accepts(TOK("From <64> to <36>.")[1:] + [TOK.eos_token_id])
    with pytest.raises(SystemExit):
        inference.parse_args(["--synthetic", "--constrain_grounding", "--share_visual", "true"])
    assert "--share_visual" in capsys.readouterr().err
