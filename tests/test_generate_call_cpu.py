"""generate()'s host side without a GPU:
  1. call.resolve_call maps the kwargs to ONE mode and the fields of that mode (a hand-written table);
  2. every refusal that depends on the kwargs alone comes from resolve_call, and through generate() / generate_shared() before any engine call;
  3. the engine sees, call by call, what it saw before generate() was built on the resolved call: tests/golden/generate_call_traces.json holds the call lists of the
     recording stub engine (test_contrastive_host_cpu) for every scenario of `scenarios()`, written by `python tests/test_generate_call_cpu.py --record` from the code as it
     was before that change.  Tensors are recorded as shape and dtype, everything else by value."""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the package on sys.path)
from grounded_video_llm_amd import grammar as GR, lib as L, logits as LP
from test_contrastive_host_cpu import _stub_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_call_traces.json")
V, EOS, PAD = 640, 2, 0


def _grammar(vocab=V):
    b = GR.GrammarBuilder(vocab)
    word, eos = b.token_class([11, 12, 13]), b.token_class([EOS])
    s0, s1 = b.state(), b.state()
    b.edge(s0, word, s0)
    b.edge(s0, eos, s1)
    return b.build(s0)


GRAMMAR = _grammar()
RULES = dict(sequence_bias={(11,): 2.0, (12, 13): -1.5}, bad_words_ids=[[14], [15, 16]], suppress_tokens=[17], begin_suppress_tokens=[18], forced_eos_token_id=EOS)
NEG = lambda n: dict(guidance_scale=2.0, negative_prompt_ids=[[4, 5 + i] for i in range(n)])

# name, kwargs (or n samples -> kwargs), mode, the fields of the Call that the row is about
TABLE = [
    ("greedy", {}, "greedy", dict(sampling_args=(False,), n_return=1, num_beams=1, max_new=2048)),
    ("greedy_args_ignored", dict(do_sample=False, num_beams=1, temperature=0.2, top_p=None, top_k=4, max_new_tokens=5), "greedy", dict(sampling_args=(False,), max_new=5)),
    ("sample", dict(do_sample=True, seed=1), "sample", dict(sampling_args=(True, 1.0, 50, None, 1), warpers={})),
    ("sample_cli", dict(do_sample=True, temperature=0.2, top_p=None, seed=7), "sample", dict(sampling_args=(True, 0.2, 50, None, 7))),
    ("sample_top_k_none", dict(do_sample=True, temperature=0.7, top_k=None, top_p=0.9, seed=3), "sample", dict(sampling_args=(True, 0.7, 0, 0.9, 3))),
    ("sample_warpers", dict(do_sample=True, seed=2, min_p=0.1, typical_p=0.9, epsilon_cutoff=0.0), "sample", dict(warpers=dict(min_p=0.1, typical_p=0.9))),
    ("beam", dict(num_beams=4, max_new_tokens=4), "beam", dict(num_beams=4, beam_impl="host", sampling_args=(False,), length_penalty=1.0, early_stopping=False)),
    ("beam_sample", dict(num_beams=4, do_sample=True, seed=5, top_k=None, max_new_tokens=4), "beam-sample",
     dict(sampling_args=(False,), beam_sample=dict(temperature=1.0, top_k=None, top_p=None, seed=5, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None))),
    ("group_beam", dict(num_beams=6, num_beam_groups=3, diversity_penalty=0.5, max_new_tokens=4), "group-beam", dict(groups=(3, 0.5), num_beams=6)),
    ("contrastive", dict(penalty_alpha=0.6, top_k=4, max_new_tokens=4), "contrastive", dict(contrastive=(4, 0.6))),
    ("not_contrastive_sampled", dict(penalty_alpha=0.6, top_k=4, do_sample=True, seed=1), "sample", dict(contrastive=None, sampling_args=(True, 1.0, 4, None, 1))),
    ("not_contrastive_top_k_1", dict(penalty_alpha=0.6, top_k=1), "greedy", dict(contrastive=None)),
    ("not_contrastive_alpha_0", dict(penalty_alpha=0, top_k=4), "greedy", dict(contrastive=None)),
    ("guidance_off_beam", dict(guidance_scale=1, num_beams=4, max_new_tokens=4), "beam", dict(guidance=None)),
    ("guided", NEG, "guided", dict(guidance=2.0, negative_texts=None)),
    ("guided_sampled", lambda n: dict(NEG(n), do_sample=True, seed=9), "guided", dict(sampling_args=(True, 1.0, 50, None, 9))),
    ("fanout", dict(do_sample=True, num_return_sequences=3, seed=4), "fan-out",
     dict(n_return=3, sampling_args=(True, 1.0, 50, None, 4), seq_sampling=dict(do_sample=True, temperature=1.0, top_k=50, top_p=None, seed=4))),
    ("beam_n_best", dict(num_beams=3, num_return_sequences=2, max_new_tokens=4), "beam", dict(n_return=2, num_beams=3)),
    ("beam_device", dict(num_beams=4, beam_impl="device", length_penalty=0.5, early_stopping=True), "beam", dict(beam_impl="device", length_penalty=0.5, early_stopping=True)),
    ("group_beam_device", dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.0, beam_impl="device"), "group-beam", dict(groups=(2, 1.0), beam_impl="device")),
    ("greedy_rules_grammar", dict(RULES, grammar=GRAMMAR, repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=2, max_new_tokens=6), "greedy",
     dict(grammar=GRAMMAR, rules=LP.resolve_rules(RULES, EOS, 6, V))),
    ("beam_rules_grammar", dict(RULES, grammar=GRAMMAR, repetition_penalty=1.3, num_beams=2, max_new_tokens=3), "beam", dict(grammar=GRAMMAR)),
    ("contrastive_rules", dict(RULES, penalty_alpha=0.6, top_k=4, min_length=30, max_new_tokens=4), "contrastive", {}),
    ("greedy_scores", dict(return_dict_in_generate=True, output_scores=True), "greedy", dict(want_logprobs=0)),
    ("sample_top_logprobs", dict(do_sample=True, seed=1, return_dict_in_generate=True, top_logprobs=3), "sample", dict(want_logprobs=3)),
    ("fanout_scores", dict(do_sample=True, seed=1, num_return_sequences=2, return_dict_in_generate=True, output_scores=True), "fan-out", dict(want_logprobs=0)),
    ("beam_scores", dict(num_beams=2, return_dict_in_generate=True, output_scores=True, max_new_tokens=3), "beam", dict(want_logprobs=0)),
]
SEARCH_MODES = {"beam", "beam-sample", "group-beam", "contrastive"}


def _kw(kw, n):
    return kw(n) if callable(kw) else dict(kw)


def _resolve(kw, entry="generate", n=2, vocab=V, draw_seed=None):
    from grounded_video_llm_amd.call import resolve_call

    def no_draw():
        raise AssertionError("a seeded or greedy call draws no seed")
    return resolve_call(kw, entry=entry, n_samples=n, eos_id=EOS, pad_id=PAD, vocab=vocab, draw_seed=draw_seed or no_draw)


# ---- 1. modes ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,mode,fields", TABLE, ids=[r[0] for r in TABLE])
def test_mode_table(name, kw, mode, fields):
    c = _resolve(_kw(kw, 2))
    assert c.mode.value == mode
    assert c.device_selects == (mode not in SEARCH_MODES)
    for k, want in fields.items():
        assert getattr(c, k) == want, (k, getattr(c, k), want)
    if name.startswith("guided"):
        assert c.negative_ids == [[4, 5], [4, 6]]
    assert c.eos_id == EOS and c.pad_id == PAD


def test_device_selects_is_false_exactly_for_the_four_searches():
    from grounded_video_llm_amd.call import Mode
    assert {m.value for m in Mode} == {"greedy", "sample", "beam", "beam-sample", "group-beam", "contrastive", "guided", "fan-out"}
    seen = {}
    for _, kw, mode, _ in TABLE:
        seen[mode] = _resolve(_kw(kw, 2)).device_selects
    assert seen == {m.value: m.value not in SEARCH_MODES for m in Mode}


def test_processors_follow_the_embedding_length():
    c = _resolve(dict(min_length=30, repetition_penalty=1.5))
    assert c.processors(10) == LP.Processors(1.5, 0, 20, EOS) and c.processors(40) == LP.Processors(1.5, 0, 0, EOS)
    assert _resolve(dict(min_length=30, min_new_tokens=3)).processors(10).min_new == 3
    assert _resolve({}).processors(10) == LP.Processors(1.0, 0, 0, EOS) and not _resolve({}).processors(10).active


def test_unseeded_calls_draw_once_and_fan_out_twice():
    draws = iter(range(100, 200))
    one = _resolve(dict(do_sample=True), draw_seed=lambda: next(draws))
    assert one.sampling_args[4] == 100 and one.seq_sampling is None
    fan = _resolve(dict(do_sample=True, num_return_sequences=2), draw_seed=lambda: next(draws))
    assert fan.sampling_args[4] == 101 and fan.seq_sampling["seed"] == 102              # the engine's default takes the first draw, the sequences the second
    bs = _resolve(dict(do_sample=True, num_beams=2), draw_seed=lambda: next(draws))
    assert bs.beam_sample["seed"] == 103 and next(draws) == 104


SHARED_REFUSED = [(lambda n: dict(guidance_scale=2.0, negative_prompts=["n"] * n), "generate_shared.*guidance_scale != 1 is not supported"),
                  (dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.0), "generate_shared.*num_beam_groups"),
                  (dict(penalty_alpha=0.6, top_k=4), "generate_shared.*contrastive")]


def test_generate_shared_modes():
    for kw, mode in ((dict(), "greedy"), (dict(do_sample=True, seed=1), "sample"), (dict(do_sample=True, seed=1, num_return_sequences=3), "fan-out"),
                     (dict(num_beams=4), "greedy"), (dict(num_beams=4, do_sample=True), "greedy")):      # num_beams alone was never honoured there: greedy
        c = _resolve(kw, entry="generate_shared", n=1)
        assert c.mode.value == mode and c.device_selects
    with pytest.raises(ValueError, match="entry"):
        _resolve({}, entry="score")


# ---- 2. refusals before any work ---------------------------------------------------------------------------------------------------------------------------
class _NoEngine:
    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} reached")


REFUSED = [  # kwargs (or n samples -> kwargs), the message
    # test_num_return_cpu
    (dict(num_return_sequences=2), "Greedy methods without beam search do not support `num_return_sequences` different than 1"),
    (dict(do_sample=False, num_beams=1, num_return_sequences=3), "Greedy methods without beam search do not support `num_return_sequences` different than 1"),
    (dict(num_beams=3, num_return_sequences=4), r"`num_return_sequences` \(4\) has to be smaller or equal to `num_beams` \(3\)"),
    (dict(num_beams=3, do_sample=True, num_return_sequences=4), r"`num_return_sequences` \(4\) has to be smaller or equal to `num_beams` \(3\)"),
    (dict(do_sample=True, num_return_sequences=0), "`num_return_sequences` has to be a strictly positive integer"),
    (dict(do_sample=True, num_return_sequences=-2), "`num_return_sequences` has to be a strictly positive integer"),
    (lambda n: dict(do_sample=True, num_return_sequences=2, guidance_scale=2.0, negative_prompts=["n"] * n), "guidance_scale with num_return_sequences > 1 is not supported"),
    # test_guidance_ref_cpu
    (dict(guidance_scale=2.0), "needs the negative prompt"),
    (lambda n: dict(guidance_scale=2.0, negative_prompts=["n"] * n, negative_prompt_ids=[[1]] * n), "exactly one"),
    (lambda n: dict(guidance_scale=2.0, negative_prompts=["n"] * (n + 1)), "samples need . negative prompts"),
    (dict(guidance_scale=2.0, negative_prompts="n"), "list of strings"),
    (lambda n: dict(guidance_scale=2.0, negative_prompt_ids=[[1]] * (n - 1) + [[640]]), "outside the vocabulary"),
    (lambda n: dict(guidance_scale=2.0, negative_prompts=["n"] * n, num_beams=2), "num_beams > 1 is not supported"),
    (lambda n: dict(guidance_scale=float("nan"), negative_prompts=["n"] * n), "guidance_scale"),
    # test_group_beam_host_cpu
    (dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.0, do_sample=True), "`do_sample` must be set to `False`"),
    (dict(num_beams=4, diversity_penalty=1.0, do_sample=True), "`do_sample` must be set to `False`"),
    (dict(num_beams=4, num_beam_groups=3, diversity_penalty=1.0), "divisible by `num_beam_groups`"),
    (dict(num_beams=2, num_beam_groups=4, diversity_penalty=1.0), "smaller or equal than `num_beams`"),
    (dict(num_beam_groups=2, diversity_penalty=1.0), "smaller or equal than `num_beams`"),
    (dict(num_beams=4, num_beam_groups=2), "otherwise your groups will be identical"),
    (dict(num_beams=4, num_beam_groups=2, diversity_penalty=0.0), "otherwise your groups will be identical"),
    (dict(num_beams=4, diversity_penalty=1.0), "`num_beam_groups` should be greater than 1"),
    (dict(num_beams=4, num_beam_groups=1, diversity_penalty=0.5), "`num_beam_groups` should be greater than 1"),
    (dict(num_beams=4, num_beam_groups=2, diversity_penalty=-1.0), "float strictly larger than 0"),
    (dict(num_beams=4, num_beam_groups=2, diversity_penalty=1), "float strictly larger than 0"),
    (dict(num_beams=4, num_beam_groups=2, diversity_penalty="1.0"), "float strictly larger than 0"),
    (dict(num_beams=4, num_beam_groups=2, diversity_penalty=float("nan")), "float strictly larger than 0"),
    (dict(num_beams=4, num_beam_groups=0, diversity_penalty=1.0), "strictly positive integer"),
    (dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.0, num_return_sequences=5), r"`num_return_sequences` \(5\) has to be smaller or equal to `num_beams`"),
    (dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.0, constraints=[object()]), "constrained beams"),
    (dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.0, force_words_ids=[[1]]), "constrained beams"),
    (lambda n: dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.0, guidance_scale=2.0, negative_prompts=["n"] * n), "guidance_scale"),
    # test_contrastive_host_cpu
    (lambda n: dict(penalty_alpha=0.6, top_k=4, guidance_scale=2.0, negative_prompts=["n"] * n), "guidance_scale"),
    (dict(penalty_alpha=0.6, top_k=4, num_return_sequences=2), "num_return_sequences"),
    (dict(penalty_alpha=0.6, top_k=4, top_logprobs=2, return_dict_in_generate=True), "top_logprobs"),
    (dict(penalty_alpha=0.6, top_k=17), "at most 16"),
    (dict(penalty_alpha=1.5, top_k=4), "penalty_alpha"),
    (dict(penalty_alpha=-1.0), "penalty_alpha"),
    # test_logits_processors_cpu
    (dict(repetition_penalty=2), "`penalty` has to be a strictly positive float, but is 2"),
    (dict(repetition_penalty=0.0), "strictly positive float"),
    (dict(repetition_penalty=-1.0), "strictly positive float"),
    (dict(no_repeat_ngram_size=2.5), "`ngram_size` has to be a strictly positive integer"),
    (dict(no_repeat_ngram_size=2.0), "`ngram_size` has to be a strictly positive integer"),
    (dict(min_new_tokens=2.5), "`min_length` has to be a non-negative integer, but is 2.5"),
    # test_token_rules_cpu
    (dict(sequence_bias={}), "`sequence_bias` has to be a non-empty dictionary"),
    (dict(sequence_bias={(1, 2): 1.0, 3: 2.0}), "`sequence_bias` has to be a dict with tuples as keys"),
    (dict(sequence_bias={(1, -2): 1.0}), "non-empty tuple of positive integers"),
    (dict(sequence_bias={(1,): 1}), "dict with floats as values"),
    (dict(sequence_bias=[[[1, 2], 1]]), "non-empty list of lists of positive integers and float"),
    (dict(sequence_bias={(3, 700): 1.0}), r"The model vocabulary size is 640, but the following tokens were being biased: \[700\]"),
    (dict(bad_words_ids=[]), "`bad_words_ids` has to be a non-empty list"),
    (dict(bad_words_ids=[3]), "`bad_words_ids` has to be a list of lists"),
    (dict(bad_words_ids=[[-1]]), "has to be a list of positive integers"),
    (dict(bad_words_ids=[[]]), "non-empty"),
    (dict(bad_words_ids=[list(range(1, 18))]), "exceeds the limit of 16 ids per entry"),
    (dict(forced_eos_token_id=-1), "`eos_token_id` has to be a list of positive integers"),
    (dict(forced_eos_token_id=[1.5]), "`eos_token_id` has to be a list of positive integers"),
    (dict(suppress_tokens=[1.5]), "`suppress_tokens` has to be a list of integers"),
    # test_logprobs_cpu
    (dict(return_dict_in_generate=True, top_logprobs=-1), "`top_logprobs` has to be an integer in 0 .. 8"),
    (dict(return_dict_in_generate=True, top_logprobs=99), "`top_logprobs` has to be an integer in 0 .. 8"),
    (dict(top_logprobs=2, num_beams=3), "`top_logprobs` is not supported with num_beams > 1"),
    (dict(return_dict_in_generate=True, output_logits=True), "output_logits=True is not supported"),
    # beam_impl
    (dict(beam_impl="gpu"), "beam_impl must be 'host' or 'device'"),
    (dict(beam_impl="device", num_beams=2, do_sample=True), "beam_impl='device' is beam search"),
    # the ones that used to reach the engine first
    (dict(sequence_bias={(1, 2.5): 1.0}), "non-empty tuple of positive integers"),
    (dict(prefix_allowed_tokens_fn=lambda b, ids: [1]), "prefix_allowed_tokens_fn is a Python callback"),
    (dict(grammar="From <s> to <e>."), "grammar must be a grounded_video_llm_amd.grammar.Grammar, not str"),
    (dict(grammar=_grammar(V + 1)), "the grammar classifies 641 ids, the model's vocabulary holds 640"),
    (dict(do_sample=True, temperature=0.0), "`temperature` has to be a strictly positive float"),
    (dict(do_sample=True, top_p=1.5), "`top_p` has to be a float > 0 and <= 1"),
    (dict(num_beams=2, do_sample=True, temperature=0.0), "`temperature` has to be a strictly positive float"),
    (dict(min_p=2.0), "`min_p` has to be a float in the \\[0, 1\\] interval"),
    (dict(do_sample=True, typical_p=1.5), "`typical_p` has to be a float > 0 and < 1"),
    (dict(top_logprobs=99), "`top_logprobs` has to be an integer in 0 .. 8"),
]
# the same through generate_shared: its own refusals, and what both entries share
SHARED_ONLY = SHARED_REFUSED + [(dict(num_beams=3, num_return_sequences=2), "generate_shared.*num_return_sequences > 1 is built for sampling"),
                                (dict(num_return_sequences=2), "Greedy methods")]
BOTH = [r for r in REFUSED if not callable(r[0]) and not ({"num_beams", "num_beam_groups", "diversity_penalty", "penalty_alpha", "beam_impl", "guidance_scale"} & set(r[0]))]


def _no_engine_model():
    m = _stub_model()
    m.engine = _NoEngine()
    return m


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("kw,match", REFUSED, ids=[f"{i}" for i in range(len(REFUSED))])
def test_generate_refuses_before_any_engine_call(kw, match, n):
    kw = _kw(kw, n)
    with pytest.raises(ValueError, match=match):
        _resolve(kw, n=n)
    samples = {"prompts": ["a"] * n, "video_ids": ["x"] * n, "spatial_pixel_values": torch.zeros((n, 1))}
    with pytest.raises(ValueError, match=match):
        _no_engine_model().generate(samples, **kw)


@pytest.mark.parametrize("kw,match", SHARED_ONLY + BOTH, ids=[f"{i}" for i in range(len(SHARED_ONLY + BOTH))])
def test_generate_shared_refuses_before_any_engine_call(kw, match):
    kw = _kw(kw, 1)
    with pytest.raises(ValueError, match=match):
        _resolve(kw, entry="generate_shared", n=1)
    with pytest.raises(ValueError, match=match):
        _no_engine_model().generate_shared({"spatial_pixel_values": torch.zeros((1, 1))}, ["a", "b"], **kw)


def test_the_first_of_two_errors_stays_the_first():
    for kw, match in ((dict(beam_impl="x", guidance_scale=2.0), "beam_impl"), (dict(guidance_scale=2.0, num_return_sequences=0), "negative prompt"),
                      (dict(num_return_sequences=0, num_beams=4, num_beam_groups=3, diversity_penalty=1.0), "num_return_sequences"),
                      (dict(num_beams=4, num_beam_groups=3, diversity_penalty=1.0, penalty_alpha=2.0), "num_beam_groups"),
                      (dict(penalty_alpha=2.0, top_logprobs=99), "penalty_alpha"), (dict(top_logprobs=99, repetition_penalty=0.0), "top_logprobs"),
                      (dict(repetition_penalty=0.0, min_p=2.0), "penalty"), (dict(min_p=2.0, do_sample=True, temperature=0.0), "min_p"),
                      (dict(do_sample=True, temperature=0.0, bad_words_ids=[]), "temperature"), (dict(bad_words_ids=[], grammar="x"), "bad_words_ids")):
        with pytest.raises(ValueError, match=match):
            _resolve(kw)
    assert len(BOTH) >= 30


# ---- 3. the engine sees the same calls -----------------------------------------------------------------------------------------------------------------------
def _enc(x):
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if x is ...:
        return "..."
    if isinstance(x, torch.Tensor):
        return {"tensor": list(x.shape), "dtype": str(x.dtype)}
    if isinstance(x, np.ndarray):
        return {"ndarray": list(x.shape), "dtype": str(x.dtype)}
    if isinstance(x, (np.integer, np.floating)):
        return x.item()
    if dataclasses.is_dataclass(x):
        return {type(x).__name__: {f.name: _enc(getattr(x, f.name)) for f in dataclasses.fields(x)}}
    if isinstance(x, dict):
        return {str(k): _enc(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_enc(v) for v in x]
    raise TypeError(f"cannot record {type(x).__name__}")


def _model(logits, n_visual=6, pool=None):
    m = _stub_model(logits=logits, n_visual=n_visual, pool=pool)
    m.tokenizer_image_token = lambda text: [1, 20, -200, 21] + [30 + ord(c) % 64 for c in text]      # prompts part ways behind the video
    return m


def _trace(m, result):
    return [[name, _enc(a), _enc(kw)] for name, a, kw in m.engine.calls] + [["<return>", _enc(result), {}]]


def scenarios():
    """name -> a function that runs one call on a fresh stub model and returns its trace"""
    out = {}

    def gen(kw, n, pool=None):
        def run():
            m = _model(logits=True, pool=pool)
            samples = {"prompts": ["what", "when is it", "who", "where"][:n], "video_ids": ["x"] * n, "spatial_pixel_values": torch.zeros((n, 1))}
            try:
                return _trace(m, m.generate(samples, **_kw(kw, n)))
            except L.GvlError as e:                          # a pool too small for one item: the error goes through, everything is given back
                return _trace(m, f"GvlError {e.status}")
        return run
    for name, kw, _, _ in TABLE:
        for n in (1, 3):
            out[f"generate/{name}/{n}"] = gen(kw, n)
    # a KV pool that holds fewer sequences than the call needs: the batch runs in groups, a half-admitted pair is given back
    scores = dict(return_dict_in_generate=True, output_scores=True)
    for pool in (1, 2, 3):
        out[f"pool/greedy/4/{pool}"] = gen(scores, 4, pool)
    for pool in (1, 2, 3, 4, 5):
        out[f"pool/guided/3/{pool}"] = gen(lambda n: dict(NEG(n), **scores), 3, pool)
    out["pool/fanout/2/3"] = gen(dict(do_sample=True, seed=4, num_return_sequences=5), 2, 3)

    def shared(kw, prompts, n_visual):
        def run():
            m = _model(logits=True, n_visual=n_visual)
            got = m.generate_shared({"spatial_pixel_values": torch.zeros((1, 1))}, prompts, **kw)
            return _trace(m, got) + [["<last_shared_prefix>", getattr(m, "last_shared_prefix", None), {}]]
        return run
    shared_kw = dict(greedy={}, sampled=dict(do_sample=True, seed=6, top_p=0.9), fanout=dict(do_sample=True, seed=6, num_return_sequences=3),
                     fanout_17=dict(do_sample=True, seed=6, num_return_sequences=17, return_dict_in_generate=True, output_scores=True),
                     rules_grammar=dict(RULES, grammar=GRAMMAR, min_length=300, repetition_penalty=1.2, max_new_tokens=6, return_dict_in_generate=True, top_logprobs=2))
    for name, kw in shared_kw.items():
        for prompts in (["what"], ["what", "when is it", "who"]):
            for n_visual in (200, 6):                      # 200 visual rows: a shared prefix of 128; 6: nothing worth sharing
                out[f"generate_shared/{name}/{len(prompts)}/{n_visual}"] = shared(kw, prompts, n_visual)

    def score(n_visual, top):
        def run():
            m = _model(logits=True, n_visual=n_visual)
            got = m.score({"spatial_pixel_values": torch.zeros((1, 1))}, ["what", "what"], continuation_ids=[[11, 12], [13]], top_logprobs=top)
            return _trace(m, got)
        return run
    out["score/2/200"], out["score/2/6/top"] = score(200, None), score(6, 2)

    def unseeded(kw):
        def run():
            torch.manual_seed(123)
            m = _model(logits=True)
            samples = {"prompts": ["what", "who"], "video_ids": ["x"] * 2, "spatial_pixel_values": torch.zeros((2, 1))}
            got = m.generate(samples, **kw)
            return _trace(m, got) + [["<next draw>", int(torch.randint(0, 2 ** 62, (1,)).item()), {}]]
        return run
    out["unseeded/sample"], out["unseeded/fanout"] = unseeded(dict(do_sample=True)), unseeded(dict(do_sample=True, num_return_sequences=3))
    out["unseeded/beam_sample"] = unseeded(dict(do_sample=True, num_beams=2, max_new_tokens=3))
    return out


def record():
    return {name: run() for name, run in scenarios().items()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_scenarios_are_the_recorded_ones(golden):
    assert sorted(golden) == sorted(scenarios())
    assert len(golden) == 2 * len(TABLE) + 9 + 20 + 2 + 3


@pytest.mark.parametrize("name", sorted(scenarios()))
def test_engine_sees_the_recorded_calls(golden, name):
    got = json.loads(json.dumps(scenarios()[name]()))
    want = golden[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, i, g, w)
    assert len(got) == len(want), (name, [c[0] for c in got[len(want):]], [c[0] for c in want[len(got):]])


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    with open(GOLDEN, "w") as f:
        json.dump(record(), f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
