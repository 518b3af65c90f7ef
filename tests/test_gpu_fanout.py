"""-m gpu: gvl_seq_fanout (Engine.seq_fanout) -- n siblings of a freshly prefilled sequence, n answers from ONE prefill -- and what is built on it
(generate(num_return_sequences=n), generate_shared, ClipScheduler) plus the n best beams (gvl_beam_search_n), on tiny 2-layer models at head dims 64 (Phi MHA),
96 (Phi MHA) and 128 (Llama GQA, 2 KV heads).  The contract is bit identity: sibling i's ids AND log-probabilities are those of an independent sequence prefilled with the
same embeddings under seq_set_sampling(stream = streams[i]) and the same settings, whatever decode path and group it travels in.  The references are computed once per
(model, setting, prompt length) and shared by every n_new and decode path."""
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, bf  # noqa: E402
from grounded_video_llm_amd import engine as E, grammar as GR, lib as L, logits as LP, prompts as P, serve, synth  # noqa: E402
from grounded_video_llm_amd.model import LLAVA_NEXT_VIDEO, SyntheticTokenizer, fanout_stream  # noqa: E402
from test_gpu_extend_varlen import MODELS, make_engine  # noqa: E402

NEW = 8                                   # ids per answer (the first one is the prefill's / the fan-out's)
LENGTHS = (20, 64, 65, 127, 130)          # one partial page, nothing shared | no partial page, no copy | first / last row of a partial page | two shared pages + 2 rows
N_NEW = (1, 2, 15)
SRC_STREAM = 7
STREAMS = [100 + 3 * i for i in range(15)]
SEED = 4242
V = 400


def _grammar():
    """a non-decreasing run of the ids 300 .. 399 (SET and GE on one edge) between other tokens: constrains from the second id of a run on"""
    b = GR.GrammarBuilder(V)
    last = b.token_class(range(V - 100, V), ordinal=True)
    s0, s1 = b.state(), b.state()
    b.edge(s0, 0, s0); b.edge(s0, last, s1, set_reg=True); b.edge(s1, last, s1, set_reg=True, ge_reg=True); b.edge(s1, 0, s0)
    return b.build(s0)


SAMPLED = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=SEED)
# name -> (sampling of every member without its stream, processors, rule-set kwargs, grammar?, top_n)
SETTINGS = {
    "greedy": (dict(do_sample=False), None, None, False, 0),
    "sampled": (SAMPLED, None, None, False, 0),
    "penalty": (SAMPLED, dict(repetition_penalty=1.3), None, False, 0),
    # the non-idempotent case: a second application of the biases to the first row would change the siblings' first draws and log-probabilities
    # (30 biased ids of 400, so that the 20 kept ones hold some of them whatever the row is)
    "sequence_bias": (SAMPLED, None, dict(sequence_bias={**{(t,): 3.0 + 0.05 * t for t in range(0, 60, 2)}, (123,): -2.0, (399,): 4.0, (5, 9): 6.0}), False, 0),
    "grammar": (SAMPLED, None, None, True, 0),
    "top_logprobs": (SAMPLED, None, None, False, 3),
}


@pytest.fixture(scope="module", params=list(MODELS))
def ctx(request):
    eng, geo = make_engine(request.param)
    g = torch.Generator(device=DEV); g.manual_seed(23)
    c = SimpleNamespace(eng=eng, geo=geo, name=request.param, refs={}, free0=eng.kv_info()["free_pages"], rules={}, gid=eng.grammar_create(_grammar()))
    c.pool = (torch.randn((1024, geo.hidden), device=DEV, generator=g) * 0.5).to(bf)
    yield c
    for rid in c.rules.values():
        eng.rules_destroy(rid)
    eng.grammar_destroy(c.gid)
    assert eng.kv_info()["free_pages"] == c.free0, "pages leaked or double-freed"
    eng.close()


def emb(c, S):
    return c.pool[S:2 * S]


def apply(c, seq, setting, stream):
    """the settings of one member; stream None: no sampling setting of its own (it follows the engine's)"""
    smp, procs, rules, gram, top_n = SETTINGS[setting]
    if procs:
        c.eng.seq_set_processors(seq, **procs)
    if rules:
        if setting not in c.rules:
            c.rules[setting] = c.eng.rules_create(LP.resolve_rules(rules, None, NEW, V))
        c.eng.seq_set_token_rules(seq, c.rules[setting])
    if gram:
        c.eng.seq_set_grammar(seq, c.gid)
    c.eng.seq_set_logprobs(seq, top_n)
    if stream is not None:
        c.eng.seq_set_sampling(seq, dict(smp, stream=stream))


def read(c, seq, setting):
    ids = c.eng.seq_read(seq, 0, NEW)
    lp, top = c.eng.seq_read_logprobs(seq, 0, NEW, top=SETTINGS[setting][4] > 0)
    assert len(ids) == NEW and len(lp) == NEW and all(math.isfinite(x) for x in lp)
    return ids, lp, top


def reference(c, setting, S, stream):
    """an independent sequence: its own prefill of the same embeddings under seq_set_sampling(stream), decoded alone"""
    key = (setting, S, stream)
    if key not in c.refs:
        s = c.eng.seq_alloc(S + NEW + 1)
        apply(c, s, setting, stream)
        c.eng.prefill(s, emb(c, S))
        c.eng.decode_greedy(s, NEW, None)
        c.refs[key] = read(c, s, setting)
        c.eng.seq_free(s)
    return c.refs[key]


def fan(c, setting, S, n_new, src_stream=SRC_STREAM):
    src = c.eng.seq_alloc(S + NEW + 1)
    apply(c, src, setting, src_stream)
    first = c.eng.prefill(src, emb(c, S), want_logits=True)
    return src, c.eng.seq_fanout(src, n_new, S + NEW + 1, STREAMS[:n_new], first)


def decode(c, seqs, path):
    if path == "batch":
        c.eng.decode_greedy_batch(seqs, NEW, None)
    elif path in ("steps1", "eager"):
        for _ in range(NEW - 1):
            c.eng.decode_steps(seqs, 1)
    else:
        c.eng.decode_steps(seqs, 5); c.eng.decode_steps(seqs, NEW - 1 - 5)


PATHS = ("batch", "steps1", "steps5", "eager")


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_siblings_equal_independent_sequences_bit_for_bit(ctx, setting):
    c = ctx
    free0 = c.eng.kv_info()["free_pages"]
    runs = 0
    for S in LENGTHS:
        want_src = reference(c, setting, S, SRC_STREAM)
        want = [reference(c, setting, S, st) for st in STREAMS]
        if setting == "greedy":
            assert all(w == want_src for w in want)                   # every sibling equals the source
        for k, n_new in enumerate(N_NEW):
            for path in (PATHS if n_new == 15 or S in (65, 127) else PATHS[k::3] + PATHS[k + 1:k + 2]):
                c.eng.debug_set("decode_graph", 0 if path == "eager" else 1)
                try:
                    src, sibs = fan(c, setting, S, n_new)
                    decode(c, [src] + sibs, path)
                    got_src, got = read(c, src, setting), [read(c, s, setting) for s in sibs]
                finally:
                    c.eng.debug_set("decode_graph", 1)
                for s in [src] + sibs:
                    c.eng.seq_free(s)
                assert got_src == want_src, (c.name, setting, S, n_new, path, "the source changed")
                for i in range(n_new):
                    assert got[i] == want[i], (c.name, setting, S, n_new, path, i, got[i], want[i])
                runs += 1
    assert runs >= 5 * 6 and c.eng.kv_info()["free_pages"] == free0


def test_siblings_of_a_source_that_follows_the_engine_setting(ctx):
    """the effective setting of a source without one of its own is the engine's at the time of the call: the siblings take it as their own, on their streams"""
    c, S = ctx, 65
    c.eng.set_sampling(True, 0.8, 20, 0.9, SEED)
    try:
        src = c.eng.seq_alloc(S + NEW + 1)
        c.eng.seq_set_logprobs(src, 0)
        first = c.eng.prefill(src, emb(c, S), want_logits=True)
        sibs = c.eng.seq_fanout(src, 3, S + NEW + 1, STREAMS[:3], first)
    finally:
        c.eng.set_sampling(False)                                    # the siblings keep what they took: the engine is greedy again from here on
    c.eng.decode_greedy_batch(sibs, NEW, None)
    got = [read(c, s, "sampled") for s in sibs]
    for s in [src] + sibs:
        c.eng.seq_free(s)
    assert got == [reference(c, "sampled", S, st) for st in STREAMS[:3]]


@pytest.mark.parametrize("S", [65, 127])
def test_sibling_kv_equals_a_clone_of_the_source(ctx, S):
    c = ctx
    src, (sib,) = fan(c, "sampled", S, 1)
    cl = c.eng.seq_clone(src, S + NEW + 1)
    a = c.eng.decode_step_logits(sib, 5).clone()
    b = c.eng.decode_step_logits(cl, 5).clone()
    for s in (src, sib, cl):
        c.eng.seq_free(s)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_not_a_trivial_pass(ctx):
    c, S = ctx, 65
    hot = dict(do_sample=True, temperature=1.5, top_k=0, seed=SEED)
    SETTINGS["hot"] = (hot, None, None, False, 0)
    try:
        want = [reference(c, "hot", S, st) for st in STREAMS]
        assert len({tuple(w[0]) for w in want}) >= 2, "the independent answers of this seed are all the same: the case shows nothing"
        src, sibs = fan(c, "hot", S, 15)
        decode(c, [src] + sibs, "batch")
        got = [read(c, s, "hot") for s in sibs]
        for s in [src] + sibs:
            c.eng.seq_free(s)
        assert got == want and len({tuple(g[0]) for g in got}) >= 2
    finally:
        del SETTINGS["hot"]


@pytest.mark.parametrize("order", ["source_first", "siblings_first"])
def test_page_accounting_and_lifetime(ctx, order):
    c = ctx
    for S in LENGTHS:
        free0 = c.eng.kv_info()["free_pages"]
        cap = S + NEW + 1
        src = c.eng.seq_alloc(cap)
        apply(c, src, "sampled", SRC_STREAM)
        first = c.eng.prefill(src, emb(c, S), want_logits=True)
        before = c.eng.kv_info()["free_pages"]
        sibs = c.eng.seq_fanout(src, 3, cap, STREAMS[:3], first)
        private = (cap + 63) // 64 - S // 64
        assert c.eng.kv_info()["free_pages"] == before - 3 * private
        if order == "source_first":                                  # the siblings decode correctly on pages the source no longer holds
            torch.cuda.synchronize()
            c.eng.seq_free(src)
            filler = c.eng.seq_alloc(cap)                             # the pages the source gave back are handed out again, and written
            c.eng.prefill(filler, c.pool[:S])
            decode(c, sibs, "batch")
            got = [read(c, s, "sampled") for s in sibs]
            c.eng.seq_free(filler)
            for s in sibs:
                c.eng.seq_free(s)
        else:
            decode(c, [src] + sibs, "batch")
            got = [read(c, s, "sampled") for s in sibs]
            for s in sibs + [src]:
                c.eng.seq_free(s)
        assert got == [reference(c, "sampled", S, st) for st in STREAMS[:3]], (c.name, S, order)
        assert c.eng.kv_info()["free_pages"] == free0


def snapshot(c, live):
    return c.eng.kv_info(), [(s, c.eng.seq_read(s, 0, 64), c.eng.seq_read_logprobs(s, 0, 64)) for s in live]


def test_refusals_change_nothing(ctx):
    c, S = ctx, 65
    eng = c.eng
    cap = S + NEW + 1
    src = eng.seq_alloc(cap)
    apply(c, src, "sampled", SRC_STREAM)
    first = eng.prefill(src, emb(c, S), want_logits=True)
    sibs = eng.seq_fanout(src, 2, cap, STREAMS[:2], first)
    stale = eng.seq_alloc(cap); apply(c, stale, "sampled", 1); eng.prefill(stale, emb(c, S)); eng.decode_steps([stale], 1)      # not fresh: it has decoded a step
    lead, fol = eng.seq_alloc(cap), eng.seq_alloc(cap)
    for s in (lead, fol):
        eng.seq_set_logprobs(s, 0)
    lc, lu = eng.prefill(lead, emb(c, S), want_logits=True), eng.prefill(fol, emb(c, 20), want_logits=True)
    eng.seq_set_guidance(lead, fol, 1.5, lc, lu)
    total = eng.kv_info()["total_pages"]
    live = [src] + sibs + [stale, lead, fol]
    torch.cuda.synchronize()
    snap = snapshot(c, live)
    cases = [
        ("unknown source", lambda: eng.seq_fanout(999, 1, cap, [1], first), L.ERR_ARG),
        ("a free slot as source", lambda: eng.seq_fanout(250, 1, cap, [1], first), L.ERR_ARG),
        ("not fresh", lambda: eng.seq_fanout(stale, 1, cap, [1], first), L.ERR_STATE),
        ("n_new 0", lambda: eng.seq_fanout(src, 0, cap, [], first), L.ERR_ARG),
        ("n_new 16", lambda: eng.seq_fanout(src, 16, cap, list(range(16)), first), L.ERR_ARG),
        ("max_tokens == pos", lambda: eng.seq_fanout(src, 1, S, [1], first), L.ERR_ARG),
        ("max_tokens > max_seq", lambda: eng.seq_fanout(src, 1, c.geo.max_seq + 1, [1], first), L.ERR_ARG),
        ("leader of a pair", lambda: eng.seq_fanout(lead, 1, cap, [1], first), L.ERR_STATE),
        ("follower of a pair", lambda: eng.seq_fanout(fol, 1, cap, [1], first), L.ERR_STATE),
        ("pages", lambda: eng.seq_fanout(src, 15, 64 * (total // 15 + 2), list(range(15)), first), L.ERR_OOM),   # 15 x (pages - the shared one) > the whole pool
    ]
    for what, call, status in cases:
        with pytest.raises(L.GvlError) as e:
            call()
        assert e.value.status == status, (what, e.value.status, str(e.value))
        assert "gvl_seq_fanout" in str(e.value)
        assert snapshot(c, live) == snap, what
    out, st1, ptr = (L.C.c_int * 2)(), (L.C.c_uint32 * 2)(1, 2), L.C.c_void_p(first.data_ptr())
    for what, args in (("NULL streams", (src, 1, cap, None, ptr, out)), ("NULL logits", (src, 1, cap, st1, None, out)), ("NULL ids", (src, 1, cap, st1, ptr, None))):
        assert eng.lib.gvl_seq_fanout(eng.ctx, *args, eng.stream) == L.ERR_ARG, what
        assert b"gvl_seq_fanout" in eng.lib.gvl_last_error(eng.ctx) and snapshot(c, live) == snap, what
    more = eng.seq_fanout(src, 1, cap, STREAMS[2:3], first)                            # the source is still fresh: the call may be repeated
    decode(c, [src] + sibs + more, "batch")                                           # ... and everything decodes to the references
    assert [read(c, s, "sampled") for s in sibs + more] == [reference(c, "sampled", S, st) for st in STREAMS[:3]]
    assert read(c, src, "sampled") == reference(c, "sampled", S, SRC_STREAM)
    for s in [lead, fol, src, stale] + sibs + more:                                   # the leader first: freeing it unbinds the pair
        eng.seq_free(s)


def test_slot_exhaustion_is_all_or_nothing():
    eng, geo = make_engine("phi_d64", kv_pages=300)
    try:
        x = (torch.randn((20, geo.hidden), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)) * 0.5).to(bf)
        src = eng.seq_alloc(40)
        first = eng.prefill(src, x, want_logits=True)
        fillers = [eng.seq_alloc(8) for _ in range(256 - 1 - 2)]                     # two slots are left
        torch.cuda.synchronize()
        before = (eng.kv_info(), eng.seq_read(src, 0, 4))
        with pytest.raises(L.GvlError) as e:
            eng.seq_fanout(src, 3, 40, [1, 2, 3], first)
        assert e.value.status == L.ERR_OOM and (eng.kv_info(), eng.seq_read(src, 0, 4)) == before
        sibs = eng.seq_fanout(src, 2, 40, [1, 2], first)
        assert len(set(sibs) | {src} | set(fillers)) == 256
        eng.decode_greedy_batch([src] + sibs, 4, None)
        for s in fillers + sibs + [src]:
            eng.seq_free(s)
        assert eng.kv_info()["free_pages"] == 300
    finally:
        eng.close()


# ---- generate(num_return_sequences=n), generate_shared, the scheduler and the n best beams on a tiny model with both towers -------------------------------------
@pytest.fixture(scope="module")
def tiny():
    llm, hid, vocab = "phi3.5", 128, 640
    short, long = synth.longrope_factors(32)
    geo = E.TowerGeometry(llm=llm, clip_hidden=64, clip_inter=128, clip_layers=3, clip_heads=4, iv2_dim=64, iv2_inter=128, iv2_depth=3, iv2_heads=4, hidden=hid, inter=256,
                          layers=2, heads=4, kv_heads=4, vocab=vocab, rope_short=short, rope_long=long, rope_theta=10000.0, max_seq=2048, max_segs=6, kv_pages=96, max_prefill=1024)
    sd = {"vision_tower": synth.clip_weights(64, 128, 3, seed="fan.clip"), "video_encoder": synth.iv2_weights(64, 128, 3, 2, seed="fan.iv2"),
          "projectors": synth.projector_weights(llm, hid, 64, 64, seed="fan.proj"), "language_model": synth.llm_weights("phi3", hid, 256, 2, 4, 4, vocab, True, seed="fan.llm")}
    tok = SyntheticTokenizer(vocab, 300)
    model = LLAVA_NEXT_VIDEO(stage="sft", max_txt_len=64, num_frames=4, num_segs=2, num_temporal_tokens=300, lora=False, llm=llm, geometry=geo, tokenizer=tok, state_dicts=sd,
                             device=DEV)
    prompts = [P.build_prompt(llm, "grounding", "When does the person open the door in the video?"), P.build_prompt(llm, "qa", "Describe the video in detail please.")]
    sp, tp = synth.det_tensor("fan.sp", (2, 2, 3, 336, 336)).to(DEV), synth.det_tensor("fan.tp", (2, 4, 3, 224, 224)).to(DEV)
    samples = {"prompts": prompts, "spatial_pixel_values": sp, "temporal_pixel_values": tp, "video_ids": ["a", "b"]}
    yield SimpleNamespace(model=model, samples=samples, prompts=prompts, sp=sp, tp=tp)
    info = model.engine.kv_info()
    assert info["free_pages"] == info["total_pages"], "KV pages leaked"
    model.engine.close()


HOT = dict(do_sample=True, num_beams=1, max_new_tokens=8, temperature=1.5, top_k=0)


def test_generate_returns_n_answers_per_prompt(tiny):
    m, samples = tiny.model, tiny.samples
    t3 = m.generate(samples, seed=9, num_return_sequences=3, **HOT)
    assert isinstance(t3, list) and len(t3) == 6 and all(isinstance(t, str) for t in t3)           # prompt-major: the three answers of prompt 0, then prompt 1's
    assert t3 == m.generate(samples, seed=9, num_return_sequences=3, **HOT)                         # reproducible under a seed
    t2 = m.generate(samples, seed=9, num_return_sequences=2, **HOT)
    assert t2 == t3[0:2] + t3[3:5]                                                                  # the answers for n' < n are a prefix, per prompt
    assert len(set(m.generate(samples, seed=9, num_return_sequences=16, **HOT)[:16])) > 1           # 16 answers: a fan-out in two parts; they are not all the same
    one = {"prompts": samples["prompts"][1:], "spatial_pixel_values": tiny.sp[1:], "temporal_pixel_values": tiny.tp[1:], "video_ids": ["b"]}
    o = m.generate(one, seed=9, num_return_sequences=3, return_dict_in_generate=True, output_scores=True, **HOT)
    assert len(o.sequences) == 3 and len(o.transition_scores) == 3
    # answer j of a prompt is what a sequence of its own on stream fanout_stream(prompt index, j) gives
    eng = m.engine
    feats = m.encode_images(one)
    ids_arr, mask = P.left_pad_truncate([m.tokenizer_image_token(one["prompts"][0])], 0, m.max_txt_len)
    e = eng.splice([int(t) for t, k in zip(ids_arr[0], mask[0]) if k], feats[0])
    for j in range(3):
        s = eng.seq_alloc(e.shape[0] + 8)
        eng.seq_set_sampling(s, dict(do_sample=True, temperature=1.5, top_k=0, top_p=None, seed=9, stream=fanout_stream(0, j)))
        eng.prefill(s, e)
        ids = eng.decode_greedy(s, 8, m.tokenizer.eos_token_id)
        eng.seq_free(s)
        assert o.sequences[j] == ids, j
    r = m.generate(samples, seed=9, num_return_sequences=3, return_dict_in_generate=True, top_logprobs=2, **HOT)
    assert len(r.sequences) == len(r.texts) == len(r.top_logprobs) == 6 and r.texts == t3
    assert all(len(tl) == len(s) and all(len(x) == 2 for x in tl) for tl, s in zip(r.top_logprobs, r.sequences))
    assert m.generate(samples, seed=9, num_return_sequences=1, **HOT) == m.generate(samples, seed=9, **HOT)     # 1 / None: today's path


def test_generate_with_a_small_pool_falls_back_to_parts(tiny, monkeypatch):
    m, samples = tiny.model, tiny.samples
    one = {"prompts": samples["prompts"][:1], "spatial_pixel_values": tiny.sp[:1], "temporal_pixel_values": tiny.tp[:1], "video_ids": ["a"]}
    want = m.generate(one, seed=3, num_return_sequences=6, **HOT)
    eng = m.engine
    ids_arr, mask = P.left_pad_truncate([m.tokenizer_image_token(one["prompts"][0])], 0, m.max_txt_len)
    S = eng.splice([int(t) for t, k in zip(ids_arr[0], mask[0]) if k], m.encode_images(one)[0]).shape[0]
    room = (S + 8 + 63) // 64 + 2                                             # one answer's pages and two more: at most two siblings fit beside their source
    hog = []
    while eng.kv_info()["free_pages"] > room:
        hog.append(eng.seq_alloc(64 * min(8, eng.kv_info()["free_pages"] - room)))
    prefills = []
    real = eng.prefill
    monkeypatch.setattr(eng, "prefill", lambda *a, **k: (prefills.append(1), real(*a, **k))[1])
    try:
        assert m.generate(one, seed=3, num_return_sequences=6, **HOT) == want
        assert 2 <= len(prefills) <= 6                                         # parts: more than one prefill, and the same six answers
    finally:
        for s in hog:
            eng.seq_free(s)


def test_n_best_beams(tiny):
    m, samples = tiny.model, tiny.samples
    kw = dict(do_sample=False, num_beams=3, max_new_tokens=8, return_dict_in_generate=True, output_scores=True)
    host = m.generate(samples, num_return_sequences=3, beam_impl="host", **kw)
    dev = m.generate(samples, num_return_sequences=3, beam_impl="device", **kw)
    assert len(host.sequences) == 6 and host.sequences == dev.sequences and host.texts == dev.texts
    for o in (host, dev):
        assert len(o.sequences_scores) == 6
        for p in (0, 3):
            assert o.sequences_scores[p] >= o.sequences_scores[p + 1] >= o.sequences_scores[p + 2]
            assert len({tuple(s) for s in o.sequences[p:p + 3]}) == 3
    assert all(abs(a - b) < 1e-4 for a, b in zip(host.sequences_scores, dev.sequences_scores))
    for impl, o in (("host", host), ("device", dev)):
        best = m.generate(samples, beam_impl=impl, **kw)
        assert best.sequences == [o.sequences[0], o.sequences[3]] and best.sequences_scores == [o.sequences_scores[0], o.sequences_scores[3]]
    two = m.generate(samples, num_return_sequences=2, **kw)
    assert two.sequences == host.sequences[0:2] + host.sequences[3:5]
    bs = m.generate(samples, do_sample=True, num_beams=3, num_return_sequences=2, seed=4, max_new_tokens=6)    # beam-sample: the two best of a seeded search
    assert len(bs) == 4 and bs == m.generate(samples, do_sample=True, num_beams=3, num_return_sequences=2, seed=4, max_new_tokens=6)


def test_generate_shared_returns_n_per_prompt(tiny):
    m = tiny.model
    one = {"spatial_pixel_values": tiny.sp[:1], "temporal_pixel_values": tiny.tp[:1], "video_ids": ["a"]}
    shared = m.generate_shared(one, tiny.prompts, seed=5, num_return_sequences=3, **HOT)
    assert m.last_shared_prefix >= 128                                         # the prompts were prefilled behind one shared prefix, then fanned out
    per_prompt = [m.generate({**one, "prompts": [p]}, seed=5, num_return_sequences=3, **HOT) for p in tiny.prompts]
    assert len(shared) == 6 and shared == per_prompt[0] + per_prompt[1]
    assert m.generate_shared(one, tiny.prompts[:1], seed=5, num_return_sequences=3, **HOT) == per_prompt[0]      # one prompt: nothing to share, the same answers


def test_scheduler_members_do_not_depend_on_the_schedule(tiny):
    m = tiny.model
    eng = m.engine
    feats = m.encode_images(tiny.samples)
    rows = [m.tokenizer_image_token(p) for p in tiny.prompts]
    embs = [eng.splice(r, feats[i]) for i, r in enumerate(rows)]
    eng.set_sampling(False)                                                       # requests without a setting of their own follow the engine's: greedy
    seen = []
    for max_active in (3, 8):
        for chunk in (1, 8):
            sch = serve.ClipScheduler(eng, m.tokenizer.eos_token_id, max_active=max_active, chunk=chunk)
            other = sch.submit(embs[1], 10)
            rids = sch.submit(embs[0], 10, num_return_sequences=3, temperature=0.7, seed=5)
            late = sch.submit(embs[1], 10, do_sample=False)
            out = sch.run()
            assert len(rids) == 3 and out[other] == out[late]
            seen.append([out[r] for r in rids])
    assert all(s == seen[0] for s in seen[1:]), seen
    assert embs[0].shape[0] > 128 and embs[0].shape[0] % 128                      # behind a resident prefix (add_prefix): only the rows behind it are prefilled, same answers
    sch = serve.ClipScheduler(eng, m.tokenizer.eos_token_id, max_active=4, chunk=4)
    pid = sch.add_prefix(embs[0])
    rids = sch.submit(embs[0], 10, num_return_sequences=3, temperature=0.7, seed=5, prefix=pid)
    out = sch.run()
    sch.drop_prefix(pid)
    assert [out[r] for r in rids] == seen[0] and sch.stats["prefix_rows_saved"] == embs[0].shape[0] // 128 * 128
    for j in range(3):                                                            # answer j is the request's own sampling on stream j
        s = eng.seq_alloc(embs[0].shape[0] + 10)
        eng.seq_set_sampling(s, dict(do_sample=True, temperature=0.7, top_k=50, top_p=None, seed=5, stream=j))
        eng.prefill(s, embs[0])
        ids = eng.decode_greedy(s, 10, m.tokenizer.eos_token_id)
        eng.seq_free(s)
        assert seen[0][j] == ids, j
