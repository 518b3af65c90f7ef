"""-m gpu: decoding grammars on the device (the GRAMMAR stage of csrc/gvl_logits.hip, grammars of gvl_grammar_create): the operator bit for bit against the
torch restatement of the whole ordered pipeline (tests/grammar_ref.py, itself pinned to the installed transformers by tests/test_grammar_ref_cpu.py), generate()
against a KV-cached oracle loop with the same restatement, every way of decoding agreeing with the single-sequence answer, beam search on both implementations,
and the lifetime / error rules of a grammar.

The synthetic tokenizer hashes words to ids and cannot turn them back (it prints w<id>), and it joins tokens with spaces; so the text checks decode the answer's
three literal words by their ids (_text), drop the space in front of the full stop, and then match `From <\\d+> to <\\d+>\\.` with s <= e; the ids are checked
against the grammar itself as well, and generate()'s own text against the tokenizer's decode.
A sequence's mask is a function of ITS OWN generated ids: a clone of a sequence with a grammar takes the source's ids with it (gvl_seq_clone), so a clone taken
mid-answer continues the answer; a fork shares prompt pages only, so a fork taken mid-answer answers exactly as a sequence on its own, and a fork whose prefix
would hold generated ids is refused.  inference.py --constrain_grounding runs once on synthetic weights."""
import math
import random
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gvl_oracle as O  # noqa: E402
from gpu_util import DEV  # noqa: E402
from grammar_ref import restate, same_bits  # noqa: E402
from grounded_video_llm_amd import grammar as GR, lib as L, logits as LP, prompts as P, serve  # noqa: E402
from grounded_video_llm_amd.model import SyntheticTokenizer  # noqa: E402
from test_gpu_token_rules import _build, _pages_back, _rules, _samples  # noqa: E402  (the same tiny geometry: hidden 128, 2 layers, vocab 640)

bf = torch.bfloat16
ANSWER = re.compile(r"From <(\d+)> to <(\d+)>\.")
QUESTION = "When does the person open the door in the video?"


@pytest.fixture(scope="module")
def phi():
    m = _build("phi3.5")
    yield m
    m[0].engine.close()


def _text(tok, ids):
    """The ids as text.  The synthetic tokenizer hashes words to ids and cannot turn them back (its batch_decode prints w<id>), so the three literal words of
    the answer are looked up by THEIR ids here; every other id decodes as the tokenizer decodes it."""
    words = {tok._word(w): w for w in ("From", "to", ".")}
    return " ".join(words.get(int(i)) or tok.batch_decode([[int(i)]], skip_special_tokens=True)[0] for i in ids if int(i) != tok.eos_token_id)


def _in_language(text):
    m = ANSWER.fullmatch(text.replace(" .", "."))
    return bool(m) and int(m.group(1)) <= int(m.group(2))


# ---- 1. the operator ----------------------------------------------------------------------------------------------------------------
def _ring(V):
    """256 states x 16 classes: 16 contiguous classes, the last one ordinal; state s takes class s % 15 or the ordinal class (SET every 64 states, GE otherwise)"""
    tc = np.minimum(np.arange(V) * 16 // V, 15)
    base = [-1] * 15 + [int(np.nonzero(tc == 15)[0][0])]
    tr = np.full((256, 16), GR.FORBIDDEN)
    for s in range(256):
        tr[s, s % 15] = (s + 1) % 256
        tr[s, 15] = ((s + 1) % 256) | (GR.SET if s % 64 == 0 else GR.GE)
    return GR.Grammar(256, 16, 0, V, tc, base, tr)


def _full(V):
    """64 states x 64 classes, the 8 KB table full: two thirds of the 4096 entries lead somewhere, the odd classes ordinal with SET / GE edges"""
    tc = np.arange(V) * 64 // V
    base = [int(np.nonzero(tc == c)[0][0]) if c % 2 else -1 for c in range(64)]
    tr = np.full((64, 64), GR.FORBIDDEN)
    for s in range(64):
        for c in range(64):
            if (s + c) % 3:
                tr[s, c] = ((s * 7 + c) % 64) | ((GR.SET if (s + c) % 5 == 0 else GR.GE if (s + c) % 5 == 1 else 0) if c % 2 else 0)
    return GR.Grammar(64, 64, 0, V, tc, base, tr)


def _tail(V):
    """an ordinal class that ends at the row's last id V - 1: a non-decreasing run of its ids (SET and GE on one edge) between other tokens"""
    b = GR.GrammarBuilder(V)
    last = b.token_class(range(V - 100, V), ordinal=True)
    s0, s1 = b.state(), b.state()
    b.edge(s0, 0, s0); b.edge(s0, last, s1, set_reg=True); b.edge(s1, last, s1, set_reg=True, ge_reg=True); b.edge(s1, 0, s0)
    return b.build(s0)


def _sentence(g, n, rng):
    """up to n ids the grammar accepts one after the other (a random walk over its classes that enters an END state only where nothing else is left, and stops there)"""
    ids_of = [np.nonzero(g.token_class == c)[0] for c in range(g.n_classes)]
    ends = [g.is_end(s) for s in range(g.n_states)]
    state, reg, out = g.start, 0, []
    while len(out) < n and not ends[state]:
        edges = [(c, int(g.trans[state, c])) for c in range(g.n_classes) if g.trans[state, c] != GR.FORBIDDEN and len(ids_of[c]) and
                 not (int(g.trans[state, c]) & GR.GE and reg >= len(ids_of[c]))]
        edges = [x for x in edges if not ends[x[1] & GR.NEXT_MASK]] or edges
        c, e = edges[rng.randrange(len(edges))]
        o = rng.randrange(reg if e & GR.GE else 0, len(ids_of[c]))
        out.append(int(ids_of[c][o]))
        if e & GR.SET:
            reg = o
        state = e & GR.NEXT_MASK
    return out


# (history length, grammar, what the history does, rule set, penalty, ngram, min_new): the first row alone (B = 1), the first five, all sixteen
ROWS = [(8192, "ordered", "in", "mix", 1.3, 3, 0), (0, None, "in", None, 1.0, 0, 0), (0, "interval", "in", None, 1.0, 0, 0), (1, "interval", "in", None, 1.0, 0, 0),
        (2, "interval", "in", None, 1.0, 0, 0), (1023, "ring", "in", None, 1.0, 0, 0), (1024, "full", "in", None, 1.0, 0, 0), (1025, "ordered", "in", "mix", 0.7, 2, 2000),
        (6, "interval", "end", None, 1.0, 0, 0), (3, "interval", "forbidden", None, 1.0, 0, 0), (4, "ordered", "outside", None, 1.0, 0, 0), (2, None, "in", "mix", 1.3, 2, 0),
        (8192, "ring", "in", None, 1.0, 0, 0), (1024, "tail", "in", None, 1.0, 0, 0), (5, "interval", "in", "force5", 1.0, 0, 0), (8192, "full", "in", "sup", 1.0, 0, 0)]


def test_op_with_grammar_equals_restatement_bit_for_bit(phi):
    eng = phi[0].engine
    g = torch.Generator().manual_seed(13)
    rng = random.Random(13)
    assert {0, 1, 2, 1023, 1024, 1025, 8192} <= {r[0] for r in ROWS}
    for V in (640, 32064 + 302, 128256 + 302):
        tok = SyntheticTokenizer(V, 300)
        eos = tok.eos_token_id
        grammars = {"interval": GR.grounding_grammar(tok, 300, eos, "interval"), "ordered": GR.grounding_grammar(tok, 300, eos, "ordered"), "ring": _ring(V),
                    "full": _full(V), "tail": _tail(V)}
        assert grammars["ring"].trans.shape == (256, 16) and grammars["full"].trans.size == GR.MAX_TRANS and grammars["tail"].token_class[V - 1] == 1
        rnd = lambda n: [int(t) for t in torch.randint(0, V, (n,), generator=g)]
        sets = {"mix": _rules(suppress=rnd(40), sb={(V - 1,): 0.5, (7,): -3.5, (tok.tok2id["<150>"],): 2.0}, bw={(V - 2,): -math.inf, (tok.tok2id["<151>"],): -math.inf}),
                "force5": _rules(force=[eos], force_at=5), "sup": _rules(suppress=rnd(300) + [V - 1])}
        gids = {k: eng.grammar_create(v) for k, v in grammars.items()}
        rids = {k: eng.rules_create(v) for k, v in sets.items()}
        try:
            hists = []
            for n, gname, what, *_ in ROWS:
                if gname is None:
                    h = rnd(n)
                else:
                    gr = grammars[gname]
                    h = _sentence(gr, n - (what in ("forbidden", "outside")), rng)
                    if what == "forbidden":
                        h.append(tok.tok2id["<timestamp_grounding>"])             # never allowed, here where the literal "to" must stand
                    elif what == "outside":
                        h.append(V)
                    elif gname == "ordered":                                      # end inside a pair (state B: eos and the earlier timestamps are forbidden)
                        h[-1] = tok.tok2id["<150>"] if gr.walk(h[:-1])[1] == gr.start else tok._word("the")
                    elif gname == "tail":                                         # end inside a run, the register at 50: the run's lower ids are forbidden, V - 1 is not
                        h[-2:] = [3, V - 50]
                    on, state, _ = gr.walk(h)
                    assert len(h) == n and on == (what in ("in", "end")) and (not on or gr.is_end(state) == (what == "end")), (gname, what)
                hists.append(h)
            for B in (1, 5, 16):
                x = torch.randn((B, V), generator=g) * 4.0
                x[:, ::7] = 0.0
                x[:, 3::11] = -0.0
                x[:, 5::13] = -math.inf
                pen, ngr, mnw = [r[4] for r in ROWS[:B]], [r[5] for r in ROWS[:B]], [r[6] for r in ROWS[:B]]
                args = (hists[:B], pen, ngr, mnw, [eos] * B)
                rl = [rids.get(r[3]) for r in ROWS[:B]]
                got = eng.op_logits_process(x.to(DEV).contiguous(), *args, rules=rl, grammar=[gids.get(r[1]) for r in ROWS[:B]]).cpu()
                without = eng.op_logits_process(x.to(DEV).contiguous(), *args, rules=rl).cpu()           # the launch with no grammar in it
                for b_ in range(B):
                    n, gname, what, rname, *_ = ROWS[b_]
                    ref = restate(x[b_], hists[b_], grammars.get(gname), sets.get(rname), pen[b_], ngr[b_], mnw[b_], eos)
                    assert not torch.isnan(ref).any()
                    assert torch.equal(got[b_], ref), (V, B, b_, ROWS[b_])
                    if gname is None:
                        assert same_bits(got[b_], without[b_]), (V, B, b_)
                        continue
                    masked = what == "in"
                    # what the grammar changed, it changed in the restatement too: nothing in OFF / END rows, something in every other (but a forced eos
                    # overrides the grammar: the same row either way)
                    same = torch.equal(ref, restate(x[b_], hists[b_], None, sets.get(rname), pen[b_], ngr[b_], mnw[b_], eos))
                    assert torch.equal(got[b_], without[b_]) == same, (V, B, b_)
                    assert same if not masked else (not same or rname == "force5"), ("the grammar did nothing / something", V, B, b_)
                    if rname is None:                                             # the grammar alone: the sign of every zero as well
                        assert same_bits(got[b_], ref), (V, B, b_, ROWS[b_])
                        assert same_bits(got[b_], x[b_]) == (not masked), (V, B, b_, ROWS[b_])        # END and OFF rows come back unchanged, bit for bit
                    if gname == "tail":
                        assert math.isfinite(float(ref[V - 1])) or math.isinf(float(x[b_, V - 1]))         # the row's last id is in the ordinal class and allowed
        finally:
            for i in rids.values():
                eng.rules_destroy(i)
            for i in gids.values():
                eng.grammar_destroy(i)


# ---- 2. generate(), greedy, against the oracle ----------------------------------------------------------------------------------------
def test_generate_with_interval_grammar_matches_oracle(phi):
    model, sd, tok, geo, sp, tp = phi
    eng, eos = model.engine, tok.eos_token_id
    gr = GR.grounding_grammar(tok, 300, eos, "interval")
    samples = _samples("phi3.5", sp, tp, [QUESTION])
    ids = O.tokenizer_image_token(samples["prompts"][0], tok, tok.bos_token_id)
    ref_vis = O.encode_images(sp, tp, sd["vision_tower"], sd["video_encoder"], sd["projectors"], "phi3.5", clip_layers=3, clip_heads=4, iv2_depth=3, iv2_heads=4, emu=True)[0]
    ocfg = O.LLMConfig("phi3", 128, 256, 2, 4, geo.kv_heads, 640, 1e-5, geo.rope_theta, 131072, 4096, geo.rope_short, geo.rope_long)
    W = sd["language_model"]
    ref_emb = O.splice(torch.tensor(ids), ref_vis, W["model.embed_tokens.weight"], emu=True)
    out = model.generate(samples, do_sample=False, max_new_tokens=12, grammar=gr, return_dict_in_generate=True)
    got = list(out.sequences[0])
    # oracle: KV-cached llm_forward loop + the restatement on every step's row
    e = O._r(W["model.embed_tokens.weight"], True)
    cache = [None] * ocfg.layers
    logits = O.llm_forward(ocfg, W, ref_emb, True, cache, 0, last_only=True)
    n, ref_ids, margins, scales = ref_emb.shape[0], [], [], []
    while len(ref_ids) < 12:
        s = restate(logits[-1], ref_ids, gr)
        top2 = torch.topk(s, 2)
        ref_ids.append(int(top2.indices[0])); margins.append(float(top2.values[0] - top2.values[1])); scales.append(float(logits[-1].abs().max()))
        if ref_ids[-1] == eos:
            break
        logits = O.llm_forward(ocfg, W, e[ref_ids[-1]][None], True, cache, n, last_only=True)
        n += 1
    for i, (a, b) in enumerate(zip(got, ref_ids)):
        if a != b:
            print(f"[parity] grammar: ids part ways at token {i} ({a} vs {b}); oracle margin {margins[i] / scales[i]:.3e} of the logit scale")
            assert margins[i] < min(2 * 2e-2 * scales[i], 0.25), (i, a, b, margins[i], scales[i])
            break
    else:
        assert len(got) == len(ref_ids)
    assert gr.accepts(got) and gr.accepts(ref_ids) and len(got) == 6 and got[-1] == eos
    assert _in_language(_text(tok, got)), _text(tok, got)
    assert out.texts[0] == tok.batch_decode([got], skip_special_tokens=True)[0].strip()
    # the same prompt without the grammar: seeded random weights never answer in the language -- the test shows the feature, not the weights
    plain = model.generate(samples, do_sample=False, max_new_tokens=12, return_dict_in_generate=True)
    assert not _in_language(_text(tok, plain.sequences[0])) and not gr.accepts(list(plain.sequences[0])), plain.texts
    with pytest.raises(ValueError, match="grammar="):
        model.generate(samples, do_sample=False, max_new_tokens=12, prefix_allowed_tokens_fn=gr.as_prefix_allowed_tokens_fn())
    _pages_back(eng)


# ---- 3. every route gives the same ids ------------------------------------------------------------------------------------------------
def test_every_route_gives_the_same_ids(phi):
    model, sd, tok, geo, sp, tp = phi
    eng, eos = model.engine, tok.eos_token_id
    eng.set_logits_processors(); eng.set_token_rules(None); eng.set_grammar(None); eng.set_sampling(False)
    gr = GR.grounding_grammar(tok, 300, eos, "interval")
    embs = [(torch.randn((S, 128), generator=torch.Generator().manual_seed(100 + S)) * 1.5).to(bf).to(DEV) for S in (37, 64, 90)]
    plain = [eng.generate_ids(e, 12, eos) for e in embs]
    gid = eng.grammar_create(gr)
    try:
        alone = eng.generate_ids(embs[1], 12, eos, grammar=gid)
        assert gr.accepts(alone) and not gr.accepts(plain[1])
        # a batch of three whose neighbours have no grammar; graph replay on and off
        for graph in (1, 0):
            eng.debug_set("decode_graph", graph)
            seqs = [eng.seq_alloc(e.shape[0] + 12) for e in embs]
            try:
                eng.seq_set_grammar(seqs[1], gid)
                eng.prefill_batch(seqs, embs)
                assert eng.decode_greedy_batch(seqs, 12, eos) == [plain[0], alone, plain[2]], graph
            finally:
                for s_ in seqs:
                    eng.seq_free(s_)
        eng.debug_set("decode_graph", 1)
        # the continuous-batching scheduler: chunks of 8 steps run past the answer's eos (an END state: rows untouched, ids discarded)
        for max_active in (1, 3):
            sch = serve.ClipScheduler(eng, eos, max_active=max_active, chunk=8)
            rq = [sch.submit(e, 12, grammar=gid if i == 1 else None) for i, e in enumerate(embs)]
            out = sch.run()
            assert [out[r] for r in rq] == [plain[0], alone, plain[2]], max_active
        # seeded sampling, each request with its own (seed, stream): in the language, whatever the grouping
        sampled = []
        for max_active in (1, 3):
            sch = serve.ClipScheduler(eng, eos, max_active=max_active, chunk=8)
            rq = [sch.submit(e, 12, grammar=gid, do_sample=True, temperature=1.5, top_k=0, seed=11 + i) for i, e in enumerate(embs)]
            out = sch.run()
            sampled.append([out[r] for r in rq])
            assert all(gr.accepts(x) for x in sampled[-1]), sampled[-1]
        assert sampled[0] == sampled[1]
        # a fork taken mid-answer, within the prompt (128 rows: whole pages and whole query blocks): the source is three ids into its answer; the fork shares the
        # prompt's pages, inherits the grammar, holds none of those ids, and behind its own tail gives a whole answer -- the one a sequence on its own gives
        long = (torch.randn((150, 128), generator=torch.Generator().manual_seed(250)) * 1.5).to(bf).to(DEV)
        base = eng.seq_alloc(128 + 12)
        eng.seq_set_grammar(base, gid)
        eng.prefill(base, long[:128])
        eng.decode_steps([base], 2)
        assert len(eng.seq_read(base)) == 3
        fork = eng.seq_fork(base, 128, 150 + 12)
        try:
            eng.prefill_extend(fork, long[128:])
            forked = eng.decode_greedy(fork, 12, eos)
            assert forked == eng.generate_ids(long, 12, eos, grammar=gid) and gr.accepts(forked)
        finally:
            eng.seq_free(fork); eng.seq_free(base)
        # a fork whose prefix would reach INTO the answer (62 prompt rows, four ids generated: the first page boundary lies behind two of them) is refused: the rows
        # appended behind a fork are embeddings, so its walk could not go on.  With the grammar off the same fork is an ordinary one
        short = (torch.randn((62, 128), generator=torch.Generator().manual_seed(62)) * 1.5).to(bf).to(DEV)
        src = eng.seq_alloc(62 + 12)
        eng.seq_set_grammar(src, gid)
        eng.prefill(src, short)
        eng.decode_steps([src], 3)
        free0 = eng.kv_info()["free_pages"]
        with pytest.raises(L.GvlError) as e:
            eng.seq_fork(src, 64, 100)
        assert e.value.status == L.ERR_STATE and "grammar" in str(e.value) and eng.kv_info()["free_pages"] == free0
        eng.seq_set_grammar(src, None)
        eng.seq_free(eng.seq_fork(src, 64, 100))
        eng.seq_free(src)
        # a clone taken mid-answer takes the source's answer so far with it (ids, count, the id to feed next): what the caller reads from it is the source's
        # prefix plus a continuation in the language -- under greedy decoding the source's own answer.  Without a grammar a clone's list starts empty, as ever
        src = eng.seq_alloc(64 + 24)
        eng.seq_set_grammar(src, gid)
        eng.seq_set_logprobs(src, 2)
        eng.prefill(src, embs[1])
        eng.decode_steps([src], 2)
        head = eng.seq_read(src)
        assert head == alone[:3]
        clone = eng.seq_clone(src, 64 + 24)
        try:
            assert eng.seq_read(clone) == head and eng.seq_read_logprobs(clone, 0, 3, top=True) == eng.seq_read_logprobs(src, 0, 3, top=True)
            eng.decode_steps([clone], 1)                                         # on its own first, then beside the source, which is one step behind
            eng.decode_steps([src, clone], 4)
            n = len(alone)
            assert n <= 7 and eng.seq_read(src)[:n] == alone and eng.seq_read(clone)[:n] == alone
            assert eng.seq_read_logprobs(clone, 0, n, top=True) == eng.seq_read_logprobs(src, 0, n, top=True)
            eng.seq_set_grammar(src, None)
            bare = eng.seq_clone(src, 64 + 24)
            assert eng.seq_read(bare) == []
            eng.seq_free(bare)
        finally:
            eng.seq_free(clone); eng.seq_free(src)
    finally:
        eng.grammar_destroy(gid)
    assert [eng.generate_ids(e, 12, eos) for e in embs] == plain                 # nothing carries over
    # the public surface: generate() per prompt == a batch of three == generate_shared; a seeded sampled call stays in the language
    qs = [QUESTION, "What is on the table?", "Describe the video in detail please."]
    kw = dict(do_sample=False, max_new_tokens=12, grammar=gr, return_dict_in_generate=True)
    one = [list(model.generate(_samples("phi3.5", sp, tp, [q]), **kw).sequences[0]) for q in qs]
    assert all(gr.accepts(x) and _in_language(_text(tok, x)) for x in one), one
    assert [list(x) for x in model.generate(_samples("phi3.5", sp, tp, qs), **kw).sequences] == one
    shared = model.generate_shared(_samples("phi3.5", sp, tp, qs[:1]), [P.build_prompt("phi3.5", "grounding", q) for q in qs], **kw)
    assert [list(x) for x in shared.sequences] == one
    smp = dict(do_sample=True, temperature=1.5, top_p=None, max_new_tokens=12, grammar=gr, seed=11, return_dict_in_generate=True, output_scores=True)
    s1, s2 = model.generate(_samples("phi3.5", sp, tp, qs[:1]), **smp), model.generate(_samples("phi3.5", sp, tp, qs[:1]), **smp)
    assert s1.sequences == s2.sequences and gr.accepts(list(s1.sequences[0])) and _in_language(_text(tok, s1.sequences[0]))
    again = model.generate(_samples("phi3.5", sp, tp, qs[:1]), do_sample=False, max_new_tokens=12, return_dict_in_generate=True)
    assert not gr.accepts(list(again.sequences[0])) and not _in_language(_text(tok, again.sequences[0]))      # the grammar is gone with its call
    _pages_back(eng)


# ---- 4. beams -------------------------------------------------------------------------------------------------------------------------
def test_beam_search_with_grammar(phi):
    model, sd, tok, geo, sp, tp = phi
    eng, eos = model.engine, tok.eos_token_id
    gr = GR.grounding_grammar(tok, 300, eos, "interval")
    row = O.tokenizer_image_token(P.build_prompt("phi3.5", "grounding", QUESTION), tok, tok.bos_token_id)
    feats = model.encode_images(_samples("phi3.5", sp, tp, ["x"]))[0]
    plain = model.beam_generate_ids(row, feats, 3, 12)
    gid = eng.grammar_create(gr)
    try:
        host = model.beam_generate_ids(row, feats, 3, 12, grammar=gid, impl="host")
        device = model.beam_generate_ids(row, feats, 3, 12, grammar=gid, impl="device")
        # the same search with the whole pipeline restated on the CPU on the same step rows
        dev_op, calls = eng.op_logits_process, []

        def cpu_op(lp, hists, *a, rules=None, grammar=None):
            calls.append(grammar)
            return torch.stack([restate(lp[j], hists[j], gr if grammar == gid else None) for j in range(lp.shape[0])]).to(lp.device)
        eng.op_logits_process = cpu_op
        try:
            ref = model.beam_generate_ids(row, feats, 3, 12, grammar=gid)
        finally:
            eng.op_logits_process = dev_op
        assert calls and all(c == gid for c in calls)
        assert host == device == ref and gr.accepts(host) and _in_language(_text(tok, host)) and host != plain and not gr.accepts(plain)
        for impl in ("host", "device"):
            text = model.generate(_samples("phi3.5", sp, tp, [QUESTION]), num_beams=3, do_sample=False, max_new_tokens=12, grammar=gr, beam_impl=impl)
            assert text[0] == tok.batch_decode([host], skip_special_tokens=True)[0].strip(), (impl, text)
    finally:
        eng.grammar_destroy(gid)
    _pages_back(eng)


# ---- 5. lifetime and errors -------------------------------------------------------------------------------------------------------------
def test_grammar_lifetime_and_errors(phi):
    model, sd, tok, geo, sp, tp = phi
    eng, eos = model.engine, tok.eos_token_id
    eng.set_logits_processors(); eng.set_token_rules(None); eng.set_grammar(None)
    gr = GR.grounding_grammar(tok, 300, eos, "interval")
    emb = (torch.randn((40, 128), generator=torch.Generator().manual_seed(5)) * 1.5).to(bf).to(DEV)
    plain = eng.generate_ids(emb, 12, eos)
    gid = eng.grammar_create(gr)
    want = eng.generate_ids(emb, 12, eos, grammar=gid)
    assert gr.accepts(want) and want != plain

    def status(fn, *a, **kw):
        with pytest.raises(L.GvlError) as e:
            fn(*a, **kw)
        return e.value.status, str(e.value)
    seq = eng.seq_alloc(64)
    eng.seq_set_grammar(seq, gid)
    assert status(eng.grammar_destroy, gid)[0] == L.ERR_STATE                     # referenced by a live sequence
    eng.prefill(seq, emb)
    clone = eng.seq_clone(seq, 64)                                                # a clone keeps the grammar ...
    eng.seq_free(seq)
    assert status(eng.grammar_destroy, gid)[0] == L.ERR_STATE                     # ... and its reference
    eng.seq_free(clone)
    eng.set_grammar(gid)                                                          # the default counts as a reference too
    assert status(eng.grammar_destroy, gid)[0] == L.ERR_STATE
    assert eng.generate_ids(emb, 12, eos) == want                                 # sequences allocated now start with the grammar
    eng.set_grammar(None)
    eng.grammar_destroy(gid)                                                      # after seq_free / the default cleared: fine
    assert status(eng.grammar_destroy, gid)[0] == L.ERR_ARG                       # twice: no such grammar
    assert status(eng.set_grammar, gid)[0] == L.ERR_ARG and status(eng.set_grammar, 63)[0] == L.ERR_ARG and status(eng.set_grammar, -2)[0] == L.ERR_ARG
    seq = eng.seq_alloc(64)
    assert status(eng.seq_set_grammar, seq, 5)[0] == L.ERR_ARG and status(eng.seq_set_grammar, 999, None)[0] == L.ERR_ARG
    x = torch.zeros((1, 640), device=DEV)
    assert status(eng.op_logits_process, x, [[]], 1.0, 0, 0, eos, grammar=7)[0] == L.ERR_ARG           # an unknown id at the operator
    # a vocabulary other than the model's: created, but bound to no sequence; the operator wants it equal to its row width
    other = GR.grounding_grammar(SyntheticTokenizer(700, 300), 300, eos, "interval")
    oid = eng.grammar_create(other)
    for fn, a in ((eng.set_grammar, (oid,)), (eng.seq_set_grammar, (seq, oid))):
        st, msg = status(fn, *a)
        assert st == L.ERR_ARG and "700 ids" in msg and "640" in msg
    st, msg = status(eng.op_logits_process, x, [[]], 1.0, 0, 0, eos, grammar=oid)
    assert st == L.ERR_ARG and "700 ids" in msg
    eng.seq_free(seq)
    eng.grammar_destroy(oid)
    with pytest.raises(ValueError, match="700 ids"):
        model.generate(_samples("phi3.5", sp, tp, [QUESTION]), max_new_tokens=4, grammar=other)
    # a description the library's checker refuses (built past the Python checks): GVL_ERR_ARG with the header's message

    class Raw:
        n_states, n_classes, start, vocab = 1, 1, 0, 640
        token_class, class_base, trans = np.zeros(640, dtype=np.uint8), np.array([-1], dtype=np.int32), np.array([GR.SET], dtype=np.uint16)
    st, msg = status(eng.grammar_create, Raw)
    assert st == L.ERR_ARG and "SET / GE on a class that is not ordinal" in msg
    Raw.trans, Raw.n_states = np.full(257, GR.FORBIDDEN, dtype=np.uint16), 257
    st, msg = status(eng.grammar_create, Raw)
    assert st == L.ERR_ARG and "n_states is 257" in msg
    # 64 live grammars, not one more; every one of them released
    got = [eng.grammar_create(gr) for _ in range(64)]
    assert sorted(got) == list(range(64)) and status(eng.grammar_create, gr)[0] == L.ERR_ARG
    for i in got:
        eng.grammar_destroy(i)
    assert status(eng.grammar_destroy, 0)[0] == L.ERR_ARG                         # every grammar is gone
    assert eng.generate_ids(emb, 12, eos) == plain
    _pages_back(eng)


# ---- 6. the command line ----------------------------------------------------------------------------------------------------------------
def test_inference_cli_constrain_grounding(monkeypatch, capsys):
    """inference.py --synthetic --constrain_grounding, as a user runs it: the grounding call (and only it) carries a grammar over the model's vocabulary, and its ids
    are a sentence of the language; the other two prompts are answered freely."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import inference
    calls, real = [], inference.LLAVA_NEXT_VIDEO.generate

    def spy(self, samples, **kw):
        out = real(self, samples, **kw)
        calls.append((self, kw.get("grammar"), out))
        return out
    monkeypatch.setattr(inference.LLAVA_NEXT_VIDEO, "generate", spy)
    try:
        inference.main(["--synthetic", "--constrain_grounding", "--do_sample", "false", "--output_scores"])
        assert len(calls) == 3 and [c[1] is not None for c in calls] == [True, False, False]
        model, g, out = calls[0]
        assert g.vocab == model.geo.vocab and g.accepts([int(t) for t in out.sequences[0]]), out.sequences
        assert not g.accepts([int(t) for t in calls[1][2].sequences[0]])
        assert "******grounding example******" in capsys.readouterr().out
    finally:
        for m in {id(c[0]): c[0] for c in calls}.values():
            m.engine.close()
