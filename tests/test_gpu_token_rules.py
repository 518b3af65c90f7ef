"""-m gpu: HF generate()'s token rules (sequence_bias, bad_words_ids, forced_eos_token_id, suppress_tokens, begin_suppress_tokens) on the
device (csrc/gvl_logits.hip, rule sets of gvl_rules_create): the operator bit for bit against the torch restatement of the whole ordered
pipeline (tests/token_rules_ref.py, itself pinned to the installed transformers by tests/test_token_rules_cpu.py), generate() against a
KV-cached oracle loop with the same restatement, every way of decoding agreeing with the single-sequence answer, beam search, and the
lifetime / error rules of a rule set."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import gvl_oracle as O  # noqa: E402
from gpu_util import DEV  # noqa: E402
from grounded_video_llm_amd import engine as E, lib as L, logits as LP, prompts as P, serve, synth  # noqa: E402
from grounded_video_llm_amd.model import LLAVA_NEXT_VIDEO, SyntheticTokenizer  # noqa: E402
from token_rules_ref import has_subsequence, restate_rules  # noqa: E402

bf = torch.bfloat16


def _build(llm):
    """The tiny geometry of tests/test_gpu_logits_processors.py."""
    hid, vocab = 128, 640
    kind = "phi3" if llm == "phi3.5" else "llama"
    short, long = synth.longrope_factors(32)
    geo = E.TowerGeometry(llm=llm, clip_hidden=64, clip_inter=128, clip_layers=3, clip_heads=4, iv2_dim=64, iv2_inter=128, iv2_depth=3,
                          iv2_heads=4, hidden=hid, inter=256, layers=2, heads=4, kv_heads=4 if kind == "phi3" else 2, vocab=vocab,
                          rope_short=short if kind == "phi3" else None, rope_long=long if kind == "phi3" else None,
                          rope_theta=10000.0 if kind == "phi3" else 500000.0, max_seq=2048, max_segs=6, kv_pages=40, max_prefill=1024)
    sd = {"vision_tower": synth.clip_weights(64, 128, 3, seed="gen.clip"),
          "video_encoder": synth.iv2_weights(64, 128, 3, 2, seed="gen.iv2"),
          "projectors": synth.projector_weights(llm, hid, 64, 64, seed="gen.proj"),
          "language_model": synth.llm_weights(kind, hid, 256, 2, 4, geo.kv_heads, vocab, True, seed="gen.llm")}
    tok = SyntheticTokenizer(vocab, 300)
    model = LLAVA_NEXT_VIDEO(stage="sft", max_txt_len=64, num_frames=4, num_segs=2, num_temporal_tokens=300, lora=False, llm=llm,
                             geometry=geo, tokenizer=tok, state_dicts=sd, device=DEV)
    sp = synth.det_tensor("gen.sp", (1, 2, 3, 336, 336))
    tp = synth.det_tensor("gen.tp", (1, 4, 3, 224, 224))
    return model, sd, tok, geo, sp, tp


@pytest.fixture(scope="module")
def phi():
    m = _build("phi3.5")
    yield m
    m[0].engine.close()


def _samples(llm, sp, tp, prompts):
    n = len(prompts)
    return {"prompts": [P.build_prompt(llm, "grounding", q) for q in prompts], "spatial_pixel_values": sp.expand(n, -1, -1, -1, -1).contiguous().to(DEV),
            "temporal_pixel_values": tp.expand(n, -1, -1, -1, -1).contiguous().to(DEV), "video_ids": ["synthetic"] * n}


def _pages_back(eng):
    kv = eng.kv_info()
    assert kv["free_pages"] == kv["total_pages"], kv


def _rules(suppress=(), begin=(), force=(), force_at=0, sb=None, bw=None):
    return LP.TokenRules(tuple(suppress), tuple(begin), 0, tuple(force), force_at, LP.group_by_target(sb) if sb else LP.BiasTable(),
                         LP.group_by_target(bw, "bad_words_ids") if bw else LP.BiasTable())


TAIL = [601, 17, 333, 5, 90, 444, 12, 8, 256, 31, 77, 500, 3, 64, 129]          # the last 15 ids of every history that is long enough


def _rule_sets(V, g):
    """name -> TokenRules for rows of width V: every kind on its own, and one set with all kinds and 1 024 multi-token entries."""
    rnd = lambda n: [int(t) for t in torch.randint(0, V, (n,), generator=g)]
    a, b, c = V - 1, V // 2, 7
    t1, t2 = TAIL[-1], TAIL[-2]
    # entry lengths 1, 2 and 16; target a: a length-1 bias plus two matching multi-token entries (the sum order); a non-matching entry; a
    # biased token that sits in the history (t1) for the rows with a penalty
    sb = {(t1, a): 1e8, (a,): 0.1, (t2, t1, a): -1e8, tuple(TAIL) + (b,): 2.75, (c,): -3.5, (t2, c): 1.25, (t1,): 6.0, (9, 9, b): 4.0, (b,): -0.5}
    bw = {(a - 1,): -math.inf, (t1, b + 1): -math.inf, tuple(TAIL) + (c + 1,): -math.inf, (4, 4, c + 2): -math.inf, (t1, t1): -math.inf, (0,): -math.inf}
    many_sb, many_bw = dict(sb), dict(bw)
    pool = rnd(40)
    multi = lambda d: sum(len(k) > 1 for k in d)
    i = 0
    while multi(many_sb) < 1024:                                                # 1 024 multi-token entries per table, lengths 2 .. 16, 40 targets
        n, k = 2 + i % 15, i // 3                                               # every third entry matches the histories' tail
        key = tuple(TAIL[-(2 + k % 15 - 1):]) + (pool[(k // 15) % 40],) if i % 3 == 0 else tuple(rnd(n - 1)) + (pool[i % 40],)
        many_sb.setdefault(key, float(torch.randn((), generator=g)) * 3.0)
        i += 1
    i = 0
    while multi(many_bw) < 1024:
        n, k = 2 + i % 15, i // 5
        key = tuple(TAIL[-(2 + k % 15 - 1):]) + (pool[(k // 15) % 40],) if i % 5 == 0 else tuple(rnd(n - 1)) + (pool[(i * 7) % 40],)
        many_bw.setdefault(key, -math.inf)
        i += 1
    every = _rules(rnd(300), [c, b, 11], [b, 2], 8192, many_sb, many_bw)
    assert sum(n > 0 for _, n in every.sequence_bias.entry_prefix) == 1024 and sum(n > 0 for _, n in every.bad_words.entry_prefix) == 1024
    big = torch.randperm(V, generator=g)[:V - 300].tolist()
    return {"bias": _rules(sb=sb), "bad": _rules(bw=bw), "force16": _rules(force=[5], force_at=16), "begin": _rules(begin=[1, a, 40]),
            "sup300": _rules(suppress=rnd(300)), "supbig": _rules(suppress=big), "all": every}


# (history length, rule set, penalty, ngram, min_new): the first row alone (B = 1), the first five, all sixteen
ROWS = [(2048, "all", 1.3, 3, 0), (0, None, 1.0, 0, 0), (16, "bias", 1.0, 0, 0), (16, "bad", 1.0, 0, 0), (15, "all", 0.7, 2, 20),
        (16, "force16", 1.0, 0, 0), (0, "begin", 1.0, 0, 0), (1, "begin", 1.0, 0, 0), (2, "sup300", 1.3, 0, 0), (8192, "supbig", 1.0, 2, 0),
        (1, "bias", 1.2, 0, 3), (2, "bad", 1.0, 0, 0), (0, "all", 1.5, 2, 1), (2048, "bias", 2.5, 0, 0), (15, "force16", 1.0, 0, 0),
        (8192, "all", 1.3, 3, 9000)]


def test_op_with_rules_equals_restatement_bit_for_bit(phi):
    eng = phi[0].engine
    g = torch.Generator().manual_seed(11)
    assert sorted({r[0] for r in ROWS}) == [0, 1, 2, 15, 16, 2048, 8192]
    for V in (640, 32064 + 302, 128256 + 302):
        sets = _rule_sets(V, g)
        ids = {k: eng.rules_create(v) for k, v in sets.items()}
        try:
            for B in (1, 5, 16):
                x = torch.randn((B, V), generator=g) * 4.0
                x[:, ::7] = 0.0
                x[:, 3::11] = -0.0
                x[:, 5::13] = -math.inf
                hists = []
                for L_, *_ in ROWS[:B]:
                    h = [int(t) for t in torch.randint(0, V, (L_,), generator=g)]
                    k = min(L_, len(TAIL))
                    h[L_ - k:] = TAIL[len(TAIL) - k:]
                    if L_ >= 64:
                        h[40:43] = h[L_ - 3:]                                      # an n-gram that the suffix repeats
                    hists.append(h)
                pen, ngr, mnw = [r[2] for r in ROWS[:B]], [r[3] for r in ROWS[:B]], [r[4] for r in ROWS[:B]]
                eos = [3] * B
                got = eng.op_logits_process(x.to(DEV).contiguous(), hists, pen, ngr, mnw, eos, rules=[ids.get(r[1]) for r in ROWS[:B]]).cpu()
                for b_ in range(B):
                    ref = restate_rules(x[b_], hists[b_], sets.get(ROWS[b_][1]), pen[b_], ngr[b_], mnw[b_], eos[b_])
                    assert not torch.isnan(ref).any()
                    assert torch.equal(got[b_], ref), (V, B, b_, ROWS[b_])
                    if ROWS[b_][1] is not None:                          # the rules matter, except where begin_index / force_at is not reached
                        same = torch.equal(ref, restate_rules(x[b_], hists[b_], None, pen[b_], ngr[b_], mnw[b_], eos[b_]))
                        assert same == (b_ in (7, 14)), ("rules did nothing / something", ROWS[b_])
        finally:
            for i in ids.values():
                eng.rules_destroy(i)


def _plain_and_kwargs(run, eos, vocab):
    """The issue's recipe: rules built from a plain greedy run p (16 ids) through `run(kw) -> ids`."""
    p = run({})
    assert len(p) == 16 and eos not in p, "precondition: the plain run fills its 16 tokens"
    u = next(t for t in range(5, vocab) if t not in p and t != eos)              # an id the plain answer never uses
    kw = dict(bad_words_ids=[[p[0]], p[2:4]], suppress_tokens=[p[1], vocab - 1, vocab - 2], sequence_bias={(u,): 1000.0, (u, u): -2000.0},
              forced_eos_token_id=eos, max_new_tokens=16)
    q = run(kw)
    kw["begin_suppress_tokens"] = [q[0]]                                         # the new first id
    return p, u, q, kw


def _check_rules_visible(got, p, u, q, kw, eos):
    assert p[0] not in got and not has_subsequence(got, p[2:4]), got             # no banned id, no banned sequence
    assert not any(t in got for t in kw["suppress_tokens"]), got
    assert got[0] != q[0] and u in got and got != p, (got, q, p)
    assert len(got) < 16 or got[-1] == eos, got                                  # a 16-token answer ends in eos


@pytest.mark.parametrize("llm", ["phi3.5", "llama3"])
def test_generate_with_rules_matches_oracle(llm, phi):
    model, sd, tok, geo, sp, tp = phi if llm == "phi3.5" else _build(llm)
    eng, eos = model.engine, tok.eos_token_id
    kind = "phi3" if llm == "phi3.5" else "llama"
    samples = _samples(llm, sp, tp, ["When does the person open the door in the video?"])
    ids = O.tokenizer_image_token(samples["prompts"][0], tok, tok.bos_token_id)
    ref_vis = O.encode_images(sp, tp, sd["vision_tower"], sd["video_encoder"], sd["projectors"], llm, clip_layers=3, clip_heads=4,
                              iv2_depth=3, iv2_heads=4, emu=True)[0]
    ocfg = O.LLMConfig(kind, 128, 256, 2, 4, geo.kv_heads, 640, 1e-5, geo.rope_theta, 131072, 4096, geo.rope_short, geo.rope_long)
    W = sd["language_model"]
    ref_emb = O.splice(torch.tensor(ids), ref_vis, W["model.embed_tokens.weight"], emu=True)
    feats = model.encode_images(samples)
    ids_arr, mask = P.left_pad_truncate([ids], tok.pad_token_id, model.max_txt_len)
    eng.set_logits_processors()

    def run(kw):
        rules = LP.resolve_rules(kw, eos, 16, geo.vocab)
        rid = eng.rules_create(rules) if rules.active else None
        try:
            eng.set_token_rules(rid)
            return model.generate_ids(ids_arr, mask, feats, 16)[0]
        finally:
            eng.set_token_rules(None)
            if rid is not None:
                eng.rules_destroy(rid)
    p, u, q, kw = _plain_and_kwargs(run, eos, geo.vocab)
    got = run(kw)
    # oracle: KV-cached llm_forward loop + the restatement on every step's row
    rules = LP.resolve_rules(kw, eos, 16, geo.vocab)
    e = O._r(W["model.embed_tokens.weight"], True)
    cache = [None] * ocfg.layers
    logits = O.llm_forward(ocfg, W, ref_emb, True, cache, 0, last_only=True)
    n, ref_ids, margins, scales = ref_emb.shape[0], [], [], []
    while len(ref_ids) < 16:
        s = restate_rules(logits[-1], ref_ids, rules)
        top2 = torch.topk(s, 2)
        ref_ids.append(int(top2.indices[0])); margins.append(float(top2.values[0] - top2.values[1])); scales.append(float(logits[-1].abs().max()))
        if ref_ids[-1] == eos:
            break
        logits = O.llm_forward(ocfg, W, e[ref_ids[-1]][None], True, cache, n, last_only=True)
        n += 1
    for i, (a, b) in enumerate(zip(got, ref_ids)):
        if a != b:
            print(f"[parity] token rules({llm}): ids part ways at token {i} ({a} vs {b}); oracle margin {margins[i] / scales[i]:.3e} of the logit scale")
            assert margins[i] < min(2 * 2e-2 * scales[i], 0.25), (i, a, b, margins[i], scales[i])
            break
    else:
        assert len(got) == len(ref_ids)
    _check_rules_visible(got, p, u, q, kw, eos)
    _check_rules_visible(ref_ids, p, u, q, kw, eos)
    text = model.generate(samples, do_sample=False, **kw)                          # the public surface, same kwargs
    assert text[0] == tok.batch_decode([got], skip_special_tokens=True)[0].strip()
    _pages_back(eng)
    if llm != "phi3.5":
        eng.close()


def test_decode_paths_agree_with_rules(phi):
    model, sd, tok, geo, sp, tp = phi
    eng, eos = model.engine, tok.eos_token_id
    eng.set_logits_processors()
    eng.set_token_rules(None)
    embs = [(torch.randn((S, 128), generator=torch.Generator().manual_seed(100 + S)) * 1.5).to(bf).to(DEV) for S in (37, 64, 90)]
    plain = [eng.generate_ids(e, 24, eos) for e in embs]
    kws = []
    for p in plain:
        u = next(t for t in range(5, 640) if t not in p and t != eos)
        kws.append(dict(bad_words_ids=[[p[0]], p[2:4]], suppress_tokens=[p[1]], begin_suppress_tokens=[p[4]], sequence_bias={(p[5], u): 500.0, (u,): -1.0},
                        forced_eos_token_id=eos))
    kws[1] = dict(suppress_tokens=plain[1][:6])                                    # a different kind of set for the second request
    rids = [eng.rules_create(LP.resolve_rules(kw, eos, 24, 640)) for kw in kws]
    try:
        single = [eng.generate_ids(e, 24, eos, rules=r) for e, r in zip(embs, rids)]
        assert all(s != p for s, p in zip(single, plain))
        assert len(single[0]) < 24 or single[0][-1] == eos
        # a batch of 3 (a different rule set per sequence, one decode group) == 3 single calls; graph replay on and off
        for graph in (1, 0):
            eng.debug_set("decode_graph", graph)
            seqs = [eng.seq_alloc(e.shape[0] + 24) for e in embs]
            try:
                for s_, r in zip(seqs, rids):
                    eng.seq_set_token_rules(s_, r)
                eng.prefill_batch(seqs, embs)
                assert eng.decode_greedy_batch(seqs, 24, eos) == single, graph
            finally:
                for s_ in seqs:
                    eng.seq_free(s_)
        eng.debug_set("decode_graph", 1)
        # rules next to processors in one group, one member with neither
        procs = LP.Processors(1.3, 2, 3, eos)
        mixed = [eng.generate_ids(embs[0], 24, eos, processors=procs, rules=rids[0]), plain[1], eng.generate_ids(embs[2], 24, eos, processors=procs)]
        seqs = [eng.seq_alloc(e.shape[0] + 24) for e in embs]
        try:
            eng.seq_set_processors(seqs[0], *procs.args()); eng.seq_set_token_rules(seqs[0], rids[0]); eng.seq_set_processors(seqs[2], *procs.args())
            eng.prefill_batch(seqs, embs)
            assert eng.decode_greedy_batch(seqs, 24, eos) == mixed
        finally:
            for s_ in seqs:
                eng.seq_free(s_)
    finally:
        for r in rids:
            eng.rules_destroy(r)
    # the continuous-batching scheduler: per-request kwargs, members at different steps, sets freed at retirement
    sch = serve.ClipScheduler(eng, eos, max_active=3, chunk=5)
    ids_ = [sch.submit(e, 24, **kw) for e, kw in zip(embs, kws)]
    out = sch.run()
    assert [out[r] for r in ids_] == single
    assert [eng.generate_ids(e, 24, eos) for e in embs] == plain                    # nothing carries over
    _pages_back(eng)


def test_generate_surface_with_rules(phi):
    model, sd, tok, geo, sp, tp = phi
    eng, eos = model.engine, tok.eos_token_id
    qs = ["When does the person open the door in the video?", "What is on the table?", "Describe the video in detail please."]
    plain = model.generate(_samples("phi3.5", sp, tp, qs[:1]), do_sample=False, max_new_tokens=14, return_dict_in_generate=True)
    p = plain.sequences[0]
    kw = dict(bad_words_ids=[[p[0]], p[2:4]], suppress_tokens=[p[1]], forced_eos_token_id=eos, max_new_tokens=14)
    one = [model.generate(_samples("phi3.5", sp, tp, [q]), do_sample=False, return_dict_in_generate=True, **kw) for q in qs]
    assert one[0].sequences[0] != p and p[0] not in one[0].sequences[0] and p[1] not in one[0].sequences[0]
    texts = [o.texts[0] for o in one]
    assert model.generate(_samples("phi3.5", sp, tp, qs), do_sample=False, **kw) == texts           # bs 3 == 3 single calls
    assert model.generate_shared(_samples("phi3.5", sp, tp, qs[:1]), [P.build_prompt("phi3.5", "grounding", q) for q in qs], do_sample=False, **kw) == texts
    # a call without the kwargs gives the plain ids again: nothing carries over, every set was destroyed
    again = model.generate(_samples("phi3.5", sp, tp, qs[:1]), do_sample=False, max_new_tokens=14, return_dict_in_generate=True)
    assert again.sequences[0] == p
    # seeded sampling with rules: reproducible, and the bans hold
    smp = dict(kw, do_sample=True, temperature=1.5, top_p=None, return_dict_in_generate=True)
    s1 = model.generate(_samples("phi3.5", sp, tp, qs[:1]), seed=11, **smp)
    s2 = model.generate(_samples("phi3.5", sp, tp, qs[:1]), seed=11, **smp)
    assert s1.sequences == s2.sequences and p[0] not in s1.sequences[0] and p[1] not in s1.sequences[0]
    assert len(s1.sequences[0]) < 14 or s1.sequences[0][-1] == eos
    with pytest.raises(ValueError, match="non-empty list"):
        model.generate(_samples("phi3.5", sp, tp, qs[:1]), bad_words_ids=[])
    with pytest.raises(ValueError, match="exceed the limit of 1024"):
        model.generate(_samples("phi3.5", sp, tp, qs[:1]), bad_words_ids=[[1 + i % 600, 1 + i // 600] for i in range(1025)])
    _pages_back(eng)


def test_beam_search_with_rules(phi):
    model, sd, tok, geo, sp, tp = phi
    eng, eos = model.engine, tok.eos_token_id
    row = O.tokenizer_image_token(P.build_prompt("phi3.5", "grounding", "When does the person open the door in the video?"), tok, tok.bos_token_id)
    feats = model.encode_images(_samples("phi3.5", sp, tp, ["x"]))[0]
    plain = model.beam_generate_ids(row, feats, 3, 16)
    assert len(plain) >= 4
    rule_obj = LP.resolve_rules(dict(bad_words_ids=[[plain[0]], plain[2:4]], suppress_tokens=[plain[1]], forced_eos_token_id=eos), eos, 16, geo.vocab)
    procs = LP.Processors(1.0, 2, 0, eos)
    rid = eng.rules_create(rule_obj)
    try:
        got = model.beam_generate_ids(row, feats, 3, 16, processors=procs, rules=rid)
        # the same search with the whole pipeline restated on the CPU on the same step rows
        dev_op = eng.op_logits_process
        calls = []

        def cpu_op(lp, hists, *a, rules=None):
            calls.append(rules)
            return torch.stack([restate_rules(lp[j], hists[j], rule_obj if rules == rid else None, *procs.args()) for j in range(lp.shape[0])]).to(lp.device)
        eng.op_logits_process = cpu_op
        try:
            ref = model.beam_generate_ids(row, feats, 3, 16, processors=procs, rules=rid)
        finally:
            eng.op_logits_process = dev_op
        assert calls and all(c == rid for c in calls) and got == ref
        assert got != plain and plain[0] not in got and plain[1] not in got
        assert len(got) < 16 or got[-1] == eos
        # through the public surface
        samples = _samples("phi3.5", sp, tp, ["When does the person open the door in the video?"])
        text = model.generate(samples, num_beams=3, do_sample=False, max_new_tokens=16, no_repeat_ngram_size=2, bad_words_ids=[[plain[0]], plain[2:4]],
                              suppress_tokens=[plain[1]], forced_eos_token_id=eos)
        assert text[0] == tok.batch_decode([got], skip_special_tokens=True)[0].strip()
    finally:
        eng.rules_destroy(rid)
    _pages_back(eng)


def test_rule_set_lifetime_and_errors(phi):
    model, sd, tok, geo, sp, tp = phi
    eng, eos = model.engine, tok.eos_token_id
    eng.set_logits_processors()
    eng.set_token_rules(None)
    emb = (torch.randn((40, 128), generator=torch.Generator().manual_seed(5)) * 1.5).to(bf).to(DEV)
    plain = eng.generate_ids(emb, 12, eos)
    rid = eng.rules_create(LP.resolve_rules(dict(suppress_tokens=plain[:4]), eos, 12, 640))
    want = eng.generate_ids(emb, 12, eos, rules=rid)
    assert want != plain and not set(want) & set(plain[:4])

    def status(fn, *a):
        with pytest.raises(L.GvlError) as e:
            fn(*a)
        return e.value.status, str(e.value)
    seq = eng.seq_alloc(64)
    eng.seq_set_token_rules(seq, rid)
    assert status(eng.rules_destroy, rid)[0] == L.ERR_STATE                       # referenced by a live sequence
    eng.prefill(seq, emb)
    clone = eng.seq_clone(seq, 64)                                                # a clone keeps the rules ...
    eng.seq_free(seq)
    assert status(eng.rules_destroy, rid)[0] == L.ERR_STATE                       # ... and its reference
    eng.seq_free(clone)
    eng.set_token_rules(rid)                                                      # the default counts as a reference too
    assert status(eng.rules_destroy, rid)[0] == L.ERR_STATE
    assert eng.generate_ids(emb, 12, eos) == want                                 # sequences allocated now start with the set
    eng.set_token_rules(None)
    eng.rules_destroy(rid)                                                        # after seq_free / the default cleared: fine
    assert status(eng.rules_destroy, rid)[0] == L.ERR_ARG                         # twice: no such set
    assert status(eng.set_token_rules, rid)[0] == L.ERR_ARG
    assert eng.generate_ids(emb, 12, eos) == plain
    # over-capacity sets: GVL_ERR_ARG with a message, nothing truncated (built past the Python checks)
    over = LP.TokenRules(bad_words=LP.BiasTable(tuple((i, i, 1) for i in range(1025)), (-math.inf,) * 1025, tuple((i, 1) for i in range(1025)), tuple(range(1025))))
    st, msg = status(eng.rules_create, over)
    assert st == L.ERR_ARG and "1025 multi-token entries, the limit is 1024" in msg
    long_ = LP.TokenRules(sequence_bias=LP.BiasTable(((5, 0, 1),), (1.0,), ((0, 16),), tuple(range(16))))
    st, msg = status(eng.rules_create, long_)
    assert st == L.ERR_ARG and "17 ids, the limit is 16" in msg
    st, msg = status(eng.rules_create, LP.TokenRules(suppress=tuple(range(LP.MAX_IDS + 1))))
    assert st == L.ERR_ARG and "the limit is 262144" in msg
    twice = LP.TokenRules(sequence_bias=LP.BiasTable(((5, 0, 1), (5, 1, 1)), (1.0, 2.0), ((0, 0), (0, 0)), ()))
    assert status(eng.rules_create, twice)[0] == L.ERR_ARG                        # one thread owns one target
    _pages_back(eng)
