"""-m gpu: classifier-free guidance against a negative sequence (gvl_seq_set_guidance / gvl_op_guidance; guidance_rows_kernel and follow_commit_kernel,
csrc/gvl_pick.hip).  The operator bit for bit against the library's own log-softmax followed by torch's separate fp32 ops, and inside the derived bound of the
float64 restatement (tests/guidance_ref.py); guided decoding exactly equal -- ids and log-probabilities -- to an oracle built from teacher-forced steps and the
operator entries; the pair invariants and refusals; generate() and the ClipScheduler on the tiny models."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import guidance_ref as GR  # noqa: E402
from gpu_util import DEV, bf  # noqa: E402
from grounded_video_llm_amd import grammar as GRM, lib as L, logits as LP, prompts as P, serve  # noqa: E402
from test_gpu_extend_varlen import make_engine  # noqa: E402

NEW = 12


# ---- the operator -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def phi():
    eng, geo = make_engine("phi_d64")
    yield eng
    eng.close()


@pytest.mark.parametrize("n,pairs", GR.op_cases())
def test_op_guidance(phi, n, pairs):
    eng = phi
    x = GR.op_rows(n, pairs)                                       # 2 * pairs + 1 rows: pair p = (row p, row pairs + p); the last row belongs to nobody
    R = x.shape[0]
    pr = [(p, pairs + p) for p in range(pairs)]
    sc = [GR.SCALES[p % 4] for p in range(pairs)]
    xd = x.to(DEV).contiguous()
    got = eng.op_guidance(xd.clone(), pr, sc)
    # (a) bit for bit: the library's log-softmax of each row, then torch's separate fp32 sub, mul, add on the device
    ls = eng.op_beam_normalize(xd[:2 * pairs].clone())              # (the entry takes up to 16 rows: the pairs' own)
    for p, (c, u) in enumerate(pr):
        want = torch.add(torch.mul(torch.sub(ls[c], ls[u]), sc[p]), ls[u])
        assert torch.equal(got[c].view(torch.int32), want.view(torch.int32)), (n, pairs, p)
    # (d) the negative rows and the row nobody names are untouched
    for r in range(pairs, R):
        assert torch.equal(got[r].view(torch.int32), xd[r].view(torch.int32)), (n, pairs, r)
    # (b) every entry inside the derived bound of the float64 restatement
    gc = got.cpu()
    worst = 0.0
    for p, (c, u) in enumerate(pr):
        G, _, _ = GR.guided_row(x[c], x[u], sc[p])
        ratio = float(((gc[c].double() - G).abs() / GR.bound(x[c], x[u], sc[p])).max())
        worst = max(worst, ratio)
    print(f"[guidance] n {n} pairs {pairs}: the kernel uses {worst:.3f} of the bound")
    assert worst <= 1.0
    # (c) a pair's output does not depend on the rows it occupies or on its fellow travellers: the last pair alone, in other rows, with a row pitch > n
    c, u = pr[-1]
    y = torch.full((3, n + 5), 7.0, device=DEV)
    y[2, :n] = xd[c]; y[0, :n] = xd[u]
    z = eng.op_guidance(y[:, :n], [(2, 0)], [sc[-1]])
    assert torch.equal(z[2].view(torch.int32), got[c].view(torch.int32)) and torch.equal(z[0], xd[u]) and bool((y[:, n:] == 7.0).all()) and bool((y[1] == 7.0).all())


def test_op_guidance_refusals(phi):
    x = torch.zeros((4, 400), device=DEV)
    for pr, sc in (([(0, 0)], [1.5]), ([(0, 1), (0, 2)], [1.5, 1.5]), ([(0, 1), (2, 0)], [1.5, 1.5]), ([(0, 1)], [float("inf")]), ([(0, 1)] * 9, [1.5] * 9)):
        with pytest.raises((L.GvlError, ValueError)):
            phi.op_guidance(x, pr, sc)
    with pytest.raises(ValueError):
        phi.op_guidance(x, [(0, 4)], [1.5])
    assert bool((x == 0).all())
    phi.op_guidance(x, [(0, 1), (2, 1)], [1.5, 0.5])                # one negative row may serve two pairs


# ---- guided decoding against the oracle ------------------------------------------------------------------------------------------------------
def _embs(geo, seed, n, lo=20, hi=90):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn((int(torch.randint(lo, hi, (1,), generator=g)), geo.hidden), generator=g) * 0.5).to(bf).to(DEV) for _ in range(n)]


def _grammar(V):
    """the first id comes from the last 100, then a non-decreasing run of them, or anything else and start over"""
    b = GRM.GrammarBuilder(V)
    last = b.token_class(range(V - 100, V), ordinal=True)
    s0, s1 = b.state(), b.state()
    b.edge(s0, last, s1, set_reg=True); b.edge(s1, last, s1, set_reg=True, ge_reg=True); b.edge(s1, 0, s0)
    return b.build(s0)


def _open_pair(eng, ec, en, scale, max_new=NEW, procs=None, grammar=None, sampling=None, logprobs=0, slack=0):
    s = eng.seq_alloc(ec.shape[0] + max_new)
    f = eng.seq_alloc(en.shape[0] + max_new + slack)
    lc, lu = eng.prefill(s, ec, want_logits=True), eng.prefill(f, en, want_logits=True)     # RAW rows: the leader takes its settings after its prefill
    LP.apply_seq_options(eng, s, LP.SeqOptions(procs, logprobs, sampling=... if sampling is None else sampling, grammar=... if grammar is None else grammar))
    eng.seq_set_guidance(s, f, scale, lc, lu)
    return s, f


def _oracle(eng, ec, en, scale, max_new=NEW, procs=LP.OFF, grammar=None, sampling=None):
    """calls that exist without guided pairs: both prompts prefilled with their logits; per step the operator entries on the host-held rows, then the token fed to
    BOTH sequences by one teacher-forced batched step"""
    sc, sn = eng.seq_alloc(ec.shape[0] + max_new), eng.seq_alloc(en.shape[0] + max_new)
    try:
        rows = torch.stack([eng.prefill(sc, ec, want_logits=True), eng.prefill(sn, en, want_logits=True)])
        ids, lps = [], []
        while True:
            eng.op_guidance(rows, [(0, 1)], [scale])
            g = rows[0:1].contiguous()
            if procs.active or grammar is not None:
                eng.op_logits_process(g, [ids], *procs.args(), grammar=grammar)
            tok, lp, _, _ = eng.op_select_rows(g, [sampling], top_n=0, steps=[len(ids)])
            ids.append(int(tok[0])); lps.append(float(lp[0]))
            if len(ids) >= max_new:
                return ids, lps
            rows = eng.decode_step_logits_batch([sc, sn], [ids[-1], ids[-1]])
    finally:
        eng.seq_free(sc); eng.seq_free(sn)


def _free(eng, *pairs):
    for s, f in pairs:
        eng.seq_free(s)
        eng.seq_free(f)


@pytest.fixture(scope="module", params=["phi_d64", "llama_d128_gqa", "phi_d96"])
def eg(request):
    eng, geo = make_engine(request.param)
    free0 = eng.kv_info()["free_pages"]
    yield eng, geo
    assert eng.kv_info()["free_pages"] == free0, "pages leaked"
    eng.close()


SAMPLED = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=11, stream=3)
VARIANTS = {"greedy": dict(), "sampled": dict(sampling=SAMPLED), "penalty": dict(procs=LP.Processors(1.6, 2, 0, -1)), "grammar": dict(grammar=True),
            "sampled+penalty+grammar": dict(sampling=SAMPLED, procs=LP.Processors(1.3, 0, 0, -1), grammar=True)}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_guided_decode_equals_the_oracle(eg, variant):
    eng, geo = eg
    kw = dict(VARIANTS[variant])
    gid = eng.grammar_create(_grammar(geo.vocab)) if kw.pop("grammar", False) else None
    ec, en = _embs(geo, 3, 2)
    try:
        want, want_lp = _oracle(eng, ec, en, 1.5, grammar=gid, procs=kw.get("procs", LP.OFF), sampling=kw.get("sampling"))
        plain = eng.generate_ids(ec, NEW, None)
        runs = {}
        for how in ("greedy_batch", "steps1", "steps5", "no_graph"):
            eng.debug_set("decode_graph", 0 if how == "no_graph" else 1)
            s, f = _open_pair(eng, ec, en, 1.5, grammar=gid, **kw)
            try:
                if how.startswith("steps"):
                    k = int(how[5:])
                    done = 1
                    while done < NEW:
                        eng.decode_steps([s], min(k, NEW - done)); done += min(k, NEW - done)
                    ids = eng.seq_read(s, 0, NEW)
                else:
                    ids = eng.decode_greedy_batch([s], NEW, None)[0]
                lp, _ = eng.seq_read_logprobs(s, 0, NEW)
                assert eng.seq_read(f, 0, NEW) == ids, (variant, how)            # the follower's ids are the leader's
                runs[how] = (ids, lp)
            finally:
                _free(eng, (s, f))
        eng.debug_set("decode_graph", 1)
        for how, (ids, lp) in runs.items():
            assert ids == want, (variant, how, ids, want)
            assert lp == want_lp, (variant, how)                                  # bit for bit: every row is batch-invariant
        if gid is not None:
            assert want[0] >= geo.vocab - 100
        print(f"[guidance] {variant}: guided {want} | unguided {plain}")
    finally:
        if gid is not None:
            eng.grammar_destroy(gid)


def test_invariants(eg):
    eng, geo = eg
    embs = _embs(geo, 9, 20)
    ec, en = embs[0], embs[1]
    # a negative identical to the prompt: lc == lu bitwise, the guided row is lu, the ids are the unguided greedy ids at any scale
    plain = eng.generate_ids(ec, NEW, None)
    for scale in (1.5, -1.0, 3.0):
        s, f = _open_pair(eng, ec, ec.clone(), scale)
        assert eng.decode_greedy_batch([s], NEW, None)[0] == plain, scale
        _free(eng, (s, f))
    want, _ = _oracle(eng, ec, en, 2.0)
    assert want != plain
    others = [eng.generate_ids(e, NEW, None) for e in embs[4:17]]
    # next to 0, 1 and 13 plain neighbours (in front of it and behind it), and three pairs together
    for nb in (0, 1, 13):
        s, f = _open_pair(eng, ec, en, 2.0)
        nbs = [eng.seq_alloc(e.shape[0] + NEW) for e in embs[4:4 + nb]]
        if nbs:
            eng.prefill_batch(nbs, embs[4:4 + nb])
        order = nbs[:nb // 2] + [s] + nbs[nb // 2:]
        got = eng.decode_greedy_batch(order, NEW, None)
        assert got[nb // 2] == want and got[:nb // 2] + got[nb // 2 + 1:] == others[:nb], nb
        assert eng.seq_read(f, 0, NEW) == want
        for q in nbs:
            eng.seq_free(q)
        _free(eng, (s, f))
    wants = [_oracle(eng, embs[2 * i], embs[2 * i + 1], sc)[0] for i, sc in ((0, 2.0), (1, 0.5), (2, 3.0))]
    prs = [_open_pair(eng, embs[2 * i], embs[2 * i + 1], sc) for i, sc in ((0, 2.0), (1, 0.5), (2, 3.0))]
    assert eng.decode_greedy_batch([p[0] for p in prs], NEW, None) == wants
    _free(eng, *prs)
    # leader eos ends both members, the neighbour runs on
    eos = want[4]
    cut = want[:want.index(eos) + 1]
    s, f = _open_pair(eng, ec, en, 2.0)
    q = eng.seq_alloc(embs[4].shape[0] + NEW); eng.prefill(q, embs[4])
    other = others[0][:others[0].index(eos) + 1] if eos in others[0] else others[0]
    assert eng.decode_greedy_batch([s, q], NEW, eos) == [cut, other]
    nf = len(eng.seq_read(f, 0, NEW))
    assert len(cut) <= nf <= len(cut) + 2 and eng.seq_read(f, 0, len(cut)) == cut       # (the host sees eos up to two steps late: the pair may have run on together)
    assert len(eng.seq_read(s, 0, NEW)) == nf
    eng.seq_free(q)
    # after the leader is freed the follower decodes as a plain sequence
    eng.seq_free(s)
    more = eng.decode_greedy_batch([f], nf + 3, None)[0]
    assert len(more) == nf + 3 and more[:len(cut)] == cut
    eng.seq_free(f)


def _state(eng, seqs):
    return eng.kv_info()["free_pages"], [eng.seq_read(q, 0, 64) for q in seqs]


def test_refusals_leave_everything_as_it_was(eg):
    eng, geo = eg
    ec, en, ex = _embs(geo, 21, 3)
    s, f = _open_pair(eng, ec, en, 1.5, slack=64)
    q = eng.seq_alloc(ex.shape[0] + NEW); lq = eng.prefill(q, ex, want_logits=True)
    before = _state(eng, [s, f, q])
    one = ex[:1]

    def refused(fn, *a, status=L.ERR_STATE):
        with pytest.raises(L.GvlError) as e:
            fn(*a)
        assert e.value.status == status, (fn.__name__, e.value)
        assert _state(eng, [s, f, q]) == before, fn.__name__
    # a bound follower: any decode, prefill-extend or score call, and freeing it
    refused(eng.decode_greedy_batch, [f], 4, None)
    refused(eng.decode_greedy_batch, [q, f], 4, None)
    refused(eng.decode_steps, [f], 1)
    refused(eng.prefill_extend, f, one)
    refused(eng.prefill_extend_batch, [f], [one])
    refused(eng.score_extend_batch, [f], [one], [[5]])
    refused(eng.seq_free, f)
    # either member: fork, clone, beam search, the teacher-forced steps
    for m in (s, f):
        refused(eng.seq_fork, m, 64, 256)
        refused(eng.seq_clone, m, 512)
        refused(eng.beam_search, m, lq, 2, 4, None)
        refused(eng.decode_step_logits, m, 5)
        refused(eng.decode_step_logits_batch, [q, m], [5, 5])
    # binding: a member of a pair, the same sequence twice, a sequence past its first token, a non-finite scale, too little capacity
    l2 = lq.clone()
    refused(eng.seq_set_guidance, q, f, 1.5, lq, l2)
    refused(eng.seq_set_guidance, s, q, 1.5, lq, l2)
    refused(eng.seq_set_guidance, q, q, 1.5, lq, l2, status=L.ERR_ARG)
    refused(eng.seq_set_guidance, q, 9999, 1.5, lq, l2, status=L.ERR_ARG)
    refused(eng.seq_set_guidance, q, s, float("nan"), lq, l2, status=L.ERR_ARG)
    eng.seq_set_guidance(s, None)                                   # unbind: both are plain again, still at their first token
    assert _state(eng, [s, f, q]) == before
    refused(eng.seq_set_guidance, f, q, 1.5, lq, l2)                # f has 64 tokens more room than q: q cannot follow it
    eng.decode_steps([q], 1)
    before = _state(eng, [s, f, q])
    refused(eng.seq_set_guidance, s, q, 1.5, lq, l2)                # q is past its first token
    for m in (s, f, q):
        eng.seq_free(m)


# ---- generate() and the scheduler on the tiny models ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_model():
    from test_gpu_logits_processors import _build
    m = _build("phi3.5")
    yield m
    m[0].engine.close()


def test_generate_with_guidance(tiny_model):
    from test_gpu_logits_processors import _pages_back, _samples
    model, sd, tok, geo, sp, tp = tiny_model
    eng = model.engine
    qs = ["when does the person open the door?", "what happens after the dog runs away?"]
    samples = _samples("phi3.5", sp, tp, qs)
    base = model.generate(samples, max_new_tokens=10)
    assert model.generate(samples, max_new_tokens=10, guidance_scale=1) == base and model.generate(samples, max_new_tokens=10, guidance_scale=None) == base
    feats = model.encode_images(samples)
    pad = tok.pad_token_id or 0
    ids_arr, mask = P.left_pad_truncate([model.tokenizer_image_token(t) for t in samples["prompts"]], pad, model.max_txt_len)
    conds = [eng.splice([int(t) for t, m in zip(ids_arr[i], mask[i]) if m], feats[i]) for i in range(2)]
    eos = tok.eos_token_id
    for negs in (["describe the video.", "what is shown?"],                                  # text-only: the video-free contrast
                 [P.build_prompt("phi3.5", "qa", "answer with a wrong time."), "no video here"]):   # with the <image> slot: the same video, another instruction
        got = model.generate(samples, max_new_tokens=10, guidance_scale=2.0, negative_prompts=negs, return_dict_in_generate=True)
        for i in range(2):
            row = model.tokenizer_image_token(negs[i])
            ne = eng.splice(row, feats[i]) if P.IMAGE_TOKEN_INDEX in row else eng.embed_ids(row)
            sc, sn = eng.seq_alloc(conds[i].shape[0] + 10), eng.seq_alloc(ne.shape[0] + 10)
            fc, fu = eng.prefill(sc, conds[i], want_logits=True), eng.prefill(sn, ne, want_logits=True)
            want = GR.generate(lambda t: eng.decode_step_logits(sc, t), lambda t: eng.decode_step_logits(sn, t), fc, fu, 2.0, 10, eos, GR.greedy)
            eng.seq_free(sc); eng.seq_free(sn)
            assert list(got.sequences[i]) == want, (negs, i)
    ids = [model.tokenizer_image_token("describe the video.")] * 2
    a = model.generate(samples, max_new_tokens=10, guidance_scale=2.0, negative_prompts=["describe the video."] * 2)
    assert model.generate(samples, max_new_tokens=10, guidance_scale=2.0, negative_prompt_ids=ids) == a
    for kw in (dict(), dict(negative_prompts=["a", "b"], num_beams=2)):
        with pytest.raises(ValueError):
            model.generate(samples, max_new_tokens=4, guidance_scale=2.0, **kw)
    with pytest.raises(ValueError):
        model.generate_shared(_samples("phi3.5", sp, tp, qs[:1]), qs, max_new_tokens=4, guidance_scale=2.0, negative_prompts=["a", "b"])
    _pages_back(eng)


def test_scheduler_guided_ids_do_not_depend_on_the_schedule(eg):
    eng, geo = eg
    embs = _embs(geo, 33, 8)
    want = {0: _oracle(eng, embs[0], embs[1], 2.0, 10)[0], 1: _oracle(eng, embs[2], embs[3], 0.5, 7)[0]}
    plain = [eng.generate_ids(e, 9, None) for e in embs[4:8]]
    for max_active, chunk, n_plain in ((2, 1, 0), (3, 4, 2), (8, 3, 4), (16, 16, 4)):
        sch = serve.ClipScheduler(eng, None, max_active=max_active, chunk=chunk)
        order = []
        for i in range(max(n_plain, 2)):
            if i < n_plain:
                order.append(("p", i, sch.submit(embs[4 + i], 9)))
            if i < 2:
                order.append(("g", i, sch.submit(embs[2 * i], (10, 7)[i], guidance_scale=(2.0, 0.5)[i], negative=embs[2 * i + 1])))
        out = sch.run()
        for kind, i, rid in order:
            assert out[rid] == (want[i] if kind == "g" else plain[i]), (max_active, chunk, n_plain, kind, i)
        assert sch.stats["max_concurrent"] <= max_active
    with pytest.raises(ValueError):
        serve.ClipScheduler(eng, None, max_active=1).submit(embs[0], 4, guidance_scale=2.0, negative=embs[1])
    with pytest.raises(ValueError):
        serve.ClipScheduler(eng, None).submit(embs[0], 4, guidance_scale=2.0)
