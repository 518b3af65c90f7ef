"""-m gpu: per-sequence sampling (gvl_seq_set_sampling, SeqSelect::own_sampling; pick_tokens -> select_rows_kernel) on the tiny Phi-3.5 and Llama geometries:
a decode group that mixes a greedy sequence, a follower of the ctx setting and sequences with their own settings gives every member the ids and
log-probabilities it gets on its own, with graph replay on and off; followers without new warpers are today's sampler; a request's ids do not depend on
its place in the scheduler's traffic; forks and clones carry the setting; the reported alternatives lie in the restated kept set of the teacher-forced rows;
generate()'s arguments."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import warpers_ref as WR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from grounded_video_llm_amd import engine as E, prompts as P, serve  # noqa: E402

from test_gpu_logits_processors import _build, _pages_back, _samples  # noqa: E402  (same tiny geometries)

bf = torch.bfloat16
NEW = 12
CTX = dict(temperature=0.9, top_k=20, top_p=0.95, seed=5)                       # the ctx setting the follower uses
GREEDY = dict(do_sample=False)
OWN1 = dict(do_sample=True, temperature=0.7, top_k=0, top_p=0.9, seed=101, stream=3)
OWN2 = dict(do_sample=True, temperature=1.2, top_k=50, top_p=0.95, min_p=0.02, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=2e-3, seed=202, stream=1)
MEMBERS = (..., GREEDY, OWN1, OWN2)                                             # ...: follows the ctx setting (first: it takes the ctx's random stream 0)


@pytest.fixture(scope="module")
def models():
    """llm -> its tiny model, built on first use, one engine per geometry for the whole module"""
    made = {}

    def get(llm):
        if llm not in made:
            made[llm] = _build(llm)
        return made[llm]
    yield get
    for m in made.values():
        m[0].engine.close()


@pytest.fixture(scope="module")
def phi(models):
    return models("phi3.5")


def _embs(lens=(37, 64, 90, 21), seed=300):
    return [(torch.randn((S, 128), generator=torch.Generator().manual_seed(seed + S)) * 1.5).to(bf).to(DEV) for S in lens]


def _ctx_sampling(eng):
    eng.set_sampling(True, CTX["temperature"], CTX["top_k"], CTX["top_p"], CTX["seed"])


def _open(eng, emb, setting, top_n=2):
    s = eng.seq_alloc(emb.shape[0] + NEW)
    if setting is not ...:
        eng.seq_set_sampling(s, setting)
    eng.seq_set_logprobs(s, top_n)
    return s


def _result(eng, s):
    ids = eng.seq_read(s, 0, NEW)
    lp, top = eng.seq_read_logprobs(s, 0, len(ids), top=True)
    return ids, [np.float32(v).tobytes() for v in lp], [[(i, np.float32(v).tobytes()) for i, v in t] for t in top]


def _group(eng, embs, members, how):
    """the members prefilled and decoded together -> each one's (ids, lp bits, top bits)"""
    _ctx_sampling(eng)
    seqs = [_open(eng, e, m) for e, m in zip(embs, members)]
    try:
        eng.prefill_batch(seqs, embs)
        if how == "batch":
            eng.decode_greedy_batch(seqs, NEW, None)
        else:                                                                   # gvl_decode_steps in uneven chunks
            for k in (1, 4, NEW - 6):
                eng.decode_steps(seqs, k)
        return [_result(eng, s) for s in seqs]
    finally:
        for s in seqs:
            eng.seq_free(s)


@pytest.mark.parametrize("graph", [1, 0])
@pytest.mark.parametrize("how", ["batch", "steps"])
@pytest.mark.parametrize("llm", ["phi3.5", "llama3"])
def test_mixed_group_equals_each_member_alone(models, llm, how, graph):
    eng = models(llm)[0].engine
    embs = _embs()
    eng.debug_set("decode_graph", graph)
    try:
        alone = [_group(eng, [e], [m], how)[0] for e, m in zip(embs, MEMBERS)]
        together = _group(eng, embs, MEMBERS, how)
        assert together == alone
        assert all(len(r[0]) == NEW for r in alone)
        # the greedy member: the ids of an engine that never heard of sampling
        eng.set_sampling(False)
        assert alone[1][0] == eng.generate_ids(embs[1], NEW, None)
        # the sampled members really sample (their own settings differ from greedy and from each other's draws)
        greedy = [eng.generate_ids(e, NEW, None) for e in embs]
        assert any(alone[i][0] != greedy[i] for i in (0, 2, 3))
    finally:
        eng.debug_set("decode_graph", 1)
        eng.set_sampling(False)
    _pages_back(eng)


def test_followers_without_new_warpers_are_todays_sampler(phi):
    """no own setting anywhere and the new warpers off: gvl_set_sampling_ex is gvl_set_sampling, and a ctx-wide new warper changes the ids and goes away again"""
    eng = phi[0].engine
    embs = _embs()

    def run():
        seqs = [eng.seq_alloc(e.shape[0] + NEW) for e in embs]
        try:
            eng.prefill_batch(seqs, embs)
            return eng.decode_greedy_batch(seqs, NEW, None)
        finally:
            for s in seqs:
                eng.seq_free(s)
    _ctx_sampling(eng)
    plain = run()
    g = E.sampling_struct(True, CTX["temperature"], CTX["top_k"], CTX["top_p"], seed=CTX["seed"], stream=77)      # the stream field is ignored here
    eng._chk(eng.lib.gvl_set_sampling_ex(eng.ctx, C.byref(g)), "gvl_set_sampling_ex")
    assert run() == plain
    eng.set_sampling(True, CTX["temperature"], CTX["top_k"], CTX["top_p"], CTX["seed"], min_p=0.5, typical_p=0.3)
    warped = run()
    assert warped != plain
    eng.set_sampling(True, CTX["temperature"], CTX["top_k"], CTX["top_p"], CTX["seed"], min_p=0.5, typical_p=0.3)
    assert run() == warped                                                       # reproducible
    _ctx_sampling(eng)                                                           # plain gvl_set_sampling switches the new warpers off again
    assert run() == plain
    eng.set_sampling(False)
    _pages_back(eng)


def test_request_ids_do_not_depend_on_the_traffic(phi):
    eng = phi[0].engine
    embs = _embs((37, 64, 90, 21, 50))
    own = dict(temperature=0.8, min_p=0.05, epsilon_cutoff=1e-3, seed=77)
    _ctx_sampling(eng)
    s = _open(eng, embs[0], dict(own, do_sample=True, stream=0), top_n=0)
    try:
        eng.prefill_batch([s], embs[:1])
        eng.decode_greedy_batch([s], NEW, None)
        want = eng.seq_read(s, 0, NEW)
    finally:
        eng.seq_free(s)
    for max_active in (1, 4):
        for first in (True, False):
            _ctx_sampling(eng)
            sch = serve.ClipScheduler(eng, None, max_active=max_active, chunk=5)
            others = [lambda e=e, kw=kw: sch.submit(e, NEW, **kw) for e, kw in zip(embs[1:4], ({}, dict(do_sample=False), dict(temperature=1.1, seed=77)))]
            if first:
                rid = sch.submit(embs[0], NEW, **own)
            for f in others:
                f()
            if not first:
                rid = sch.submit(embs[0], NEW, **own)
            assert sch.run()[rid] == want, (max_active, first)
    eng.set_sampling(False)
    _pages_back(eng)


def test_fork_and_clone_carry_the_setting(phi):
    model, sd, tok, geo, sp, tp = phi
    eng = model.engine
    eng.set_sampling(False)
    full = _embs((150,), seed=900)[0]
    s = _open(eng, full, OWN2)
    try:
        eng.prefill_batch([s], [full])
        eng.decode_greedy_batch([s], NEW, None)
        want = _result(eng, s)
    finally:
        eng.seq_free(s)
    # a fork (shared first 128 tokens) of a sequence with its own setting continues as the sequence itself would: the setting came with it
    root = _open(eng, full[:128], OWN2)
    fork = None
    try:
        eng.prefill_batch([root], [full[:128]])
        fork = eng.seq_fork(root, 128, 150 + NEW)
        eng.prefill_extend(fork, full[128:])
        eng.decode_greedy_batch([fork], NEW, None)
        assert _result(eng, fork) == want
        # clones: the copy carries the setting (its generation count restarts at 0, include/gvl.h).  Two clones on the source's stream repeat each other;
        # one moved to another stream diverges; one reset to follow the (greedy) ctx setting is greedy
        last = eng.seq_read(root, 0, 1)[0]
        clones = [eng.seq_clone(root, 128 + NEW + 1) for _ in range(4)]
        try:
            eng.seq_set_sampling(clones[2], dict(OWN2, stream=OWN2["stream"] + 1))
            eng.seq_set_sampling(clones[3], None)
            rows = [eng.decode_step_logits(c, last).cpu().numpy() for c in clones]
            assert all(np.array_equal(r, rows[0]) for r in rows)
            eng.decode_steps(clones, NEW - 1)
            out = [eng.seq_read(c, 0, NEW) for c in clones]
            assert out[0] == out[1] and len(out[0]) == NEW
            assert out[2] != out[0]
            assert out[0][0] == WR.select(rows[0], OWN2, 0)[0] or WR.select(rows[0], OWN2, 0)[1] < 1e-3      # the clone's first draw: its own seed and stream, step 0
            assert out[3][0] == int(np.argmax(rows[0]))
        finally:
            for c in clones:
                eng.seq_free(c)
    finally:
        if fork is not None:
            eng.seq_free(fork)
        eng.seq_free(root)
    # generate_shared (one prefix, forked per prompt) honours the new warpers: reproducible per seed, and they change the answers
    qs = ["When does the person open the door in the video?", "What is on the table?", "Describe the video in detail please."]
    prompts = [P.build_prompt("phi3.5", "grounding", q) for q in qs]
    kw = dict(do_sample=True, temperature=1.5, top_k=0, seed=4, max_new_tokens=NEW)
    a = model.generate_shared(_samples("phi3.5", sp, tp, qs[:1]), prompts, min_p=0.4, **kw)
    assert a == model.generate_shared(_samples("phi3.5", sp, tp, qs[:1]), prompts, min_p=0.4, **kw)
    assert a != model.generate_shared(_samples("phi3.5", sp, tp, qs[:1]), prompts, **kw)
    eng.set_sampling(False)
    _pages_back(eng)


@pytest.mark.parametrize("own", [dict(do_sample=True, temperature=1.0, top_k=0, min_p=0.002, seed=8, stream=2),
                                 dict(do_sample=True, temperature=1.3, top_k=0, epsilon_cutoff=3e-4, seed=9, stream=0),
                                 dict(do_sample=True, temperature=1.1, top_k=100, min_p=0.001, epsilon_cutoff=2e-4, seed=10, stream=5)])
def test_reported_alternatives_lie_in_the_restated_kept_set(phi, own):
    eng = phi[0].engine
    eng.set_sampling(False)
    emb = _embs((45,), seed=500)[0]
    s = _open(eng, emb, own, top_n=8)
    t = _open(eng, emb, GREEDY, top_n=-1)
    try:
        eng.prefill_batch([s], [emb])
        eng.decode_greedy_batch([s], NEW, None)
        ids = eng.seq_read(s, 0, NEW)
        _, top = eng.seq_read_logprobs(s, 0, len(ids), top=True)
        rows = [eng.prefill(t, emb, want_logits=True).cpu().numpy()]
        for i in ids[:-1]:                                                       # teacher-forced: the rows the selections saw
            rows.append(eng.decode_step_logits(t, i).cpu().numpy())
        for g, (row, i, alts) in enumerate(zip(rows, ids, top)):
            keep = WR.select(row, own, g)[2]
            assert keep[i], (g, i)
            assert len(alts) == min(8, int(keep.sum())) and all(keep[a] for a, _ in alts), (g, alts)
    finally:
        eng.seq_free(s)
        eng.seq_free(t)
    _pages_back(eng)


def test_generate_arguments_and_state(phi):
    model, sd, tok, geo, sp, tp = phi
    one = lambda **kw: model.generate(_samples("phi3.5", sp, tp, ["What is on the table?"]), max_new_tokens=NEW, **kw)
    greedy = one(do_sample=False)
    sampled = one(do_sample=True, temperature=1.5, top_k=0, seed=3)
    with pytest.raises(ValueError, match=r"`min_p` has to be a float in the \[0, 1\] interval, but is 2.0"):
        one(min_p=2.0)
    with pytest.raises(ValueError, match="`typical_p` has to be a float > 0 and < 1"):
        one(do_sample=True, typical_p=0.0)
    assert one(typical_p=0.9, do_sample=False) == greedy                         # the warpers are ignored without do_sample, as in HF
    warped = one(do_sample=True, temperature=1.5, top_k=0, seed=3, min_p=0.4, typical_p=0.5, epsilon_cutoff=1e-3, eta_cutoff=2e-3)
    assert warped != sampled
    assert warped == one(do_sample=True, temperature=1.5, top_k=0, seed=3, min_p=0.4, typical_p=0.5, epsilon_cutoff=1e-3, eta_cutoff=2e-3)
    # nothing carries over from one call to the next
    assert one(do_sample=True, temperature=1.5, top_k=0, seed=3) == sampled
    assert one(do_sample=False) == greedy
    assert model.engine.generate_ids(_embs((30,))[0], 4, None) == model.engine.generate_ids(_embs((30,))[0], 4, None)
    # beam-sample runs the same stages on the host (beam.warp_scores)
    b1 = one(do_sample=True, num_beams=2, temperature=1.5, top_k=0, seed=3, min_p=0.05, typical_p=0.95)
    assert b1 == one(do_sample=True, num_beams=2, temperature=1.5, top_k=0, seed=3, min_p=0.05, typical_p=0.95)
    _pages_back(model.engine)
