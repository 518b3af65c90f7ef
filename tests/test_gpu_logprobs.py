"""-m gpu: log-probabilities of the selected tokens (argmax_kernel / sample_kernel with a logprob mode, csrc/gvl_pick.hip): the operator against fp64
log_softmax of the (warped) row, tokens unchanged by the mode, and every decode path (graph replay, batch, scheduler, shared prefix) giving the
same lists bit for bit, each entry matching the teacher-forced row."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gvl_oracle as O  # noqa: E402
from gpu_util import DEV  # noqa: E402
from grounded_video_llm_amd import engine as E, logits as LP, prompts as P, serve, synth  # noqa: E402
from grounded_video_llm_amd.model import LLAVA_NEXT_VIDEO, SyntheticTokenizer  # noqa: E402

from test_gpu_logits_processors import _build, _pages_back, _samples, restate  # noqa: E402  (same tiny geometries)

bf = torch.bfloat16


def tol(ref):
    return 1e-4 + 1e-5 * abs(ref)


def ref_logprobs(row, inv_temp=1.0, keep=None):
    """fp64 log-probabilities of a row under (s - m) * invT restricted to `keep` (None: every entry)."""
    s = torch.as_tensor(row, dtype=torch.float64)
    z = (s - s.max()) * inv_temp
    if keep is not None:
        z = torch.where(torch.as_tensor(keep), z, torch.full_like(z, -math.inf))
    return torch.log_softmax(z, dim=-1)


def ref_top(row, lp, n, keep=None):
    """fp64 top-n ids of the finite (kept) entries, by value descending, lower id first on ties; padded with -1."""
    s = torch.as_tensor(row, dtype=torch.float64)
    ok = torch.isfinite(s) & (torch.ones_like(s, dtype=torch.bool) if keep is None else torch.as_tensor(keep))
    idx = torch.nonzero(ok).flatten()
    order = sorted(zip((-s[idx]).tolist(), idx.tolist()))[:n]
    ids = [i for _, i in order]
    return ids + [-1] * (n - len(ids)), [float(lp[i]) for i in ids] + [-math.inf] * (n - len(ids))


def kept_set(x, T, top_k, top_p):
    """The sampler's kept set in fp64 (include/gvl.h): temperature -> top-k (ties with the k-th score kept) -> top-p, an entry kept iff the
    probability mass of STRICTLY larger entries is < top_p (HF's ascending cumsum splits a tie at the cut by position; this keeps the tie).
    Also returns whether an entry whose decision lies within fp32 rounding of the cut carries enough mass to move a value beyond the tolerance."""
    km = O.sample_keep_mask(x, T, top_k, None)
    if top_p is None or not 0.0 < top_p < 1.0:
        return km, False
    s = x.astype(np.float64) / T
    p = np.where(km, np.exp(s - s[km].max()), 0.0)
    p /= p.sum()
    desc = np.sort(p)[::-1]
    before = np.concatenate([[0.0], np.cumsum(desc)[:-1]])
    greater = before[np.searchsorted(-desc, -p, side="left")]     # mass of the strictly larger entries
    keep = km & (greater < top_p)
    return keep, bool(np.any(km & (np.abs(greater - top_p) < 1e-5) & (p > 2e-5)))


@pytest.fixture(scope="module")
def phi():
    m = _build("phi3.5")
    yield m
    m[0].engine.close()


def _rows(g, B, n):
    x = torch.randn((B, n), generator=g) * torch.tensor([0.5, 2.0, 4.0, 30.0])[torch.arange(B) % 4][:, None]     # wide ranges
    x[:, 5::97] = x[:, :1]                                          # ties with entry 0
    x[1::2, 7::13] = -math.inf                                      # -inf entries
    x[:, 11] = x.max(dim=1).values                                  # a tie at the maximum: the lower id wins
    x[:, 3] = x[:, 11]
    if B >= 3:
        x[2, :] = -math.inf; x[2, [17, 40, 41]] = torch.tensor([1.0, 0.5, 0.5])   # fewer finite entries than N: padding
    return x


@pytest.mark.parametrize("n", [32064, 128256])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_op_greedy_logprobs(phi, n, B):
    eng = phi[0].engine
    x = _rows(torch.Generator().manual_seed(n + B), B, n)
    top_n = [(8, 0, 8, 3, -1, 1)[b % 6] for b in range(B)]
    xd = x.to(DEV).contiguous()
    toks, lp, ti, tv = eng.op_select_logprobs(xd, top_n)
    off, _, _, _ = eng.op_select_logprobs(xd, -1)                  # the off instantiation: today's argmax
    assert torch.equal(toks, off)
    toks, lp, ti, tv = toks.cpu(), lp.cpu(), ti.cpu(), tv.cpu()
    for b in range(B):
        assert int(toks[b]) == int(torch.argmax(x[b]))
        if top_n[b] < 0:
            assert math.isnan(float(lp[b])) and int(ti[b, 0]) == -2
            continue
        r = ref_logprobs(x[b])
        assert abs(float(lp[b]) - float(r[toks[b]])) <= tol(float(r[toks[b]])), (n, B, b)
        if top_n[b] == 0:
            assert int(ti[b, 0]) == -2
            continue
        ids, vals = ref_top(x[b], r, top_n[b])
        assert ti[b, :top_n[b]].tolist() == ids, (n, B, b)
        assert ti[b, top_n[b]:].tolist() == [-1] * (8 - top_n[b])
        for j in range(8):
            want = vals[j] if j < top_n[b] else -math.inf
            got = float(tv[b, j])
            assert (got == want == -math.inf) or abs(got - want) <= tol(want), (n, B, b, j, got, want)
        assert ti[b, 0] == toks[b] and tv[b, 0] == lp[b]           # the greedy token is the top entry, with the same value


@pytest.mark.parametrize("n", [32064, 128256])
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("T,top_k,top_p", [(0.7, 5, None), (1.0, 0, 0.9), (0.2, 50, 0.9), (1.3, 50, 0.5), (1.0, 3, None)])
def test_op_sampling_logprobs(phi, n, B, T, top_k, top_p):
    eng = phi[0].engine
    x = _rows(torch.Generator().manual_seed(n + 7 * B + top_k), B, n)
    rng = np.random.default_rng(n + B)
    streams = [int(v) for v in rng.integers(0, 2 ** 31, B)]
    steps = [int(v) for v in rng.integers(0, 4000, B)]
    seed = 0x0123_4567_89AB_CDEF
    top_n = [(8, 0, 8, 5, -1, 2)[b % 6] for b in range(B)]
    xd = x.to(DEV).contiguous()
    toks, lp, ti, tv = eng.op_select_logprobs(xd, top_n, True, T, top_k, top_p, seed, streams, steps)
    assert torch.equal(toks, eng.op_sample(xd, T, top_k, top_p, seed, streams, steps))     # the same draw as gvl_op_sample
    toks, lp, ti, tv = toks.cpu(), lp.cpu(), ti.cpu(), tv.cpu()
    skipped = 0
    for b in range(B):
        if top_n[b] < 0:
            assert math.isnan(float(lp[b]))
            continue
        xb = x[b].numpy()
        keep, amb = kept_set(xb, T, top_k, top_p)
        if amb:
            skipped += 1
            continue
        r = ref_logprobs(xb, 1.0 / T, keep)
        t = int(toks[b])
        assert keep[t]
        assert abs(float(lp[b]) - float(r[t])) <= tol(float(r[t])), (n, B, b, float(lp[b]), float(r[t]))
        if top_n[b] == 0:
            continue
        ids, vals = ref_top(xb, r, top_n[b], keep)
        assert ti[b, :top_n[b]].tolist() == ids, (n, B, b)
        assert ti[b, top_n[b]:].tolist() == [-1] * (8 - top_n[b])
        for j in range(top_n[b]):
            got, want = float(tv[b, j]), vals[j]
            assert (got == want == -math.inf) or abs(got - want) <= tol(want), (n, B, b, j, got, want)
    assert skipped <= 2


def _embs():
    return [(torch.randn((S, 128), generator=torch.Generator().manual_seed(300 + S)) * 1.5).to(bf).to(DEV) for S in (37, 64, 90)]


def _teacher_forced(eng, emb, ids, procs=LP.OFF, inv_temp=1.0, keep_fn=None):
    """fp64 log-probability of every id of `ids` from the rows of a teacher-forced sequence (prefill row first), processors restated on the CPU."""
    seq = eng.seq_alloc(emb.shape[0] + len(ids) + 1)
    out = []
    try:
        eng.seq_set_processors(seq, *LP.OFF.args())
        eng.seq_set_logprobs(seq, -1)
        row = eng.prefill(seq, emb, want_logits=True)
        for i, t in enumerate(ids):
            s = restate(row, ids[:i], *procs.args())
            keep = keep_fn(s) if keep_fn else None
            out.append(float(ref_logprobs(s, inv_temp, keep)[t]))
            if i + 1 < len(ids):
                row = eng.decode_step_logits(seq, t)
    finally:
        eng.seq_free(seq)
    return out


@pytest.mark.parametrize("llm", ["phi3.5", "llama3"])
def test_decode_paths_give_the_same_logprobs(llm, phi):
    model, sd, tok, geo, sp, tp = phi if llm == "phi3.5" else _build(llm)
    eng = model.engine
    eos = tok.eos_token_id
    embs = _embs()
    procs = [LP.Processors(1.3, 2, 0, eos), LP.OFF, LP.Processors(1.0, 3, 0, eos)]
    eng.set_sampling(False)
    eng.set_logits_processors()
    plain = [eng.generate_ids(e, 20, None, processors=p) for e, p in zip(embs, procs)]
    single = [eng.generate_ids(e, 20, None, processors=p, logprobs=8) for e, p in zip(embs, procs)]
    assert [s_[0] for s_ in single] == plain                      # ids with logprobs on == off
    assert all(len(s_[1][0]) == 20 and len(s_[1][1]) == 20 for s_ in single)
    # decode_greedy over two calls (two captures of the step graph) == one call
    seq = eng.seq_alloc(embs[0].shape[0] + 21)
    try:
        eng.seq_set_processors(seq, *procs[0].args()); eng.seq_set_logprobs(seq, 8)
        eng.prefill(seq, embs[0])
        a = eng.decode_greedy(seq, 9, None)
        b = eng.decode_greedy(seq, 20, None)                     # continues the sequence; returns every id generated so far
        assert a == single[0][0][:9] and b == single[0][0]
        assert eng.seq_read_logprobs(seq, 0, 20, top=True) == single[0][1]
    finally:
        eng.seq_free(seq)
    # a batch of 3 (one row with logprobs off): the other rows' lists are bit-identical
    for graph in (1, 0):
        eng.debug_set("decode_graph", graph)
        seqs = [eng.seq_alloc(e.shape[0] + 21) for e in embs]
        try:
            for i, (s_, p) in enumerate(zip(seqs, procs)):
                eng.seq_set_processors(s_, *p.args()); eng.seq_set_logprobs(s_, -1 if i == 1 else 8)
            eng.prefill_batch(seqs, embs)
            assert eng.decode_greedy_batch(seqs, 20, None) == plain
            for i in (0, 2):
                assert eng.seq_read_logprobs(seqs[i], 0, 20, top=True) == single[i][1], (graph, i)
        finally:
            for s_ in seqs:
                eng.seq_free(s_)
    eng.debug_set("decode_graph", 1)
    # the scheduler (gvl_decode_steps, chunk 8)
    sch = serve.ClipScheduler(eng, None, max_active=3, chunk=8)
    rids = [sch.submit(embs[0], 20, repetition_penalty=1.3, no_repeat_ngram_size=2, logprobs=8), sch.submit(embs[1], 20, logprobs=8),
            sch.submit(embs[2], 20, no_repeat_ngram_size=3, logprobs=0)]
    out = sch.run()
    assert [out[r] for r in rids] == plain
    assert sch.logprobs(rids[0]) == single[0][1] and sch.logprobs(rids[1]) == single[1][1]
    assert sch.logprobs(rids[2]) == (single[2][1][0], None)
    # each entry against fp64 log_softmax of the teacher-forced row (the prefill's first token included)
    for i in range(3):
        want = _teacher_forced(eng, embs[i], plain[i], procs[i])
        got = single[i][1][0]
        assert all(abs(g - w) <= tol(w) for g, w in zip(got, want)), (llm, i)
        assert [t[0][0] for t in single[i][1][1]] == plain[i] and [t[0][1] for t in single[i][1][1]] == got
    # seeded sampling: ids on == off, each entry against the warped teacher-forced row
    T, K = 0.8, 20
    eng.set_sampling(True, T, K, None, 5)
    s_off = eng.generate_ids(embs[0], 16, None)
    eng.set_sampling(True, T, K, None, 5)
    s_on = eng.generate_ids(embs[0], 16, None, logprobs=4)
    assert s_on[0] == s_off
    eng.set_sampling(False)
    want = _teacher_forced(eng, embs[0], s_off, LP.OFF, 1.0 / T, lambda s: torch.as_tensor(O.sample_keep_mask(s.numpy(), T, K, None)))
    assert all(abs(g - w) <= tol(w) for g, w in zip(s_on[1][0], want))
    assert all(len(t) == 4 for t in s_on[1][1])
    _pages_back(eng)
    if llm != "phi3.5":
        eng.close()


def test_generate_surface(phi):
    model, sd, tok, geo, sp, tp = phi
    qs = ["When does the person open the door in the video?", "What is on the table?", "Describe the video in detail please."]
    kw = dict(do_sample=False, max_new_tokens=12)
    plain = [model.generate(_samples("phi3.5", sp, tp, [q]), **kw)[0] for q in qs]
    one = [model.generate(_samples("phi3.5", sp, tp, [q]), return_dict_in_generate=True, output_scores=True, top_logprobs=3, **kw) for q in qs]
    assert [o.texts[0] for o in one] == plain
    assert all(len(o.transition_scores[0]) == len(o.sequences[0]) == len(o.top_logprobs[0]) for o in one)
    only = model.generate(_samples("phi3.5", sp, tp, qs[:1]), return_dict_in_generate=True, **kw)
    assert only.sequences == one[0].sequences and only.transition_scores is None and only.top_logprobs is None
    bs3 = model.generate(_samples("phi3.5", sp, tp, qs), return_dict_in_generate=True, output_scores=True, top_logprobs=3, **kw)
    assert bs3.transition_scores == [o.transition_scores[0] for o in one] and bs3.top_logprobs == [o.top_logprobs[0] for o in one]
    sh = model.generate_shared(_samples("phi3.5", sp, tp, qs[:1]), [P.build_prompt("phi3.5", "grounding", q) for q in qs],
                               return_dict_in_generate=True, output_scores=True, top_logprobs=3, **kw)
    assert sh.texts == plain and sh.transition_scores == bs3.transition_scores and sh.top_logprobs == bs3.top_logprobs
    assert model.generate(_samples("phi3.5", sp, tp, qs[:1]), **kw) == plain[:1]        # nothing carries over
    with pytest.raises(ValueError):
        model.generate(_samples("phi3.5", sp, tp, qs[:1]), return_dict_in_generate=True, top_logprobs=9, **kw)
    with pytest.raises(ValueError):
        model.generate(_samples("phi3.5", sp, tp, qs[:1]), num_beams=3, top_logprobs=2, max_new_tokens=8)
    _pages_back(model.engine)


def test_beam_search_scores(phi):
    model, sd, tok, geo, sp, tp = phi
    s = _samples("phi3.5", sp, tp, ["When does the person open the door in the video?"])
    for lp in (1.0, 0.5):
        kw = dict(num_beams=3, do_sample=False, max_new_tokens=12, length_penalty=lp)
        plain = model.generate(s, **kw)
        out = model.generate(s, return_dict_in_generate=True, output_scores=True, **kw)
        assert out.texts == plain
        tr = out.transition_scores[0]
        assert len(tr) == len(out.sequences[0])
        assert abs(out.sequences_scores[0] - sum(tr) / len(tr) ** lp) < 1e-3
    _pages_back(model.engine)
