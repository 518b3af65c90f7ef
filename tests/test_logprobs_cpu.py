"""Per-token log-probabilities of generate() (grounded_video_llm_amd/logprobs.py, beam.py with_scores, the device kernels' definition restated in
torch) pinned against the installed transformers' generate(output_scores=True, return_dict_in_generate=True) + compute_transition_scores on a
tiny LlamaForCausalLM with inputs_embeds; the kwarg resolution and the scheduler's plumbing on the host.  No GPU."""
import math
import warnings

import pytest
import torch

from grounded_video_llm_amd import logits as LP
from grounded_video_llm_amd import logprobs as LPR
from grounded_video_llm_amd.beam import beam_search, warp_scores

from test_logits_processors_cpu import _fwd, _tiny, restate  # noqa: E402  (same tiny model, same processor restatement)


def kernel_lp(row: torch.Tensor, tok: int, inv_temp: float = 1.0, keep=None) -> float:
    """The selection kernels' definition (fp32): (s_tok - m) * invT - log(sum over the kept set of exp((s_i - m) * invT)); -inf entries add 0."""
    s = row.float()
    m = s.max()
    e = torch.exp((s - m) * inv_temp)
    if keep is not None:
        e = torch.where(keep, e, torch.zeros_like(e))
    return float((s[tok] - m) * inv_temp - torch.log(e.sum()))


def kernel_top(row: torch.Tensor, n: int, inv_temp: float = 1.0, keep=None):
    """The N best finite (kept) entries by value, lower id first on ties, with the kernel's log-probabilities; padded with (-1, -inf)."""
    s = row.float()
    ok = torch.isfinite(s) if keep is None else (torch.isfinite(s) & keep)
    cand = sorted(((-float(s[i]), i) for i in torch.nonzero(ok).flatten().tolist()))[:n]
    out = [(i, kernel_lp(s, i, inv_temp, keep)) for _, i in cand]
    return out + [(-1, -math.inf)] * (n - len(out))


def _gen(m, emb, **kw):
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        out = m.generate(inputs_embeds=emb, pad_token_id=0, output_scores=True, return_dict_in_generate=True, **kw)
        return out


def _transition(m, out, normalize, beams=False):
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        if beams:
            return m.compute_transition_scores(out.sequences, out.scores, out.beam_indices, normalize_logits=normalize)
        return m.compute_transition_scores(out.sequences, out.scores, normalize_logits=normalize)


@pytest.mark.parametrize("kw", [{}, dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(repetition_penalty=0.8, no_repeat_ngram_size=2)])
def test_greedy_logprobs_equal_hf_transition_scores(kw):
    m, E = _tiny()
    for seed in range(4):
        emb = torch.randn((1, 7, 32), generator=torch.Generator().manual_seed(seed)) * 2.0
        out = _gen(m, emb, do_sample=False, max_new_tokens=16, eos_token_id=None, **kw)
        ids = out.sequences[0].tolist()
        assert len(ids) == 16                                   # inputs_embeds: sequences hold the new ids only
        ref = _transition(m, out, True)[0].tolist()
        procs = LP.resolve(kw, None, emb.shape[1])
        for t, tok in enumerate(ids):
            row = restate(_fwd(m, E, emb, ids[:t]), ids[:t], *procs.args())
            assert int(torch.argmax(row)) == tok
            lp = kernel_lp(row, tok)
            assert abs(lp - ref[t]) < 1e-5, (seed, kw, t, lp, ref[t])
            # top-N: HF's processed row (out.scores) normalised, best 8 -- the top-1 entry is the chosen token with the same value
            hf = torch.log_softmax(out.scores[t][0].float(), dim=-1)
            top = kernel_top(row, 8)
            assert top[0] == (tok, lp)
            hv, hi = torch.topk(hf, 8)
            assert [i for i, _ in top] == hi.tolist()
            assert all(abs(v - float(w)) < 1e-5 for (_, v), w in zip(top, hv))


def test_sampling_logprobs_equal_hf_transition_scores():
    m, E = _tiny()
    T, K, TP = 0.7, 5, 0.9
    n_tok = 0
    for seed in range(4):
        emb = torch.randn((1, 7, 32), generator=torch.Generator().manual_seed(seed)) * 2.0
        torch.manual_seed(100 + seed)
        out = _gen(m, emb, do_sample=True, temperature=T, top_k=K, top_p=TP, max_new_tokens=12, eos_token_id=None)
        ids = out.sequences[0].tolist()
        ref = _transition(m, out, True)[0].tolist()
        for t, tok in enumerate(ids):                           # teacher-forced on HF's draws
            row = _fwd(m, E, emb, ids[:t])
            keep = torch.isfinite(warp_scores(row[None], T, K, TP, min_keep=1)[0])     # HF's kept set: temperature -> top-k -> top-p
            assert keep[tok]
            assert torch.equal(torch.isfinite(out.scores[t][0]), keep)
            lp = kernel_lp(row, tok, 1.0 / T, keep)
            assert abs(lp - ref[t]) < 1e-5, (seed, t, lp, ref[t])
            top = kernel_top(row, 8, 1.0 / T, keep)
            nk = int(keep.sum())
            assert [i for i, _ in top[nk:]] == [-1] * (8 - nk) if nk < 8 else True     # padding when fewer than N are kept
            n_tok += 1
    assert n_tok == 48


@pytest.mark.parametrize("length_penalty,kw", [(1.0, {}), (0.5, {}), (1.0, dict(no_repeat_ngram_size=2))])
def test_beam_scores_equal_hf(length_penalty, kw):
    m, E = _tiny()
    checked = 0
    for seed in range(4):
        emb = torch.randn((1, 7, 32), generator=torch.Generator().manual_seed(seed)) * 2.0
        free = _gen(m, emb, num_beams=3, do_sample=False, max_new_tokens=8, eos_token_id=None).sequences[0].tolist()
        for eos in (None, free[2]):
            out = _gen(m, emb, num_beams=3, do_sample=False, max_new_tokens=10, eos_token_id=eos, length_penalty=length_penalty, early_stopping=False, **kw)
            ref_ids = out.sequences[0].tolist()
            ref_tr = _transition(m, out, False, beams=True)[0].tolist()
            procs = LP.resolve(kw, eos, emb.shape[1])
            beams = [[] for _ in range(3)]

            def step(parents, toks):
                beams[:] = [beams[p_] + [t] for p_, t in zip(parents, toks)]
                return torch.stack([_fwd(m, E, emb, b) for b in beams])

            process = None
            if procs.active:
                def process(hists, lp):
                    return torch.stack([restate(lp[j], hists[j], *procs.args()) for j in range(lp.shape[0])])
            ids, score, tr = beam_search(step, _fwd(m, E, emb, []), 3, 10, eos, length_penalty, False, process=process, with_scores=True)
            beams[:] = [[] for _ in range(3)]
            assert beam_search(step, _fwd(m, E, emb, []), 3, 10, eos, length_penalty, False, process=process) == ids      # default: ids only
            while ref_ids and ref_ids[-1] == 0 and len(ref_ids) > len(ids):
                ref_ids, ref_tr = ref_ids[:-1], ref_tr[:-1]
            assert ids == ref_ids, (seed, eos, ids, ref_ids)
            assert len(tr) == len(ids)
            assert all(abs(a - b) < 1e-5 for a, b in zip(tr, ref_tr)), (tr, ref_tr)
            assert abs(score - float(out.sequences_scores[0])) < 1e-5, (score, float(out.sequences_scores[0]))
            assert abs(score - sum(tr) / len(tr) ** length_penalty) < 1e-4
            checked += 1
    assert checked == 8


def test_resolve_kwargs():
    o = LPR.resolve({})
    assert (o.return_dict, o.output_scores, o.top, o.top_n) == (False, False, None, -1)
    assert LPR.resolve(dict(output_scores=True)).top_n == -1                 # no dict: today's return value, nothing computed
    assert LPR.resolve(dict(return_dict_in_generate=True)).top_n == -1       # sequences only
    assert LPR.resolve(dict(return_dict_in_generate=True, output_scores=True)).top_n == 0
    assert LPR.resolve(dict(return_dict_in_generate=True, top_logprobs=5)).top_n == 5
    assert LPR.resolve(dict(return_dict_in_generate=True, output_scores=True, top_logprobs=0)).top_n == 0
    assert LPR.resolve(dict(return_dict_in_generate=True, output_scores=True, num_beams=3)).top_n == 0
    for bad in (-1, 9, 2.0, True, "3"):
        with pytest.raises(ValueError):
            LPR.resolve(dict(return_dict_in_generate=True, top_logprobs=bad))
    with pytest.raises(ValueError):
        LPR.resolve(dict(top_logprobs=2, num_beams=3))
    with pytest.raises(ValueError):
        LPR.resolve(dict(return_dict_in_generate=True, output_logits=True))
    LPR.resolve(dict(output_logits=True))                                   # without a dict HF ignores it too


def test_build_output():
    o = LPR.resolve(dict(return_dict_in_generate=True))
    r = LPR.build_output(["a"], [[5, 6]], o)
    assert r.sequences == [[5, 6]] and r.transition_scores is None and r.top_logprobs is None and r.sequences_scores is None
    o = LPR.resolve(dict(return_dict_in_generate=True, output_scores=True, top_logprobs=2))
    lps = [([-0.1, -0.2, -0.3], [[(5, -0.1), (7, -2.0)], [(6, -0.2)], [(1, -0.3), (2, -0.4)]])]
    r = LPR.build_output(["a"], [[5, 6]], o, lps)
    assert r.transition_scores == [[-0.1, -0.2]] and r.top_logprobs == [[[(5, -0.1), (7, -2.0)], [(6, -0.2)]]]
    assert LPR.top_pairs([3, 4, -1, -1], [-0.5, -1.5, -math.inf, -math.inf], 4) == [(3, -0.5), (4, -1.5)]
    assert LPR.top_pairs([3, 4, 9], [-0.5, -1.5, -2.0], 2) == [(3, -0.5), (4, -1.5)]


class _ScriptedEngine:
    """The ClipScheduler's engine surface on the CPU: sequence s emits 100 + s; its i-th log-probability is -(s + i / 100)."""

    def __init__(self):
        self.n, self.live, self.gen, self.lp = 0, set(), {}, {}

    def seq_alloc(self, cap):
        self.n += 1
        self.live.add(self.n)
        self.gen[self.n] = 0
        return self.n

    def seq_free(self, s):
        self.live.discard(s)

    def seq_set_logprobs(self, s, top_n):
        assert s in self.live
        self.lp[s] = top_n

    def prefill_batch(self, seqs, embeds):
        for s in seqs:
            self.gen[s] = 1

    def decode_steps(self, seqs, k):
        for s in seqs:
            self.gen[s] += k

    def seq_read(self, s, first, cap):
        return [100 + s] * max(0, min(self.gen[s] - first, cap))

    def seq_read_logprobs(self, s, first, cap, top=False):
        assert s in self.live                                    # read before the slot is freed
        n = max(0, min(self.gen[s] - first, cap))
        lp = [-(s + (first + i) / 100) for i in range(n)]
        return lp, ([[(100 + s, v)] * self.lp[s] for v in lp] if top else None)


def test_scheduler_logprobs_align_with_ids():
    from grounded_video_llm_amd.serve import ClipScheduler
    eng = _ScriptedEngine()
    sch = ClipScheduler(eng, eos_id=None, max_active=4, chunk=3)
    emb = torch.zeros((5, 4))
    a = sch.submit(emb, 7, logprobs=0)
    b = sch.submit(emb, 5)
    c = sch.submit(emb, 4, logprobs=3)
    out = sch.run()
    assert eng.lp == {1: 0, 3: 3}                                # request b keeps the engine's default: no call
    lp, top = sch.logprobs(a)
    assert len(lp) == len(out[a]) == 7 and top is None and lp == [-(1 + i / 100) for i in range(7)]
    lp, top = sch.logprobs(c)
    assert len(lp) == len(top) == len(out[c]) == 4 and all(len(t) == 3 for t in top)
    with pytest.raises(KeyError):
        sch.logprobs(b)
    for bad in (-1, 9, 1.5, True):
        with pytest.raises(ValueError):
            sch.submit(emb, 4, logprobs=bad)


def test_scheduler_logprobs_truncated_at_eos():
    from grounded_video_llm_amd.serve import ClipScheduler
    eng = _ScriptedEngine()
    sch = ClipScheduler(eng, eos_id=101, max_active=2, chunk=4)     # sequence 1 emits its eos (101) as its first id
    a = sch.submit(torch.zeros((3, 4)), 10, logprobs=0)
    out = sch.run()
    assert out[a] == [101] and sch.logprobs(a) == ([-1.0], None)


def test_new_symbols_are_exported():
    from grounded_video_llm_amd import lib
    for name in ("gvl_set_logprobs", "gvl_seq_set_logprobs", "gvl_seq_read_logprobs", "gvl_op_select_logprobs"):
        assert name in lib.EXPORTS
