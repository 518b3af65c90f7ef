"""-m gpu: diverse (group) beam search on the device (gvl_group_beam_search; the Hamming stage of csrc/gvl_logits.hip, beam_group_merge_kernel in csrc/gvl_pick.hip).
  1. the Hamming stage bit for bit against its torch restatement: alone, in front of a repetition penalty on the same token, behind a sequence_bias on the same token,
     with a grammar in the same launch,
  2. a group's candidates against float64, ties and -inf exactly, and the group's choice (eos in front, a done group),
  3. Engine.group_beam_search against beam.py's group_beam_search driven by the same kernels through its hooks (ids, scores, transition scores; at every step the tokens
     the device chose equal the host bookkeeping's),
  4. generate() on both beam_impls on prompts whose host-side candidates are >= 1e-4 apart; num_return_sequences = k; four different first tokens at (4, 4), lambda 1e4,
  5. lifetime: the KV pool and the caller's sequence after every call, error calls included; a group that finishes early gives its beams back at once."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV  # noqa: E402
from grounded_video_llm_amd import beam as B, grammar as GR, lib as L, logits as LP  # noqa: E402
from test_gpu_beam import PROMPTS, _bits, _build, _exact_order, _free_pages, _qualifying_case, _row_and_feats, _samples  # noqa: E402


@pytest.fixture(scope="module")
def phi():
    m = _build("phi3.5")
    yield m
    m[0].engine.close()


def f32(x):
    return torch.tensor(x, dtype=torch.float32)


# ---- 1. the Hamming stage ---------------------------------------------------------------------------------------------------------
def _rows(B_, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B_, n), generator=g) * 4.0
    x[:, 5::13] = float("-inf")
    x[:, 3::11] = -0.0
    return x


def _list(n):
    """one token once, one twice, one three times, an id >= n, an id on a -inf entry (5): 8 entries"""
    a, b, c = 1, 7, n - 1
    return [b, a, c, b, c, n + 5, 5, c], (a, b, c)


def _penalty(y, hist, p):
    """RepetitionPenaltyLogitsProcessor on one row: every distinct history token once"""
    y = y.clone()
    for t in set(hist):
        y[t] = y[t] * f32(p) if y[t] < 0 else y[t] / f32(p)
    return y


@pytest.mark.parametrize("n", [33, 1025, 640])
def test_hamming_stage_bit_for_bit(phi, n):
    model, sd, tok, geo, sp, tp = phi
    eng, eos = model.engine, tok.eos_token_id
    lst, (a, b, c) = _list(n)
    for B_ in (1, 2, 16):
        for lam in (0.1, 1.0, 5.0):
            x = _rows(B_, n, 100 * n + B_)
            none = ([[]] * B_, 1.0, 0, 0, None)
            # alone; an empty list changes nothing
            got = eng.op_logits_process(x.to(DEV).contiguous(), *none, hamming=(lst, lam)).cpu()
            ref = B.hamming_penalty(x, lst, lam)
            assert torch.equal(_bits(got), _bits(ref)), (n, B_, lam)
            assert got[0, c] == x[0, c] - f32(lam) * f32(3.0) and got[0, b] == x[0, b] - f32(lam) * f32(2.0) and got[0, 5] == float("-inf")
            assert torch.equal(_bits(eng.op_logits_process(x.to(DEV).contiguous(), *none, hamming=([], lam)).cpu()), _bits(x))
            # in front of a repetition penalty that hits the same tokens: (s - lambda c) * p, not s * p - lambda c
            hists = [[b, c, 2, b][:1 + r % 4] for r in range(B_)]
            got = eng.op_logits_process(x.to(DEV).contiguous(), hists, 1.3, 0, 0, None, hamming=(lst, lam)).cpu()
            ref = torch.stack([_penalty(B.hamming_penalty(x[r:r + 1], lst, lam)[0], hists[r], 1.3) for r in range(B_)])
            assert torch.equal(_bits(got), _bits(ref)), (n, B_, lam)
            wrong = torch.stack([B.hamming_penalty(_penalty(x[r], hists[r], 1.3)[None], lst, lam)[0] for r in range(B_)])
            assert not torch.equal(_bits(got), _bits(wrong))
    # behind a sequence_bias on the same token: (s + bias) - lambda c
    rid = eng.rules_create(LP.resolve_rules(dict(sequence_bias={(b,): 2.5, (a,): -0.3}), eos, 16, n))
    try:
        for B_ in (1, 16):
            x = _rows(B_, n, 7 * n + B_)
            got = eng.op_logits_process(x.to(DEV).contiguous(), [[]] * B_, 1.0, 0, 0, None, rules=rid, hamming=(lst, 0.7)).cpu()
            y = x.clone()
            y[:, b] = y[:, b] + f32(2.5)
            y[:, a] = y[:, a] + f32(-0.3)
            assert torch.equal(_bits(got), _bits(B.hamming_penalty(y, lst, 0.7))), (n, B_)
    finally:
        eng.rules_destroy(rid)


def test_hamming_stage_with_a_grammar_in_the_same_launch(phi):
    """no sequence_bias in the launch: the Hamming stage is the first to store, so the whole launch equals the launch without it on rows penalised in torch"""
    model, sd, tok, geo, sp, tp = phi
    eng, eos, n = model.engine, tok.eos_token_id, geo.vocab
    gid = eng.grammar_create(GR.grounding_grammar(tok, 300, eos, "interval"))
    try:
        for B_ in (1, 2, 16):
            x = _rows(B_, n, B_)
            hists = [[] for _ in range(B_)]
            args = (hists, 1.2, 0, 0, eos)
            plain = eng.op_logits_process(x.to(DEV).contiguous(), *args, grammar=gid).cpu()
            allowed = torch.isfinite(plain[0]).nonzero().flatten().tolist()
            assert allowed and len(allowed) < n                                              # the grammar masks something and leaves something
            lst = _list(n)[0] + [allowed[0]] * 2                                             # ... and the term lands on a token it allows, too
            got = eng.op_logits_process(x.to(DEV).contiguous(), *args, grammar=gid, hamming=(lst, 0.9)).cpu()
            ref = eng.op_logits_process(B.hamming_penalty(x, lst, 0.9).to(DEV).contiguous(), *args, grammar=gid).cpu()
            assert torch.equal(_bits(got), _bits(ref)), B_
            assert not torch.equal(_bits(got), _bits(plain))
    finally:
        eng.grammar_destroy(gid)


# ---- 2. a group's candidates and its choice -----------------------------------------------------------------------------------------
def _first_non_eos(idx, n, s, eos):
    out = [i % n for i in idx if eos is None or i % n != eos][:s]
    return out + [-1] * (s - len(out))


@pytest.mark.parametrize("s,n", [(1, 2), (1, 1025), (2, 1025), (4, 32064), (16, 4099)])
def test_group_candidates_against_float64_and_the_choice(phi, s, n):
    """the bounds of tests/test_gpu_beam.py::test_candidates_against_float64: idx exactly, |vals - ref| and |proc - ref| <= 1e-4, vals == fp32(proc + score) bit for bit"""
    eng = phi[0].engine
    case = _qualifying_case(s, n)
    assert case is not None
    seed, rows, scores, ref_lp, ref_t, top = case
    want = top.indices[:2 * s]
    for eos in (None, int(want[0]) % n, int(want[-1]) % n):                          # no eos; the BEST candidate is eos; the last one is
        vals, idx, proc, chosen = (x.cpu() for x in eng.op_beam_group(rows.to(DEV), scores, eos=eos, pad=3, logprobs=False))
        assert idx.tolist() == want.tolist()
        assert float((vals.double() - ref_t[want]).abs().max()) <= 1e-4 and float((proc.double() - ref_lp[want]).abs().max()) <= 1e-4
        assert torch.equal(_bits(vals), _bits(proc + scores[idx.long() // n]))
        assert chosen.tolist() == _first_non_eos(idx.tolist(), n, s, eos), (s, n, eos)
    # the same list from log-probability rows (what the search hands it), bit for bit
    normed = eng.op_beam_normalize(rows.to(DEV).clone())
    again = eng.op_beam_group(normed, scores, eos=None, pad=3, logprobs=True)
    assert all(torch.equal(_bits(x.cpu()), _bits(y)) for x, y in zip(again[:3], (vals, idx, proc)))
    # a done group: no candidates, the pad id (none: an id that counts nowhere)
    assert eng.op_beam_group(None, None, pad=3, done=True, s=s)[3].tolist() == [3] * s
    assert eng.op_beam_group(None, None, pad=None, done=True, s=s)[3].tolist() == [-1] * s


def test_group_ties_and_minus_infinity_are_exact(phi):
    eng = phi[0].engine
    for s, n in ((1, 2), (1, 700), (2, 5000), (4, 8), (16, 2048)):
        z, sc = torch.zeros((s, n)), torch.full((s,), -0.5)
        v, i, p, ch = eng.op_beam_group(z.to(DEV), sc, eos=1, pad=0, logprobs=True)
        assert i.cpu().tolist() == list(range(2 * s)) and ch.cpu().tolist() == _first_non_eos(list(range(2 * s)), n, s, 1)
    # the first step: ONE row, scores [0, -1e9, ...]: every candidate comes from the first beam
    g = torch.Generator().manual_seed(3)
    for s, n in ((1, 100), (2, 640), (4, 32064), (16, 1000)):
        perm = torch.randperm(n, generator=g)
        row = -0.01 * perm.float()
        sc = torch.full((s,), -1e9)
        sc[0] = 0.0
        v, i, p, ch = eng.op_beam_group(row.to(DEV), sc, eos=None, pad=0, logprobs=True, stride0=True)
        assert i.cpu().tolist() == torch.argsort(perm)[:2 * s].tolist() and ch.cpu().tolist() == torch.argsort(perm)[:s].tolist()
    # rows with fewer than 2s finite entries: the finite ones first, then the lowest flat indices among -inf; -inf candidates are chosen like any other non-eos one
    s, n = 2, 2000
    rows = torch.full((s, n), float("-inf"))
    rows[0, [1500, 3]] = torch.tensor([-1.0, -2.0])
    rows[1, 7] = -0.5
    sc = torch.tensor([-0.125, 0.0])
    v, i, p, ch = eng.op_beam_group(rows.to(DEV), sc, eos=None, pad=0, logprobs=True)
    assert i.cpu().tolist() == _exact_order(rows, sc, s) == [n + 7, 1500, 3, 0]
    rows = torch.full((s, n), float("-inf"))
    rows[:, 9] = 0.0
    v, i, p, ch = eng.op_beam_group(rows.to(DEV), sc, eos=9, pad=0, logprobs=True)
    assert i.cpu().tolist() == [n + 9, 9, 0, 1] and ch.cpu().tolist() == [0, 1]
    v, i, p, ch = eng.op_beam_group(rows.to(DEV), sc, eos=0, pad=0, logprobs=True)
    assert ch.cpu().tolist() == [9, 9]


# ---- 3. the search against beam.py over the same kernels ------------------------------------------------------------------------------
def _python_group_search(phi, row, feats, k, G, lam, max_new, hooks_of, eos, pad, length_penalty=1.0, early=False, num_return=1, first_grammar=None):
    """beam.py's group bookkeeping over this engine's sequences (model.beam_generate_ids' stepping); hooks_of(state) -> (process or None, candidates or None);
    state["raw"] = the raw logits rows of the step ([V] before the first step, then [k, V] with zero rows for finished groups).
    first_grammar: the prompt's row comes from a prefill of a sequence that carries this grammar, as the device path's caller hands it to the library (gvl_prefill returns
    the row its own token selection has already masked; gvl_beam_search has always started from that row) -- the beams themselves run with every option off."""
    model, sd, tok, geo, sp, tp = phi
    eng = model.engine
    gi = eng.decode_group_info()
    emb = eng.splice(row, feats)
    cap = min(emb.shape[0] + max_new + 1, geo.max_seq)
    beams, fresh = [eng.seq_alloc(cap)], []
    state = {"raw": None, "first": True}
    try:
        LP.apply_seq_options(eng, beams[0], LP.SeqOptions.OFF)
        first = eng.prefill(beams[0], emb, want_logits=True)
        if first_grammar is not None:
            tmp = eng.seq_alloc(emb.shape[0])
            try:
                LP.apply_seq_options(eng, tmp, dataclasses.replace(LP.SeqOptions.OFF, grammar=first_grammar))
                first = eng.prefill(tmp, emb, want_logits=True)
            finally:
                eng.seq_free(tmp)
        state["raw"] = first

        def step(parents, toks):
            keep, new = {}, [None] * len(parents)
            for j, p_ in enumerate(parents):
                if p_ is None:
                    continue
                if p_ in keep:
                    new[j] = eng.seq_clone(beams[p_], cap)
                    fresh.append(new[j])
                else:
                    keep[p_] = j
            for p_, j in keep.items():
                new[j] = beams[p_]
            losers = [s_ for p_, s_ in enumerate(beams) if p_ not in keep and s_ is not None]
            beams[:] = new
            del fresh[:]
            for s_ in losers:
                eng.seq_free(s_)
            live = [j for j, s_ in enumerate(beams) if s_ is not None]
            ls, lt = [beams[j] for j in live], [toks[j] for j in live]
            if len(ls) <= gi["max_group"] and (gi["any_size"] or len(ls) in (1, 2, 4)):
                got = eng.decode_step_logits_batch(ls, lt)
            else:
                got = torch.stack([eng.decode_step_logits(s_, t) for s_, t in zip(ls, lt)])
            raw = torch.zeros((len(parents), got.shape[-1]), dtype=torch.float32, device=got.device)
            raw[torch.as_tensor(live, device=got.device)] = got
            state["raw"], state["first"] = raw, False
            return raw
        process, candidates = hooks_of(state)
        return B.group_beam_search(step, first, k, G, lam, max_new, eos, length_penalty, early, process, True, candidates=candidates, num_return=num_return, pad_id=pad)
    finally:
        for s_ in set(x for x in list(beams) + fresh if x is not None):
            eng.seq_free(s_)


def _device_hooks(eng, k, G, eos, pad, procs, rid, gid, log):
    """the library's per-step chain, operator by operator: normalise every row once, then per group the processor launch (with the Hamming list the group launches left on
    the device), the group's candidates and its choice.  log: per step the k tokens on the device after the last group."""
    s = k // G
    active = procs is not None or rid is not None or gid is not None

    def hooks_of(state):
        st = {"last": G, "work": None, "cur": None}

        def begin(group):
            if group <= st["last"]:                              # a new step: every row normalised once, the finished groups' entries are the pad id
                raw, first = state["raw"], state["first"]
                norm = eng.op_beam_normalize((raw[None] if first else raw).clone().contiguous())
                st["work"] = [norm.clone() for _ in range(G)] if first else [norm[g * s:(g + 1) * s].contiguous() for g in range(G)]
                st["cur"] = torch.full((k,), -1 if pad is None else pad, dtype=torch.int32, device=DEV)
                log.append(None)
            st["last"] = group

        def process(histories, rows, group, prev_tokens, diversity_penalty):
            begin(group)
            assert st["cur"][:group * s].tolist() == list(prev_tokens)          # the device's choice of the earlier groups IS the host bookkeeping's
            if active or group > 0:
                hists = histories[:st["work"][group].shape[0]]
                kw = dict(rules=rid, grammar=gid)
                if group > 0:
                    kw["hamming"] = (st["cur"][:group * s].contiguous(), diversity_penalty)
                eng.op_logits_process(st["work"][group], hists, *(procs if procs is not None else LP.OFF).args(), **kw)
            return st["work"][group]

        def candidates(rows, scores, group):
            first = state["first"]
            v, i, p, ch = eng.op_beam_group(rows[0].contiguous() if first else rows, scores, eos=eos, pad=pad, logprobs=True, stride0=first)
            st["cur"][group * s:(group + 1) * s] = ch
            log[-1] = st["cur"].tolist()
            return v.tolist(), i.tolist(), p.tolist()
        return process, candidates
    return hooks_of


@pytest.mark.parametrize("k,G", [(2, 2), (4, 2), (4, 4), (6, 3)])
def test_library_group_search_equals_beam_py_over_the_same_kernels(phi, k, G):
    model, sd, tok, geo, sp, tp = phi
    eng, eos, pad = model.engine, tok.eos_token_id, tok.pad_token_id
    row, feats = _row_and_feats(phi)
    free0 = _free_pages(eng)
    plain = model.beam_generate_ids(row, feats, 3, 12, impl="device")
    rule_obj = LP.resolve_rules(dict(bad_words_ids=[[plain[0]]], sequence_bias={(plain[1],): 1.5}, suppress_tokens=[plain[2]]), eos, 10, geo.vocab)
    procs = LP.Processors(1.3, 2, 0, eos)
    rid = eng.rules_create(rule_obj)
    gid = eng.grammar_create(GR.grounding_grammar(tok, 300, eos, "interval"))
    try:
        for name, pr, ru, gr in (("plain", None, None, None), ("processors + rules", procs, rid, None), ("grammar", None, None, gid)):
            for lam, n_ret in ((1.0, 1), (0.3, k)):
                got = model.beam_generate_ids(row, feats, k, 10, processors=pr, rules=ru, grammar=gr, with_scores=True, impl="device", num_return=n_ret,
                                              num_beam_groups=G, diversity_penalty=lam)
                dev_tokens = eng.group_beam_tokens(k)
                log = []
                ref = _python_group_search(phi, row, feats, k, G, lam, 10, _device_hooks(eng, k, G, eos, pad, pr, ru, gr, log), eos, pad, num_return=n_ret,
                                           first_grammar=gr)
                for g_, r_ in zip([got] if n_ret == 1 else got, [ref] if n_ret == 1 else ref):
                    assert g_[0] == r_[0], (k, G, name, lam)
                    assert g_[1] == r_[1], (k, G, name, lam)
                    assert np.asarray(g_[2], dtype=np.float32).tobytes() == np.asarray(r_[2], dtype=np.float32).tobytes()
                    assert len(g_[2]) == len(g_[0]) <= 10
                assert dev_tokens == log and len(log) >= 1, (k, G, name, lam)       # at every step the device's current tokens are the bookkeeping's
                assert _free_pages(eng) == free0
    finally:
        eng.grammar_destroy(gid)
        eng.rules_destroy(rid)


# ---- 4. generate() ---------------------------------------------------------------------------------------------------------------------
def test_generate_on_both_beam_impls(phi):
    """the rule of tests/test_gpu_beam.py: a recording hook (torch top 2s + 1 on beam.py's own rows, per group) measures the host path's smallest gap between neighbouring
    candidates; where it is >= 1e-4 both implementations must pick the same candidates, hence the same ids.  At least half of the fixed prompt list must qualify."""
    model, sd, tok, geo, sp, tp = phi
    eng, eos, pad = model.engine, tok.eos_token_id, tok.pad_token_id
    k, G, lam, max_new, qualified = 4, 2, 1.0, 8, 0
    s = k // G
    free0 = _free_pages(eng)
    kw = dict(num_beams=k, num_beam_groups=G, diversity_penalty=lam, do_sample=False, max_new_tokens=max_new)
    for q in PROMPTS:
        row, feats = _row_and_feats(phi, q)
        gaps = []

        def hooks_of(state):
            def hook(rows, scores, group):
                top = torch.topk((rows + scores[:, None]).reshape(-1), 2 * s + 1, largest=True, sorted=True)
                gaps.append(float((top.values[:-1] - top.values[1:]).min()))
                idx = top.indices[:2 * s]
                return top.values[:2 * s].tolist(), idx.tolist(), rows.reshape(-1)[idx].tolist()
            return None, hook
        host = _python_group_search(phi, row, feats, k, G, lam, max_new, hooks_of, eos, pad)[0]
        assert host == model.beam_generate_ids(row, feats, k, max_new, num_beam_groups=G, diversity_penalty=lam)          # the hook is the host path
        print(f"[group beam] prompt {q!r}: smallest host-side candidate gap {min(gaps):.3e} over {len(gaps)} group steps")
        if min(gaps) < 1e-4:
            continue
        qualified += 1
        assert model.beam_generate_ids(row, feats, k, max_new, impl="device", num_beam_groups=G, diversity_penalty=lam) == host
        smp = _samples("phi3.5", sp, tp, [q])
        assert model.generate(smp, beam_impl="device", **kw) == model.generate(smp, **kw)
    print(f"[group beam] {qualified} of {len(PROMPTS)} prompts keep their candidates 1e-4 apart")
    assert 2 * qualified >= len(PROMPTS)
    # groups change the answer set: plain beams at the same k are what these arguments gave while they were ignored
    smp = _samples("phi3.5", sp, tp, [PROMPTS[0]])
    for impl in ("host", "device"):
        out = model.generate(smp, beam_impl=impl, return_dict_in_generate=True, output_scores=True, num_return_sequences=k, **kw)
        assert len(out.sequences) == k and all(a >= b for a, b in zip(out.sequences_scores, out.sequences_scores[1:]))
        plain = model.generate(smp, beam_impl=impl, return_dict_in_generate=True, output_scores=True, num_return_sequences=k, num_beams=k, max_new_tokens=max_new)
        assert [list(x) for x in out.sequences] != [list(x) for x in plain.sequences]
    assert _free_pages(eng) == free0


def test_one_beam_per_group_and_a_large_penalty_gives_different_first_tokens(phi):
    model, sd, tok, geo, sp, tp = phi
    eng = model.engine
    row, feats = _row_and_feats(phi)
    for impl in ("host", "device"):
        res = model.beam_generate_ids(row, feats, 4, 6, impl=impl, num_return=4, num_beam_groups=4, diversity_penalty=1e4)
        firsts = [r[0] for r in res]
        assert len(set(firsts)) == 4, (impl, res)
    emb = eng.splice(row, feats)
    seq = eng.seq_alloc(emb.shape[0] + 8)
    try:
        LP.apply_seq_options(eng, seq, LP.SeqOptions.OFF)
        first = eng.prefill(seq, emb, want_logits=True)
        eng.group_beam_search(seq, first, 4, 4, 1e4, 1, None, None)
        best = torch.topk(first, 4).indices.tolist()
        assert eng.group_beam_tokens(4) == [best]                                  # the G groups' first tokens: the G best tokens of the prompt's row, in order
    finally:
        eng.seq_free(seq)


# ---- 5. lifetime ---------------------------------------------------------------------------------------------------------------------
def test_the_pool_and_the_callers_sequence_survive_every_group_call(phi):
    model, sd, tok, geo, sp, tp = phi
    eng, eos, pad = model.engine, tok.eos_token_id, tok.pad_token_id
    row, feats = _row_and_feats(phi)
    emb = eng.splice(row, feats)
    free0 = _free_pages(eng)
    fresh = eng.seq_alloc(emb.shape[0] + 12)
    LP.apply_seq_options(eng, fresh, LP.SeqOptions.OFF)
    eng.prefill(fresh, emb)
    greedy = eng.decode_greedy(fresh, 10, None)
    eng.seq_free(fresh)
    seq = eng.seq_alloc(emb.shape[0] + 12)
    try:
        LP.apply_seq_options(eng, seq, LP.SeqOptions.OFF)
        first = eng.prefill(seq, emb, want_logits=True)
        held = _free_pages(eng)
        a = eng.group_beam_search(seq, first, 4, 2, 1.0, 10, eos, pad, with_scores=True, num_return=4)
        assert _free_pages(eng) == held
        assert eng.group_beam_search(seq, first, 4, 2, 1.0, 10, eos, pad, with_scores=True, num_return=4) == a and _free_pages(eng) == held
        assert eng.group_beam_search(seq, first, 4, 4, 0.5, 2, eos, pad) and _free_pages(eng) == held
        assert eng.group_beam_search(seq, first, 6, 3, 0.5, 3, eos, None, early_stopping=True) and _free_pages(eng) == held

        def refused(match, *args, **kw):
            with pytest.raises(L.GvlError, match=match) as e:
                eng.group_beam_search(*args, **kw)
            assert e.value.status == L.ERR_ARG and _free_pages(eng) == held
        refused("num_beam_groups", seq, first, 4, 3, 1.0, 8, eos, pad)
        refused("num_beam_groups", seq, first, 4, 1, 1.0, 8, eos, pad)
        refused("num_beam_groups", seq, first, 4, 8, 1.0, 8, eos, pad)
        refused("diversity_penalty", seq, first, 4, 2, 0.0, 8, eos, pad)
        refused("diversity_penalty", seq, first, 4, 2, -1.0, 8, eos, pad)
        refused("diversity_penalty", seq, first, 4, 2, float("nan"), 8, eos, pad)
        refused("num_beams", seq, first, 32, 2, 1.0, 8, eos, pad)
        refused("max_new_tokens", seq, first, 4, 2, 1.0, 0, eos, pad)
        refused("never", seq, first, 4, 2, 1.0, 8, eos, pad, 1.0, "never")
        refused("bad seq", 200, first, 4, 2, 1.0, 8, eos, pad)
        assert eng.decode_greedy(seq, 10, None) == greedy                          # the caller's sequence is where it was
    finally:
        eng.seq_free(seq)
    assert _free_pages(eng) == free0


def test_a_group_that_finishes_early_gives_its_beams_back_before_the_search_ends(phi):
    """k = 4, G = 2, no pad id (a finished group's tokens read -1).  A sequence_bias on eos makes hypotheses close early; the first setting in a fixed list at which one
    group is finished at some step while the other goes on is used (that there is one is asserted).  Behind the reorder of the step at which the group finished the
    search holds only the other group's s clones, and the pool holds more free pages than behind the step before."""
    model, sd, tok, geo, sp, tp = phi
    eng, eos = model.engine, tok.eos_token_id
    row, feats = _row_and_feats(phi)
    emb = eng.splice(row, feats)
    k, G, s = 4, 2, 2
    free0 = _free_pages(eng)
    seq = eng.seq_alloc(emb.shape[0] + 16)
    found = None
    try:
        LP.apply_seq_options(eng, seq, LP.SeqOptions.OFF)
        first = eng.prefill(seq, emb, want_logits=True)
        held = _free_pages(eng)
        for early in (False, True):
            for bias in (2.0, 3.0, 4.0, 5.0, 6.0, 8.0):
                rid = eng.rules_create(LP.resolve_rules(dict(sequence_bias={(eos,): bias}), eos, 12, geo.vocab))
                try:
                    eng.group_beam_search(seq, first, k, G, 1.0, 12, eos, None, early_stopping=early, rules=rid)
                finally:
                    eng.rules_destroy(rid)
                assert _free_pages(eng) == held
                toks, pool = eng.group_beam_tokens(k), eng.group_beam_pool()
                assert len(pool) == len(toks) - 1
                gone = [[all(t == -1 for t in st[g * s:(g + 1) * s]) for g in range(G)] for st in toks]
                steps = [i for i, d in enumerate(gone) if sum(d) == 1]
                if steps and found is None:
                    found = (early, bias, steps[0], toks, pool)
        assert found is not None, "no setting finishes one group while the other goes on"
        early, bias, t, toks, pool = found
        print(f"[group beam] early_stopping {early}, eos bias {bias}: one group is finished from step {t} of {len(toks)}; (clones, free pages) per step {pool}")
        # the group was finished by step t - 1's candidates: behind THAT step's reorder its beams are gone
        assert t >= 1 and pool[t - 1][0] == s and (t < 2 or pool[t - 2][0] == k)
        assert t < 2 or pool[t - 1][1] > pool[t - 2][1]                             # pages are taken when a sequence opens: the finished group's came back
        assert all(c == s for c, _ in pool[t - 1:])
    finally:
        eng.seq_free(seq)
    assert _free_pages(eng) == free0
