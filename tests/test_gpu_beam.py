"""-m gpu: beam search inside the library (gvl_beam_search; csrc/gvl_beam.h + beam_rows_kernel / beam_merge_kernel / beam_normalize_kernel).
  1. the candidate kernels against a float64 reference (seeds searched by the test so that the reference order is unambiguous),
  2. ties and -inf, exact: the order is (value descending, flat index ascending) over every entry,
  3. normalize + candidates on log-probabilities == candidates on raw logits, bit for bit; launches are reproducible,
  4. Engine.beam_search against beam.py's bookkeeping driven by the same kernels through the `candidates` hook (ids, score, transition scores),
  5. against the torch host path, on prompts whose host-side candidate gaps exceed the fp32 log-softmax difference,
  6. lifetime: the KV pool after every call (error calls included) and the caller's sequence after a search."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gvl_oracle as O  # noqa: E402
from gpu_util import DEV  # noqa: E402
from grounded_video_llm_amd import beam as B, engine as E, lib as L, logits as LP, prompts as P, synth  # noqa: E402
from grounded_video_llm_amd.model import LLAVA_NEXT_VIDEO, SyntheticTokenizer  # noqa: E402

QUESTION = "When does the person open the door in the video?"
PROMPTS = [QUESTION, "What is on the table?", "Describe the video in detail please.", "Who enters the room first?", "Where is the red cup at the end?",
           "How many people are there?", "What happens after the door closes?", "Is the window open?"]


def _build(llm):
    """The tiny geometry of tests/test_gpu_token_rules.py (hidden 128: the VALU-fallback decode path, groups of 1 / 2 / 4)."""
    hid, vocab = 128, 640
    short, long = synth.longrope_factors(32)
    geo = E.TowerGeometry(llm=llm, clip_hidden=64, clip_inter=128, clip_layers=3, clip_heads=4, iv2_dim=64, iv2_inter=128, iv2_depth=3,
                          iv2_heads=4, hidden=hid, inter=256, layers=2, heads=4, kv_heads=4, vocab=vocab, rope_short=short, rope_long=long,
                          rope_theta=10000.0, max_seq=2048, max_segs=6, kv_pages=40, max_prefill=1024)
    sd = {"vision_tower": synth.clip_weights(64, 128, 3, seed="gen.clip"),
          "video_encoder": synth.iv2_weights(64, 128, 3, 2, seed="gen.iv2"),
          "projectors": synth.projector_weights(llm, hid, 64, 64, seed="gen.proj"),
          "language_model": synth.llm_weights("phi3", hid, 256, 2, 4, geo.kv_heads, vocab, True, seed="gen.llm")}
    tok = SyntheticTokenizer(vocab, 300)
    model = LLAVA_NEXT_VIDEO(stage="sft", max_txt_len=64, num_frames=4, num_segs=2, num_temporal_tokens=300, lora=False, llm=llm,
                             geometry=geo, tokenizer=tok, state_dicts=sd, device=DEV)
    sp = synth.det_tensor("gen.sp", (1, 2, 3, 336, 336))
    tp = synth.det_tensor("gen.tp", (1, 4, 3, 224, 224))
    return model, sd, tok, geo, sp, tp


def _samples(llm, sp, tp, prompts):
    n = len(prompts)
    return {"prompts": [P.build_prompt(llm, "grounding", q) for q in prompts], "spatial_pixel_values": sp.expand(n, -1, -1, -1, -1).contiguous().to(DEV),
            "temporal_pixel_values": tp.expand(n, -1, -1, -1, -1).contiguous().to(DEV), "video_ids": ["synthetic"] * n}


@pytest.fixture(scope="module")
def phi():
    m = _build("phi3.5")
    yield m
    m[0].engine.close()


def _free_pages(eng):
    return eng.kv_info()["free_pages"]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- 1. candidates against float64 -----------------------------------------------------------------------------------------------
SHAPES = [(2, 4), (2, 1023), (3, 1025), (4, 32064), (16, 32064), (16, 128558)]


def _qualifying_case(k, n):
    """rows 3 N(0,1) fp32 [k, n], scores U[-3, 0] -- the first of at most 40 seeds whose float64 top 2k + 1 are pairwise >= 5e-4 apart and (k >= 3) come from >= 2 rows"""
    for seed in range(40):
        g = torch.Generator().manual_seed(1000 * k + 7919 * seed + n)
        rows = 3.0 * torch.randn((k, n), generator=g, dtype=torch.float32)
        scores = -3.0 * torch.rand((k,), generator=g, dtype=torch.float32)
        lp = torch.log_softmax(rows.double(), dim=-1)
        t = (lp + scores.double()[:, None]).reshape(-1)
        top = torch.topk(t, min(2 * k + 1, t.numel()), largest=True, sorted=True)
        gaps = top.values[:-1] - top.values[1:]
        if float(gaps.min()) >= 5e-4 and (k < 3 or len(set((top.indices // n).tolist())) >= 2):
            return seed, rows, scores, lp.reshape(-1), t, top
    return None


@pytest.mark.parametrize("k,n", SHAPES)
def test_candidates_against_float64(phi, k, n):
    """|vals - ref| and |proc - ref| <= 1e-4: >= 4 x the fp32 worst case for |t| < 64 -- 125 strided adds + the butterfly ~ 8e-6 relative on Z, plus expf / logf ulps,
    plus 3.8e-6 for the final rounding.  idx exactly; vals == fp32(proc + score[beam]) bit for bit."""
    eng = phi[0].engine
    case = _qualifying_case(k, n)
    assert case is not None, "no seed among 40 separates the float64 reference's top 2k + 1 by 5e-4"      # a precondition, asserted
    seed, rows, scores, ref_lp, ref_t, top = case
    vals, idx, proc = (x.cpu() for x in eng.op_beam_candidates(rows.to(DEV), scores, logprobs=False))
    want = top.indices[:2 * k]
    print(f"[beam] k {k} n {n} seed {seed}: max |vals - ref| {float((vals.double() - ref_t[want]).abs().max()):.3e}, "
          f"max |proc - ref| {float((proc.double() - ref_lp[want]).abs().max()):.3e}")
    assert idx.tolist() == want.tolist()
    assert float((vals.double() - ref_t[want]).abs().max()) <= 1e-4
    assert float((proc.double() - ref_lp[want]).abs().max()) <= 1e-4
    assert torch.equal(_bits(vals), _bits(proc + scores[idx.long() // n]))


# ---- 2. ties and -inf, exact -----------------------------------------------------------------------------------------------------
def _exact_order(rows, scores, k):
    """the first 2k of (fp32(rows + score) descending, flat index ascending): on log-probability rows the kernel's t is this very fp32 add"""
    t = (rows + scores[:, None]).reshape(-1).numpy()
    order = np.lexsort((np.arange(t.size), -t.astype(np.float64)))          # -inf stays -inf: sorts last, index ascending among equals
    return order[:2 * k].tolist()


def _cand_idx(eng, rows, scores, **kw):
    return eng.op_beam_candidates(rows.to(DEV).contiguous(), scores, **kw)[1].cpu().tolist()


def test_ties_and_minus_infinity_are_ordered_by_flat_index(phi):
    eng = phi[0].engine
    g = torch.Generator().manual_seed(5)
    # all-equal rows, equal scores: flat indices 0 .. 2k - 1 -- as log-probabilities and as raw logits (every lp = -log n)
    for k, n in ((4, 5000), (16, 2048), (2, 4)):
        z, s = torch.zeros((k, n)), torch.full((k,), -0.5)
        assert _cand_idx(eng, z, s, logprobs=True) == list(range(2 * k))
        assert _cand_idx(eng, z, s, logprobs=False) == list(range(2 * k))
    # a repeated maximum: the lower id first; the rest in the exact fp32 order
    k, n = 2, 3000
    rows = -1.0 - torch.rand((k, n), generator=g)
    rows[0, [2500, 17, 1999]] = 0.0
    rows[1, [2999, 0]] = 0.0
    s = torch.tensor([0.0, -0.25])
    got = _cand_idx(eng, rows, s, logprobs=True)
    assert got[:3] == [17, 1999, 2500] and got == _exact_order(rows, s, k)
    assert _cand_idx(eng, rows, torch.zeros(k), logprobs=True)[:4] == [17, 1999, 2500, n + 0]
    # two identical rows, equal scores: the lower beam first
    k, n = 3, 1025
    rows = -torch.rand((1, n), generator=g).expand(k, n).clone()
    rows[2] -= 10.0
    s = torch.zeros(k)
    got = _cand_idx(eng, rows, s, logprobs=True)
    assert got == _exact_order(rows, s, k) and [i // n for i in got] == [0, 1, 0, 1, 0, 1] and got[0] + n == got[1]
    # rows with fewer than 2k finite entries: the finite ones first, then the lowest flat indices among -inf
    k, n = 4, 2000
    rows = torch.full((k, n), float("-inf"))
    rows[0, [1500, 3]] = torch.tensor([-1.0, -2.0])
    rows[2, [7]] = -0.5
    rows[3, [1999, 0, 11]] = torch.tensor([-3.0, -4.0, -5.0])
    s = torch.tensor([-0.125, 0.0, -0.25, -0.5])
    got = _cand_idx(eng, rows, s, logprobs=True)
    assert got == _exact_order(rows, s, k) and got == [2 * n + 7, 1500, 3, 3 * n + 1999, 3 * n, 3 * n + 11, 0, 1]
    # ... and through the log-softmax (every row keeps a finite entry; a -inf logit is a -inf log-probability)
    rows[1, 5] = 0.0
    got = _cand_idx(eng, rows, s, logprobs=False)
    assert got[0] == n + 5 and sorted(got[1:7]) == sorted([2 * n + 7, 1500, 3, 3 * n + 1999, 3 * n, 3 * n + 11]) and got[7] == 0
    # the first step: ONE row for every beam, scores [0, -1e9, ...] -- beams 1 .. k - 1 collide at -1e9 entry for entry and lose to all of row 0
    for k, n in ((4, 32064), (16, 1000), (2, 4)):
        perm = torch.randperm(n, generator=g)
        row = -0.01 * perm.float()
        s = torch.full((k,), -1e9)
        s[0] = 0.0
        got = _cand_idx(eng, row, s, stride0=True)
        assert all(i < n for i in got) and got == torch.argsort(perm)[:2 * k].tolist()
        # the colliding beams among themselves: with every score at -1e9 the order is the flat index alone wherever fp32 cannot tell the entries apart
        got = _cand_idx(eng, torch.zeros(n), torch.full((k,), -1e9), stride0=True, logprobs=True)
        assert got == list(range(2 * k))


# ---- 3. normalize ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n", [(3, 1025), (4, 32064), (16, 128558)])
def test_normalize_then_logprob_candidates_equals_raw_candidates_bit_for_bit(phi, k, n):
    eng = phi[0].engine
    g = torch.Generator().manual_seed(k * n)
    rows = (3.0 * torch.randn((k, n), generator=g)).to(DEV)
    scores = -3.0 * torch.rand((k,), generator=g)
    a = eng.op_beam_candidates(rows, scores, logprobs=False)
    a2 = eng.op_beam_candidates(rows, scores, logprobs=False)
    normed = eng.op_beam_normalize(rows.clone())
    b = eng.op_beam_candidates(normed, scores, logprobs=True)
    for x, y, z in zip(a, a2, b):
        assert torch.equal(_bits(x), _bits(y)) and torch.equal(_bits(x), _bits(z))
    assert torch.equal(_bits(eng.op_beam_normalize(rows.clone())), _bits(normed))
    assert float((normed.double().exp().sum(-1) - 1.0).abs().max()) < 1e-4


# ---- 4. Engine.beam_search against beam.py over the same kernels -------------------------------------------------------------------
def _row_and_feats(phi, question=QUESTION):
    model, sd, tok, geo, sp, tp = phi
    row = O.tokenizer_image_token(P.build_prompt("phi3.5", "grounding", question), tok, tok.bos_token_id)
    return row, model.encode_images(_samples("phi3.5", sp, tp, ["x"]))[0]


def _python_search(phi, row, feats, k, max_new, hook_of, length_penalty=1.0, early=False):
    """beam.py's bookkeeping over this engine's sequences (model.beam_generate_ids' clone / free stepping), candidates from hook_of(state): state["raw"] = the raw
    logits rows of the step (one row [V] before the first step), state["hist"] = the beams' generated ids"""
    model, sd, tok, geo, sp, tp = phi
    eng, eos = model.engine, tok.eos_token_id
    gi = eng.decode_group_info()
    emb = eng.splice(row, feats)
    cap = min(emb.shape[0] + max_new + 1, geo.max_seq)
    beams, fresh = [eng.seq_alloc(cap)], []
    state = {"raw": None, "hist": [[] for _ in range(k)], "first": True}
    try:
        LP.apply_seq_options(eng, beams[0], LP.SeqOptions.OFF)
        first = eng.prefill(beams[0], emb, want_logits=True)
        state["raw"] = first

        def step(parents, toks):
            keep, new = {}, [None] * len(parents)
            for j, p_ in enumerate(parents):
                if p_ in keep:
                    new[j] = eng.seq_clone(beams[p_], cap)
                    fresh.append(new[j])
                else:
                    keep[p_] = j
            for p_, j in keep.items():
                new[j] = beams[p_]
            losers = [s_ for p_, s_ in enumerate(beams) if p_ not in keep]
            beams[:] = new
            del fresh[:]
            for s_ in losers:
                eng.seq_free(s_)
            state["hist"] = [state["hist"][p_] + [t] for p_, t in zip(parents, toks)]
            state["first"] = False
            if len(beams) <= gi["max_group"] and (gi["any_size"] or len(beams) in (1, 2, 4)):
                state["raw"] = eng.decode_step_logits_batch(beams, toks)
            else:
                state["raw"] = torch.stack([eng.decode_step_logits(s_, t) for s_, t in zip(beams, toks)])
            return state["raw"]
        return B.beam_search(step, first, k, max_new, eos, length_penalty, early, None, None, True, candidates=hook_of(state))
    finally:
        for s_ in set(x for x in list(beams) + fresh if x is not None):
            eng.seq_free(s_)


def _device_hook(eng, k, procs=None, rid=None):
    """the library's per-step pipeline, operator by operator: (normalize -> processors / rules ->) candidates"""
    def hook_of(state):
        def hook(rows, scores):
            raw, first = state["raw"], state["first"]
            if procs is None and rid is None:
                v, i, p = eng.op_beam_candidates(raw.contiguous(), scores, logprobs=False, stride0=first)
            else:
                work = eng.op_beam_normalize((raw[None] if first else raw).clone().contiguous())
                hists = state["hist"][:work.shape[0]]
                work = eng.op_logits_process(work, hists, *(procs if procs is not None else LP.OFF).args(), **({} if rid is None else {"rules": rid}))
                v, i, p = eng.op_beam_candidates(work[0].contiguous() if first else work, scores, logprobs=True, stride0=first)
            return v.tolist(), i.tolist(), p.tolist()
        return hook
    return hook_of


@pytest.mark.parametrize("k", [2, 3, 4])
def test_library_search_equals_beam_py_over_the_same_kernels(phi, k):
    model, sd, tok, geo, sp, tp = phi
    eng, eos = model.engine, tok.eos_token_id
    row, feats = _row_and_feats(phi)
    free0 = _free_pages(eng)
    plain16 = model.beam_generate_ids(row, feats, 3, 16, impl="device")
    assert len(plain16) >= 4
    rule_obj = LP.resolve_rules(dict(bad_words_ids=[[plain16[0]], plain16[2:4]], suppress_tokens=[plain16[1]], forced_eos_token_id=eos), eos, 16, geo.vocab)
    procs = LP.Processors(1.0, 2, 0, eos)
    rid = eng.rules_create(rule_obj)
    try:
        for max_new in (12, 16):
            for pr, ru in ((None, None), (procs, rid)):
                got = model.beam_generate_ids(row, feats, k, max_new, processors=pr, rules=ru, with_scores=True, impl="device")
                ref = _python_search(phi, row, feats, k, max_new, _device_hook(eng, k, pr, ru))
                assert got[0] == ref[0], (k, max_new, pr is not None)
                assert abs(got[1] - ref[1]) <= 1e-12 * abs(ref[1])
                assert np.asarray(got[2], dtype=np.float32).tobytes() == np.asarray(ref[2], dtype=np.float32).tobytes()
                assert len(got[2]) == len(got[0]) <= max_new
                if pr is not None:
                    assert plain16[0] not in got[0] and plain16[1] not in got[0]
                assert _free_pages(eng) == free0
    finally:
        eng.rules_destroy(rid)


# ---- 5. against the torch host path ------------------------------------------------------------------------------------------------
def test_device_search_equals_the_host_path_where_the_candidates_are_separated(phi):
    """A recording hook (torch top 2k + 1 on beam.py's own rows) measures the host path's smallest gap between neighbouring candidates over all steps; where it is >= 1e-4
    (>= 10 x the fp32 log-softmax difference at |score| < 64) both implementations must pick the same candidates, hence the same ids."""
    model, sd, tok, geo, sp, tp = phi
    eng = model.engine
    k, max_new, qualified = 3, 12, 0
    free0 = _free_pages(eng)
    for q in PROMPTS:
        row, feats = _row_and_feats(phi, q)
        gaps = []

        def hook_of(state):
            def hook(rows, scores):
                t = rows + scores[:, None]
                top = torch.topk(t.reshape(-1), 2 * k + 1, largest=True, sorted=True)
                gaps.append(float((top.values[:-1] - top.values[1:]).min()))
                idx = top.indices[:2 * k]
                return top.values[:2 * k].tolist(), idx.tolist(), rows.reshape(-1)[idx].tolist()
            return hook
        host = _python_search(phi, row, feats, k, max_new, hook_of)[0]
        assert host == model.beam_generate_ids(row, feats, k, max_new)          # the hook is the host path
        print(f"[beam] prompt {q!r}: smallest host-side candidate gap {min(gaps):.3e} over {len(gaps)} steps")
        if min(gaps) < 1e-4:
            continue
        qualified += 1
        assert model.beam_generate_ids(row, feats, k, max_new, impl="device") == host
        s = _samples("phi3.5", sp, tp, [q])
        kw = dict(num_beams=k, do_sample=False, max_new_tokens=max_new)
        assert model.generate(s, beam_impl="device", **kw) == model.generate(s, **kw)
    assert qualified >= 2, f"only {qualified} of {len(PROMPTS)} prompts keep their candidates 1e-4 apart"
    s = _samples("phi3.5", sp, tp, [QUESTION])
    out = model.generate(s, num_beams=k, do_sample=False, max_new_tokens=max_new, beam_impl="device", return_dict_in_generate=True, output_scores=True)
    assert len(out.sequences[0]) <= max_new and out.sequences_scores is not None
    with pytest.raises(ValueError, match="beam_impl"):
        model.generate(s, num_beams=k, do_sample=True, max_new_tokens=4, beam_impl="device")
    with pytest.raises(ValueError, match="beam_impl"):
        model.generate(s, num_beams=k, max_new_tokens=4, beam_impl="gpu")
    assert _free_pages(eng) == free0


# ---- 6. lifetime -------------------------------------------------------------------------------------------------------------------
def test_the_pool_and_the_callers_sequence_survive_every_call(phi):
    model, sd, tok, geo, sp, tp = phi
    eng, eos = model.engine, tok.eos_token_id
    row, feats = _row_and_feats(phi)
    emb = eng.splice(row, feats)
    free0 = _free_pages(eng)
    fresh = eng.seq_alloc(emb.shape[0] + 12)
    LP.apply_seq_options(eng, fresh, LP.SeqOptions.OFF)
    eng.prefill(fresh, emb)
    greedy = eng.decode_greedy(fresh, 10, None)
    eng.seq_free(fresh)

    seq = eng.seq_alloc(emb.shape[0] + 12)
    empty = eng.seq_alloc(64)
    try:
        LP.apply_seq_options(eng, seq, LP.SeqOptions.OFF)
        first = eng.prefill(seq, emb, want_logits=True)
        held = _free_pages(eng)
        a = eng.beam_search(seq, first, 3, 12, eos, with_scores=True)
        assert _free_pages(eng) == held
        b = eng.beam_search(seq, first, 3, 12, eos, with_scores=True)           # the sequence was not consumed: the same search again
        assert a == b and _free_pages(eng) == held
        assert eng.beam_search(seq, first, 4, 1, eos) and _free_pages(eng) == held

        def refused(status, match, *a, **kw):
            with pytest.raises(L.GvlError, match=match) as e:
                eng.beam_search(*a, **kw)
            assert e.value.status == status and _free_pages(eng) == held
        refused(L.ERR_ARG, "num_beams", seq, first, 1, 8, eos)
        refused(L.ERR_ARG, "num_beams", seq, first, 17, 8, eos)
        refused(L.ERR_ARG, "max_new_tokens", seq, first, 3, 0, eos)
        refused(L.ERR_ARG, "never", seq, first, 3, 8, eos, 1.0, "never")
        refused(L.ERR_ARG, "rule set", seq, first, 3, 8, eos, rules=999)
        refused(L.ERR_STATE, "not prefilled", empty, first, 3, 8, eos)
        refused(L.ERR_ARG, "bad seq", 200, first, 3, 8, eos)
        refused(L.ERR_ARG, "penalty", seq, first, 3, 8, eos, processors=LP.Processors(-1.0, 0, 0, eos))
        # cap < max_new_tokens: only the C ABI can say that
        prm = L.GvlBeamParams(3, 8, eos, 1.0, 0, 1.0, 0, 0, -1, -1)
        ids, n = (C.c_int32 * 8)(), C.c_int(0)
        rc = eng.lib.gvl_beam_search(eng.ctx, seq, C.c_void_p(first.data_ptr()), C.byref(prm), ids, 7, C.byref(n), None, None, eng.stream)
        assert rc == L.ERR_ARG and b"cap" in eng.lib.gvl_last_error(eng.ctx) and _free_pages(eng) == held
        # "never" is legal without a positive penalty
        assert eng.beam_search(seq, first, 3, 8, eos, 0.0, "never") and _free_pages(eng) == held
        # the caller's sequence is where it was: its greedy continuation is the fresh prefill's
        assert eng.decode_greedy(seq, 10, None) == greedy
    finally:
        eng.seq_free(seq)
        eng.seq_free(empty)
    assert _free_pages(eng) == free0
