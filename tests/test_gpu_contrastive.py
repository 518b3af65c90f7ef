"""-m gpu: contrastive search inside the library (gvl_contrastive_search; csrc/gvl_contrastive.hip + gvl_contrastive.h), against tests/contrastive_ref.py [ext].
  1. the rank kernel, exact: entries in {0, +-1}, inverse norms 1/2 or 1/4 -- every cosine a multiple of 1/16 --, ties, a context of one row;
  2. the rank kernel against float64 at (k, n_ctx, D) up to (16, 8195, 3072): |pen - ref| <= 2 D 2^-24, |score - ref| <= alpha (that) + 1e-6, the selection on a seed
     whose float64 margin is >= 4 D 2^-24;
  3. invariance: a candidate's pen is bit-identical for k = 2 and k = 16 and with the bank truncated behind its arg-max row;
  4. the bank: append == gvl_op_rmsnorm bit for bit, inverse norms, the prefill's rows (last row x lm_head == the returned logits; == teacher-forced rows within the
     decode-vs-prefill bound), keep_hidden leaves the logits alone, untaught entries refuse;
  5. the search along its own trajectory: every step recomputed in float64 from a replay (teacher-forced second sequence, clones, batched candidate steps);
  6. alpha = 0 is greedy decoding, bit for bit;  7. processors and rules shape the candidate set;  8. ownership;  9. generate().
Tiny two-layer models: Phi at hidden 128 (the VALU decode path: candidate parts of 4 / 2 / 1), Phi at hidden 256 and Llama (GQA) at hidden 512 (skinny-MFMA path)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import contrastive_ref as R  # noqa: E402
from gpu_util import DEV, bf, llm_engine, tiny_geo  # noqa: E402
from grounded_video_llm_amd import grammar as GR, lib as L, logits as LP, synth  # noqa: E402

U = 2.0 ** -24
VOCAB = 640
MODELS = {"phi_valu": dict(llm="phi3.5", hidden=128, heads=4, kv_heads=4), "phi_mfma": dict(llm="phi3.5", hidden=256, heads=4, kv_heads=4),
          "llama_mfma": dict(llm="llama3", hidden=512, heads=4, kv_heads=2)}


def make_engine(name, **geo_kw):
    m = MODELS[name]
    kw = dict(llm=m["llm"], hidden=m["hidden"], inter=256, layers=2, heads=m["heads"], kv_heads=m["kv_heads"], vocab=VOCAB, max_seq=1024, max_prefill=768, kv_pages=96)
    if m["llm"] == "phi3.5":
        kw["rope_short"], kw["rope_long"] = synth.longrope_factors(m["hidden"] // m["heads"])
    else:
        kw.update(rope_theta=500000.0, rope_orig_max_pos=0)
    kw.update(geo_kw)
    geo = tiny_geo(**kw)
    W = synth.llm_weights("phi3" if m["llm"] == "phi3.5" else "llama", m["hidden"], 256, 2, m["heads"], m["kv_heads"], VOCAB, True, seed="t.cs." + name, device=DEV)
    return llm_engine(geo, W), geo, W


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(name):
        if name not in made:
            made[name] = make_engine(name)
            assert made[name][0].decode_group_info()["any_size"] == (0 if name == "phi_valu" else 1)      # the decode path the name promises
        return made[name]
    yield get
    for eng, _, _ in made.values():
        eng.close()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _free(eng):
    return eng.kv_info()["free_pages"]


def _prompt_ids(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(3, VOCAB, (n,), generator=g).tolist()


def _pen_bound(D):
    return 2.0 * D * U


# ---- 1. rank, exact --------------------------------------------------------------------------------------------------------------------------
def _pm1_rows(n, D, nnz, g):
    """rows with `nnz` entries of +-1 (nnz 4 or 16: norm 2 or 4), as bf16, with their exact inverse norms"""
    x = torch.zeros((n, D))
    for r in range(n):
        cols = torch.randperm(D, generator=g)[:nnz]
        x[r, cols] = (torch.randint(0, 2, (nnz,), generator=g) * 2 - 1).float()
    return x, torch.full((n,), 1.0 / float(np.sqrt(nnz)))


@pytest.mark.parametrize("k,n_ctx,D", [(2, 1, 64), (4, 1, 128), (4, 37, 128), (5, 200, 256), (16, 1000, 3072)])
def test_rank_is_exact_on_signed_unit_entries(engines, k, n_ctx, D):
    eng = engines("phi_valu")[0]
    g = torch.Generator().manual_seed(17 * k + n_ctx)
    parts = [_pm1_rows(n_ctx - n_ctx // 2, D, 4, g), _pm1_rows(n_ctx // 2, D, 16, g)]
    bank = torch.cat([p[0] for p in parts]); binv = torch.cat([p[1] for p in parts])
    cparts = [_pm1_rows(k - k // 2, D, 16, g), _pm1_rows(k // 2, D, 4, g)]
    cand = torch.cat([p[0] for p in cparts]); cinv = torch.cat([p[1] for p in cparts])
    cand[k - 1] = cand[0]; cinv[k - 1] = cinv[0]                       # a duplicate candidate: the same penalty
    if n_ctx > 3:
        bank[n_ctx - 2] = cand[1] * 1.0; binv[n_ctx - 2] = cinv[1]     # a context row equal to candidate 1: cosine exactly 1
    p = torch.tensor([2.0 ** -(1 + (i % 4)) for i in range(k)])
    p[k - 1] = p[0]                                                    # ... and the same p: equal scores, the lower rank must win
    cos = (cand.double() @ bank.double().T) * binv.double()[None, :] * cinv.double()[:, None]     # multiples of 1/16: exact in fp32 and float64
    assert torch.equal(cos * 16, torch.round(cos * 16))
    want_pen = cos.max(dim=1).values
    for alpha in (0.5, 0.25, 1.0, 0.0):
        want_score = (1.0 - alpha) * p.double() - alpha * want_pen       # dyadic: exact
        pen, score, sel = eng.op_contrastive_rank(bank.to(bf).to(DEV), binv.to(DEV), cand.to(bf).to(DEV), cinv.to(DEV), p.to(DEV), alpha)
        assert torch.equal(_bits(pen), _bits(want_pen.float())), (alpha, pen.cpu(), want_pen)
        assert torch.equal(_bits(score), _bits(want_score.float()))
        assert int(sel) == int(torch.argmax(want_score))                  # torch.argmax: the first maximum
        assert float(want_score[k - 1]) == float(want_score[0])
    if n_ctx > 3:
        assert float(want_pen[1]) == 1.0
    # every score equal: rank 0
    pen, score, sel = eng.op_contrastive_rank(bank[:1].to(bf).to(DEV), binv[:1].to(DEV), cand[:1].expand(k, D).contiguous().to(bf).to(DEV), cinv[:1].expand(k).contiguous().to(DEV),
                                              torch.full((k,), 0.25, device=DEV), 0.5)
    assert int(sel) == 0 and len(set(_bits(score).tolist())) == 1


def test_rank_refuses_what_it_cannot_serve(engines):
    eng = engines("phi_valu")[0]
    z = lambda *s: torch.zeros(s, device=DEV)
    for k, n, D, alpha, word in ((1, 4, 128, 0.5, "k"), (17, 4, 128, 0.5, "k"), (4, 4, 96, 0.5, "multiple of 64"), (4, 4, 128, 1.5, "alpha"), (4, 4, 128, float("nan"), "alpha")):
        with pytest.raises(L.GvlError, match=word) as e:
            eng.op_contrastive_rank(z(n, D).to(bf), z(n), z(k, D).to(bf), z(k), z(k), alpha)
        assert e.value.status == L.ERR_ARG


# ---- 2. rank against float64 -----------------------------------------------------------------------------------------------------------------
def _rank_case(eng, k, n_ctx, D, seed):
    """bank rows / candidates ~ N(0,1) through the library's own normalisation code (weight 1), one planted context row per candidate with cosine ~ 0.9"""
    g = torch.Generator(device=DEV).manual_seed(1000 * seed + 31 * k + n_ctx + D)
    cand_x = torch.randn((k, D), device=DEV, generator=g)
    bank_x = torch.randn((n_ctx, D), device=DEV, generator=g)
    rows = torch.randperm(n_ctx, device=DEV, generator=g)[:min(k, n_ctx)]
    for i, r in enumerate(rows.tolist()):
        bank_x[r] = 0.9 * cand_x[i] + (1.0 - 0.81) ** 0.5 * bank_x[r]
    ones = torch.ones((D,), device=DEV, dtype=bf)
    bank, binv = eng.op_hidden_bank_append(bank_x.to(bf), ones, 1e-5)
    cand, cinv = eng.op_hidden_bank_append(cand_x.to(bf), ones, 1e-5)
    p = torch.softmax(2.0 * torch.randn((k + 5,), device=DEV, generator=g), dim=-1).sort(descending=True).values[:k].contiguous()
    return bank, binv, cand, cinv, p


@pytest.mark.parametrize("k,n_ctx,D", [(2, 1, 128), (4, 63, 128), (5, 65, 3072), (16, 1025, 4096), (16, 8195, 3072)])
def test_rank_against_float64(engines, k, n_ctx, D):
    eng, alpha = engines("phi_valu")[0], 0.6
    bound = _pen_bound(D)
    chosen = None
    for seed in range(40):
        bank, binv, cand, cinv, p = _rank_case(eng, k, n_ctx, D, seed)
        ref_pen, _ = R.degeneration_penalty(cand.float().cpu().numpy(), bank.float().cpu().numpy())
        ref_sel, ref_score = R.select(p.cpu().numpy(), ref_pen, alpha)
        if R.margin(ref_score) >= 4.0 * D * U:
            chosen = seed
            break
    assert chosen is not None, "no seed among 40 separates the float64 best and second-best score by 4 D 2^-24"       # a precondition, asserted
    pen, score, sel = eng.op_contrastive_rank(bank, binv, cand, cinv, p, alpha)
    e_pen = float(np.abs(pen.cpu().numpy().astype(np.float64) - ref_pen).max())
    e_sc = float(np.abs(score.cpu().numpy().astype(np.float64) - ref_score).max())
    print(f"[contrastive] rank k {k} n_ctx {n_ctx} D {D} seed {chosen}: max |pen - ref| {e_pen:.3e} (bound {bound:.3e}), max |score - ref| {e_sc:.3e}, "
          f"max pen {float(ref_pen.max()):.3f}, margin {R.margin(ref_score):.3e}")
    if n_ctx >= k:
        assert float(ref_pen.min()) > 0.8                                  # the planted rows carry the maximum: it is not noise
    assert e_pen <= bound
    assert e_sc <= alpha * bound + 1e-6
    assert int(sel) == ref_sel
    # the inverse norms the cosines used, against float64: (D / 2 + 2) 2^-24 relative
    ref_inv = 1.0 / np.linalg.norm(bank.float().cpu().numpy().astype(np.float64), axis=1)
    assert float(np.abs(binv.cpu().numpy() / ref_inv - 1.0).max()) <= (D / 2 + 2) * U


# ---- 3. invariance ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ctx,D", [(300, 128), (1025, 3072)])
def test_a_candidates_penalty_does_not_depend_on_k_the_context_length_or_the_grid(engines, n_ctx, D):
    eng = engines("phi_valu")[0]
    bank, binv, cand, cinv, p = _rank_case(eng, 16, n_ctx, D, 3)
    pen16, _, _ = eng.op_contrastive_rank(bank, binv, cand, cinv, p, 0.6)
    for k in (2, 5, 8):
        penk, _, _ = eng.op_contrastive_rank(bank, binv, cand[:k].contiguous(), cinv[:k].contiguous(), p[:k].contiguous(), 0.6)
        assert torch.equal(_bits(penk), _bits(pen16[:k])), k
    # candidates 14 and 15 alone, as a k = 2 call: the same bits as at ranks 14 / 15 of the k = 16 call
    pen2, _, _ = eng.op_contrastive_rank(bank, binv, cand[14:].contiguous(), cinv[14:].contiguous(), p[14:].contiguous(), 0.6)
    assert torch.equal(_bits(pen2), _bits(pen16[14:]))
    _, arg = R.degeneration_penalty(cand.float().cpu().numpy(), bank.float().cpu().numpy())
    for i in (0, 7, 15):                                                    # the bank truncated behind candidate i's arg-max row: another grid, the same maximum
        n = int(arg[i]) + 1
        pent, _, _ = eng.op_contrastive_rank(bank[:n].contiguous(), binv[:n].contiguous(), cand, cinv, p, 0.6)
        assert int(_bits(pent)[i]) == int(_bits(pen16)[i]), (i, n)


# ---- 4. the bank -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [64, 128, 256, 2048, 3072, 4096, 8192])
def test_append_equals_rmsnorm_bit_for_bit(engines, cols):
    eng = engines("phi_valu")[0]
    g = torch.Generator(device=DEV).manual_seed(cols)
    n = 9                                                                  # three blocks of four rows, the last one partial
    wide = (torch.randn((n, cols + 64), device=DEV, generator=g) * 3.0).to(bf)
    w = (1.0 + 0.1 * torch.randn((cols,), device=DEV, generator=g)).to(bf)
    x = wide[:, :cols]                                                     # row pitch cols + 64: the decode step's rows are read in place
    rows, inv = eng.op_hidden_bank_append(x, w, 1e-5)
    want = eng.op_rmsnorm(x.contiguous(), w, 1e-5)
    assert torch.equal(_bits(rows), _bits(want))
    ref = 1.0 / np.linalg.norm(rows.float().cpu().numpy().astype(np.float64), axis=1)
    rel = float(np.abs(inv.cpu().numpy() / ref - 1.0).max())
    print(f"[contrastive] append cols {cols}: inverse norms within {rel:.3e} relative of float64 (bound {(cols / 2 + 2) * U:.3e})")
    assert rel <= (cols / 2 + 2) * U


S_BANK = 129                                                               # one page boundary crossed twice, not a multiple of any tile


def _keep_prefill(eng, emb, extra=2, grammar=None):
    seq = eng.seq_alloc(emb.shape[0] + extra)
    if grammar is not None:
        eng.seq_set_grammar(seq, grammar)
    eng.seq_keep_hidden(seq)
    return seq, eng.prefill(seq, emb, want_logits=True).clone()


@pytest.mark.parametrize("name", list(MODELS))
def test_bank_of_a_prefill(engines, name):
    eng, geo, W = engines(name)
    ids = _prompt_ids(S_BANK, 5)
    emb = eng.embed_ids(ids)
    free0 = _free(eng)
    seq, lg = _keep_prefill(eng, emb)
    plain = eng.seq_alloc(S_BANK + 2)
    try:
        rows, inv = eng.seq_read_hidden(seq, 0, S_BANK)
        # b. the last bank row through the lm_head, in float64, is the returned row of logits (1e-2 of the logit scale: the bf16 bound of gpu_util)
        h = rows[S_BANK - 1].float().cpu().double()
        ref = W["lm_head.weight"].float().cpu().double() @ h + W["lm_head.bias"].float().cpu().double()
        scale = float(ref.abs().max())
        e_head = float((lg.cpu().double() - ref).abs().max()) / scale
        wrong = float((lg.cpu().double() - (W["lm_head.weight"].float().cpu().double() @ rows[S_BANK - 2].float().cpu().double() + W["lm_head.bias"].float().cpu().double())).abs().max()) / scale
        print(f"[contrastive] {name}: lm_head(bank[S - 1]) vs the prefill's logits {e_head:.2e} of the logit scale (row S - 2 instead: {wrong:.2e})")
        assert e_head <= 1e-2 and wrong > 1e-2
        ref_inv = 1.0 / np.linalg.norm(rows.float().cpu().numpy().astype(np.float64), axis=1)
        assert float(np.abs(inv.cpu().numpy() / ref_inv - 1.0).max()) <= (geo.hidden / 2 + 2) * U
        # d. keep_hidden leaves the logits alone (the tail and the full last layer are the same rows), within the decode-vs-prefill bound
        lg_plain = eng.prefill(plain, emb, want_logits=True).clone()
        g = torch.Generator(device=DEV); g.manual_seed(9)
        flip = (torch.randint(0, 2, emb.shape, device=DEV, generator=g) * 2 - 1).float()
        pert_seq = eng.seq_alloc(S_BANK + 2)
        pert = eng.prefill(pert_seq, (emb.float() * (1.0 + flip * 2.0 ** -7)).to(bf), want_logits=True).clone()
        eng.seq_free(pert_seq)
        floor = float((pert - lg_plain).abs().max()) / scale
        e_keep = float((lg - lg_plain).abs().max()) / scale
        print(f"[contrastive] {name}: keep-hidden logits vs plain {e_keep:.2e}; 1-ulp input noise moves them by {floor:.2e}")
        assert e_keep < max(1e-2, 2.0 * floor)
        # c. the same rows from a prefill of one row and S - 1 teacher-forced steps
        tf = eng.seq_alloc(S_BANK + 2)
        try:
            eng.seq_keep_hidden(tf)
            eng.prefill(tf, emb[:1].contiguous())
            for t in ids[1:]:
                eng.decode_step_logits(tf, t)
            rows_tf, inv_tf = eng.seq_read_hidden(tf, 0, S_BANK)
        finally:
            eng.seq_free(tf)
        hs = float(rows.float().abs().max())
        e_rows = float((rows.float() - rows_tf.float()).abs().max()) / hs
        pk = eng.seq_alloc(S_BANK + 2)
        try:
            eng.seq_keep_hidden(pk)
            eng.prefill(pk, (emb.float() * (1.0 + flip * 2.0 ** -7)).to(bf))
            rows_p, _ = eng.seq_read_hidden(pk, 0, S_BANK)
        finally:
            eng.seq_free(pk)
        floor_rows = float((rows.float() - rows_p.float()).abs().max()) / hs
        print(f"[contrastive] {name}: bank of one prefill vs 1 row + {S_BANK - 1} teacher-forced steps {e_rows:.2e} of the hidden scale; 1-ulp input noise: {floor_rows:.2e}")
        assert e_rows < max(1e-2, 2.0 * floor_rows)
        assert torch.equal(_bits(rows[:1]), _bits(rows_tf[:1]))           # row 0 sees no other row: the same bits from both
        # e. entries that are not taught the bank refuse
        other = eng.seq_alloc(40)
        try:
            eng.seq_keep_hidden(other)
            for call in (lambda: eng.prefill_batch([other], [emb[:20].contiguous()]), lambda: eng.seq_fanout(seq, 2, S_BANK + 2, [0, 1], lg),
                         lambda: eng.decode_greedy(seq, 2, None), lambda: eng.beam_search(seq, lg, 2, 2, None), lambda: eng.seq_fork(seq, 64, 200)):
                with pytest.raises(L.GvlError, match="hidden") as e:
                    call()
                assert e.value.status == L.ERR_STATE
            with pytest.raises(L.GvlError, match="before the prefill") as e:
                eng.seq_keep_hidden(seq)
            assert e.value.status == L.ERR_STATE
            with pytest.raises(L.GvlError, match="keeps no hidden") as e:
                eng.seq_read_hidden(plain, 0, 1)
            assert e.value.status == L.ERR_STATE
            with pytest.raises(L.GvlError, match="rows") as e:
                eng.seq_read_hidden(seq, S_BANK, 1)
            assert e.value.status == L.ERR_ARG
        finally:
            eng.seq_free(other)
    finally:
        eng.seq_free(seq)
        eng.seq_free(plain)
    assert _free(eng) == free0


# ---- 5. the search along its own trajectory -----------------------------------------------------------------------------------------------------
S_PROMPT = 52                                                              # + 24 new tokens: the partial page is copied at every step, and the page boundary is crossed
MAX_NEW = 24


def _parts(eng, n):
    if eng.decode_group_info()["any_size"]:
        return [n]
    out = []
    while n:
        s = 4 if n >= 4 else (2 if n >= 2 else 1)
        out.append(s); n -= s
    return out


def _replay(eng, geo, emb, out_ids, trace, k, alpha, process=None):
    """Every step of `trace` recomputed in float64 from a second keep-hidden sequence that is teacher-forced along out_ids.  Returns the number of steps that fell
    under a margin clause.  process(ids_so_far, row fp32 [1, V] on the device) -> the processed row (None: none)."""
    D, bound = geo.hidden, _pen_bound(geo.hidden)
    rep, row = _keep_prefill(eng, emb, MAX_NEW + 2)
    under = 0
    try:
        for t, tok in enumerate(out_ids):
            n_ctx = emb.shape[0] + t
            if process is not None:
                row = process(out_ids[:t], row.clone().reshape(1, -1)).reshape(-1)
            # the row the search took its candidates from is, bit for bit, the replayed row behind op_logits_process (the raw row where nothing processes it)
            assert torch.equal(_bits(row.reshape(1, -1)), _bits(trace["rows"][t:t + 1])), t
            ids64, p64, p_all = R.top_k_candidates(row.cpu().numpy(), k + 1)
            # neighbours 1e-6 apart; two masked ids (p = 0 both) are ordered by id on both sides, so they count as separated
            sep = all(a - b >= 1e-6 or (a == 0.0 and b == 0.0) for a, b in zip(p64[:-1], p64[1:]))
            got_ids, got_p, got_pen, sel = trace["ids"][t], np.asarray(trace["p"][t]), np.asarray(trace["pen"][t]), trace["sel"][t]
            if sep:
                assert got_ids == ids64[:k].tolist(), (t, got_ids, ids64)
            else:
                assert sorted(got_ids) != [] and len(set(got_ids)) == k
            assert float(np.abs(got_p - p_all[got_ids]).max()) <= 1e-6, (t, got_p, p_all[got_ids])
            # the candidates, one step each, on clones of the replay sequence
            clones = [eng.seq_clone(rep, n_ctx + 2) for _ in range(k)]
            try:
                o = 0
                for n in _parts(eng, k):
                    eng.decode_step_logits_batch(clones[o:o + n], got_ids[o:o + n])
                    o += n
                cand = torch.cat([eng.seq_read_hidden(c, n_ctx, 1)[0] for c in clones])
            finally:
                for c in clones:
                    eng.seq_free(c)
            ctx_rows, _ = eng.seq_read_hidden(rep, 0, n_ctx)
            ref_pen, _ = R.degeneration_penalty(cand.float().cpu().numpy(), ctx_rows.float().cpu().numpy())
            assert float(np.abs(got_pen - ref_pen).max()) <= bound, (t, got_pen, ref_pen)
            ref_sel, ref_score = R.select(p_all[got_ids], ref_pen, alpha)
            ref_score = np.where(p_all[got_ids] > 0.0, ref_score, -np.inf)  # a masked id fills its place in the trace and is never chosen (gvl.h)
            ref_sel = int(np.argmax(ref_score))
            assert got_p[sel] > 0.0
            if R.margin(ref_score) >= 2.0 * (alpha * bound + 1e-6):
                assert sel == ref_sel, (t, sel, ref_sel, ref_score)
            if not sep or R.margin(ref_score) < 2.0 * (alpha * bound + 1e-6):
                under += 1
            assert tok == got_ids[sel]                                     # the output is what the trace selected
            row = eng.decode_step_logits(rep, tok).clone()
            committed, _ = eng.seq_read_hidden(rep, n_ctx, 1)
            assert torch.equal(_bits(committed), _bits(cand[sel:sel + 1]))  # teacher-forced alone == the winner's row in its candidate batch
            assert torch.equal(_bits(committed), _bits(trace["hidden"][t:t + 1]))   # ... == the row the search committed to its bank
    finally:
        eng.seq_free(rep)
    return under


@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("k,alpha", [(2, 0.3), (4, 0.6), (5, 0.6), (5, 0.3), (2, 0.6), (4, 0.3)])
def test_search_along_its_own_trajectory(engines, name, k, alpha):
    eng, geo, W = engines(name)
    emb = eng.embed_ids(_prompt_ids(S_PROMPT, 23))
    free0 = _free(eng)
    seq, first = _keep_prefill(eng, emb)
    try:
        ids, trace = eng.contrastive_search(seq, first, k, alpha, MAX_NEW, None, with_trace=True)
    finally:
        eng.seq_free(seq)
    assert len(ids) == MAX_NEW and len(trace["sel"]) == MAX_NEW and _free(eng) == free0
    under = _replay(eng, geo, emb, ids, trace, k, alpha)
    print(f"[contrastive] {name} k {k} alpha {alpha}: {under} of {MAX_NEW} steps under a margin clause; ranks chosen {trace['sel']}")
    assert under <= MAX_NEW // 10
    assert _free(eng) == free0


# ---- 6. alpha = 0 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_alpha_zero_is_greedy_decoding(engines, name):
    eng, geo, W = engines(name)
    emb = eng.embed_ids(_prompt_ids(S_PROMPT, 29))
    greedy = eng.generate_ids(emb, MAX_NEW, None)
    seq, first = _keep_prefill(eng, emb)
    try:
        for k in (2, 5):
            ids, trace = eng.contrastive_search(seq, first, k, 0.0, MAX_NEW, None, with_trace=True)
            assert ids == greedy and trace["sel"] == [0] * MAX_NEW
    finally:
        eng.seq_free(seq)


# ---- 7. processors in place --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["phi_valu", "llama_mfma"])
def test_processors_and_rules_shape_the_candidate_set(engines, name):
    eng, geo, W = engines(name)
    emb = eng.embed_ids(_prompt_ids(S_PROMPT, 23))
    k, alpha = 4, 0.6
    seq, first = _keep_prefill(eng, emb)
    try:
        plain, ptrace = eng.contrastive_search(seq, first, k, alpha, MAX_NEW, None, with_trace=True)
        banned = [plain[0], plain[3]]
        rules = LP.resolve_rules(dict(bad_words_ids=[[b] for b in banned]), None, MAX_NEW, VOCAB)
        rid = eng.rules_create(rules)
        try:
            procs = LP.Processors(1.0, 2, 0, 2)                             # no_repeat_ngram_size = 2
            ids, trace = eng.contrastive_search(seq, first, k, alpha, MAX_NEW, None, processors=procs, rules=rid, with_trace=True)
            assert all(b not in row for b in banned for row in trace["ids"]) and any(b in row for b in banned for row in ptrace["ids"])
            pairs = list(zip(ids[:-1], ids[1:]))
            assert len(set(pairs)) == len(pairs)                            # no 2-gram twice
            for t in range(1, len(ids)):                                    # ... because the id that would complete one is not even a candidate
                done = {b for a, b in zip(ids[:t - 1], ids[1:t]) if a == ids[t - 1]}
                assert not done & set(trace["ids"][t]), t
            process = lambda hist, row: eng.op_logits_process(row, [hist], 1.0, 2, 0, None, rules=rid)
            under = _replay(eng, geo, emb, ids, trace, k, alpha, process)   # every step's processed row == op_logits_process on the replayed row, bit for bit
            assert under <= MAX_NEW // 10
        finally:
            eng.rules_destroy(rid)
    finally:
        eng.seq_free(seq)


@pytest.mark.parametrize("name", ["phi_valu", "llama_mfma"])
def test_the_grounding_grammar_shapes_the_candidate_set(engines, name):
    """The sequence carries the grammar; the search feeds the mask the ids IT chose so far.  Every candidate that kept a probability is an id the grammar allows behind
    those ids (where fewer than k ids are allowed the remaining places hold masked ids with p = 0, never chosen), every processed row equals gvl_op_logits_process_ex
    on the replayed raw row bit for bit, and the answer is a sentence of the language."""
    from grounded_video_llm_amd.model import SyntheticTokenizer
    eng, geo, W = engines(name)
    tok = SyntheticTokenizer(VOCAB, 300)
    eos = tok.eos_token_id
    g = GR.grounding_grammar(tok, 300, eos, "interval")
    emb = eng.embed_ids(_prompt_ids(S_PROMPT, 23))
    k, alpha = 4, 0.6
    free0 = _free(eng)
    gid = eng.grammar_create(g)
    try:
        plain_seq, plain_first = _keep_prefill(eng, emb)
        seq, first = _keep_prefill(eng, emb, grammar=gid)
        try:
            plain, ptrace = eng.contrastive_search(plain_seq, plain_first, k, alpha, MAX_NEW, eos, with_trace=True)
            ids, trace = eng.contrastive_search(seq, first, k, alpha, MAX_NEW, eos, with_trace=True)
        finally:
            eng.seq_free(seq)
            eng.seq_free(plain_seq)
        masked_steps = shaped = 0
        for t, (cands, ps, sel) in enumerate(zip(trace["ids"], trace["p"], trace["sel"])):
            ok = g.allowed(ids[:t])
            if ok is None:
                continue
            masked_steps += 1
            assert all(ok[c] for c, p in zip(cands, ps) if p > 0.0), (t, cands, ps)
            assert all(p == 0.0 for c, p in zip(cands, ps) if not ok[c]), (t, cands, ps)
            assert ok[ids[t]] and ps[sel] > 0.0 and cands[sel] == ids[t]
            if t < len(ptrace["ids"]) and ids[:t] == plain[:t]:
                shaped += any(not ok[c] for c in ptrace["ids"][t])      # the unconstrained search had a candidate here that the grammar forbids
        assert masked_steps >= 1 and shaped >= 1 and ids != plain
        assert ids[-1] != eos or g.accepts(ids)
        assert g.walk(ids)[0]                                            # every id was allowed where it stands
        process = lambda hist, row: eng.op_logits_process(row, [hist], 1.0, 0, 0, None, grammar=gid)
        under = _replay(eng, geo, emb, ids, trace, k, alpha, process)
        print(f"[contrastive] {name} grammar: {len(ids)} ids {ids}, {masked_steps} masked steps, {under} steps under a margin clause")
        assert under <= len(ids) // 2                                    # the replay checked the choice itself on most steps
    finally:
        eng.grammar_destroy(gid)
    assert _free(eng) == free0


# ---- 8. ownership --------------------------------------------------------------------------------------------------------------------------------------
def test_the_pool_and_the_callers_sequence_survive_every_call(engines):
    eng, geo, W = engines("phi_valu")
    emb = eng.embed_ids(_prompt_ids(S_PROMPT, 31))
    free0 = _free(eng)
    seq, first = _keep_prefill(eng, emb, 12)
    plain, empty = eng.seq_alloc(S_PROMPT + 4), eng.seq_alloc(64)
    try:
        eng.prefill(plain, emb)
        eng.seq_keep_hidden(empty)
        held = _free(eng)
        a = eng.contrastive_search(seq, first, 4, 0.6, 10, None, with_trace=True)
        assert _free(eng) == held
        b = eng.contrastive_search(seq, first, 4, 0.6, 10, None, with_trace=True)      # not consumed: the same search again
        assert a[0] == b[0] and a[1]["sel"] == b[1]["sel"] and np.array_equal(np.float32(a[1]["pen"]), np.float32(b[1]["pen"])) and _free(eng) == held
        eos = a[0][0]
        assert eng.contrastive_search(seq, first, 4, 0.6, 10, eos) == [eos] and _free(eng) == held      # eos at step 0
        eos3 = a[0][3]
        cut = eng.contrastive_search(seq, first, 4, 0.6, 10, eos3)
        assert cut == a[0][:a[0].index(eos3) + 1] and _free(eng) == held

        def refused(status, match, *args, **kw):
            with pytest.raises(L.GvlError, match=match) as e:
                eng.contrastive_search(*args, **kw)
            assert e.value.status == status and _free(eng) == held
        refused(L.ERR_ARG, "top_k", seq, first, 1, 0.6, 8, None)
        refused(L.ERR_ARG, "top_k", seq, first, 17, 0.6, 8, None)
        refused(L.ERR_ARG, "penalty_alpha", seq, first, 4, 1.5, 8, None)
        refused(L.ERR_ARG, "max_new_tokens", seq, first, 4, 0.6, 0, None)
        refused(L.ERR_ARG, "rule set", seq, first, 4, 0.6, 8, None, rules=999)
        refused(L.ERR_ARG, "penalty", seq, first, 4, 0.6, 8, None, processors=LP.Processors(-1.0, 0, 0, 2))
        refused(L.ERR_ARG, "bad seq", 200, first, 4, 0.6, 8, None)
        refused(L.ERR_STATE, "not prefilled", empty, first, 4, 0.6, 8, None)
        refused(L.ERR_STATE, "keeps no hidden", plain, first, 4, 0.6, 8, None)
        # the pool too small for the clones: all or nothing
        hogs = []
        try:
            while _free(eng) >= 2:
                hogs.append(eng.seq_alloc(min(64 * (_free(eng) - 1), 1024)))
            low = _free(eng)
            with pytest.raises(L.GvlError) as e:
                eng.contrastive_search(seq, first, 8, 0.6, 10, None)
            assert e.value.status == L.ERR_OOM and _free(eng) == low
        finally:
            for h in hogs:
                eng.seq_free(h)
        assert _free(eng) == held
        assert eng.contrastive_search(seq, first, 4, 0.6, 10, None) == a[0]             # and the caller's sequence is where it was
        rows, _ = eng.seq_read_hidden(seq, 0, S_PROMPT)
        assert rows.shape[0] == S_PROMPT
    finally:
        for s in (seq, plain, empty):
            eng.seq_free(s)
    assert _free(eng) == free0


# ---- 9. generate() ---------------------------------------------------------------------------------------------------------------------------------------
def test_generate_surface():
    from test_gpu_beam import PROMPTS, _build, _samples
    model, sd, tok, geo, sp, tp = _build("phi3.5")
    try:
        eng = model.engine
        free0 = _free(eng)
        s = _samples("phi3.5", sp, tp, PROMPTS)
        kw = dict(penalty_alpha=0.6, top_k=4, max_new_tokens=16)
        got = model.generate(s, **kw)
        greedy = model.generate(s, max_new_tokens=16, do_sample=False)
        out = model.generate(s, return_dict_in_generate=True, output_scores=True, **kw)
        assert out.texts == got and len(got) == len(PROMPTS)
        import gvl_oracle as O
        from grounded_video_llm_amd import prompts as P
        feats = model.encode_images(_samples("phi3.5", sp, tp, ["x"]))[0]
        for q, seq_ids, ps, pens in zip(PROMPTS, out.sequences, out.transition_scores, out.degeneration_penalties):
            row = O.tokenizer_image_token(P.build_prompt("phi3.5", "grounding", q), tok, tok.bos_token_id)
            direct = model.contrastive_generate_ids(row, feats, 4, 0.6, 16, with_scores=True)
            assert direct[0] == seq_ids and direct[1] == ps and direct[2] == pens
            assert len(ps) == len(pens) == len(seq_ids) and all(0.0 <= x <= 1.0 for x in ps) and all(-1.0001 <= x <= 1.0001 for x in pens)
        differ = sum(a != b for a, b in zip(got, greedy))
        print(f"[contrastive] generate(penalty_alpha=0.6, top_k=4) differs from greedy on {differ} of {len(PROMPTS)} prompts")
        assert differ >= 1
        # a grammar constrains every chosen id
        g = GR.grounding_grammar(tok, 300, tok.eos_token_id, "interval")
        s1 = _samples("phi3.5", sp, tp, PROMPTS[:2])
        gout = model.generate(s1, grammar=g, return_dict_in_generate=True, **kw)
        for seq_ids in gout.sequences:
            if seq_ids and seq_ids[-1] == tok.eos_token_id:
                assert g.accepts(seq_ids)
        assert gout.sequences == model.generate(s1, grammar=g, return_dict_in_generate=True, **kw).sequences
        for bad, match in ((dict(guidance_scale=2.0, negative_prompts=["n"] * 2), "guidance_scale"), (dict(num_return_sequences=2), "num_return_sequences"),
                           (dict(top_logprobs=2, return_dict_in_generate=True), "top_logprobs")):
            with pytest.raises(ValueError, match=match):
                model.generate(s1, **dict(kw, **bad))
        with pytest.raises(ValueError, match="at most 16"):
            model.generate(s1, penalty_alpha=0.6, top_k=17, max_new_tokens=4)
        with pytest.raises(ValueError, match="penalty_alpha"):
            model.generate(s1, penalty_alpha=1.5, top_k=4, max_new_tokens=4)
        assert _free(eng) == free0
    finally:
        model.engine.close()
