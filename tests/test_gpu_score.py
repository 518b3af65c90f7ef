"""-m gpu: teacher-forced scoring (gvl_score_extend_varlen / Engine.score_extend_batch / LLAVA_NEXT_VIDEO.score) on the tiny 2-layer models of
test_gpu_logits_processors._build (Phi MHA with LongRoPE, Llama GQA).
  * bit identities: a member's lp / rank / top lists do not depend on the group (1, 3, 8 members), the launch form (varlen_extend 1 / 0), the 64-row chunk of the
    score tail it falls into, or on whether its first 128 rows came from a cached prefix or from the call itself;
  * state: every member ends as after prefill_extend_batch of the same rows (last logits, the next greedy ids), with the attention launches the plan names;
  * values: against the fp32 oracle's full-row logits (float64 log-softmax), the reference's training-loss goldens, and gvl_prefill of truncated prompts;
  * the Python surface: model.score of k pairs == k calls of one pair == the same without prefix sharing; generate_shared unchanged by the shared prefix rule's move."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import gvl_oracle as O  # noqa: E402
import prefill_plan as PP  # noqa: E402
from conftest import load_golden  # noqa: E402
from gpu_util import DEV, bf, llm_engine, tiny_geo  # noqa: E402
from grounded_video_llm_amd import prompts as P, synth  # noqa: E402
from grounded_video_llm_amd.lib import GvlError  # noqa: E402

from test_gpu_llm import _ocfg, _phi_geo  # noqa: E402
from test_gpu_logits_processors import _build, _pages_back  # noqa: E402

NEW = 6                                                  # greedy ids compared after a call
MEMBERS = [(128, 70), (0, 1), (64, 37), (0, 63), (64, 64), (128, 1), (0, 65), (64, 13)]     # (cached prefix, new rows): tails 1 .. 70 around the 64-token page
DENSE = [(0, 40), (64, 40), (128, 40)]                   # every row scored: 120 scored rows, the 64-row chunks of the score tail cut through the second member


class Ctx:
    def __init__(self, llm):
        self.llm = llm
        self.model, self.sd, self.tok, _, self.sp, self.tp = _build(llm)
        self.eng, self.geo = self.model.engine, self.model.geo
        g = torch.Generator(device=DEV); g.manual_seed(23)
        self.common = (torch.randn((128, self.geo.hidden), device=DEV, generator=g) * 0.5).to(bf)
        self.pool = (torch.randn((1024, self.geo.hidden), device=DEV, generator=g) * 0.5).to(bf)
        self.base = self.eng.seq_alloc(128)
        self.eng.prefill(self.base, self.common)
        self.refs = {}

    def tail(self, key):
        p, n = key
        off = (p // 64 * 131 + n * 7) % 900
        return self.pool[off:off + n]

    def nxt(self, key):
        p, n = key
        if key in DENSE:
            return [(r * 53 + p + 5) % self.geo.vocab for r in range(n)]
        return [-100 if (n > 1 and r % 7 == 3) else (r * 37 + p + n * 11) % self.geo.vocab for r in range(n)]

    def open(self, key):
        p, n = key
        return self.eng.seq_fork(self.base, p, p + n + NEW + 1) if p else self.eng.seq_alloc(n + NEW + 1)

    def score(self, members, top_n=8):
        """one score_extend_batch over the members -> (sequences, (lp, rank, top ids, top lp, last logits))"""
        seqs = [self.open(k) for k in members]
        return seqs, self.eng.score_extend_batch(seqs, [self.tail(k) for k in members], [self.nxt(k) for k in members], top_n, want_logits=True)

    def alone(self, key):
        """the member scored in a call of its own (varlen_extend at its default), and what it generates next -- computed once and shared"""
        if key not in self.refs:
            seqs, out = self.score([key])
            first = self.eng.seq_read(seqs[0], 0, 1)
            ids = self.eng.decode_greedy(seqs[0], NEW, None)
            self.eng.seq_free(seqs[0])
            self.refs[key] = ([t.clone() for t in out], first, ids)
        return self.refs[key]

    def n_scored(self, key):
        return sum(t != -100 for t in self.nxt(key))


@pytest.fixture(scope="module", params=["phi3.5", "llama3"])
def ctx(request):
    c = Ctx(request.param)
    yield c
    c.eng.seq_free(c.base)
    _pages_back(c.eng)
    c.eng.close()


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_members_equal_alone(c, members, out, what):
    lp, rank, ti, tv, lg = out
    assert lp.shape[0] == sum(c.n_scored(k) for k in members)
    at = 0
    for i, k in enumerate(members):
        n = c.n_scored(k)
        (wlp, wrank, wti, wtv, wlg), _, _ = c.alone(k)
        assert torch.equal(bits(lp[at:at + n]), bits(wlp)), f"{c.llm} {what}: member {i} {k}: lp differs from the member scored alone"
        assert torch.equal(rank[at:at + n], wrank) and torch.equal(ti[at:at + n], wti) and torch.equal(bits(tv[at:at + n]), bits(wtv)), f"{c.llm} {what}: member {i} {k}"
        assert torch.equal(bits(lg[i]), bits(wlg[0])), f"{c.llm} {what}: member {i} {k}: last logits"
        at += n


@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("n", [1, 3, 8])
def test_a_member_does_not_depend_on_its_group_or_the_launch_form(ctx, n, form):
    c, eng = ctx, ctx.eng
    members = MEMBERS[:n]
    free = eng.kv_info()["free_pages"]
    for k in members:
        c.alone(k)
    eng.debug_set("varlen_extend", form)
    try:
        plan = PP.of_geometry(c.geo, [k[1] for k in members], [k[0] for k in members], varlen_extend=form)
        (seqs, out), launches, _ = PP.profiled_attn(eng, lambda: c.score(members))
        firsts = [eng.seq_read(s, 0, 1) for s in seqs]
        ids = eng.decode_greedy_batch(seqs, NEW, None)
        for s in seqs:
            eng.seq_free(s)
    finally:
        eng.debug_set("varlen_extend", 1)
    # the score flag changes no step of a layer (tests/test_prefill_score_plan_cpu.py), so the plan without it names the attention launches
    assert launches == c.geo.layers * PP.n_attn(plan), f"{c.llm} group of {n}, varlen_extend {form}: {launches} attention launches, planned {PP.n_attn(plan)} per layer"
    assert_members_equal_alone(c, members, out, f"group of {n}, varlen_extend {form}")
    for i, k in enumerate(members):
        assert firsts[i] == c.alone(k)[1] and ids[i] == c.alone(k)[2], (c.llm, n, form, k)
    assert eng.kv_info()["free_pages"] == free


def test_the_chunk_boundary_crosses_a_member(ctx):
    c = ctx
    assert sum(c.n_scored(k) for k in DENSE) == 120
    seqs, out = c.score(DENSE)
    for s in seqs:
        c.eng.seq_free(s)
    assert_members_equal_alone(c, DENSE, out, "120 scored rows")
    # top_n = 0 and a smaller top_n report the same lp / rank, and the lists' first entries
    seqs, (lp0, rank0, ti0, tv0, _) = c.score(DENSE, top_n=0)
    for s in seqs:
        c.eng.seq_free(s)
    seqs, (lp3, rank3, ti3, tv3, _) = c.score(DENSE, top_n=3)
    for s in seqs:
        c.eng.seq_free(s)
    assert ti0 is None and tv0 is None
    assert torch.equal(bits(lp0), bits(out[0])) and torch.equal(rank0, out[1]) and torch.equal(bits(lp3), bits(out[0])) and torch.equal(rank3, out[1])
    assert torch.equal(ti3[:, :3], out[2][:, :3]) and torch.equal(bits(tv3[:, :3]), bits(out[3][:, :3])) and bool((ti3[:, 3:] == -1).all()) and bool(torch.isinf(tv3[:, 3:]).all())


def test_prefix_of_128_equals_the_whole_prompt_from_empty(ctx):
    c, eng = ctx, ctx.eng
    for key in ((128, 70), (128, 1)):
        whole = torch.cat([c.common, c.tail(key)], 0)
        s = eng.seq_alloc(whole.shape[0] + 1)
        lp, rank, ti, tv, lg = eng.score_extend_batch([s], [whole], [[-100] * 128 + c.nxt(key)], 8, want_logits=True)
        eng.seq_free(s)
        (wlp, wrank, wti, wtv, wlg), _, _ = c.alone(key)
        assert torch.equal(bits(lp), bits(wlp)) and torch.equal(rank, wrank) and torch.equal(ti, wti) and torch.equal(bits(tv), bits(wtv)) and torch.equal(bits(lg), bits(wlg)), (c.llm, key)


def test_members_end_as_after_prefill_extend_batch(ctx):
    c, eng = ctx, ctx.eng
    seqs = [c.open(k) for k in MEMBERS]
    lg = eng.prefill_extend_batch(seqs, [c.tail(k) for k in MEMBERS], want_logits=True).clone()
    firsts = [eng.seq_read(s, 0, 1) for s in seqs]
    ids = eng.decode_greedy_batch(seqs, NEW, None)
    for s in seqs:
        eng.seq_free(s)
    seqs, out = c.score(MEMBERS, top_n=0)
    assert torch.equal(bits(out[4]), bits(lg)), f"{c.llm}: last logits after scoring differ from prefill_extend_batch's"
    assert [eng.seq_read(s, 0, 1) for s in seqs] == firsts and eng.decode_greedy_batch(seqs, NEW, None) == ids
    for s in seqs:
        eng.seq_free(s)


def lsm64(logits):
    return torch.log_softmax(torch.as_tensor(logits).double(), dim=-1)


def test_against_the_fp32_oracle(ctx):
    """max|lp - lp32| <= max(2 x 1e-2 x max|logits32|, 2.5 x max|lp_emu - lp32|): the project's 1e-2 logit tolerance carried through log-softmax (Lipschitz constant 2 in
    the sup norm), with check_bf16_class's factor over the bf16-emulating oracle.  Rank 0 wherever the fp32 top-1 margin exceeds twice the logit bound."""
    c, eng = ctx, ctx.eng
    S = 70
    x = c.pool[300:300 + S]
    W = c.sd["language_model"]
    ocfg = _ocfg(c.geo)
    l32 = O.llm_forward(ocfg, W, x.float().cpu(), False, None, 0, last_only=False)
    lemu = O.llm_forward(ocfg, W, x.float().cpu(), True, None, 0, last_only=False)
    top2 = l32.double().topk(2, dim=-1)
    g = torch.Generator().manual_seed(5)
    for what, tg in (("the fp32 argmax", top2.indices[:, 0].tolist()), ("seeded ids", torch.randint(0, c.geo.vocab, (S,), generator=g).tolist())):
        s = eng.seq_alloc(S + 1)
        lp, rank, _, _ = eng.score_extend_batch([s], [x], [tg], 0)
        eng.seq_free(s)
        idx = torch.tensor(tg)[:, None]
        lp32, lpe = lsm64(l32).gather(1, idx)[:, 0], lsm64(lemu).gather(1, idx)[:, 0]
        logit_bound = 1e-2 * float(l32.abs().max())
        err, e_emu = float((lp.cpu().double() - lp32).abs().max()), float((lpe - lp32).abs().max())
        bound = max(2 * logit_bound, 2.5 * e_emu)
        print(f"[parity] score {c.llm} {S} rows, targets = {what}: max|lp - lp32| = {err:.3e} (bound {bound:.3e}; bf16-emulating oracle {e_emu:.3e}; max|logits32| {float(l32.abs().max()):.3f})")
        assert err <= bound
        if what == "the fp32 argmax":
            clear = (top2.values[:, 0] - top2.values[:, 1]) > 2 * logit_bound
            assert int(clear.sum()) >= 1
            assert bool((rank.cpu()[clear] == 0).all()), f"{c.llm}: a row whose fp32 margin exceeds {2 * logit_bound:.3e} does not rank the fp32 argmax first"
            print(f"[parity] score {c.llm}: rank 0 on all {int(clear.sum())} of {S} rows whose fp32 top-1 margin exceeds {2 * logit_bound:.3e}")


def test_against_prefill_of_truncated_prompts(ctx):
    """|lp - log_softmax(last_logits)[t]| <= 2 x 1e-2 x max|last_logits| at 4 rows: the scored row's logits come from a GEMM behind a bf16 norm pass, gvl_prefill's from
    the GEMV with the norm fused -- equal up to rounding, not bitwise"""
    c, eng = ctx, ctx.eng
    key = (0, 65)
    x, tg = c.tail(key), [(r * 29 + 3) % c.geo.vocab for r in range(65)]
    s = eng.seq_alloc(66)
    lp, _, _, _ = eng.score_extend_batch([s], [x], [tg], 0)
    eng.seq_free(s)
    for r in (0, 31, 63, 64):
        s = eng.seq_alloc(r + 2)
        last = eng.prefill(s, x[:r + 1], want_logits=True).cpu()
        eng.seq_free(s)
        want, bound = float(lsm64(last)[tg[r]]), 2e-2 * float(last.abs().max())
        print(f"[parity] score {c.llm} row {r} vs prefill of the truncated prompt: |lp - ref| = {abs(float(lp[r]) - want):.3e} (bound {bound:.3e})")
        assert abs(float(lp[r]) - want) <= bound


def test_a_vocabulary_that_is_no_multiple_of_sixteen():
    """the fine-tuned vocabularies are 32 366 and 128 558: the score tail's GEMM takes the columns up to the last multiple of 16 (its whole-row epilogue; N % 4 == 0 is
    the GEMM's contract), head_cols_kernel the rest.  vocab 414 = 400 + 14: every column against gvl_prefill's last logits of the truncated prompt (the GEMV takes any
    N) through targets in both parts and the top lists, and a group against its members alone."""
    V, hid = 414, 256
    short, long = synth.longrope_factors(hid // 4)
    geo = tiny_geo(llm="phi3.5", hidden=hid, inter=512, layers=2, heads=4, kv_heads=4, vocab=V, max_seq=512, max_prefill=256, kv_pages=32, rope_short=short, rope_long=long)
    eng = llm_engine(geo, synth.llm_weights("phi3", hid, 512, 2, 4, 4, V, True, seed="t.score.v414", device=DEV))
    g = torch.Generator(device=DEV); g.manual_seed(3)
    x = (torch.randn((70, hid), device=DEV, generator=g) * 0.5).to(bf)
    tg = [(V - 1 - r) if r % 2 else (r * 5) % 400 for r in range(70)]           # odd rows: ids 413, 411, ... in and around the last 14 columns
    s = eng.seq_alloc(71)
    lp, rank, ti, tv = eng.score_extend_batch([s], [x], [tg], 8)
    eng.seq_free(s)
    for r in (1, 3, 13, 64, 69):
        s = eng.seq_alloc(r + 2)
        last = eng.prefill(s, x[:r + 1], want_logits=True).cpu()
        eng.seq_free(s)
        ref = lsm64(last)
        bound = 2e-2 * float(last.abs().max())
        assert abs(float(lp[r]) - float(ref[tg[r]])) <= bound, (r, float(lp[r]), float(ref[tg[r]]))
        order = sorted(range(V), key=lambda i: (-float(last[i]), i))
        got = ti[r].tolist()
        # the lists agree with the prefill's order wherever its neighbours are further apart than the bound; every listed value is that id's log-probability
        for j in range(8):
            assert abs(float(tv[r, j]) - float(ref[got[j]])) <= bound, (r, j)
            if j < 7 and float(last[order[j]] - last[order[j + 1]]) > 2 * bound and (j == 0 or float(last[order[j - 1]] - last[order[j]]) > 2 * bound):
                assert got[j] == order[j], (r, j)
        print(f"[parity] score vocab {V} row {r} (target {tg[r]}) vs prefill of the truncated prompt: |lp - ref| = {abs(float(lp[r]) - float(ref[tg[r]])):.3e} (bound {bound:.3e})")
    # the 14 columns behind the GEMM's hold real logits: over the 70 rows some of them reach the top lists
    assert int((ti >= 400).sum()) >= 1
    halves = [x[:33], x[33:]]
    seqs = [eng.seq_alloc(40), eng.seq_alloc(40)]
    both = eng.score_extend_batch(seqs, halves, [tg[:33], tg[33:]], 8)
    for q in seqs:
        eng.seq_free(q)
    s = eng.seq_alloc(40)
    second = eng.score_extend_batch([s], [halves[1]], [tg[33:]], 8)
    eng.seq_free(s)
    for u, v in zip(both, second):
        assert torch.equal(bits(u[33:]), bits(v))
    assert eng.kv_info()["free_pages"] == eng.kv_info()["total_pages"]
    eng.close()


def test_against_the_reference_training_loss_goldens():
    """-mean(lp) over the labelled rows within 5e-3 relative of the reference's loss (the bound of test_forward_loss_matches_reference_golden)"""
    meta, g = load_golden("train_loss")
    c, lc = meta["cfg"], meta["llama_cfg"]
    engines = [(llm_engine(_phi_geo(c), synth.llm_weights("phi3", c["hidden"], c["inter"], c["layers"], c["heads"], c["kv_heads"], c["vocab"], True, seed=meta["seed"])),
                c, meta["cases"]),
               (llm_engine(tiny_geo(llm="llama3", hidden=lc["hidden"], inter=lc["inter"], layers=lc["layers"], heads=lc["heads"], kv_heads=lc["kv_heads"], vocab=lc["vocab"],
                                    rope_theta=lc["rope_theta"], rope_orig_max_pos=0),
                           synth.llm_weights("llama", lc["hidden"], lc["inter"], lc["layers"], lc["heads"], lc["kv_heads"], lc["vocab"], True, seed=meta["llama_seed"])),
                lc, meta["llama_cases"])]
    for eng, cfg, cases in engines:
        for name, m in cases.items():
            x = synth.det_tensor(m["x"], (1, m["S"], cfg["hidden"]), 0.5)[0].to(DEV).to(bf)
            nxt = [int(v) for v in m["labels"][1:]] + [-100]           # HF's labels are aligned with the rows and shifted inside: row r predicts labels[r + 1]
            s = eng.seq_alloc(m["S"] + 1)
            lp, _, _, _ = eng.score_extend_batch([s], [x], [nxt], 0)
            eng.seq_free(s)
            ref = float(g[name + "_loss"])
            got = -float(lp.double().mean())
            print(f"[parity] score {name}: -mean(lp) {got:.6f} reference loss {ref:.6f} over {lp.shape[0]} tokens")
            assert lp.shape[0] == m["n_valid"] and abs(got - ref) < 5e-3 * ref
        eng.close()


def test_refusals_leave_the_pool_and_the_sequences_as_they_were(ctx):
    c, eng = ctx, ctx.eng
    members = MEMBERS[:3]
    for k in members:
        c.alone(k)
    free0 = eng.kv_info()["free_pages"]
    seqs = [c.open(k) for k in members]
    tails, nxt = [c.tail(k) for k in members], [c.nxt(k) for k in members]
    free = eng.kv_info()["free_pages"]
    bad_id = [list(t) for t in nxt]; bad_id[2][-1] = c.geo.vocab
    neg_id = [list(t) for t in nxt]; neg_id[0][0] = -1
    for what, args in {"top_n = 9": (seqs, tails, nxt, 9), "top_n = -1": (seqs, tails, nxt, -1), "a target = vocab": (seqs, tails, bad_id, 8), "a target = -1": (seqs, tails, neg_id, 8),
                       "a sequence twice": (seqs + [seqs[0]], tails + [tails[0]], nxt + [nxt[0]], 8), "an empty tail": (seqs, tails[:2] + [c.pool[:0]], nxt[:2] + [[]], 8)}.items():
        with pytest.raises(GvlError) as e:
            eng.score_extend_batch(*args)
        assert e.value.status == -1, what
        assert eng.kv_info()["free_pages"] == free, what
    out = eng.score_extend_batch(seqs, tails, nxt, 8, want_logits=True)          # the sequences are as they were: the valid call gives what it gives on fresh ones
    for s in seqs:
        eng.seq_free(s)
    assert_members_equal_alone(c, members, out, "after refused calls")
    assert eng.kv_info()["free_pages"] == free0


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------------------------------------
QUESTION = "What is the person doing in the video? Options: (A) opening a door (B) cooking (C) reading a book (D) running"
OPTIONS = ["(A) opening a door", "(B) cooking", "(C) reading a book", "(D) running"]


def one_video(c):
    return {"spatial_pixel_values": c.sp.to(DEV), "temporal_pixel_values": c.tp.to(DEV), "video_ids": ["synthetic"]}


def slots_and_pages_back(c):
    """nothing of a call stays live: every page is back in the pool, and the lowest free sequence slot is the one that was free before (the base holds slot 0)"""
    kv = c.eng.kv_info()
    assert kv["free_pages"] == kv["total_pages"] - 2, kv                      # the fixture's base holds 128 tokens
    s = c.eng.seq_alloc(1)
    c.eng.seq_free(s)
    assert s == c.slot


def test_model_score_pairs_do_not_depend_on_each_other_or_on_sharing(ctx):
    c, model = ctx, ctx.model
    s = c.eng.seq_alloc(1); c.eng.seq_free(s); c.slot = s
    one = one_video(c)
    q = P.build_prompt(c.llm, "qa", QUESTION)
    shared = model.score(one, [q] * 4, OPTIONS, top_logprobs=3)
    assert model.last_shared_prefix >= 128 and model.last_shared_prefix % 128 == 0
    slots_and_pages_back(c)
    singles = [model.score(one, [q], [o], top_logprobs=3)[0] for o in OPTIONS]
    assert model.last_shared_prefix == 0
    slots_and_pages_back(c)
    assert shared == singles, f"{c.llm}: four pairs in one call differ from one call per pair"
    unshared = model.score(one, [q] * 4, OPTIONS, top_logprobs=3, share_prefix=False)
    assert model.last_shared_prefix == 0 and unshared == shared, f"{c.llm}: sharing the prefix changes the scores"
    slots_and_pages_back(c)
    for o, opt in zip(shared, OPTIONS):
        ids = c.tok(opt)[1:]                                                 # the synthetic tokenizer prepends BOS: a continuation carries none
        assert o.token_ids == ids and len(o.token_logprobs) == len(o.ranks) == len(o.top_logprobs) == len(ids)
        assert all(math.isfinite(v) and v < 0 for v in o.token_logprobs) and o.sum_logprob == sum(o.token_logprobs) and o.mean_logprob == o.sum_logprob / len(ids)
        for t, lp, r, top in zip(o.token_ids, o.token_logprobs, o.ranks, o.top_logprobs):
            assert len(top) == 3 and [v for _, v in top] == sorted((v for _, v in top), reverse=True)
            if r < 3:
                assert top[r] == (t, lp)                                     # a listed id sits at its rank, with the same value
            else:
                assert t not in [i for i, _ in top] and lp <= top[2][1]
    # continuation_ids is the same path; nine pairs form two groups; append_eos scores one more token and leaves the others as they are
    by_ids = model.score(one, [q] * 4, continuation_ids=[o.token_ids for o in shared], top_logprobs=3)
    assert by_ids == shared
    nine = model.score(one, [q] * 9, (OPTIONS * 3)[:9], top_logprobs=3)
    assert nine[:4] == shared and nine[4:8] == shared and nine[8] == shared[0]
    eos = model.score(one, [q] * 4, OPTIONS, top_logprobs=3, append_eos=True)
    for a, b in zip(eos, shared):
        assert a.token_ids == b.token_ids + [c.tok.eos_token_id] and a.token_logprobs[:-1] == b.token_logprobs and a.ranks[:-1] == b.ranks
    slots_and_pages_back(c)
    # different prompts about the video: the prefix ends where they part ways; same numbers as alone
    q2 = P.build_prompt(c.llm, "qa", "What happens at the end of the video?")
    mixed = model.score(one, [q, q2], [OPTIONS[0], "the person leaves"])
    assert mixed[0].token_logprobs == shared[0].token_logprobs and mixed[0].top_logprobs is None
    assert mixed[1] == model.score(one, [q2], ["the person leaves"])[0]
    slots_and_pages_back(c)
    # errors come before any device work and leave nothing behind
    for kw in (dict(continuations=OPTIONS, top_logprobs=9), dict(continuations=OPTIONS[:3]), dict(), dict(continuations=OPTIONS, continuation_ids=[[5]] * 4),
               dict(continuation_ids=[[5]] * 3 + [[c.geo.vocab]]), dict(continuation_ids=[[5]] * 3 + [[]]), dict(continuation_ids=[[5]] * 3 + [[7] * c.geo.max_seq])):
        with pytest.raises(ValueError):
            model.score(one, [q] * 4, **kw)
        slots_and_pages_back(c)


def test_generate_shared_is_unchanged_by_the_shared_prefix_helper(ctx):
    """generate_shared's texts equal one generate() per prompt (the statement test_gpu_extend_varlen makes on these prompts), and the helper both callers now use
    returns what the rule inside _generate_shared_prefix returned: restated here in its former words"""
    c, model = ctx, ctx.model
    prompts = [P.build_prompt(c.llm, "grounding", "When does the person open the door in the video?"), P.build_prompt(c.llm, "grounding", "When does the dog jump?"),
               P.build_prompt(c.llm, "qa", "Describe the video in detail please.")]
    one = one_video(c)
    texts = model.generate_shared(one, prompts, do_sample=False, num_beams=1, max_new_tokens=10)
    rows = [model.tokenizer_image_token(t) for t in prompts]
    n_vis = model._n_visual(one)
    k = rows[0].index(P.IMAGE_TOKEN_INDEX)
    assert all(r[:k + 1] == rows[0][:k + 1] for r in rows)
    tail = 0
    while all(k + 1 + tail < len(r) for r in rows) and len({r[k + 1 + tail] for r in rows}) == 1:
        tail += 1
    want = min(k + n_vis + tail, min(len(r) - 1 + n_vis for r in rows) - 1) // 128 * 128
    assert model.last_shared_prefix == want >= 128
    assert texts == [model.generate({**one, "prompts": [p]}, do_sample=False, num_beams=1, max_new_tokens=10)[0] for p in prompts]
    # the cases the rule declines: one prompt, prompts that differ before the image slot, nothing in common past 128 rows, the LongRoPE condition
    lens = [len(r) - 1 + n_vis for r in rows]
    assert model._shared_prefix(rows[:1], n_vis, lens[:1], lens[0] - 1) == 0
    assert model._shared_prefix([rows[0], [rows[0][0] + 1] + rows[1][1:]], n_vis, lens[:2], min(lens[:2]) - 1) == 0
    assert model._shared_prefix(rows, n_vis, lens, 127) == 0 and model._shared_prefix(rows, n_vis, lens, 128) == 128
    if model.geo.rope_long is not None:
        omax = model.geo.rope_orig_max_pos
        assert model._shared_prefix(rows, n_vis, [omax + 1] + lens[1:], min(lens) - 1) == (0 if want <= omax else want)
