"""-m gpu: gvl_prefill_extend_varlen (Engine.prefill_extend_batch) -- a ragged prefill whose members each sit behind their own cached prefix -- on tiny 2-layer
models at head dims 64 (Phi MHA), 96 (Phi MHA) and 128 (Llama GQA, 2 KV heads), modelled on test_gpu_llm.py::test_prefix_sharing_fork_and_extend_prefill.
The contract is bit identity: every member ends exactly as after its OWN gvl_prefill_extend (gvl_prefill when it is empty) -- logits, first token, greedy continuation
(which reads every KV page the prefill wrote) -- under both launch forms (gvl_debug_set "varlen_extend" 1: one grid per step and layer; 0: per-sequence launches).
Sizes: prefixes 0 / 64 / 128 / 192 / 320 forked from two bases (so the block tables differ), tails 1 ... 200 around the 64-token page and the 128-row query block."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, bf, check, llm_engine, tiny_geo  # noqa: E402
from grounded_video_llm_amd import engine as E, prompts as P, serve, synth  # noqa: E402
import prefill_plan as PP  # noqa: E402

NEW = 9                      # greedy continuation tokens
MODELS = {
    "phi_d64": dict(llm="phi3.5", hidden=256, heads=4, kv_heads=4),
    "phi_d96": dict(llm="phi3.5", hidden=384, heads=4, kv_heads=4),
    "llama_d128_gqa": dict(llm="llama3", hidden=512, heads=4, kv_heads=2),
}
# (base, prefix, tail rows); base None = an empty sequence (its "tail" is its whole prompt)
GROUPS = {
    2: [(0, 64, 1), (1, 320, 200)],
    3: [(0, 128, 37), (None, 0, 63), (1, 192, 64)],
    5: [(0, 320, 65), (1, 64, 127), (None, 0, 128), (0, 192, 129), (1, 128, 1)],
    8: [(1, 64, 1), (0, 128, 37), (None, 0, 63), (0, 192, 64), (1, 320, 65), (0, 64, 127), (1, 128, 128), (None, 0, 129)],
}
_KEYS = [k for g in GROUPS.values() for k in g]          # every tail and prefix size the kernels branch on, both bases, groups of 2 / 3 / 5 / 8
assert {k[2] for k in _KEYS} == {1, 37, 63, 64, 65, 127, 128, 129, 200} and {k[1] for k in _KEYS} == {0, 64, 128, 192, 320} and {k[0] for k in _KEYS} == {None, 0, 1}


def make_engine(name, **geo_kw):
    m = MODELS[name]
    kw = dict(llm=m["llm"], hidden=m["hidden"], inter=512, layers=2, heads=m["heads"], kv_heads=m["kv_heads"], vocab=400, max_seq=1024, max_prefill=768, kv_pages=128)
    if m["llm"] == "phi3.5":
        kw["rope_short"], kw["rope_long"] = synth.longrope_factors(m["hidden"] // m["heads"])
    else:
        kw.update(rope_theta=500000.0, rope_orig_max_pos=0)
    kw.update(geo_kw)
    geo = tiny_geo(**kw)
    W = synth.llm_weights("phi3" if m["llm"] == "phi3.5" else "llama", m["hidden"], 512, 2, m["heads"], m["kv_heads"], 400, True, seed="t.extvl." + name, device=DEV)
    return llm_engine(geo, W), geo


def make_ctx(name, **geo_kw):
    eng, geo = make_engine(name, **geo_kw)
    g = torch.Generator(device=DEV); g.manual_seed(17)
    c = SimpleNamespace(eng=eng, geo=geo, name=name, refs={}, work={}, free0=eng.kv_info()["free_pages"])
    c.commons = [(torch.randn((400, geo.hidden), device=DEV, generator=g) * 0.5).to(bf) for _ in range(2)]
    c.pool = (torch.randn((2048, geo.hidden), device=DEV, generator=g) * 0.5).to(bf)
    c.bases = open_bases(c)
    return c


def open_bases(c):
    bases = []
    for x in c.commons:
        bases.append(c.eng.seq_alloc(320))
        c.eng.prefill(bases[-1], x[:320])
    return bases


@pytest.fixture(scope="module", params=list(MODELS))
def ctx(request):
    c = make_ctx(request.param)
    yield c
    for b in c.bases:
        c.eng.seq_free(b)
    assert c.eng.kv_info()["free_pages"] == c.free0, "pages leaked or double-freed"
    c.eng.close()


def tail(c, key):
    b, p, n = key
    off = ((b or 0) * 7 + p // 64 * 13 + n * 3) % 1000
    return c.pool[off:off + n]


def open_member(c, key, bases=None):
    b, p, n = key
    return c.eng.seq_fork((bases or c.bases)[b], p, p + n + NEW + 1) if p else c.eng.seq_alloc(n + NEW + 1)


def own(c, key):
    """(logits, first token, greedy ids) of the member's own gvl_prefill_extend / gvl_prefill -- computed once per model and shared by the tests"""
    if key not in c.refs:
        s = open_member(c, key)
        lg = (c.eng.prefill_extend(s, tail(c, key), want_logits=True) if key[1] else c.eng.prefill(s, tail(c, key), want_logits=True)).clone()
        first = c.eng.seq_read(s, 0, 1)
        ids = c.eng.decode_greedy(s, NEW, None)
        c.eng.seq_free(s)
        c.refs[key] = (lg, first, ids)
    return c.refs[key]


def ragged(c, members, bases=None):
    """one prefill_extend_batch over the members -> (sequences, logits [n][vocab], first tokens)"""
    seqs = [open_member(c, k, bases) for k in members]
    lg = c.eng.prefill_extend_batch(seqs, [tail(c, k) for k in members], want_logits=True)
    return seqs, lg, [c.eng.seq_read(s, 0, 1) for s in seqs]


def assert_planned_launches(c, members, form, want):
    """The results cannot say which launches a group took (every form is bit-identical): the plan can, and the library's own count of attention launches must agree
    with it -- booked with the same work whatever the form.  One extra prefill of the group, with gvl_prof_enable on."""
    assert sum(k[2] for k in members) <= c.geo.max_prefill                   # one group
    p = PP.of_geometry(c.geo, [k[2] for k in members], [k[1] for k in members], varlen_extend=form)
    assert PP.forms(p) == want, (c.name, members, form, PP.forms(p))
    (seqs, _, _), launches, work = PP.profiled_attn(c.eng, lambda: ragged(c, members))
    for s in seqs:
        c.eng.seq_free(s)
    assert launches == c.geo.layers * PP.n_attn(p), f"{c.name} {members} varlen_extend {form}: {launches} attention launches, planned {PP.n_attn(p)} per layer"
    assert c.work.setdefault(tuple(members), work) == work, f"{c.name} {members} varlen_extend {form}: attention work {work} vs {c.work[tuple(members)]} under the other form"


def assert_members_equal_their_own_extend(c, members, what):
    want = [own(c, k) for k in members]
    seqs, lg, firsts = ragged(c, members)
    ids = c.eng.decode_greedy_batch(seqs, NEW, None)
    for s in seqs:
        c.eng.seq_free(s)
    for i, (k, w) in enumerate(zip(members, want)):
        assert torch.equal(lg[i], w[0]), f"{c.name} {what}: member {i} {k}: last_logits differ from its own extend"
        assert firsts[i] == w[1], f"{c.name} {what}: member {i} {k}: first token {firsts[i]} vs {w[1]}"
        assert ids[i] == w[2] and len(ids[i]) == len(w[2]), f"{c.name} {what}: member {i} {k}: greedy continuation {ids[i]} vs {w[2]}"


@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("n", sorted(GROUPS))
def test_bit_identical_to_each_members_own_extend(ctx, n, form):
    free = ctx.eng.kv_info()["free_pages"]
    ctx.eng.debug_set("varlen_extend", form)
    try:
        assert_members_equal_their_own_extend(ctx, GROUPS[n], f"group of {n}, varlen_extend {form}")
        assert_planned_launches(ctx, GROUPS[n], form, (("RAGGED_EXT",),) * 2 if form else (("ONE",) * n,) * 2)
    finally:
        ctx.eng.debug_set("varlen_extend", 1)
    assert ctx.eng.kv_info()["free_pages"] == free


def test_against_a_full_prefill_and_bases_freed_before_their_forks(ctx):
    """a prefix that is a multiple of 128 (whole query blocks): bit-identical to ONE prefill of the whole prompt; an odd multiple of 64: within the bound
    test_prefix_sharing_fork_and_extend_prefill uses for the single-sequence extend (1e-2).  The bases are freed before the forks decode."""
    c, eng = ctx, ctx.eng
    members = [(0, 128, 37), (1, 256, 65), (0, 64, 129), (1, 192, 200), (0, 256, 1)]

    def full(key):
        e = torch.cat([c.commons[key[0]][:key[1]], tail(c, key)], 0)
        s = eng.seq_alloc(e.shape[0] + NEW + 1)
        lg = eng.prefill(s, e, want_logits=True).clone()
        ids = eng.decode_greedy(s, NEW, None)
        eng.seq_free(s)
        return lg, ids

    refs = [full(k) for k in members]
    free = eng.kv_info()["free_pages"]
    bases = open_bases(c)
    seqs, lg, _ = ragged(c, members, bases)
    for b in bases:
        eng.seq_free(b)
    ids = eng.decode_greedy_batch(seqs, NEW, None)
    for s in seqs:
        eng.seq_free(s)
    assert eng.kv_info()["free_pages"] == free, "pages leaked or double-freed"
    for i, k in enumerate(members):
        if k[1] % 128 == 0:
            assert torch.equal(lg[i], refs[i][0]) and ids[i] == refs[i][1], f"{c.name}: member {k}: differs from the full prefill of its prompt"
        else:
            check(lg[i], refs[i][0], 1e-2, f"{c.name}: ragged extend at prefix {k[1]} (not a query-block boundary) vs full prefill")


def test_groups_split_by_member_count_and_by_rows(ctx):
    """more than GVL_MAX_PREFILL_BATCH = 8 members, and more than cfg.max_prefill = 768 rows: the call forms several groups in call order, same results"""
    eleven = [(i % 2, (64, 128, 192, 320)[i % 4], (1, 37, 63, 64, 65)[i % 5]) for i in range(10)] + [(None, 0, 63)]
    assert len(set(eleven)) == 11
    assert_members_equal_their_own_extend(ctx, eleven, "11 members")
    rows = [(0, 64, 200), (1, 128, 200), (0, 192, 200), (1, 320, 200), (None, 0, 129)]
    assert sum(k[2] for k in rows) > ctx.geo.max_prefill
    assert_members_equal_their_own_extend(ctx, rows, "929 rows on a 768-row workspace")


def test_sampled_followers_draw_as_sequential_extends_would(ctx):
    """ctx sampling on: a member's random stream is its place in the prefill order since gvl_set_sampling -- one ragged call hands them out in call order"""
    c, eng = ctx, ctx.eng
    members = GROUPS[5]
    for b in c.bases:
        eng.seq_free(b)
    out = {}
    try:
        for how in ("ragged", "sequential"):
            assert eng.kv_info()["free_pages"] == c.free0                    # nothing live: the stream numbering restarts
            eng.set_sampling(True, temperature=1.5, top_k=0, seed=29)
            bases = open_bases(c)
            if how == "ragged":
                seqs, _, firsts = ragged(c, members, bases)
            else:
                seqs = [open_member(c, k, bases) for k in members]
                for s, k in zip(seqs, members):
                    eng.prefill_extend(s, tail(c, k)) if k[1] else eng.prefill(s, tail(c, k))
                firsts = [eng.seq_read(s, 0, 1) for s in seqs]
            out[how] = (firsts, eng.decode_greedy_batch(seqs, NEW, None))
            for s in seqs + bases:
                eng.seq_free(s)
    finally:
        eng.set_sampling(False)
        c.bases = open_bases(c)
    assert out["ragged"] == out["sequential"]
    greedy = [own(c, k)[2] for k in members]
    assert out["ragged"][1] != greedy, "temperature 1.5 drew the greedy ids for every member: sampling was not on"


def test_errors_leave_the_pool_and_the_sequences_as_they_were(ctx):
    c, eng = ctx, ctx.eng
    members = GROUPS[3]
    free0 = eng.kv_info()["free_pages"]
    seqs = [open_member(c, k) for k in members]
    tails = [tail(c, k) for k in members]
    odd = eng.seq_alloc(300)
    eng.prefill(odd, c.pool[:100])                                             # holds 100 tokens: not whole pages
    free = eng.kv_info()["free_pages"]
    bad = {
        "a member whose tokens are not whole pages": (seqs + [odd], tails + [c.pool[:5]]),
        "an empty tail": (seqs, tails[:2] + [c.pool[:0]]),
        "a tail past the sequence's max_tokens": (seqs, tails[:2] + [c.pool[:64 + NEW + 2]]),
        "a tail longer than cfg.max_prefill": (seqs, tails[:2] + [c.pool[:c.geo.max_prefill + 1]]),
        "a sequence twice": (seqs + [seqs[0]], tails + [tails[0]]),
        "an unknown sequence": (seqs + [12345], tails + [tails[0]]),
    }
    for what, (ss, es) in bad.items():
        with pytest.raises(RuntimeError):
            eng.prefill_extend_batch(ss, es)
        assert eng.kv_info()["free_pages"] == free, what
    eng.seq_free(odd)
    # ... and the sequences are as they were: the valid call now gives what it gives on fresh ones
    lg = eng.prefill_extend_batch(seqs, tails, want_logits=True)
    ids = eng.decode_greedy_batch(seqs, NEW, None)
    for s in seqs:
        eng.seq_free(s)
    for i, k in enumerate(members):
        assert torch.equal(lg[i], own(c, k)[0]) and ids[i] == own(c, k)[2], (c.name, k)
    assert eng.kv_info()["free_pages"] == free0


def test_members_on_both_sides_of_the_longrope_switch():
    """LongRoPE picks a factor set per launch from where a sequence ENDS (pos + new rows against rope_orig_max_pos): a ragged group that straddles the switch cannot
    take one RoPE launch -- each member must still come out as its own extend, and so must a group that lies wholly past the switch"""
    c = make_ctx("phi_d96", rope_orig_max_pos=200)
    try:
        mixed = [(0, 128, 37), (0, 192, 64), (None, 0, 63), (1, 128, 129), (1, 64, 136), (None, 0, 201)]     # ends: 165, 256, 63, 257, 200 (the last short one), 201
        assert sorted((k[1] + k[2] > 200) for k in mixed) == [False] * 3 + [True] * 3
        for form in (1, 0):
            c.eng.debug_set("varlen_extend", form)
            assert_members_equal_their_own_extend(c, mixed, f"straddling rope_orig_max_pos, varlen_extend {form}")
            assert_members_equal_their_own_extend(c, [k for k in mixed if k[1] + k[2] > 200], f"all past rope_orig_max_pos, varlen_extend {form}")
            assert_members_equal_their_own_extend(c, [k for k in mixed if k[1] + k[2] <= 200], f"all within rope_orig_max_pos, varlen_extend {form}")
            # the straddling group keeps RoPE / KV append per member (one factor set per launch) and still shares the attention grid
            assert_planned_launches(c, mixed, form, ((("ONE",) * 6, ("RAGGED_EXT",)) if form else (("ONE",) * 6,) * 2))
            for side in ([k for k in mixed if k[1] + k[2] > 200], [k for k in mixed if k[1] + k[2] <= 200]):
                assert_planned_launches(c, side, form, (("RAGGED_EXT",),) * 2 if form else (("ONE",) * 3,) * 2)
        # the two factor sets do differ at these positions: the same rows behind the same prefix, ending on either side of the switch
        a, b = own(c, (1, 64, 136))[0], own(c, (1, 64, 137))[0]
        assert not torch.equal(a, b)
    finally:
        for b in c.bases:
            c.eng.seq_free(b)
        assert c.eng.kv_info()["free_pages"] == c.free0
        c.eng.close()


def test_clip_scheduler_with_prefixes_on_the_device(ctx):
    """prefixed and plain requests mixed, drop_prefix mid-run: the ids of every request equal Engine.generate_ids of its full prompt"""
    c, eng = ctx, ctx.eng
    free0 = eng.kv_info()["free_pages"]
    clips = [c.commons[0][:300], c.commons[1][:200]]                           # P = 256 and 128
    spec = [(0, 37), (None, 63), (1, 1), (0, 129), (1, 64), (None, 200), (0, 5), (1, 90), (0, 64)]
    prompts = [torch.cat([clips[k], c.pool[100 * i:100 * i + n]], 0) if k is not None else c.pool[100 * i:100 * i + n] for i, (k, n) in enumerate(spec)]
    want = [eng.generate_ids(e, 12, None) for e in prompts]
    sch = serve.ClipScheduler(eng, None, max_active=3, chunk=4)
    pids = [sch.add_prefix(x) for x in clips]
    assert [sch.prefixes[p].rows for p in pids] == [256, 128]
    rids = [sch.submit(e, 12, prefix=None if k is None else pids[k]) for e, (k, _) in zip(prompts, spec)]
    sch.step()
    assert sch.queue and any(r.prefix == pids[0] for r in sch.queue)
    sch.drop_prefix(pids[0])                                                   # queued requests still name it: the holder lives until the last of them is admitted
    out = sch.run()
    assert [out[r] for r in rids] == want
    assert sch.stats["prefix_rows_saved"] == 4 * 256 + 3 * 128 and pids[0] not in sch.prefixes
    sch.drop_prefix(pids[1])
    assert eng.kv_info()["free_pages"] == free0


def test_generate_shared_texts_do_not_depend_on_the_launch_form():
    from grounded_video_llm_amd.model import LLAVA_NEXT_VIDEO, SyntheticTokenizer
    llm, hid, vocab = "phi3.5", 128, 640
    short, long = synth.longrope_factors(32)
    tok = SyntheticTokenizer(vocab, 300)
    prompts = [P.build_prompt(llm, "grounding", "When does the person open the door in the video?"), P.build_prompt(llm, "grounding", "When does the dog jump?"),
               P.build_prompt(llm, "qa", "Describe the video in detail please.")]
    sd = {"vision_tower": synth.clip_weights(64, 128, 3, seed="gen.clip"), "video_encoder": synth.iv2_weights(64, 128, 3, 2, seed="gen.iv2"),
          "projectors": synth.projector_weights(llm, hid, 64, 64, seed="gen.proj"), "language_model": synth.llm_weights("phi3", hid, 256, 2, 4, 4, vocab, True, seed="gen.llm")}
    geo = E.TowerGeometry(llm=llm, clip_hidden=64, clip_inter=128, clip_layers=3, clip_heads=4, iv2_dim=64, iv2_inter=128, iv2_depth=3, iv2_heads=4, hidden=hid,
                          inter=256, layers=2, heads=4, kv_heads=4, vocab=vocab, rope_short=short, rope_long=long, rope_theta=10000.0, max_seq=2048, max_segs=6, kv_pages=60,
                          max_prefill=1024)
    model = LLAVA_NEXT_VIDEO(stage="sft", max_txt_len=64, num_frames=4, num_segs=2, num_temporal_tokens=300, lora=False, llm=llm, geometry=geo, tokenizer=tok,
                             state_dicts=sd, device=DEV)
    one = {"spatial_pixel_values": synth.det_tensor("gen.sp", (1, 2, 3, 336, 336)).to(DEV), "temporal_pixel_values": synth.det_tensor("gen.tp", (1, 4, 3, 224, 224)).to(DEV),
           "video_ids": ["x"]}
    texts = {}
    for form in (1, 0):
        model.engine.debug_set("varlen_extend", form)
        texts[form] = model.generate_shared(one, prompts, do_sample=False, num_beams=1, max_new_tokens=10)
        assert model.last_shared_prefix >= 128 and model.last_shared_prefix % 128 == 0
    assert texts[1] == texts[0] and len(texts[1]) == 3
    model.engine.debug_set("varlen_extend", 1)
    assert texts[1] == [model.generate({**one, "prompts": [p]}, do_sample=False, num_beams=1, max_new_tokens=10)[0] for p in prompts]
    assert model.engine.kv_info()["free_pages"] == model.engine.kv_info()["total_pages"]
    model.engine.close()
