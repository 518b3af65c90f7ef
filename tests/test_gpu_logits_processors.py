"""-m gpu: HF generate()'s logits processors (repetition_penalty, no_repeat_ngram_size, min_new_tokens / min_length) on the device
(csrc/gvl_logits.hip): the operator bit for bit against a torch restatement, generate() against a KV-cached oracle loop with the same
restatement, the processors visibly changing answers, and every way of decoding (batch, graph replay, shared prefix, scheduler, sampling,
beam search) agreeing with the single-sequence answer."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import gvl_oracle as O  # noqa: E402
from gpu_util import DEV  # noqa: E402
from grounded_video_llm_amd import engine as E, logits as LP, prompts as P, serve, synth  # noqa: E402
from grounded_video_llm_amd.model import LLAVA_NEXT_VIDEO, SyntheticTokenizer  # noqa: E402

bf = torch.bfloat16


def restate(scores: torch.Tensor, hist, penalty=1.0, ngram=0, min_new=0, eos=-1) -> torch.Tensor:
    """CPU torch restatement of one row (IEEE fp32 multiply / divide): penalty once per distinct generated id, n-gram bans, eos ban."""
    s = scores.detach().float().cpu().clone()
    L = len(hist)
    if penalty != 1.0 and L:
        h = torch.tensor(hist, dtype=torch.long)
        g = s.gather(0, h)
        s.scatter_(0, h, torch.where(g < 0, g * penalty, g / penalty))
    if ngram > 0 and L >= ngram:
        suf = list(hist[L - ngram + 1:])
        for i in range(L - ngram + 1):
            if list(hist[i:i + ngram - 1]) == suf:
                s[hist[i + ngram - 1]] = -math.inf
    if eos >= 0 and L < min_new:
        s[eos] = -math.inf
    return s


def _has_repeated_ngram(ids, n):
    grams = [tuple(ids[i:i + n]) for i in range(len(ids) - n + 1)]
    return len(grams) != len(set(grams))


def _build(llm):
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


def test_op_logits_process_equals_restatement_bit_for_bit(phi):
    eng = phi[0].engine
    g = torch.Generator().manual_seed(7)
    for V in (640, 32064 + 302, 128256 + 302):
        for B in (1, 5, 16):
            x = torch.randn((B, V), generator=g) * 4.0
            x[:, ::7] = 0.0                                           # zeros (and -0.0) next to negative and positive scores
            x[:, 3::11] = -0.0
            hists, pen, ngr, mnw, eos = [], [], [], [], []
            for b in range(B):
                n = (0, 1, 2, 3, 5)[b % 5]
                nn = n if n > 0 else 3
                L = (0, 1, nn - 1, nn, 2048, 8192)[(b + B) % 6]
                pool = torch.randint(0, V, (6,), generator=g)          # heavy duplicates: a handful of ids, repeated
                h = pool[torch.randint(0, 6, (L,), generator=g)].tolist() if b % 2 == 0 else torch.randint(0, V, (L,), generator=g).tolist()
                if L >= 4 and b % 3 == 0:
                    h[L // 2:L // 2 + 3] = h[L - 3:]                     # an n-gram that the suffix repeats
                e = h[len(h) // 2] if (h and b % 4 != 3) else (5 if b % 4 == 3 else -1)   # eos inside the history, or elsewhere / none
                hists.append(h); pen.append((1.0, 1.3, 0.7, 2.5)[b % 4]); ngr.append(n); mnw.append((0, 3, 9000, L + 1)[b % 4]); eos.append(e)
            got = eng.op_logits_process(x.to(DEV).contiguous(), hists, pen, ngr, mnw, eos).cpu()
            for b in range(B):
                ref = restate(x[b], hists[b], pen[b], ngr[b], mnw[b], eos[b])
                assert torch.equal(got[b].view(torch.int32), ref.view(torch.int32)), (V, B, b, len(hists[b]), pen[b], ngr[b], mnw[b], eos[b])


@pytest.mark.parametrize("llm", ["phi3.5", "llama3"])
def test_generate_with_processors_matches_oracle(llm, phi):
    model, sd, tok, geo, sp, tp = phi if llm == "phi3.5" else _build(llm)
    kind = "phi3" if llm == "phi3.5" else "llama"
    samples = _samples(llm, sp, tp, ["When does the person open the door in the video?"])
    ids = O.tokenizer_image_token(samples["prompts"][0], tok, tok.bos_token_id)
    ref_vis = O.encode_images(sp, tp, sd["vision_tower"], sd["video_encoder"], sd["projectors"], llm, clip_layers=3, clip_heads=4,
                              iv2_depth=3, iv2_heads=4, emu=True)[0]
    ocfg = O.LLMConfig(kind, 128, 256, 2, 4, geo.kv_heads, 640, 1e-5, geo.rope_theta, 131072, 4096, geo.rope_short, geo.rope_long)
    W = sd["language_model"]
    ref_emb = O.splice(torch.tensor(ids), ref_vis, W["model.embed_tokens.weight"], emu=True)
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=ref_emb.shape[0] + 4)
    procs = LP.resolve(kw, tok.eos_token_id, ref_emb.shape[0])
    assert procs.min_new == 4
    # oracle: KV-cached llm_forward loop + the restatement on every step's row
    e = O._r(W["model.embed_tokens.weight"], True)
    cache = [None] * ocfg.layers
    logits = O.llm_forward(ocfg, W, ref_emb, True, cache, 0, last_only=True)
    n, ref_ids, margins, scales = ref_emb.shape[0], [], [], []
    while len(ref_ids) < 16:
        s = restate(logits[-1], ref_ids, *procs.args())
        top2 = torch.topk(s, 2)
        ref_ids.append(int(top2.indices[0])); margins.append(float(top2.values[0] - top2.values[1])); scales.append(float(logits[-1].abs().max()))
        if ref_ids[-1] == tok.eos_token_id:
            break
        logits = O.llm_forward(ocfg, W, e[ref_ids[-1]][None], True, cache, n, last_only=True)
        n += 1
    feats = model.encode_images(samples)
    ids_arr, mask = P.left_pad_truncate([ids], tok.pad_token_id, model.max_txt_len)
    got = model.generate_ids(ids_arr, mask, feats, 16, processors=procs)[0]
    for i, (a, b) in enumerate(zip(got, ref_ids)):
        if a != b:
            print(f"[parity] processors({llm}): ids part ways at token {i} ({a} vs {b}); oracle margin {margins[i] / scales[i]:.3e} of the logit scale")
            assert margins[i] < min(2 * 2e-2 * scales[i], 0.25), (i, a, b, margins[i], scales[i])
            break
    else:
        assert len(got) == len(ref_ids)
    assert not _has_repeated_ngram(got, 2)
    text = model.generate(samples, do_sample=False, max_new_tokens=16, **kw)
    assert text[0] == tok.batch_decode([got], skip_special_tokens=True)[0].strip()
    _pages_back(model.engine)
    if llm != "phi3.5":
        model.engine.close()


def test_processors_change_the_answer(phi):
    eng = phi[0].engine
    eng.set_logits_processors()
    found = None
    for seed in range(8):                                              # a fixed tiny seed on which plain greedy loops
        emb = (torch.randn((40, 128), generator=torch.Generator().manual_seed(seed)) * 1.5).to(bf).to(DEV)
        plain = eng.generate_ids(emb, 32, None, processors=LP.OFF)
        if _has_repeated_ngram(plain, 2):
            found = (emb, plain)
            break
    assert found is not None, "precondition: plain greedy repeats a bigram within 32 tokens on one of the seeds"
    emb, plain = found
    ng = eng.generate_ids(emb, 32, None, processors=LP.Processors(ngram=2))
    assert len(ng) == 32 and not _has_repeated_ngram(ng, 2), ng
    eos = plain[0]                                                    # eos = the plain run's first token
    assert eng.generate_ids(emb, 32, eos, processors=LP.OFF) == [eos]
    for k in (1, 4, 9):
        out = eng.generate_ids(emb, 32, eos, processors=LP.Processors(min_new=k, eos=eos))
        assert eos not in out[:k] and len(out) > k, (k, out)
    pen = eng.generate_ids(emb, 32, None, processors=LP.Processors(penalty=1.5))
    assert pen != plain
    _pages_back(eng)


def test_decode_paths_agree_with_processors(phi):
    model, sd, tok, geo, sp, tp = phi
    eng = model.engine
    eos = tok.eos_token_id
    embs = [(torch.randn((S, 128), generator=torch.Generator().manual_seed(100 + S)) * 1.5).to(bf).to(DEV) for S in (37, 64, 90)]
    procs = [LP.Processors(1.3, 2, 3, eos), LP.Processors(0.8, 0, 5, eos), LP.Processors(1.0, 3, 0, eos)]
    single = [eng.generate_ids(e, 24, eos, processors=p) for e, p in zip(embs, procs)]
    # a batch of 3 (different settings per sequence, one decode group) == 3 single calls; graph replay on and off
    for graph in (1, 0):
        eng.debug_set("decode_graph", graph)
        seqs = [eng.seq_alloc(e.shape[0] + 24) for e in embs]
        try:
            for s_, p in zip(seqs, procs):
                eng.seq_set_processors(s_, *p.args())
            eng.prefill_batch(seqs, embs)
            assert eng.decode_greedy_batch(seqs, 24, eos) == single, graph
        finally:
            for s_ in seqs:
                eng.seq_free(s_)
    eng.debug_set("decode_graph", 1)
    # the continuous-batching scheduler (gvl_decode_steps: members at different steps, different settings, one group)
    sch = serve.ClipScheduler(eng, eos, max_active=3, chunk=5)
    rids = [sch.submit(embs[0], 24, repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3),
            sch.submit(embs[1], 24, repetition_penalty=0.8, min_new_tokens=5), sch.submit(embs[2], 24, no_repeat_ngram_size=3)]
    out = sch.run()
    assert [out[r] for r in rids] == single
    # off means today: 1.0 / 0 / 0 leave every id as without processors
    eng.set_logits_processors()
    base = [eng.generate_ids(e, 24, eos) for e in embs]
    eng.set_logits_processors(1.0, 0, 0, eos)
    assert [eng.generate_ids(e, 24, eos) for e in embs] == base
    assert [eng.generate_ids(e, 24, eos, processors=LP.OFF) for e in embs] == base
    _pages_back(eng)


def test_generate_surface_with_processors(phi):
    model, sd, tok, geo, sp, tp = phi
    qs = ["When does the person open the door in the video?", "What is on the table?", "Describe the video in detail please."]
    kw = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, max_new_tokens=14)
    one = [model.generate(_samples("phi3.5", sp, tp, [q]), do_sample=False, **kw)[0] for q in qs]
    assert model.generate(_samples("phi3.5", sp, tp, qs), do_sample=False, **kw) == one          # bs 3 == 3 single calls
    # off means today, through the public surface
    plain = model.generate(_samples("phi3.5", sp, tp, qs[:1]), do_sample=False, max_new_tokens=14)
    assert model.generate(_samples("phi3.5", sp, tp, qs[:1]), do_sample=False, max_new_tokens=14, repetition_penalty=1.0, no_repeat_ngram_size=0,
                          min_new_tokens=0) == plain
    # generate_shared == one generate() per prompt, each prompt with ITS OWN min_length adjustment
    n_vis = 2 * model.engine.tokens_per_seg
    lens = [len(O.tokenizer_image_token(P.build_prompt("phi3.5", "grounding", q), tok, tok.bos_token_id)) - 1 + n_vis for q in qs]
    kws = dict(kw, min_length=min(lens) + 6)
    one_s = [model.generate(_samples("phi3.5", sp, tp, [q]), do_sample=False, **kws)[0] for q in qs]
    assert model.generate_shared(_samples("phi3.5", sp, tp, qs[:1]), [P.build_prompt("phi3.5", "grounding", q) for q in qs], do_sample=False, **kws) == one_s
    # seeded sampling with processors: reproducible; top_k = 1 is greedy with processors
    smp = dict(kw, do_sample=True, temperature=1.5, top_p=None)
    s1 = model.generate(_samples("phi3.5", sp, tp, qs[:1]), seed=11, **smp)
    assert s1 == model.generate(_samples("phi3.5", sp, tp, qs[:1]), seed=11, **smp)
    assert model.generate(_samples("phi3.5", sp, tp, qs[:1]), seed=3, top_k=1, **smp) == one[:1]
    with pytest.raises(ValueError):
        model.generate(_samples("phi3.5", sp, tp, qs[:1]), repetition_penalty=0.0)
    _pages_back(model.engine)


def test_beam_search_with_processors(phi):
    model, sd, tok, geo, sp, tp = phi
    eng = model.engine
    row = O.tokenizer_image_token(P.build_prompt("phi3.5", "grounding", "When does the person open the door in the video?"), tok, tok.bos_token_id)
    feats = model.encode_images(_samples("phi3.5", sp, tp, ["x"]))[0]
    procs = LP.Processors(1.0, 2, 0, tok.eos_token_id)
    got = model.beam_generate_ids(row, feats, 3, 16, processors=procs)
    assert not _has_repeated_ngram(got, 2), got
    # the same search with the processors restated on the CPU on the same step rows
    dev_op = eng.op_logits_process
    calls = []

    def cpu_op(lp, hists, *a):
        calls.append(len(hists))
        return torch.stack([restate(lp[j], hists[j], *procs.args()) for j in range(lp.shape[0])]).to(lp.device)
    eng.op_logits_process = cpu_op
    try:
        ref = model.beam_generate_ids(row, feats, 3, 16, processors=procs)
    finally:
        eng.op_logits_process = dev_op
    assert calls and got == ref
    plain = model.beam_generate_ids(row, feats, 3, 16)
    if _has_repeated_ngram(plain, 2):
        assert plain != got
    _pages_back(eng)
