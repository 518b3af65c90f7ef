"""-m gpu: the engine on a KV pool whose LOW pages are taken.  Sequences get the lowest free pages first (SeqTable::reset_pool / open), so every other test and the benchmark
run on the first few dozen pages of their pools: page offsets of a few MB.  A server whose pool has filled up runs at the other end -- in production the offsets inside a
layer's slice pass 2^31 bytes and come within a fifth of 2^31 elements, the layer bases pass 100 GB.  Here a tiny 2-layer model gets a pool whose per-layer slice is LARGER
than 2^31 elements (17.5 GB for both pools), and one fixed, seeded scenario -- every entry that reads or writes KV pages: prefill, ragged prefill, fork + extend, ragged
extend over different prefixes, scoring, clone (kv_page_copy_kernel) and fan-out (kv_page_fanout_kernel) of a partial last page, greedy decode alone and in a group of 16,
the batched teacher-forced step, a beam search -- runs three times:

  (a)  on the fresh pool: low pages, as everywhere else;
  (b)  after everything is freed and FILLER sequences (host-only: gvl_seq_alloc runs no kernel) hold every page below ceil(2^31 / page elements).  Asserted through
       gvl_debug_seq_pages: the fillers hold EVERY page below the threshold -- so no other sequence can be given one, the beam search's internal clones included,
       which nobody can query -- and every page of every sequence the scenario holds lies at or above it ((a)'s lay below).  Without this the test could pass on
       low pages;
  (c)  after the fillers are freed and THEN (b)'s sequences: the free list is a stack, so (c) is handed exactly the pages (b) wrote, in the opposite order -- every
       sequence lands on pages that hold another sequence's keys and values, partial last pages on pages that were full.  Asserted through gvl_debug_seq_pages: every
       page (c) holds was written before, and the assignment differs from (b)'s.  A kernel that depends on what a page held before (unzeroed head-dim padding, V^T
       tail slots, the rest of a partial page after a clone or fan-out) differs here.

(b) and (c) must equal (a) BIT FOR BIT in every logits row, id, log-probability, rank and score.  The pool accounting returns to total == free.
Two geometries: Llama-style 8 KV heads x 128 on the skinny-MFMA decode path (hidden 1024), and Phi-style 4 x 96 (hidden 384: the VALU fallback, a page size that is
no power of two).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, bf, llm_engine, tiny_geo  # noqa: E402
from grounded_video_llm_amd import synth  # noqa: E402

NEW = 8                       # greedy steps
VOCAB = 400
SPARE = 600                   # pages above the threshold: the scenario holds fewer than 150 at once, the last filler may take up to a filler's worth less one
MODELS = {
    "llama_8x128_mfma": dict(llm="llama3", hidden=1024, heads=8, kv_heads=8, max_seq=16384, mfma=True),
    "phi_4x96_valu": dict(llm="phi3.5", hidden=384, heads=4, kv_heads=4, max_seq=32768, mfma=False),
}


def make_engine(name):
    m = MODELS[name]
    D = m["hidden"] // m["heads"]
    page_elems = m["kv_heads"] * 64 * D
    first_high = -(-(1 << 31) // page_elems)                # the first page whose element offset inside a layer is >= 2^31
    kw = dict(llm=m["llm"], hidden=m["hidden"], inter=512, layers=2, heads=m["heads"], kv_heads=m["kv_heads"], vocab=VOCAB, max_seq=m["max_seq"], max_prefill=768,
              kv_pages=first_high + SPARE)
    if m["llm"] == "phi3.5":
        kw["rope_short"], kw["rope_long"] = synth.longrope_factors(D)
    else:
        kw.update(rope_theta=500000.0, rope_orig_max_pos=0)
    geo = tiny_geo(**kw)
    W = synth.llm_weights("phi3" if m["llm"] == "phi3.5" else "llama", m["hidden"], 512, 2, m["heads"], m["kv_heads"], VOCAB, True, seed="t.kvhigh." + name, device=DEV)
    return llm_engine(geo, W), geo, page_elems, first_high


def scenario(eng, X, group):
    """-> (everything the scenario computed, the pages of every sequence it holds, by name, those sequences): the caller frees them"""
    out, live = {}, {}

    def hold(name, *seqs):
        live.update({f"{name}[{i}]": s for i, s in enumerate(seqs)})

    cpu = lambda t: t.detach().clone().cpu()
    # prefill, then 8 greedy steps alone
    s0 = eng.seq_alloc(200 + 24)
    hold("prefill", s0)
    out["prefill.logits"] = cpu(eng.prefill(s0, X[:200], want_logits=True))
    out["prefill.ids"] = eng.decode_greedy(s0, NEW, None)
    # ragged prefill of 3 prompts, decoded together
    lens = (65, 130, 31)
    b3 = [eng.seq_alloc(n + NEW + 1) for n in lens]
    hold("prefill_batch", *b3)
    eng.prefill_batch(b3, [X[100 + 200 * i:100 + 200 * i + n] for i, n in enumerate(lens)])
    out["batch.first"] = [eng.seq_read(s, 0, 1) for s in b3]
    out["batch.ids"] = eng.decode_greedy_batch(b3, NEW, None)
    # fork + extend
    bases = [eng.seq_alloc(320), eng.seq_alloc(320)]
    hold("base", *bases)
    eng.prefill(bases[0], X[700:1020])
    eng.prefill(bases[1], X[1000:1320])
    f = eng.seq_fork(bases[0], 192, 192 + 70 + NEW + 1)
    hold("fork", f)
    out["extend.logits"] = cpu(eng.prefill_extend(f, X[1400:1470], want_logits=True))
    out["extend.ids"] = eng.decode_greedy(f, NEW, None)
    # ragged extend over members with different prefixes (two bases, an empty member)
    keys = ((0, 64, 37), (1, 128, 127), (None, 0, 63), (0, 256, 65))
    ms = [eng.seq_fork(bases[b], p, p + n + NEW + 1) if p else eng.seq_alloc(n + NEW + 1) for b, p, n in keys]
    hold("extend_varlen", *ms)
    out["extend_varlen.logits"] = cpu(eng.prefill_extend_batch(ms, [X[1500 + 11 * i:1500 + 11 * i + n] for i, (_, _, n) in enumerate(keys)], want_logits=True))
    out["extend_varlen.first"] = [eng.seq_read(s, 0, 1) for s in ms]
    out["extend_varlen.ids"] = eng.decode_greedy_batch(ms, NEW, None)
    # scoring given ids behind cached prefixes
    skeys = ((1, 64, 40), (None, 0, 70))
    ss = [eng.seq_fork(bases[b], p, p + n + 2) if p else eng.seq_alloc(n + 2) for b, p, n in skeys]
    hold("score", *ss)
    nxt = [[(7 * r + 3 * i) % VOCAB if r % 5 else -100 for r in range(n)] for i, (_, _, n) in enumerate(skeys)]
    lp, rank, ti, tv, lg = eng.score_extend_batch(ss, [X[1700 + 90 * i:1700 + 90 * i + n] for i, (_, _, n) in enumerate(skeys)], nxt, top_n=3, want_logits=True)
    torch.cuda.synchronize()
    out["score"] = [cpu(t) for t in (lp, rank, ti, tv, lg)]
    # clone of a sequence with a partial last page, one teacher-forced step on both
    assert (200 + NEW) % 64
    cl = eng.seq_clone(s0, 200 + 24)
    hold("clone", cl)
    out["clone.logits"] = cpu(eng.decode_step_logits(cl, 7))
    out["clone.source"] = cpu(eng.decode_step_logits(s0, 7))
    # fan-out to 3 siblings from a prompt that does not end on a page boundary
    src = eng.seq_alloc(150 + NEW + 1)
    first = eng.prefill(src, X[1850:2000], want_logits=True)
    sib = eng.seq_fanout(src, 3, 150 + NEW + 1, [1, 2, 3], first)
    hold("fanout", src, *sib)
    out["fanout.ids"] = eng.decode_greedy_batch([src] + sib, NEW, None)
    # 16 sequences decoded together, then one batched teacher-forced step on the largest group one step takes
    glens = [5, 17, 60, 64, 33, 1, 100, 63, 128, 2, 77, 65, 31, 9, 90, 40]
    g16 = [eng.seq_alloc(n + NEW + 4) for n in glens]
    hold("group16", *g16)
    eng.prefill_batch(g16, [X[37 * i:37 * i + n] for i, n in enumerate(glens)])
    out["group16.ids"] = eng.decode_greedy_batch(g16, NEW, None)
    out["group.step_logits"] = cpu(eng.decode_step_logits_batch(g16[:group], [(3 * i + 1) % VOCAB for i in range(group)]))
    # a short beam search (the library clones and frees beams inside)
    bs = eng.seq_alloc(100 + 12)
    hold("beam", bs)
    first = eng.prefill(bs, X[1200:1300], want_logits=True)
    out["beam"] = eng.beam_search(bs, first, 3, 6, None, with_scores=True)
    torch.cuda.synchronize()
    return out, {name: eng.seq_pages(s) for name, s in live.items()}, list(live.values())


def free_all(eng, seqs):
    for s in seqs:
        eng.seq_free(s)


def pages_of(held):
    return {p for ps in held.values() for p in ps}


def same(a, b):
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("name", list(MODELS))
def test_a_pool_whose_low_pages_are_taken_computes_the_same_bits(name):
    eng, geo, page_elems, first_high = make_engine(name)
    try:
        info = eng.kv_info()
        total = info["total_pages"]
        assert total == info["free_pages"] == first_high + SPARE
        layer_stride = info["pool_bytes"] // (geo.layers * 2 * 2)                 # elements of one layer's slice of one pool
        assert layer_stride == total * page_elems > 1 << 31 and first_high * page_elems >= 1 << 31 > (first_high - 1) * page_elems
        gi = eng.decode_group_info()
        assert (gi["max_group"] == 16 and gi["any_size"] == 1) == MODELS[name]["mfma"], "this geometry was chosen for the other decode path"
        group = 16 if gi["any_size"] else gi["max_group"]
        X = (torch.randn((2048, geo.hidden), device=DEV, generator=torch.Generator(device=DEV).manual_seed(23)) * 0.5).to(bf)

        a, pages_a, seqs = scenario(eng, X, group)                                 # (a) the fresh pool
        free_all(eng, seqs)
        assert eng.kv_info()["free_pages"] == total
        assert max(p for ps in pages_a.values() for p in ps) < 1024 < first_high and all(pages_a.values()), "(a) was meant to run on low pages"
        assert len({tuple(x) for x in a["group16.ids"]}) > 1 and len(a["beam"][0]) == 6 and bool(torch.isfinite(a["score"][0]).all())

        fillers, low = [], set()                                                   # (b) every page below the threshold is held by a filler
        per = (geo.max_seq + 63) // 64
        while len(low) < first_high:
            assert len(fillers) * per < first_high + per, "the fillers do not reach the low pages"
            fillers.append(eng.seq_alloc(geo.max_seq))
            low |= {p for p in eng.seq_pages(fillers[-1]) if p < first_high}
        assert low == set(range(first_high))
        left = eng.kv_info()["free_pages"]
        assert left == total - len(fillers) * per and left >= 150
        b, pages_b, seqs_b = scenario(eng, X, group)
        lowest = min(pages_of(pages_b))
        assert lowest >= first_high and lowest * page_elems >= 1 << 31, f"(b) ran on page {lowest}, below {first_high}"
        assert eng.kv_info()["free_pages"] == left - len(pages_of(pages_b))
        print(f"[parity] {name}: {total} pages of {page_elems} elements per layer; (b) ran on pages {lowest} .. {max(p for ps in pages_b.values() for p in ps)} "
              f"(element offsets inside a layer from {lowest * page_elems}, 2^31 = {1 << 31}) behind {len(fillers)} fillers; (a) on pages 0 .. {max(p for ps in pages_a.values() for p in ps)}")

        free_all(eng, fillers)                                                     # (c) the fillers go first, (b)'s sequences last: their pages are on top of the stack
        free_all(eng, seqs_b)
        assert eng.kv_info()["free_pages"] == total
        c, pages_c, seqs = scenario(eng, X, group)
        free_all(eng, seqs)
        written = pages_of(pages_a) | pages_of(pages_b)
        assert pages_of(pages_c) <= written and pages_of(pages_c) == pages_of(pages_b), f"(c) ran on pages nobody wrote before: {sorted(pages_of(pages_c) - written)[:8]}"
        moved = [k for k in pages_b if pages_c[k] != pages_b[k]]
        assert len(moved) >= len(pages_b) - 2 and pages_c["prefill[0]"] != pages_b["prefill[0]"], "(c) was meant to give every sequence another sequence's dirty pages"

        for key in a:
            assert same(a[key], b[key]), f"{name}: {key} on pages above 2^31 elements differs from the fresh pool"
            assert same(a[key], c[key]), f"{name}: {key} on reused pages differs from the fresh pool"
        info = eng.kv_info()
        assert info["total_pages"] == info["free_pages"] == total, "pages leaked or double-freed"
        print(f"[parity] {name}: {len(a)} collected results bit-identical on the fresh pool, above 2^31 elements and on {len(pages_of(pages_c))} reused, dirty pages "
              f"({len(moved)} of {len(pages_b)} sequences on other pages than in (b))")
    finally:
        eng.close()
        torch.cuda.empty_cache()
