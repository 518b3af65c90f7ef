"""What contrastive search costs per token next to greedy decoding: full-width Phi-3.5 (synthetic weights), a prompt of ~3.5 k rows, no eos (every run makes `steps`
tokens).  Within one process, alternating: greedy decoding of a clone of the prefilled sequence (the parent commit's code path, untouched), gvl_contrastive_search with
top_k 4 and 6 on the keep-hidden twin of that sequence, and -- to split the search's step -- a bare batched teacher-forced step of k clones (what the candidates cost
without clones, candidate launches and ranking).  Wall time per token, `reps` repetitions each; then ONE profiled run of each (gvl_prof): the ranking launch of a
step has its own category (GVL_PROF_CS_RANK: rank + finish kernels), the step's k - 1 clones are one bracket (GVL_PROF_CS_CLONE), and everything a contrastive step
adds to the k-row decode step (clones, candidate launches, the rows' normalisation, rank + finish) is the difference of GVL_PROF_OTHER + GVL_PROF_CS_RANK between the
search and the bare steps.
--greedy-only times the greedy path alone and touches nothing this mode added: the same file, copied into a checkout of the parent commit, gives the yardstick.
  python tools/contrastive_cost.py [--reps 3] [--steps 24] [--topk 4,6] [--context 3519] [--greedy-only]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _gvl_bootstrap  # noqa: E402,F401
import torch  # noqa: E402
from grounded_video_llm_amd import engine as E, logits as LP, synth, weights as Wt  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--steps", type=int, default=24)
ap.add_argument("--topk", default="4,6")
ap.add_argument("--context", type=int, default=3519)
ap.add_argument("--alpha", type=float, default=0.6)
ap.add_argument("--greedy-only", action="store_true")
args = ap.parse_args()
dev = "cuda:0"
geo = E.TowerGeometry(llm="phi3.5", max_seq=4096, max_prefill=3712, kv_pages=0, max_segs=1)
geo.rope_short, geo.rope_long = synth.longrope_factors(96)
eng = E.Engine(geo, dev, towers=("llm",))
W = synth.llm_weights("phi3", geo.hidden, geo.inter, geo.layers, geo.heads, geo.kv_heads, geo.vocab, True, seed="d2e", device=dev)
eng.load_packed(Wt.pack_llm(W, "phi3", geo.layers, geo.heads, geo.kv_heads, geo.max_seq, geo.rope_theta, geo.rope_short, geo.rope_long)); del W
torch.cuda.empty_cache()
eng.finalize()
g = torch.Generator(device=dev); g.manual_seed(1)
emb = (torch.randn((args.context, geo.hidden), device=dev, generator=g) * 0.5).to(torch.bfloat16)
cap = args.context + args.steps + 2
print(f"phi3.5 full width, prompt {args.context} rows, {args.steps} tokens per run, penalty_alpha {args.alpha}, decode groups {eng.decode_group_info()}", flush=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def prefill_ms(keep_hidden):
    s = eng.seq_alloc(cap)
    LP.apply_seq_options(eng, s, LP.SeqOptions.OFF)
    if keep_hidden:
        eng.seq_keep_hidden(s)
    try:
        return timed(lambda: eng.prefill(s, emb))[1]
    finally:
        eng.seq_free(s)


def greedy():
    """a fresh prefill (outside the timed region: it selects the first id), then `steps` greedy decode steps; returns (ids, ms)"""
    c = eng.seq_alloc(cap)
    LP.apply_seq_options(eng, c, LP.SeqOptions.OFF)
    try:
        eng.prefill(c, emb)
        return timed(lambda: eng.decode_greedy(c, args.steps + 1, None))
    finally:
        eng.seq_free(c)


if args.greedy_only:
    first_ids = greedy()[0]                                  # warm-up
    runs = []
    for r in range(args.reps):
        out, ms = greedy()
        assert out == first_ids
        runs.append(ms / args.steps)
    m = sorted(runs)[len(runs) // 2]
    print(f"{'greedy':>22}: {m:8.3f} ms per token ({1e3 / m:7.1f} tokens/s)   runs {[round(x, 3) for x in runs]}   prefill {prefill_ms(False):.1f} ms", flush=True)
    sys.exit(0)

prefill_ms(False); prefill_ms(True)                          # warm-up
ms_plain, ms_keep = prefill_ms(False), prefill_ms(True)
keep = eng.seq_alloc(cap)
LP.apply_seq_options(eng, keep, LP.SeqOptions.OFF)
eng.seq_keep_hidden(keep)
first = eng.prefill(keep, emb, want_logits=True)
src = eng.seq_alloc(cap)
LP.apply_seq_options(eng, src, LP.SeqOptions.OFF)
eng.prefill(src, emb)
print(f"prefill of {args.context} rows: plain {ms_plain:.1f} ms, keep-hidden (no last-layer tail + bank append) {ms_keep:.1f} ms", flush=True)


def bare_steps(k):
    cl = [eng.seq_clone(src, cap) for _ in range(k)]
    try:
        for s in range(args.steps):
            eng.decode_step_logits_batch(cl, [7 + s + i for i in range(k)])
        torch.cuda.synchronize()
    finally:
        for c in cl:
            eng.seq_free(c)


ks = [int(x) for x in args.topk.split(",")]
paths = {}
for k in ks:
    paths[f"contrastive k={k}"] = (lambda k=k: eng.contrastive_search(keep, first, k, args.alpha, args.steps, None))
    paths[f"bare {k}-row steps"] = (lambda k=k: bare_steps(k))
ids = {n: f() for n, f in paths.items()}                     # warm-up of every launch sequence
ids["greedy"] = greedy()[0]
names = ["greedy"] + list(paths)
res = {n: [] for n in names}
for r in range(args.reps):
    for n in names[r % len(names):] + names[:r % len(names)]:
        out, ms = greedy() if n == "greedy" else timed(paths[n])
        assert out == ids[n]
        res[n].append(ms / args.steps)
med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
for n in names:
    print(f"{n:>22}: {med[n]:8.3f} ms per token ({1e3 / med[n]:7.1f} tokens/s)   runs {[round(x, 3) for x in res[n]]}", flush=True)

prof = {}
for n in names:
    if n == "greedy":
        continue
    eng.prof_enable(True)
    paths[n]()
    prof[n] = {c: eng.prof_read(i) for i, c in enumerate(("gemm", "attn", "gemv", "decode_attn", "other", "cs_rank", "cs_clone"))}
    eng.prof_enable(False)
for k in ks:
    a, b = prof[f"contrastive k={k}"], prof[f"bare {k}-row steps"]
    d_ms = (a["other"][0] + a["cs_rank"][0] - b["other"][0]) / args.steps
    d_n = (a["other"][1] + a["cs_rank"][1] - b["other"][1]) / args.steps
    print(f"k={k}: rank launch (rank + finish kernels) {a['cs_rank'][0] / a['cs_rank'][1] * 1e3:.1f} us per step ({a['cs_rank'][1]} records); the {k - 1} clones of a step "
          f"{a['cs_clone'][0] / a['cs_clone'][1] * 1e3:.1f} us per step ({a['cs_clone'][1]} brackets)", flush=True)
    print(f"k={k}: per step the search adds {d_n:.1f} launches / {d_ms * 1e3:.1f} us of GVL_PROF_OTHER + GVL_PROF_CS_RANK (clones, candidates, normalisation, rank + finish) to the bare "
          f"{k}-row step; projections {a['gemv'][0] / args.steps:.3f} vs {b['gemv'][0] / args.steps:.3f} ms, decode attention {a['decode_attn'][0] / args.steps:.3f} vs "
          f"{b['decode_attn'][0] / args.steps:.3f} ms per step", flush=True)
print("JSON " + json.dumps({"context": args.context, "steps": args.steps, "ms_per_token": med, "prefill_ms": {"plain": ms_plain, "keep_hidden": ms_keep},
                            "prof": {n: {c: list(v) for c, v in p.items()} for n, p in prof.items()}}))
