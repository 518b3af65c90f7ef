"""Beam search per step, host path against library path: full-width Phi-3.5 (synthetic weights), a prompt of ~3.5 k rows, num_beams 4 and 16, no eos
(every search runs max_new steps).  Host path = beam.py's bookkeeping over gvl_seq_clone + gvl_decode_step_logits_batch with torch's log-softmax / top-2k
and a .tolist() per step (model.beam_generate_ids' stepping); library path = gvl_beam_search (its own candidate kernels, candidates in host-mapped memory).
The two alternate within one process on the same prefilled sequence; wall time per search / steps.  Under `rocprofv3 --kernel-trace --stats -- python
tools/beam_search_ab.py --reps 1` the stats table shows the three kernels (beam_rows_kernel, beam_merge_kernel, beam_normalize_kernel) next to the
at::native kernels of the host path.
  python tools/beam_search_ab.py [--reps 3] [--steps 24] [--beams 4,16] [--processors]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _gvl_bootstrap  # noqa: E402,F401
import torch  # noqa: E402
from grounded_video_llm_amd import beam as B, engine as E, logits as LP, synth, weights as Wt  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--steps", type=int, default=24)
ap.add_argument("--beams", default="4,16")
ap.add_argument("--context", type=int, default=3519)
ap.add_argument("--processors", action="store_true", help="no_repeat_ngram_size 2 on both paths (normalize + logits_process + candidates on the library path)")
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
procs = LP.Processors(1.0, 2, 0, -1) if args.processors else None
gi = eng.decode_group_info()
print(f"phi3.5 full width, prompt {args.context} rows, {args.steps} steps per search, processors {'on' if procs else 'off'}, decode groups {gi}", flush=True)
seq = eng.seq_alloc(args.context)
LP.apply_seq_options(eng, seq, LP.SeqOptions.OFF)
first = eng.prefill(seq, emb, want_logits=True)
cap = min(args.context + args.steps + 1, geo.max_seq)


def host_search(k):
    """model.beam_generate_ids' stepping from a clone of the prefilled sequence"""
    beams, fresh = [eng.seq_clone(seq, cap)], []
    process = None
    if procs is not None:
        def process(histories, logprobs):
            return eng.op_logits_process(logprobs.float().contiguous(), histories, *procs.args())
    try:
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
            if len(beams) <= gi["max_group"] and (gi["any_size"] or len(beams) in (1, 2, 4)):
                return eng.decode_step_logits_batch(beams, toks)
            return torch.stack([eng.decode_step_logits(s_, t) for s_, t in zip(beams, toks)])
        return B.beam_search(step, first, k, args.steps, None, 1.0, False, None, process=process)
    finally:
        for s_ in set(x for x in list(beams) + fresh if x is not None):
            eng.seq_free(s_)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0) / args.steps


summary = {}
for k in [int(x) for x in args.beams.split(",")]:
    paths = {"host": lambda: host_search(k), "library": lambda: eng.beam_search(seq, first, k, args.steps, None, processors=procs)}
    ids = {n: f() for n, f in paths.items()}                 # warm-up of both launch sequences
    res = {n: [] for n in paths}
    names = list(paths)
    for r in range(args.reps):
        for n in names[r % 2:] + names[:r % 2]:
            out, ms = timed(paths[n])
            assert out == ids[n]
            res[n].append(ms)
    med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
    summary[k] = med
    print(f"k={k:2d}  ms/step " + " | ".join(f"{n} {' '.join(f'{x:.3f}' for x in res[n])}" for n in names) + f" | same ids: {ids['host'] == ids['library']}", flush=True)
    print(f"k={k:2d}  median host {med['host']:.3f} ms  library {med['library']:.3f} ms ({100 * (med['library'] / med['host'] - 1):+.1f} %)", flush=True)
eng.seq_free(seq)
eng.close()
print("summary", {k: {n: round(v, 3) for n, v in m.items()} for k, m in summary.items()}, flush=True)
