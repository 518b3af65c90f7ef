"""What the groups of diverse beam search add to a beam step: full-width Phi-3.5 (synthetic weights), a prompt of ~3.5 k rows, num_beams 4 and 16, no eos (every
search runs max_new steps).  Per k three library searches alternate within one process on the same prefilled sequence: plain gvl_beam_search (this code path is the
parent commit's, untouched), gvl_group_beam_search with G = 2 and with G = k (one beam per group); wall time per search / steps.  The step is the batched decode
step; the groups add one normalise and per group a processor launch (g > 0), beam_rows_kernel and beam_group_merge_kernel -- about 3 G short dependent launches.
  python tools/group_beam_cost.py [--reps 3] [--steps 24] [--beams 4,16]"""
import argparse
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
ap.add_argument("--beams", default="4,16")
ap.add_argument("--context", type=int, default=3519)
ap.add_argument("--penalty", type=float, default=1.0)
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
print(f"phi3.5 full width, prompt {args.context} rows, {args.steps} steps per search, diversity_penalty {args.penalty}, decode groups {eng.decode_group_info()}", flush=True)
seq = eng.seq_alloc(args.context)
LP.apply_seq_options(eng, seq, LP.SeqOptions.OFF)
first = eng.prefill(seq, emb, want_logits=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0) / args.steps


summary = {}
for k in [int(x) for x in args.beams.split(",")]:
    paths = {"plain": lambda: eng.beam_search(seq, first, k, args.steps, None),
             "G=2": lambda: eng.group_beam_search(seq, first, k, 2, args.penalty, args.steps, None),
             f"G={k}": lambda: eng.group_beam_search(seq, first, k, k, args.penalty, args.steps, None)}
    ids = {n: f() for n, f in paths.items()}                 # warm-up of every launch sequence
    res = {n: [] for n in paths}
    names = list(paths)
    for r in range(args.reps):
        for n in names[r % 3:] + names[:r % 3]:
            out, ms = timed(paths[n])
            assert out == ids[n]
            res[n].append(ms)
    med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
    summary[k] = med
    print(f"k={k:2d}  ms/step " + " | ".join(f"{n} {' '.join(f'{x:.3f}' for x in res[n])}" for n in names), flush=True)
    print(f"k={k:2d}  median " + "  ".join(f"{n} {med[n]:.3f} ms ({100 * (med[n] / med['plain'] - 1):+.1f} %)" for n in names), flush=True)
eng.seq_free(seq)
eng.close()
print("summary", {k: {n: round(v, 3) for n, v in m.items()} for k, m in summary.items()}, flush=True)
