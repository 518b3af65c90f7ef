"""Decode step time with log-probabilities off / chosen token only / top-8 (argmax_kernel's logprob modes, csrc/gvl_pick.hip): full-width Phi-3.5
(synthetic weights), the bench's decode context (3.5 k tokens at the measured steps), groups of B = 1 and 8 sequences; the three modes rotate
within one process (same box, same engine, same sequences), timed with device events around graph-replayed decode calls (gvl_decode_greedy_batch).
  python tools/decode_logprobs_ab.py [--reps 4] [--steps 32] [--batches 1,8]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _gvl_bootstrap  # noqa: E402,F401
import torch  # noqa: E402
from grounded_video_llm_amd import engine as E, synth, weights as Wt  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--steps", type=int, default=32)
ap.add_argument("--batches", default="1,8")
ap.add_argument("--hist", type=int, default=2048, help="ids generated before the measured steps")
ap.add_argument("--context", type=int, default=3519)
args = ap.parse_args()
dev = "cuda:0"
geo = E.TowerGeometry(llm="phi3.5", max_seq=4096, max_prefill=3712, kv_pages=0, max_segs=1)
geo.rope_short, geo.rope_long = synth.longrope_factors(96)
eng = E.Engine(geo, dev, towers=("llm",))
W = synth.llm_weights("phi3", geo.hidden, geo.inter, geo.layers, geo.heads, geo.kv_heads, geo.vocab, True, seed="d2e", device=dev)
eng.load_packed(Wt.pack_llm(W, "phi3", geo.layers, geo.heads, geo.kv_heads, geo.max_seq, geo.rope_theta, geo.rope_short, geo.rope_long)); del W
torch.cuda.empty_cache()
eng.finalize()
MODES = {"off": -1, "chosen": 0, "top8": 8}
S = args.context - args.hist                   # prompt rows: the history fills the rest of the context
g = torch.Generator(device=dev); g.manual_seed(1)
emb = (torch.randn((S, geo.hidden), device=dev, generator=g) * 0.5).to(torch.bfloat16)
print(f"phi3.5 full width, prompt {S} + history {args.hist} = context {args.context}; modes {MODES}", flush=True)
summary = {}
for B in [int(x) for x in args.batches.split(",")]:
    cap = S + args.hist + 3 * args.reps * args.steps + 3 * 4 + 8
    seqs = [eng.seq_alloc(cap) for _ in range(B)]
    for s in seqs:
        eng.seq_set_logprobs(s, -1)
    eng.prefill_batch(seqs, [emb] * B)
    eng.decode_greedy_batch(seqs, args.hist, None)           # fill the context up to the measured length (log-probabilities off)
    n_gen = args.hist
    names = list(MODES)
    for mode in names:                                       # warm-up of every launch sequence
        for s in seqs:
            eng.seq_set_logprobs(s, MODES[mode])
        eng.decode_greedy_batch(seqs, n_gen + 4, None); n_gen += 4
    res = {m: [] for m in names}
    for r in range(args.reps):
        for mode in names[r % 3:] + names[:r % 3]:           # rotate the order
            for s in seqs:
                eng.seq_set_logprobs(s, MODES[mode])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.decode_greedy_batch(seqs, n_gen + args.steps, None)
            e1.record(); torch.cuda.synchronize()
            n_gen += args.steps
            res[mode].append(e0.elapsed_time(e1) / args.steps)
    for s in seqs:
        eng.seq_free(s)
    med = {m: sorted(v)[len(v) // 2] for m, v in res.items()}
    summary[B] = med
    print(f"B={B:2d}  ms/step " + " | ".join(f"{m} {' '.join(f'{x:.4f}' for x in res[m])}" for m in names), flush=True)
    print(f"B={B:2d}  median off {med['off']:.4f} ms  " + "  ".join(f"{m} {med[m]:.4f} ms ({1e3 * (med[m] - med['off']):+.1f} us, {100 * (med[m] / med['off'] - 1):+.2f} %)"
                                                            for m in names[1:]), flush=True)
eng.close()
print("summary", {b: {m: round(v, 4) for m, v in med.items()} for b, med in summary.items()}, flush=True)
