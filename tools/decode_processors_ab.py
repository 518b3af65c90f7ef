"""Decode step time with HF's logits processors off vs on (csrc/gvl_logits.hip): full-width Phi-3.5 (synthetic weights), the bench's decode
context (3.5 k tokens at the measured steps), a 2048-id generated history, groups of B = 1 and 8 sequences; off / on alternate within one
process (same box, same engine, same sequences), timed with device events around graph-replayed decode calls (gvl_decode_greedy_batch).
  on = repetition_penalty 1.2 + no_repeat_ngram_size 3 (+ min_new_tokens 0: no eos in the run)
  python tools/decode_processors_ab.py [--reps 4] [--steps 32] [--batches 1,8]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _gvl_bootstrap  # noqa: E402,F401
import torch  # noqa: E402
from grounded_video_llm_amd import engine as E, logits as LP, synth, weights as Wt  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--steps", type=int, default=32)
ap.add_argument("--batches", default="1,8")
ap.add_argument("--hist", type=int, default=2048)
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
ON = LP.Processors(penalty=1.2, ngram=3)
S = args.context - args.hist                   # prompt rows: the history fills the rest of the context
g = torch.Generator(device=dev); g.manual_seed(1)
emb = (torch.randn((S, geo.hidden), device=dev, generator=g) * 0.5).to(torch.bfloat16)
print(f"phi3.5 full width, prompt {S} + history {args.hist} = context {args.context}; on = {ON}", flush=True)
summary = {}
for B in [int(x) for x in args.batches.split(",")]:
    cap = S + args.hist + 2 * args.reps * args.steps + args.steps + 8
    seqs = [eng.seq_alloc(cap) for _ in range(B)]
    for s in seqs:
        eng.seq_set_processors(s, *LP.OFF.args())
    eng.prefill_batch(seqs, [emb] * B)
    eng.decode_greedy_batch(seqs, args.hist, None)           # the history: 2048 generated ids per sequence (processors off)
    n_gen = args.hist
    for mode in ("off", "on"):                               # warm-up of both launch sequences
        for s in seqs:
            eng.seq_set_processors(s, *(ON if mode == "on" else LP.OFF).args())
        eng.decode_greedy_batch(seqs, n_gen + 4, None); n_gen += 4
    res = {"off": [], "on": []}
    for r in range(args.reps):
        for mode in (("off", "on") if r % 2 == 0 else ("on", "off")):
            for s in seqs:
                eng.seq_set_processors(s, *(ON if mode == "on" else LP.OFF).args())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.decode_greedy_batch(seqs, n_gen + args.steps, None)
            e1.record(); torch.cuda.synchronize()
            n_gen += args.steps
            res[mode].append(e0.elapsed_time(e1) / args.steps)
    for s in seqs:
        eng.seq_free(s)
    off, on = sorted(res["off"]), sorted(res["on"])
    mo, mn = off[len(off) // 2], on[len(on) // 2]
    summary[B] = (mo, mn)
    print(f"B={B:2d}  ms/step off {' '.join(f'{x:.4f}' for x in res['off'])} | on {' '.join(f'{x:.4f}' for x in res['on'])}", flush=True)
    print(f"B={B:2d}  median off {mo:.4f} ms  on {mn:.4f} ms  delta {1e3 * (mn - mo):+.1f} us/step ({100 * (mn / mo - 1):+.2f} %)", flush=True)
eng.close()
print("summary", {b: {"off_ms": round(v[0], 4), "on_ms": round(v[1], 4), "pct": round(100 * (v[1] / v[0] - 1), 2)} for b, v in summary.items()}, flush=True)
