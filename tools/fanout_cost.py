"""What n sampled answers to ONE question about ONE 96-frame clip cost: generate(num_return_sequences=n) -- one vision encode, one prefill, gvl_seq_fanout, the n
answers decoded together -- against n separate generate() calls on the same commit (what a user did before, and what HF's prompt expansion costs in prefills).
Phi-3.5 geometry, synthetic weights, a prompt of the benchmark's size (12 x 285 visual rows + about 100 text tokens), 12 new tokens per answer (min_new_tokens keeps
eos away so that every answer has 12).  The two forms alternate inside one process; per form the mean and the spread of the timed calls are printed as a markdown table
(profiles/fanout_cost.md holds one run).  The structural claim -- one vision encode and one prefill per prompt whatever n is -- is read off gvl_prof_read's launch counts
in a separate, untimed pass.
    python tools/fanout_cost.py [--n 1 4 8 16] [--reps 5]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _gvl_bootstrap  # noqa
import torch
from grounded_video_llm_amd import engine as E, lib as L, synth
from grounded_video_llm_amd.model import LLAVA_NEXT_VIDEO, SyntheticTokenizer

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="+", default=[1, 4, 8, 16])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--new-tokens", type=int, default=12)
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"

dev = "cuda:0"
geo = E.TowerGeometry(llm="phi3.5", max_seq=4608, max_prefill=4096, kv_pages=0)
geo.rope_short, geo.rope_long = synth.longrope_factors(96)
sd = {"vision_tower": synth.clip_weights(seed="fc.clip", device=dev), "video_encoder": synth.iv2_weights(frames=8, seed="fc.iv2", device=dev),
      "projectors": synth.projector_weights("phi3.5", seed="fc.proj", device=dev), "language_model": synth.llm_weights("phi3", seed="fc.llm", device=dev)}
tok = SyntheticTokenizer(geo.vocab, 300)
model = LLAVA_NEXT_VIDEO(stage="sft", max_txt_len=512, num_frames=96, num_segs=12, llm="phi3.5", geometry=geo, tokenizer=tok, state_dicts=sd, device=dev)
del sd
torch.cuda.empty_cache()
g = torch.Generator(device=dev); g.manual_seed(3)
prompt = " ".join(f"s{i}" for i in range(34)) + " <image> " + " ".join(f"q{i}" for i in range(64))
samples = {"prompts": [prompt], "spatial_pixel_values": torch.randn((1, 12, 3, 336, 336), device=dev, generator=g),
           "temporal_pixel_values": torch.randn((1, 96, 3, 224, 224), device=dev, generator=g), "video_ids": ["v"]}
T = args.new_tokens
kw = dict(do_sample=True, num_beams=1, temperature=0.7, top_k=50, max_new_tokens=T, min_new_tokens=T, return_dict_in_generate=True)
eng = model.engine


def fanned(n):
    return model.generate(samples, seed=11, num_return_sequences=n, **kw).sequences


def separate(n):
    return [model.generate(samples, seed=11 + j, **kw).sequences[0] for j in range(n)]


def clock(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def launches():
    return {name: eng.prof_read(cat)[1] for name, cat in (("gemm", L.PROF_GEMM), ("attn", L.PROF_ATTN), ("gemv", L.PROF_GEMV), ("decode_attn", L.PROF_DECODE_ATTN))}


def counted(fn, n):
    a = launches()
    fn(n)
    b = launches()
    return {k: b[k] - a[k] for k in a}


rows = []
for n in args.n:
    clock(fanned, n); clock(separate, n)                                 # every shape of the timed window, warm
    tf, ts = [], []
    for _ in range(args.reps):                                           # alternating: both forms see the same neighbours on the host
        t, out = clock(fanned, n); tf.append(t)
        assert len(out) == n and all(len(s) == T for s in out)
        t, out = clock(separate, n); ts.append(t)
        assert len(out) == n and all(len(s) == T for s in out)
    mean = lambda v: sum(v) / len(v)
    rows.append((n, mean(tf), min(tf), max(tf), mean(ts), min(ts), max(ts)))
    print(f"[fanout] n={n}: generate(num_return_sequences=n) {mean(tf):.1f} ms ({min(tf):.1f} .. {max(tf):.1f}) | n generate() calls {mean(ts):.1f} ms "
          f"({min(ts):.1f} .. {max(ts):.1f}) | ratio {mean(ts) / mean(tf):.2f}", flush=True)

# structure: launch counts of the vision + prefill families (GEMM, attention) do not depend on n; the decode families do.  Eager steps: a replayed graph's launches
# are not bracketed by the profiler's events.
eng.debug_set("decode_graph", 0)
eng.prof_enable(True)
counts = {("fanned", n): counted(fanned, n) for n in (1, max(args.n))}
counts[("separate", max(args.n))] = counted(separate, max(args.n))
eng.prof_enable(False)
eng.debug_set("decode_graph", 1)
nmax = max(args.n)
one, many, sep = counts[("fanned", 1)], counts[("fanned", nmax)], counts[("separate", nmax)]
# ONE vision encode and ONE prefill whatever n is, against n of each
structure_ok = many["gemm"] == one["gemm"] and many["attn"] == one["attn"] and sep["gemm"] == nmax * one["gemm"] and sep["attn"] == nmax * one["attn"]

print(f"\nOne MI355X, Phi-3.5 geometry, synthetic weights, one 96-frame clip, a prompt of {eng.tokens_per_seg * 12} visual + {len(model.tokenizer_image_token(prompt)) - 1} "
      f"text rows, {T} new tokens per answer, temperature 0.7, top_k 50; mean (min .. max) of {args.reps} calls per form, the two forms alternating, one warm-up call each.\n")
print("| n | generate(num_return_sequences=n), ms | n generate() calls, ms | ratio |")
print("|---|---|---|---|")
for n, a, alo, ahi, b, blo, bhi in rows:
    print(f"| {n} | {a:.1f} ({alo:.1f} .. {ahi:.1f}) | {b:.1f} ({blo:.1f} .. {bhi:.1f}) | {b / a:.2f} |")
print("\nLaunches per call (gvl_prof_read; eager decode steps):\n")
print("| form | GEMM | attention (towers + prefill) | decode projections | decode attention |")
print("|---|---|---|---|---|")
for name, c in ((f"generate(num_return_sequences=1)", one), (f"generate(num_return_sequences={nmax})", many), (f"{nmax} generate() calls", sep)):
    print(f"| {name} | {c['gemm']} | {c['attn']} | {c['gemv']} | {c['decode_attn']} |")
print(f"\nOne vision encode and one prefill per prompt whatever n is (GEMM and attention launches of n = {nmax} equal those of n = 1; {nmax} calls take {nmax} times as many): "
      f"{'confirmed' if structure_ok else 'NOT confirmed'}")
sys.exit(0 if structure_ok else 1)
