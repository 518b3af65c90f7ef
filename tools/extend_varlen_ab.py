"""A/B of the ragged extend prefill (gvl_prefill_extend_varlen) at full width: Phi-3.5-3.8B on synthetic weights, a 3 456-row shared prefix, N = 3 and 8 tails of
~100 rows each.  Three ways to prefill the N tails, alternating in one process, device-event times around the calls only (forks are opened outside the timed span):
  varlen 1     one Engine.prefill_extend_batch, gvl_debug_set("varlen_extend", 1): one RoPE/KV-append, one V^T and one attention launch per layer for the group
  varlen 0     the same call with per-sequence launches of the single-sequence extend kernels (GEMMs still shared)
  sequential   N Engine.prefill_extend calls (N streams of the decoder weights)
and checks that the three leave the same first tokens.
  python tools/extend_varlen_ab.py [rounds [forms]]          prints a markdown table (profiles/extend_varlen_ab.md holds a recorded one)
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/extend_varlen_ab.py 2 "varlen 1"          per-kernel times of ONE form, in a run of its own"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _gvl_bootstrap  # noqa
import torch
from grounded_video_llm_amd import engine as E, synth, weights as Wt

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
forms = tuple(sys.argv[2].split(",")) if len(sys.argv) > 2 else ("varlen 1", "varlen 0", "sequential")
assert set(forms) <= {"varlen 1", "varlen 0", "sequential"}, forms
dev, PREFIX = "cuda:0", 3456
geo = E.TowerGeometry(llm="phi3.5", max_seq=4096, max_prefill=3712, kv_pages=0, max_segs=1)
geo.rope_short, geo.rope_long = synth.longrope_factors(96)
eng = E.Engine(geo, dev, towers=("llm",))
W = synth.llm_weights("phi3", geo.hidden, geo.inter, geo.layers, geo.heads, geo.kv_heads, geo.vocab, True, seed="evl", device=dev)
eng.load_packed(Wt.pack_llm(W, "phi3", geo.layers, geo.heads, geo.kv_heads, geo.max_seq, geo.rope_theta, geo.rope_short, geo.rope_long)); del W
torch.cuda.empty_cache()
eng.finalize()
g = torch.Generator(device=dev); g.manual_seed(2)
prefix = (torch.randn((PREFIX, geo.hidden), device=dev, generator=g) * 0.5).to(torch.bfloat16)
base = eng.seq_alloc(PREFIX)
eng.prefill(base, prefix)
LENS = {3: (101, 86, 121), 8: (101, 86, 121, 97, 110, 93, 104, 88)}


def once(tails, how):
    seqs = [eng.seq_fork(base, PREFIX, PREFIX + t.shape[0] + 2) for t in tails]
    eng.debug_set("varlen_extend", 0 if how == "varlen 0" else 1)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    if how == "sequential":
        for s, t in zip(seqs, tails):
            eng.prefill_extend(s, t)
    else:
        eng.prefill_extend_batch(seqs, tails)
    t1.record()
    t1.synchronize()
    first = [eng.seq_read(s, 0, 1) for s in seqs]
    for s in seqs:
        eng.seq_free(s)
    return t0.elapsed_time(t1), first


print(f"| tails | form | ms (median of {rounds}) | min | max | first tokens equal to {forms[-1]}'s |\n|---|---|---|---|---|---|")
for n, lens in LENS.items():
    tails = [(torch.randn((k, geo.hidden), device=dev, generator=g) * 0.5).to(torch.bfloat16) for k in lens]
    ms, firsts = {f: [] for f in forms}, {}
    for f in forms:
        once(tails, f)                                          # warm-up
    for _ in range(rounds):
        for f in forms:                                         # alternating
            t, firsts[f] = once(tails, f)
            ms[f].append(t)
    for f in forms:
        v = sorted(ms[f])
        print(f"| {n} x ~{sum(lens) // n} rows | {f} | {v[len(v) // 2]:.2f} | {v[0]:.2f} | {v[-1]:.2f} | {firsts[f] == firsts[forms[-1]]} |", flush=True)
eng.debug_set("varlen_extend", 1)
eng.seq_free(base)
eng.close()
