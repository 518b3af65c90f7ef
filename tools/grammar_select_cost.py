"""What a decoding grammar costs per token selection (csrc/gvl_logits.hip, the GRAMMAR stage: a serial walk of thread 0 over the L generated ids, recomputed at
every step), next to the processor launch it rides in and to one decode step.  Full-width Phi-3.5 (synthetic weights), V = 32366.
  * the processor launch on its own (gvl_op_logits_process_ex / _rules), timed by the library's own events around the launch (gvl_prof): one row of the launch has
    the "ordered" grounding grammar and a history of L ids it accepts -- against the yardstick, the same launch with a 300-id suppress list on that row instead
    (logits_process_kernel's rules instantiation); B = 1 and 16 rows, L = 12, 64, 1024, 8192;
  * one decode step of B = 1 and 16 sequences behind a 3 k-token context (graph-replayed gvl_decode_greedy_batch, device events), grammar off;
  * the launches of one 8-step decode chunk per family (gvl_prof_read), default settings: the default path must launch what it launched before.
The suppress-list rows and the decode figures need nothing new, so the tool also runs on a build without grammars (its table then has no grammar column).
  python tools/grammar_select_cost.py [--reps 200] [--out FILE]"""
import argparse
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _gvl_bootstrap  # noqa: E402,F401
import torch  # noqa: E402
from grounded_video_llm_amd import engine as E, logits as LP, synth, weights as Wt  # noqa: E402
from grounded_video_llm_amd.model import SyntheticTokenizer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--context", type=int, default=3072)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = "cuda:0"
geo = E.TowerGeometry(llm="phi3.5", max_seq=4096, max_prefill=3712, kv_pages=0, max_segs=1)
geo.rope_short, geo.rope_long = synth.longrope_factors(96)
eng = E.Engine(geo, dev, towers=("llm",))
W = synth.llm_weights("phi3", geo.hidden, geo.inter, geo.layers, geo.heads, geo.kv_heads, geo.vocab, True, seed="d2e", device=dev)
eng.load_packed(Wt.pack_llm(W, "phi3", geo.layers, geo.heads, geo.kv_heads, geo.max_seq, geo.rope_theta, geo.rope_short, geo.rope_long)); del W
torch.cuda.empty_cache()
eng.finalize()
V = geo.vocab
tok = SyntheticTokenizer(V, 300)
eos = tok.eos_token_id
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


has_grammar = hasattr(eng, "grammar_create")
gid = None
if has_grammar:
    from grounded_video_llm_amd import grammar as GR
    gr = GR.grounding_grammar(tok, 300, eos, "ordered")
    gid = eng.grammar_create(gr)
rng = random.Random(3)
T0 = tok.tok2id["<0>"]


def history(n):
    """n ids the ordered grammar accepts: words, with a timestamp pair (start <= end) every 16 ids"""
    h = [3 + rng.randrange(T0 - 3) for _ in range(n)]
    for i in range(4, n - 1, 16):
        s = rng.randrange(301)
        h[i], h[i + 1] = T0 + s, T0 + rng.randrange(s, 301)
    return h


sup = eng.rules_create(LP.TokenRules(suppress=tuple(rng.randrange(V) for _ in range(300))))
g = torch.Generator(device=dev); g.manual_seed(1)


def launch_us(B, L, **kw):
    """microseconds of one processor launch of B rows (row 0 carries `kw`, every row a history of L ids), by the events the library puts around it"""
    x = torch.randn((B, V), device=dev, generator=g)
    hists = [history(L) for _ in range(B)]
    if has_grammar:
        assert gr.walk(hists[0])[0]
    per_row = {k: [v] + [None] * (B - 1) for k, v in kw.items()}
    for _ in range(5):
        eng.op_logits_process(x.clone(), hists, 1.0, 0, 0, eos, **per_row)
    eng.prof_enable(True)
    for _ in range(args.reps):
        eng.op_logits_process(x.clone(), hists, 1.0, 0, 0, eos, **per_row)
    ms, n, _ = eng.prof_read(4)
    eng.prof_enable(False)
    assert n == args.reps, (n, args.reps)
    return 1e3 * ms / n


say(f"processor launch, V = {V}, us per launch (mean of {args.reps}; library events around the launch)")
say(f"{'B':>3} {'L':>5} {'suppress row':>13}" + (f" {'grammar row':>12} {'delta':>8}" if has_grammar else ""))
table = {}
for B in (1, 16):
    for L_ in (12, 64, 1024, 8192):
        a = launch_us(B, L_, rules=sup)
        b = launch_us(B, L_, grammar=gid) if has_grammar else None
        table[(B, L_)] = (a, b)
        say(f"{B:>3} {L_:>5} {a:>13.2f}" + (f" {b:>12.2f} {b - a:>+8.2f}" if has_grammar else ""))
eng.rules_destroy(sup)

# one decode step at the same B, and what one decode chunk launches
emb = (torch.randn((args.context, geo.hidden), device=dev, generator=g) * 0.5).to(torch.bfloat16)
for B in (1, 16):
    seqs = [eng.seq_alloc(args.context + 3 * args.steps + 64) for _ in range(B)]
    for i in range(0, B, 4):
        eng.prefill_batch(seqs[i:i + 4], [emb] * len(seqs[i:i + 4]))
    n_gen = 16
    eng.decode_greedy_batch(seqs, n_gen, None)
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.decode_greedy_batch(seqs, n_gen + args.steps, None)
        e1.record(); torch.cuda.synchronize()
        n_gen += args.steps
        ts.append(1e3 * e0.elapsed_time(e1) / args.steps)
    step = sorted(ts)[1]
    say(f"decode step, B = {B:2d}, context {args.context}: {step:.1f} us (median of 3 x {args.steps} graph-replayed steps: {' '.join(f'{t:.1f}' for t in ts)})")
    for L_ in (12, 64, 1024, 8192):
        a, b = table[(B, L_)]
        if b is not None:
            say(f"    L = {L_:>4}: grammar row {b:.2f} us = {100 * b / step:.2f} % of the step; over the suppress row {b - a:+.2f} us = {100 * (b - a) / step:+.2f} %")
    eng.prof_enable(True)
    eng.decode_steps(seqs, 8)
    fam = {name: int(eng.prof_read(cat)[1]) for name, cat in (("gemm", 0), ("attn", 1), ("gemv", 2), ("decode_attn", 3), ("other", 4))}
    eng.prof_enable(False)
    say(f"launches of one 8-step decode chunk, B = {B:2d}, default settings: {fam}")
    for s in seqs:
        eng.seq_free(s)
if gid is not None:
    eng.grammar_destroy(gid)
eng.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
