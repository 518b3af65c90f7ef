"""A/B of teacher-forced scoring (gvl_score_extend_varlen) at full width: Phi-3.5-3.8B on synthetic weights, ONE clip's prompt of 3 456 shared rows + ~50 rows of
question text, 8 candidate answers of ~12 tokens.  Two routes to the 8 sums of log-probabilities, alternating in one process:
  score         the new path: one base prefill of the 3 456 shared rows, 8 forks, ONE Engine.score_extend_batch over the 8 tails (question rows + candidate); timed with and
                without the base prefill (a caller who scores several questions about a clip pays the base once)
  forward_loss  the only route without it: Engine.forward_loss of the whole spliced prompt per candidate, labels on the candidate's tokens (8 full prefills; its code is
                what it was before gvl_score_extend_varlen existed)
Device-event times around the calls (forward_loss synchronises inside; the events still bracket it); fork / free outside the timed span.  Also prints how far the two
routes' sums are apart (fp32 logits against forward_loss's bf16 logits).
  python tools/score_ab.py [rounds]                 prints a markdown table (profiles/score_ab.md holds a recorded one)
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/score_ab.py 3 score0|score8      the score route alone at top_n = 0 / 8, for per-kernel times in a run of its own"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _gvl_bootstrap  # noqa
import torch
from grounded_video_llm_amd import engine as E, scoring as SC, synth, weights as Wt

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
mode = sys.argv[2] if len(sys.argv) > 2 else "ab"
assert mode in ("ab", "score0", "score8"), mode
dev, PREFIX, QUESTION = "cuda:0", 3456, 50
CANDS = (12, 11, 13, 12, 10, 14, 12, 12)
# the A/B runs at Phi-3.5's own vocabulary (32 064): forward_loss's lm_head GEMM needs vocab % 4 == 0.  The profiler runs take the fine-tuned one (32 366 = + 302 temporal
# tokens), where the score tail's GEMM computes 32 352 columns and head_cols_kernel the 14 behind them.
geo = E.TowerGeometry(llm="phi3.5", max_seq=4096, max_prefill=3712, kv_pages=0, max_segs=1, vocab=32064 if mode == "ab" else 32366)
geo.rope_short, geo.rope_long = synth.longrope_factors(96)
eng = E.Engine(geo, dev, towers=("llm",))
W = synth.llm_weights("phi3", geo.hidden, geo.inter, geo.layers, geo.heads, geo.kv_heads, geo.vocab, True, seed="evl", device=dev)
eng.load_packed(Wt.pack_llm(W, "phi3", geo.layers, geo.heads, geo.kv_heads, geo.max_seq, geo.rope_theta, geo.rope_short, geo.rope_long)); del W
torch.cuda.empty_cache()
eng.finalize()
g = torch.Generator(device=dev); g.manual_seed(4)
rows = lambda n: (torch.randn((n, geo.hidden), device=dev, generator=g) * 0.5).to(torch.bfloat16)
prompt = rows(PREFIX + QUESTION)                       # the clip's visual rows + system prompt (shared), then the question
cands = [rows(c) for c in CANDS]                       # the candidates' embedding rows ...
cand_ids = [torch.randint(0, geo.vocab, (c,), generator=g, device=dev).tolist() for c in CANDS]     # ... and the ids they stand for
P = PREFIX + QUESTION
pairs = [SC.assemble(P, ids, PREFIX, geo.max_seq) for ids in cand_ids]
full = [torch.cat([prompt, c], 0) for c in cands]


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def score(top_n):
    """-> (ms of base prefill + scored pass, ms of the scored pass alone, the 8 sums of log-probabilities)"""
    a0, a1 = events(); b0, b1 = events()
    base = eng.seq_alloc(PREFIX)
    a0.record(); eng.prefill(base, prompt[:PREFIX]); a1.record()
    seqs = [eng.seq_fork(base, PREFIX, f.shape[0]) for f in full]
    b0.record()
    lp, rank, ti, tv = eng.score_extend_batch(seqs, [f[sl] for f, (sl, _) in zip(full, pairs)], [nxt for _, nxt in pairs], top_n)
    b1.record(); b1.synchronize()
    for s in seqs + [base]:
        eng.seq_free(s)
    out = SC.fold(cand_ids, lp.cpu().tolist(), rank.cpu().tolist())
    return a0.elapsed_time(a1) + b0.elapsed_time(b1), b0.elapsed_time(b1), [o.sum_logprob for o in out]


def forward_loss():
    t0, t1 = events()
    t0.record()
    sums = []
    for f, ids in zip(full, cand_ids):
        labels = [-100] * P + ids                       # HF's convention: aligned with the rows, shifted inside
        s, n = eng.forward_loss(f, labels)
        assert n == len(ids)
        sums.append(-s)
    t1.record(); t1.synchronize()
    return t0.elapsed_time(t1), sums


if mode != "ab":
    for _ in range(rounds):
        ms, tail_ms, _ = score(0 if mode == "score0" else 8)
        print(f"{mode}: base prefill + scored pass {ms:.2f} ms, scored pass alone {tail_ms:.2f} ms", flush=True)
else:
    score(0); score(8); forward_loss()                  # warm-up
    t = {"score, top_n 0": [], "score, top_n 8": [], "forward_loss x 8": []}
    tails = {"score, top_n 0": [], "score, top_n 8": []}
    for _ in range(rounds):                             # alternating
        for k in t:
            if k.startswith("score"):
                ms, tail_ms, s_new = score(0 if k.endswith("0") else 8)
                tails[k].append(tail_ms)
            else:
                ms, s_old = forward_loss()
            t[k].append(ms)
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"| route | ms (median of {rounds}) | min | max | of which the scored pass alone (median) |\n|---|---|---|---|---|")
    for k, v in t.items():
        print(f"| {k} | {med(v):.2f} | {min(v):.2f} | {max(v):.2f} | {med(tails[k]):.2f} |" if k in tails else f"| {k} | {med(v):.2f} | {min(v):.2f} | {max(v):.2f} | - |")
    rel = max(abs(a - b) / abs(b) for a, b in zip(s_new, s_old))
    print(f"\nsums of log-probabilities, score vs forward_loss: largest relative difference {rel:.2e} over {len(CANDS)} candidates "
          f"(ranking {'equal' if sorted(range(8), key=lambda i: -s_new[i]) == sorted(range(8), key=lambda i: -s_old[i]) else 'differs'})")
eng.close()
