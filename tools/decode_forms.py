"""Greedy decode in every form of the decode step (csrc/gvl_decode_plan.h), with decode_graph off so that every launch is visible, for a kernel trace:
    rocprofv3 --kernel-trace --stats -d <out> -- python tools/decode_forms.py [tree]
Three 2-layer Phi models -- the tiny one (hidden 64: VALU path), hidden 512 (the smallest with the fused RMSNorm), full width (hidden 3072) -- each decoding groups of
1, 3, 5 and 16 sequences (the VALU path takes them as 1; 2 + 1; 4 + 1; 4 x 4) for 6 tokens, then one teacher-forced step whose logits are hashed.
`tree` (default: this one) is the checkout whose library runs, or GVL_LIB_PATH names another build of the library: the same script traces two builds, whose per-kernel
dispatch counts, ids and logits hashes must then be equal (profiles/decode_plan_dispatches.md).
    python tools/decode_forms.py [tree] --time
instead times the eager (decode_graph = 0) single-sequence decode of each model, 3 runs of 64 tokens: tokens/s is host-bound there, which is what a change of
decode_step's host code would move."""
import hashlib
import os
import sys
import time

args = [a for a in sys.argv[1:] if not a.startswith("--")]
ROOT = os.path.abspath(args[0]) if args else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402
from gpu_util import DEV, bf, llm_engine, tiny_geo  # noqa: E402
from grounded_video_llm_amd import lib, synth  # noqa: E402

MODELS = (dict(hidden=64, inter=128, heads=4, vocab=100), dict(hidden=512, inter=512, heads=4, vocab=128), dict(hidden=3072, inter=8192, heads=32, vocab=512))
NEW = 6
print("library:", lib.LIB_PATH)
for m in MODELS:
    hid, heads = m["hidden"], m["heads"]
    short, long = synth.longrope_factors(hid // heads)
    geo = tiny_geo(llm="phi3.5", hidden=hid, inter=m["inter"], layers=2, heads=heads, kv_heads=heads, vocab=m["vocab"], max_seq=256, max_prefill=128, kv_pages=48,
                   rope_short=short, rope_long=long)
    eng = llm_engine(geo, synth.llm_weights("phi3", hid, m["inter"], 2, heads, heads, m["vocab"], True, seed="decode_forms", device=DEV))
    eng.debug_set("decode_graph", 0)
    g = torch.Generator(device=DEV); g.manual_seed(9)
    pool = (torch.randn((512, hid), device=DEV, generator=g) * 0.5).to(bf)
    info = eng.decode_group_info()
    if "--time" in sys.argv:
        rates = []
        for _ in range(3):
            s = eng.seq_alloc(100)
            eng.prefill(s, pool[:20])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids = eng.decode_greedy(s, 65, None)
            rates.append((len(ids) - 1) / (time.perf_counter() - t0))
            eng.seq_free(s)
        print(f"hidden {hid}: eager single-sequence decode", " ".join(f"{r:.1f}" for r in rates), "tokens/s")
        eng.close()
        continue
    for n in (1, 3, 5, 16):
        seqs = [eng.seq_alloc(5 + 4 * i + NEW + 2) for i in range(n)]
        for i, s in enumerate(seqs):
            eng.prefill(s, pool[13 * i:13 * i + 5 + 4 * i])
        ids = eng.decode_greedy_batch(seqs, NEW, None)
        rows = []
        for o in range(0, n, info["max_group"]):               # one teacher-forced step of the group, in steps of a size the path takes
            part = seqs[o:o + info["max_group"]]
            if info["any_size"] or len(part) in (1, 2, 4):
                rows.append(eng.decode_step_logits_batch(part, [7] * len(part)))
            else:
                rows += [eng.decode_step_logits(s, 7)[None] for s in part]
        h = hashlib.sha256(torch.cat(rows).cpu().numpy().tobytes()).hexdigest()[:16]
        print(f"hidden {hid} group {n}: ids {ids} logits sha256 {h}")
        for s in seqs:
            eng.seq_free(s)
    torch.cuda.synchronize()
    eng.close()
