"""One prefill per launch form on a tiny 2-layer Phi model (hidden 256, 4 heads of 64, rope_orig_max_pos = 200), for a kernel trace:
    rocprofv3 --kernel-trace --stats -d <out> -- python tools/prefill_forms.py [tree]
single; uniform 3 x 64 (BATCHED); ragged under varlen_attn 1 / 2 / 0; a group behind prefixes under varlen_extend 1 / 0; a group that straddles rope_orig_max_pos.
`tree` (default: this one) is the checkout whose library runs: the same script traces two trees, whose per-kernel dispatch counts must then be equal name by name
(profiles/prefill_plan_dispatches.md)."""
import os
import sys

ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402
from gpu_util import DEV, bf, llm_engine, tiny_geo  # noqa: E402
from grounded_video_llm_amd import lib, synth  # noqa: E402

short, long = synth.longrope_factors(64)
geo = tiny_geo(llm="phi3.5", hidden=256, inter=512, layers=2, heads=4, kv_heads=4, vocab=400, max_seq=1024, max_prefill=768, kv_pages=128, rope_short=short, rope_long=long,
               rope_orig_max_pos=200)
eng = llm_engine(geo, synth.llm_weights("phi3", 256, 512, 2, 4, 4, 400, True, seed="prefill_forms", device=DEV))
g = torch.Generator(device=DEV); g.manual_seed(5)
pool = (torch.randn((2048, 256), device=DEV, generator=g) * 0.5).to(bf)
eng.debug_set("prefill_group", 8)
first = []


def fresh(lens, run):
    seqs = [eng.seq_alloc(n + 2) for n in lens]
    run(seqs, [pool[17 * i:17 * i + n] for i, n in enumerate(lens)])
    first.append([eng.seq_read(s, 0, 1) for s in seqs])
    for s in seqs:
        eng.seq_free(s)


def behind(base, members):
    seqs = [eng.seq_fork(base, p, p + n + 2) if p else eng.seq_alloc(n + 2) for p, n in members]
    eng.prefill_extend_batch(seqs, [pool[31 * i:31 * i + n] for i, (_, n) in enumerate(members)])
    first.append([eng.seq_read(s, 0, 1) for s in seqs])
    for s in seqs:
        eng.seq_free(s)


fresh([100], lambda s, x: eng.prefill(s[0], x[0]))
fresh([64, 64, 64], eng.prefill_batch)
for va in (1, 2, 0):
    eng.debug_set("varlen_attn", va)
    fresh([7, 64, 61, 65, 130], eng.prefill_batch)
eng.debug_set("varlen_attn", 1)
base = eng.seq_alloc(320)
eng.prefill(base, pool[1000:1320])
for ve in (1, 0):
    eng.debug_set("varlen_extend", ve)
    behind(base, [(192, 64), (128, 129), (0, 201)])            # every member ends past rope_orig_max_pos
eng.debug_set("varlen_extend", 1)
behind(base, [(128, 37), (192, 64), (0, 63)])                  # ends 165, 256, 63: both sides of it
eng.seq_free(base)
torch.cuda.synchronize()
print("library:", lib.LIB_PATH)
print("first tokens per prefill:", first)
eng.close()
