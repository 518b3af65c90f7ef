"""Time of one token-selection launch on a 16 x 32064 group of fp32 rows (the Phi-3.5 vocabulary, the decode group size): sample_kernel at T / top-k / top-p
(gvl_op_sample) against the per-row kernel select_rows_kernel (gvl_op_select_rows; csrc/gvl_pick.hip) with the same T / k / p per row and with every warper on
(min_p, typical_p, epsilon_cutoff, eta_cutoff as well), and a half-greedy group.  The variants rotate within one process (same box, same rows), each timed with
device events around `--iters` back-to-back launches, `--reps` times; the output is one JSON line with the per-launch microseconds of every repetition.
A record only: token selection is one launch per decode step (bench.py decodes greedily and never reaches these kernels).
  python tools/select_rows_bench.py [--n 32064] [--batch 16] [--iters 200] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _gvl_bootstrap  # noqa: E402,F401
import torch  # noqa: E402
from grounded_video_llm_amd import engine as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=32064)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = "cuda:0"
eng = E.Engine(E.TowerGeometry(max_segs=1), dev, towers=())                            # the operators need a ctx, not a model
B, n = args.batch, args.n
g = torch.Generator().manual_seed(1)
x = (torch.randn((B, n), generator=g) * torch.tensor([0.5, 2.0, 4.0, 30.0])[torch.arange(B) % 4][:, None]).to(dev).contiguous()
T, K, P, SEED = 0.7, 50, 0.9, 1234
streams, steps = list(range(B)), [7] * B
tkp = [dict(do_sample=True, temperature=T, top_k=K, top_p=P, seed=SEED, stream=b) for b in range(B)]
allw = [dict(r, min_p=0.02, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3) for r in tkp]
half = [r if b % 2 else None for b, r in enumerate(allw)]
VARIANTS = {
    "sample_kernel T/k/p": lambda: eng.op_sample(x, T, K, P, SEED, streams, steps),
    "select_rows T/k/p": lambda: eng.op_select_rows(x, tkp, -1, steps),
    "select_rows all warpers": lambda: eng.op_select_rows(x, allw, -1, steps),
    "select_rows all warpers, half greedy": lambda: eng.op_select_rows(x, half, -1, steps),
}
assert torch.equal(VARIANTS["sample_kernel T/k/p"](), VARIANTS["select_rows T/k/p"]()[0]), "the per-row kernel at T / k / p must draw sample_kernel's tokens"
names = list(VARIANTS)
for f in VARIANTS.values():                                    # warm-up: code objects, allocator
    for _ in range(10):
        f()
torch.cuda.synchronize()
res = {m: [] for m in names}
for r in range(args.reps):
    for m in names[r % len(names):] + names[:r % len(names)]:   # rotate the order
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            VARIANTS[m]()
        e1.record(); torch.cuda.synchronize()
        res[m].append(round(e0.elapsed_time(e1) * 1000.0 / args.iters, 2))
out = {"what": f"us per call (launch + host wrapper), {B} x {n} fp32 rows, {args.iters} back-to-back calls per figure, T={T} top_k={K} top_p={P}", "device": torch.cuda.get_device_name(0),
       "us_per_call": res, "median_us": {m: sorted(v)[len(v) // 2] for m, v in res.items()}}
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(line + "\n")
eng.close()
