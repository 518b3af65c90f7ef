"""Every form of the vision towers and the glue on tiny models, one sha256 per output: the evidence that two trees launch the same kernels and compute the same bits.
   python tools/vision_forms.py [tree]        tree = the root of the checkout whose library runs (default: this one)
   rocprofv3 --kernel-trace --stats -- python tools/vision_forms.py [tree]     once per tree; compare the per-kernel dispatch counts and the hashes
The towers are the ones of tests/test_gpu_vision_plan.py, n = 2, under the full product of gvl_debug_set patch_fused x vision_in_place x norm_fused x attn_pipe x attn_pipe_rows;
the glue runs for both LLM kinds.  Uses only entry points that exist on either side of the change it was written for (profiles/vision_plan_dispatches.md)."""
import hashlib
import itertools
import os
import sys

import torch

TREE = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TREE)
import _gvl_bootstrap  # noqa: E402,F401
from grounded_video_llm_amd import engine as E, synth, weights as Wt  # noqa: E402

DEV = "cuda:0"
KNOBS = ("patch_fused", "vision_in_place", "norm_fused", "attn_pipe", "attn_pipe_rows")
PRODUCT = list(itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 1, 2), (128, 256)))
TOWERS = [("clip", 64, 128, 4, 1, 28, 2), ("clip", 256, 512, 4, 1, 28, 2), ("clip", 1024, 256, 16, 1, 28, 1), ("iv2", 64, 128, 4, 2, 28, 3), ("iv2", 704, 256, 8, 2, 28, 2),
          ("iv2", 704, 256, 8, 8, 84, 1), ("iv2", 256, 512, 2, 2, 28, 2), ("iv2", 1408, 384, 16, 2, 28, 1)]
BASE = dict(clip_hidden=64, clip_inter=128, clip_layers=3, clip_heads=4, clip_image=28, clip_patch=14, iv2_dim=64, iv2_inter=128, iv2_depth=4, iv2_heads=4, iv2_image=28, iv2_patch=14,
            frames_per_seg=2, hidden=64, inter=128, layers=2, heads=4, kv_heads=4, vocab=100, max_seq=512, max_segs=2, kv_pages=16, max_prefill=256)


def sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


for tower, C, inter, heads, frames, image, layers in TOWERS:
    seed = f"vplan.{tower}.{C}.{heads}.{frames}.{image}"
    if tower == "clip":
        eng = E.Engine(E.TowerGeometry(**dict(BASE, clip_hidden=C, clip_inter=inter, clip_layers=layers + 1, clip_heads=heads, clip_image=image)), DEV, towers=("clip",))
        eng.load_packed(Wt.pack_clip(synth.clip_weights(C, inter, layers + 1, image, 14, seed=seed), layers))
        px = synth.det_tensor(seed + ".px", (2, 3, image, image)).to(DEV)
        run = lambda: eng.clip_encode(px)
    else:
        eng = E.Engine(E.TowerGeometry(**dict(BASE, iv2_dim=C, iv2_inter=inter, iv2_depth=layers + 1, iv2_heads=heads, iv2_image=image, frames_per_seg=frames)), DEV, towers=("iv2",))
        eng.load_packed(Wt.pack_iv2(synth.iv2_weights(C, inter, layers + 1, frames, image, 14, seed=seed), layers, frames))
        px = synth.det_tensor(seed + ".px", (2, 3, frames, image, image)).to(DEV)
        run = lambda: eng.iv2_encode(px)
    eng.finalize()
    for k in PRODUCT:
        for name, v in zip(KNOBS, k):
            eng.debug_set(name, v)
        print(f"{tower} {C}/{heads} f{frames} i{image} L{layers} knobs {' '.join(map(str, k))}: {sha(run())}", flush=True)
    eng.close()

for llm in ("phi3.5", "llama3"):
    eng = E.Engine(E.TowerGeometry(**dict(BASE, llm=llm, clip_image=336, iv2_image=224, hidden=256)), DEV, towers=("clip", "iv2", "proj"))
    eng.load_packed(Wt.pack_clip(synth.clip_weights(64, 128, 3, 336, 14, seed="vplan.glue.clip"), 2))
    eng.load_packed(Wt.pack_iv2(synth.iv2_weights(64, 128, 4, 2, 224, 14, seed="vplan.glue.iv2"), 3, 2))
    eng.load_packed(Wt.pack_projectors(synth.projector_weights(llm, 256, 64, 64, seed="vplan.glue.proj." + llm), llm))
    eng.finalize()
    cf = synth.det_tensor("vplan.glue.cf", (2, 576, 64)).to(DEV)
    vf = synth.det_tensor("vplan.glue.vf", (2, 512, 64)).to(torch.bfloat16).to(DEV)
    print(f"glue {llm}: {sha(eng.build_visual(cf, vf))}", flush=True)
    eng.close()
