"""-m gpu: the launches a tower's call books are the plan's (csrc/gvl_vision_plan.h through tests/vision_plan.py), under every knob setting that changes the plan, on the
smallest shapes that reach each branch; and the forms the knobs switch between are bit-identical where the towers' tests say so (tests/test_gpu_towers.py): every
vision_in_place for CLIP, 0 = 2 for InternVideo2 (and = 1 unless q is normalised on load), attn_pipe 0 = 1 = 2, attn_pipe_rows 128 = 256, patch_fused where the fused kernel
does not serve the width.  The result tests cannot see which form ran; gvl_prof_read can."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, tiny_geo  # noqa: E402
from grounded_video_llm_amd import engine as E, weights as Wt, synth  # noqa: E402
import vision_plan as V  # noqa: E402

PRODUCT = [dict(zip(V.KNOBS, k)) for k in itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 1, 2), (128, 256))]

# tower, width, inter, heads, frames, image, layers run: the branch it reaches
TOWERS = [
    ("clip", 64, 128, 4, 1, 28, 2),        # head dim 16 in 64: pages + V rows, three-pass patch embedding
    ("clip", 256, 512, 4, 1, 28, 2),       # 4 heads of 64: q, k, v in place, no qkv_post
    ("clip", 1024, 256, 16, 1, 28, 1),     # the fused patch embedding
    ("iv2", 64, 128, 4, 2, 28, 3),         # fused RMSNorm with a first, a middle and a last block; no pipelined form
    ("iv2", 704, 256, 8, 2, 28, 2),        # 8 heads of 88: q normalised on load, ones row, the pipelined kernel
    ("iv2", 704, 256, 8, 8, 84, 1),        # S = 289: attn_pipe_rows 256 cuts the attention into two kernel launches of one booked launch
    ("iv2", 256, 512, 2, 2, 28, 2),        # 2 heads of 128: V^T pages forced
    ("iv2", 1408, 384, 16, 2, 28, 1),      # the fused patch embedding, 11-wide kernel
]


def engine_of(tower, C, inter, heads, frames, image, layers):
    seed = f"vplan.{tower}.{C}.{heads}.{frames}.{image}"
    if tower == "clip":
        geo = tiny_geo(clip_hidden=C, clip_inter=inter, clip_layers=layers + 1, clip_heads=heads, clip_image=image, max_segs=2)
        eng = E.Engine(geo, DEV, towers=("clip",))
        eng.load_packed(Wt.pack_clip(synth.clip_weights(C, inter, layers + 1, image, 14, seed=seed), layers))
        px = synth.det_tensor(seed + ".px", (2, 3, image, image))
        run = lambda: eng.clip_encode(px.to(DEV))
    else:
        geo = tiny_geo(iv2_dim=C, iv2_inter=inter, iv2_depth=layers + 1, iv2_heads=heads, iv2_image=image, frames_per_seg=frames, max_segs=2)
        eng = E.Engine(geo, DEV, towers=("iv2",))
        eng.load_packed(Wt.pack_iv2(synth.iv2_weights(C, inter, layers + 1, frames, image, 14, seed=seed), layers, frames))
        px = synth.det_tensor(seed + ".px", (2, 3, frames, image, image))
        run = lambda: eng.iv2_encode(px.to(DEV))
    eng.finalize()
    return eng, run


@pytest.mark.parametrize("tower,C,inter,heads,frames,image,layers", TOWERS)
def test_a_tower_books_the_plans_launches_under_every_knob(tower, C, inter, heads, frames, image, layers):
    kind = V.CLIP if tower == "clip" else V.IV2
    tiled = C == 1024 if tower == "clip" else C in (1024, 1408)          # gvl_finalize_weights makes the tile-order patch weight for these widths, and the folded weights always
    plans = {}
    for k in PRODUCT:                                                     # one encode per distinct plan
        plans.setdefault(V.tower(kind, 2, C, inter, heads, image, frames, layers, tiled, True, **k), k)
    eng, run = engine_of(tower, C, inter, heads, frames, image, layers)
    outs = {}
    for p, k in plans.items():
        for name, v in k.items():
            eng.debug_set(name, v)
        out, n_gemm, n_attn, n_other = V.profiled(eng, run)
        assert (n_gemm, n_attn, n_other) == (p.n_gemm, p.n_attn, p.n_other) == V.counts(p.lines), (k, p[:11])
        assert bool(torch.isfinite(out.float()).all())
        outs.setdefault((p.patch_fused, p.nf, p.q_on_load), []).append((k, out))
    eng.close()
    assert len(plans) > 1 and len(outs) == len({(p.patch_fused, p.nf, p.q_on_load) for p in plans})
    for same in outs.values():                                            # operand paths, attention kernels and their row split: bit for bit
        for k, out in same[1:]:
            assert torch.equal(out, same[0][1]), (same[0][0], k)
    reached = {(p.patch_fused, p.vt_pages, p.qk_rows, p.q_on_load, p.nf) for p in plans}
    assert any(r[0] for r in reached) == tiled and any(r[2] for r in reached) == (tower == "clip" and C // heads == 64)
    assert any(r[3] for r in reached) == (tower == "iv2" and C // heads == 88) and any(r[4] for r in reached) == (tower == "iv2") and any(not r[1] for r in reached) == (C // heads != 128)


@pytest.mark.parametrize("llm", ["phi3.5", "llama3"])
def test_the_glue_books_the_plans_launches(llm):
    hid = 256
    geo = tiny_geo(llm=llm, clip_image=336, iv2_image=224, hidden=hid, max_segs=2)
    eng = E.Engine(geo, DEV, towers=("clip", "iv2", "proj"))
    eng.load_packed(Wt.pack_clip(synth.clip_weights(64, 128, 3, 336, 14, seed="vplan.glue.clip"), 2))
    eng.load_packed(Wt.pack_iv2(synth.iv2_weights(64, 128, 4, 2, 224, 14, seed="vplan.glue.iv2"), 3, 2))
    eng.load_packed(Wt.pack_projectors(synth.projector_weights(llm, hid, 64, 64, seed="vplan.glue.proj." + llm), llm))
    eng.finalize()
    cf = synth.det_tensor("vplan.glue.cf", (2, 576, 64)).to(DEV)
    vf = synth.det_tensor("vplan.glue.vf", (2, 512, 64)).to(torch.bfloat16).to(DEV)
    p = V.glue(llm == "phi3.5", 2, hid, 64, 64, 2)
    vis, n_gemm, n_attn, n_other = V.profiled(eng, lambda: eng.build_visual(cf, vf))
    assert (n_gemm, n_attn, n_other) == (p.n_gemm, p.n_attn, p.n_other) == V.counts(p.lines) == ((6, 0, 3) if llm == "phi3.5" else (4, 0, 3))
    assert list(vis.shape) == [2 * eng.tokens_per_seg, hid] and bool(torch.isfinite(vis.float()).all())
    assert torch.equal(eng.build_visual(cf, vf), vis)
    eng.close()
