"""CPU tests of tests/vision_ref.py: the references of test_gpu_vision_ops.py agree with the oracle's definitions, a correct implementation stays inside every bound on
every input the GPU tests use, and the kernel bugs those tests exist for are caught.  A plain fp32 / bf16 torch emulation of the documented arithmetic stands in for a
correct kernel; its deliberate mutations (vision_ref.MUTATIONS) stand in for the bugs."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vision_ref as V  # noqa: E402
import gvl_oracle as O  # noqa: E402

bf = torch.bfloat16
CASES = V.patch_cases()
IDS = [c.name() for c in CASES]


def case_of(mode, image, T, n, C, kind):
    return next(c for c in CASES if (c.mode, c.image, c.T, c.n, c.C, c.kind) == (mode, image, T, n, C, kind))


def glue_f(n, C, seed=5):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randn((n, 576, C), generator=g) * 3.0


# ---- (a) the references are the oracle's definitions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_patch_reference_is_the_oracles_embedding(c):
    """float64 reference vs the oracle's CLIP / InternVideo2 embedding functions (fp32, bf16-emulating): the difference is inside the reference's own bound plus the
    oracle's fp32 noise -- and exact on the integer cases of InternVideo2"""
    ref, bound = V.patch_reference(c)
    p = c.patch
    w = c.W[:, :3 * p * p].float()
    if c.mode == 0:
        Wd = {"vision_model.embeddings.patch_embedding.weight": w.view(c.C, 3, p, p), "vision_model.embeddings.class_embedding": c.cls,
              "vision_model.embeddings.position_embedding.weight": c.pos, "vision_model.pre_layrnorm.weight": c.lnw, "vision_model.pre_layrnorm.bias": c.lnb}
        got = O.clip_embeddings(c.px[:, :, 0], Wd, emu=True)
    else:
        Wd = {"patch_embed.proj.weight": w.view(c.C, 3, 1, p, p), "patch_embed.proj.bias": c.bias, "cls_token": c.cls.float().view(1, 1, -1),
              "pos_embed": c.pos.float()[None]}
        got = O.iv2_embed(c.px, Wd, emu=True)
    if c.kind == "exact" and c.mode == 1:
        assert torch.equal(got.double(), ref)
    else:
        msg, _ = V.bound_violations(got.reshape(-1, c.C), ref.reshape(-1, c.C), bound.reshape(-1, c.C), c.name())
        assert msg is None, msg


def test_layernorm_reference_is_torch_layer_norm():
    for rows in V.NORM_ROWS:
        for cols in V.LN_COLS:
            x, w, b = V.norm_rows(rows, cols, 1, torch.float32)
            v = V.layernorm_bound(x.double(), torch.zeros_like(x, dtype=torch.float64), w.double(), b.double(), 1e-5, out_bf16=False)
            assert torch.allclose(v.x, F.layer_norm(x.double(), (cols,), w.double(), b.double(), 1e-5), rtol=1e-12, atol=1e-12)
            assert torch.equal(v.x[2], b.double()) if rows == 5 else True            # the all-zero row is the bias exactly


def test_glue_references_are_the_oracles():
    f = glue_f(2, 8)
    sub = torch.arange(32, dtype=torch.float32) - 7.5
    assert torch.equal(V.hd_merge_ref(f, sub), O.add_image_newline_phi3(O.hd_merge_2x2_phi3(f), sub).to(bf))
    assert torch.equal(V.emulate_hd_merge(f, sub), V.hd_merge_ref(f, sub))
    assert float((V.pool_spatial_ref(f).x - V._rbf(O.pool_spatial_llama(f.double()))).abs().max()) == 0.0
    fb = (torch.randn((2, 3, 256, 8), generator=torch.Generator().manual_seed(9)) * 2).to(bf)
    assert float((V.pool_temporal_ref(fb).x.reshape(2, 48, 8) - V._rbf(O.pool_temporal(fb.double().reshape(2, 768, 8), 3))).abs().max()) == 0.0
    # im2col: the columns of the reference times the weight rows are the convolution
    c = case_of(1, 28, 3, 5, 1024, "exact")
    A = V.patchify_ref(c.px, c.patch, c.Kp)
    assert A.shape == (c.M, c.Kp) and not bool(A[:, V.KREAL:].any())
    conv = V._conv(c.px.double(), c.W.double(), c.patch, c.n, c.T, c.L).reshape(c.M, c.C)
    assert torch.equal(A[:, :V.KREAL].double() @ c.W[:, :V.KREAL].double().T, conv)


# ---- (b) the emulation is inside every bound, on every input the GPU tests use ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_emulated_patch_embedding_meets_the_check(c):
    buf, out = V.emulate_patch(c)
    msg, worst, ndiff = V.check_patch(c, out, c.name())
    assert msg is None, msg
    assert V.guard_damage(buf, c.n * c.S) == 0
    if c.kind == "exact" and c.mode == 0:
        assert worst < 1.0


def test_exact_cases_hit_what_they_claim():
    """every pixel column, pixel row and channel of a patch carries a nonzero pixel somewhere in the largest cases; the shapes have the tails the kernel's paths need"""
    for c in (case_of(0, 98, 1, 2, 1024, "exact"), case_of(0, 42, 1, 11, 1024, "exact"), case_of(1, 56, 2, 3, 1408, "exact")):
        hit = c.px.abs().view(c.n, 3, c.T, c.g, 14, c.g, 14).sum((0, 2, 3, 5))
        assert bool((hit > 0).all()), "a (channel, pixel row, pixel column) of the patch is never exercised"
    Ms = {(c.mode, c.image, c.n): c.M for c in CASES}
    assert Ms[(0, 14, 1)] == 1 and Ms[(0, 42, 11)] == 99 and Ms[(0, 98, 2)] == 98 and Ms[(1, 28, 5)] == 60 and Ms[(1, 56, 3)] == 96


@pytest.mark.parametrize("rows", V.NORM_ROWS)
def test_emulated_norms_meet_their_bounds(rows):
    for cols in V.LN_COLS:
        x, w, b = V.norm_rows(rows, cols, 1, torch.float32)
        v = V.layernorm_bound(x.double(), torch.zeros((rows, cols), dtype=torch.float64), w.double(), b.double(), 1e-5, out_bf16=True, depth=V.wave_sum_depth(cols))
        msg, _ = V.bound_violations(V.emulate_layernorm(x, w, b, 1e-5, True), v.x, v.e, f"layernorm {rows}x{cols}")
        assert msg is None, msg
    for cols in V.RMS_COLS:
        x, w, _ = V.norm_rows(rows, cols, 2, bf)
        v = V.rmsnorm_bound(x.double(), torch.zeros((rows, cols), dtype=torch.float64), w.double(), 1e-6, depth=V.wave_sum_depth(cols))
        got = V.emulate_rmsnorm(x, w, 1e-6)
        msg, _ = V.bound_violations(got, v.x, v.e, f"rmsnorm {rows}x{cols}")
        assert msg is None, msg
        if rows == 5:
            assert not bool(got[2].any())                                          # the all-zero row gives 0


def test_emulated_pools_meet_their_bounds():
    for C in (4, 1024):
        f = glue_f(2, C)
        v = V.pool_spatial_ref(f)
        msg, _ = V.bound_violations(V.emulate_pool_spatial(f).reshape(-1, C), v.x.reshape(-1, C), v.e.reshape(-1, C), f"pool_spatial C{C}")
        assert msg is None, msg
        fi, want = V.pool_spatial_exact_input(2, C, 3)
        assert torch.equal(V.emulate_pool_spatial(fi), want) and torch.equal(V.pool_spatial_ref(fi).x, want.double())
    for C, T in ((8, 1), (8, 3), (1408, 1), (1408, 3)):
        fb = (torch.randn((2, T, 256, C), generator=torch.Generator().manual_seed(C + T)) * 2).to(bf)
        v = V.pool_temporal_ref(fb)
        msg, _ = V.bound_violations(V.emulate_pool_temporal(fb).reshape(-1, C), v.x.reshape(-1, C), v.e.reshape(-1, C), f"pool_temporal C{C} T{T}")
        assert msg is None, msg
        fi = V.int_field((2, T, 256, C), -8, 8, 11).to(bf)
        assert torch.equal(V.emulate_pool_temporal(fi), V.pool_temporal_ref(fi).x.to(bf))
        assert torch.equal(V.pool_temporal_ref(fi).x.to(bf).double(), fi.double().view(2, T, 4, 4, 4, 4, C).mean((3, 5)).reshape(2, T, 16, C))


# ---- (c) every mutation is caught ----------------------------------------------------------------------------------------------------------------------------------------
def patch_caught(c, mutate):
    buf, out = V.emulate_patch(c, mutate)
    msg, _, _ = V.check_patch(c, out, c.name())
    return msg is not None or V.guard_damage(buf, c.n * c.S) > 0


@pytest.mark.parametrize("mutate", ["drop_px13", "pos_off1", "cls_pos1", "dup_tail"])
@pytest.mark.parametrize("kind", ["exact", "bounded"])
def test_patch_mutations_are_caught_in_both_towers(mutate, kind):
    assert patch_caught(case_of(0, 42, 1, 11, 1024, kind), mutate), f"CLIP: {mutate} passes"
    for C in V.IV2_DIMS:
        assert patch_caught(case_of(1, 28, 3, 5, C, kind), mutate), f"InternVideo2 C{C}: {mutate} passes"


@pytest.mark.parametrize("kind", ["exact", "bounded"])
def test_frame_taken_from_the_previous_one_is_caught(kind):
    for C in V.IV2_DIMS:
        assert patch_caught(case_of(1, 28, 3, 5, C, kind), "frame_prev")


def test_glue_mutations_are_caught():
    f = glue_f(3, 8)
    sub = torch.arange(32, dtype=torch.float32) - 7.5
    for m in ("sub_gn_col0", "dydx_swap"):
        assert not torch.equal(V.emulate_hd_merge(f, sub, m), V.hd_merge_ref(f, sub)), m
    v = V.pool_spatial_ref(f)
    msg, _ = V.bound_violations(V.emulate_pool_spatial(f, "window_shift").reshape(-1, 8), v.x.reshape(-1, 8), v.e.reshape(-1, 8), "shifted window")
    assert msg is not None
    fi, want = V.pool_spatial_exact_input(2, 4, 3)
    assert not torch.equal(V.emulate_pool_spatial(fi, "window_shift"), want)


@pytest.mark.parametrize("cols", V.LN_COLS)
def test_one_pass_variance_is_caught(cols):
    x, w, b = V.norm_rows(1, cols, 1, torch.float32)                               # the row of 1000 + noise
    v = V.layernorm_bound(x.double(), torch.zeros((1, cols), dtype=torch.float64), w.double(), b.double(), 1e-5, out_bf16=True, depth=V.wave_sum_depth(cols))
    msg, _ = V.bound_violations(V.emulate_layernorm(x, w, b, 1e-5, True, one_pass=True), v.x, v.e, f"one-pass layernorm {cols}")
    assert msg is not None, "a one-pass variance stays inside the bound"


@pytest.mark.parametrize("grp", V.GROUPINGS)
def test_groups_written_with_the_wrong_stride_are_caught(grp):
    gr, gs, off = grp
    M = 4 * gr + (gr + 1) // 2
    dense = V.int_field((M, 8), -50, 50, 4).to(bf)
    good = V.scatter_groups(dense, gr, gs, off)
    assert V.check_grouped(good, dense, gr, gs, off) == (0, 0)
    assert int((good == V.SENT).all(1).sum()) == good.shape[0] - M                 # every row between the groups keeps the sentinel
    bad = V.scatter_groups(dense, gr, gs, off, "stride_is_rows")
    wrong, lost = V.check_grouped(bad, dense, gr, gs, off)
    assert wrong > 0 or lost > 0
