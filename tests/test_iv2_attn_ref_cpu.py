"""CPU tests of tests/iv2_attn_ref.py over THE list test_gpu_iv2_attn.py runs: iv2_attn_ref.emulate -- the documented arithmetic of the InternVideo2 attention forms in
plain torch -- stands in for a correct kernel and must pass both comparisons on every case and every launch of it; with mut=... it stands in for wrong kernels, and every
mutation must be reported by iv2_attn_ref.judge, the comparison the GPU test uses, on at least one case of the list.  The conditions the list is built for are asserted
here, not assumed: both passes of the pipelined kernel are predicted (blocks redone for every row, for one row, and not at all; the survive regime keeps whole blocks in
the normal pass), every late_gap is realised on the rounded operands, the float64 reference is finite, the page images are what qkv_post_ref says, and no case is left out."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as A  # noqa: E402
import iv2_attn_ref as R  # noqa: E402
import qkv_post_ref as QP  # noqa: E402

SPECS = R.cases()


@functools.lru_cache(maxsize=None)
def case(n):
    return R.build(SPECS[n])


@functools.lru_cache(maxsize=None)
def bound(n, form2):
    return R.elementwise_bound(case(n), 2 if form2 else 0)


def run(n, f, pipe, pr, mut=None, info=None):
    c = case(n)
    out = R.emulate(c, f, pipe, pr, mut=mut, info=info)
    if c.family == "exact":
        return out, R.judge(c, f, out)
    ref, bd, _ = bound(n, f == 2)
    return out, R.judge(c, f, out, ref, bd)


def test_the_list_is_what_the_module_says():
    assert len(SPECS) == len({(s["family"], s["B"], s["S"], s["H"], s["Dr"], s["what"]) for s in SPECS}), "a case twice"
    ex = [s for s in SPECS if s["family"] == "exact"]
    bd = [s for s in SPECS if s["family"] == "bounded"]
    assert {s["what"] for s in ex} == set(R.EXACT_MAPS) and {s["what"] for s in bd} == set(R.KINDS)
    for fam in (ex, bd):
        f2 = [s for s in fam if 2 in s["forms"]]
        assert {-(-s["S"] // 64) for s in f2} >= {1, 2, 3, 4, 5, 6, 8}, "key tiles"
        assert {(s["B"], s["H"]) for s in f2} == set(R.BH)
        assert {s["ld_pad"] for s in f2} == {0, 16}
        assert {s["Dr"] for s in fam} == {72, 80, 88} and all(s["forms"] == ((2, 0, 1) if s["Dr"] == 88 else (0, 1)) for s in fam)
    assert {s["S"] for s in ex} == set(R.S_LIST) and {s["S"] for s in bd} >= {40, 65, 97, 129, 161, 193, 257, 321, 512}
    assert {s["S"] % 64 for s in ex} >= {0, 1, 32, 33, 63, 40}, "tails"
    for g in R.GAPS:                                                       # each g realised (bounded_case asserts the gap itself), on both block layouts somewhere
        assert len([s for s in bd if s["what"] == f"late_gap{g}"]) >= 3
    assert all(any(s["S"] == S and s["what"] == k for s in SPECS) for S in (257, 512) for k in ("near", "first_tile", "one_late", "mixed_block")), "pipe_rows 256 at 257 and 512"
    assert max(s["B"] * s["H"] * s["S"] for s in SPECS) <= 2 * 8 * 512, "a case has grown past what the paths need"


@pytest.mark.parametrize("n", range(len(SPECS)), ids=lambda n: "%02d" % n)
def test_the_emulation_passes_every_launch_and_the_identities_hold(n):
    c = case(n)
    outs, infos = {}, {}
    for f, pipe, pr in R.launches(c):
        infos[f, pipe, pr] = {}
        out, (msg, w) = run(n, f, pipe, pr, info=infos[f, pipe, pr])
        assert msg is None, msg
        assert w <= 1.0
        outs[f, pipe, pr] = out
    eq = lambda a, b: torch.equal(A._bits(outs[a]), A._bits(outs[b]))
    assert eq((0, 0, 0), (1, 0, 0)), "forms 0 and 1 share their arithmetic"
    if 2 in c.forms:
        assert eq((2, 0, 0), (2, 2, 0)), "pipe 0 against pipe 2"
        if c.S >= 256:
            assert eq((2, 1, 0), (2, 1, 256)) and eq((2, 2, 0), (2, 2, 256)), "pipe_rows 256 against 0"
        if R.pipe1_equals_pipe0(c):
            assert not infos[2, 0, 0]["moved"], "the reference says no tile exceeds the first by 2^8, the emulation moved its reference"
            assert eq((2, 1, 0), (2, 0, 0)), "pipe 1 against pipe 0"
    if c.family == "bounded":
        for form2 in ((True, False) if 2 in c.forms else (False,)):
            ref, bd, Ab = bound(n, form2)
            assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bd).all()) and bool((bd > 0).all())
        # the entry's promise (gvl.h): finite output for |v| <= 2^27 / S; these cases stay inside it
        assert float(c.v.float().abs().max()) <= 2.0 ** 27 / c.S
        if c.what.startswith("late_gap"):
            assert float(c.v.float().abs().max()) >= 2.0 ** 10


def test_both_passes_are_predicted():
    """per 128-row query block of every case the emulation says which pass the pipelined kernel takes"""
    seen = dict(all_rows=0, one_row=0, kept=0, kept_block_of_survivors=0, idle_wave_block_redone=0, idle_wave_block_kept=0)
    for n, s in enumerate(SPECS):
        if 2 not in s["forms"]:
            continue
        c = case(n)
        for pr in (0, 256) if c.S >= 256 else (0,):
            info = {}
            R.emulate(c, 2, 1, pr, info=info)
            redo = info["redo"]
            seen["all_rows"] += sum(1 for r in redo if r[3] == r[4] and r[4] >= 128)
            seen["one_row"] += sum(1 for r in redo if r[3] == 1 and r[4] >= 128)
            seen["kept"] += info["blocks"] - len(redo)
            seen["idle_wave_block_redone"] += sum(1 for r in redo if r[4] == 1)
            if s["what"] in ("late_heavy",) and c.S >= 193:
                assert len(redo) == info["blocks"], f"{c}: a later tile is 2^130 ahead of the first, every block repeats"
            if s["what"] == "near":
                assert not redo, f"{c}: the survive regime must keep the normal pass, {len(redo)} blocks redone"
                seen["kept_block_of_survivors"] += info["blocks"]
                v, l, O = c.v.permute(0, 2, 1, 3).float(), info["l"], info["O"]
                vt = torch.gather(v, 2, c.target[..., None].expand(-1, -1, -1, c.Dr))
                assert bool((l > 2.0 ** 90).all()) and bool((l < 2.0 ** 100).all()) and torch.equal(l, l.to(R.bf).float()), f"{c}: l is not the target's rounded probability"
                assert torch.equal(O, l[..., None] * vt), f"{c}: something besides the target survived the fp32 accumulation"
                a = c.v.float().abs()
                assert float(a.min()) >= 2.0 ** -20 and float(a.max()) < 2.0 ** 21
            if s["what"] == "first_tile":
                assert not redo
            if s["what"] in ("one_late", "mixed_block"):
                assert redo and all(r[3] in (1, 2) for r in redo), f"{c}: {redo[:4]}"       # (2: head 0 of batch 0 also sends row S - 1)
            if s["what"] in ("first_tile", "near", "plain") and c.S % 128 == 1:
                seen["idle_wave_block_kept"] += 1
            if s["what"].startswith("late_gap"):
                g = c.gap
                assert (len(redo) == info["blocks"]) if g > 100 else not redo, f"{c}: {len(redo)} of {info['blocks']} blocks redone"
    assert all(v > 0 for v in seen.values()), seen


def test_pages_are_qkv_post_refs_layout():
    """pages() goes through qkv_post_ref.emulate: spot checks that the images hold this file's operands where qkv_post_ref's contract puts them"""
    c = case(next(n for n, s in enumerate(SPECS) if s["what"] == "ragged_rs" and s["S"] == 129))
    B, S, H, Dr = c.B, c.S, c.H, c.Dr
    pg = R.pages(c)
    nt = (S + 63) // 64
    bits = lambda t: t.contiguous().view(torch.int16).numpy().view(np.uint16)
    Kt, Vt, Q = pg["Kt"], pg["Vt"], pg["Q"].reshape(B, H, S, R.D)
    assert Kt.shape == (B * nt, H, 64, R.D) and Vt.shape == (B * nt, H, R.D, 64)
    b, h, j = B - 1, H - 1, S - 1
    assert np.array_equal(Kt[b * nt + j // 64, h, j % 64, :Dr], bits(c.k[b, j, h])) and Kt[b * nt + j // 64, h, j % 64, Dr] == QP.ONE and not Kt[b * nt + j // 64, h, j % 64, Dr + 1:].any()
    assert (Kt[b * nt + j // 64, h, j % 64 + 1:] == QP.SENT).all(), "K slots behind the last key are nobody's"
    assert np.array_equal(Vt[b * nt + 1, h, :Dr, 5], bits(c.v[b, 69, h])) and (Vt[:, :, Dr] == QP.ONE).all() and not Vt[:, :, Dr + 1:].any() and not Vt[b * nt + j // 64, h, :Dr, j % 64 + 1:].any()
    assert np.array_equal(Q[b, h, 7, :Dr], bits(R.qn_of(c)[b, h, 7].to(R.bf))) and not Q[..., Dr:].any()


# which cases can show a mutation at all (a filter on the list for speed: the comparison is never told)
WHERE = {
    "no_repass": lambda s: s["S"] > 64, "mask_plus": lambda s: s["S"] % 64, "mask_minus": lambda s: True, "skip_kb2_at_33": lambda s: s["S"] % 64 == 33, "pad_dup": lambda s: s["S"] % 64,
    "vlast_no_ones": lambda s: s["S"] % 64, "k_pad_zero": lambda s: s["S"] > 64, "q_rs_prev": lambda s: s["what"] == "ragged_rs", "q_rs_batch0": lambda s: s["what"] == "ragged_rs" and s["B"] > 1,
    "q_nw_no_head": lambda s: s["what"] == "ragged_rs", "scale_twice": lambda s: s["family"] == "bounded", "xcd_swap": lambda s: s["B"] > 1, "rows8_neither": lambda s: s["S"] in (257, 321),
    "rows8_both": lambda s: s["S"] in (257, 321), "alpha_split": lambda s: s["S"] > 64,
}


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutation_is_reported_by_the_gpu_tests_comparison(mut):
    """... by BOTH families where both can see it; the mutations that only one family can see say why"""
    one_family = {
        "scale_twice": "exact: a one-hot row stays one-hot under any scale", "q_rs_prev": "exact: q_rs = 1 everywhere", "q_rs_batch0": "exact: q_rs = 1 everywhere",
        "q_nw_no_head": "exact: q_nw = 1 everywhere", "pad_dup": "exact: a duplicated key with a duplicated V row is (1 + n) v / (1 + n)",
        "mask_plus": "exact: as pad_dup", "alpha_split": "exact: alpha = 0 on every move, and 0 x l = 0 either way",
    }
    assert set(WHERE) == set(R.MUTATIONS)
    hit = {}
    for n, s in enumerate(SPECS):
        if 2 not in s["forms"] or not WHERE[mut](s) or s["family"] in hit:
            continue
        for f, pipe, pr in R.launches(case(n)):
            if f != 2:
                continue
            _, (msg, _) = run(n, f, pipe, pr, mut=mut)
            if msg is not None:
                hit[s["family"]] = (str(case(n)), (f, pipe, pr), msg[:300])
                break
        if len(hit) == 2:
            break
    print(f"[mutation] {mut}: {hit}")
    want = {"bounded"} if mut in one_family else {"exact", "bounded"}
    assert want <= set(hit), f"{mut}: seen by {sorted(hit)} only"
