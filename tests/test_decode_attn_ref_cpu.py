"""CPU tests of tests/decode_attn_ref.py: the references of test_gpu_decode_attn_exact.py can fail, and a correct implementation stays inside them.
decode_attn_ref.emulate -- the two decode-attention kernels' documented arithmetic in plain torch, reading the pages through the tables -- stands in for a correct kernel over
THE lists the GPU test runs (exact_cases / bounded_cases); its twelve mutations stand in for defects these kernels could plausibly have, and each must be rejected by a
case OF THOSE LISTS, which the test names."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_attn_ref as R  # noqa: E402
from attn_ref import SENT, _bits  # noqa: E402

bf = torch.bfloat16
EXACT, BOUNDED = R.exact_cases(), R.bounded_cases()


def build(e):
    return R.onehot_case(e["lens"], e["H"], e["KV"], e["Dr"], e["seed"], share=e["share"])


def shape_of(c, e):
    return (e["cpb"], R.min_gsplit(c, e["cpb"]) if e["gsplit_min"] else 0, e["hpb"])


def judge_exact(c, out):
    assert bool((out[:, c.H * c.Dr:] == SENT).all()), f"{c}: the emulation wrote to the guard columns"
    return R.onehot_mismatch(out[:, :c.H * c.Dr].contiguous(), c)


def test_the_lists_are_what_the_issue_asks_for():
    assert len(R.GEOS) == 21 and len(EXACT) == 21 * 16 and len(BOUNDED) == len(R.BOUNDED_GEOS) * len(R.KINDS)
    for i in range(len(R.GEOS)):
        mine = [e for e in EXACT if e["geo"] == i]
        assert sorted(e["lens"][0] for e in mine if len(e["lens"]) == 1) == R.LENS and any(len(e["lens"]) == 3 for e in mine) and any(len(e["lens"]) == 16 and e["share"] for e in mine)
    for key, vals in (("cpb", set(R.CPBS)), ("gsplit_min", {0, 1}), ("out_tiled", {0, 1}), ("pad", {False, True})):
        assert {e[key] for e in EXACT} == vals and {e[key] for e in BOUNDED} == vals, key
    assert {R.split_rule(L)[1:] for L in (256, 257, 833, 1025, 4096, 4097, 8256)} == {(1, 4), (2, 3), (4, 4), (5, 4), (16, 4), (16, 5), (16, 9)}
    assert R.place(4097, 4 * 64 + 3) == (4, 0, 0, 1) and R.place(8256, 128 * 64) == (128, 14, 2, 0) and R.split_rule(8256)[0] - 14 * 9 == 3        # second trip; 15th split short, 16th empty
    assert {g[4] for g in R.GEOS} == R.REACHABLE and len(R.REACHABLE) == 12


def test_onehot_operands_and_layout_are_what_the_docstring_says():
    c = R.onehot_case([257, 130, 64], 4, 2, 80, seed=5)
    assert c.D == 96 and c.table_stride == 8 and c.n_pages == 5 + 3 + 1 + 3 + 2
    for t in R.target_sets(c)[:3]:
        c.set_targets(t)
        for b, L in enumerate(c.lens):
            s = torch.einsum("hd,jhd->hj", c.q[b, :, :80].float(), c.k[b].float().repeat_interleave(2, dim=1))
            top = s.topk(2, dim=-1)
            assert float(s.abs().max()) <= 64 * c.nb and torch.equal(top.indices[:, 0], c.target[b])
            assert L == 1 or bool((top.values[:, 0] - top.values[:, 1] >= 128).all())
            n, rem = (L + 63) // 64, L - (L - 1) // 64 * 64
            tab = c.tables[b].tolist()
            assert tab[:n] != list(range(n)) and len(set(tab[:n])) == n and set(tab[n:]) == {c.poison[b]} and c.poison[b] not in tab[:n]
            # the documented layout, read back element by element
            for j in (0, L // 2, L - 1):
                for g in range(2):
                    assert torch.equal(c.Kt[tab[j // 64], g, j % 64, :80], c.k[b][j, g]) and torch.equal(c.Vt[tab[j // 64], g, :80, j % 64], c.v[b][j, g])
            assert bool((c.Kt[tab[:n], :, :, 80:] == 0).all()) and bool((c.q[..., 80:] == 0).all()) and bool((c.Vt[tab[:n], :, 80:].float().abs() >= 9e29).all())
            win = c.q[b, :, :80].float() / 64                                    # [H, Dr]: the winning codes
            for page, lo in ((tab[n - 1], rem), (c.poison[b], 0)):
                for g in range(2):
                    for slot in range(lo, 64):
                        assert torch.equal(c.Kt[page, g, slot, :80].float(), win[g * 2 + slot % 2]), "decoy K rows equal a head's winning code"
                    assert torch.isfinite(c.Vt[page, g, :80, lo:].float()).all() and c.Vt[page, g, 0, lo:].view(torch.int16).unique().numel() == 64 - lo
    used = set(c.tables.flatten().tolist())
    assert all(bool(torch.isnan(c.Kt[p].float()).all()) for p in range(c.n_pages) if p not in used) and len(used) < c.n_pages
    sets = R.target_sets(R.onehot_case([4097], 2, 2, 64, seed=1))
    hit = {int(x) for t in sets for x in t.flatten()}
    assert {x // 64 for x in hit} == set(range(65)) and {0, 4096, 4095}.issubset(hit) and all({s * 5 * 64, min(4097, (s + 1) * 5 * 64) - 1}.issubset(hit) for s in range(13))


def test_shared_prefix_pages_are_the_same_pages():
    c = R.onehot_case(R.LENS16, 2, 2, 64, seed=3, share=R.SHARE16)
    a, b, n = R.SHARE16
    assert torch.equal(c.tables[a, :n], c.tables[b, :n]) and int(c.tables[a, n]) != int(c.tables[b, n])
    assert not torch.equal(_bits(c.v[a][n * 64:R.LENS16[a]]), _bits(c.v[b][n * 64:R.LENS16[a]]))


@pytest.mark.parametrize("geo", range(len(R.GEOS)))
def test_emulation_reproduces_every_exact_case_bit_for_bit(geo):
    """every case of the GPU list; of each case's target sets the first, the middle and the last one (the GPU test goes through all of them)"""
    for e in (e for e in EXACT if e["geo"] == geo):
        c = build(e)
        sets = R.target_sets(c)
        for t in {0: sets[0], len(sets) // 2: sets[len(sets) // 2], len(sets) - 1: sets[-1]}.values():
            c.set_targets(t)
            out, part = R.emulate(c, shape_of(c, e))
            msg = judge_exact(c, out)
            assert msg is None, msg


@pytest.mark.parametrize("n", range(len(BOUNDED)))
def test_emulation_stays_inside_the_elementwise_bound(n):
    e = BOUNDED[n]
    c = R.bounded_case(e["kind"], e["lens"], e["H"], e["KV"], e["Dr"], e["seed"])
    out, _ = R.emulate(c, shape_of(c, e))
    ref, bound, Abs = R.elementwise_bound(c)
    msg, worst = R.bound_violations(out[:, :c.H * c.Dr], ref, bound, c)
    lead = float(((out[:, :c.H * c.Dr].double() - ref).abs() / (2 * 2.0 ** -8 * Abs)).max())
    print(f"[decode-attn-ref] emulation {c}: worst err / bound {worst:.3f} (err / (2 2^-8 Abs) {lead:.3f})")
    assert msg is None, msg
    assert float(bound.min()) > 0 and bool(torch.isfinite(bound).all())


# mutation -> (geometry index in GEOS, lens): the case OF THE GPU LIST that rejects it in the exact family
CAUGHT_BY_EXACT = {
    "mask_plus": (0, [65]), "mask_minus": (0, [64]), "drop_second_trip": (6, [4097]), "pps_floor": (1, [257]), "drop_last_split": (9, [257]), "merge_all_nsplit": (14, [833]),
    "no_rescale_wave": (2, [255]), "no_rescale_merge": (11, [1025]), "gqa_mod": (7, [63]), "table_identity": (18, [2]), "table_of_seq0": (0, R.LENS3), "dout_stride": (3, [1]),
}
# mutation -> (geometry index, kind): the bounded case of the GPU list that rejects it as well
CAUGHT_BY_BOUNDED = {"mask_plus": (0, "late_heavy"), "mask_minus": (4, "late_heavy"), "drop_last_split": (20, "late_heavy"), "merge_all_nsplit": (9, "plain"),
                     "no_rescale_merge": (13, "split_skew"), "no_rescale_wave": (15, "spike"), "gqa_mod": (7, "plain"), "table_of_seq0": (19, "early_heavy"),
                     "drop_second_trip": (17, "split_skew")}


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutation_is_rejected_by_a_case_of_the_gpu_list(mut):
    geo, lens = CAUGHT_BY_EXACT[mut]
    (e,) = [e for e in EXACT if e["geo"] == geo and e["lens"] == lens]
    c = build(e)
    caught = None
    for i, t in enumerate(R.target_sets(c)):
        c.set_targets(t)
        assert judge_exact(c, R.emulate(c, shape_of(c, e))[0]) is None
        out, _ = R.emulate(c, shape_of(c, e), mut=mut)
        msg = R.onehot_mismatch(out[:, :c.H * c.Dr].contiguous(), c)
        if msg is None and bool((out[:, c.H * c.Dr:] != SENT).any()):
            msg = "guard columns written"
        if msg is not None:
            caught = (i, msg)
            break
    assert caught, f"{mut}: the exact case {c} of the GPU list does not see it"
    print(f"[decode-attn-ref] {mut}: rejected by exact case {R.GEOS[geo][:4]} lens {lens}, target set {caught[0]}: {caught[1][:300]}")
    assert "target key" in caught[1] and "split" in caught[1] and "wave" in caught[1] or caught[1] == "guard columns written"
    if mut in CAUGHT_BY_BOUNDED:
        geo, kind = CAUGHT_BY_BOUNDED[mut]
        (e,) = [e for e in BOUNDED if e["geo"] == geo and e["kind"] == kind]
        c = R.bounded_case(kind, e["lens"], e["H"], e["KV"], e["Dr"], e["seed"])
        ref, bound, _ = R.elementwise_bound(c)
        msg, w = R.bound_violations(R.emulate(c, shape_of(c, e), mut=mut)[0][:, :c.H * c.Dr], ref, bound, c)
        assert msg is not None, f"{mut}: the bounded case {c} does not see it (worst err / bound {w:.3f})"
        print(f"[decode-attn-ref] {mut}: rejected by bounded case {R.GEOS[geo][:4]} {kind}: worst err / bound {w:.3g}")


def test_a_stale_record_is_only_read_by_a_wrong_merge():
    """the workspace discipline the GPU test asserts: a correct merge reads the ns records it published, whatever the rest of the workspace holds"""
    c = R.onehot_case([257, 4097], 4, 2, 64, seed=2)
    a, pa = R.emulate(c)
    b, pb = R.emulate(c, part=torch.zeros_like(R.decoy_part(c)))
    assert torch.equal(_bits(a), _bits(b)) and judge_exact(c, a) is None
    rec = pa.view(2, 4, 16, 66)
    assert bool((rec[0, :, 2:, 64] == R.DECOY_M).all()) and bool((rec[0, :, :2, 64] != R.DECOY_M).all()) and bool((rec[1, :, :, 64] != R.DECOY_M).all())


def test_a_single_wrong_bit_is_found_with_its_place():
    c = R.onehot_case([65, 833], 4, 2, 64, seed=4)
    out = R.emulate(c)[0][:, :256].contiguous()
    bits = _bits(out).clone()
    bits[1, 3 * 64 + 17] ^= 1
    msg = R.onehot_mismatch(bits.view(bf), c)
    t = int(c.target[1, 3])
    page, split, wave, trip = R.place(833, t)
    assert msg is not None and "1 of" in msg and "(sequence 1, head 3, d 17)" in msg and f"target key {t} in page {page}, split {split}, wave {wave}, trip {trip}" in msg, msg
    nan = out.clone()
    nan[0, 5] = float("nan")
    assert "1 of" in R.onehot_mismatch(nan, c)
