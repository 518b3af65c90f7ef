"""CPU tests of tests/prefill_attn_ref.py: the references of test_gpu_prefill_attn.py can fail, and a correct implementation stays inside them.
prefill_attn_ref.emulate -- attn_fwd_kernel's documented arithmetic reading the pages through the tables -- stands in for a correct kernel over THE lists the GPU test
runs, and with mut=... for twelve wrong ones: every one of them must be reported by the comparisons the GPU test asserts with, on cases of those lists.
Three more wrong kernels form a page's offset in 32 bits: they are the identity on those lists and must be reported on every relocated case
(prefill_attn_ref.relocated_cases), read through sparse pools."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as A  # noqa: E402
import prefill_attn_ref as P  # noqa: E402
from attn_ref import _bits  # noqa: E402

EXACT, GROUPS_EXACT, BOUNDED, GROUPS_BOUNDED = P.exact_cases(), P.group_cases("exact"), P.bounded_cases(), P.group_cases("bounded")


def test_without_a_prefix_it_is_attn_ref_bit_for_bit():
    """qpos0 = 0, Sk = S, one member: the same data, the same expectation and the same emulated output as attn_ref -- the generalisation adds nothing of its own"""
    for S, H, KV, Dr, target in ((130, 4, 2, 64, "diag"), (65, 4, 4, 32, "hash"), (200, 8, 1, 80, "tile_first"), (129, 4, 2, 128, "zero")):
        D = 64 if Dr <= 64 else 96 if Dr <= 96 else 128
        c = P.make(dict(form="single", B=1, S=S, qpos0=0, Sk=S, H=H, KV=KV, D=D, Dout=Dr, causal=1, ring=0, target=target, seed=5))
        a = A.onehot_case(1, S, H, KV, Dr, 1, target, 5)
        q, k, v = a.split()
        assert torch.equal(_bits(c.q[0]), _bits(q[0])) and torch.equal(_bits(c.k[0]), _bits(k[0])) and torch.equal(_bits(c.v[0]), _bits(v[0]))
        assert torch.equal(_bits(c.expect), _bits(a.expect)) and torch.equal(c.target[0], a.target[0])
        assert torch.equal(_bits(P.emulate(c)), _bits(A.emulate(a, guard=P.GUARD_ROWS)))
    for kind in A.KINDS:
        c = P.make(dict(form="single", B=1, S=150, qpos0=0, Sk=150, H=4, KV=2, D=96, Dout=80, causal=1, ring=0, kind=kind, seed=3))
        assert torch.equal(_bits(P.emulate(c)), _bits(A.emulate(c.full[0], guard=P.GUARD_ROWS))), kind
        ref, bound = P.elementwise_bound(c)
        r, b, _ = A.elementwise_bound(c.full[0])
        assert torch.equal(ref, r) and torch.equal(bound, b)


def test_the_pools_are_what_the_file_says():
    s = next(s for s in GROUPS_EXACT if s.get("share"))
    c = P.make(s)
    m0, m1 = c.members[0], c.members[1]
    assert m1.table[:3] == m0.table[:3] and m1.table[3] != m0.table[3] and m1.qpos0 == 192, "two members share their prefix pages"
    for c in (c, P.make(EXACT[40]), P.make(BOUNDED[52])):
        named = set()
        for m in c.members:
            tiles = (m.Sk + 63) // 64
            assert len(m.table) > tiles and not 0 <= m.table[tiles] < c.n_pages, "a spare entry behind the tiles that is no page"
            named |= set(m.table[:tiles])
            if m.Sk % 64:
                pg, n = m.table[tiles - 1], m.Sk % 64
                assert bool(torch.isnan(c.Kt[pg, :, n:].float()).all()) and bool((c.Vt[pg, :, :c.Dr, n:].float().abs() == float(torch.tensor(P.VPAD).to(P.bf))).all())
                assert bool(torch.isfinite(c.Kt[pg, :, :n].float()).all()) and bool(torch.isfinite(c.Vt[pg].float()).all())
        free = sorted(set(range(c.n_pages)) - named)
        assert len(free) == 4 and bool(torch.isnan(c.Kt[free].float()).all()) and bool(torch.isnan(c.Vt[free].float()).all())
        assert [m.table[t] for m in c.members for t in range((m.Sk + 63) // 64)] != list(range(len(named))), "not the implicit page order"
        assert bool(torch.isnan(c.Q[c.rows * c.H * c.D:].float()).all())


def test_the_lists_hold_what_the_kernel_branches_on():
    single = EXACT + BOUNDED
    shapes = {(s["qpos0"], s["S"]) for s in single if s["Sk"] == s["qpos0"] + s["S"] and s["causal"]}
    assert shapes == set(P.SHAPES) == {(64, 1), (64, 31), (64, 33), (64, 64), (64, 65), (128, 129), (192, 130), (0, 130), (960, 65)}
    assert any(s["causal"] and s["Sk"] == s["qpos0"] + s["S"] + 70 for s in EXACT) and any(not s["causal"] and s["Sk"] > s["S"] for s in EXACT)
    for lst in (EXACT, BOUNDED):
        assert {(s["D"], s["Dout"]) for s in lst} == set(P.DGEOS) and {(s["H"], s["KV"]) for s in lst} == set(P.HKV) and {s["B"] for s in lst} == {1, 2} and {s["ring"] for s in lst} == {0, 2, 3}
    for sh in P.SHAPES:
        mine = [s for s in EXACT if (s["qpos0"], s["S"]) == sh and s["Sk"] == sum(sh)]
        assert {s["target"] for s in mine} == set(P.CAUSAL_MAPS) and {(s["D"], s["Dout"]) for s in mine} == set(P.DGEOS)
        assert {s["kind"] for s in BOUNDED if (s["qpos0"], s["S"]) == sh} == set(A.KINDS)
    assert {len(g) for g in P.GROUPS} == {1, 2, 8} and {x for g in P.GROUPS for x in g} == {1, 65, 128, 129, 31}
    for lst in (GROUPS_EXACT, GROUPS_BOUNDED):
        for D, Dout in P.DGEOS:
            mine = [s for s in lst if (s["D"], s["Dout"]) == (D, Dout) and not s.get("share")]
            assert {(s["form"], tuple(s["lens"])) for s in mine} == {(f, g) for f in ("ragged", "ext") for g in P.GROUPS}
            assert any(s["form"] == "ext" and set(s["vl_pos0"][:len(s["lens"])]) == {0} for s in mine) and any(s["form"] == "ext" and set(s["vl_pos0"]) == {0, 64, 192} for s in mine)


def test_a_correct_implementation_passes_every_exact_case_and_the_bounded_ones_tried_here():
    for s in EXACT + GROUPS_EXACT:
        c = P.make(s)
        out = P.emulate(c)
        msg = P.onehot_mismatch(out[:c.rows], c)
        assert msg is None, msg
        assert bool((out[c.rows:] == P.SENT).all())
    worst = 0.0
    for s in BOUNDED[::3] + GROUPS_BOUNDED[::4]:
        c = P.make(s)
        ref, bound = P.elementwise_bound(c)
        msg, w = P.bound_violations(P.emulate(c)[:c.rows], ref, bound, c)
        assert msg is None, msg
        worst = max(worst, w)
    assert 0.3 < worst <= 1.0


def _caught(s, mut):
    c = P.make(s)
    out = P.emulate(c, mut)[:c.rows]
    if "target" in s:
        return P.onehot_mismatch(out, c)
    ref, bound = P.elementwise_bound(c)
    return P.bound_violations(out, ref, bound, c)[0]


def pick(lst, **kw):
    return [s for s in lst if all(s.get(k) == v for k, v in kw.items())]


# mutation -> the cases of the GPU lists that exist for it (each one MUST report it)
PROOFS = {
    "mask_plus": pick(BOUNDED, kind="late_heavy", qpos0=64, S=33) + pick(BOUNDED, kind="late_heavy", qpos0=960),
    "mask_minus": pick(EXACT, target="diag", D=96)[:4] + pick(GROUPS_EXACT, target="diag", D=64, form="ext")[:2],
    "skip_no_qpos0": pick(EXACT, target="diag", qpos0=64, S=33)[:2] + pick(EXACT, target="first_new", qpos0=960)[:2] + pick(GROUPS_EXACT, target="diag", form="ext", vl_pos0=P.EXT_POS0[0])[:3],
    "mask_no_qpos0": pick(EXACT, target="diag", qpos0=64, S=65)[:2] + pick(EXACT, target="first_new", qpos0=192)[:2] + pick(GROUPS_EXACT, target="tile_first", form="ext", vl_pos0=P.EXT_POS0[0])[:3],
    "n_tiles_from_S": pick(EXACT, target="diag", qpos0=128)[:2] + pick(EXACT, target="first_new", qpos0=64, S=1)[:2] + pick(GROUPS_EXACT, target="diag", form="ext", vl_pos0=P.EXT_POS0[0])[:3],
    "no_tail_mask": pick(EXACT, causal=0),
    "wrong_member_table": pick(EXACT, B=2, target="diag")[:3] + pick(GROUPS_EXACT, target="zero", lens=P.GROUPS[1])[:3] + pick(GROUPS_EXACT, target="hash", lens=P.GROUPS[2])[:2],
    "prefix_offset_dropped": pick(EXACT, target="diag", qpos0=64, S=64)[:2] + pick(EXACT, target="first_new", qpos0=960)[:1] + pick(GROUPS_EXACT, target="diag", form="ext", vl_pos0=P.EXT_POS0[0])[:3],
    "member_off_by_one": pick(GROUPS_EXACT, target="zero", lens=P.GROUPS[1])[:3] + pick(GROUPS_EXACT, target="diag", lens=P.GROUPS[2])[:3] + pick(GROUPS_EXACT, target="hash", share=(1, 0)),
    "gqa_mod": pick(EXACT, H=4, KV=2, target="hash")[:3] + pick(GROUPS_EXACT, H=4, KV=2, target="diag")[:2],
    "no_rescale_O": pick(BOUNDED, kind="spike", qpos0=192) + pick(BOUNDED, kind="late_heavy", qpos0=960) + pick(GROUPS_BOUNDED, kind="late_heavy")[:2],
    "skip_last8": pick(EXACT, target="zero")[:3] + pick(GROUPS_EXACT, target="zero")[:2],
}


@pytest.mark.parametrize("mut", [m for m in P.MUTATIONS if m not in P.PAGE_MUTATIONS])             # the page mutations: test_page_offsets_formed_in_32_bits_...
def test_every_mutation_is_caught_by_the_comparisons_of_the_gpu_test(mut):
    assert len(PROOFS[mut]) >= 2, mut
    for s in PROOFS[mut]:
        msg = _caught(s, mut)
        assert msg is not None, f"{mut} is not reported on {s}"
        assert "member" in msg and ("query block" in msg) and "wave" in msg, msg
    print(f"[mutation] {mut}: caught on {len(PROOFS[mut])} cases; e.g. {msg[:400]}")


def test_dropping_qpos0_from_the_need_mask_predicate_alone_changes_no_bit():
    """(t * 64 + 63 > qw) is true wherever (t * 64 + 63 > qpos0 + qw) is: the mask is applied to tiles that need none, every key of which passes it"""
    for s in pick(EXACT, target="hash")[::4] + pick(GROUPS_EXACT, target="hash", form="ext")[::3] + BOUNDED[::11]:
        c = P.make(s)
        assert torch.equal(_bits(P.emulate(c, "need_mask_pred_no_qpos0")), _bits(P.emulate(c))), s


def test_a_group_member_is_its_own_single_sequence_launch_in_the_reference_too():
    for s in GROUPS_BOUNDED[::5] + pick(GROUPS_EXACT, target="hash")[::4]:
        c = P.make(s)
        whole = P.emulate(c)
        for u, m in enumerate(c.members):
            d = P.single_launch_of(c, u)
            assert (d.qpos0, d.Sk) == (m.qpos0, m.qpos0 + m.S) and torch.equal(_bits(P.emulate(d)[:m.S]), _bits(whole[m.row0:m.row0 + m.S]))


# ---- the relocated cases ------------------------------------------------------------------------------------------------------------------------------------------------
RELOCATED = P.relocated_cases()


def _judge(c, out):
    if hasattr(c, "target"):
        return P.onehot_mismatch(out, c)
    ref, bound = P.elementwise_bound(c)
    return P.bound_violations(out, ref, bound, c)[0]


def test_the_relocated_cases_are_cases_of_the_lists_on_pages_above_2_to_the_31():
    every = EXACT + GROUPS_EXACT + BOUNDED + GROUPS_BOUNDED
    assert all(s in every for s, _ in RELOCATED) and sorted(k for _, k in RELOCATED) == [30] + [31] * (len(RELOCATED) - 1)
    hi = [s for s, k in RELOCATED if k == 31]
    single = [s for s in hi if s["form"] == "single"]
    assert {s["causal"] for s in single} == {0, 1} and 0 in {s["ring"] for s in single} and {s["ring"] for s in single} - {0}
    assert any(s["form"] == "ragged" and len(s["lens"]) == 8 for s in hi) and any(s["form"] == "ext" and s.get("share") for s in hi)
    assert any(s["form"] == "ext" and len(s["lens"]) == 8 and any(s["vl_pos0"]) for s in hi) and {s["D"] for s in hi} == {64, 96, 128} and any("kind" in s for s in hi)
    for s, k in RELOCATED:
        c, small = P.make_relocated(s, k), P.make(s)
        pe = c.KV * 64 * c.D
        named = sorted({m.table[t] for m in c.members for t in range((m.Sk + 63) // 64)})
        assert c.page_elems == pe and c.n_pages == P.POOL_ELEMS // pe and min(named) * pe >= 1 << k and (c.page0 - 1) * pe < 1 << k
        assert k == 31 or (1 << 31) <= min(named) * pe * 2 and (max(named) + 1) * pe * 2 <= 1 << 32
        assert sorted(c.Kt.pages) == named == sorted(c.Vt.pages), "only the named pages are written"
        for m, ms in zip(c.members, small.members):
            assert [x - c.page0 for x in m.table[:-1]] == ms.table[:-1] and not 0 <= m.table[-1] < c.n_pages, "the same permutation, moved; the spare entry is no page"
            for t in range((m.Sk + 63) // 64):               # the same pages, bit for bit
                assert torch.equal(_bits(c.Kt[m.table[t]]), _bits(small.Kt[ms.table[t]])) and torch.equal(_bits(c.Vt[m.table[t]]), _bits(small.Vt[ms.table[t]]))
        assert torch.equal(_bits(c.Q), _bits(small.Q))
        if "target" in s:
            assert torch.equal(_bits(c.expect), _bits(small.expect))


@pytest.mark.parametrize("n", range(len(RELOCATED)))
def test_page_offsets_formed_in_32_bits_are_caught_on_every_relocated_case(n):
    """the unmutated emulation, reading the sparse pools through the tables, passes and equals the emulation on the small pools bit for bit; a page offset taken mod 2^31
    elements or mod 2^32 bytes is reported on every case above 2^31 elements.  On the case above 2^30 those two ARE the identity (every offset is below 2^31 elements =
    2^32 bytes) -- what that placement catches is the SIGNED 32-bit byte offset, which every case reports."""
    s, k = RELOCATED[n]
    c = P.make_relocated(s, k)
    ok = P.emulate(c)
    assert _judge(c, ok[:c.rows]) is None and torch.equal(_bits(ok), _bits(P.emulate(P.make(s))))
    for mut in P.PAGE_MUTATIONS:
        out = P.emulate(c, mut)
        if k == 30 and mut != "page_byte_int32":
            assert torch.equal(_bits(out), _bits(ok))
            continue
        msg = _judge(c, out[:c.rows])
        assert msg is not None and "member" in msg and "query block" in msg, (mut, msg)
        assert bool(torch.isnan(out[:c.rows].float()).all()), "every row multiplies the NaN it finds in front of the case's pages"
    small = P.make(s)                                        # on the small pools of the lists the three are the identity
    for mut in P.PAGE_MUTATIONS:
        assert torch.equal(_bits(P.emulate(small, mut)), _bits(P.emulate(small)))
