"""CPU tests of tests/attn_ref.py: the references of test_gpu_attn_exact.py can fail, and a correct implementation stays inside them.
attn_ref.emulate -- the kernel's documented arithmetic in plain torch -- stands in for a correct kernel; its mutations stand in for the kernel bugs that the old
max-over-the-output check() cannot see.  Every mutation must be rejected by the exact (one-hot) family AND by the bounded kind designed for it; where a mutation's damage is
confined to long rows the old statistic is asserted to stay inside its 1.5e-2 on plain data -- that blindness is the reason this file exists."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402

bf = torch.bfloat16
OLD_TOL = 1.5e-2            # tests/test_gpu_ops.py::test_attention


def maps(causal):
    return R.CAUSAL_MAPS if causal else R.FULL_MAPS


# (B, S, H, KV, Dr): every head dim of the issue, GQA ratios 1 / 2 / 4, lengths with a tail tile of 1 and of 63 keys, one wave, several query blocks
ONEHOT_SHAPES = [(2, 193, 4, 2, 16), (1, 257, 2, 2, 64), (2, 191, 4, 1, 88), (1, 320, 4, 4, 96), (1, 129, 4, 2, 128), (3, 33, 2, 1, 64), (1, 1, 2, 2, 16)]


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("B,S,H,KV,Dr", ONEHOT_SHAPES)
def test_emulation_reproduces_every_onehot_case_bit_for_bit(B, S, H, KV, Dr, causal):
    for target in maps(causal):
        c = R.onehot_case(B, S, H, KV, Dr, causal, target, seed=S + Dr)
        out = R.emulate(c, guard=3)
        msg = R.onehot_mismatch(out[:B * S], c)
        assert msg is None, msg
        assert bool((out[B * S:] == R.SENT).all())
        # the float64 softmax of the operands is one-hot at the target (the other keys: e^-128 and less, 0 in fp32 -- not in float64, where 2^100 e^-128 is a number)
        q, k, _ = c.split()
        s = torch.einsum("bihd,bjhd->bhij", q.double(), k.double().repeat_interleave(H // KV, dim=2))
        if causal:
            s = s.masked_fill(~torch.ones(S, S, dtype=torch.bool).tril(), float("-inf"))
        p = torch.softmax(s, -1)
        assert torch.equal(p.argmax(-1), c.target) and float(p.amax(-1).min()) == 1.0 and float((p.sum(-1) - 1).abs().max()) < 1e-50, f"{c}: not one-hot"


def test_onehot_operands_are_what_the_docstring_says():
    c = R.onehot_case(2, 577, 4, 2, 64, 0, "perm", seed=5)
    q, k, v = c.split()
    s = torch.einsum("bihd,bjhd->bhij", q.float(), k.float().repeat_interleave(2, dim=2))
    top = s.topk(2, dim=-1)
    assert float(s.abs().max()) <= 896 and bool((top.values[..., 0] - top.values[..., 1] >= 128).all())
    assert torch.equal(top.indices[..., 0], c.target)
    for bb in range(2):
        for hh in range(4):
            assert c.target[bb, hh].unique().numel() == 577, "perm: every key is some row's target"
    a = v.float().abs()
    assert float(a.min()) >= 2.0 ** -100 and float(a.max()) < 2.0 ** 101 and bool((v.float() < 0).any()) and bool((v.float() > 0).any())
    assert all(v[0, j, 0].view(torch.int16).unique().numel() == 64 for j in (0, 1, 576)), "V: distinct over d within a row"
    assert R._bits(v).view(-1, 64).unique(dim=0).shape[0] == 2 * 577 * 2, "V rows: distinct over (batch, key, KV head)"
    # the reference point must move with alpha = 0 on rows whose target is not in the first tile: a kernel that skips the rescale of O fails (see the mutation below)
    e = R.onehot_case(1, 257, 2, 2, 64, 0, "edges", seed=1)
    assert sorted(e.target.unique().tolist()) == [0, 31, 32, 63, 64, 65, 255, 256]


BOUNDED_SHAPES = [(2, 193, 4, 2, 64, 1), (1, 333, 2, 2, 88, 0), (2, 130, 4, 1, 128, 1), (1, 257, 2, 1, 16, 0), (1, 200, 2, 2, 96, 1)]


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("B,S,H,KV,Dr,causal", BOUNDED_SHAPES)
def test_emulation_stays_inside_the_elementwise_bound(B, S, H, KV, Dr, causal, kind):
    c = R.bounded_case(B, S, H, KV, Dr, causal, kind, seed=S + Dr)
    out = R.emulate(c)
    ref, bound, Abs = R.elementwise_bound(c)
    msg, worst = R.bound_violations(out, ref, bound, c)
    lead = float(((out.double() - ref).abs() / (2 * 2.0 ** -8 * Abs)).max())
    print(f"[attn-ref] emulation {c}: worst err / bound {worst:.3f} (err / (2 2^-8 Abs) {lead:.3f}); old statistic {R.old_stat(out, ref):.2e}, per-row statistic "
          f"{R.row_stat(out, ref, Abs, Dr):.2e}")
    assert msg is None, msg
    assert float(bound.min()) > 0
    # chunking does not change the reference
    ref2, bound2, _ = R.elementwise_bound(c, chunk=64)
    assert torch.allclose(ref, ref2, rtol=1e-13, atol=0) and torch.allclose(bound, bound2, rtol=1e-9, atol=0)


def rejected_by_onehot(mut, B, S, H, KV, Dr, causal, target, expect_in_msg=(), guard=0, mut_rows=None):
    c = R.onehot_case(B, S, H, KV, Dr, causal, target, seed=9)
    assert R.onehot_mismatch(R.emulate(c), c) is None
    out = R.emulate(c, mut=mut, guard=guard, mut_rows=mut_rows)
    msg = R.onehot_mismatch(out[:B * S], c)
    assert msg is not None, f"{mut}: the exact family ({target}) does not see it"
    for x in expect_in_msg:
        assert x in msg, (x, msg)
    return c, out, msg


def rejected_by_bounded(mut, B, S, H, KV, Dr, causal, kind, expect_in_msg=(), guard=0, mut_rows=None):
    c = R.bounded_case(B, S, H, KV, Dr, causal, kind, seed=21)
    ref, bound, Abs = R.elementwise_bound(c)
    msg, worst = R.bound_violations(R.emulate(c), ref, bound, c)
    assert msg is None, msg
    out = R.emulate(c, mut=mut, guard=guard, mut_rows=mut_rows)
    msg, w = R.bound_violations(out[:B * S], ref, bound, c)
    assert msg is not None, f"{mut}: the bounded kind {kind} does not see it (worst err / bound {w:.3f})"
    for x in expect_in_msg:
        assert x in msg, (x, msg)
    return c, out, msg


def old_statistic_on_plain(mut, B, S, H, KV, Dr, causal, mut_rows=None):
    c = R.bounded_case(B, S, H, KV, Dr, causal, "plain", seed=33)
    ref, bound, Abs = R.elementwise_bound(c)
    out = R.emulate(c, mut=mut, mut_rows=mut_rows)
    return R.old_stat(out, ref), R.old_stat(R.emulate(c), ref), R.bound_violations(out, ref, bound, c)[0]


def test_mutation_1_causal_mask_off_by_one():
    """key i hidden: exact `diag` (the target itself disappears) and bounded late_heavy.  key i + 1 visible: bounded late_heavy, where the leaked key takes e / (1 + e) of
    the mass; a one-hot row gives a leaked key p = 0 unless its query asks for that key, so the exact family sees it on rows whose query is the code of key i + 1 (below)"""
    rejected_by_onehot("mask_minus", 1, 193, 2, 2, 64, 1, "diag", ("target key",))
    rejected_by_bounded("mask_plus", 1, 193, 2, 2, 64, 1, "late_heavy", ("diagonal key",))
    rejected_by_bounded("mask_minus", 1, 193, 2, 2, 64, 1, "late_heavy")
    # rows of a causal one-hot case that take the query of key i + 1 from a permutation case: the leaked key's V row must come out
    c = R.onehot_case(1, 193, 2, 2, 64, 1, "diag", seed=9)
    c2 = R.onehot_case(1, 193, 2, 2, 64, 0, "perm", seed=9)
    q, k, v = c.split()
    q2, _, _ = c2.split()
    rows = (c2.target[0, 0] == torch.arange(193) + 1).nonzero().flatten()       # rows of the permutation that ask for key i + 1: under the causal mask they must NOT get it
    assert rows.numel() >= 1
    c.qkv.view(1, 193, 6, 64)[:, rows, 0] = q2[:, rows, 0]
    good, leak = R.emulate(c), R.emulate(c, mut="mask_plus")
    r = int(rows[0])
    assert not torch.equal(good[r, :64], leak[r, :64]) and torch.equal(leak[r, :64], v[0, r + 1, 0]), "the leaked key's V row must appear"


def test_mutation_2_diagonal_dropped_for_the_last_row_of_a_query_block():
    c, out, msg = rejected_by_onehot("drop_diag", 1, 384, 2, 2, 96, 1, "diag", ("i 127,", "i 383,", "target key 383", "wave 3", "key tile 5"))
    assert "12 of" not in msg and f"{3 * 2 * 96} of" in msg and "in 3 rows" in msg          # rows 127, 255, 383 of both heads, nothing else
    rejected_by_bounded("drop_diag", 1, 384, 2, 2, 96, 1, "late_heavy", ("i 127,", "i 383,"))
    # the old statistic: the damage in a LONG row (the last row of the last query block of S = 768) vanishes under the scale the first rows set
    S = 768
    old, clean, new = old_statistic_on_plain("drop_diag", 1, S, 2, 2, 96, 1, mut_rows=torch.tensor([S - 1]))
    print(f"[attn-ref] drop_diag in row {S - 1} only, plain data: old statistic {old:.2e} (clean {clean:.2e}, limit {OLD_TOL})")
    assert old <= OLD_TOL, "the old check() must be blind to this"


def test_mutation_3_pad_keys_unmasked_and_duplicating_the_last_key():
    """bounded: late_heavy non-causal (the mass sits on the last real keys: S - 1 counted 1 + n times).  exact: `last` with the V^T pages' zero pad; with the pad V duplicated
    too a one-hot row gives (1 + n) v / (1 + n) = v -- asserted, so that nobody relies on the exact family for it"""
    rejected_by_bounded("pad_dup", 1, 191, 2, 2, 64, 0, "late_heavy", ("last key 190",))         # 1 pad key
    rejected_by_bounded("pad_dup", 1, 193, 2, 2, 64, 0, "late_heavy")                            # 63 pad keys
    rejected_by_onehot("pad_dup_vzero", 1, 191, 2, 2, 64, 0, "last", ("target key 190",))
    c = R.onehot_case(1, 191, 2, 2, 64, 0, "last", seed=9)
    assert R.onehot_mismatch(R.emulate(c, mut="pad_dup"), c) is None, "documented blind spot of the one-hot family"


def test_mutation_4_keys_swapped_in_the_PV_product():
    c, out, msg = rejected_by_onehot("swap_pv", 1, 193, 2, 2, 64, 0, "perm", ("the whole output row equals the V row of key",))
    wrong = (R._bits(out) != R._bits(c.expect)).any(1)
    t = c.target[0]                                                                              # [H, S]: a row is wrong iff one of its heads targets a swapped key
    swapped = ((t % 16 == 3) | (t % 16 == 5)) & (t - t % 16 + 5 < 193)
    assert torch.equal(wrong, swapped.any(0))
    rejected_by_onehot("swap_pv", 1, 193, 2, 2, 64, 1, "diag", ("i 3,",))
    rejected_by_bounded("swap_pv", 1, 193, 2, 2, 64, 1, "late_heavy")


def test_mutation_5_gqa_head_mapping():
    _, _, msg = rejected_by_onehot("gqa_mod", 2, 129, 4, 2, 64, 0, "perm", ("h 1,",))
    rejected_by_onehot("gqa_mod", 1, 129, 4, 2, 64, 1, "diag")
    rejected_by_bounded("gqa_mod", 2, 129, 4, 2, 64, 1, "scaled_rows", ("h 1,",))
    c = R.onehot_case(1, 129, 4, 4, 64, 0, "perm", seed=9)                                       # ratio 1: h % KV == h // 1, not a mutation
    assert R.onehot_mismatch(R.emulate(c, mut="gqa_mod"), c) is None


def test_mutation_6_rescale_of_O_skipped():
    rejected_by_onehot("no_rescale_O", 1, 257, 2, 2, 64, 0, "last", ("target key 256", "key tile 4"))
    rejected_by_onehot("no_rescale_O", 1, 257, 2, 2, 64, 1, "diag")
    rejected_by_bounded("no_rescale_O", 1, 257, 2, 2, 64, 0, "spike")
    rejected_by_bounded("no_rescale_O", 1, 257, 2, 2, 64, 1, "spike")
    old, clean, new = old_statistic_on_plain("no_rescale_O", 1, 257, 2, 2, 64, 0)
    print(f"[attn-ref] no_rescale_O, plain data: old statistic {old:.2e} (clean {clean:.2e}, limit {OLD_TOL})")
    assert old <= OLD_TOL, "on std-1 data the reference never moves after a row's first tile: the old check() is blind to this"


def test_mutation_7_last_eight_columns_unwritten():
    _, _, msg = rejected_by_onehot("skip_last8", 1, 65, 2, 2, 88, 0, "edges", ("d 80)", "d 87)"))
    assert f"{65 * 2 * 8} of" in msg
    rejected_by_bounded("skip_last8", 1, 65, 2, 2, 88, 0, "scaled_rows", ("d 80)", "d 87)"))


def test_mutation_8_rows_beyond_S_written():
    B, S = 2, 130
    t0 = int(R.onehot_case(B, S, 2, 2, 64, 0, "perm", seed=9).target[0, 0, S - 1])
    c, out, msg = rejected_by_onehot("rows_shift", B, S, 2, 2, 64, 0, "perm", ("(b 1, h 0, i 0, d 0)", f"equals the V row of key {t0} (batch 0, KV head 0;"), guard=4)
    assert "in 1 rows" in msg                                                                    # batch 1's row 0 took batch 0's query 129
    touched = (out[B * S:] != R.SENT).nonzero()
    assert touched.numel() and int(touched[0][0]) == 0, "and the first row behind the output is written"
    assert bool((R.emulate(c, guard=4)[B * S:] == R.SENT).all())
    rejected_by_bounded("rows_shift", B, S, 2, 2, 64, 0, "scaled_rows", ("(b 1, h 0, i 0,",), guard=4)


def test_a_single_wrong_bit_is_found_with_its_place():
    c = R.onehot_case(2, 300, 4, 2, 64, 1, "hash", seed=4)
    out = R.emulate(c)
    bits = R._bits(out).clone()
    bits[300 + 290, 3 * 64 + 17] ^= 1
    msg = R.onehot_mismatch(bits.view(bf), c)
    t = int(c.target[1, 3, 290])
    assert msg is not None and "1 of" in msg and "(b 1, h 3, i 290, d 17)" in msg and f"target key {t}, query block 2, wave 1, key tile {t // 64}" in msg, msg
    assert R.old_stat(bits.view(bf), c.expect.double()) <= OLD_TOL
    nan = out.clone()
    nan[5, 5] = float("nan")
    assert "1 of" in R.onehot_mismatch(nan, c)
