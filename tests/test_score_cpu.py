"""CPU: the two host-side halves of teacher-forced scoring.  tests/score_ref.py (the float64 row semantics the GPU operator test compares against) against
torch.log_softmax and a plain sort, on seeded rows with ties, -inf entries and a tie at the maximum; and grounded_video_llm_amd/scoring.py (row / target assembly, folding
of the packed device outputs) on hand-written cases."""
import math

import numpy as np
import pytest
import torch

import score_ref as R
from grounded_video_llm_amd import lib, scoring as SC


def rows(seed, B, n):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, n), generator=g) * torch.tensor([0.5, 2.0, 4.0, 30.0])[torch.arange(B) % 4][:, None]
    x[:, 5::97] = x[:, :1]                                          # ties with entry 0
    x[1::2, 7::13] = -math.inf
    x[:, 11] = x.max(dim=1).values                                  # a tie at the maximum: the lower id wins
    x[:, 3] = x[:, 11]
    x[2, :] = -math.inf
    x[2, [17, 40, 41]] = torch.tensor([1.0, 0.5, 0.5])              # fewer finite entries than N
    return x


@pytest.mark.parametrize("n", [100, 1025])
def test_ref_against_log_softmax_and_a_sort(n):
    x = rows(n, 6, n)
    for b in range(x.shape[0]):
        row = x[b].numpy()
        want = torch.log_softmax(x[b].double(), dim=-1).numpy()
        got = R.logprobs(row)
        fin = np.isfinite(want)
        assert np.array_equal(fin, np.isfinite(got)) and np.all(got[~fin] == -math.inf)
        assert np.max(np.abs(got[fin] - want[fin])) < 1e-12
        # the strict order by a plain sort of (-value, id) pairs over ALL entries
        order = sorted(range(n), key=lambda i: (-float(row[i]), i))
        pos = {i: r for r, i in enumerate(order)}
        for t in (0, 3, 5, 7, 11, 17, 41, n - 1, int(np.argmax(row))):
            lp, rk, ids, vals = R.score_row(row, t, 8)
            assert rk == pos[t], (b, t)
            assert (lp == want[t]) or abs(lp - want[t]) < 1e-12
            finite = [i for i in order if math.isfinite(row[i])][:8]
            assert ids == finite + [-1] * (8 - len(finite))
            assert all((v == -math.inf) if i < 0 else abs(v - want[i]) < 1e-12 for i, v in zip(ids, vals))
            if rk < 8 and math.isfinite(row[t]):
                assert ids[rk] == t and vals[rk] == lp              # a listed target sits at its rank
        # the tie at the maximum: entries 3 and 11 hold it, 3 wins
        if b != 2:
            assert R.rank(row, 3) == 0 and R.rank(row, 11) == 1 and R.top(row, 2)[0] == [3, 11]
        assert R.score_row(row, 5, 0)[2:] == ([], [])
    assert R.top(x[2].numpy(), 8)[0] == [17, 40, 41] + [-1] * 5 and R.top(x[2].numpy(), 8)[1][3:] == [-math.inf] * 5
    assert R.score_row(x[1].numpy(), 7, 0)[0] == -math.inf           # a target at -inf
    assert R.rank(x[1].numpy(), 7) == int(np.isfinite(x[1].numpy()).sum())   # behind every finite entry, first of the -inf ones


def test_assemble_rows_and_targets():
    # 5 prompt rows, continuation [7, 8, 9], no prefix: rows 0 .. 7; row 4 predicts 7, row 5 -> 8, row 6 -> 9, row 7 (the last continuation token) is fed, not scored
    sl, nxt = SC.assemble(5, [7, 8, 9], 0, 64)
    assert (sl.start, sl.stop) == (0, 8) and nxt == [-100] * 4 + [7, 8, 9, -100]
    # behind a prefix of 128 of 130 prompt rows: rows 128 .. 132 run
    sl, nxt = SC.assemble(130, [7, 8, 9], 128, 4096)
    assert (sl.start, sl.stop) == (128, 133) and nxt == [-100, 7, 8, 9, -100]
    # the prefix may reach up to the last prompt row, never over it
    sl, nxt = SC.assemble(129, [4], 128, 4096)
    assert (sl.start, sl.stop) == (128, 130) and nxt == [4, -100]
    with pytest.raises(ValueError, match="last prompt row"):
        SC.assemble(128, [4], 128, 4096)
    # one-token continuation from scratch
    assert SC.assemble(3, [9], 0, 16)[1] == [-100, -100, 9, -100]
    # over length: never truncated
    assert SC.assemble(10, [1] * 6, 0, 16)[0].stop == 16
    with pytest.raises(ValueError, match="never truncates"):
        SC.assemble(10, [1] * 7, 0, 16)
    with pytest.raises(ValueError):
        SC.assemble(10, [], 0, 16)
    # the scored rows are exactly the continuation's tokens, in order
    for P, C, prefix in ((5, 3, 0), (130, 12, 128), (200, 1, 128)):
        c = list(range(50, 50 + C))
        nxt = SC.assemble(P, c, prefix, 4096)[1]
        assert [t for t in nxt if t != SC.NOT_SCORED] == c and len(nxt) == P + C - prefix


def test_continuation_ids_and_eos():
    tok = lambda s: [1] + [10 + len(w) for w in s.split()]           # a tokenizer that prepends BOS = 1
    assert SC.continuation_ids(tok, "a bb ccc", 1) == [11, 12, 13]
    assert SC.continuation_ids(tok, "a bb", 1, append_eos=True, eos_token_id=2) == [11, 12, 2]
    assert SC.continuation_ids(lambda s: [11, 12], "x", 1) == [11, 12]          # a tokenizer without BOS: nothing is stripped
    assert SC.continuation_ids(tok, "a", None) == [1, 11]                       # no BOS id known: the ids as they come
    assert SC.with_eos([5], True, 2) == [5, 2]
    with pytest.raises(ValueError, match="eos_token_id"):
        SC.with_eos([5], True, None)
    with pytest.raises(ValueError, match="at least one token"):
        SC.continuation_ids(tok, "", 1)
    # append_eos adds one scored row: the row of the last text token predicts EOS
    assert SC.assemble(4, SC.with_eos([7, 8], True, 2), 0, 64)[1] == [-100, -100, -100, 7, 8, 2, -100]


def test_fold_packed_outputs():
    conts = [[7, 8, 9], [4]]
    lp = [-0.5, -1.5, -2.0, -0.25]
    rank = [0, 3, 1, 0]
    out = SC.fold(conts, lp, rank)
    assert [o.token_ids for o in out] == conts and [o.token_logprobs for o in out] == [[-0.5, -1.5, -2.0], [-0.25]]
    assert [o.ranks for o in out] == [[0, 3, 1], [0]] and all(o.top_logprobs is None for o in out)
    assert out[0].sum_logprob == -4.0 and out[0].mean_logprob == -4.0 / 3 and out[1].sum_logprob == out[1].mean_logprob == -0.25
    ti = [[7, 1, -1, -1, -1, -1, -1, -1], [2, 3, 8, -1, -1, -1, -1, -1], [5, 9, 1, 2, 3, 4, 6, 7], [4, -1, -1, -1, -1, -1, -1, -1]]
    tv = [[-0.5, -1.0] + [-math.inf] * 6, [-0.1, -0.2, -1.5] + [-math.inf] * 5, [-1.0, -2.0, -3.0, -4.0, -5.0, -6.0, -7.0, -8.0], [-0.25] + [-math.inf] * 7]
    out = SC.fold(conts, lp, rank, ti, tv, 3)
    assert out[0].top_logprobs == [[(7, -0.5), (1, -1.0)], [(2, -0.1), (3, -0.2), (8, -1.5)], [(5, -1.0), (9, -2.0), (1, -3.0)]]     # first top_n, padding dropped
    assert out[1].top_logprobs == [[(4, -0.25)]]
    with pytest.raises(ValueError):
        SC.fold(conts, lp[:3], rank[:3])
    assert SC.resolve_top(None) == 0 and SC.resolve_top(8) == 8
    for bad in (9, -1, True, 2.0):
        with pytest.raises(ValueError):
            SC.resolve_top(bad)


def test_abi_binds_the_scoring_entry_points():
    for name in ("gvl_score_extend_varlen", "gvl_op_score_rows"):
        assert name in lib.EXPORTS
