"""-m gpu: score_rows_kernel (csrc/gvl_pick.hip) through gvl_op_score_rows -- the log-probability, rank and top list of a GIVEN id per row of fp32 logits --
against the float64 restatement tests/score_ref.py, and bit for bit against the selection kernels' log-probability mode (gvl_op_select_logprobs) on the same rows.
Widths: 100 (below one block's stride of 1024), 640, 1025 (one past it), 32064 and 128256 (the two real vocabularies); 1, 3 and 65 rows (more than the 16 a
selection launch takes).  Rows as test_gpu_logprobs._rows builds them: wide ranges, ties, -inf entries, a tie at the maximum, a row with fewer finite entries than N.
Targets: the maximum (id 3), its tie (11: rank 1), a -inf entry on odd rows (7), id 0 and its ties (5), id n - 1."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import score_ref as R  # noqa: E402
from gpu_util import DEV  # noqa: E402
from grounded_video_llm_amd.lib import GvlError  # noqa: E402

from test_gpu_extend_varlen import make_engine  # noqa: E402  (a tiny LLM-only engine: the operator needs a context, not a model)
from test_gpu_logprobs import _rows, tol  # noqa: E402

WIDTHS = [100, 640, 1025, 32064, 128256]
ROWS = [1, 3, 65]


@pytest.fixture(scope="module")
def eng():
    e, _ = make_engine("phi_d64")
    yield e
    e.close()


def bits(t):
    return t.contiguous().view(torch.int32)


def target_sets(n, B):
    """six target vectors: each kind of target on every row once"""
    kinds = [3, 11, 7, 0, n - 1, 5]
    return [[kinds[(b + s) % 6] for b in range(B)] for s in range(6)]


_REF = {}


def reference(n, B):
    """(rows, per row float64 log-probabilities, per row top-8 (ids, values)) -- computed once per shape and shared"""
    if (n, B) not in _REF:
        x = _rows(torch.Generator().manual_seed(1000 * B + n), B, n)
        lps = [R.logprobs(x[b].numpy()) for b in range(B)]
        _REF[(n, B)] = (x, lps, [R.top(x[b].numpy(), 8, lps[b]) for b in range(B)])
    return _REF[(n, B)]


@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("B", ROWS)
def test_against_the_float64_restatement(eng, n, B):
    x, lps, tops = reference(n, B)
    xd = x.to(DEV).contiguous()
    worst = 0.0
    for s, tg in enumerate(target_sets(n, B)):
        top_n = (8, 0, 3)[s % 3]
        lp, rank, ti, tv = (t.cpu() for t in eng.op_score_rows(xd, tg, top_n))
        for b in range(B):
            row = x[b].numpy()
            want = float(lps[b][tg[b]])
            got = float(lp[b])
            if want == -math.inf:
                assert got == -math.inf, (n, B, b, tg[b], got)
            else:
                assert abs(got - want) <= tol(want), (n, B, b, tg[b], got, want)
                worst = max(worst, abs(got - want))
            assert int(rank[b]) == R.rank(row, tg[b]), (n, B, b, tg[b])
            if top_n == 0:
                assert ti[b].tolist() == [-2] * 8 and all(math.isnan(v) for v in tv[b].tolist())          # untouched
                continue
            ids, vals = tops[b]
            ids, vals = ids[:top_n] + [-1] * (8 - top_n), vals[:top_n] + [-math.inf] * (8 - top_n)
            assert ti[b].tolist() == ids, (n, B, b)
            for j in range(8):
                g = float(tv[b, j])
                assert (g == vals[j] == -math.inf) or abs(g - vals[j]) <= tol(vals[j]), (n, B, b, j, g, vals[j])
            if int(rank[b]) < top_n and math.isfinite(row[tg[b]]):
                assert int(ti[b, int(rank[b])]) == tg[b] and float(tv[b, int(rank[b])]) == got          # a listed target sits at its rank, with its value
    print(f"[parity] score_rows n {n} rows {B}: max |lp - float64| = {worst:.3e} (tol 1e-4 + 1e-5 |ref|)")


@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("B", ROWS)
def test_bitwise_against_the_selection_kernels(eng, n, B):
    """the same rows through greedy selection with log-probabilities and the top 8, 16 rows at a time: equal top lists; lp equal to the selected token's where the
    target is the argmax, and to the list's entry wherever the target is listed"""
    x, _, _ = reference(n, B)
    xd = x.to(DEV).contiguous()
    sel = [eng.op_select_logprobs(xd[b0:b0 + 16], 8) for b0 in range(0, B, 16)]
    toks, slp, sti, stv = (torch.cat([s[j] for s in sel]) for j in range(4))
    hit_argmax = hit_listed = 0
    for tg in target_sets(n, B):
        lp, rank, ti, tv = eng.op_score_rows(xd, tg, 8)
        assert torch.equal(ti, sti) and torch.equal(bits(tv), bits(stv)), (n, B)
        t = torch.tensor(tg, dtype=torch.int32, device=DEV)
        am = t == toks
        assert torch.equal(bits(lp[am]), bits(slp[am])) and bool((rank[am] == 0).all()) and bool((rank[~am] > 0).all())
        listed = sti == t[:, None]
        assert torch.equal(bits(lp[listed.any(1)]), bits(stv[listed])), (n, B)
        assert torch.equal(rank[listed.any(1)].long(), listed.long().argmax(1)[listed.any(1)])
        hit_argmax += int(am.sum()); hit_listed += int(listed.any(1).sum())
    assert hit_argmax >= 1 and hit_listed > hit_argmax


def test_row_stride_and_rows_do_not_matter(eng):
    """a row's results do not depend on where it sits: rows ld > n apart (a slice of a wider buffer, 4-byte aligned rows only), and each row on its own"""
    n, B = 1025, 65
    x, _, _ = reference(n, B)
    xd = x.to(DEV).contiguous()
    wide = torch.full((B, n + 3), 77.0, device=DEV)                 # what lies between the rows would win every maximum if it were read
    wide[:, :n] = xd
    tg = target_sets(n, B)[0]
    a = eng.op_score_rows(xd, tg, 8)
    b = eng.op_score_rows(wide[:, :n], tg, 8)
    for u, v in zip(a, b):
        assert torch.equal(bits(u), bits(v))
    for r in (0, 2, 17, 64):
        one = eng.op_score_rows(xd[r:r + 1], tg[r:r + 1], 8)
        for u, v in zip(a, one):
            assert torch.equal(bits(u[r:r + 1]), bits(v))


def test_refusals_leave_the_outputs_untouched(eng):
    n, B = 640, 3
    x, _, _ = reference(n, B)
    xd = x.to(DEV).contiguous()

    def fresh():
        return (torch.full((B,), 5.0, device=DEV), torch.full((B,), 55, dtype=torch.int32, device=DEV),
                torch.full((B, 8), 555, dtype=torch.int32, device=DEV), torch.full((B, 8), 5.5, device=DEV))

    for top_n in (9, -1):
        out = fresh()
        with pytest.raises(GvlError):
            eng.op_score_rows(xd, [0, 1, 2], top_n, out=out)
        torch.cuda.synchronize()
        assert all(torch.equal(u, v) for u, v in zip(out, fresh()))
    for bad in ([0, n, 2], [0, 1, -1]):
        out = fresh()
        with pytest.raises(ValueError):
            eng.op_score_rows(xd, bad, 8, out=out)
        torch.cuda.synchronize()
        assert all(torch.equal(u, v) for u, v in zip(out, fresh()))
    # top_n = 0 writes lp and rank only
    out = fresh()
    eng.op_score_rows(xd, [3, 3, 17], 0, out=out)
    assert torch.equal(out[2], fresh()[2]) and torch.equal(out[3], fresh()[3]) and out[1].tolist() == [0, 0, 0]
    # targets that live on the device are taken as they are: one outside [0, n) never indexes its row
    lp, rank, ti, tv = eng.op_score_rows(xd, torch.tensor([n, 3, -7], dtype=torch.int32, device=DEV), 8)
    assert lp.tolist()[0] == -math.inf and lp.tolist()[2] == -math.inf and rank.tolist() == [-1, 0, -1]
    assert torch.equal(ti, eng.op_score_rows(xd, [0, 3, 0], 8)[2])
