"""CPU tests of tests/gemm_ref.py: the references of test_gpu_gemm_exact.py can fail, and a correct implementation stays inside them.
A plain torch emulation of the kernels' documented arithmetic (bf16 operands, fp32 matmul, the rounding points of gvl_gemm_epi.h) stands in for a correct kernel; four
mutations of its output stand in for the kernel bugs the old max-over-the-matrix check() cannot see."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R  # noqa: E402

bf = torch.bfloat16
SHAPES = [(130, 260, 192), (257, 128, 448), (64, 512, 1024)]


def old_check_err(got, ref):
    """gpu_util.check()'s statistic (restated: gpu_util imports the GPU package)"""
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


@pytest.mark.parametrize("epi", sorted(R.EXACT_EPIS))
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_emulation_reproduces_exact_case_bit_for_bit(M, N, K, epi):
    if "rowsq" in epi and N % 64:
        N = 256
    c = R.exact_case(M, N, K, epi, seed=3)
    out, sq = R.emulate(c)
    assert R.exact_mismatch(out, c.expect, epi) is None, R.exact_mismatch(out, c.expect, epi)
    if c.expect_rowsq is not None:
        assert R.exact_mismatch(sq, c.expect_rowsq, epi + " rowsq") is None
    # and the gathered expectation is the matmul: float64 on the dense operands
    dense = c.A.double() @ c.W.double().T
    ev = c
    if ev.rowscale is not None:
        dense = dense * ev.rowscale.double()[:, None]
    if ev.bias is not None:
        dense = dense + ev.bias.double()
    if ev.gamma is not None:
        dense = dense * ev.gamma.double()
    if ev.resid is not None:
        dense = dense + ev.resid.double()
    assert torch.equal(dense, c.expect.double())


@pytest.mark.parametrize("K", [192, 448, 1408, 4096])
def test_exact_operands_cover_every_chunk_and_the_last_k(K):
    """every 128-row block (a wave tile's rows) has an entry in every 8-element chunk of every k-tile, every row has one at the last k, all 8 elements of a chunk occur,
    partial sums stay integers <= 48, W is not symmetric"""
    rows = torch.arange(1024, dtype=torch.int64)
    idx, sign = R.exact_A_entries(rows, K, seed=5)
    assert bool((idx[:, 0] == K - 1).all()) and set(sign.unique().tolist()) == {-1, 1}
    if K // 8 <= 128 * 7:
        for b in range(0, 1024, 128):
            assert (idx[b:b + 128, 1:] // 8).unique().numel() == K // 8, f"rows {b}..{b + 127} miss a chunk"
    else:
        assert (idx[:, 1:] // 8).unique().numel() == K // 8
    assert (idx[:, 1:] % 8).unique().numel() == 8
    W = R.exact_W_int(torch.arange(256), torch.arange(K), 5)
    assert int(W.min()) == -6 and int(W.max()) == 6 and not torch.equal(W[:, :256], W[:, :256].T)
    A = R.exact_A(rows, K, 5).double()
    assert float((A.abs() @ W.double().abs().T).max()) <= 48


@pytest.mark.parametrize("epi", sorted(R.BOUNDED_EPIS))
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_emulation_stays_inside_the_elementwise_bound(M, N, K, epi):
    if "rowsq" in epi and N % 64:
        N = 256
    c = R.bounded_case(M, N, K, epi, seed=11)
    out, sq = R.emulate(c)
    ref, bound, sq_ref, sq_bound = R.elementwise_bound(c)
    msg, worst = R.bound_violations(out, ref, bound, f"{epi} {M}x{N}x{K}")
    print(f"[gemm-ref] emulation {epi} {M}x{N}x{K}: worst err / bound {worst:.3f}")
    assert msg is None, msg
    if sq_ref is not None:
        msg, _ = R.bound_violations(sq, sq_ref, sq_bound, f"{epi} rowsq")
        assert msg is None, msg
    # the bound is a bf16-level statement per element, not a matrix-level one: nowhere wider than 4 bf16 ulps of the reference plus the accumulation term's share
    assert float(bound.min()) > 0


def _small_row_case():
    c = R.bounded_case(300, 512, 256, "plain", seed=2)
    out, _ = R.emulate(c)
    ref, bound, _, _ = R.elementwise_bound(c)
    return c, out, ref, bound


def test_one_ulp_in_a_small_row_passes_the_old_check_and_fails_the_new_one():
    """the reason this file exists"""
    c, out, ref, bound = _small_row_case()
    scale = c.A.float().abs().amax(1)
    r = int(scale.argmin())                                   # a row ~2^-6 of the typical scale, 2^-12 of the largest
    assert float(scale[r]) < float(scale.max()) * 2.0 ** -10
    col = 301
    bits = out.view(torch.int16).clone()
    bits[r, col] += 3                                         # three bf16 ulps: outside any rounding ambiguity, still 2^-12 of the matrix scale
    mut = bits.view(bf)
    assert old_check_err(mut, c.A.float() @ c.W.float().T) <= 6e-3, "the old check() must be blind to this"
    msg, _ = R.bound_violations(mut, ref, bound, "mutated")
    assert msg is not None and f"({r}, {col})" in msg and "1 of" in msg, msg
    # and on exact data a single ulp is caught, with its place
    e = R.exact_case(300, 512, 256, "bias", seed=2)
    eo, _ = R.emulate(e)
    eb = eo.view(torch.int16).clone()
    eb[299, 511] += 1
    msg = R.exact_mismatch(eb.view(bf), e.expect, "mutated")
    assert msg is not None and "1 of" in msg and "(299, 511)" in msg and "tile (row 1, column 1)" in msg, msg
    assert old_check_err(eb.view(bf), e.expect) <= 6e-3


def test_swapped_columns_inside_one_tile_are_rejected():
    for case in (R.exact_case(300, 512, 256, "plain", seed=4), ):
        out, _ = R.emulate(case)
        mut = out.clone()
        mut[:, [260, 263]] = mut[:, [263, 260]]
        msg = R.exact_mismatch(mut, case.expect, "swapped")
        assert msg is not None and "(0, 260)" in msg or "260)" in msg, msg
        assert "column 1)" in msg
    c, out, ref, bound = _small_row_case()
    mut = out.clone()
    mut[:, [260, 263]] = mut[:, [263, 260]]
    msg, _ = R.bound_violations(mut, ref, bound, "swapped")
    assert msg is not None and "260)" in msg and "263)" in msg, msg


def test_a_dropped_last_k_tile_is_rejected():
    e = R.exact_case(300, 512, 256, "plain", seed=6)
    short = (e.A[:, :192].float() @ e.W[:, :192].float().T).to(bf)
    msg = R.exact_mismatch(short, e.expect, "k-tile dropped")
    assert msg is not None and "first (0, " in msg, msg
    wrong_rows = (short != e.expect).any(1)
    assert bool(wrong_rows.all()), "every row carries an entry at the last k"
    c, out, ref, bound = _small_row_case()
    short = (c.A[:, :192].float() @ c.W[:, :192].float().T).to(bf)
    msg, _ = R.bound_violations(short, ref, bound, "k-tile dropped")
    assert msg is not None and "first (" in msg, msg


def test_a_row_beyond_M_written_is_rejected():
    """the tests hand the kernel a C of exactly M rows inside a larger allocation whose tail must stay as it was: here, a result with one more row than expected"""
    e = R.exact_case(300, 512, 256, "plain", seed=8)
    out, _ = R.emulate(e)
    guard = torch.zeros((8, 512), dtype=bf)
    buf = torch.cat([out, guard])
    buf[300, 17] = 1.0
    msg = R.exact_mismatch(buf[300:], guard, "rows beyond M", row0=300)
    assert msg is not None and "(300, 17)" in msg and "1 of" in msg, msg
    assert R.exact_mismatch(torch.cat([out, guard])[300:], guard, "rows beyond M", row0=300) is None
    assert "shape" in R.exact_mismatch(buf, e.expect, "too many rows")
