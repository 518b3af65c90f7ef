"""-m gpu: every form of the bf16 GEMM (tile_cfg 0 = the automatic plan, 1, 21, 22, 82, 84, 86, 87, 88, 85; 88 under gemm_narrow 0 / 1 / 2) against an INDEPENDENT
reference (tests/gemm_ref.py) -- where test_gpu_gemm4.py only compares the forms with each other.
  exact cases    integer operands on which every partial sum and every epilogue intermediate is exactly representable: output and row statistics must equal the
                 integer expectation BIT FOR BIT; the failure names the count of wrong elements, the first and last one and their 256 x 256 tiles.
  bounded cases  dense data with row scales 2^-6 ... 2^6 and outlier columns against a float64 reference: ZERO elements outside the derived per-element bound
                 (gemm_ref.elementwise_bound); the largest err / bound per case is printed.
  large operands A >= 4 GiB and W >= 4 GiB (the 256 x 256 forms address operands with 32-bit DMA offsets: gvl_launch_gemm hands such a launch to cfg 21, an explicit
                 82 / 88 included) -- bit for bit on the first 512, the 512 straddling byte offset 2^32 and the last 512 rows / columns.
The output buffer carries GUARD rows behind row M - 1 (and the statistics buffer too): a kernel that writes a row beyond M changes them.
What the library documents for a configuration that does not serve an epilogue is what the tests require: 84 ... 88 fall back towards 82 (gvl_gemm.hip, gvl_launch_gemm; gvl.h
"gemm_a4") and must still give the right answer; tile_cfg 1 / 85 (per-lane epilogue, A/B only) REJECT the fused-RMSNorm operands (row scale / row statistics) with an error.
Which kernel a (shape, epilogue, tile_cfg) runs is asked from the library's own plan (tests/gemm_plan.py): the forms are bit-identical, and many edge shapes here fall back on
purpose, so test_the_cases_exercise_every_form asserts that for every epilogue each of 84 / 86 / 87 / 88 / 22 that serves it -- and 22 as a remainder of the automatic
plan -- really runs on at least one shape of the list, and the 4 GiB cases assert that no 256 x 256 form runs.
N moves in steps of 4 around 128 / 256: N % 4 == 0 is the library's contract (gvl_launch_gemm returns -1 otherwise), the row statistics need N % 64 == 0."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, bf, tiny_geo  # noqa: E402
from grounded_video_llm_amd import engine as E, lib as L  # noqa: E402
import gemm_ref as R  # noqa: E402
import gemm_plan as G  # noqa: E402
from test_gpu_gemm4 import NARROW_SHAPES, P_SHAPES  # noqa: E402

CFGS = [0, 1, 21, 22, 82, 84, 86, 87, 88, 85]
NO_ROWS = (1, 85)          # per-lane epilogue only: no row scale / row statistics
GUARD = 264                # rows behind the matrix that must stay untouched: more than a 256-row tile's overhang
SENT = -7.0


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(tiny_geo(), DEV, towers=())
    yield e
    e.close()


def run(eng, c, cfg):
    """one launch through gvl_op_gemm / gvl_op_gemm_rows into guarded buffers -> (out [M, n_out], rowsq or None); asserts the guard rows kept their fill"""
    M, N, K = c.M, c.N, c.K
    n_out = N // 2 if c.act == R.ACT_SILU_MUL else N
    buf = torch.full((M + GUARD, n_out), SENT, dtype=torch.float32 if c.out_f32 else bf, device=DEV)
    p = E._ptr
    A, W = c.A.contiguous(), c.W.contiguous()
    sq = None
    if c.rows:
        want_sq = "rowsq" in c.flags
        sq = torch.full((M + GUARD, N // 64), float("nan"), dtype=torch.float32, device=DEV) if want_sq else None
        rc = eng.lib.gvl_op_gemm_rows(eng.ctx, p(A), p(W), p(buf), M, N, K, p(c.bias), p(c.gamma), p(c.resid), c.act, p(c.rowscale), p(sq), N // 64 if want_sq else 0, cfg, eng.stream)
    else:
        rc = eng.lib.gvl_op_gemm(eng.ctx, p(A), p(W), p(buf), M, N, K, p(c.bias), p(c.gamma), p(c.resid), c.act, 1 if c.out_f32 else 0, cfg, eng.stream)
    eng._chk(rc, f"gemm tile_cfg {cfg}")
    torch.cuda.synchronize()
    touched = (buf[M:] != SENT).nonzero()
    assert touched.numel() == 0, f"tile_cfg {cfg} {c.epi} {M}x{N}x{K}: {touched.shape[0]} elements of the rows BEYOND M written, first at row {M + int(touched[0][0])}, column {int(touched[0][1])}"
    if sq is not None:
        assert bool(torch.isnan(sq[M:]).all()), f"tile_cfg {cfg} {c.epi} {M}x{N}x{K}: row statistics written beyond row M"
        sq = sq[:M]
    return buf[:M], sq


def variants(eng):
    """(label, tile_cfg, gemm_narrow or None)"""
    for cfg in CFGS:
        if cfg == 88:
            for nar in (1, 2, 0):
                yield f"88/narrow={nar}", 88, nar
        else:
            yield str(cfg), cfg, None


def for_every_form(eng, c, judge):
    try:
        for label, cfg, nar in variants(eng):
            if nar is not None:
                eng.debug_set("gemm_narrow", nar)
            if c.rows and (cfg in NO_ROWS or c.N % 16):            # documented: an error, nothing launched (the row operands exist in the staged whole-row epilogue only:
                with pytest.raises(L.GvlError):                    # 16-byte output rows, not tile_cfg 1 / 85)
                    run(eng, c, cfg)
                continue
            out, sq = run(eng, c, cfg)
            judge(label, out, sq)
    finally:
        eng.debug_set("gemm_narrow", 1)


# k-tile counts: 2 (below the 4-wave forms' minimum of 3: they fall back), 3, 4, 5; around the pipelined statements' minima (7 / 9 / 12 / 15 / 16 k-tiles per epilogue:
# GVL_A4P_MIN_NK_E*), odd and even; M and N one step below, at and above 128 and 256; N <= 128; M = 1; more tiles than compute units
EDGE_SHAPES = [(300, 256, 128), (256, 256, 192), (300, 512, 256), (513, 384, 320), (520, 512, 384), (700, 512, 448), (700, 512, 512), (600, 1408, 704), (600, 512, 768),
               (600, 512, 832), (515, 1408, 960), (515, 1408, 1024), (515, 704, 1088),
               (127, 124, 448), (128, 128, 448), (129, 132, 448), (255, 252, 1024), (256, 256, 1024), (257, 260, 1024), (1, 1408, 1408), (1, 64, 192), (5000, 64, 1088),
               (20000, 4096, 256)]
REAL_SHAPES = [(24588, 1408, 1408), (24588, 6144, 1408), (3519, 16384, 3072), (27696, 1024, 4096)]
EXACT_SHAPES = EDGE_SHAPES + [s for s in P_SHAPES + NARROW_SHAPES + REAL_SHAPES if s not in EDGE_SHAPES]
EXACT_SHAPES = sorted(set(EXACT_SHAPES), key=EXACT_SHAPES.index)


@pytest.mark.parametrize("M,N,K", EXACT_SHAPES)
def test_exact_cases_bit_for_bit(eng, M, N, K):
    ran = 0
    for epi in R.EXACT_EPIS:
        if "rowsq" in epi and N % 64:
            continue                                      # the library's contract for the statistics: N % 64 == 0
        c = R.exact_case(M, N, K, epi, seed=M + N + K, device=DEV)

        def judge(label, out, sq, c=c, epi=epi):
            msg = R.exact_mismatch(out, c.expect, f"tile_cfg {label} {epi} {M}x{N}x{K}")
            assert msg is None, msg
            if c.expect_rowsq is not None:
                msg = R.exact_mismatch(sq, c.expect_rowsq, f"tile_cfg {label} {epi} {M}x{N}x{K} row statistics (column = 64-column block)")
                assert msg is None, msg

        for_every_form(eng, c, judge)
        ran += 1
    assert ran >= 7


BOUNDED_SHAPES = [(300, 512, 1024), (1000, 1408, 1408), (513, 768, 1088), (2049, 256, 448), (3000, 1024, 192)]


def epi_code(flags):
    act = R.ACT_QUICK_GELU if "qgelu" in flags else R.ACT_GELU if "gelu" in flags else R.ACT_SILU_MUL if "silu" in flags else R.ACT_NONE
    return act | sum(bit for name, bit in (("f32", G.F32), ("resid", G.RESID), ("gamma", G.GAMMA), ("bias", G.BIAS), ("rowscale", G.ROWSCALE), ("rowsq", G.ROWSQ)) if name in flags)


@pytest.mark.parametrize("epis,shapes,planner", [(R.EXACT_EPIS, EXACT_SHAPES, True), (R.BOUNDED_EPIS, BOUNDED_SHAPES, False)], ids=["exact", "bounded"])
def test_the_cases_exercise_every_form(epis, shapes, planner):
    for name, flags in epis.items():
        e = epi_code(flags)
        ok = [s for s in shapes if not (e & G.ROWSQ and s[1] % 64) and not (e & (G.ROWSCALE | G.ROWSQ) and s[1] % 16)]
        for cfg, form in G.FORM_OF_CFG.items():
            serves = form == G.T64x128 or (e in G.A4P_MIN_NK if form == G.A4P else e in G.A4_EPIS)
            hit = [s for s in ok if form in G.forms(*s, e, cfg)]
            assert bool(hit) == serves, f"{name}: tile_cfg {cfg} (form {form}) {'runs on no shape of the list' if serves else f'unexpectedly runs on {hit}'}"
        if planner:
            assert any(len(f) > 1 and G.T64x128 in f for f in (G.forms(*s, e, 0) for s in ok)), f"{name}: no shape on which the automatic plan splits off a 64 x 128 remainder"


@pytest.mark.parametrize("M,N,K", BOUNDED_SHAPES)
def test_bounded_cases_inside_the_elementwise_bound(eng, M, N, K):
    for epi in R.BOUNDED_EPIS:
        c = R.bounded_case(M, N, K, epi, seed=M * 3 + N + K, device=DEV)
        ref, bound, sq_ref, sq_bound = R.elementwise_bound(c)
        worst = {}

        def judge(label, out, sq):
            msg, w = R.bound_violations(out, ref, bound, f"tile_cfg {label} {epi} {M}x{N}x{K}")
            worst[label] = w
            assert msg is None, msg
            if sq_ref is not None:
                msg, wq = R.bound_violations(sq, sq_ref, sq_bound, f"tile_cfg {label} {epi} {M}x{N}x{K} row statistics")
                worst[label] = max(w, wq)
                assert msg is None, msg

        try:
            for_every_form(eng, c, judge)
        finally:
            print(f"[gemm-bound] {epi:24s} {M}x{N}x{K}: largest err / bound {max(worst.values(), default=float('nan')):.3f} over {len(worst)} forms "
                  f"({', '.join(f'{k}: {v:.3f}' for k, v in worst.items())})")


# ---- operands of 4 GiB and more ------------------------------------------------------------------------------------------------------------------------------------
BIG = (1 << 19) + 1024      # rows of 4096 bf16 = 8 KiB: row 2^19 starts at byte offset 2^32
BIG_K = 4096


def bands(n):
    edge = (1 << 32) // (BIG_K * 2)
    return [(0, 512), (edge - 256, edge + 256), (n - 512, n)]


def test_A_of_more_than_4_GiB(eng):
    """M K 2 = 2^32 + 8 MiB, N = 256.  Rows are generated and checked in pieces: no large matmul, no second copy of A"""
    M, N, K, seed = BIG, 256, BIG_K, 41
    c = R.Case(M, N, K, "plain", R.EXACT_EPIS["plain"])
    try:
        c.A = torch.empty((M, K), dtype=bf, device=DEV)
        assert c.A.numel() * 2 >= 1 << 32
        for r in range(0, M, 32768):
            rows = torch.arange(r, min(M, r + 32768), device=DEV, dtype=torch.int64)
            c.A[r:r + 32768] = R.exact_A(rows, K, seed)
        cols = torch.arange(N, device=DEV, dtype=torch.int64)
        c.W = R.exact_W_int(cols, torch.arange(K, device=DEV, dtype=torch.int64), seed).to(bf)
        for cfg in (0, 82, 88):
            assert not set(G.forms(M, N, K, 0, cfg)) & set(G.BIG_FORMS)
            out, _ = run(eng, c, cfg)
            for lo, hi in bands(M):
                want = R.exact_expected(torch.arange(lo, hi, device=DEV, dtype=torch.int64), cols, K, seed, c.flags).to(bf)
                msg = R.exact_mismatch(out[lo:hi], want, f"tile_cfg {cfg} A >= 4 GiB, rows {lo}..{hi - 1}", row0=lo)
                assert msg is None, msg
            del out
    finally:
        c.A = c.W = None
        torch.cuda.empty_cache()


def test_W_of_more_than_4_GiB(eng):
    """N K 2 = 2^32 + 8 MiB, M = 256, with a bias (its offsets run to 4 N bytes)"""
    M, N, K, seed = 256, BIG, BIG_K, 43
    c = R.Case(M, N, K, "bias", R.EXACT_EPIS["bias"])
    try:
        c.W = torch.empty((N, K), dtype=bf, device=DEV)
        assert c.W.numel() * 2 >= 1 << 32
        ks = torch.arange(K, device=DEV, dtype=torch.int64)
        for r in range(0, N, 16384):
            c.W[r:r + 16384] = R.exact_W_int(torch.arange(r, min(N, r + 16384), device=DEV, dtype=torch.int64), ks, seed).to(bf)
        rows = torch.arange(M, device=DEV, dtype=torch.int64)
        c.A = R.exact_A(rows, K, seed)
        c.bias = R.exact_vectors(rows, torch.arange(N, device=DEV, dtype=torch.int64), seed, c.flags)["bias"]
        for cfg in (0, 82, 88):
            assert not set(G.forms(M, N, K, G.BIAS, cfg)) & set(G.BIG_FORMS)
            out, _ = run(eng, c, cfg)
            for lo, hi in bands(N):
                want = R.exact_expected(rows, torch.arange(lo, hi, device=DEV, dtype=torch.int64), K, seed, c.flags).to(bf)
                msg = R.exact_mismatch(out[:, lo:hi], want, f"tile_cfg {cfg} W >= 4 GiB, columns {lo}..{hi - 1}", col0=lo)
                assert msg is None, msg
            del out
    finally:
        c.A = c.W = c.bias = None
        torch.cuda.empty_cache()
