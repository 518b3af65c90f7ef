"""CPU: gemm_plan (csrc/gvl_gemm_plan.h) -- which kernel form(s) a GEMM launch takes -- against the decisions of the launcher it replaced, and against properties that
hold whatever the table says.  All GEMM forms are bit-identical by design, so no result test can notice a wrong choice of form; this one can.
tests/golden/gemm_launch_plans.json: see its "doc" (how it was recorded) -- every GEMM geometry and epilogue of the bench step and the Llama-3-8B / Phi-3.5 prefill, every
explicit tile_cfg of tests/ and tools/, K / 64 around each minimum of the 4-wave kernels, M and N around 1 / 128 / 256 / 512, the tile-count thresholds of the automatic
choice, operands at 2^32 bytes, rows that are not whole 16-byte pieces under the row-statistics epilogues (refused), every gemm_a4 mode and lab override, and
1 500 seeded random geometries; for 256 and for 304 compute units, so that the arithmetic is not tuned to one number."""
import json
import os

import pytest

import gemm_plan as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "gemm_launch_plans.json")) as f:
        g = json.load(f)
    g["cases"] = [G.case(*c) for c in g["cases"]]
    return g


@pytest.fixture(scope="module", params=[256, 304])
def planned(request, golden):
    return request.param, G.plans(golden["cases"], request.param)


def test_header_builds_as_plain_host_cxx():
    """the header is host-only: the host compiler builds it with -Wall -Wextra -Werror -pedantic, no HIP header in sight"""
    assert os.access(G.dumper(), os.X_OK)


def test_case_list_is_what_the_doc_says(golden):
    assert golden["n_model"] >= 150 and len(golden["cases"]) - golden["n_structured"] >= 1500
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "gemm_launch_plans.json")) < 300 * 1024


def test_every_launch_equals_the_recorded_one(planned, golden):
    n_cu, got = planned
    base = golden["plans"]["256"]
    want = base if n_cu == 256 else [b if w == 0 else w for w, b in zip(golden["plans"]["304"], base)]
    bad = []
    for c, g, w in zip(golden["cases"], got, want):
        flat = -1 if g is None else [x for l in g[0] for x in l]
        if flat != w:
            bad.append((c, flat, w))
    assert not bad, f"{len(bad)} of {len(want)} plans differ at {n_cu} CUs; first (case, got, recorded): {bad[:3]}"


def test_launches_tile_the_output_exactly_once(planned, golden):
    n_cu, got = planned
    for c, g in zip(golden["cases"], got):
        if g is None:
            continue
        M, N = c[0], c[1]
        ls = g[0]
        assert 1 <= len(ls) <= 3
        assert all(0 <= m0 < m1 <= M and 0 <= n0 < n1 <= N for _, _, m0, m1, n0, n1 in ls), (c, ls)
        assert sum((m1 - m0) * (n1 - n0) for _, _, m0, m1, n0, n1 in ls) == M * N, (c, ls)
        for i, a in enumerate(ls):
            for b in ls[i + 1:]:
                assert a[3] <= b[2] or b[3] <= a[2] or a[5] <= b[4] or b[5] <= a[4], f"{c}: launches overlap: {ls}"
        assert all(n0 % 256 == 0 and m0 % 256 == 0 for _, _, m0, _, n0, _ in ls), (c, ls)      # pointer offsets keep the 16-byte alignment and whole 64-column blocks


def test_no_256_form_gets_an_operand_of_4_GiB(planned, golden):
    n_cu, got = planned
    seen = 0
    for c, g in zip(golden["cases"], got):
        if g is None:
            continue
        K, lda, ldw = c[2], c[5], c[6] or c[2]
        for form, _, m0, m1, n0, n1 in g[0]:
            if form in G.BIG_FORMS:
                assert m1 * lda * 2 < 1 << 32 and (n1 - n0) * ldw * 2 < 1 << 32, (c, g[0])
            if form in (G.A4_S0, G.A4_S1, G.A4_S2, G.A4P):      # the buffer descriptors address up to 256 rows past the matrix
                assert (m1 + 256) * lda * 2 < 1 << 32 and (n1 - n0 + 256) * ldw * 2 < 1 << 32, (c, g[0])
            seen += form not in G.BIG_FORMS and (c[0] * lda * 2 >= 1 << 32 or c[1] * ldw * 2 >= 1 << 32)
    assert seen >= 20          # the list does hold such operands


def test_no_4_wave_form_gets_an_epilogue_or_K_it_does_not_serve(planned, golden):
    n_cu, got = planned
    for c, g in zip(golden["cases"], got):
        if g is None:
            continue
        K, epi = c[2], c[3]
        for form, e, *_ in g[0]:
            assert e in (-1, epi) and (e == -1 or e in G.STAGED), (c, g[0])
            if form in (G.A4_S0, G.A4_S1, G.A4_S2):
                assert e in G.A4_EPIS and K // 64 >= 3, (c, g[0])
            if form == G.A4P:
                assert e in G.A4P_MIN_NK and K // 64 >= G.A4P_MIN_NK[e], (c, g[0])
            if epi & (G.ROWSCALE | G.ROWSQ):
                assert e == epi and form not in (G.LOCKSTEP_128, G.PP_LANE), (c, g[0])      # the fused-RMSNorm epilogues exist in the staged form only


def test_a_split_is_never_costed_higher_than_the_whole_launch(planned, golden):
    n_cu, got = planned
    splits = 0
    for c, g in zip(golden["cases"], got):
        if g is None:
            continue
        ls, whole, chosen = g
        if len(ls) > 1:
            splits += 1
            assert chosen < whole, (c, g)
            assert whole == -(-((c[0] + 255) // 256 * ((c[1] + 255) // 256)) // n_cu), (c, g)
        assert chosen <= whole
    assert splits >= 50
