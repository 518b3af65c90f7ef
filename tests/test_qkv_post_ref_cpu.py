"""CPU tests of tests/qkv_post_ref.py: the reference of test_gpu_qkv_post.py can fail, and a correct implementation stays inside it.
qkv_post_ref.emulate -- the contract of gvl_qkv_post (include/gvl.h) in plain numpy -- stands in for a correct kernel over THE list the GPU test runs, and with mut=... for
seventeen wrong ones: every one of them must be reported by the same qkv_post_ref.mismatch the GPU test asserts with, on at least one case of that list.
Three more wrong kernels form a page's offset in 32 bits: they are the identity on that list and must be reported on every relocated case (qkv_post_ref.relocated_cases),
evaluated over sparse pools."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qkv_post_ref as R  # noqa: E402

SPECS = R.cases()


def test_round_to_nearest_even_on_bit_patterns_agrees_with_torch_and_with_the_float64_form():
    rng = np.random.RandomState(3)
    x = (rng.standard_normal(200000) * np.exp2(rng.randint(-40, 40, 200000))).astype(np.float32)
    base = R.f32_of_bits(rng.randint(0x0080, 0x7F00, 4096).astype(np.uint16))
    half = R.f32_of_bits(np.full(4096, 0x3B80, dtype=np.uint16))                       # 2^-8: with base (1 + 2^-8) is exactly between two bf16 numbers -- the ties
    x = np.concatenate([x, base, -base, base + base * half, -(base + base * half), base + base * half * np.float32(1.0000001)])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = R.round_bf16_bits(x)
    assert np.array_equal(got, want)
    assert np.array_equal(R.round_bf16_f64(x.astype(np.float64)), R.f32_of_bits(got).astype(np.float64))
    assert np.array_equal(R.f32_of_bits(want), torch.from_numpy(want.view(np.int16)).view(torch.bfloat16).float().numpy())
    assert R.ulp_bf16(np.array([1.0, 1.99, 2.0, 0.75]))[:].tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8]


def test_the_data_is_what_the_file_says():
    for narrow, lo, hi in ((False, -30, 30), (True, -4, 4)):
        b = R.data_bits(300, 448, 5, narrow)
        ex = (b >> 7) & 255
        nz = (b & 0x7FFF) != 0
        assert (narrow and nz.all()) or (not narrow and 0 < (~nz).sum() < b.size // 20)
        assert ex[nz].min() == 127 + lo and ex[nz].max() == 127 + hi, "normal values only, over the whole stated range"
        assert 0.4 < (b >> 15).mean() < 0.6
        chunks = np.ascontiguousarray(b).view(np.dtype((np.void, 16))).reshape(-1)          # 16-byte chunks: a misplaced one cannot equal the right one
        assert np.unique(chunks).size == chunks.size
    cos, sin = R.trig_tables(200, 64, 5)
    for t in (cos, sin):
        assert t.dtype == np.float32 and np.array_equal(R.f32_of_bits(R.round_bf16_bits(t)), t), "bf16-representable fp32 values"
        assert 0.25 <= np.abs(t).min() and np.abs(t).max() < 2 and np.unique(t.view(np.uint32)).size > 500
    assert not np.array_equal(cos, sin) and not np.array_equal(cos[1], cos[0]) and not np.array_equal(cos[:, 1], cos[:, 0])


def test_the_list_holds_every_geometry_length_and_form_the_kernels_branch_on():
    sp = SPECS
    single = [s for s in sp if s["form"] == "single"]
    for geo in R.GEOS:
        for mode in (0, 1, 2):
            mine = [s for s in single if s["geo"] == geo and s["mode"] == mode]
            assert {s["S"] for s in mine if not s["table"]} == set(R.LENS) == {s["S"] for s in mine if s["table"]}
            assert {s["B"] for s in mine if not s["table"]} == {1, 3} and {s["pos0"] for s in mine if s["table"] and s["vt"]} == {0, 64, 192}
            assert any(not s["vt"] for s in mine)
    assert any(s["pos0"] & 63 for s in single if not s["vt"]) and not any(s["pos0"] & 63 for s in single if s["vt"])
    iv2 = [s for s in single if s["geo"] == R.GEO_IV2]
    assert {(s["mode"], s["q_rs"]) for s in iv2} == {(0, False), (1, False), (1, True)} and all(s["k_ones"] for s in iv2 if s["q_rs"])
    H, KV, Dr, _ = R.GEO_IV2
    assert H * Dr // 8 <= 192 and R.GEO_WIDE[0] * R.GEO_WIDE[2] // 8 > 192, "in_regs serves 192 chunks per lane set: one geometry on each side"
    assert {s["mode"] for s in single if s["geo"] == R.GEO_WIDE} == {1} and {s["S"] for s in single if s["geo"] == R.GEO_WIDE} == set(R.LENS)
    padded = [s for s in sp if s["geo"][3] > s["geo"][2]]
    assert {(s["k_ones"], s["ones_row"]) for s in padded} == {(0, 0), (0, 1), (1, 0), (1, 1)} and not any(s["k_ones"] or s["ones_row"] for s in sp if s["geo"][3] == s["geo"][2])
    # ragged: 1, 2 and 8 members; a 4-row block with three members, one with two, a member that ends exactly on a block boundary
    assert {len(g) for g in R.GROUPS} == {1, 2, 8} and {x for g in R.GROUPS for x in g} == {1, 2, 3, 64, 65, 130}
    spans, ends = set(), False
    for g in R.GROUPS:
        owner = np.repeat(np.arange(len(g)), g)
        for r in range(0, owner.size, 4):
            spans.add(np.unique(owner[r:r + 4]).size)
        ends |= any(e % 4 == 0 for e in np.cumsum(g)[:-1])
    assert {2, 3} <= spans and ends
    for geo in R.GEOS:
        assert {tuple(s["lens"]) for s in sp if s["form"] == "ragged" and s["geo"] == geo} == set(R.GROUPS)
        ext = [s for s in sp if s["form"] == "ext" and s["geo"] == geo]
        assert {tuple(s["lens"]) for s in ext} == set(R.GROUPS)
        assert any(set(s["vl_pos0"][:len(s["lens"])]) == {0} for s in ext) and any(set(s["vl_pos0"][:len(s["lens"])]) == {0, 64, 128} for s in ext)
    for s in sp[::7]:                                  # tables: permuted, longer than the tiles of the sequence, pages nobody names
        c = R.build(s)
        named = {m.table[t] for m in c.members for t in range(m.pos0 >> 6, (m.pos0 + m.rows + 63) >> 6)}
        assert named <= set(range(c.n_pages)) and len(named) <= c.n_pages - 3
        if s["form"] != "single" or s["table"]:
            assert all(len(m.table) > (m.pos0 + m.rows + 63) >> 6 for m in c.members)


def test_the_exact_rope_emulation_is_anchored_to_a_float64_formula_without_rounding_steps():
    """two roundings of the products, one fp32 addition (exact or rounded at 2^-24, far below), one rounding of the sum: within one bf16 ulp of the result plus one of
    each product -- and the typical error is far smaller, so the anchor would see a wrong formula"""
    n = 0
    for s in (s for s in SPECS if s["mode"] == 2 and s["form"] == "single" and s["S"] in (5, 130)):
        c = R.build(s)
        m = c.members[0]
        x = c.qkv[:m.rows, :c.H * c.Dr].reshape(m.rows, c.H, c.Dr)
        pos = m.pos0 + np.arange(m.rows)
        got = R.f32_of_bits(R.rope(x, pos, c.cos, c.sin)).astype(np.float64)
        y, a, b = R.rope_f64(x, pos, c.cos, c.sin)
        err = np.abs(got - y)
        assert (err <= R.ulp_bf16(y) + R.ulp_bf16(a) + R.ulp_bf16(b)).all(), str(c)
        nz = a + b > 0
        assert np.median(err[nz] / (a + b)[nz]) < 2.0 ** -8
        for mut in ("rope_sign", "partner_same_half", "cos_stride_Dr", "pos_plus_1"):
            bad = R.f32_of_bits(R.rope(x, pos, c.cos, c.sin, mut)).astype(np.float64)
            assert (np.abs(bad - y) > R.ulp_bf16(y) + R.ulp_bf16(a) + R.ulp_bf16(b)).mean() > 0.5 or (mut == "cos_stride_Dr" and m.pos0 + m.rows == 1), (str(c), mut)
        n += 1
    assert n >= 10


def test_a_correct_implementation_passes_every_case_of_the_list():
    """modes 0 / 2: emulate IS the expectation; mode 1: the fp32 emulation must lie inside the float64 bound, the bound must be tight (of the order of one bf16 rounding)"""
    stats = {}
    for s in SPECS:
        c = R.build(s)
        e = R.expect(c)
        msg = R.mismatch(c, R.emulate(c), e, stats)
        assert msg is None, msg
        if c.mode == 1:
            _, ref, bound = e.bounded["Kt"]
            assert (bound <= 2.0 ** -7 * np.abs(ref) * (1.5 + 2.0 ** -8)).all() and (bound > 0).all()   # half an ulp (<= 2^-8 relative); with a flip (<= 2^-7) one and a half of the larger value
            # a flip needs a rounding boundary within ~n 2^-24 relative of x rs, against a spacing of 2^-8 ... 2^-7: n 2^-15, a few per cent at the widest row
            assert ref.size < 512 or (bound > 2.0 ** -8 * np.abs(ref)).mean() < 4 * (c.H * c.Dr) * 2.0 ** -15, "a flip of the inner rounding is possible for a small minority only"
            if c.q_rs:
                assert (e.bounded["q_rs"][2] < (c.H * c.Dr + 8) * R.U32 * e.bounded["q_rs"][1]).all()      # n roundings of the sum and a handful more
    assert 0 < stats["Kt"] <= 1.0 and 0 < stats["Q"] <= 1.0 and 0 < stats["q_rs"] <= 1.0


def _applies(mut, s):
    if mut in ("rope_sign", "partner_same_half", "cos_stride_Dr", "pos_plus_1", "one_rounding"):
        return s["mode"] == 2
    if mut == "rms_per_head":
        return s["mode"] == 1
    if mut == "q_rs_writes_Q":
        return s["q_rs"]
    if mut in ("member_off_by_one", "q_row0_dropped"):
        return s["form"] != "single" and len(s["lens"]) > 1
    if mut == "neighbour_table":
        return (s["form"] != "single" and len(s["lens"]) > 1) or (s["form"] == "single" and s["B"] > 1)
    if mut == "v_ext_tile_at_64t":
        return s["form"] == "ext"
    if mut == "pad_not_zeroed":
        return s["geo"][3] > s["geo"][2]
    if mut in ("k_ones_missing", "k_ones_col_plus_1"):
        return bool(s["k_ones"])
    if mut == "ones_row_missing":
        return bool(s["ones_row"] and s["vt"])
    return True


@pytest.mark.parametrize("mut", [m for m in R.MUTATIONS if m not in R.PAGE_MUTATIONS])       # the page mutations: test_page_offsets_formed_in_32_bits_...
def test_every_mutation_is_caught_by_the_comparison_of_the_gpu_test(mut):
    caught, tried, first = 0, 0, None
    for s in SPECS:
        if not _applies(mut, s) or tried >= 40:
            continue
        c = R.build(s)
        tried += 1
        msg = R.mismatch(c, R.emulate(c, mut), R.expect(c))
        if msg is not None:
            caught += 1
            first = first or msg
    assert caught >= 1, f"{mut}: not one of {tried} cases of the list reports it"
    assert "member" in first and "source row" in first or "no table" in first or "guard" in first, first
    print(f"[mutation] {mut}: caught in {caught} of {tried} cases; e.g. {first[:300]}")


def test_mutations_are_caught_where_they_must_be():
    """the cases that exist FOR a defect report it: pos0 > 0 for the slot, a padded head dim for the pad, S % 64 != 0 for the V^T tail, an extend member behind a prefix"""
    def reported(s, mut):
        c = R.build(s)
        return R.mismatch(c, R.emulate(c, mut), R.expect(c)) is not None

    for s in SPECS:
        single = s["form"] == "single"
        pad = s["geo"][3] > s["geo"][2]
        if single and s["table"]:
            assert reported(s, "slot_ignores_pos0") == (s["pos0"] > 0), s
        if s["vt"] and (single or len(s["lens"]) == 1):
            S = s["S"] if single else s["lens"][0]
            assert reported(s, "v_tail_not_zeroed") == (S % 64 != 0), s
        if s["form"] == "ext":
            assert reported(s, "v_ext_tile_at_64t") == any(p > 0 for p in s["vl_pos0"][:len(s["lens"])]), s
        if s["seed"] % 3 == 0:
            assert reported(s, "pad_not_zeroed") == pad, s
            assert reported(s, "k_ones_missing") == bool(s["k_ones"]) == reported(s, "k_ones_col_plus_1"), s
            assert reported(s, "ones_row_missing") == bool(s["ones_row"] and s["vt"]), s
            if s["form"] != "single" and len(s["lens"]) > 1:
                assert reported(s, "member_off_by_one") and reported(s, "q_row0_dropped") and reported(s, "neighbour_table"), s
            if s["mode"] == 2:
                assert reported(s, "rope_sign") and reported(s, "partner_same_half") and reported(s, "one_rounding"), s


def test_a_group_member_is_its_own_single_sequence_launch_in_the_reference_too():
    for s in (s for s in SPECS if s["form"] != "single" and s["seed"] % 2 == 0):
        c = R.build(s)
        whole = R.emulate(c)
        for u, m in enumerate(c.members):
            d = R.single_launch_of(c, u)
            one = R.emulate(d)
            assert np.array_equal(one.Q[:d.q_elems], whole.Q[m.row0 * c.H * c.D:(m.row0 + m.rows) * c.H * c.D])
            pages = [m.table[t] for t in range(m.pos0 >> 6, (m.pos0 + m.rows + 63) >> 6)]
            assert np.array_equal(one.Kt[pages], whole.Kt[pages]) and np.array_equal(one.Vt[pages], whole.Vt[pages])
            rest = np.setdiff1d(np.arange(c.n_pages), pages)
            assert (one.Kt[rest] == R.SENT).all() and (one.Vt[rest] == R.SENT).all()


def test_the_report_names_buffer_place_member_and_source_row():
    s = next(s for s in SPECS if s["form"] == "ext" and len(s["lens"]) == 8 and any(s["vl_pos0"]))
    c = R.build(s)
    e = R.expect(c)
    got = R.emulate(c)
    m = c.members[4]
    pos = m.pos0 + 10
    got.Kt[m.table[pos >> 6], c.KV - 1, pos & 63, 3] ^= 1
    msg = R.mismatch(c, got, e)
    assert f"Kt: 1 of" in msg and f"page {m.table[pos >> 6]} = tile {pos >> 6} of member 4, KV head {c.KV - 1}, slot {pos & 63}, d 3" in msg and f"source row {m.row0 + 10}" in msg, msg
    got = R.emulate(c)
    free = next(p for p in range(c.n_pages) if all(p not in mm.table for mm in c.members))
    got.Vt[free, 0, 1, 2] = 0
    got.Q[c.q_elems + 5] = 0
    msg = R.mismatch(c, got, e)
    assert "a page no table of this launch names" in msg and "guard element 5" in msg and "nobody may write here" in msg, msg


# ---- the relocated cases ------------------------------------------------------------------------------------------------------------------------------------------------
RELOCATED = R.relocated_cases()


def _named(c):
    return sorted({m.table[t] for m in c.members for t in range(m.pos0 >> 6, (m.pos0 + m.rows + 63) >> 6)})


def test_the_relocated_cases_are_cases_of_the_list_on_pages_above_2_to_the_31():
    assert all(s in SPECS for s, _ in RELOCATED) and [k for _, k in RELOCATED].count(30) == 1 and {k for _, k in RELOCATED} == {30, 31}
    hi = [s for s, k in RELOCATED if k == 31]
    assert {s["form"] for s in hi} == {"single", "ragged", "ext"} and all(s["table"] for s in hi if s["form"] == "single")
    assert {s["mode"] for s in hi} == {0, 1, 2} and any(s["q_rs"] for s in hi) and any(not s["vt"] for s in hi)
    assert {s["geo"][2:] for s in hi} >= {(64, 64), (128, 128), (80, 96), (88, 96)}
    assert any(any(s["vl_pos0"][:len(s["lens"])]) for s in hi if s["form"] == "ext") and any(s["pos0"] > 0 for s in hi if s["form"] == "single")
    for s, k in RELOCATED:
        c, small = R.build_relocated(s, k), R.build(s)
        pe = c.KV * 64 * c.D
        assert c.page_elems == pe and c.n_pages * pe <= R.POOL_ELEMS < (c.n_pages + 1) * pe and c.page0 + c.win <= c.n_pages
        assert min(_named(c)) * pe >= 1 << k and (c.page0 - 1) * pe < 1 << k, "the first page at or above 2^k elements"
        assert k == 31 or (1 << 31) <= min(_named(c)) * pe * 2 and max(_named(c)) * pe * 2 < 1 << 32, "k = 30: byte offsets between 2^31 and 2^32"
        assert [x - c.page0 for x in _named(c)] == _named(small) and c.win == small.win, "the same permutation, moved"
        for m, ms in zip(c.members, small.members):        # what is no page in the small case is no page here either
            assert all((a - c.page0 == b) if 0 <= b < small.n_pages else not 0 <= a < c.n_pages for a, b in zip(m.table, ms.table))
        e, es = R.expect(c), R.expect(small)                 # the expectation does not depend on first_page
        for name in ("Q", "Kt", "Vt", "q_rs"):
            assert np.array_equal(getattr(e.bits, name), getattr(es.bits, name))
            assert (name in e.bounded) == (name in es.bounded) and all(np.array_equal(a, b) for a, b in zip(e.bounded.get(name, ()), es.bounded.get(name, ())))


@pytest.mark.parametrize("n", range(len(RELOCATED)))
def test_page_offsets_formed_in_32_bits_are_caught_on_every_relocated_case(n):
    """the unmutated emulation passes; a page offset taken mod 2^31 elements or mod 2^32 bytes is reported on every case above 2^31 elements.  On the case above 2^30 those
    two ARE the identity (every offset is below 2^31 elements = 2^32 bytes: no unsigned 32-bit form is wrong there) -- what that placement catches is the SIGNED 32-bit
    byte offset, which every case reports."""
    s, k = RELOCATED[n]
    c = R.build_relocated(s, k)
    e = R.expect(c)
    ok = R.emulate(c)
    assert R.mismatch(c, ok, e) is None and not ok.stray
    for mut in R.PAGE_MUTATIONS:
        got = R.emulate(c, mut)
        msg = R.mismatch(c, got, e)
        if k == 30 and mut != "page_byte_int32":
            assert msg is None and not got.stray and all(np.array_equal(getattr(got, x), getattr(ok, x)) for x in ("Q", "Kt", "Vt", "q_rs"))
            continue
        assert msg is not None and "member" in msg and "source row" in msg and "still the sentinel: not written" in msg and "written outside pages" in msg, (mut, msg)
        assert len(got.stray) == len(_named(c)) * (2 if c.vt else 1) and (got.Kt == R.SENT).all() and (got.Vt == R.SENT).all()
        lo = [off for _, off in got.stray]
        assert all(off + c.page_elems <= c.page0 * c.page_elems for off in lo), "the wrapped writes land in front of the case's pages: in the part of the pool the GPU test keeps all sentinel"
        assert mut == "page_byte_int32" or all(off >= 0 for off in lo)
        assert np.array_equal(got.Q, ok.Q) and np.array_equal(got.q_rs, ok.q_rs)
    small = R.build(s)                                       # on the small pools of the list the three are the identity
    for mut in R.PAGE_MUTATIONS:
        assert R.mismatch(small, R.emulate(small, mut), R.expect(small)) is None
