"""CPU: prefill_plan and prefill_group_size (csrc/gvl_prefill_plan.h) -- which launches a prefill group takes, in which order -- against the decisions of the llm_prefill
they were cut out of, and against properties that hold whatever the table says.  Every prefill form is bit-identical per row to the single-sequence path by design, so no
result test can notice a group that fell back to per-sequence launches; this one can.
tests/golden/prefill_launch_plans.json: see its "doc" (how it was recorded).  A seeded enumeration, no full product: one sequence at every length behind every prefix;
uniform groups of 2 .. 8 on both sides of the 256-page-id capacity (8 x 2048 rows = 256 ids, 8 x 2049 = 264); equal lengths behind prefixes; groups that straddle
rope_orig_max_pos = 200 / 4096 by their lengths and by their prefixes; seeded ragged groups of every size with and without prefixes -- each under varlen_attn 1 / 2 / 0 x
varlen_extend 1 / 0 and up to six (rope_orig_max_pos, long table) settings, with seeded last_layer_tail / norm_fused / widths / loss; those four in full on five groups;
nb = 0 and 9, the prefixes 32 and -64 at every place, a loss behind a prefix and a loss for a group."""
import json
import os

import pytest

import prefill_plan as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "prefill_launch_plans.json")
FIELDS = ("group", "rope", "widths", "loss", "varlen_attn", "varlen_extend", "last_layer_tail", "norm_fused")


def case_kw(g, c):
    c = dict(zip(FIELDS, c))
    hidden, qkv_width, gate_up_width, fused_weights = g["widths"][c["widths"]]
    rope_orig_max_pos, long_table = g["rope"][c["rope"]]
    return dict(rope_orig_max_pos=rope_orig_max_pos, long_table=long_table, loss=c["loss"], hidden=hidden, qkv_width=qkv_width, gate_up_width=gate_up_width,
                fused_weights=fused_weights, varlen_attn=c["varlen_attn"], varlen_extend=c["varlen_extend"], last_layer_tail=c["last_layer_tail"], norm_fused=c["norm_fused"])


@pytest.fixture(scope="module")
def golden():
    with open(PATH) as f:
        g = json.load(f)
    g["full"] = [(tuple(g["groups"][c[0]][0]), tuple(g["groups"][c[0]][1]), case_kw(g, c)) for c, _ in g["cases"]]
    return g


@pytest.fixture(scope="module")
def planned(golden):
    return P.plans([P.plan_line(lens, pos0, **kw) for lens, pos0, kw in golden["full"]])


def served(golden, planned):
    for (lens, pos0, kw), p in zip(golden["full"], planned):
        if isinstance(p, P.Plan):
            yield lens, (pos0 or (0,) * len(lens)), kw, p


def ends_long(kw, L, p0):
    return bool(kw["rope_orig_max_pos"] > 0 and kw["long_table"] and p0 + L > kw["rope_orig_max_pos"])


def test_header_builds_as_plain_host_cxx():
    """the header is host-only: the host compiler builds it with -Wall -Wextra -Werror -pedantic, no HIP header in sight"""
    assert os.access(P.dumper(), os.X_OK)
    for h in ("gvl_prefill_plan.h", "gvl_limits.h"):
        with open(os.path.join(P.CSRC, h)) as f:
            text = f.read()
        assert "#include <hip" not in text and "getenv" not in text and "static " not in text.replace("static_assert", ""), h


def test_case_list_is_what_the_doc_says(golden):
    full = golden["full"]
    assert len(full) >= 3000 and len(golden["group_size"]["cases"]) >= 300 and len(golden["group_size"]["cases"]) == len(golden["group_size"]["sizes"])
    assert os.path.getsize(PATH) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "gemm_launch_plans.json"))
    assert {len(lens) for lens, _, _ in full} == set(range(10))
    assert {1, 63, 64, 65, 128, 200, 201, 2049, 3519} <= {L for lens, _, _ in full for L in lens}
    assert {0, 64, 192, 3456, 32, -64} <= {p for _, pos0, _ in full for p in pos0} | {0}
    assert {(kw["rope_orig_max_pos"], kw["long_table"]) for _, _, kw in full} == {(o, t) for o in (0, 200, 4096) for t in (0, 1)}
    for f, vals in (("varlen_attn", (0, 1, 2)), ("varlen_extend", (0, 1)), ("last_layer_tail", (0, 1)), ("norm_fused", (0, 1)), ("loss", (0, 1))):
        assert {kw[f] for _, _, kw in full} == set(vals), f
    assert ((2048,) * 8, ()) in {(lens, pos0) for lens, pos0, _ in full} and ((2049,) * 8, ()) in {(lens, pos0) for lens, pos0, _ in full}
    straddling = [(lens, pos0) for lens, pos0, kw in full if 2 <= len(lens) <= 8 and len({ends_long(kw, L, p) for L, p in zip(lens, pos0 or (0,) * len(lens))}) == 2]
    assert sum(not pos0 for _, pos0 in straddling) >= 50 and sum(bool(pos0) for _, pos0 in straddling) >= 50


def test_every_plan_equals_the_recorded_one(planned, golden):
    bad, count = [], {}
    for (c, want), got in zip(golden["cases"], planned):
        if isinstance(got, P.Plan):
            flat = [got.M, got.batched_table, got.nf, got.tail, got.last_rows, list(got.chunks), [x for s in got.steps for x in s]]
            want = want if isinstance(want, int) else want[:6] + [golden["steps"][want[6]]]
        else:
            flat = got
            count[got] = count.get(got, 0) + 1
        if flat != want:
            bad.append((c, flat, want))
    assert not bad, f"{len(bad)} of {len(planned)} plans differ; first (case, got, recorded): {bad[:3]}"
    assert set(count) == {P.BAD_BATCH, P.BAD_PREFIX, P.LOSS_BEHIND_PREFIX, P.LOSS_GROUP} and min(count.values()) >= 10 and sum(count.values()) < len(planned) - 2500
    assert P.reasons() == {-1: "llm_prefill: batch must be 1 .. 8 sequences", -2: "llm_prefill: a cached prefix is whole pages",
                           -3: "llm_prefill: no loss tail behind a cached prefix", -4: "llm_prefill: loss tail takes one sequence"}


def test_every_group_size_equals_the_recorded_one(golden):
    gs = golden["group_size"]
    got = P.plans([P.group_line(lens, cap, max_rows) for cap, max_rows, lens in gs["cases"]])
    assert got == gs["sizes"]
    for (cap, max_rows, lens), n in zip(gs["cases"], got):                 # table-free: never past cap or max_rows, except at a group of one; and no smaller than need be
        assert 1 <= n <= min(cap, len(lens)) and (n == 1 or sum(lens[:n]) <= max_rows), (cap, max_rows, lens, n)
        assert n == min(cap, len(lens)) or sum(lens[:n + 1]) > max_rows, (cap, max_rows, lens, n)
    assert len({n for n in got}) == 8


def test_every_member_is_covered_by_one_post_and_one_attention_launch(planned, golden):
    seen = set()
    for lens, pos0, kw, p in served(golden, planned):
        nb = len(lens)
        off = [sum(lens[:b]) for b in range(nb + 1)]
        assert p.M == off[nb]
        for kind in (P.POST, P.ATTN):
            steps = [s for s in p.steps if s.kind == kind]
            assert sorted(u for s in steps for u in range(s.first, s.first + s.count)) == list(range(nb)), (lens, pos0, kw, p)
            for s in steps:
                seen.add((kind, s.form))
                if s.form == P.ONE:
                    assert (s.count, s.B, s.S, s.pos0) == (1, 1, lens[s.first], pos0[s.first]) and s.Sk == (s.pos0 + s.S if kind == P.ATTN and s.pos0 else 0), (lens, pos0, s)
                elif s.form == P.BATCHED:
                    assert (s.first, s.count, s.B, s.S, s.pos0, s.Sk) == (0, nb, nb, lens[0], 0, 0) and set(lens) == {lens[0]} and not any(pos0) and p.batched_table, (lens, pos0, s)
                    assert nb * -(-lens[0] // 64) <= P.DEFAULTS["page_id_cap"]
                else:
                    assert (s.first, s.count, s.B, s.S, s.pos0, s.Sk) == (0, nb, 1, max(lens), 0, 0) and any(pos0) == (s.form == P.RAGGED_EXT), (lens, pos0, s)
                # one LongRoPE table per launch: a ragged launch never mixes short-table and long-table members
                if kind == P.POST:
                    assert {ends_long(kw, lens[u], pos0[u]) for u in range(s.first, s.first + s.count)} == {bool(s.use_long)}, (lens, pos0, kw, s)
                else:
                    assert not s.use_long
        assert p.batched_table == any(s.form == P.BATCHED for s in p.steps)
        # the order: post(u), attn(u) per member, or every post in front of the one grid
        kinds = [s.kind for s in p.steps]
        na = P.n_attn(p)
        assert kinds == ([P.POST, P.ATTN] * na if na > 1 else [P.POST] * (len(kinds) - 1) + [P.ATTN]), (lens, pos0, kw, kinds)
        assert [s.first for s in p.steps if s.kind == P.POST] == sorted(s.first for s in p.steps if s.kind == P.POST)
    assert seen == {(k, f) for k in (P.POST, P.ATTN) for f in range(4)}


def test_the_knobs_choose_the_form(planned, golden):
    n = dict.fromkeys(("one", "off", "batched", "ragged", "ragged2", "split", "ext", "ext_split"), 0)
    for lens, pos0, kw, p in served(golden, planned):
        nb, f = len(lens), P.forms(p)
        ext = any(pos0)
        same_table = len({ends_long(kw, L, q) for L, q in zip(lens, pos0)}) == 1
        if nb == 1:
            n["one"] += 1
            assert f == (("ONE",), ("ONE",)), (lens, pos0, kw, f)                       # whatever the knobs are
        elif p.batched_table:
            n["batched"] += 1
            assert f == (("BATCHED",), ("BATCHED",)), (lens, pos0, kw, f)
        elif not (kw["varlen_extend"] if ext else kw["varlen_attn"]):
            n["off"] += 1
            assert f == (("ONE",) * nb,) * 2, (lens, pos0, kw, f)                         # nb launches of form ONE each
        else:
            grid = "RAGGED_EXT" if ext else "RAGGED"
            one_post = same_table and (ext or kw["varlen_attn"] == 1)
            n["ext" if ext and one_post else "ext_split" if ext else "ragged" if one_post else "ragged2" if same_table else "split"] += 1
            assert f == ((grid,) if one_post else ("ONE",) * nb, (grid,)), (lens, pos0, kw, f)
    assert min(n.values()) >= 40, n


def test_all_prefixes_zero_is_the_plan_without_prefixes(golden):
    groups = sorted({(lens, kw["varlen_attn"], kw["varlen_extend"], kw["rope_orig_max_pos"], kw["long_table"]) for lens, _, kw in golden["full"] if 1 <= len(lens) <= 8})
    kws = [dict(varlen_attn=va, varlen_extend=ve, rope_orig_max_pos=o, long_table=t) for _, va, ve, o, t in groups]
    without = P.plans([P.plan_line(g[0], (), **kw) for g, kw in zip(groups, kws)])
    zeros = P.plans([P.plan_line(g[0], (0,) * len(g[0]), **kw) for g, kw in zip(groups, kws)])
    flipped = P.plans([P.plan_line(g[0], (), **dict(kw, varlen_extend=1 - kw["varlen_extend"])) for g, kw in zip(groups, kws)])
    assert len(groups) >= 500 and without == zeros == flipped                            # and varlen_extend means nothing without a prefix


def test_tail_last_rows_and_head_chunks(planned, golden):
    tails = set()
    for lens, pos0, kw, p in served(golden, planned):
        nb = len(lens)
        nf = bool(kw["norm_fused"] and kw["fused_weights"] and kw["hidden"] % 64 == 0 and kw["qkv_width"] % 16 == 0 and kw["gate_up_width"] % 16 == 0)
        assert bool(p.nf) == nf and bool(p.tail) == bool(kw["last_layer_tail"] and not kw["loss"] and (not nf or kw["hidden"] // 64 % 4 == 0)), (lens, kw, p)
        assert p.last_rows == (P.LAST_TAIL if p.tail else P.LAST_STRIDED if nb == 1 or p.batched_table else P.LAST_GATHERED), (lens, pos0, kw, p)
        assert sum(p.chunks) == nb and set(p.chunks) <= {4, 2, 1} and list(p.chunks) == sorted(p.chunks, reverse=True) and len(p.chunks) <= 3, (lens, p.chunks)
        assert not kw["loss"] or nb == 1
        tails.add((nf, bool(p.tail), p.last_rows))
    assert tails == {(nf, tail, last) for nf in (False, True) for tail, last in ((True, P.LAST_TAIL), (False, P.LAST_STRIDED), (False, P.LAST_GATHERED))}, tails
