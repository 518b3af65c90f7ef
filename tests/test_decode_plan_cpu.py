"""CPU: decode_plan, the grouping helpers and the path predicates (csrc/gvl_decode_plan.h) -- which launches one decode step takes and what each projection reads --
against the decisions of the decode_step, the three grouping loops and the three inline predicates they were cut out of, and against properties that hold whatever the
table says.  The batched forms are bit-identical to the single-sequence ones and the fused-RMSNorm form differs from the unfused one in rounding only, so no result test
can notice a model that lost a form; this one can.
tests/golden/decode_launch_plans.json: see its "doc" (how it was recorded).  The whole reachable product: B 0 .. 17 x both paths x weight format 0 / 1 / 2 (MFMA path only:
gvl_finalize_weights refuses a quantised format on the other, recorded through its predicate) x norm_fused 0 / 1 x folded copies present / absent x hidden 64, 256, 512,
1024, 3072, 4096 x 1 .. 3 layers; the grouping of 0 .. 40 sequences on both paths."""
import itertools
import json
import os

import pytest

import decode_plan as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "decode_launch_plans.json")
HIDDENS = (64, 256, 512, 1024, 3072, 4096)
CONSUMERS, PRODUCERS = (D.QKV, D.GATE_UP, D.HEAD), (D.O_PROJ, D.DOWN)


@pytest.fixture(scope="module")
def golden():
    with open(PATH) as f:
        g = json.load(f)
    g["parsed"] = [(ln.split()[0], dict(t.split("=", 1) for t in ln.split()[1:])) for ln in g["lines"]]
    return g


@pytest.fixture(scope="module")
def planned(golden):
    """per recorded case: (B, mfma, fmt, norm_fused, folded, hidden, layers), what was recorded behind it, the plan or refusal of the header"""
    keys = [tuple(c[:7]) for c in golden["cases"]]
    got = D.ask([D.plan_line(B, layers, hidden, mfma, fmt, folded, nf) for B, mfma, fmt, nf, folded, hidden, layers in keys])
    return [(k, c[7:], p) for k, c, p in zip(keys, golden["cases"], got)]


def served(planned):
    return [(k, rec, p) for k, rec, p in planned if isinstance(p, D.Plan)]


def walk(p, key):
    """the launches of the step as decode_step walks the plan: (launcher, what the recorded line must say) in order"""
    B, mfma, fmt, nf, folded, hidden, layers = key

    def proj(kind, l):
        e = p.proj[kind]
        name = "head" if kind == D.HEAD else f"L{l}." + ("qkv" if kind <= D.QKV else D.KIND_NAMES[kind])
        want = {"cat": "2", "W": f"{name}.{D.WEIGHT_NAMES[e.weight]}", "batchB": "1", "ptrs": "1"}
        if e.scales:
            want.update(w_fp8=str(fmt), wscale=f"{name}.scales")
        norm_w = "norm" if kind == D.HEAD else f"L{l}." + ("ln2" if kind == D.GATE_UP else "ln1")
        want.update({D.X_NORM: dict(x="d_x", norm_w=norm_w, eps="1"), D.XN: dict(x="d_xn"), D.XT_SQ: dict(x="d_xt", sq_in="d_sqpart", sq_n=str(hidden // 16), eps="1"),
                     D.ATTN: dict(x="d_attn"), D.ACT: dict(x="d_act")}[e.input])
        if e.sq_out:
            want.update(sq_out="d_sqpart", out_tiled2="d_xt")
        if e.out_tiled:
            want.update(out_tiled="1")
        return D.LAUNCHER_NAMES[e.launcher], want

    norm = lambda w: ("gvl_launch_norm_tiled", dict(cat="4", x="d_x", xn="d_xn", w=w))
    out = [("gvl_launch_embed_norm", dict(cat="4", x="d_x", xn="d_xn", w="L0.ln1")) if p.embed_norm else ("gvl_launch_gather_tok_rows", dict(cat="4", dst="d_x"))]
    for l in range(layers):
        out.append(proj(D.QKV if l else D.QKV0, l))
        out.append(("gvl_launch_decode_attention", dict(cat="3", out="d_attn", **({"out_tiled": "1"} if p.attn_out_tiled else {}))))
        out.append(proj(D.O_PROJ, l))
        out += [norm(f"L{l}.ln2")] if p.norm_launches else []
        out += [proj(D.GATE_UP, l), proj(D.DOWN, l)]
        out += [norm(f"L{l + 1}.ln1" if l + 1 < layers else "norm")] if p.norm_launches else []
    return out + [proj(D.HEAD, 0), ("pick_tokens", dict(cat="4"))]


# the arguments the plan decides: a recorded line must carry exactly those the walk expects, none besides
DECIDED = ("W", "x", "norm_w", "eps", "sq_in", "sq_n", "sq_out", "out_tiled2", "out_tiled", "w_fp8", "wscale")


def test_header_builds_as_plain_host_cxx():
    """the header is host-only: the host compiler builds it with -Wall -Wextra -Werror -pedantic, no HIP header in sight, gvl_limits.h its only include"""
    assert os.access(D.dumper(), os.X_OK)
    for h in ("gvl_decode_plan.h", "gvl_limits.h"):
        with open(os.path.join(D.CSRC, h)) as f:
            text = f.read()
        assert "#include <hip" not in text and "getenv" not in text and "static " not in text.replace("static_assert", ""), h
        assert [ln for ln in text.splitlines() if ln.startswith("#include")] == (['#include "gvl_limits.h"'] if h == "gvl_decode_plan.h" else []), h


def test_case_list_is_the_whole_reachable_product(golden):
    keys = [tuple(c[:7]) for c in golden["cases"]]
    want = {(B, mfma, fmt, nf, folded, hidden, layers) for B in range(18) for mfma in (0, 1) for fmt in ((0, 1, 2) if mfma else (0,)) for nf in (0, 1) for folded in (0, 1)
            for hidden in HIDDENS for layers in (1, 2, 3)}
    assert len(keys) == len(set(keys)) == 5184 and set(keys) == want
    assert all(len(golden["grouping"][m]) == 41 for m in "01")
    assert os.path.getsize(PATH) <= 1.05 * os.path.getsize(os.path.join(ROOT, "tests", "golden", "gemm_launch_plans.json"))


def test_every_step_equals_the_recorded_one(planned, golden):
    bad, refused = [], 0
    for key, rec, p in planned:
        if not isinstance(p, D.Plan):
            refused += 1
            if not (len(rec) == 1 and rec[0].split(" ", 1)[1] == D.reasons()[p]):
                bad.append((key, p, rec))
            continue
        if len(rec) != 2:
            bad.append((key, p, rec))
            continue
        lines = [golden["parsed"][i] for i in golden["sequences"][rec[1]]]
        want = walk(p, key)
        ok = len(lines) == len(want) and bool(rec[0]) == D.rs(p)
        for (name, args), (wname, wargs) in zip(lines, want):
            ok = ok and name == wname and all(args.get(k) == v for k, v in wargs.items())
            if name in D.LAUNCHER_NAMES:
                ok = ok and all(k in wargs for k in DECIDED if k in args)
        cats = [args["cat"] for _, args in lines]
        ok = ok and (cats.count("2"), cats.count("3"), cats.count("4") - 1) == (p.n_gemv, p.n_attn, p.n_other)
        if not ok:
            bad.append((key, p, lines))
    assert not bad, f"{len(bad)} of {len(planned)} steps differ; first (case, got, recorded): {bad[:2]}"
    assert D.reasons() == {-1: "decode_step: unsupported batch"}
    # refused: B = 0 and 17 on the MFMA path; 0, 3 and 5 .. 17 on the VALU path
    assert refused == 2 * 3 * 72 + 15 * 72


def test_grouping_admission_and_group_info_equal_the_recorded_ones(golden):
    lines = [f"G {m} {n}" for m in (0, 1) for n in range(41)] + [f"A {m} {n}" for m in (0, 1) for n, _ in golden["admit"][str(m)]]
    got = D.ask(lines)
    assert [list(s) for s in got[:41]] == golden["grouping"]["0"] and [list(s) for s in got[41:82]] == golden["grouping"]["1"]
    recorded = [1 - r for m in "01" for _, r in golden["admit"][m]]
    assert got[82:] == recorded and {n for n, _ in golden["admit"]["0"]} >= set(range(-1, 19))
    for m in (0, 1):                                                   # gvl_decode_group_info: (max_group, any_size)
        assert [D.group_size(m, D.MAX_BATCH), int(D.batch_ok(m, 3))] == golden["group_info"][str(m)] == [[4, 0], [16, 1]][m]
    assert D.parts(0, 7) == (4, 2, 1) and D.parts(0, 3) == (2, 1) and D.parts(1, 35) == (16, 16, 3) and D.parts(1, 0) == ()


def test_parts_are_admitted_sizes_that_sum_to_n():
    ns = list(range(0, 300))
    for mfma in (0, 1):
        got = D.ask([f"G {mfma} {n}" for n in ns])
        sizes = sorted({s for p in got for s in p})
        admitted = D.ask([f"A {mfma} {s}" for s in sizes])
        assert all(admitted) and sizes == ([1, 2, 4] if not mfma else list(range(1, 17)))
        greedy = D.ask([f"S {mfma} {n}" for n in ns[1:]])
        for n, p in zip(ns, got):
            assert sum(p) == n and list(p) == sorted(p, reverse=True), (mfma, n, p)
            assert not p or p[0] == greedy[n - 1]                       # each part is the largest admitted size for what is left
            assert mfma or 3 not in p
    assert [B for B in range(-2, 20) if D.batch_ok(0, B)] == [1, 2, 4] and [B for B in range(-2, 20) if D.batch_ok(1, B)] == list(range(1, 17))


def test_path_predicates_equal_the_recorded_conditions(golden):
    m = golden["mfma_ok"]
    cases = list(itertools.product(*m["axes"]))
    assert m["keys"] == ["hidden", "inter", "heads", "head_dim"] and len(cases) == len(m["bits"]) >= 3000
    got = D.ask(["M %d %d %d %d" % c for c in cases])
    assert "".join(map(str, got)) == m["bits"] and 0 < sum(got) < len(got)
    assert D.mfma_ok(3072, 8192, 32, 96) and D.mfma_ok(256, 256, 4, 64) and not D.mfma_ok(64, 128, 4, 16) and not D.mfma_ok(8192, 8192, 64, 128)
    q = golden["quant_refused"]
    cases = list(itertools.product(*q["axes"]))
    assert q["keys"] == ["mfma", "fmt", "hidden", "inter", "attn_width"] and len(cases) == len(q["bits"]) >= 8000
    ok = D.ask(["Q %d %d %d %d" % c[1:] for c in cases])
    # gvl_finalize_weights refuses a quantised format off the MFMA path, and on it wherever the predicate says no
    assert "".join(str(int(not (c[0] and o))) for c, o in zip(cases, ok)) == q["bits"] and 0 < sum(ok) < len(ok)
    assert D.quant_ok(0, 64, 64, 64) and D.quant_ok(1, 512, 1024, 512) and not D.quant_ok(2, 512, 1024, 512) and D.quant_ok(2, 1024, 2048, 1024)


def test_rs_is_the_recorded_condition_and_what_the_plan_shows(planned):
    keys = sorted({(mfma, fmt, nf, folded, hidden) for (B, mfma, fmt, nf, folded, hidden, layers), _, _ in planned})
    ok = dict(zip(keys, D.ask(["R %d %d %d %d %d" % k for k in keys])))
    for (B, mfma, fmt, nf, folded, hidden, layers), rec, p in served(planned):
        assert D.rs(p) == bool(ok[(mfma, fmt, nf, folded, hidden)]) == bool(rec[0]) == bool(mfma and not fmt and nf and folded and hidden in (512, 1024, 3072, 4096))
    assert not D.rs_ok(1, 0, 1, 1, 256) and D.rs_ok(1, 0, 1, 1, 512) and not D.rs_ok(1, 0, 1, 1, 4096 + 512)   # hidden / 16 partials: whole 32s, 256 at the most


def test_what_rs_implies(planned):
    n_rs = 0
    for key, _, p in served(planned):
        inputs = [p.proj[k].input for k in CONSUMERS]
        if D.rs(p):
            n_rs += 1
            assert not p.norm_launches and inputs == [D.XT_SQ] * 3 and all(p.proj[k].weight == D.TILED_FOLDED for k in CONSUMERS) and all(p.proj[k].sq_out for k in PRODUCERS), (key, p)
        else:
            assert D.XT_SQ not in inputs and not any(e.sq_out or e.weight == D.TILED_FOLDED for e in p.proj), (key, p)
            assert len(set(inputs)) == 1 and inputs[0] == p.proj[D.QKV0].input
        # layer 0's qkv: no projection produced its input -- the old norm path, never the raw copy, never a folded weight; the step's first launch serves it
        q0 = p.proj[D.QKV0]
        assert q0.input in (D.X_NORM, D.XN) and q0.weight != D.TILED_FOLDED and p.embed_norm == (q0.input == D.XN), (key, p)
        assert p.norm_launches == (not D.rs(p) and q0.input == D.XN)
        assert (p.proj[D.O_PROJ].input, p.proj[D.DOWN].input) == (D.ATTN, D.ACT)
    assert n_rs == 16 * 4 * 3                                          # B 1 .. 16 x the four hiddens that have the form x 1 .. 3 layers


def test_path_and_format_choose_launcher_weight_and_scales(planned):
    for (B, mfma, fmt, nf, folded, hidden, layers), _, p in served(planned):
        for kind, e in enumerate(p.proj):
            assert e.launcher == (D.DGEMM if mfma else D.GEMV) and bool(e.scales) == bool(mfma and fmt), (kind, e)
            assert e.weight == D.ROW_MAJOR if not mfma else e.weight in (D.TILED, D.TILED_FOLDED)
            assert not (fmt and e.weight == D.TILED_FOLDED)                                     # a quantised format never selects a folded copy
            assert bool(e.out_tiled) == bool(mfma and kind == D.GATE_UP)
        assert bool(p.attn_out_tiled) == bool(mfma)


def test_launch_counts(planned):
    for (B, mfma, fmt, nf, folded, hidden, layers), _, p in served(planned):
        assert (p.n_gemv, p.n_attn) == (4 * layers + 1, layers) and p.n_other == 1 + (2 * layers if p.norm_launches else 0)


def test_the_plan_reads_B_through_admission_and_the_consumer_norm_limit_only(planned):
    by_rest = {}
    for key, _, p in planned:
        by_rest.setdefault(key[1:], {})[key[0]] = p
    for rest, plans in by_rest.items():
        admitted = [B for B in range(18) if D.batch_ok(rest[0], B)] if rest[2:] == (0, 0, 64, 1) else ([1, 2, 4] if not rest[0] else list(range(1, 17)))
        assert sorted(B for B, p in plans.items() if isinstance(p, D.Plan)) == admitted
        small, large = ({plans[B] for B in admitted if (B <= D.MAX_VALU_BATCH) == s} for s in (True, False))
        assert len(small) == 1 and len(large) == (1 if rest[0] else 0), rest
        if rest[0]:
            (s,), (g,) = small, large
            assert not s.embed_norm and g.embed_norm and s.proj[D.QKV0].input == D.X_NORM and g.proj[D.QKV0].input == D.XN
            assert s._replace(embed_norm=0, norm_launches=0, n_other=0, proj=0) == g._replace(embed_norm=0, norm_launches=0, n_other=0, proj=0)
