"""CPU: attn_plan, decode_attn_plan and decode_attn_shape (csrc/gvl_attn_plan.h) -- which attention kernel a launch takes, on which grid -- against the decisions of the
launchers they replaced, and against properties that hold whatever the table says.  All attention forms are bit-identical by design, so no result test can notice a wrong
choice of form; this one can.
tests/golden/attn_launch_plans.json: see its "doc" (how it was recorded).  A fixed enumeration, no full product.  Prefill: nine base launches (the Llama-3 / Phi-3.5
prefill, the towers' paged, V-in-place, q,k,v-in-place and normalised-q launches, a ragged prefill); on each: S = 1 ... 16385, every head dim with Dout at, below, above it
and not a multiple of 8, extend contexts (valid, too short, without a table), every pitch too small, not a multiple of 8 and at the 4 GiB edge of a 64-row tile, every
optional operand added or dropped, every alignment fact false; on one base per mode also B KV = 1, 3, 8, 9 x H / KV = 1, 4 and not integral, ring, pipe, pipe_rows,
ones_row, k_ones, causal and each knob off its default; S x B KV on three of them; S x pipe x pipe_rows on the pipelined kernel; ragged groups of 1, 3, 8, 9 sequences,
empty and too long ones, missing tables, every field the mode forbids.  Decode: every head dim x group size x knob, x heads per block; cpb x nsplit x gsplit and batch x
nsplit.  Shape: batches of 1, 2, 16 at contexts of 1 ... 8192 tokens, both overrides, capturing or not."""
import json
import os

import pytest

import attn_plan as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "attn_launch_plans.json")


@pytest.fixture(scope="module")
def golden():
    with open(PATH) as f:
        g = json.load(f)
    p = g["prefill"]
    p["full"] = [dict(A.PREFILL_DEFAULTS, **{**p["bases"][b], **ov}) for b, ov in p["cases"]]
    g["shape"]["cases"] = [[g["shape"]["batches"][c[0]]] + c[1:] for c in g["shape"]["cases"]]
    return g


@pytest.fixture(scope="module")
def planned(golden):
    return dict(prefill=A.plans([A.prefill_line(**c) for c in golden["prefill"]["full"]]),
                decode=A.plans([A.decode_line(**dict(zip(A.DECODE_FIELDS, c))) for c in golden["decode"]["cases"]]),
                shape=A.plans([A.shape_line(*c) for c in golden["shape"]["cases"]]))


def test_header_builds_as_plain_host_cxx():
    """the header is host-only: the host compiler builds it with -Wall -Wextra -Werror -pedantic, no HIP header in sight"""
    assert os.access(A.dumper(), os.X_OK)
    for h in ("gvl_attn_plan.h", "gvl_limits.h"):
        with open(os.path.join(A.CSRC, h)) as f:
            text = f.read()
        assert "#include <hip" not in text and "getenv" not in text and "static " not in text.replace("static_assert", ""), h


def test_case_list_is_what_the_doc_says(golden):
    assert len(golden["prefill"]["cases"]) >= 900 and len(golden["decode"]["cases"]) >= 500 and len(golden["shape"]["cases"]) >= 600
    assert all(len(c) == len(p) for c, p in ((s["cases"], s["plans"]) for s in (golden["prefill"], golden["decode"], golden["shape"])))
    assert os.path.getsize(PATH) < 128 * 1024
    full = golden["prefill"]["full"]
    for f, vals in (("D", (64, 96, 128, 80)), ("S", (1, 127, 128, 129, 255, 256, 257, 2049, 16384, 16385)), ("ring", (0, 2, 3)), ("pipe", (0, 1, 2)), ("pipe_rows", (128, 256)),
                    ("ones_row", (0, 1)), ("k_ones", (0, 1)), ("causal", (0, 1)), ("vl_n", (1, 3, 8, 9)), ("no_ones", (0, 1))):
        assert set(vals) <= {c[f] for c in full}, f
    assert {1, 3, 8, 9} <= {c["B"] * c["KV"] for c in full}
    assert any(c["lazy"] != 8.0 for c in full) and any(c["H"] % c["KV"] for c in full)


def test_every_prefill_launch_equals_the_recorded_one(planned, golden):
    bad, refused = [], 0
    for c, got, want in zip(golden["prefill"]["cases"], planned["prefill"], golden["prefill"]["plans"]):
        flat = -1 if got is None else [x for l in got for x in l[1:]]
        refused += got is None
        if flat != want:
            bad.append((c, flat, want))
    assert not bad, f"{len(bad)} of {len(planned['prefill'])} plans differ; first (case, got, recorded): {bad[:3]}"
    assert 300 < refused < len(planned["prefill"]) - 500


def test_every_decode_launch_and_shape_equals_the_recorded_one(planned, golden):
    for what in ("decode", "shape"):
        bad = [(c, got, want) for c, got, want in zip(golden[what]["cases"], planned[what], golden[what]["plans"]) if (-1 if got is None else list(got)) != want]
        assert not bad, f"{what}: {len(bad)} of {len(planned[what])} differ; first (case, got, recorded): {bad[:3]}"


def test_query_rows_are_covered_exactly_once(planned, golden):
    two = 0
    for c, got in zip(golden["prefill"]["full"], planned["prefill"]):
        if got is None:
            continue
        assert 1 <= len(got) <= 2
        two += len(got) == 2
        at = 0
        for l in got:
            assert l.q_begin == at and l.q_rows > 0, (c, got)
            at += l.q_rows
            rows = [c["vl_rows"][u + 1] - c["vl_rows"][u] for u in range(c["vl_n"])] if l.VL else [l.q_rows]
            blocks = sum(-(-r // (32 * l.NWAVES)) for r in rows)                   # query blocks x (H / KV) x (KV B padded to the 8 XCDs)
            assert l.grid == blocks * (c["H"] // c["KV"]) * (-(-c["KV"] * c["B"] // 8) * 8) and l.block == 64 * l.NWAVES, (c, l)
            assert l.lds == (2 * 2 * 64 * 96 * 2 + 64 * 96 * 2 if l.family == A.IV2_PIPE else l.NS * 2 * 64 * l.D * 2 + 1024), (c, l)
            assert 0.0 <= l.lazy <= 64.0 and l.lazy == (c["lazy"] if 0.0 <= c["lazy"] <= 64.0 else 8.0)
        assert at == c["S"], (c, got)
    assert two >= 10          # the 8-wave + 4-wave split of the pipelined kernel is in the list


def test_the_mode_is_the_operands_and_the_template_arguments_follow_it(planned, golden):
    for c, got in zip(golden["prefill"]["full"], planned["prefill"]):
        for l in got or ():
            p = c["present"]
            want = A.RAGGED if c["vl_n"] else A.QNORM_V_ROWS if p & A.Q_RS else A.QKV_ROWS if p & A.KROWS else A.V_ROWS if p & A.VROWS else A.PAGED
            assert l.mode == want and (l.VROW, l.VL) == ((0, 1) if want == A.RAGGED else (want, 0)), (c, l)
            assert l.D == c["D"] and (l.family == A.FWD or l.mode == A.QNORM_V_ROWS), (c, l)
            assert not l.ONES or (c["ones_row"] and not c["causal"] and not c["no_ones"] and l.D == 96), (c, l)


# list entries that no recorded case plans, with the reason each exists
NEVER_PLANNED = {
    ("gqa", 96, 4, 1): "staged tiles need power-of-two rows, so the plan always takes STG 0 at D = 96; the replaced launcher compiled it anyway and the list keeps the code object unchanged",
    ("gqa", 96, 16, 1): "as (96, 4, 1)",
}


def test_planned_instantiations_are_exactly_the_lists(planned):
    seen = set()
    for got in planned["prefill"]:
        seen |= {A.kernel_of(l) for l in got or ()}
    seen |= {A.kernel_of(l) for l in planned["decode"] if l is not None}
    assert seen <= A.lists(), f"planned but not in the lists of gvl_attn_plan.h (the dispatch would refuse them): {sorted(seen - A.lists())}"
    assert A.lists() - seen == set(NEVER_PLANNED), f"in the lists, planned by no recorded case and not explained: {sorted(A.lists() - seen - set(NEVER_PLANNED))}"
    assert len(A.lists()) == 15 + 2 + 12 + 9


def test_decode_launch_is_normalised_and_its_grid_holds_every_unit(planned, golden):
    for c, l in zip(golden["decode"]["cases"], planned["decode"]):
        if l is None:
            continue
        H, KV = c[0], c[1]
        G = H // KV
        assert 1 <= l.batch <= 16 and l.cpb >= 1 and 1 <= l.gsplit <= c[3] <= 16 and H % KV == 0, (c, l)
        if l.family == A.GQA:
            assert 1 < G <= 16 and G % l.hpb == 0 and l.hpb <= l.t1 and (l.t2 == 0 or l.D in (64, 128)), (c, l)
            assert (l.grid_x, l.grid_y, l.grid_z) == (H // l.hpb * l.gsplit * l.batch, 1, 1), (c, l)
        elif l.t1 == 1:
            assert G > 1 and l.grid_x == 8 and l.grid_z == 1 and l.grid_y % G == 0 and l.grid_y // G * 8 >= KV * l.gsplit * l.batch > (l.grid_y // G - 1) * 8, (c, l)
        else:
            assert (l.t1 == 0) == (G == 1) and (l.grid_x, l.grid_y, l.grid_z) == (H, l.gsplit, l.batch), (c, l)


def test_shape_offers_every_sequence_its_splits(planned, golden):
    for c, s in zip(golden["shape"]["cases"], planned["shape"]):
        pos, H, KV, nsplit, fc, fh, capturing = c
        G = H // KV
        if capturing:
            assert s == A.Shape(nsplit, 1, 0), (c, s)            # valid whatever the positions are when the graph is replayed
            continue
        need = max(min(nsplit, max(1, -(-(p + 1) // 256))) for p in pos)
        assert s.cpb == (fc if 1 <= fc <= 16 else 1) and s.gsplit == -(-need // s.cpb), (c, s)
        assert s.hpb == (0 if G == 1 else fh if fh >= 1 and G % fh == 0 else s.hpb) and (G == 1 or G % s.hpb == 0), (c, s)


def test_op_iv2_attention_reaches_every_ones_form_and_both_pipelined_forms():
    """gvl_op_iv2_attention's launches (tests/test_gpu_iv2_attn.py asserts them per case): the descriptor alone chooses the kernel"""
    k = lambda *a, **kw: [A.kernel_of(l) for l in A.op_iv2_attention(*a, **kw)]
    for Dr in (72, 80, 88):
        assert k(2, 129, 3, Dr, 0) == [("fwd", 96, 4, 2, 1, 0, 0)] and k(2, 129, 3, Dr, 1) == [("fwd", 96, 4, 2, 1, 1, 0)]
    assert k(3, 257, 5, 88, 2, 0) == k(3, 257, 5, 88, 2, 0, 256) == [("fwd", 96, 4, 2, 1, 3, 0)]
    for pipe in (1, 2):
        assert k(3, 257, 5, 88, 2, pipe) == [("iv2_pipe", 4)] and k(3, 257, 5, 88, 2, pipe, 256) == [("iv2_pipe", 8), ("iv2_pipe", 4)]
        assert k(1, 512, 3, 88, 2, pipe, 256) == [("iv2_pipe", 8)] and k(1, 255, 3, 88, 2, pipe, 256) == [("iv2_pipe", 4)]
    l8, l4 = A.op_iv2_attention(3, 321, 5, 88, 2, 1, 256, ld=3 * 5 * 88 + 16)
    assert (l8.q_begin, l8.q_rows, l4.q_begin, l4.q_rows) == (0, 256, 256, 65) and l8.block == 512 and l4.block == 256 and l8.grid == 16 * 1 and l4.grid == 16 * 1
    assert A.op_iv2_attention(1, 16385, 3, 88, 2, 1) is None and A.op_iv2_attention(1, 129, 3, 88, 2, 1, ld=3 * 3 * 88 + 4) is None and A.op_iv2_attention(1, 129, 3, 80, 2, 1) is None
    assert {kk for f in (0, 1, 2) for kk in k(1, 129, 3, 88, f)} | {("iv2_pipe", 4), ("iv2_pipe", 8)} == {x for x in A.lists() if (x[0] == "fwd" and x[4] == 1) or x[0] == "iv2_pipe"}
