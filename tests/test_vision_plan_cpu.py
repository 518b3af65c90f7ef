"""CPU: vision_plan, glue_plan, vision_operand_path, patch_embed_fused_ok and the workspace tables (csrc/gvl_vision_plan.h) -- which launches clip_encode, iv2_encode and
build_visual take, in which order, with which arguments, in which workspace -- against the launches of the functions they were cut out of.  The towers' forms are bit-identical
or equal within the towers' tolerances by design, so no result test can notice a tower that silently lost one; this one can.
tests/golden/vision_launch_plans.json: see its "doc" (how it was recorded).  Both towers at the real geometries and at the tiny ones of tests/test_gpu_vision_plan.py; head dims
16, 64, 88, 96, 100 and 128; widths with and without a factor of 64; inter % 16 != 0; layers_run 1 .. 3 (and 23 / 39); n = 1, 2, 3, 96 and on both sides of the 2^32
pixel-offset limit; the folded weights and the tile-order patch weight present and absent -- each under the full product of the five knobs; the glue for both LLM kinds; and
gvl_op_attention over causal x vision_in_place x head dim."""
import itertools
import json
import os

import pytest

import vision_plan as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "vision_launch_plans.json")
KNOB_PRODUCT = set(itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 1, 2), (128, 256)))


@pytest.fixture(scope="module")
def golden():
    with open(PATH) as f:
        return json.load(f)


def recorded(golden, seq):
    """the launch lines of sequence `seq`: an item is a line that names no layer, or [block, first layer, layers] = the block's lines with # = the layer, once per layer"""
    out = []
    for item in golden["sequences"][seq]:
        if isinstance(item, int):
            out.append(golden["lines"][item])
        else:
            out += [golden["lines"][i].replace("[#].", f"[{l}].") for l in range(item[1], item[1] + item[2]) for i in golden["blocks"][item[0]]]
    return out


@pytest.fixture(scope="module")
def towers(golden):
    """[(config, knobs, recorded bytes, recorded allocs, recorded lines, the dumper's TowerCall)]"""
    order = sorted(KNOB_PRODUCT)
    cases = [(cfg, dict(zip(V.KNOBS, k)), nbytes, golden["allocs"][pairs[2 * j]], recorded(golden, pairs[2 * j + 1]))
             for cfg, (nbytes, pairs) in zip(golden["towers"], golden["tower_cases"]) for j, k in enumerate(order)]
    got = V.ask([V.tower_line(*cfg, **k) for cfg, k, _, _, _ in cases])
    return [c + (g,) for c, g in zip(cases, got)]


@pytest.fixture(scope="module")
def glues(golden):
    cases = [(c[:6], c[6], c[7], golden["allocs"][c[8]], recorded(golden, c[9])) for c in golden["glue_cases"]]
    got = V.ask([V.glue_line(*cfg) for cfg, _, _, _, _ in cases])
    return [c + (g,) for c, g in zip(cases, got)]


def fused_ok_py(tower, n, T, image, patch, C):
    """the geometries patch_embed_kernel serves, restated for the property test below"""
    return patch == 14 and image % 14 == 0 and C in (1024, 1408) and n * 3 * T * image * image < 0xffffffff and (tower == V.IV2 or (C == 1024 and T == 1))


def differing(cases):
    """(config, knobs or None, first differing line pair) of every case whose walk does not print the recorded lines, line by line"""
    bad = []
    for c in cases:
        want, got = c[-2], list(c[-1].lines)
        if got != want:
            at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            bad.append((c[0], c[1] if isinstance(c[1], dict) else None, got[at:at + 1], want[at:at + 1]))
    return bad


def test_header_builds_as_plain_host_cxx():
    """the header is host-only: the host compiler builds it with -Wall -Wextra -Werror -pedantic, no HIP header in sight"""
    assert os.access(V.dumper(), os.X_OK)
    with open(os.path.join(V.CSRC, "gvl_vision_plan.h")) as f:
        text = f.read()
    assert "#include <hip" not in text and "getenv" not in text and "static " not in text.replace("static_assert", "")


def test_case_list_is_what_the_doc_says(golden, towers, glues):
    cfgs = [tuple(t) for t in golden["towers"]]
    by_cfg = {}
    for cfg, k, *_ in towers:
        by_cfg.setdefault(tuple(cfg), set()).add(tuple(k[f] for f in V.KNOBS))
    assert set(by_cfg) == set(cfgs) and all(ks == KNOB_PRODUCT for ks in by_cfg.values()) and all(len(c[1]) == 2 * len(KNOB_PRODUCT) for c in golden["tower_cases"])   # every tower under the full product
    assert (0, 2, 1024, 4096, 16, 336, 14, 1, 23, 1, 0) in cfgs and (1, 2, 1408, 6144, 16, 224, 14, 8, 39, 1, 1) in cfgs
    for tower in (V.CLIP, V.IV2):
        mine = [c for c in cfgs if c[0] == tower]
        assert {16, 64, 88, 96, 100, 128} <= {c[2] // c[4] for c in mine}
        assert {1, 2, 3} <= {c[8] for c in mine} and {1, 2, 96} <= {c[1] for c in mine}
        assert {True, False} == {c[2] % 64 == 0 for c in mine} == {bool(c[9]) for c in mine}
        pixels = lambda c: c[1] * 3 * c[7] * c[5] * c[5]
        assert any(pixels(c) < 0xffffffff <= pixels(c[:1] + (c[1] + 1,) + c[2:]) and c[:1] + (c[1] + 1,) + c[2:] in mine for c in mine)    # n and n + 1 straddle the 2^32 limit
    iv2 = [c for c in cfgs if c[0] == V.IV2]
    assert any(c[3] % 16 for c in iv2) and {0, 1} == {c[10] for c in iv2}
    assert {(c[0][0], c[0][1]) for c in glues} == {(phi, n) for phi in (0, 1) for n in (1, 2, 96)}
    ops = golden["op_cases"]
    assert {(o[0], o[6], o[5]) for o in ops} >= {(v, c, d) for v in (0, 1, 2) for c in (0, 1) for d in (16, 64, 88, 96, 128)} and any(o[7] for o in ops)
    assert os.path.getsize(PATH) < 1 << 20


def test_every_tower_walk_prints_the_recorded_launches(towers):
    bad = differing(towers)
    assert not bad, f"{len(bad)} of {len(towers)} calls differ; first (config, knobs, got, recorded): {bad[:3]}"
    assert len(towers) >= 2500 and sum(len(c[4]) for c in towers) >= 50000


def test_every_glue_walk_prints_the_recorded_launches(glues):
    bad = differing(glues)
    assert not bad, f"{len(bad)} of {len(glues)} calls differ; first: {bad[:3]}"
    for (phi, *_), _, _, _, want, g in glues:
        assert (g.hd_merge, g.glb_row) == (phi, phi) and len(want) == (9 if phi else 7)


def test_three_doctored_expectations_are_reported(towers, glues):
    """the comparison notices a changed argument, a dropped launch and a swapped pair"""
    cfg, k, b, a, want, got = next(c for c in towers if c[0][0] == V.IV2 and c[0][8] == 3 and c[5].nf)
    i = next(i for i, ln in enumerate(want) if "gvl_launch_attention" in ln)
    doctored = (want[:i] + [want[i].replace(" B=", " B=1")] + want[i + 1:], want[:i] + want[i + 1:], want[:i - 1] + [want[i], want[i - 1]] + want[i + 1:])
    for d in doctored:
        assert d != want and len(differing([(cfg, k, b, a, d, got)])) == 1
    assert not differing([(cfg, k, b, a, want, got)])
    gcase = glues[0]
    assert len(differing([gcase[:4] + (gcase[4][::-1], gcase[5])])) == 1


def test_workspace_sums_equal_the_recorded_bytes_and_hold_every_buffer(towers, glues):
    seen = set()
    for cfg, k, nbytes, allocs, _, g in towers:
        assert g.bytes == nbytes, (cfg, k, g.bytes, nbytes)                                 # clip_bytes / iv2_bytes: the arena size does not change
        table = {name: elem * count for name, elem, count in g.table}
        assert [name for name, _, _ in g.table][:10] == ["x", "h", "qkv", "att", "mlp", "pA", "pO", "Q", "Kt", "Vt"] and len(table) == (10 if cfg[0] == V.CLIP else 13)
        for name, asked in allocs:
            assert table[name] >= asked, (cfg, k, name, table[name], asked)
            seen.add((name, table[name] == asked))
        assert {name for name, _ in allocs} == set(table)
    assert ("sq", False) in seen and ("sq", True) in seen and {s for s in seen if not s[1]} == {("sq", False)}   # sq alone is larger than asked, with norm_fused off
    for cfg, nbytes, fbytes, allocs, _, g in glues:
        assert (g.bytes, g.feats_bytes) == (nbytes, fbytes), (cfg, g.bytes, nbytes, g.feats_bytes, fbytes)
        table = {name: elem * count for name, elem, count in g.table}
        assert all(table[name] >= asked for name, asked in allocs) and [name for name, _ in allocs] == [name for name, _, _ in g.table][:6]
    # the table is a function of the geometry alone
    by_cfg = {}
    for cfg, _, _, _, _, g in towers:
        by_cfg.setdefault(tuple(cfg), set()).add((g.bytes, g.table))
    assert all(len(v) == 1 for v in by_cfg.values())


def test_plan_counts_equal_the_recorded_launches(towers, glues):
    for cfg, k, _, _, want, g in towers:
        assert (g.n_gemm, g.n_attn, g.n_other) == V.counts(want), (cfg, k)
    for cfg, _, _, _, want, g in glues:
        assert (g.n_gemm, g.n_attn, g.n_other) == V.counts(want), cfg


def test_the_knobs_choose_the_form(towers):
    """properties that hold whatever the table says, read off the plan, and every form reached"""
    n = dict.fromkeys(("fused", "three", "pages", "v_rows", "qk_rows", "q_on_load", "nf", "unfused", "pipe", "pipe256"), 0)
    for cfg, k, _, _, want, g in towers:
        tower, C, heads, L = cfg[0], cfg[2], cfg[4], cfg[8]
        Dr = C // heads
        D = V.pad_head(Dr)
        assert g.patch_fused == bool(k["patch_fused"] and cfg[9] and fused_ok_py(tower, cfg[1], cfg[7], cfg[5], cfg[6], C)), (cfg, k)
        assert g.vt_pages == (not k["vision_in_place"] or D == 128) and g.qkv_post == (not g.qk_rows)
        assert g.qk_rows == (tower == V.CLIP and k["vision_in_place"] == 1 and Dr == 64) and g.q_on_load == (tower == V.IV2 and k["vision_in_place"] == 1 and Dr == 88)
        assert g.nf == bool(tower == V.IV2 and k["norm_fused"] and cfg[10] and C % 64 == 0 and cfg[3] % 16 == 0)
        assert (g.pipe, g.pipe_rows) == ((k["attn_pipe"], k["attn_pipe_rows"]) if g.q_on_load else (0, 0))
        assert g.first == V.Block(True, not g.nf, g.nf, g.nf and L > 1) and g.middle == V.Block(not g.nf, not g.nf, g.nf, g.nf) and g.last == V.Block(not g.nf, not g.nf, g.nf, False)
        assert sum("rowsq=" in ln for ln in want) == (2 * L - 1 if g.nf else 0) == sum("rowscale=" in ln for ln in want)
        assert sum("gvl_launch_qkv_post" in ln for ln in want) == (L if g.qkv_post else 0)
        for key, hit in (("fused", g.patch_fused), ("three", not g.patch_fused), ("pages", g.vt_pages), ("v_rows", not g.vt_pages and g.qkv_post and not g.q_on_load), ("qk_rows", g.qk_rows),
                         ("q_on_load", g.q_on_load), ("nf", g.nf), ("unfused", tower == V.IV2 and not g.nf), ("pipe", g.pipe == 1), ("pipe256", g.pipe_rows == 256)):
            n[key] += bool(hit)
    assert min(n.values()) >= 40, n


def test_op_attention_takes_the_towers_operand_path(golden):
    """gvl_op_attention (gvl_ops.hip) asks vision_operand_path; its recorded launches say what the parent's own copy of the decision chose"""
    ops = golden["op_cases"]
    paths = V.ask([f"P {vip} {V.pad_head(Dr)} {Dr} {causal} {V.CLIP}" for vip, B, S, H, KV, Dr, causal, *_ in ops])
    served = 0
    for (vip, B, S, H, KV, Dr, causal, rc, _, seq), p in zip(ops, paths):
        lines = recorded(golden, seq)
        if rc:
            assert Dr % 8 and not lines
            continue
        served += 1
        post = [ln for ln in lines if "gvl_launch_qkv_post" in ln]
        attn = [ln for ln in lines if "gvl_launch_attention" in ln]
        assert len(attn) == 1 and len(post) + 1 == len(lines) and lines[-1] == attn[0]
        assert p.qkv_post == bool(post) and p.qk_rows == (" Qrows=" in attn[0]) == (" Krows=" in attn[0]) and p.vt_pages == (" Vrows=" not in attn[0])
        assert not post or p.vt_pages == (" Vt=" in post[0])
        assert not (p.q_on_load or p.ones_row or p.k_ones or p.attn_ones_row or p.attn_k_ones)
    assert served >= 60
