"""CPU: prefill_plan (csrc/gvl_prefill_plan.h) under PrefillGeometry.score -- the launches of a group whose rows are scored (gvl_score_extend_varlen).  A score tail reads
rows anywhere in the group, behind any prefixes: the plan refuses neither a prefix nor a group, takes exactly the per-layer steps of the same geometry without the flag, and
differs from it only in the last layer's tail, which is off (tail / last_rows are those of last_layer_tail = 0).  Built on tests/c/prefill_score_plan_dump.cc, whose case
line carries the flag; the recorded plans of tests/test_prefill_plan_cpu.py (flag off) are untouched by this file.
Seeded sweep: nb 1 .. 8, ragged and equal lengths, prefixes 0 and multiples of 64, both sides of rope_orig_max_pos, every knob setting."""
import os
import random
import subprocess
import tempfile

import pytest

import prefill_plan as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_AND_LOSS = -5                                          # GVL_PREFILL_SCORE_AND_LOSS


@pytest.fixture(scope="module")
def exe():
    out = os.path.join(tempfile.mkdtemp(prefix="gvl_score_plan_"), "prefill_score_plan_dump")
    cmd = ["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", P.CSRC, os.path.join(ROOT, "tests", "c", "prefill_score_plan_dump.cc"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run(exe, cases):
    """cases: (lens, pos0, kw, score) -> per case a (P.Plan, off) pair or a refusal"""
    lines = [P.plan_line(lens, pos0, **kw) + f" {int(score)}" for lens, pos0, kw, score in cases]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    got = r.stdout.splitlines()
    assert len(got) == len(lines)
    out = []
    for ln, g in zip(lines, got):
        if "|" not in g:
            out.append(int(g))
        else:
            plan, off = g.split("|")
            out.append((P.parse(ln, plan), tuple(int(x) for x in off.split())))
    return out


def sweep():
    rng = random.Random(20260319)
    cases = []
    for nb in range(1, 9):
        for rep in range(40):
            if rep % 5 == 0:
                lens = (rng.choice((1, 7, 64, 65, 200)),) * nb
            else:
                lens = tuple(rng.choice((1, 2, 13, 40, 63, 64, 65, 70, 128, 190, 201, 333)) for _ in range(nb))
            pos0 = () if rep % 3 == 0 else tuple(64 * rng.choice((0, 0, 1, 2, 3, 54)) for _ in range(nb))
            for va in (0, 1, 2):
                for ve in (0, 1):
                    kw = dict(varlen_attn=va, varlen_extend=ve, last_layer_tail=rng.randrange(2), norm_fused=rng.randrange(2),
                              rope_orig_max_pos=rng.choice((0, 200, 4096)), long_table=rng.randrange(2))
                    if rng.randrange(4) == 0:
                        kw.update(hidden=rng.choice((256, 320, 100)), fused_weights=rng.randrange(2))
                    cases.append((lens, pos0, kw))
    for tail in (0, 1):                                       # every knob setting in full on one ragged group behind prefixes and one without
        for nf in (0, 1):
            for va in (0, 1, 2):
                for ve in (0, 1):
                    for pos0 in ((), (128, 0, 64)):
                        cases.append(((70, 1, 33), pos0, dict(varlen_attn=va, varlen_extend=ve, last_layer_tail=tail, norm_fused=nf, rope_orig_max_pos=200, long_table=1)))
    return cases


def test_score_plan_is_the_plain_plan_with_the_last_layer_tail_off(exe):
    cases = sweep()
    scored = run(exe, [(lens, pos0, kw, 1) for lens, pos0, kw in cases])
    plain = run(exe, [(lens, pos0, kw, 0) for lens, pos0, kw in cases])
    no_tail = run(exe, [(lens, pos0, dict(kw, last_layer_tail=0), 0) for lens, pos0, kw in cases])
    # the flag off is the plan the existing dump prints (the recorded plans' tool): a geometry without the member reads false
    assert [p[0] for p in plain] == P.plans([P.plan_line(lens, pos0, **kw) for lens, pos0, kw in cases])
    seen = {"ext": 0, "group": 0, "tail_differs": 0, "straddle": 0}
    for (lens, pos0, kw), s, p, t in zip(cases, scored, plain, no_tail):
        assert not isinstance(s, int), (lens, pos0, kw, s)                      # no refusal for a prefix or a group
        (sp, soff), (pp, poff), (tp, _) = s, p, t
        assert soff == poff == tuple(sum(lens[:b]) for b in range(len(lens) + 1))
        assert (sp.M, sp.nf, sp.batched_table, sp.steps) == (pp.M, pp.nf, pp.batched_table, pp.steps), (lens, pos0, kw)
        assert (sp.tail, sp.last_rows, sp.chunks) == (0, tp.last_rows, tp.chunks) and sp == tp, (lens, pos0, kw)
        assert sp.last_rows == (P.LAST_STRIDED if len(lens) == 1 or sp.batched_table else P.LAST_GATHERED)
        seen["ext"] += any(pos0)
        seen["group"] += len(lens) > 1
        seen["tail_differs"] += sp != pp
        ends = {bool(kw["rope_orig_max_pos"] and kw["long_table"] and q + L > kw["rope_orig_max_pos"]) for L, q in zip(lens, pos0 or (0,) * len(lens))}
        seen["straddle"] += len(ends) == 2
    assert min(seen.values()) >= 100, seen
    assert {len(lens) for lens, _, _ in cases} == set(range(1, 9))


def test_refusals_under_score(exe):
    r = subprocess.run([exe, "reasons"], capture_output=True, text=True)
    assert r.returncode == 0
    reasons = {int(ln.split(" ", 1)[0]): ln.split(" ", 1)[1] for ln in r.stdout.splitlines()}
    assert reasons[SCORE_AND_LOSS] == "llm_prefill: a score tail and a loss tail exclude each other"
    assert {k: reasons[k] for k in (-1, -2, -3, -4)} == P.reasons()             # the old four keep their words
    g3, ext = ((5, 9, 70), ()), ((5,), (64,))
    # score && loss: the new refusal, whatever else holds -- also where the loss alone would have been refused for its prefix or its group
    for lens, pos0 in (((5,), ()), g3, ext):
        assert run(exe, [(lens, pos0, dict(loss=1), 1)]) == [SCORE_AND_LOSS]
    # the two loss refusals still stand without the flag and are absent under it (without a loss request)
    assert run(exe, [(ext[0], ext[1], dict(loss=1), 0), (g3[0], g3[1], dict(loss=1), 0)]) == [P.LOSS_BEHIND_PREFIX, P.LOSS_GROUP]
    assert all(not isinstance(p, int) for p in run(exe, [(ext[0], ext[1], {}, 1), (g3[0], g3[1], {}, 1), ((3, 4, 5, 6, 7, 8, 9, 10), (64,) * 8, {}, 1)]))
    # what is refused for every request stays refused
    assert run(exe, [((), (), {}, 1), ((1,) * 9, (), {}, 1), ((5, 6), (0, 32), {}, 1), ((5,), (-64,), {}, 1)]) == [P.BAD_BATCH, P.BAD_BATCH, P.BAD_PREFIX, P.BAD_PREFIX]
