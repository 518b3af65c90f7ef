"""CPU: diverse (group) beam search on the host.
  1. beam.py's group_beam_search against tests/group_beam_ref.py, the literal restatement of transformers 4.40.1 (_group_beam_search + BeamSearchScorer with groups +
     HammingDiversityLogitsProcessor): ids, scores as Python floats and transition scores, EXACTLY, on a seeded synthetic model;
  2. csrc/gvl_beam.h's GroupBeamState (tests/c/group_beam_check.cc, built with the host compiler) against beam.py step by step on the candidate lists beam.py saw;
  3. hand-written cases: a done group hands pad to the later groups' counts, its beams never become hypotheses, the later pooled hypothesis wins equal scores;
  4. generate()'s validation errors, before any engine work;
  5. with s = 1 and a large penalty the groups' first tokens are the G best tokens of the prompt's row -- which plain beam search (the parent's answer to these
     arguments: it ignored them) does not give;  num_beam_groups=1, diversity_penalty=0.0 is the call without them."""
import atexit
import functools
import itertools
import os
import shutil
import subprocess
import tempfile
import zlib

import pytest
import torch

import conftest  # noqa: F401  (puts the package on sys.path)
from grounded_video_llm_amd import beam as B, model as M
from group_beam_ref import group_beam_search_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grounded-video-llm_amd", "csrc")
EARLY = {False: 0, True: 1, "never": 2}
V = 40
PAD = 5
KG = [(2, 2), (4, 2), (4, 4), (6, 3), (16, 4), (16, 16)]
LAMBDAS = (0.5, 1.0, 5.0)
EOS_MODES = {"absent": (None, 0.0), "rare": (7, -1.0), "frequent": (7, 3.5)}


def model(seed, eos, eos_bias):
    """a beam's logits are a pure function of its history (tests/test_beam_host_cpu.py::model)"""
    def logits_of(hist):
        g = torch.Generator().manual_seed(zlib.crc32(repr((seed, list(hist))).encode()))
        x = 2.0 * torch.randn(V, generator=g, dtype=torch.float32)
        if eos is not None:
            x[eos] += eos_bias
        return x
    return logits_of


@functools.lru_cache(maxsize=None)
def checker():
    tmp = tempfile.mkdtemp(prefix="gvl_group_beam_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "group_beam_check")
    cmd = ["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", CSRC, os.path.join(ROOT, "tests", "c", "group_beam_check.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def replay(k, G, vocab, max_new, eos, pad, lp, early, n_ret, record):
    """the checker's lines for `record`: per step a list of G candidate lists (empty: the group was done)"""
    lines = [f"{k} {G} {vocab} {max_new} {-1 if eos is None else eos} {-1 if pad is None else pad} {float(lp).hex()} {EARLY[early]} {n_ret}"]
    for groups in record:
        lines.append("  ".join(" ".join([str(len(c))] + [f"{float(v).hex()} {int(i)} {float(p).hex()}" for v, i, p in c]) for c in groups))
    r = subprocess.run([checker()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr, r.stdout)
    return [ln.split("|") for ln in r.stdout.splitlines()]


def recording_hook(G, s, record, script=None):
    """beam.py's `candidates` hook: the torch top-2s of the group (or the next scripted list), recorded per step and group"""
    last = [G]

    def hook(rows, scores, group):
        if group <= last[0]:
            record.append([[] for _ in range(G)])
        last[0] = group
        if script is not None:
            c = script[len(record) - 1][group]
        else:
            top = torch.topk((rows + scores[:, None]).reshape(-1), 2 * s, largest=True, sorted=True)
            c = list(zip(top.values.tolist(), top.indices.tolist(), rows.reshape(-1)[top.indices].tolist()))
        record[-1][group] = list(c)
        return [v for v, _, _ in c], [i for _, i, _ in c], [p for _, _, p in c]
    return hook


def python_side(k, G, lam, vocab, max_new, eos, pad, lp, early, n_ret, hook, logits_of):
    """beam.py through the hook -> (result or ("error", text), the (parents, tokens) every step() call saw)"""
    seen, beams = [], [[] for _ in range(k)]

    def step(parents, toks):
        seen.append(([-1 if p is None else p for p in parents], list(toks)))
        beams[:] = [None if p is None else beams[p] + [t] for p, t in zip(parents, toks)]
        return torch.stack([torch.zeros(vocab) if b is None else logits_of(b) for b in beams])
    try:
        return B.group_beam_search(step, logits_of([]), k, G, lam, max_new, eos, lp, early, None, True, candidates=hook, num_return=n_ret, pad_id=pad), seen
    except ValueError as e:
        return ("error", str(e)), seen


def compare_checker(py, seen, out, n_ret):
    steps = [o for o in out if o[0].startswith("step")]
    for (parents, toks), o in zip(seen, steps):
        assert [int(x) for x in o[1].split()] == parents and [int(x) for x in o[2].split()] == toks, (o, parents, toks)
        assert o[0].split()[1] == "0"
    if py[0] == "error":
        assert out[-1][0].startswith("error"), out[-1]
        assert int(out[-1][0].split()[1]) == (-2 if "fewer than" in py[1] else -1)
        return
    assert len(steps) == len(seen) + 1 and steps[-1][0].split()[1] == "1"
    fins = [o for o in out if o[0].startswith("final")]
    res = [py] if n_ret == 1 else py
    assert len(fins) == len(res) == n_ret
    for fin, (ids, score, ts) in zip(fins, res):
        assert float(fin[0].split()[1]) == score, (fin[0], repr(score))
        assert [int(x) for x in fin[1].split()] == ids
        assert [float(x) for x in fin[2].split()] == ts


@pytest.mark.parametrize("k,G", KG)
def test_beam_py_equals_the_literal_restatement_and_the_header_equals_beam_py(k, G):
    """early_stopping x length_penalty x eos mode x max_new in full (108 runs per (k, G)); lambda and num_return cycle through the runs so that every value of each meets
    every (k, G), every early_stopping mode and every eos mode."""
    s = k // G
    stats = {"runs": 0, "errors": 0, "done_group_steps": 0, "ended_early": 0, "closed": 0}
    grid = itertools.product((False, True, "never"), (0.0, 0.8, 1.0, 2.0), EOS_MODES.items(), (1, 2, 12))
    for i, (early, lp, (mode, (eos, bias)), max_new) in enumerate(grid):
        lam, n_ret = LAMBDAS[(i + i // 3) % 3], (1, k)[(i // 2 + i // 9) % 2]
        logits_of = model(zlib.crc32(repr((k, G, early, lp, mode, max_new)).encode()), eos, bias)
        record = []
        py, seen = python_side(k, G, lam, V, max_new, eos, PAD, lp, early, n_ret, recording_hook(G, s, record), logits_of)
        try:
            ref = group_beam_search_ref(logits_of, k, G, lam, max_new, eos, PAD, lp, early, n_ret)
        except ValueError as e:
            ref = ("error", str(e))
        if py[0] == "error":
            assert ref[0] == "error" and ref[1] == py[1]
        else:
            assert py == ref, (k, G, early, lp, mode, max_new, lam, n_ret)
            # the hook changes nothing: beam.py's own torch path, entered through beam_search's arguments
            beams = [[] for _ in range(k)]

            def step(parents, toks):
                beams[:] = [None if p is None else beams[p] + [t] for p, t in zip(parents, toks)]
                return torch.stack([torch.zeros(V) if b is None else logits_of(b) for b in beams])
            assert B.beam_search(step, logits_of([]), k, max_new, eos, lp, early, None, None, True, num_return=n_ret, num_beam_groups=G, diversity_penalty=lam,
                                 pad_id=PAD) == py
        compare_checker(py, seen, replay(k, G, V, max_new, eos, PAD, lp, early, n_ret, record), n_ret)
        stats["runs"] += 1
        stats["errors"] += py[0] == "error"
        stats["ended_early"] += py[0] != "error" and len(record) < max_new
        stats["done_group_steps"] += sum(1 for groups in record if any(not c for c in groups))
        stats["closed"] += sum(1 for groups in record for c in groups for r, (_, ix, _) in enumerate(c[:s]) if eos is not None and ix % V == eos)
    # the runs reached the rules that matter: closed hypotheses, "never" errors, steps at which some group was already done while another went on, early ends
    assert stats["runs"] == 108 and min(stats["errors"], stats["ended_early"], stats["closed"]) > 0, stats
    if G < k or k <= 4:
        assert stats["done_group_steps"] > 0, stats


# ---- hand-written candidate scripts ----------------------------------------------------------------------------------------------------
def scripted(k, G, lam, vocab, max_new, eos, pad, lp, early, n_ret, script, process=None):
    record = []
    s = k // G
    seen = []

    def step(parents, toks):
        seen.append(([-1 if p is None else p for p in parents], list(toks)))
        return torch.zeros((k, vocab))
    py = B.group_beam_search(step, torch.zeros(vocab), k, G, lam, max_new, eos, lp, early, process, True, candidates=recording_hook(G, s, record, script),
                             num_return=n_ret, pad_id=pad)
    compare_checker(py, seen, replay(k, G, vocab, max_new, eos, pad, lp, early, n_ret, record), n_ret)
    return py, seen, record


def test_a_done_group_hands_pad_to_the_later_counts_and_never_becomes_a_hypothesis():
    # k = 2, G = 2 (s = 1), eos 7, early_stopping True.  Step 1: group 0's best candidate is eos -> its one hypothesis exists -> done; its beam goes on with token 3.
    # Step 2: group 0 is not processed -- its token is pad (5), which group 1's Hamming term must count; group 1 closes too.
    counted = []

    def process(histories, rows, group, prev_tokens, diversity_penalty):
        counted.append((group, list(prev_tokens)))
        return rows
    script = [[[(-0.25, 7, -0.25), (-0.5, 3, -0.5)], [(-0.75, 4, -0.75), (-1.0, 6, -1.0)]],
              [[], [(-1.0, 7, -0.25), (-1.5, 2, -0.75)]]]
    py, seen, record = scripted(2, 2, 1.0, 8, 6, 7, 5, 1.0, True, 2, script, process)
    assert counted == [(0, []), (1, [3]), (1, [5])]                       # step 2: group 0 was skipped, its pad is what group 1 sees
    assert seen == [([0, 0], [3, 4])] and record[1][0] == []
    # the pooled hypotheses: group 0's [] + eos (score -0.25 / 1) and group 1's [4] + eos (-1.0 / 2); group 0's running beam [3, pad] is in neither
    assert py == [([7], -0.25, [-0.25]), ([4, 7], -0.5, [-0.75, -0.25])]
    # without a pad id the done group's tokens count nowhere
    counted.clear()
    scripted(2, 2, 1.0, 8, 6, 7, None, 1.0, True, 1, script, process)
    assert counted[-1] == (1, [-1]) and B.hamming_penalty(torch.zeros((1, 8)), [-1], 1.0).abs().sum() == 0


def test_a_done_groups_open_beams_are_not_added_at_the_end():
    # max_new 2: group 0 is done after step 1 (early_stopping True); at the end only group 1's open beam joins the pool
    script = [[[(-0.25, 7, -0.25), (-0.5, 3, -0.5)], [(-0.75, 4, -0.75), (-1.0, 6, -1.0)]],
              [[], [(-1.0, 2, -0.25), (-1.5, 1, -0.75)]]]
    py, seen, _ = scripted(2, 2, 1.0, 8, 2, 7, 5, 1.0, True, 2, script)
    assert py == [([7], -0.25, [-0.25]), ([4, 2], -0.5, [-0.75, -0.25])]


def test_among_the_pooled_hypotheses_the_later_one_wins_equal_scores():
    # both groups' only beams end open with the same score: group 1's hypothesis is later in the pool and comes first
    script = [[[(-1.0, 3, -1.0), (-2.0, 1, -2.0)], [(-1.0, 4, -1.0), (-2.0, 2, -2.0)]]]
    py, _, _ = scripted(2, 2, 1.0, 8, 1, None, None, 1.0, False, 2, script)
    assert py == [([4], -1.0, [-1.0]), ([3], -1.0, [-1.0])]
    assert scripted(2, 2, 1.0, 8, 1, None, None, 1.0, False, 1, script)[0] == ([4], -1.0, [-1.0])


def test_the_hamming_term_is_one_rounded_product_and_one_subtract():
    lam, rows = 0.1, torch.tensor([[0.3, -1.7, float("-inf"), 2.5, -0.0]])
    got = B.hamming_penalty(rows, [1, 1, 1, 3, 2, 9, -1], lam)
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    assert got[0, 1] == f(-1.7) - f(0.1) * f(3.0) and got[0, 3] == f(2.5) - f(0.1) * f(1.0)
    assert got[0, 0] == rows[0, 0] and got[0, 2] == float("-inf") and got[0, 4] == 0.0


# ---- validation ------------------------------------------------------------------------------------------------------------------------
class _NoEngine:
    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} reached")


def test_generate_validates_the_group_arguments_before_any_work():
    from types import SimpleNamespace
    m = M.LLAVA_NEXT_VIDEO.__new__(M.LLAVA_NEXT_VIDEO)
    m.engine, m.geo = _NoEngine(), SimpleNamespace(vocab=640)
    samples = {"prompts": ["a"], "video_ids": ["x"], "spatial_pixel_values": torch.zeros((1, 1))}
    bad = [(dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.0, do_sample=True), "`do_sample` must be set to `False`"),
           (dict(num_beams=4, diversity_penalty=1.0, do_sample=True), "`do_sample` must be set to `False`"),
           (dict(num_beams=4, num_beam_groups=3, diversity_penalty=1.0), "divisible by `num_beam_groups`"),
           (dict(num_beams=2, num_beam_groups=4, diversity_penalty=1.0), "smaller or equal than `num_beams`"),
           (dict(num_beam_groups=2, diversity_penalty=1.0), "smaller or equal than `num_beams`"),
           (dict(num_beams=4, num_beam_groups=2), "otherwise your groups will be identical"),
           (dict(num_beams=4, num_beam_groups=2, diversity_penalty=0.0), "otherwise your groups will be identical"),
           (dict(num_beams=4, diversity_penalty=1.0), "`num_beam_groups` should be greater than 1"),
           (dict(num_beams=4, num_beam_groups=1, diversity_penalty=0.5), "`num_beam_groups` should be greater than 1"),
           (dict(num_beams=4, num_beam_groups=2, diversity_penalty=-1.0), "float strictly larger than 0"),
           (dict(num_beams=4, num_beam_groups=2, diversity_penalty=1), "float strictly larger than 0"),
           (dict(num_beams=4, num_beam_groups=2, diversity_penalty="1.0"), "float strictly larger than 0"),
           (dict(num_beams=4, num_beam_groups=2, diversity_penalty=float("nan")), "float strictly larger than 0"),
           (dict(num_beams=4, num_beam_groups=0, diversity_penalty=1.0), "strictly positive integer"),
           (dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.0, num_return_sequences=5), r"`num_return_sequences` \(5\) has to be smaller or equal to `num_beams`"),
           (dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.0, constraints=[object()]), "constrained beams"),
           (dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.0, force_words_ids=[[1]]), "constrained beams"),
           (dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.0, guidance_scale=2.0, negative_prompts=["n"]), "guidance_scale")]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            m.generate(samples, **kw)
    with pytest.raises(ValueError, match="generate_shared.*num_beam_groups"):
        m.generate_shared({"spatial_pixel_values": torch.zeros((1, 1))}, ["a"], num_beams=4, num_beam_groups=2, diversity_penalty=1.0)
    assert M.beam_groups(dict()) is None and M.beam_groups(dict(num_beams=4, num_beam_groups=1, diversity_penalty=0.0)) is None
    assert M.beam_groups(dict(num_beams=4, num_beam_groups=None, diversity_penalty=None)) is None
    assert M.beam_groups(dict(num_beams=6, num_beam_groups=3, diversity_penalty=0.5)) == (3, 0.5)
    with pytest.raises(ValueError, match="must be set to `False`"):
        B.beam_search(lambda p, t: None, torch.zeros(V), 4, 3, None, sample={}, num_beam_groups=2, diversity_penalty=1.0)


def test_the_scheduler_refuses_groups():
    from grounded_video_llm_amd import serve
    from test_host_logic import _Emb, _ScriptedEngine
    sch = serve.ClipScheduler(_ScriptedEngine(64), 2, max_active=2)
    with pytest.raises(ValueError, match="num_beam_groups"):
        sch.submit(_Emb(4, 1), 4, num_beam_groups=2, diversity_penalty=1.0)
    with pytest.raises(ValueError, match="num_beam_groups"):
        sch.submit(_Emb(4, 1), 4, diversity_penalty=1.0)


# ---- the property plain beam search does not have ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [2, 4, 16])
def test_with_one_beam_per_group_and_a_large_penalty_the_first_tokens_are_the_best_tokens_of_the_prompt_row(G):
    logits_of = model(G, None, 0.0)
    best = torch.topk(torch.log_softmax(logits_of([]), dim=-1), G).indices.tolist()
    firsts = []

    def step(parents, toks):
        firsts.append(list(toks))
        raise StopIteration

    with pytest.raises(StopIteration):
        B.beam_search(step, logits_of([]), G, 4, min(set(range(V)) - set(best)), num_beam_groups=G, diversity_penalty=1e4, pad_id=0)      # eos: not among the G best
    assert firsts[0] == best and len(set(firsts[0])) == G
    # plain beam search at the same k -- what these arguments gave while they were ignored -- starts every beam from the same row too, but orders them alike only by chance
    # later on; its FIRST tokens are the same G best, so the difference must show in the results: with groups every returned sequence starts with a different token
    beams = [[] for _ in range(G)]

    def step2(parents, toks):
        beams[:] = [None if p is None else beams[p] + [t] for p, t in zip(parents, toks)]
        return torch.stack([torch.zeros(V) if b is None else logits_of(b) for b in beams])
    res = B.beam_search(step2, logits_of([]), G, 4, None, num_return=G, num_beam_groups=G, diversity_penalty=1e4, pad_id=0)
    assert sorted(r[0] for r in res) == sorted(best)


def test_one_group_and_no_penalty_is_the_call_without_them():
    for k, eos in ((2, None), (4, 7), (16, 7)):
        logits_of = model(k, eos, 1.0)
        out = []
        for kw in (dict(), dict(num_beam_groups=1, diversity_penalty=0.0, pad_id=3)):
            beams = [[] for _ in range(k)]

            def step(parents, toks):
                beams[:] = [beams[p] + [t] for p, t in zip(parents, toks)]
                return torch.stack([logits_of(b) for b in beams])
            out.append(B.beam_search(step, logits_of([]), k, 8, eos, 1.0, False, None, None, True, num_return=k, **kw))
        assert out[0] == out[1]
