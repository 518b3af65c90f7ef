"""The host bookkeeping of gvl_beam_search (csrc/gvl_beam.h) on the CPU, against beam.py: tests/c/beam_check.cc includes that header alone, is built with the
host C++ compiler (so the header needs no HIP) and replays the per-step candidate lists that beam.beam_search saw through its `candidates` hook.  A seeded
synthetic model whose logits are a pure function of a beam's history drives beam.py; the hook does the torch top-2k and records every list.  Parents, tokens,
the final ids, the hypothesis score (as a double) and the transition scores must be equal EXACTLY.  Hand-written candidate scripts pin the remaining rules."""
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
from grounded_video_llm_amd.beam import beam_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grounded-video-llm_amd", "csrc")
ERR_NEVER, ERR_FEW = -1, -2                        # gvl_beam::Status
EARLY = {False: 0, True: 1, "never": 2}
V = 40                                             # >= 2 x 16


@functools.lru_cache(maxsize=None)
def checker():
    tmp = tempfile.mkdtemp(prefix="gvl_beam_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "beam_check")
    cmd = ["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", CSRC, os.path.join(ROOT, "tests", "c", "beam_check.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def replay(k, vocab, max_new, eos, lp, early, record):
    """the checker's lines for `record` (per step a list of (value, flat index, processed log-probability))"""
    lines = [f"{k} {vocab} {max_new} {-1 if eos is None else eos} {float(lp).hex()} {EARLY[early]}"]
    for cands in record:
        lines.append(" ".join([str(len(cands))] + [f"{float(v).hex()} {int(i)} {float(p).hex()}" for v, i, p in cands]))
    r = subprocess.run([checker()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return [ln.split("|") for ln in r.stdout.splitlines()]


def python_side(k, vocab, max_new, eos, lp, early, hook, logits_of):
    """beam.py through the hook -> (result or ("error", text), the (parents, tokens) every step() call saw)"""
    seen, beams = [], [[] for _ in range(k)]

    def step(parents, toks):
        seen.append((list(parents), list(toks)))
        beams[:] = [beams[p] + [t] for p, t in zip(parents, toks)]
        return torch.stack([logits_of(b) for b in beams])
    try:
        return beam_search(step, logits_of([]), k, max_new, eos, lp, early, None, None, True, candidates=hook), seen
    except ValueError as e:
        return ("error", str(e)), seen


def compare(py, seen, out, k):
    """every line of the checker against what beam.py did"""
    steps = [o for o in out if o[0].startswith("step")]
    for (parents, toks), o in zip(seen, steps):
        assert [int(x) for x in o[1].split()] == parents and [int(x) for x in o[2].split()] == toks
        assert o[0].split()[1] == "0"                                  # beam.py stepped again: the checker said "continue"
    if py[0] == "error":
        assert out[-1][0].startswith("error"), out[-1]
        code = int(out[-1][0].split()[1])
        assert code == (ERR_FEW if "fewer than" in py[1] else ERR_NEVER), (code, py[1])
        assert len(steps) == len(seen)
        return
    ids, score, ts = py
    assert len(steps) == len(seen) + 1 and steps[-1][0].split()[1] == "1"
    fin = out[-1]
    assert fin[0].split()[0] == "final"
    assert float(fin[0].split()[1]) == score, (fin[0], repr(score))    # %.17g round-trips a double
    assert [int(x) for x in fin[1].split()] == ids
    assert [float(x) for x in fin[2].split()] == ts


# ---- a seeded synthetic model: the logits of a beam are a pure function of its history -----------------------------------------------
def model(seed, eos, eos_bias):
    def logits_of(hist):
        g = torch.Generator().manual_seed(zlib.crc32(repr((seed, list(hist))).encode()))
        x = 2.0 * torch.randn(V, generator=g, dtype=torch.float32)
        if eos is not None:
            x[eos] += eos_bias
        return x
    return logits_of


def topk_hook(k, record):
    def hook(rows, scores):
        t = rows + scores[:, None]
        top = torch.topk(t.reshape(-1), 2 * k, largest=True, sorted=True)
        vals, idxs, pv = top.values.tolist(), top.indices.tolist(), rows.reshape(-1)[top.indices].tolist()
        record.append(list(zip(vals, idxs, pv)))
        return vals, idxs, pv
    return hook


EOS_MODES = {"absent": (None, 0.0), "rare": (7, -1.0), "frequent": (7, 3.5)}


@pytest.mark.parametrize("k", [2, 3, 4, 16])
def test_bookkeeping_equals_beam_py(k):
    stats = {"closed": 0, "skipped": 0, "errors_never": 0, "done_early": 0, "runs": 0}
    for early, lp, (mode, (eos, bias)), max_new in itertools.product((False, True, "never"), (0.0, 0.8, 1.0, 2.0), EOS_MODES.items(), (1, 2, 12)):
        seed = zlib.crc32(repr((k, early, lp, mode, max_new)).encode())
        logits_of = model(seed, eos, bias)
        record = []
        py, seen = python_side(k, V, max_new, eos, lp, early, topk_hook(k, record), logits_of)
        out = replay(k, V, max_new, eos, lp, early, record)
        compare(py, seen, out, k)
        # the hook changes nothing: beam.py's own torch path gives the same answer
        if py[0] != "error":
            beams = [[] for _ in range(k)]

            def step(parents, toks):
                beams[:] = [beams[p] + [t] for p, t in zip(parents, toks)]
                return torch.stack([logits_of(b) for b in beams])
            assert beam_search(step, logits_of([]), k, max_new, eos, lp, early, None, None, True) == py
        stats["runs"] += 1
        stats["errors_never"] += py[0] == "error" and "never" in py[1]
        stats["done_early"] += py[0] != "error" and len(record) < max_new
        for cands in record:                                           # what the candidate lists exercised
            n_next = 0
            for rank, (_, ix, _) in enumerate(cands):
                if eos is not None and ix % V == eos:
                    stats["closed" if rank < k else "skipped"] += 1
                else:
                    n_next += 1
                if n_next == k:
                    break
    # the runs reached every rule: hypotheses closed at rank < k, eos skipped at rank >= k, the "never" error, searches that stopped before max_new
    assert stats["runs"] == 108 and min(stats["closed"], stats["skipped"], stats["errors_never"], stats["done_early"]) > 0, stats


# ---- hand-written candidate scripts, through beam.py and the checker alike -------------------------------------------------------------
def scripted(k, vocab, max_new, eos, lp, early, script):
    it = iter(script)

    def hook(rows, scores):
        c = next(it)
        return [v for v, _, _ in c], [i for _, i, _ in c], [p for _, _, p in c]
    py, seen = python_side(k, vocab, max_new, eos, lp, early, hook, lambda hist: torch.zeros(vocab))
    out = replay(k, vocab, max_new, eos, lp, early, script[:len(seen) + 1])
    compare(py, seen, out, k)
    return py, out


def test_equal_final_scores_the_last_added_hypothesis_wins():
    py, _ = scripted(2, 8, 1, None, 1.0, False, [[(-1.0, 3, -1.0), (-1.0, 5, -1.0), (-2.0, 1, -2.0), (-3.0, 2, -3.0)]])
    assert py == ([5], -1.0, [-1.0])


def test_eos_is_appended_only_while_the_output_is_shorter_than_max_new():
    # the eos of rank 0 at the last step closes [1]; it wins over the open beams and becomes [1, eos]: exactly max_new ids
    s = [[(-0.125, 1, -0.125), (-0.25, 2, -0.25), (-1.0, 3, -1.0), (-2.0, 4, -2.0)],
         [(-0.15625, 7, -0.03125), (-0.5, 3, -0.375), (-0.625, 8 + 4, -0.375), (-1.0, 5, -0.875)]]
    py, _ = scripted(2, 8, 2, 7, 1.0, False, s)
    assert py == ([1, 7], -0.15625 / 2, [-0.125, -0.03125])
    py, _ = scripted(2, 8, 1, 7, 1.0, False, [[(-0.5, 7, -0.5), (-1.0, 3, -1.0), (-2.0, 4, -2.0), (-3.0, 5, -3.0)]])
    assert py == ([7], -0.5, [-0.5])                                  # max_new 1: the empty hypothesis plus its eos
    # a longer open beam that scores better than the closed one: no eos on it
    s[1][0] = (-3.0, 7, -2.875)
    py, _ = scripted(2, 8, 2, 7, 1.0, False, s)
    assert py == ([1, 3], -0.25, [-0.125, -0.375])


def test_fewer_than_k_non_eos_candidates_is_an_error():
    py, out = scripted(2, 8, 4, 7, 1.0, False, [[(-0.5, 7, -0.5), (-1.0, 15, -1.0), (-2.0, 3, -2.0)]])
    assert py[0] == "error" and out[-1][0].split()[:2] == ["error", str(ERR_FEW)]


def test_never_with_a_positive_length_penalty_is_an_error_once_the_rule_is_evaluated():
    two_eos = [[(-0.5, 7, -0.5), (-1.0, 15, -1.0), (-2.0, 3, -2.0), (-3.0, 4, -3.0)]]
    py, out = scripted(2, 8, 4, 7, 1.0, "never", two_eos)
    assert py[0] == "error" and out[-1][0].split()[:2] == ["error", str(ERR_NEVER)]
    py, out = scripted(2, 8, 4, 7, 0.0, "never", two_eos + [[(-2.5, 1, -0.5), (-2.75, 8 + 2, 0.25), (-3.0, 3, -1.0), (-4.0, 4, -2.0)]])
    assert py[0] != "error" and py[0] == [7]                          # penalty 0: the rule is legal, and both hypotheses beat what is still running
