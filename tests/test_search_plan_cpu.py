"""CPU: the pure pieces the searches inside the library share (csrc/gvl_beam.h, driven by tests/c/search_plan_check.cc built with the host compiler).
  1. the cache reorder's plan: gvl_beam::reorder against beam.py's reorder and against a brute-force statement of the rule -- every parent vector for k = 2, 3, 4 over
     every set of closed beams (parents -1, out of range and closed included), a seeded sample at k = 16 -- and what applying a plan must give;
  2. the beam entries' value refusals: per entry every refusal alone, and every adjacent pair of the entry's order reporting the earlier one.  The texts and the orders
     are those of gvl_beam_search_n / gvl_group_beam_search before the function existed, written out here;
  3. model.py's one stepper behind beam_generate_ids (host path), plain and grouped, on a stub engine: the seq_clone / seq_free / decode_step_logits* calls and their
     arguments, against the record the two steppers it replaced left on the same stub (tests/golden/beam_stepper_calls.json)."""
import atexit
import functools
import itertools
import json
import os
import random
import shutil
import subprocess
import tempfile
import types
import zlib

import pytest
import torch

import conftest  # noqa: F401  (puts the package on sys.path)
from grounded_video_llm_amd import beam as B, logits as LP, model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grounded-video-llm_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "beam_stepper_calls.json")


@functools.lru_cache(maxsize=None)
def checker():
    tmp = tempfile.mkdtemp(prefix="gvl_search_plan_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "search_plan_check")
    cmd = ["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", CSRC, os.path.join(ROOT, "tests", "c", "search_plan_check.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def ask(lines):
    r = subprocess.run([checker()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return out


# ---- 1. the reorder plan ----------------------------------------------------------------------------------------------------------------------------------------
def brute_plan(beams, parents):
    """the rule, stated per parent: its children in beam order -- none: closed; the first keeps its sequence; the others are clones.  None: the error"""
    for p in parents:
        if p >= 0 and (p >= len(beams) or beams[p] < 0):
            return None
    src = [p if p >= 0 else -1 for p in parents]
    clones, closed = [], []
    for q, b in enumerate(beams):
        if b < 0:
            continue
        kids = [j for j, p in enumerate(parents) if p == q]
        if not kids:
            closed.append(q)
        clones += kids[1:]
    return src, sorted(clones), closed


def check_applied(beams, parents, plan):
    """what applying the plan gives: clones first (fresh ids), then the parents' own sequences, then the closes"""
    src, clones, closed = plan
    nxt, fresh = [-1] * len(parents), itertools.count(1000)
    for j in clones:
        assert beams[src[j]] >= 0 and src[j] not in closed
        nxt[j] = next(fresh)
    for j, p in enumerate(src):
        if p >= 0 and nxt[j] < 0:
            nxt[j] = beams[p]
    live = [j for j, p in enumerate(parents) if p >= 0]
    assert all(nxt[j] >= 0 for j in live) and all(nxt[j] < 0 for j in range(len(parents)) if j not in live)
    assert len({nxt[j] for j in live}) == len(live)                                       # every live child ends on a distinct sequence
    used = {p for p in parents if p >= 0}
    for q in used:                                                                        # exactly one child per parent reuses the parent's slot
        assert sum(1 for j in live if parents[j] == q and nxt[j] == beams[q]) == 1
    assert len(clones) == len(live) - len(used)                                           # clones = children - distinct parents
    assert closed == [q for q, b in enumerate(beams) if b >= 0 and q not in used]         # closed = parents without a child
    assert not (set(beams[q] for q in closed) & set(nxt))


def reorder_cases():
    cases = []
    for k in (2, 3, 4):
        for dead in itertools.product((False, True), repeat=k):
            beams = [-1 if d else 100 + q for q, d in enumerate(dead)]
            cases += [(beams, list(p)) for p in itertools.product(range(-1, k + 1), repeat=k)]    # k itself: out of range
        cases += [([100], list(p)) for p in itertools.product((-1, 0, 1), repeat=k)]      # the first step: one beam, the prompt's
    rng = random.Random(16)
    for _ in range(400):
        beams = [-1 if rng.random() < 0.25 else 100 + q for q in range(16)]
        live = [q for q, b in enumerate(beams) if b >= 0] or [0]
        wild = rng.random() < 0.2
        cases.append((beams, [rng.choice([-1] + (list(range(17)) if wild else live)) for _ in range(16)]))
    return cases


def test_reorder_plan_cxx_python_and_the_rule():
    cases = reorder_cases()
    out = ask([f"R {len(p)} {len(b)} " + " ".join(map(str, b)) + " " + " ".join(map(str, p)) for b, p in cases])
    n_err = 0
    for (beams, parents), line in zip(cases, out):
        want = brute_plan(beams, parents)
        py_beams, py_parents = [None if b < 0 else b for b in beams], [None if p < 0 else p for p in parents]
        if want is None:                                                                  # a child of a closed beam is the error, in both
            n_err += 1
            assert line == "error", (beams, parents, line)
            with pytest.raises(ValueError, match="a beam continues a closed beam"):
                B.reorder(py_beams, py_parents)
            continue
        parts = line.split("|")
        assert parts[0].strip() == "ok", (beams, parents, line)
        got = tuple([int(x) for x in part.split()] for part in parts[1:])
        assert got == want, (beams, parents, got, want)
        src, clones, closed = B.reorder(py_beams, py_parents)
        assert ([-1 if s is None else s for s in src], clones, closed) == want, (beams, parents)
        assert B.reorder(py_beams, parents)[1:] == (clones, closed)                        # a negative parent is None
        check_applied(beams, parents, want)
    assert n_err > 1000 and len(cases) - n_err > 1000                                      # both kinds, in numbers


# ---- 2. the value refusals --------------------------------------------------------------------------------------------------------------------------------------
BASE = dict(k=4, G=2, lam=1.0, nr=1, vocab=512, max_new=8, max_new_cap=64, cap=8, early=0, lp=1.0, penalty=1.0, ngram=0, min_new=0)
NEVER = 'early_stopping "never" with length_penalty > 0 needs a maximum length: not supported'
# per entry, in the entry's order: (name, what makes it the only fault, the text behind "<entry>: ")
PLAIN = [("num_return", dict(nr=5), "num_return must be 1 .. num_beams"),
         ("num_beams", dict(k=17), "num_beams must be 2 .. 16"),
         ("vocab", dict(vocab=7), "vocabulary smaller than 2 x num_beams"),
         ("int32", dict(vocab=2 ** 30), "num_beams x vocabulary must fit an int32"),
         ("max_new", dict(max_new=65, cap=65), "max_new_tokens must be 1 .. 64"),
         ("cap", dict(cap=7), "cap (room of out_ids_host) must be >= max_new_tokens"),
         ("early", dict(early=3), 'early_stopping must be 0 (False), 1 (True) or 2 ("never")'),
         ("never", dict(early=2, lp=1.0), NEVER),
         ("nan", dict(lp=float("nan")), "length_penalty is NaN"),
         ("penalty", dict(penalty=0.0), "penalty must be > 0, ngram >= 0, min_new >= 0")]
GROUP = [("num_beams", dict(k=17, G=17), "num_beams must be 2 .. 16"),
         ("groups", dict(G=3), "num_beam_groups must be 2 .. num_beams and divide num_beams"),
         ("lambda", dict(lam=0.0), "diversity_penalty must be > 0"),
         ("num_return", dict(nr=5), "num_return must be 1 .. num_beams"),
         ("vocab", dict(vocab=3), "vocabulary smaller than 2 x the beams of a group"),
         ("int32", dict(vocab=2 ** 30), "beams of a group x vocabulary must fit an int32")] + PLAIN[4:]
# two faults at once for the adjacent pairs of the order; pairs that exclude each other (vocab < 2 rows with rows x vocab > 2^31; early 3 with early 2; "never" needs
# length_penalty > 0, which NaN is not) have none
PAIRS = {("num_return", "num_beams"): dict(nr=0, k=1), ("num_beams", "vocab"): dict(k=17, vocab=7), ("int32", "max_new"): dict(vocab=2 ** 30, max_new=0),
         ("max_new", "cap"): dict(max_new=65, cap=7), ("cap", "early"): dict(cap=7, early=3), ("nan", "penalty"): dict(lp=float("nan"), penalty=-1.0),
         ("num_beams", "groups"): dict(k=1, G=0), ("groups", "lambda"): dict(G=3, lam=0.0), ("lambda", "num_return"): dict(lam=float("nan"), nr=0),
         ("num_return", "vocab"): dict(nr=0, vocab=3)}
# faults the LATER checks of a pair need spelled differently when the earlier one is of another kind
EXTRA = [("plain", dict(early=2, lp=1.0, penalty=0.0), NEVER), ("plain", dict(early=3, lp=float("nan")), 'early_stopping must be 0 (False), 1 (True) or 2 ("never")'),
         ("plain", dict(ngram=-1), "penalty must be > 0, ngram >= 0, min_new >= 0"), ("plain", dict(min_new=-1), "penalty must be > 0, ngram >= 0, min_new >= 0"),
         ("plain", dict(penalty=float("nan")), "penalty must be > 0, ngram >= 0, min_new >= 0"), ("plain", dict(max_new=0), "max_new_tokens must be 1 .. 64"),
         ("plain", dict(k=1), "num_beams must be 2 .. 16"), ("plain", dict(nr=0), "num_return must be 1 .. num_beams"),
         ("group", dict(G=1), "num_beam_groups must be 2 .. num_beams and divide num_beams"), ("group", dict(G=8), "num_beam_groups must be 2 .. num_beams and divide num_beams"),
         ("group", dict(lam=-1.0), "diversity_penalty must be > 0"),
         ("group", dict(k=32, G=2), "num_beams must be 2 .. 16"),                                                  # tests/test_gpu_group_beam.py relies on this one
         ("group", dict(k=16, G=16, vocab=7, nr=16), ""), ("plain", dict(k=16, vocab=32, nr=16), ""), ("plain", dict(early=2, lp=0.0), ""), ("plain", dict(early=2, lp=-1.0), "")]


def vline(grouped, over):
    a = dict(BASE, **over)
    return (f"V {int(grouped)} {a['k']} {a['G'] if grouped else 0} {float(a['lam']).hex() if a['lam'] == a['lam'] else 'nan'} {a['nr']} {a['vocab']} {a['max_new']} "
            f"{a['max_new_cap']} {a['cap']} {a['early']} {float(a['lp']).hex() if a['lp'] == a['lp'] else 'nan'} "
            f"{float(a['penalty']).hex() if a['penalty'] == a['penalty'] else 'nan'} {a['ngram']} {a['min_new']}")


def test_beam_refusals_alone_and_in_order():
    asked, want = [vline(False, {}), vline(True, {})], ["", ""]
    n_pairs = 0
    for grouped, table in ((False, PLAIN), (True, GROUP)):
        for name, over, text in table:
            asked.append(vline(grouped, over)); want.append(text)
        for (a, _, text), (b, _, _) in zip(table, table[1:]):
            if (a, b) in PAIRS:
                asked.append(vline(grouped, PAIRS[(a, b)])); want.append(text)
                n_pairs += 1
            else:
                assert (a, b) in (("vocab", "int32"), ("early", "never"), ("never", "nan")), (a, b)
    for which, over, text in EXTRA:
        asked.append(vline(which == "group", over)); want.append(text)
    assert n_pairs == 6 + 8
    got = ask(asked)
    for line, g, w in zip(asked, got, want):
        assert g == w, (line, g, w)


# ---- 3. the one stepper of beam_generate_ids ----------------------------------------------------------------------------------------------------------------------
VOCAB, EOS, PAD = 24, 7, 5
STEPPER_CASES = {   # name: (num_beams, groups, diversity_penalty, max_new, eos bias, decode_group_info, processors)
    "plain_k4": (4, 1, 0.0, 6, 0.0, {"max_group": 16, "any_size": 1}, False),
    "plain_k3_valu": (3, 1, 0.0, 5, 1.5, {"max_group": 4, "any_size": 0}, False),
    "plain_k4_processed": (4, 1, 0.0, 5, 0.0, {"max_group": 16, "any_size": 1}, True),
    "group_k4_g2": (4, 2, 1.0, 6, 0.0, {"max_group": 16, "any_size": 1}, False),
    "group_k4_g2_eos": (4, 2, 0.5, 8, 4.0, {"max_group": 16, "any_size": 1}, False),
    "group_k6_g3_valu_eos": (6, 3, 1.0, 8, 3.5, {"max_group": 4, "any_size": 0}, True),
    "group_k4_g4_eos": (4, 4, 2.0, 8, 4.5, {"max_group": 16, "any_size": 1}, False),
}


class StubEngine:
    """sequences are histories; a sequence's logits are a pure function of its history; ids come from a pool that hands the lowest free one out"""
    def __init__(self, seed, eos_bias, group_info):
        self.seed, self.eos_bias, self.group_info = seed, eos_bias, group_info
        self.hist, self.calls = {}, []

    def _logits(self, hist):
        g = torch.Generator().manual_seed(zlib.crc32(repr((self.seed, list(hist))).encode()))
        x = 2.0 * torch.randn(VOCAB, generator=g, dtype=torch.float32)
        x[EOS] += self.eos_bias
        return x

    def _new(self, hist):
        sid = min(set(range(len(self.hist) + 1)) - set(self.hist))
        self.hist[sid] = list(hist)
        return sid

    def splice(self, row, vis):
        return torch.zeros((len(row), 8))

    def decode_group_info(self):
        return dict(self.group_info)

    def seq_alloc(self, cap):
        return self._new([])

    def prefill(self, seq, emb, want_logits=False):
        return self._logits(self.hist[seq])

    def seq_clone(self, src, cap):
        sid = self._new(self.hist[src])
        self.calls.append(["seq_clone", int(src), int(cap), sid])
        return sid

    def seq_free(self, seq):
        self.calls.append(["seq_free", int(seq)])
        del self.hist[seq]

    def decode_step_logits(self, seq, tok):
        self.calls.append(["decode_step_logits", int(seq), int(tok)])
        self.hist[seq].append(int(tok))
        return self._logits(self.hist[seq])

    def decode_step_logits_batch(self, seqs, toks):
        self.calls.append(["decode_step_logits_batch", [int(s) for s in seqs], [int(t) for t in toks]])
        for s, t in zip(seqs, toks):
            self.hist[s].append(int(t))
        return torch.stack([self._logits(self.hist[s]) for s in seqs])

    def op_logits_process(self, logits, histories, *args, **kw):
        return logits

    def __getattr__(self, name):                              # the per-sequence option setters: nothing to do on a stub
        if name.startswith("seq_set_"):
            return lambda *a, **k: None
        raise AttributeError(name)


def run_stepper(name, model_module=M, logits_module=LP):
    k, G, lam, max_new, eos_bias, gi, processed = STEPPER_CASES[name]
    eng = StubEngine(name, eos_bias, gi)
    me = types.SimpleNamespace(engine=eng, tokenizer=types.SimpleNamespace(eos_token_id=EOS, pad_token_id=PAD), geo=types.SimpleNamespace(max_seq=64))
    procs = logits_module.Processors(penalty=1.3) if processed else None
    res = model_module.LLAVA_NEXT_VIDEO.beam_generate_ids(me, [1, 2, 3], None, k, max_new, processors=procs, with_scores=True, num_beam_groups=G, diversity_penalty=lam)
    assert not eng.hist, "every sequence goes back"
    return {"calls": eng.calls, "ids": res[0], "score": float(res[1]).hex()}


@pytest.mark.parametrize("name", sorted(STEPPER_CASES))
def test_one_stepper_reproduces_the_two(name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = run_stepper(name)
    assert got["ids"] == want["ids"] and got["score"] == want["score"]
    assert got["calls"] == want["calls"]                      # the order included: clones, install, free, step
    kinds = {c[0] for c in want["calls"]}
    assert {"seq_clone", "seq_free"} <= kinds and kinds & {"decode_step_logits", "decode_step_logits_batch"}
