"""Decoding grammars on the CPU (csrc/gvl_grammar.h: the checker, the blob packer, the reference walk; csrc/gvl_seq_table.h: a grammar's reference counts):
tests/c/grammar_check.cc includes the two headers alone and is built with the host C++ compiler, plain and with -fsanitize=address,undefined -- a stand-alone
program, nothing preloaded, no GPU.  Its self-test pins the checker's errors and limits, hand-written walks and the open / fork / close / destroy life cycle; its
`eval` mode answers for the header, and the Python mirror (grounded_video_llm_amd/grammar.py) must say the same: the same error text, the same walk, the same
allowed ids."""
import atexit
import functools
import json
import os
import random
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from grounded_video_llm_amd import grammar as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grounded-video-llm_amd", "csrc")
BUILDS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@functools.lru_cache(maxsize=None)
def checker(build):
    tmp = tempfile.mkdtemp(prefix="gvl_grammar_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "grammar_check")
    cmd = ["c++", "-std=c++17", *BUILDS[build], "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", CSRC, os.path.join(ROOT, "tests", "c", "grammar_check.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("build", list(BUILDS))
def test_header_selftest(build):
    r = subprocess.run([checker(build), "selftest"], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) >= 60 and all(ln.startswith("ok ") for ln in lines) and not r.stderr


def header_says(build, n_states, n_classes, start, vocab, token_class, class_base, trans, histories=()):
    """-> (the header's check message, [(on, state, reg, allowed ids or None)] per history)"""
    tc, cb, tr = [np.asarray(a).reshape(-1).tolist() for a in (token_class, class_base, trans)]
    words = [n_states, n_classes, start, vocab, len(tc), len(cb), len(tr), *tc, *cb, *tr, len(histories)]
    for h in histories:
        words += [len(h), *h]
    r = subprocess.run([checker(build), "eval"], input=" ".join(str(int(w)) for w in words) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = [json.loads(ln) for ln in r.stdout.splitlines()]
    return out[0]["check"], [(bool(o["on"]), o["state"], o["reg"], None if o["allowed"] == [-1] else o["allowed"]) for o in out[1:]]


def _interval(vocab=12):
    """tests/c/grammar_check.cc's interval(): ids 2 .. 9 ordinal, 10 eos; timestamp (SET) -> a word of {0, 1} -> timestamp (GE) -> eos -> END"""
    b = GR.GrammarBuilder(vocab)
    ts, eos, _never = b.token_class(range(2, 10), ordinal=True), b.token_class([10]), b.token_class([11])
    s = [b.state() for _ in range(5)]
    b.edge(s[0], ts, s[1], set_reg=True); b.edge(s[1], 0, s[2]); b.edge(s[2], ts, s[3], ge_reg=True); b.edge(s[3], eos, s[4])
    return b.build(s[0])


def _parts(g):
    return g.n_states, g.n_classes, g.start, g.vocab, g.token_class, g.class_base, g.trans


def _bad_descriptions():
    """(what, description) for every condition the library checks, as arrays past the builder"""
    g = _interval()
    ns, nc, st, V, tc, cb, tr = [np.array(x) if isinstance(x, np.ndarray) else x for x in _parts(g)]

    def mod(tc_=None, cb_=None, tr_=None, **kw):
        t, c, r = tc.copy(), cb.copy(), tr.copy()
        for arr, edits in ((t, tc_), (c, cb_), (r, tr_)):
            for k, v in (edits or {}).items():
                arr[k] = v
        d = dict(n_states=ns, n_classes=nc, start=st, vocab=V)
        d.update(kw)
        return d["n_states"], d["n_classes"], d["start"], d["vocab"], t, c, r
    yield "n_states is 0", mod(n_states=0)
    yield "n_states is 257", (257, 1, 0, 4, np.zeros(4), [-1], np.zeros(257))
    yield "n_classes is 65", (1, 65, 0, 4, np.zeros(4), [-1] * 65, np.zeros(65))
    yield "n_states * n_classes is 4097", (241, 17, 0, 4, np.zeros(4), [-1] * 17, np.zeros(4097))
    yield "vocab is 0", mod(vocab=0)
    yield "vocab is 8388609", mod(vocab=GR.MAX_VOCAB + 1)
    yield "start state 5 out of range", mod(start=5)
    yield "start state -1 out of range", mod(start=-1)
    yield "token 7 has class 4", mod(tc_={7: 4})
    yield "class 1: base -2 out of range", mod(cb_={1: -2})
    yield "class 1: base 5 out of range", mod(cb_={1: 5})
    yield "ordinal class 1 is not the contiguous id range 1 .. 8", mod(cb_={1: 1})
    yield "ordinal class 1 is not the contiguous id range 2 .. 8", mod(tc_={5: 0})
    yield "edge (state 1, class 0): SET / GE on a class that is not ordinal", mod(tr_={(1, 0): 2 | GR.SET})
    yield "edge (state 1, class 0): SET / GE on a class that is not ordinal", mod(tr_={(1, 0): 2 | GR.GE})
    yield "edge (state 1, class 0): next state 5 out of range", mod(tr_={(1, 0): 5})
    yield "edge (state 1, class 0): reserved bits set", mod(tr_={(1, 0): 2 | 0x400})
    yield "state 1 can forbid every token", mod(tc_={0: 3, 1: 3})               # the only edge of state 1 is on a class that is empty now


def test_python_check_and_the_header_give_the_same_message():
    seen = 0
    for what, d in _bad_descriptions():
        mine = GR.check(*d)
        assert what in mine, (what, mine)
        assert header_says("plain", *d)[0] == mine, what
        with pytest.raises(ValueError, match="grammar: "):
            GR.Grammar(*d)
        seen += 1
    assert seen == 18
    # the limits themselves pass, in both
    for ns, nc in ((256, 16), (64, 64), (128, 32)):
        tr = np.full((ns, nc), GR.FORBIDDEN)
        tr[:, 0] = np.arange(ns) % 256
        d = (ns, nc, 0, 64, np.zeros(64), [-1] * nc, tr)
        assert GR.check(*d) == "" and header_says("plain", *d)[0] == ""


def test_builder_raises_for_the_librarys_conditions():
    b = GR.GrammarBuilder(12)
    with pytest.raises(ValueError, match="n_states is 0"):
        b.build(0)
    b = GR.GrammarBuilder(12)
    ts = b.token_class([2, 3, 5], ordinal=True)                                 # a hole
    s = b.state()
    b.edge(s, ts, s)
    with pytest.raises(ValueError, match="not the contiguous id range"):
        b.build(s)
    b = GR.GrammarBuilder(12)
    w = b.token_class([4])
    s = b.state()
    b.edge(s, w, s, set_reg=True)
    with pytest.raises(ValueError, match="SET / GE on a class that is not ordinal"):
        b.build(s)
    b = GR.GrammarBuilder(12)
    s = b.state()
    b.edge(s, 0, 3)
    with pytest.raises(ValueError, match="next state 3 out of range"):
        b.build(s)
    b = GR.GrammarBuilder(12)
    big, small = b.token_class(range(0, 8), ordinal=True), b.token_class(range(8, 11), ordinal=True)
    s0, s1, s2 = b.state(), b.state(), b.state()
    b.edge(s0, big, s1, set_reg=True); b.edge(s1, small, s2, ge_reg=True)
    with pytest.raises(ValueError, match="state 1 can forbid every token"):
        b.build(s0)
    b = GR.GrammarBuilder(100)
    for t in range(64):
        b.token_class([t])                                                      # 65 classes with the implicit one
    b.state()
    with pytest.raises(ValueError, match="n_classes is 65"):
        b.build(0)
    b = GR.GrammarBuilder(12)
    for _ in range(257):
        b.state()
    with pytest.raises(ValueError, match="n_states is 257"):
        b.build(0)
    b = GR.GrammarBuilder(12)
    b.token_class([3])
    with pytest.raises(ValueError, match="already has class"):
        b.token_class([3])
    with pytest.raises(ValueError, match="outside"):
        b.token_class([12])
    with pytest.raises(ValueError, match="vocab is 0"):
        GR.GrammarBuilder(0)


HISTORIES = [[], [6], [6, 1], [2, 0], [9, 0], [6, 1, 6], [6, 1, 7, 10], [6, 1, 7, 10, 3], [6, 1, 5], [11], [0], [12], [-1], [6, 1, 5, 6], [6, 1, 8]]


@pytest.mark.parametrize("build", list(BUILDS))
def test_python_walk_and_allowed_equal_the_headers(build):
    g = _interval()
    msg, got = header_says(build, *_parts(g), histories=HISTORIES)
    assert msg == ""
    for h, (on, state, reg, allowed) in zip(HISTORIES, got):
        m = g.allowed(h)
        assert g.walk(h) == (on, state, reg), h
        assert (None if m is None else np.nonzero(m)[0].tolist()) == allowed, h
    assert got[1][3] == [0, 1] and got[2][3] == [6, 7, 8, 9] and got[4][3] == [9] and got[5][3] == [10] and got[6][3] is None and got[8][3] is None
    assert g.accepts([6, 1, 7, 10]) and not g.accepts([6, 1, 7]) and not g.accepts([6, 1, 5, 10])
    fn = g.as_prefix_allowed_tokens_fn()
    assert fn(0, np.array([6, 1])) == [6, 7, 8, 9] and fn(0, [6, 1, 5]) == list(range(12))      # where the device leaves the row alone HF gets every id


def test_random_grammars_and_histories_match_the_header():
    rng = random.Random(20240611)
    for _ in range(12):
        V, ns, nc = rng.choice((5, 40, 300)), rng.randrange(1, 7), rng.randrange(1, 5)
        cuts = sorted(rng.sample(range(1, V), min(nc - 1, V - 1)))              # contiguous classes, so any of them may be ordinal
        nc = len(cuts) + 1
        tc = np.zeros(V, dtype=np.int64)
        for c, lo in enumerate(cuts):
            tc[lo:] = c + 1
        base = [([0] + cuts)[c] if rng.random() < 0.6 else -1 for c in range(nc)]
        tr = np.full((ns, nc), GR.FORBIDDEN)
        for s in range(ns):
            for c in range(nc):
                if rng.random() < 0.6:
                    flags = (GR.SET if rng.random() < 0.4 else 0) | (GR.GE if rng.random() < 0.4 else 0) if base[c] >= 0 else 0
                    tr[s, c] = rng.randrange(ns) | flags
        d = (ns, nc, rng.randrange(ns), V, tc, base, tr)
        hs = [[rng.randrange(-1, V + 1) if rng.random() < 0.03 else rng.randrange(V) for _ in range(rng.randrange(0, 6))] for _ in range(40)]
        msg, got = header_says("plain", *d, histories=hs)
        assert GR.check(*d) == msg
        if msg:
            continue
        g = GR.Grammar(*d)
        for h, (on, state, reg, allowed) in zip(hs, got):
            m = g.allowed(h)
            assert g.walk(h) == (on, state, reg) and (None if m is None else np.nonzero(m)[0].tolist()) == allowed, (d, h)
