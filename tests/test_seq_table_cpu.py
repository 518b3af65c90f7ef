"""The sequence table (csrc/gvl_seq_table.h: slots, KV pages, settings and rule-set references of gvl_seq_alloc / fork / clone / free and of the
token-rule entry points) on the CPU: tests/c/seq_table_check.cc includes that header alone, is built with the host C++ compiler (so the header
needs no HIP) and replays a script of operations, printing the whole table after every line.  Hand-written scripts pin the limits and the
inheritance rules; a few thousand seeded random operations are compared, line by line, with a small Python model of the table."""
import atexit
import functools
import itertools
import json
import os
import random
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grounded-video-llm_amd", "csrc")
BAD, DUPLICATE, NO_PAGES, TOO_MANY, NO_RULES, RULES_BUSY, RULES_FULL = -1, -2, -3, -4, -5, -6, -7     # SeqStatus (gvl_seq_table.h)
SEL_OFF = [1.0, 0, 0, -1, -1, -1]                   # SeqSelect as the program prints it: penalty, ngram, min_new, eos, top_n, rules
LENGTHS = (1, 63, 64, 65, 129)                      # 1, 1, 1, 2 and 3 pages of 64 tokens


@functools.lru_cache(maxsize=None)
def checker():
    tmp = tempfile.mkdtemp(prefix="gvl_seqtab_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "seq_table_check")
    cmd = ["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", CSRC, os.path.join(ROOT, "tests", "c", "seq_table_check.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def initial(pages):
    return {"any_live": 0, "slots": 0, "free": list(range(pages - 1, -1, -1)), "ref": [0] * pages, "default": list(SEL_OFF), "seqs": {}, "rules": {}}


def check_invariants(st, pages):
    holders = [p for s in st["seqs"].values() for p in s["pages"]]
    assert len(set(st["free"])) == len(st["free"]) and not set(st["free"]) & set(holders)
    assert len(st["free"]) + len(set(holders)) == pages                       # every page is free or held, never both, never lost
    assert st["ref"] == [holders.count(p) for p in range(pages)]             # page_ref[p] = the number of holders of p
    for s in st["seqs"].values():
        assert len(s["pages"]) == s["n_pages"] == (s["max"] + 63) // 64 and len(set(s["pages"])) == len(s["pages"])
    sels = [s["sel"] for s in st["seqs"].values()] + [st["default"]]          # a rule set's count = its holders, the default included
    assert st["rules"] == {k: sum(sel[5] == int(k) for sel in sels) for k in st["rules"]}
    assert all(sel[5] == -1 or str(sel[5]) in st["rules"] for sel in sels)    # nobody references a destroyed set
    assert st["any_live"] == int(bool(st["seqs"]))


def run(script, pages=8, max_seqs=4, max_rules=3):
    """-> the table after every line of `script` (with that line's "rc"); checks the invariants and that a refused operation changed nothing"""
    lines = [ln.strip() for ln in script.strip().splitlines() if ln.strip()]
    r = subprocess.run([checker(), str(pages), str(max_seqs), str(max_rules)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = [json.loads(ln) for ln in r.stdout.splitlines()]
    assert len(out) == len(lines)
    prev = initial(pages)
    for ln, st in zip(lines, out):
        check_invariants(st, pages)
        rc = st.pop("rc")
        if rc < 0:
            assert st == prev, f"`{ln}` was refused ({rc}) but changed the table"
        prev = dict(st)
        st["rc"] = rc
    return out


def rcs(script, **kw):
    return [st["rc"] for st in run(script, **kw)]


def same_table(a, b):
    """equal up to the order of the free list and the slots the vector has grown to"""
    def norm(st):
        return {k: (sorted(v) if k == "free" else v) for k, v in st.items() if k not in ("rc", "slots")}
    return norm(a) == norm(b)


# ---- hand-written scripts ------------------------------------------------------------------------------------------------------
def test_lengths_fill_the_pool_exactly_and_everything_comes_back():
    out = run("\n".join(f"alloc {n}" for n in LENGTHS) + "\nalloc 1\nlive 4\nlive 5\n" + "\n".join(f"free {i}" for i in (2, 0, 4, 1, 3)), max_seqs=8)
    assert [st["rc"] for st in out[:8]] == [0, 1, 2, 3, 4, NO_PAGES, 0, BAD]
    assert [len(out[4]["seqs"][str(i)]["pages"]) for i in range(5)] == [1, 1, 1, 2, 3] and out[4]["free"] == []
    assert out[0]["seqs"]["0"]["pages"] == [0] and out[4]["seqs"]["4"]["pages"] == [5, 6, 7]        # pages are handed out in ascending order
    assert all(st["rc"] == 0 for st in out[8:]) and same_table(out[-1], initial(8))


def test_limits_and_their_order():
    assert rcs("alloc 1\nalloc 1\nalloc 1\nfree 0\nalloc 1\nalloc 1", max_seqs=2) == [0, 1, TOO_MANY, 0, 0, TOO_MANY]      # a freed slot is taken again
    assert rcs("alloc 64\nalloc 64\npos 0 64\nfork 0 64 128\nclone 0 128", pages=1, max_seqs=1) == [0, NO_PAGES, 0, NO_PAGES, NO_PAGES]   # both limits hit: pages are checked before slots
    assert rcs("alloc 64\npos 0 64\nfork 0 64 128\nclone 0 128", pages=2, max_seqs=1) == [0, 0, TOO_MANY, TOO_MANY]
    assert rcs("alloc 0\nalloc -5\nfork 0 0 1") == [BAD, BAD, BAD]


def test_fork_of_exactly_one_page_shares_it_until_the_last_holder_goes():
    out = run("alloc 129\npos 0 100\nfork 0 64 128\nfork 0 64 65\nfree 0\nfree 1\nfree 2")
    assert [st["rc"] for st in out] == [0, 0, 1, 2, 0, 0, 0]
    assert out[2]["seqs"]["1"] == {"max": 128, "n_pages": 2, "pos": 64, "n_gen": 0, "pages": [0, 3], "sel": SEL_OFF}
    assert out[3]["seqs"]["2"]["pages"] == [0, 4] and out[3]["ref"][:5] == [3, 1, 1, 1, 1]
    assert out[4]["ref"][:3] == [2, 0, 0] and 0 not in out[4]["free"]          # the source is gone, its shared page lives on
    assert out[5]["ref"][0] == 1 and same_table(out[6], initial(8))


def test_clone_on_and_off_a_page_boundary():
    out = run("alloc 192\npos 0 128\nclone 0 192\npos 0 100\nclone 0 129\nfree 0\nfree 1\nfree 2")
    assert [st["rc"] for st in out] == [0, 0, 1, 0, 2, 0, 0, 0]
    assert out[2]["seqs"]["1"]["pages"] == [0, 1, 3] and out[2]["seqs"]["1"]["pos"] == 128        # pos % 64 == 0: both whole pages shared
    assert out[4]["seqs"]["2"]["pages"] == [0, 4, 5] and out[4]["seqs"]["2"]["pos"] == 100        # pos % 64 != 0: the partial page is its own
    assert out[4]["ref"][:6] == [3, 2, 1, 1, 1, 1] and same_table(out[-1], initial(8))


def test_open_many_opens_all_or_none_and_otherwise_what_single_opens_give():
    """SeqTable::open_many (gvl_seq_fanout's siblings, the searches' candidates): pages and slots are counted before the first clone opens"""
    head = "alloc 129\npos 0 100\n"                                                        # 3 pages, 1 whole; a clone of 129 tokens owns 2
    assert rcs(head + "openmany 0 3 129", pages=8) == [0, 0, NO_PAGES]                       # 5 free, 6 needed: one page too few, nothing opened (run() checks the table)
    assert rcs(head + "openmany 0 3 129", pages=9, max_seqs=3) == [0, 0, TOO_MANY]            # pages for three, slots for two
    assert rcs(head + "alloc 64\nfree 1\nopenmany 0 3 129", pages=9, max_seqs=4) == [0, 0, 1, 0, 0]    # a freed slot counts
    assert rcs(head + "openmany 0 0 129\nopenmany 0 2 100\nopenmany 1 2 129\nopenmany -1 2 129", pages=9) == [0, 0, BAD, BAD, BAD, BAD]
    many = run(head + "openmany 0 3 129", pages=9)[-1]
    single = run(head + "clone 0 129\nclone 0 129\nclone 0 129", pages=9)[-1]
    assert many["rc"] == 0 and single["rc"] == 3
    assert {k: v for k, v in many.items() if k != "rc"} == {k: v for k, v in single.items() if k != "rc"}      # the same slots, pages, counts and free list, to the bit
    assert [many["seqs"][k]["pages"] for k in "123"] == [[0, 3, 4], [0, 5, 6], [0, 7, 8]] and many["free"] == []


def test_pages_of_reports_a_sequences_pages_and_refuses_the_rest():
    """SeqTable::pages_of, the body of gvl_debug_seq_pages: the count, the first min(cap, count) pages, nothing behind them; unknown / freed sequences and a negative
    cap are refused with nothing written; a null count and a null buffer with cap 0 are fine"""
    out = run("alloc 129\npos 0 100\nfork 0 64 200\npages 1 64 -1\npages 1 64 0\npages 1 64 1\npages 1 64 3\npages 1 64 4\npages 1 2 -1\npages 1 2 1\npages 1 2 2\n"
              "pages 1 0 -1\npages 1 0 0\npages 1 -2 -1\npagesnull 1 64 -1\npagesnull 1 64 3\npagesnull 1 -2 0\n"
              "pages 1 -1 -1\npages 2 64 -1\npages -1 64 -1\npages 99 64 -1\nfree 1\npages 1 64 -1\npages 0 64 2\nfree 0")
    rc = [st["rc"] for st in out]
    assert out[2]["seqs"]["1"]["pages"] == [0, 3, 4, 5] and out[2]["seqs"]["0"]["pages"] == [0, 1, 2]
    assert rc[3:8] == [4, 0, 3, 5, -77], "cap >= count: the count, every page in position order, the word behind them untouched"
    assert rc[8:11] == [4, 3, -77], "cap < count: the count is still the whole count, cap pages are written and no more"
    assert rc[11:14] == [4, -77, 4], "cap 0: only the count, with or without a buffer"
    assert rc[14:17] == [-99, 5, -77], "a null count: the pages alone; with a null buffer too, nothing at all"
    assert rc[17:21] == [BAD] * 4 and rc[22] == BAD, "cap < 0, a slot never opened, ids outside the table, a freed sequence"
    assert rc[23] == 2 and same_table(out[-1], initial(8))


def test_bad_sources():
    assert rcs("fork 0 64 128\nclone 0 64\nalloc 64\nfree 0\nfork 0 64 128\nclone 0 64\nfork -1 64 128\nfree 0\nfree -1\nfree 7") == [BAD, BAD, 0, 0, BAD, BAD, BAD, BAD, BAD, BAD]
    assert rcs("alloc 64\nfork 0 128 192\nfork 0 64 64\nfork 0 -64 64") == [0, BAD, BAD, BAD]         # more shared pages than the source holds; no room beyond the prefix


def test_alloc_takes_the_default_and_fork_and_clone_take_the_sources_settings():
    out = run("""newrules
                 newrules
                 rules -1 0
                 topn -1 3
                 proc -1 1.5 2 4 7
                 alloc 65
                 alloc 65
                 rules 1 1
                 topn 1 8
                 proc 1 0.5 3 0 -1
                 pos 1 65
                 fork 1 64 129
                 rules -1 -1
                 clone 2 130
                 clone 3 131
                 alloc 1""", pages=16, max_seqs=8)
    assert [st["rc"] for st in out] == [0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 2, 0, 3, 4, 5]
    last = out[-1]
    assert last["seqs"]["0"]["sel"] == [1.5, 2, 4, 7, 3, 0] and last["seqs"]["5"]["sel"] == [1.5, 2, 4, 7, 3, -1]      # the default at the time of the alloc
    mine = [0.5, 3, 0, -1, 8, 1]
    # the source was the LAST slot each time and the table grew (2 -> 3 and 4 -> 5 slots reallocate): its settings and pages were read before that
    assert out[11]["slots"] == 3 and out[14]["slots"] == 5
    assert [last["seqs"][k]["sel"] for k in "1234"] == [mine] * 4
    assert len({last["seqs"][k]["pages"][0] for k in "1234"}) == 1 and last["ref"][last["seqs"]["1"]["pages"][0]] == 4
    assert last["rules"] == {"0": 1, "1": 4} and last["default"] == [1.5, 2, 4, 7, 3, -1]


def test_rule_set_lifetime():
    out = run("""newrules
                 rules -1 0
                 delrules 0
                 alloc 1
                 rules -1 -1
                 delrules 0
                 rules 0 0
                 free 0
                 delrules 0
                 delrules 0
                 delrules -1
                 delrules 9
                 rules -1 0
                 rules -1 9
                 rules -1 -2
                 alloc 1
                 rules 0 3
                 rules 5 -1
                 newrules
                 newrules
                 newrules
                 newrules
                 delrules 1
                 newrules""")
    assert [st["rc"] for st in out] == [0, 0, RULES_BUSY, 0, 0, RULES_BUSY, 0, 0, 0, NO_RULES, NO_RULES, NO_RULES, NO_RULES, NO_RULES, NO_RULES,
                                        0, NO_RULES, BAD, 0, 1, 2, RULES_FULL, 0, 1]
    assert out[1]["rules"] == {"0": 1} and out[3]["rules"] == {"0": 2} and out[6]["rules"] == {"0": 1}      # setting the set a holder already has keeps its count
    assert out[8]["rules"] == {} and out[-1]["rules"] == {"0": 0, "1": 0, "2": 0}


def test_live_and_group_checks():
    assert rcs("alloc 1\nalloc 1\nalloc 1\nfree 1\nlive 0\nlive 1\nlive -1\nlive 3\ngroup 0 2\ngroup 0 2 0\ngroup 0 1 0\ngroup 2 2\ngroup\ngroup 7") == \
        [0, 1, 2, 0, 0, BAD, BAD, BAD, 0, DUPLICATE, BAD, DUPLICATE, 0, BAD]


# ---- seeded random operations against a model ------------------------------------------------------------------------------------
class Model:
    def __init__(self, pages, max_seqs, max_rules):
        self.st, self.max_seqs, self.max_rules = initial(pages), max_seqs, max_rules

    def open(self, mx, src, pos):
        st, shared, n = self.st, pos >> 6, (mx + 63) // 64
        if pos < 0 or mx <= pos or (pos != 0 if src < 0 else (str(src) not in st["seqs"] or shared > len(st["seqs"][str(src)]["pages"]))):
            return BAD
        if len(st["free"]) < n - shared:
            return NO_PAGES
        i = next(i for i in itertools.count() if str(i) not in st["seqs"])
        if i >= self.max_seqs:
            return TOO_MANY
        sel = list(st["seqs"][str(src)]["sel"] if src >= 0 else st["default"])
        pages = list(st["seqs"][str(src)]["pages"][:shared]) if src >= 0 else []
        pages += [st["free"].pop() for _ in range(n - shared)]
        for p in pages:
            st["ref"][p] += 1
        if sel[5] >= 0:
            st["rules"][str(sel[5])] += 1
        st["seqs"][str(i)] = {"max": mx, "n_pages": n, "pos": pos, "n_gen": 0, "pages": pages, "sel": sel}
        st["slots"], st["any_live"] = max(st["slots"], i + 1), 1
        return i

    def sel_of(self, seq):
        return self.st["default"] if seq == -1 else self.st["seqs"].get(str(seq), {}).get("sel")

    def apply(self, op, *a):
        st = self.st
        if op == "alloc":
            return self.open(a[0], -1, 0)
        if op == "fork":
            return self.open(a[2], a[0], a[1])
        if op == "clone":
            return self.open(a[1], a[0], st["seqs"][str(a[0])]["pos"] if str(a[0]) in st["seqs"] else 0)
        if op == "openmany":
            src = st["seqs"].get(str(a[0]))
            if src is None or a[1] < 1 or a[2] <= src["pos"]:
                return BAD
            if len(st["free"]) < a[1] * ((a[2] + 63) // 64 - (src["pos"] >> 6)):
                return NO_PAGES
            if self.max_seqs - len(st["seqs"]) < a[1]:
                return TOO_MANY
            for _ in range(a[1]):
                assert self.open(a[2], a[0], src["pos"]) >= 0
            return 0
        if op == "free":
            s = st["seqs"].pop(str(a[0]), None)
            if s is None:
                return BAD
            for p in s["pages"]:
                st["ref"][p] -= 1
                if st["ref"][p] == 0:
                    st["free"].append(p)
            if s["sel"][5] >= 0:
                st["rules"][str(s["sel"][5])] -= 1
            st["any_live"] = int(bool(st["seqs"]))
            return 0
        if op == "newrules":
            i = next(i for i in itertools.count() if str(i) not in st["rules"])
            if i >= self.max_rules:
                return RULES_FULL
            st["rules"][str(i)] = 0
            return i
        if op == "delrules":
            if a[0] < 0 or str(a[0]) not in st["rules"]:
                return NO_RULES
            if st["rules"][str(a[0])] > 0:
                return RULES_BUSY
            del st["rules"][str(a[0])]
            return 0
        if op == "pos":
            if str(a[0]) not in st["seqs"]:
                return BAD
            st["seqs"][str(a[0])]["pos"] = a[1]
            return 0
        sel = self.sel_of(a[0])                          # rules / topn / proc
        if sel is None:
            return BAD
        if op == "rules":
            if a[1] != -1 and str(a[1]) not in st["rules"]:
                return NO_RULES
            if a[1] >= 0:
                st["rules"][str(a[1])] += 1
            if sel[5] >= 0:
                st["rules"][str(sel[5])] -= 1
            sel[5] = a[1]
        elif op == "topn":
            sel[4] = a[1]
        else:
            sel[0:4] = a[1:5]
        return 0


def random_ops(rng, n, max_seqs, max_rules):
    ops = []
    seq = lambda: rng.randrange(-1, max_seqs + 1)        # noqa: E731  (-1 and max_seqs are never live: refusals are part of the mix)
    for _ in range(n):
        k = rng.random()
        if k < 0.22:
            ops.append(("alloc", rng.choice(LENGTHS + (200,))))
        elif k < 0.34:
            ops.append(("fork", seq(), rng.choice((64, 64, 128, 192, 0)), rng.choice((65, 128, 129, 200, 64))))
        elif k < 0.41:
            ops.append(("clone", seq(), rng.choice((65, 129, 200, 256))))
        elif k < 0.44:
            ops.append(("openmany", seq(), rng.randrange(0, 4), rng.choice((65, 129, 200, 256))))
        elif k < 0.52:
            ops.append(("pos", max(seq(), 0), rng.choice((0, 1, 63, 64, 65, 100, 128, 129))))
        elif k < 0.74:
            ops.append(("free", seq()))
        elif k < 0.79:
            ops.append(("newrules",))
        elif k < 0.85:
            ops.append(("delrules", rng.randrange(-1, max_rules + 1)))
        elif k < 0.93:
            ops.append(("rules", seq(), rng.randrange(-2, max_rules + 1)))
        elif k < 0.96:
            ops.append(("topn", seq(), rng.randrange(-1, 9)))
        else:
            ops.append(("proc", seq(), rng.choice((1.0, 1.5, 0.5, 2.0)), rng.randrange(0, 4), rng.randrange(0, 5), rng.randrange(-1, 9)))
    return ops


def test_random_operations_match_the_model():
    pages, max_seqs, max_rules = 8, 5, 3
    rng = random.Random(20240607)
    ops = random_ops(rng, 4000, max_seqs, max_rules)
    # then everything goes: the sequences, the default's rule set, the rule sets
    ops += [("free", i) for i in range(max_seqs)] + [("rules", -1, -1)] + [("delrules", i) for i in range(max_rules)] + [("topn", -1, -1), ("proc", -1, 1.0, 0, 0, -1)]
    out = run("\n".join(" ".join(str(x) for x in op) for op in ops), pages, max_seqs, max_rules)
    m = Model(pages, max_seqs, max_rules)
    seen = set()
    for op, st in zip(ops, out):
        rc = m.apply(*op)
        assert dict(m.st, rc=rc) == st, op
        seen.add((op[0], min(rc, 0)))
    # the mix reached every limit and every refusal
    assert {("alloc", NO_PAGES), ("alloc", TOO_MANY), ("fork", NO_PAGES), ("fork", TOO_MANY), ("fork", BAD), ("fork", 0), ("clone", NO_PAGES), ("clone", TOO_MANY),
            ("clone", BAD), ("clone", 0), ("openmany", NO_PAGES), ("openmany", TOO_MANY), ("openmany", BAD), ("openmany", 0), ("free", BAD), ("newrules", RULES_FULL), ("delrules", RULES_BUSY), ("delrules", NO_RULES), ("delrules", 0),
            ("rules", NO_RULES), ("rules", BAD), ("rules", 0)} <= seen
    assert same_table(out[-1], initial(pages))
