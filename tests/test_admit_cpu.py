"""The admission check of the sequence entries (csrc/gvl_admit.h: one table, one function over the sequence table) on the CPU: tests/c/admit_check.cc includes that
header alone, is built with the host C++ compiler (so the header needs no HIP) and replays a script of table operations and admit() calls.

* Every case of tests/golden/entry_refusals.json -- recorded on a GPU from the entries as they were before they shared this function -- is replayed: its set-up
  (tests/entry_cases.py) becomes a script, its call an admit() line, and the verdict must be the recorded status and text.  The few refusals the entries keep to
  themselves (a count out of range) are restated here; gvl_seq_fork and gvl_seq_fanout do not go through admit() and are left to the GPU replay.
* Beyond the recording: every entry on every state -- the recorded ones and ones no public call can build (a bank out of step, a bank without room, a source with a
  grammar and more ids than a list holds) -- with every number of a list of edges, against ROWS below: the table written out once more, by hand, in Python.  A call
  with two faults gets the check that stands first in the entry's order."""
import atexit
import functools
import itertools
import json
import os
import shutil
import subprocess
import tempfile

import entry_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grounded-video-llm_amd", "csrc")
ARG, STATE, OOM = -1, -2, -4
ENTRIES = ["prefill", "prefill_extend", "forward_loss", "prefill_varlen", "prefill_extend_varlen", "score_extend_varlen", "decode_greedy_batch", "decode_steps",
           "decode_step_logits", "decode_step_logits_batch", "seq_clone", "seq_clone_plain", "search", "search_hidden"]           # gvl_admit::Entry, in its order
STRIDE = {"prefill": 0, "prefill_extend": 0, "forward_loss": 0, "prefill_varlen": 1, "prefill_extend_varlen": 1, "score_extend_varlen": 1, "decode_greedy_batch": -1,
          "decode_steps": 0, "decode_step_logits": 0, "decode_step_logits_batch": 1, "seq_clone": 0, "seq_clone_plain": 0, "search": -1, "search_hidden": -1}
LIMITS = dict(max_prefill=EC.GEO["max_prefill"], max_seq=EC.GEO["max_seq"], outlist_cap=EC.OUTLIST_CAP, vocab=EC.VOCAB)


@functools.lru_cache(maxsize=None)
def checker():
    tmp = tempfile.mkdtemp(prefix="gvl_admit_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "admit_check")
    cmd = ["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", CSRC, os.path.join(ROOT, "tests", "c", "admit_check.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run(lines, pages=EC.GEO["kv_pages"], max_seqs=EC.MAX_SEQS, **lim):
    """-> [(rc, message)] per script line"""
    lim = dict(LIMITS, **lim)
    r = subprocess.run([checker(), str(pages), str(max_seqs)] + [str(lim[k]) for k in ("max_prefill", "max_seq", "outlist_cap", "vocab")],
                       input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = [ln.split("\t", 1) for ln in r.stdout.split("\n")[:-1]]
    assert len(out) == len(lines)
    return [(int(rc), msg) for rc, msg in out]


def setup_script(name):
    word = {"alloc": "open", "prefill": "prefilled", "fork": "fork", "guide": "pair", "keep_hidden": "bank", "free": "free", "fill_pages": "fill_pages", "fill_slots": "fill_slots"}
    return [" ".join([word[op]] + [str(x) for x in a]) for op, *a in EC.SETUPS[name]]


def admit_line(entry, ids, xs=None, fn="-"):
    return " ".join(str(x) for x in ["admit", ENTRIES.index(entry), fn, STRIDE[entry], len(ids)] + list(ids) + ([] if STRIDE[entry] < 0 else list(xs)))


def test_the_setup_opens_the_slots_the_cases_name():
    out = run(setup_script("base"))
    opened = [rc for (op, *_), (rc, _) in zip(EC.SETUP, out) if op in ("alloc", "fork")]
    assert opened == list(range(16)) and all(rc >= 0 for rc, _ in out)
    assert {k: v for k, v in EC.NAMES.items() if v in opened} == dict(empty=0, p64=1, p70=2, fork64=3, lead=4, foll=5, kh_empty=6, kh_pre=7, empty2=8, p64b=9, fork64b=10, p8=11,
                                                                      e64=12, fork_small=13, full=14, freed=15)


# ---- the recording -----------------------------------------------------------------------------------------------------------------------------------------
def entry_side(fn, call):
    """the refusal an entry raises itself, in front of admit(): a count out of range"""
    if fn == "decode_greedy_batch" and not 0 < call[2] <= EC.OUTLIST_CAP:
        return ARG, "gvl_decode_greedy_batch: bad arguments"
    if fn == "decode_steps" and call[2] <= 0:
        return ARG, "gvl_decode_steps: bad arguments"
    return None


def test_every_recorded_case_gets_its_recorded_verdict_from_the_pure_function():
    with open(os.path.join(ROOT, "tests", "golden", "entry_refusals.json")) as f:
        golden = json.load(f)
    assert [(g["setup"], g["call"]) for g in golden] == [(s, json.loads(json.dumps(list(c)))) for s, c in EC.cases()]
    checked, left_out = 0, set()
    for setup, group in itertools.groupby(golden, key=lambda g: g["setup"]):
        lines, want = setup_script(setup), []
        n_setup = len(lines)
        for g in group:
            fn, call = g["call"][0], g["call"]
            ids = [EC.NAMES[s] for s in (call[1] if isinstance(call[1], list) else [call[1]])]
            if fn in ("seq_fork", "seq_fanout"):
                left_out.add(fn)
                continue
            if entry_side(fn, call):
                assert (g["status"], g["text"]) == entry_side(fn, call), g
                continue
            if fn in EC.SEARCHES:
                hidden = fn == "contrastive_search"
                lines.append(admit_line("search_hidden" if hidden else "search", ids, fn="gvl_" + fn))
                if setup != "base" and hidden:          # the search's own opens behind an admitted call: the root clone, then top_k - 1 candidates at once, all or nothing
                    want.append((0, ""))
                    cap = min(20 + 2 + 1, EC.GEO["max_seq"])
                    lines += [admit_line("seq_clone_plain", ids, [cap]), f"fork {ids[0]} 20 {cap}", f"open_many {ids[0]} 3 {cap}"]
                    want += [(0, ""), None, ({"pages_free_3": -3, "slots_free_3": -4}[setup], "")]
                    lines.append(f"refusal gvl_seq_clone {want[-1][0]}")
            else:
                xs = call[2] if isinstance(call[2], list) else [call[2]]
                lines.append(admit_line(fn, ids, xs))
            want.append((g["status"], g["text"]))
        out = run(lines)
        assert all(rc >= 0 for rc, _ in out[:n_setup])
        for ln, got, w in zip(lines[n_setup:], out[n_setup:], want):
            assert w is None or got == w, (setup, ln, got, w)
            checked += 1
    assert left_out == {"seq_fork", "seq_fanout"} and checked >= 290


# ---- the table once more, by hand ------------------------------------------------------------------------------------------------------------------------
HOLDS, BADLEN, FIRST, STEP = "sequence already holds tokens", "bad length", "call gvl_prefill first", "bad token / sequence full / not prefilled"
WHOLE = "every sequence must be empty or hold a prefix of whole pages (gvl_seq_fork)"
COPY = "the source must hold tokens and max_tokens must exceed them (and fit cfg.max_seq)"
# entry: (prefix, text for no live sequence, pair: any / follower / both, bank, position, number, number first, duplicates, (status, text) of the position,
#         text of the number (None: the position's), text for x > max_prefill (None: the number's), prefix of the position's message (None: the entry's))
ROWS = {
    "prefill": ("gvl_prefill", "bad seq", "any", "allowed", "empty", "rows", True, False, (STATE, HOLDS), BADLEN, None, None),
    "prefill_extend": ("gvl_prefill_extend", "bad seq", "follower", "refused", "whole_prefix", "rows", False, False,
                       (STATE, "the sequence must hold a prefix of whole pages (gvl_seq_fork)"), BADLEN, None, None),
    "forward_loss": ("gvl_forward_loss", "bad seq", "any", "refused", "empty", "rows", True, False, (STATE, HOLDS), "bad arguments / length", None, None),
    "prefill_varlen": ("gvl_prefill_varlen", "bad seq / embeds", "any", "refused", "empty", "rows", True, True, (STATE, HOLDS), BADLEN, "seq_len exceeds cfg.max_prefill", None),
    "prefill_extend_varlen": ("gvl_prefill_extend_varlen", "bad seq / embeds", "follower", "refused", "empty_or_whole", "rows", False, True, (STATE, WHOLE), BADLEN, None, None),
    "score_extend_varlen": ("gvl_score_extend_varlen", "bad seq / embeds / next ids", "follower", "refused", "empty_or_whole", "rows", False, True, (STATE, WHOLE), BADLEN, None, None),
    "decode_greedy_batch": ("gvl_decode_greedy_batch", "bad seq", "follower", "refused", "generated", "none", False, True, (STATE, FIRST), None, None, "gvl_decode_greedy"),
    "decode_steps": ("gvl_decode_steps", "bad seq", "follower", "refused", "generated", "steps", False, True, (STATE, FIRST), "sequence would exceed its capacity", None, None),
    "decode_step_logits": ("gvl_decode_step_logits", "bad seq", "both", "in_step_room", "room_left", "token", False, False, (ARG, STEP), None, None, None),
    "decode_step_logits_batch": ("gvl_decode_step_logits_batch", "bad seq", "both", "in_step_room", "room_left", "token", False, True, (ARG, STEP), None, None, None),
    "seq_clone": ("gvl_seq_clone", "bad arguments", "both", "in_step", "prefilled", "copy_cap", False, False, (ARG, COPY), None, None, None),
    "seq_clone_plain": ("gvl_seq_clone", "bad arguments", "both", "allowed", "prefilled", "copy_cap", False, False, (ARG, COPY), None, None, None),
    "search": ("gvl_x_search", "bad seq", "both", "refused", "prefilled", "none", False, False, (STATE, "the sequence is not prefilled"), None, None, None),
    "search_hidden": ("gvl_x_search", "bad seq", "both", "required", "prefilled", "none", False, False, (STATE, "the sequence is not prefilled"), None, None, None),
}


def expect(entry, table, ids, xs, lim):
    """what ROWS says about members `ids` (table: id -> dict of the sequence's fields, absent: not live) -> (status, message)"""
    fn, bad, pair, bank, pos, num, num_first, dups, pos_fail, num_text, prefill_text, pos_fn = ROWS[entry]
    for i, sid in enumerate(ids):
        s = table.get(sid)
        if s is None:
            return ARG, f"{fn}: {bad}"
        if pair != "any" and s["lead"] >= 0:
            return STATE, f"{fn}: sequence {sid} follows guided leader {s['lead']}; name the leader"
        if pair == "both" and s["follow"] >= 0:
            return STATE, f"{fn}: sequence {sid} leads a guided pair (gvl_seq_set_guidance(seq, -1, ...) unbinds)"
        if bank == "refused" and s["cap"] > 0:
            return STATE, f"{fn}: sequence {sid} keeps its hidden states (gvl_seq_keep_hidden); this entry does not fill the bank"
        x = xs[i if STRIDE[entry] == 1 else 0] if STRIDE[entry] >= 0 else 0
        pos_ok = {"empty": s["pos"] == 0, "whole_prefix": s["pos"] > 0 and s["pos"] % 64 == 0, "empty_or_whole": s["pos"] % 64 == 0, "generated": s["ngen"] >= 1,
                  "room_left": 0 < s["pos"] < s["max"], "prefilled": s["pos"] > 0}[pos]
        faults = []                                          # of the number, in the entry's order
        if num == "rows":
            if x <= 0 or (0 if pos == "empty" else s["pos"]) + x > s["max"]:
                faults.append(num_text)
            if x > lim["max_prefill"]:
                faults.append(prefill_text or num_text)
        elif num == "steps" and (s["pos"] + x > s["max"] or s["ngen"] + x > lim["outlist_cap"]):
            faults.append(num_text)
        elif num == "token" and not 0 <= x < lim["vocab"]:
            faults.append(pos_fail[1])
        elif num == "copy_cap" and not s["pos"] < x <= lim["max_seq"]:
            faults.append(pos_fail[1])
        num_status = ARG if num_text else pos_fail[0]
        checks = [(num_status, fn, faults[0])] if faults else []
        if not pos_ok:
            checks.insert(len(checks) if num_first else 0, (pos_fail[0], pos_fn or fn, pos_fail[1]))
        if checks:
            return checks[0][0], f"{checks[0][1]}: {checks[0][2]}"
        if dups and sid in ids[:i]:
            return ARG, f"{fn}: duplicate seq"
        if bank == "required" and s["cap"] <= 0:
            return STATE, f"{fn}: the sequence keeps no hidden states (gvl_seq_keep_hidden before its prefill)"
        if bank == "in_step":
            if s["grammar"] and s["ngen"] > lim["outlist_cap"]:
                return STATE, f"{fn}: the source generated more ids than an output list holds"
            if s["cap"] > 0 and s["rows"] != s["pos"]:
                return STATE, f"{fn}: the source's hidden bank is not in step with its position"
        if (bank == "required" and s["rows"] != s["pos"]) or (bank == "in_step_room" and s["cap"] > 0 and (s["rows"] != s["pos"] or s["rows"] >= s["cap"])):
            return STATE, f"{fn}: the hidden bank is not in step with the sequence"
    return 0, ""


def product_states():
    """SETUP's table as a model, and behind it states that only the script can build -> (script lines, {id: fields})"""
    lines, table, nxt = setup_script("base"), {}, 0
    new = lambda mx, pos=0: dict(max=mx, pos=pos, ngen=0, lead=-1, follow=-1, cap=0, rows=0, grammar=False)   # noqa: E731
    for op, *a in EC.SETUP:
        if op in ("alloc", "fork"):
            table[nxt] = new(a[0]) if op == "alloc" else new(a[2], a[1])
            nxt += 1
        elif op == "prefill":
            table[a[0]].update(pos=a[1], ngen=1, rows=a[1] if table[a[0]]["cap"] else 0)
        elif op == "keep_hidden":
            table[a[0]].update(cap=table[a[0]]["max"])
        elif op == "guide":
            table[a[0]]["follow"], table[a[1]]["lead"] = a[1], a[0]
        elif op == "free":
            del table[a[0]]
    extra = [("bank behind its position", dict(max=128, pos=20, ngen=1, cap=128, rows=19)), ("bank without room", dict(max=64, pos=64, ngen=1, cap=64, rows=64)),
             ("bank in step at the last row", dict(max=64, pos=63, ngen=1, cap=64, rows=63)), ("grammar, more ids than a list holds", dict(max=300, pos=200, ngen=40, grammar=True)),
             ("grammar, ids that fit", dict(max=300, pos=200, ngen=16, grammar=True)), ("bank out of step and a grammar with too many ids", dict(max=300, pos=200, ngen=40, grammar=True, cap=300, rows=7)),
             ("partial page, nothing generated", dict(max=256, pos=65, ngen=0)), ("many ids", dict(max=512, pos=100, ngen=30))]
    for _, f in extra:
        sid = 15 if 15 not in table else nxt        # the freed slot is taken first
        nxt += sid != 15
        table[sid] = dict(new(f["max"]), **f)
        lines.append(f"open {f['max']}")
        lines += [f"set {sid} {k} {f[v]}" for k, v in (("pos", "pos"), ("ngen", "ngen"), ("cap", "cap"), ("rows", "rows")) if v in f]
        if f.get("grammar"):
            lines.append(f"grammar {sid}")
    return lines, table


def test_every_entry_on_every_state_and_edge_follows_its_row_of_the_table():
    lim = dict(LIMITS, outlist_cap=32)                     # small enough for n_gen + n_steps and for a grammar's ids to reach it
    lines, table = product_states()
    n_setup = len(lines)
    states = sorted(table) + [15 if 15 not in table else 99, -1, 77, 300]
    assert 15 in table and 99 not in table
    edges = sorted({-1, 0, 1, 2, 8, 31, 32, 33, 56, 57, 58, 63, 64, 65, 99, 100, 128, 129, 186, 187, 192, 193, 236, 237, 256, 257, 300, 301, 412, 413, 512, 513, 2 ** 31 - 1})
    calls = []
    for entry in ENTRIES:
        xs_list = [[x] for x in edges] if STRIDE[entry] >= 0 else [[]]
        for sid in states:
            calls += [(entry, [sid], xs) for xs in xs_list]
        if STRIDE[entry] != 0 or entry == "decode_steps":            # the batch entries: a second member behind a good one, two faults, a duplicate
            good = {"prefill_varlen": 8, "prefill_extend_varlen": 10, "score_extend_varlen": 10}.get(entry, 9)
            for sid in states + [good]:
                for x in (edges if STRIDE[entry] >= 0 else [0]):
                    calls.append((entry, [good, sid], [5, x] if STRIDE[entry] == 1 else [x]))
            calls += [(entry, [4, 4], [0, 0][:max(STRIDE[entry], 0) + 1]), (entry, [5, 5, 5], [1, 1, 1][:2 * max(STRIDE[entry], 0) + 1]), (entry, [77, 77], [1, 1][:max(STRIDE[entry], 0) + 1])]
    fn = lambda e: "gvl_x_search" if e.startswith("search") else "-"   # noqa: E731
    out = run(lines + [admit_line(e, ids, xs, fn(e)) for e, ids, xs in calls], **lim)
    assert all(rc >= 0 for rc, _ in out[:n_setup])
    seen = set()
    for (e, ids, xs), got in zip(calls, out[n_setup:]):
        want = expect(e, table, ids, xs, lim)
        assert got == want, (e, ids, xs, got, want)
        seen.add((e, got[1].split(": ", 1)[-1].split(" ")[0] if got[0] else "admitted"))
    assert len(calls) > 5000
    # every entry was admitted and refused, and every kind of refusal was reached
    for e in ENTRIES:
        assert (e, "admitted") in seen and len([s for s in seen if s[0] == e]) >= 3, e
    texts = {got[1] for got in out[n_setup:]}
    for part in ("not in step with the sequence", "not in step with its position", "more ids than an output list holds", "keeps no hidden states", "seq_len exceeds cfg.max_prefill",
                 "would exceed its capacity", "gvl_decode_greedy: call gvl_prefill first", "duplicate seq", "leads a guided pair", "follows guided leader"):
        assert any(part in t for t in texts), part


def test_two_faults_get_the_check_that_stands_first():
    lines, _ = product_states()
    n = len(lines)
    cases = [
        (admit_line("prefill", [1], [0]), "gvl_prefill: bad length"),                                  # length in front of the position for the entries of empty sequences
        (admit_line("prefill_extend", [2], [0]), "gvl_prefill_extend: the sequence must hold a prefix of whole pages (gvl_seq_fork)"),   # the other way round behind a prefix
        (admit_line("prefill_extend", [5], [0]), "gvl_prefill_extend: sequence 5 follows guided leader 4; name the leader"),
        (admit_line("prefill_varlen", [6], [0]), "gvl_prefill_varlen: sequence 6 keeps its hidden states (gvl_seq_keep_hidden); this entry does not fill the bank"),
        (admit_line("prefill_varlen", [0], [300]), "gvl_prefill_varlen: bad length"),                   # the capacity in front of max_prefill
        (admit_line("prefill_varlen", [0], [129]), "gvl_prefill_varlen: seq_len exceeds cfg.max_prefill"),
        (admit_line("prefill_varlen", [8, 8], [8, 0]), "gvl_prefill_varlen: bad length"),               # a member's own faults in front of "duplicate"
        (admit_line("prefill_varlen", [77, 0], [0, 0]), "gvl_prefill_varlen: bad seq / embeds"),        # members in call order
        (admit_line("decode_steps", [9, 5], [0]), "gvl_decode_steps: sequence 5 follows guided leader 4; name the leader"),
        (admit_line("decode_steps", [3], [600]), "gvl_decode_steps: call gvl_prefill first"),
        (admit_line("decode_step_logits_batch", [7, 7], [5, 5]), "gvl_decode_step_logits_batch: duplicate seq"),   # "duplicate" in front of the bank's state
        (admit_line("decode_step_logits", [15], [100]), "gvl_decode_step_logits: bad token / sequence full / not prefilled"),   # slot 15: the bank behind its position
        (admit_line("decode_step_logits", [15], [5]), "gvl_decode_step_logits: the hidden bank is not in step with the sequence"),
        (admit_line("seq_clone", [20], [513]), "gvl_seq_clone: " + COPY),                               # slot 20: bank out of step and too many ids
        (admit_line("seq_clone", [20], [400]), "gvl_seq_clone: the source generated more ids than an output list holds"),
        (admit_line("search_hidden", [0], fn="gvl_contrastive_search"), "gvl_contrastive_search: the sequence is not prefilled"),   # "not prefilled" in front of "keeps no hidden states"
        (admit_line("search_hidden", [1], fn="gvl_contrastive_search"), "gvl_contrastive_search: the sequence keeps no hidden states (gvl_seq_keep_hidden before its prefill)"),
        (admit_line("search", [7], fn="gvl_beam_search"), "gvl_beam_search: sequence 7 keeps its hidden states (gvl_seq_keep_hidden); this entry does not fill the bank"),
    ]
    out = run(lines + [c for c, _ in cases], outlist_cap=32)
    for (ln, want), got in zip(cases, out[n:]):
        assert got[1] == want and got[0] < 0, (ln, got, want)
