"""-m gpu: what the sequence entries refuse and admit, through the raw ABI.  tests/entry_cases.py lists the calls -- the ten prefill / decode entries, the three searches,
gvl_seq_fork / gvl_seq_clone / gvl_seq_fanout on every sequence state, the length edges, two faults in one call, one page or one slot too few --;
tests/golden/entry_refusals.json holds the status and the whole message each call got on the commit before the entries took their refusals from csrc/gvl_admit.h
(tools/make_entry_refusals.py).  Every call must get exactly that again, and a refused call leaves the pool and every sequence it named as they were: kv_info, their
pages, their generated ids.  One engine, no kernel beyond the set-up's tiny prefills and the admitted calls."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

from gpu_util import DEV  # noqa: E402,F401
import entry_cases as EC  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entry_refusals.json")


def test_every_entry_refuses_and_admits_what_it_did_and_a_refusal_changes_nothing():
    with open(GOLDEN) as f:
        want = json.load(f)
    listed = EC.cases()
    assert [(w["setup"], w["call"]) for w in want] == [(s, json.loads(json.dumps(list(c)))) for s, c in listed], "the golden file is not a recording of tests/entry_cases.py"
    eng = EC.make_engine()
    wrong = []

    def on_case(i, setup, call, status, text, before, after):
        w = want[i]
        if (status, text) != (w["status"], w["text"]):
            wrong.append((setup, call, (status, text), (w["status"], w["text"])))
        assert before == after, f"{setup} {call}: a refused call changed the pool or a sequence it named"

    try:
        EC.Runner(eng).replay(on_case)
    finally:
        eng.close()
    for x in wrong:
        print("setup %s, call %s: got %s, recorded %s" % x)
    assert not wrong, f"{len(wrong)} of {len(want)} calls differ from the recording"
    assert sum(w["status"] == 0 for w in want) >= 60 and sum(w["status"] != 0 for w in want) >= 250      # the list has both kinds
