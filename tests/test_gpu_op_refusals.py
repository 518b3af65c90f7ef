"""-m gpu: what the six descriptor entries of the operator level refuse and admit.  tests/op_cases.py lists the calls -- per entry the refusals its own operator test
exercises and one admitted launch of each base case --; tests/golden/op_refusals.json holds the descriptor, the status and the whole message each call got on the commit
before the entries took their refusals from csrc/gvl_op_check.h (tools/make_op_refusals.py).  Every call must get exactly that again, from the same descriptor, and a
refused call leaves every output it names as it was.  One engine; the only kernels are the admitted launches, which the operator tests run too."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

from gpu_util import DEV, tiny_geo  # noqa: E402
from grounded_video_llm_amd import engine as E  # noqa: E402
import op_cases as OC  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "op_refusals.json")


def same_descriptor(got, want):
    """the pointers' low bits come from the allocator: whether a pointer is set and whether it is 16-byte aligned must agree, every other field exactly"""
    norm = lambda v: ({"set": v["set"] != 0} if isinstance(v, dict) else [norm(x) for x in v] if isinstance(v, list) else v)   # noqa: E731
    return {k: norm(v) for k, v in got.items()} == {k: norm(v) for k, v in want.items()}


def test_every_descriptor_entry_refuses_and_admits_what_it_did_and_a_refusal_writes_nothing():
    assert OC.DEV == DEV
    with open(GOLDEN) as f:
        want = json.load(f)
    eng = E.Engine(tiny_geo(), DEV, towers=())
    wrong, seen = [], []

    def on_case(i, entry, name, fields, host, status, text, untouched):
        assert i < len(want), "more cases than the golden file records"
        w = want[i]
        assert (entry, name) == (w["entry"], w["name"]) and same_descriptor(fields, w["fields"]) and host == w["host"], f"{entry} {name}: the golden file is not a recording of tests/op_cases.py"
        if (status, text) != (w["status"], w["text"]):
            wrong.append((entry, name, (status, text), (w["status"], w["text"])))
        assert untouched is not False, f"{entry} {name}: a refused call wrote to an output"
        seen.append(entry)

    try:
        OC.replay(eng, on_case)
    finally:
        eng.close()
    for x in wrong:
        print("%s, %s: got %s, recorded %s" % x)
    assert len(seen) == len(want) and not wrong, f"{len(wrong)} of {len(want)} calls differ from the recording"
    for e in OC.ENTRIES:                                   # every entry has both kinds
        assert any(w["entry"] == e and w["status"] == 0 for w in want) and sum(w["entry"] == e and w["status"] != 0 for w in want) >= 7, e
