"""Records what the sequence entries refuse and admit: runs tests/entry_cases.py against whichever libgvl.so is built (GVL_LIB_PATH picks another build) and writes
tests/golden/entry_refusals.json -- per case the set-up, the call, the status and the text behind `failed (status N): `.  The committed file was recorded on the commit
before the entries took their refusals from csrc/gvl_admit.h; tests/test_gpu_entry_refusals.py and tests/test_admit_cpu.py hold the code to it.
    python tools/make_entry_refusals.py [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _gvl_bootstrap  # noqa: E402,F401
import entry_cases as EC  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "entry_refusals.json"))
args = ap.parse_args()

eng = EC.make_engine()
rows = []


def on_case(i, setup, call, status, text, before, after):
    assert before == after, f"case {i} {call}: a refused call changed the pool or a sequence"
    rows.append({"setup": setup, "call": list(call), "status": status, "text": text})


EC.Runner(eng).replay(on_case)
eng.close()
with open(args.out, "w") as f:
    f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
print(f"{len(rows)} cases ({sum(r['status'] == 0 for r in rows)} admitted) -> {args.out}")
