"""Records what the six descriptor entries of the operator level refuse and admit: runs tests/op_cases.py against whichever libgvl.so is built (GVL_LIB_PATH picks another
build) and writes tests/golden/op_refusals.json -- per case the entry, the name, the descriptor's fields (a pointer as null or set with its low four address bits), the
host copies of the arrays the entry reads back, the status and the text behind `failed (status N): `.  The committed file was recorded on the commit before the entries
took their refusals from csrc/gvl_op_check.h; tests/test_gpu_op_refusals.py and tests/test_op_check_cpu.py hold the code to it.
    python tools/make_op_refusals.py [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _gvl_bootstrap  # noqa: E402,F401
import op_cases as OC  # noqa: E402
from gpu_util import tiny_geo  # noqa: E402
from grounded_video_llm_amd import engine as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "op_refusals.json"))
args = ap.parse_args()

eng = E.Engine(tiny_geo(), OC.DEV, towers=())
rows = []


def on_case(i, entry, name, fields, host, status, text, untouched):
    assert untouched is not False, f"case {i} {entry} {name}: a refused call wrote to an output"
    rows.append({"entry": entry, "name": name, "fields": fields, "host": host, "status": status, "text": text})


OC.replay(eng, on_case)
eng.close()
with open(args.out, "w") as f:
    f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
print(f"{len(rows)} cases ({sum(r['status'] == 0 for r in rows)} admitted) -> {args.out}")
