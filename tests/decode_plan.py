"""Which launches one decode step takes and what each projection reads: a thin wrapper over tests/c/decode_plan_dump.cc, i.e. over the library's own decision functions
(csrc/gvl_decode_plan.h: host-only, no GPU).  Used by tests/test_decode_plan_cpu.py (recorded decisions) and by the GPU tests of the decode forms: the batched forms are
bit-identical and the fused-RMSNorm form differs in rounding only, so only the plan can say which launches a step took.

  step           the plan of one decode_step (gvl_llm.hip), or its refusal
  of_geometry    the same for a model built from an engine.TowerGeometry
  parts          the step sizes n waiting sequences are cut into
  mfma_ok / quant_ok / rs_ok / batch_ok / group_size    the predicates
  profiled       what the library itself counted: the GEMV, decode-attention and other launches of a call (gvl_prof_enable / gvl_prof_read)"""
import functools
import os
import subprocess
import tempfile
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grounded-video-llm_amd", "csrc")

QKV0, QKV, O_PROJ, GATE_UP, DOWN, HEAD = range(6)            # DecodeProj (gvl_decode_plan.h)
KIND_NAMES = ("qkv0", "qkv", "o", "gate_up", "down", "head")
GEMV, DGEMM = 0, 1                                           # DecodeLauncher
LAUNCHER_NAMES = ("gvl_launch_gemv", "gvl_launch_dgemm")
ROW_MAJOR, TILED, TILED_FOLDED = range(3)                    # DecodeWeight
WEIGHT_NAMES = ("row_major", "tiled", "tiled_folded")
X_NORM, XN, XT_SQ, ATTN, ACT = range(5)                      # DecodeInput
BAD_BATCH = -1
MAX_BATCH, MAX_VALU_BATCH = 16, 4                            # GVL_MAX_DECODE_BATCH, GVL_MAX_VALU_BATCH
PROF_GEMV, PROF_DECODE_ATTN, PROF_OTHER = 2, 3, 4            # include/gvl.h

Proj = namedtuple("Proj", "launcher weight scales input sq_out out_tiled")
Plan = namedtuple("Plan", "embed_norm attn_out_tiled norm_launches n_gemv n_attn n_other proj")


@functools.lru_cache(maxsize=None)
def dumper():
    exe = os.path.join(tempfile.mkdtemp(prefix="gvl_plan_"), "decode_plan_dump")
    cmd = ["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", CSRC, os.path.join(ROOT, "tests", "c", "decode_plan_dump.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@functools.lru_cache(maxsize=None)
def reasons():
    """refusal code -> the message decode_step fails with"""
    r = subprocess.run([dumper(), "reasons"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return {int(ln.split(" ", 1)[0]): ln.split(" ", 1)[1] for ln in r.stdout.splitlines()}


def plan_line(B, layers, hidden, mfma, fmt=0, folded=1, norm_fused=1):
    return f"P {B} {layers} {hidden} {int(mfma)} {fmt} {int(folded)} {int(norm_fused)}"


def parse(ln, g):
    t = [int(x) for x in g.split()]
    if ln[0] == "G":
        return tuple(t)
    if ln[0] != "P" or len(t) == 1:
        return t[0]                                          # a predicate, a size, or a refusal
    assert len(t) == 6 + 6 * 6, (ln, g)
    return Plan(*t[:6], tuple(Proj(*t[i:i + 6]) for i in range(6, 42, 6)))


def ask(lines):
    """case lines -> per line: a Plan, a refusal (negative int), a tuple of step sizes, or a predicate's 0 / 1"""
    r = subprocess.run([dumper()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(lines)
    return [parse(ln, g) for ln, g in zip(lines, got)]


@functools.lru_cache(maxsize=None)
def step(B, layers, hidden, mfma, fmt=0, folded=1, norm_fused=1):
    """the Plan of decode_step for B sequences (or its refusal): the geometry decode_plan reads, and the norm_fused knob of gvl_debug_set"""
    return ask([plan_line(B, layers, hidden, mfma, fmt, folded, norm_fused)])[0]


def parts(mfma, n):
    return ask([f"G {int(mfma)} {n}"])[0]


def mfma_ok(hidden, inter, heads, head_dim):
    return bool(ask([f"M {hidden} {inter} {heads} {head_dim}"])[0])


def quant_ok(fmt, hidden, inter, attn_width):
    return bool(ask([f"Q {fmt} {hidden} {inter} {attn_width}"])[0])


def rs_ok(mfma, fmt, norm_fused, folded, hidden):
    return bool(ask([f"R {int(mfma)} {fmt} {int(norm_fused)} {int(folded)} {hidden}"])[0])


def batch_ok(mfma, B):
    return bool(ask([f"A {int(mfma)} {B}"])[0])


def group_size(mfma, left):
    return ask([f"S {int(mfma)} {left}"])[0]


def of_geometry(geo, B, norm_fused=1):
    """step() for a model built from an engine.TowerGeometry as gvl_create / gvl_finalize_weights set it up: the path from decode_mfma_ok, the folded tile copies wherever
    the fused form could use them (MFMA path, bf16 decode weights, hidden % 64 == 0) -> (the path, the Plan)"""
    mfma = mfma_ok(geo.hidden, geo.inter, geo.heads, geo.hidden // geo.heads)
    fmt = int(getattr(geo, "decode_fp8", 0) or 0)
    return mfma, step(B, geo.layers, geo.hidden, mfma, fmt, int(mfma and not fmt and geo.hidden % 64 == 0), norm_fused)


def rs(p):
    """the fused-RMSNorm form: the consumers read the raw tile-order copy against the folded weights"""
    return p.proj[HEAD].input == XT_SQ


def profiled(eng, run):
    """run() with gvl_prof_enable on -> (its result, the GVL_PROF_GEMV launches it made, the GVL_PROF_DECODE_ATTN launches, the GVL_PROF_OTHER ones: per decode step
    the plan's n_other and one for token selection)"""
    eng.prof_enable(True)
    try:
        r = run()
        counts = tuple(eng.prof_read(cat)[1] for cat in (PROF_GEMV, PROF_DECODE_ATTN, PROF_OTHER))
    finally:
        eng.prof_enable(False)
    return (r,) + counts
