"""Which launches a prefill group takes, in which order: a thin wrapper over tests/c/prefill_plan_dump.cc, i.e. over the library's own decision function
(csrc/gvl_prefill_plan.h: host-only, no GPU).  Used by tests/test_prefill_plan_cpu.py (recorded decisions) and by the GPU tests of the prefill forms, which are bit-identical
by design: only the plan can say which launches a group took.

  group          the plan of one llm_prefill group (gvl_llm.hip) under gvl_debug_set varlen_attn / varlen_extend / last_layer_tail / norm_fused
  of_geometry    the same for a model built from an engine.TowerGeometry
  forms          its (post forms, attention forms), as names
  profiled_attn  what the library itself counted: the attention launches of a call (gvl_prof_enable / gvl_prof_read)"""
import functools
import os
import subprocess
import tempfile
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grounded-video-llm_amd", "csrc")

ONE, BATCHED, RAGGED, RAGGED_EXT = range(4)                 # PrefillForm (gvl_prefill_plan.h)
FORM_NAMES = ("ONE", "BATCHED", "RAGGED", "RAGGED_EXT")
POST, ATTN = 0, 1                                           # PrefillStepKind
LAST_STRIDED, LAST_GATHERED, LAST_TAIL = range(3)           # PrefillLastRows
BAD_BATCH, BAD_PREFIX, LOSS_BEHIND_PREFIX, LOSS_GROUP = -1, -2, -3, -4
MAX_BATCH = 8                                               # GVL_MAX_PREFILL_BATCH

# the case fields after the group (lens, pos0); the widths are a tiny model's whose fused RMSNorm is on and whose tail runs
DEFAULTS = dict(rope_orig_max_pos=0, long_table=0, loss=0, page_id_cap=256, hidden=256, qkv_width=192, gate_up_width=1024, fused_weights=1,
                varlen_attn=1, varlen_extend=1, last_layer_tail=1, norm_fused=1)

Step = namedtuple("Step", "kind form first count B S pos0 Sk use_long")
Plan = namedtuple("Plan", "M batched_table nf tail last_rows chunks steps")


@functools.lru_cache(maxsize=None)
def dumper():
    exe = os.path.join(tempfile.mkdtemp(prefix="gvl_plan_"), "prefill_plan_dump")
    cmd = ["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", CSRC, os.path.join(ROOT, "tests", "c", "prefill_plan_dump.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@functools.lru_cache(maxsize=None)
def reasons():
    """refusal code -> the message llm_prefill fails with"""
    r = subprocess.run([dumper(), "reasons"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return {int(ln.split(" ", 1)[0]): ln.split(" ", 1)[1] for ln in r.stdout.splitlines()}


def plan_line(lens, pos0=(), **kw):
    """nb = len(lens) (0 and 9 included: the plan refuses them); pos0 () = no prefixes"""
    c = dict(DEFAULTS, **kw)
    assert set(c) == set(DEFAULTS), sorted(set(c) - set(DEFAULTS))
    pad = lambda v: (list(v) + [0] * MAX_BATCH)[:MAX_BATCH]
    return f"P {len(lens)} " + " ".join(str(x) for x in pad(lens) + pad(pos0)) + " " + " ".join(str(int(c[f])) for f in DEFAULTS)


def group_line(lens, cap, max_rows):
    return f"G {len(lens)} {cap} {max_rows} " + " ".join(str(x) for x in lens)


def parse(ln, g):
    t = [int(x) for x in g.split()]
    if ln[0] == "G" or len(t) == 1:
        return t[0]                                         # a group's size, or a refusal
    nc = t[5]
    steps = t[7 + nc:]
    assert len(steps) == 9 * t[6 + nc], (ln, g)
    return Plan(t[0], t[1], t[2], t[3], t[4], tuple(t[6:6 + nc]), tuple(Step(*steps[i:i + 9]) for i in range(0, len(steps), 9)))


def plans(lines, exe=None):
    """case lines -> per line: a Plan, a refusal (negative int), or a group's size"""
    r = subprocess.run([exe or dumper()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    got = r.stdout.splitlines()
    assert len(got) == len(lines)
    return [parse(ln, g) for ln, g in zip(lines, got)]


@functools.lru_cache(maxsize=None)
def group(lens, pos0=(), **kw):
    """the Plan of llm_prefill for one group: lens / pos0 are tuples (new rows, tokens already held), kw the geometry and the gvl_debug_set knobs"""
    p = plans([plan_line(lens, pos0, **kw)])[0]
    assert isinstance(p, Plan), f"llm_prefill {lens} {pos0} {kw}: refused ({reasons()[p]})"
    return p


def of_geometry(geo, lens, pos0=(), **knobs):
    """group() for a model built from an engine.TowerGeometry: LongRoPE as the engine configures it (a long table exists when the geometry has long factors)"""
    long_table = geo.rope_long is not None
    return group(tuple(lens), tuple(pos0) if any(pos0) else (), rope_orig_max_pos=geo.rope_orig_max_pos if long_table else 0, long_table=int(long_table), **knobs)


def profiled_attn(eng, run):
    """run() with gvl_prof_enable on -> (its result, the attention launches it made, the work they were booked with)"""
    eng.prof_enable(True)
    try:
        r = run()
        _, launches, work = eng.prof_read(1)                # GVL_PROF_ATTN
    finally:
        eng.prof_enable(False)
    return r, launches, work


def forms(p):
    """(forms of the post launches, forms of the attention launches) of one layer, as names, in launch order"""
    return tuple(tuple(FORM_NAMES[s.form] for s in p.steps if s.kind == k) for k in (POST, ATTN))


def n_attn(p):
    return sum(s.kind == ATTN for s in p.steps)
