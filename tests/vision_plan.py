"""Which launches a vision tower's call or the glue takes, in which order, in which workspace: a thin wrapper over tests/c/vision_plan_dump.cc, i.e. over the library's own
decision functions and walk (csrc/gvl_vision_plan.h: host-only, no GPU).  Used by tests/test_vision_plan_cpu.py (recorded launches), by tests/attn_plan.py (the operand path of
an attention launch) and by the GPU tests of the towers' forms, which are bit-identical or equal within tolerance by design: only the plan can say which launches a call took.

  tower          the TowerCall of clip_encode / iv2_encode for n items under gvl_debug_set patch_fused / vision_in_place / norm_fused / attn_pipe / attn_pipe_rows
  glue           the GlueCall of build_visual
  operand_path   vision_operand_path: where the attention kernel reads q, k and v
  fused_ok       patch_embed_fused_ok
  profiled       what the library itself counted: the GEMM, attention and other launches of a call (gvl_prof_enable / gvl_prof_read)"""
import functools
import os
import subprocess
import tempfile
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grounded-video-llm_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "vision_plan_dump.cc")

CLIP, IV2 = 0, 1                                            # VisionTower (gvl_vision_plan.h)
PROF_GEMM, PROF_ATTN, PROF_OTHER = 0, 1, 4                  # include/gvl.h
KNOBS = ("patch_fused", "vision_in_place", "norm_fused", "attn_pipe", "attn_pipe_rows")
KNOB_DEFAULTS = dict(patch_fused=1, vision_in_place=1, norm_fused=1, attn_pipe=1, attn_pipe_rows=128)

Path = namedtuple("Path", "vt_pages qk_rows q_on_load qkv_post ones_row k_ones attn_ones_row attn_k_ones")
Block = namedtuple("Block", "norm1_pass norm2_pass proj_rowsq fc2_rowsq")
TowerCall = namedtuple("TowerCall", "patch_fused vt_pages qk_rows q_on_load qkv_post nf pipe pipe_rows n_gemm n_attn n_other first middle last bytes table lines")
GlueCall = namedtuple("GlueCall", "hd_merge glb_row n_gemm n_attn n_other bytes feats_bytes table lines")


def build(extra=(), name="vision_plan_dump"):
    exe = os.path.join(tempfile.mkdtemp(prefix="gvl_plan_"), name)
    cmd = ["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", *extra, "-I", CSRC, SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@functools.lru_cache(maxsize=None)
def dumper():
    return build()


def pad_head(dr):
    return 64 if dr <= 64 else 96 if dr <= 96 else 128


def tower_line(tower, n, C, inter, heads, image, patch, frames, layers_run, patch_tiled, folded, **knobs):
    """the geometry as gvl_create derives it from the configuration: patch rows, tokens, padded im2col width, real and padded head dim"""
    k = dict(KNOB_DEFAULTS, **knobs)
    assert set(k) == set(KNOBS), sorted(set(k) - set(KNOBS))
    rows = (image // patch) ** 2 * frames
    Kp = -(-3 * patch * patch // 64) * 64
    geo = (tower, n, C, inter, heads, rows + 1, rows, Kp, C // heads, pad_head(C // heads), frames, image, patch, layers_run, int(patch_tiled), int(folded))
    return "T " + " ".join(str(x) for x in geo) + " " + " ".join(str(int(k[f])) for f in KNOBS)


def glue_line(phi, n, hidden, clip_hidden, iv2_dim, frames):
    img_tok, seg_tok = (156 if phi else 64), 16 * frames
    return f"G {int(phi)} {n} {hidden} {img_tok} {seg_tok} {img_tok + seg_tok + 1} {clip_hidden} {iv2_dim} {frames} 576 {256 * frames}"


def parse(ln, block):
    head = block[0].split()
    if ln[0] == "P":
        return Path(*[int(x) for x in head[1:]])
    if ln[0] == "F":
        return bool(int(head[1]))
    t = [int(x) for x in head[1:]]
    named = {w[0]: int(w[1]) for w in (b.split() for b in block[1:]) if w[0] in ("bytes", "feats_bytes")}
    table = tuple((w[1], int(w[2]), int(w[3])) for w in (b.split() for b in block[1:]) if w[0] == "ws")
    lines = tuple(b for b in block[1:] if b.split(" ", 1)[0] in ("GEMM", "ATTN", "OTHER"))
    assert len(block) == 1 + len(named) + len(table) + len(lines), block
    if ln[0] == "T":
        return TowerCall(*t[:11], Block(*t[11:15]), Block(*t[15:19]), Block(*t[19:23]), named["bytes"], table, lines)
    return GlueCall(*t, named["bytes"], named["feats_bytes"], table, lines)


def ask(lines, exe=None):
    """case lines -> per line: a TowerCall, a GlueCall, a Path or a bool"""
    r = subprocess.run([exe or dumper()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    blocks, cur = [], []
    for out in r.stdout.splitlines():
        if out == "end":
            blocks.append(cur)
            cur = []
        else:
            cur.append(out)
    assert len(blocks) == len(lines) and not cur
    return [parse(ln, b) for ln, b in zip(lines, blocks)]


@functools.lru_cache(maxsize=None)
def tower(tower_kind, n, C, inter, heads, image, frames, layers_run, patch_tiled, folded, patch=14, **knobs):
    return ask([tower_line(tower_kind, n, C, inter, heads, image, patch, frames, layers_run, patch_tiled, folded, **knobs)])[0]


@functools.lru_cache(maxsize=None)
def glue(phi, n, hidden, clip_hidden=1024, iv2_dim=1408, frames=8):
    return ask([glue_line(phi, n, hidden, clip_hidden, iv2_dim, frames)])[0]


@functools.lru_cache(maxsize=None)
def operand_path(vision_in_place, D, Dr, causal, tower_kind):
    return ask([f"P {vision_in_place} {D} {Dr} {int(causal)} {tower_kind}"])[0]


def fused_ok(tower_kind, n, T, image, patch, C):
    return ask([f"F {tower_kind} {n} {T} {image} {patch} {C} {n * T * (image // patch) ** 2}"])[0]


def counts(lines):
    """launch lines -> (GEMM, ATTN, OTHER) launches"""
    return tuple(sum(ln.startswith(c + " ") for ln in lines) for c in ("GEMM", "ATTN", "OTHER"))


def profiled(eng, run):
    """run() with gvl_prof_enable on -> (its result, the GVL_PROF_GEMM launches it made, the GVL_PROF_ATTN launches, the GVL_PROF_OTHER ones)"""
    eng.prof_enable(True)
    try:
        r = run()
        got = tuple(eng.prof_read(cat)[1] for cat in (PROF_GEMM, PROF_ATTN, PROF_OTHER))
    finally:
        eng.prof_enable(False)
    return (r,) + got
