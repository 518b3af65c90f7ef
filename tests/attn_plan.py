"""Which kernel an attention launch takes, on which grid: a thin wrapper over tests/c/attn_plan_dump.cc, i.e. over the library's own decision functions
(csrc/gvl_attn_plan.h: host-only, no GPU).  Used by tests/test_attn_plan_cpu.py (recorded decisions) and by the GPU tests of the attention forms, which are bit-identical by
design: only the plan can say which kernel a case exercised.

The helpers that build a geometry the way a caller in the library does:
  op_attention   gvl_op_attention (gvl_ops.hip): gvl_debug_set vision_in_place / attn_ring choose the operand mode (vision_operand_path, asked through tests/vision_plan.py)
                 and the ring depth
  op_iv2_attention   gvl_op_iv2_attention (gvl_ops.hip): the descriptor's form / pipe / pipe_rows choose everything, no gvl_debug_set
  iv2_block      the attention launch of an InternVideo2 block (gvl_vision.hip): vision_in_place chooses the operand path (vision_operand_path), then attn_pipe, attn_pipe_rows
  decode_step    the decode-attention launch of decode_step (gvl_llm.hip): decode_attn_shape on the sequences' positions, then decode_attn_plan"""
import functools
import os
import subprocess
import tempfile
from collections import namedtuple

import vision_plan
from vision_plan import pad_head  # noqa: F401  (callers use attn_plan.pad_head)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grounded-video-llm_amd", "csrc")

# AttnMode, AttnFamily, DecodeAttnFamily (gvl_attn_plan.h)
PAGED, V_ROWS, QKV_ROWS, QNORM_V_ROWS, RAGGED = range(5)
MODE_NAMES = ("pages", "v in place", "q,k,v in place", "q normalised on load, v in place", "ragged causal prefill")
FWD, IV2_PIPE = 0, 1
GQA, HEAD = 0, 1
# presence / alignment bits of a prefill case
BLOCK_TABLE, VROWS, QROWS, KROWS, Q_RS, Q_NW = 1, 2, 4, 8, 16, 32
O16, VROWS16, QROWS16, KROWS16, Q_NW16 = 1, 2, 4, 8, 16
NSPLIT = 16                     # gvl_ctx::nsplit

PREFILL_FIELDS = ("B", "H", "KV", "S", "D", "Dout", "Sk", "qpos0", "causal", "ones_row", "k_ones", "ring", "pipe", "pipe_rows", "v_ld", "q_ld", "k_ld", "max_pages", "vl_n",
                  "vl_rows", "present", "vl_tables", "aligned", "lazy", "no_ones")
PREFILL_DEFAULTS = dict(B=1, H=1, KV=1, S=1, D=64, Dout=64, Sk=0, qpos0=0, causal=0, ones_row=0, k_ones=0, ring=0, pipe=0, pipe_rows=0, v_ld=0, q_ld=0, k_ld=0, max_pages=0, vl_n=0,
                        vl_rows=(), present=0, vl_tables=0, aligned=31, lazy=8.0, no_ones=0)
DECODE_FIELDS = ("H", "KV", "D", "nsplit", "batch", "hpb", "cpb", "gsplit", "no_gqa", "gqa_valu", "gqa_direct")

AttnLaunch = namedtuple("AttnLaunch", "mode family D NWAVES NS ONES VROW VL grid block lds q_begin q_rows lazy")
DecodeLaunch = namedtuple("DecodeLaunch", "family D t1 t2 grid_x grid_y grid_z batch cpb gsplit hpb")
Shape = namedtuple("Shape", "gsplit cpb hpb")


def kernel_of(l):
    """the instantiation a launch runs, as the lists of gvl_attn_plan.h name it"""
    if isinstance(l, AttnLaunch):
        return ("fwd", l.D, l.NWAVES, l.NS, l.ONES, l.VROW, l.VL) if l.family == FWD else ("iv2_pipe", l.NWAVES)
    return ("gqa", l.D, l.t1, l.t2) if l.family == GQA else ("head", l.D, l.t1)


@functools.lru_cache(maxsize=None)
def dumper():
    exe = os.path.join(tempfile.mkdtemp(prefix="gvl_plan_"), "attn_plan_dump")
    cmd = ["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", CSRC, os.path.join(ROOT, "tests", "c", "attn_plan_dump.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@functools.lru_cache(maxsize=None)
def lists():
    """THE lists of instantiations (the X-macros of gvl_attn_plan.h), as a set of kernel_of() names"""
    r = subprocess.run([dumper(), "lists"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return frozenset((t[0],) + tuple(int(x) for x in t[1:]) for t in (ln.split() for ln in r.stdout.splitlines()))


def prefill_line(**kw):
    c = dict(PREFILL_DEFAULTS, **kw)
    assert set(c) == set(PREFILL_FIELDS), sorted(set(c) - set(PREFILL_FIELDS))
    rows = list(c["vl_rows"]) + [0] * (9 - len(c["vl_rows"]))
    return "A " + " ".join(str(c[f]) for f in PREFILL_FIELDS[:19]) + " " + " ".join(str(r) for r in rows) + f" {c['present']} {c['vl_tables']} {c['aligned']} {c['lazy']!r} {c['no_ones']}"


def decode_line(**kw):
    c = dict(dict.fromkeys(DECODE_FIELDS, 0), **kw)
    return "D " + " ".join(str(c[f]) for f in DECODE_FIELDS)


def shape_line(positions, H, KV, nsplit=NSPLIT, force_cpb=0, force_hpb=0, capturing=0):
    return f"S {len(positions)} {H} {KV} {nsplit} {force_cpb} {force_hpb} {int(capturing)} " + " ".join(str(p) for p in positions)


def plans(lines):
    """case lines -> per line: None (refused), a list of AttnLaunch, a DecodeLaunch or a Shape"""
    r = subprocess.run([dumper()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    got = r.stdout.splitlines()
    assert len(got) == len(lines)
    out = []
    for ln, g in zip(lines, got):
        t = g.split()
        if t == ["-1"]:
            out.append(None)
        elif ln[0] == "A":
            out.append([AttnLaunch(*[int(x) for x in t[i:i + 13]], float(t[i + 13])) for i in range(0, len(t), 14)])
        elif ln[0] == "D":
            out.append(DecodeLaunch(*[int(x) for x in t]))
        else:
            out.append(Shape(*[int(x) for x in t]))
    return out


@functools.lru_cache(maxsize=None)
def op_attention(B, S, H, KV, Dr, causal, vision_in_place=1, attn_ring=0):
    """the launches of gvl_op_attention(B, S, H, KV, Dr, causal) under gvl_debug_set vision_in_place / attn_ring: q, k, v are the column blocks of one fused
    [B * S][(H + 2 KV) * Dr] tensor"""
    D, ld = pad_head(Dr), (H + 2 * KV) * Dr
    path = vision_plan.operand_path(vision_in_place, D, Dr, bool(causal), vision_plan.CLIP)
    kw = dict(B=B, H=H, KV=KV, S=S, D=D, Dout=Dr, causal=int(causal), ring=attn_ring)
    if not path.vt_pages:
        kw.update(present=VROWS, v_ld=ld)
    if path.qk_rows:
        kw.update(present=VROWS | QROWS | KROWS, q_ld=ld, k_ld=ld)
    p = plans([prefill_line(**kw)])[0]
    assert p is not None, f"gvl_op_attention {kw}: refused"
    return tuple(p)


@functools.lru_cache(maxsize=None)
def op_iv2_attention(B, S, H, Dr, form, pipe=0, pipe_rows=0, ld=0):
    """the launches of gvl_op_iv2_attention: form 0 = Q, K, V^T pages; 1 = Q, K pages + V in place; 2 = q normalised on load + K pages (k_ones) + V in place, where pipe /
    pipe_rows are read.  ones_row = 1 and KV = H in every form; ld = the pitch of qkv (0: 3 H Dr).  None: the plan refuses"""
    kw = dict(B=B, H=H, KV=H, S=S, D=pad_head(Dr), Dout=Dr, ones_row=1)
    ld = ld or 3 * H * Dr
    if form >= 1:
        kw.update(present=VROWS, v_ld=ld)
    if form == 2:
        kw.update(present=VROWS | QROWS | Q_RS | Q_NW, q_ld=ld, k_ones=1, pipe=pipe, pipe_rows=pipe_rows)
    p = plans([prefill_line(**kw)])[0]
    return None if p is None else tuple(p)


@functools.lru_cache(maxsize=None)
def iv2_block(n, S, H, Dr, vision_in_place=1, attn_pipe=1, attn_pipe_rows=0):
    """the attention launches of one InternVideo2 block for n segments of S tokens, H heads of Dr, under gvl_debug_set vision_in_place / attn_pipe / attn_pipe_rows"""
    D, C = pad_head(Dr), H * Dr
    path = vision_plan.operand_path(vision_in_place, D, Dr, False, vision_plan.IV2)
    kw = dict(B=n, H=H, KV=H, S=S, D=D, Dout=Dr, ones_row=path.attn_ones_row)
    if not path.vt_pages:
        kw.update(present=VROWS, v_ld=3 * C)
    if path.q_on_load:
        kw.update(present=kw.get("present", 0) | QROWS | Q_RS | Q_NW, q_ld=3 * C, k_ones=path.attn_k_ones, pipe=attn_pipe, pipe_rows=attn_pipe_rows)
    p = plans([prefill_line(**kw)])[0]
    assert p is not None, f"iv2 block attention {kw}: refused"
    return tuple(p)


@functools.lru_cache(maxsize=None)
def decode_step(positions, H, KV, Dr, force_cpb=0, force_hpb=0, capturing=False):
    """(Shape, DecodeLaunch) of the decode-attention launch of one decode step for sequences whose new tokens sit at `positions` (a tuple), H query heads on KV heads of Dr,
    under gvl_debug_set decode_attn_cpb / decode_attn_hpb; capturing: the step is being recorded into a graph (gvl_debug_set decode_graph 1)"""
    s = plans([shape_line(positions, H, KV, NSPLIT, force_cpb, force_hpb, capturing)])[0]
    l = plans([decode_line(H=H, KV=KV, D=pad_head(Dr), nsplit=NSPLIT, batch=len(positions), hpb=s.hpb, cpb=s.cpb, gsplit=s.gsplit)])[0]
    assert l is not None, f"decode attention {positions} {H}/{KV} x {Dr}: refused"
    return s, l
