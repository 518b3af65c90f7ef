"""The checks of the six descriptor entries of the operator level (csrc/gvl_op_check.h: check_<entry> on the descriptor, tables_<entry> -- one walk -- on the host copies
of pos and the block tables) on the CPU: tests/c/op_check.cc includes that header alone, is built with the host C++ compiler (so the header needs no HIP) and answers one
case per line.

* Every case of tests/golden/op_refusals.json -- recorded on a GPU from the entries as they were before they shared this header -- is replayed from its recorded
  descriptor and tables: the verdict must be the recorded status and text.  What a LAUNCHER refused behind the entry's checks (its text says so) the header must admit.
* Beyond the recording: RULES below, each entry's contract of include/gvl.h written out once more, by hand, in Python.  Per entry every rule is broken one at a time from
  a valid descriptor (the text is written out), then two at a time (the first in the entry's order wins); the table walk at its edges; a few thousand random small tables
  per entry against the restatement.
* The comparison can fail: an off-by-one page bound, a dropped once-only rule and a swapped check order, each as a doctored expectation, are reported."""
import atexit
import functools
import itertools
import json
import os
import random
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grounded-video-llm_amd", "csrc")
ARG = -1
P0 = {"set": 0}                       # a pointer that is set and 16-byte aligned
HOST_ARRAYS = ("pos", "tables", "block_table")


@functools.lru_cache(maxsize=None)
def checker():
    tmp = tempfile.mkdtemp(prefix="gvl_op_check_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "op_check")
    cmd = ["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", CSRC, os.path.join(ROOT, "tests", "c", "op_check.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def line(entry, fields, host=None):
    ptr = lambda v: "-" if v is None else f"@{v['set']}"   # noqa: E731
    out = [entry]
    for k, v in fields.items():
        if v is None:
            continue
        if k == "vl_tables":
            out.append(k + "=" + ",".join(ptr(t) for t in v))
        elif isinstance(v, dict):
            out.append(f"{k}={ptr(v)}")
        elif isinstance(v, (list, tuple)):
            out.append(k + "=" + ",".join(str(int(x)) for x in v))
        else:
            out.append(f"{k}={int(v)}")
    for k, v in (host or {}).items():
        if k == "vl_tables":
            out += [f"#vl{u}=" + ",".join(str(x) for x in t) for u, t in enumerate(v) if t is not None]
        elif v is not None:
            out.append(f"#{k}=" + ",".join(str(x) for x in v))
    return " ".join(out)


def run(lines):
    """-> [(status, text)] per line"""
    r = subprocess.run([checker()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = [ln.split("\t", 1) for ln in r.stdout.split("\n")[:-1]]
    assert len(out) == len(lines)
    return [(int(rc), msg) for rc, msg in out]


def script(cases):
    """the whole case script of this file's tests, for a run of the driver by hand"""
    return [line(e, f, h) for e, f, h in cases]


# ---- the recording -------------------------------------------------------------------------------------------------------------------------------------------------
def behind_the_checks(g):
    """a recorded refusal that a launcher raised, behind everything the header decides: the header must admit the case"""
    if g["text"].endswith(": the launcher does not serve this combination") or ": launch failed" in g["text"]:
        return True
    f = g["fields"]                   # gvl_launch_patch_embed's own refusal reads like the entry's: the entry's is about C % 16, patch <= 16 and even
    return g["entry"] == "patch_embed" and g["text"].endswith("geometry outside the fused kernel") and f["C"] % 16 == 0 and f["patch"] <= 16 and f["patch"] % 2 == 0


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "op_refusals.json")) as f:
        return json.load(f)


def test_every_recorded_case_gets_its_recorded_verdict_from_the_header():
    gold = golden()
    out = run([line(g["entry"], g["fields"], g["host"]) for g in gold])
    behind = 0
    for g, got in zip(gold, out):
        if g["status"] and behind_the_checks(g):
            assert g["status"] == ARG and got == (0, ""), (g["entry"], g["name"], got)
            behind += 1
        else:
            assert got == (g["status"], g["text"]), (g["entry"], g["name"], got, g["text"])
    assert len(gold) >= 190 and 10 <= behind <= 20 and sum(g["status"] == 0 for g in gold) >= 19


# ---- the rules once more, by hand ----------------------------------------------------------------------------------------------------------------------------------
class D(dict):
    """a descriptor: a field that is not given is 0 / null"""
    def __getattr__(self, k):
        return self.get(k) or 0


def low(p):
    return p["set"] if p else 0


PAGE, TWICE = "page outside the pools", "a page named twice among the pages the launch writes"


def walk(members, n_pages, short, once, page_ok=lambda page, n: 0 <= page < n, short_first=True):
    """members: (bad, t0, t1, table or None, page0).  page_ok / short_first: what the doctored variants change"""
    used = set()
    for bad, t0, t1, tab, page0 in members:
        if bad:
            return bad
        if tab is not None and t1 > len(tab) and short_first:
            return short
        for t in range(t0, t1):
            if tab is not None and t >= len(tab):
                return short
            page = tab[t] if tab is not None else page0 + t
            if not page_ok(page, n_pages):
                return PAGE
            if once and page in used:
                return TWICE
            used.add(page)
    return None


def patch_embed(f, h, **kw):
    if f.mode not in (0, 1):
        return "mode is 0 (CLIP) or 1 (InternVideo2)"
    if f.path not in (0, 1):
        return "path is 0 (fused) or 1 (three passes)"
    if min(f.n, f.T, f.image, f.patch, f.C, f.Kp) <= 0:
        return "n, T, image, patch, C and Kp must be positive"
    if f.image % f.patch:
        return "image must be a multiple of patch"
    if f.Kp % 8 or f.Kp < 3 * f.patch ** 2:
        return "Kp must be a multiple of 8 and hold 3 patch^2 columns"
    if not (f.px and f.W and f.cls and f.pos and f.out):
        return "px, W, cls, pos and out are required"
    if f.mode == 0 and not (f.lnw and f.lnb):
        return "CLIP needs lnw and lnb"
    if f.mode == 0 and f.T != 1:
        return "CLIP has one frame per image (T = 1)"
    if f.mode == 1 and not f.bias:
        return "InternVideo2 needs the conv bias"
    if f.path == 0 and f.im2col:
        return "the fused path forms no im2col matrix"
    if f.path == 1 and (f.Kp % 64 or f.C % 8 or (f.mode == 0 and f.C > 4096)):
        return "the three passes need Kp % 64 == 0 and C % 8 == 0 (CLIP: C <= 4096)"
    if f.n * f.T * (f.image // f.patch) ** 2 > 1 << 30:
        return "too many patch rows"
    if f.path == 0 and (f.C % 16 or f.patch > 16 or f.patch % 2):
        return "geometry outside the fused kernel"
    return None


def decode_proj(f, h, **kw):
    row = f.N // 2 if f.act == 3 else f.N
    if f.N <= 0 or f.K <= 0 or not f.W or not f.x:
        return "N, K > 0 and W, x set"
    if not 1 <= f.batch <= 16:
        return "1 <= batch <= 16"
    if f.path not in (0, 1) or f.w_fmt not in (0, 1, 2):
        return "path 0 / 1, w_fmt 0 / 1 / 2"
    if f.K % (32 if f.path == 0 else 8):
        return "K % 32 == 0 (tile order; the VALU GEMV: K % 8 == 0)"
    if f.act not in (0, 3):
        return "act is NONE or SILU_MUL"
    if f.x_is_tiled and (f.norm_w or f.path == 1):
        return "a tiled x feeds the skinny GEMM without norm_w only"
    if f.path == 1 and (f.variant or f.w_fmt or f.out_tiled or f.sq_in or f.sq_out or f.out_tiled2):
        return "the VALU GEMV has no variants, quantised weights, tiled outputs or fused-norm sums"
    if f.out_stride < 0 or (f.out_stride and f.out_stride < row):
        return "out_stride >= the output row length"
    if not f.rope_on and not f.out_bf16 and not f.out_f32:
        return "an output buffer"
    if f.path == 0 and f.batch > 1 and not f.rope_on and (f.out_f32 or f.resid or (f.out_bf16 and not f.out_tiled)) and (f.out_stride or row) % 4:
        return "out_stride % 4 == 0 for batch > 1 (8- and 16-byte epilogue stores)"
    if f.rope_on:
        if f.H < 1 or f.KV < 1 or f.Dr < 2 or f.Dr % 2 or f.D < f.Dr or f.N != (f.H + 2 * f.KV) * f.Dr:
            return "rope: Dr even, D >= Dr, N == (H + 2 KV) Dr"
        if not (f.cos_s and f.sin_s and f.pos and f.tables and f.Q and f.Kt and f.Vt):
            return "rope: tables, pos, page tables, Q, Kt, Vt set"
        if f.rope_switch > 0 and not (f.cos_l and f.sin_l):
            return "rope: long tables set when rope_switch > 0"
        if f.max_pos < 1 or f.n_pages < 1 or f.table_stride < 1 or f.q_stride < f.H * f.D:
            return "rope: max_pos, n_pages, table_stride >= 1, q_stride >= H D"
        if f.act or f.bias or f.resid:
            return "rope: no other epilogue"
    if f.path == 0 and f.w_fmt and f.K % (1024 if f.w_fmt == 2 else 512):          # since the entries share this header: in front of the read-back
        return "FP8 needs K % 512 == 0, MXFP4 K % 1024 == 0"
    if not f.rope_on:
        return None
    ts, members = f.table_stride, []
    for b in range(f.batch):                       # the one slot of the newest token
        p = h["pos"][b]
        out = p < 0 or p >= f.max_pos or p // 64 >= ts
        members.append(("position outside the tables" if out else None, p // 64, p // 64 + 1, h["tables"][b * ts:(b + 1) * ts], 0))
    return walk(members, f.n_pages, None, False, **kw)


def decode_attention(f, h, **kw):
    if not (f.q and f.Kt and f.Vt and f.tables and f.pos and f.part and f.counters and f.out):
        return "q, Kt, Vt, tables, pos, part, counters, out set"
    if not 1 <= f.batch <= 16:
        return "1 <= batch <= 16"
    if f.H <= 0 or f.KV <= 0 or f.H % f.KV or not 1 <= f.nsplit <= 16 or f.D not in (64, 96, 128):
        return "the launch plan does not serve this geometry (H % KV == 0, D 64 / 96 / 128, 1 <= nsplit <= 16)"
    if not 1 <= f.Dout <= f.D:
        return "1 <= Dout <= D"
    if f.q_stride < f.H * f.D or f.q_stride % 8 or low(f.q):
        return "q_stride >= H D, q rows 16-byte aligned"
    if not f.out_tiled and f.out_stride < f.H * f.Dout:
        return "out_stride >= H Dout"
    if f.n_pages < 1 or f.table_stride < 1:
        return "n_pages, table_stride >= 1"
    ts, members, longest = f.table_stride, [], 1
    for b in range(f.batch):                       # the first ceil((pos + 1) / 64) pages
        p = h["pos"][b]
        out = p < 0 or p >= ts * 64
        n = 0 if out else p // 64 + 1
        members.append(("position outside the tables" if out else None, 0, n, h["tables"][b * ts:(b + 1) * ts], 0))
    bad = walk(members, f.n_pages, None, False, **kw)
    if bad:
        return bad
    for b in range(f.batch):
        longest = max(longest, min(f.nsplit, (h["pos"][b] // 64 + 1 + 3) // 4))
    cpb = max(f.cpb, 1)
    gsplit = f.gsplit if 0 < f.gsplit <= f.nsplit else (f.nsplit + cpb - 1) // cpb
    if gsplit * cpb < longest:
        return "gsplit * cpb is smaller than the longest sequence's split count (the ticket would never complete)"
    return None


def rows_of(f):
    return [f.vl_rows[u + 1] - f.vl_rows[u] for u in range(f.vl_n)]


def qkv_post(f, h, once=True, **kw):
    n = f.vl_n
    if not f.qkv or not f.Kt or not (f.Q or f.q_rs):
        return "qkv, Kt and Q (or q_rs) set"
    if f.mode not in (0, 1, 2):
        return "mode 0, 1 or 2"
    if min(f.H, f.KV, f.B, f.n_pages) < 1:
        return "H, KV, B, n_pages >= 1"
    if f.Dr % 8 or (f.mode == 2 and f.Dr % 16) or f.D % 8 or f.D < f.Dr or not 8 <= f.Dr <= 128:
        return "Dr % 8 == 0 (mode 2: % 16), 8 <= Dr <= 128, D % 8 == 0, D >= Dr"
    if f.ld % 8 or f.ld < (f.H + 2 * f.KV) * f.Dr:
        return "ld % 8 == 0, ld >= (H + 2 KV) Dr"
    if f.mode == 1 and not (f.qn and f.kn):
        return "mode 1 needs qn and kn"
    if f.mode == 2 and (not f.cos or not f.sin or f.max_pos < 1):
        return "mode 2 needs cos, sin and max_pos"
    if f.q_rs and f.mode != 1:
        return "q_rs is a mode 1 form"
    if f.q_rs and not f.k_ones:
        return "q_rs needs k_ones"
    if (f.ones_row or f.k_ones) and f.D == f.Dr:
        return "ones_row / k_ones need D > Dr"
    if not 0 <= n <= 8:
        return "0 <= vl_n <= 8"
    if f.ext and (n < 1 or f.q_rs or not f.Vt):
        return "ext needs a ragged group, Vt and no q_rs"
    if n and (f.mode != 2 or f.B != 1 or f.pos0 != 0 or f.block_table):
        return "a ragged group needs mode 2, B == 1, pos0 == 0 and no block_table"
    if not n and (f.S < 1 or f.pos0 < 0):
        return "S >= 1, pos0 >= 0"
    if not n and f.Vt and f.pos0 % 64:
        return "Vt needs pos0 % 64 == 0 (V^T pages are written whole)"
    if not n and not f.block_table and f.pos0:
        return "pos0 > 0 needs a block table"
    if not n and f.block_table and f.max_pages < 1:
        return "max_pages >= 1"
    if n and f.vl_rows[0] != 0:
        return "vl_rows[0] must be 0"
    for u in range(n):
        if rows_of(f)[u] < 1:
            return "an empty ragged member"
        if not f.vl_tables[u] or f.table_len[u] < 1:
            return "every ragged member needs a block table"
        if f.ext and (f.vl_pos0[u] < 0 or f.vl_pos0[u] % 64):
            return "vl_pos0 must be a multiple of 64"
    members = []
    for i in range(n or f.B):                      # the tiles of the new positions [pos0, pos0 + rows)
        pos0 = (f.vl_pos0[i] if f.ext else 0) if n else f.pos0
        end = pos0 + (rows_of(f)[i] if n else f.S)
        tab = h["vl_tables"][i][:f.table_len[i]] if n else (h["block_table"][i * f.max_pages:(i + 1) * f.max_pages] if f.block_table else None)
        members.append(("a position outside the cos / sin tables" if f.mode == 2 and end > f.max_pos else None, pos0 // 64, (end + 63) // 64, tab, i * ((f.S + 63) // 64)))
    return walk(members, f.n_pages, "a block table shorter than ceil((pos0 + S) / 64)", once, **kw)


ATTN_PLAN = ("attn_plan does not serve this launch (D 64 / 96 / 128, Dout % 8 == 0, H % KV == 0, Sk == 0 or Sk >= qpos0 + S; ragged: causal, B == 1, Sk == qpos0 == 0, "
             "no block_table, per member a table and 1 .. S queries)")
EXT_PLAN = "attn_ext_plan does not serve this launch (causal, B == 1, Sk == qpos0 == 0, no block_table, vl_rows[0] == 0, per member a table, >= 1 query, vl_pos0 % 64 == 0)"


def heads_ok(f):
    return f.H > 0 and f.KV > 0 and f.H % f.KV == 0 and 0 < f.Dout <= f.D and f.Dout % 8 == 0 and f.D in (64, 96, 128) and not low(f.O)


def prefill_attention(f, h, **kw):
    n = f.vl_n
    if not (f.Q and f.Kt and f.Vt and f.O):
        return "Q, Kt, Vt, O set"
    if f.n_pages < 1:
        return "n_pages >= 1"
    if not 0 <= n <= 8:
        return "0 <= vl_n <= 8"
    if f.ext and n < 1:
        return "ext needs a ragged group"
    if not n and (not f.block_table or f.max_pages < 1):
        return "the single form needs a block table (implicit pages: gvl_op_attention)"
    if f.ring not in (0, 2, 3):
        return "ring 0, 2 or 3"
    if f.ext:
        ok = heads_ok(f) and f.causal and f.B == 1 and not f.Sk and not f.qpos0 and not f.block_table and f.vl_rows[0] == 0
        ok = ok and all(f.vl_tables[u] and rows_of(f)[u] > 0 and f.vl_pos0[u] >= 0 and f.vl_pos0[u] % 64 == 0 and f.vl_pos0[u] + rows_of(f)[u] <= 256 * 64 for u in range(n))
        if not ok:
            return EXT_PLAN
    else:
        ok = heads_ok(f) and f.B > 0 and 0 < f.S <= 256 * 64 and f.Sk <= 256 * 64
        if n:
            ok = ok and f.B == 1 and f.causal and not f.Sk and not f.qpos0 and not f.block_table and f.vl_rows[0] == 0 and all(f.vl_tables[u] and 0 < rows_of(f)[u] <= f.S for u in range(n))
        else:
            ok = ok and f.Sk >= 0 and f.qpos0 >= 0 and (f.Sk >= f.S + f.qpos0 if f.Sk > 0 else f.qpos0 == 0)
        if not ok:
            return ATTN_PLAN
    members = []
    for i in range(n or f.B):                      # the key tiles from the first one: causal up to the last query's, else all of Sk
        q0 = (f.vl_pos0[i] if f.ext else 0) if n else f.qpos0
        S = rows_of(f)[i] if n else f.S
        Sk = q0 + S if n else (f.Sk or f.S)
        tab = (h["vl_tables"][i] or [])[:max(f.table_len[i], 0)] if n else h["block_table"][i * f.max_pages:(i + 1) * f.max_pages]
        members.append(("table_len >= 1" if n and f.table_len[i] < 1 else None, 0, (q0 + S - 1) // 64 + 1 if f.causal else (Sk + 63) // 64, tab, 0))
    return walk(members, f.n_pages, "a block table shorter than the key tiles the launch reads", False, **kw)


def iv2_attention(f, h, **kw):
    fm = f.form
    if fm not in (0, 1, 2):
        return "form 0, 1 or 2"
    if not f.Kt or not f.out:
        return "Kt and out set"
    if fm == 0 and (not f.Q or not f.Vt or f.qkv or f.q_rs or f.q_nw):
        return "form 0 takes Q, Kt, Vt and no qkv, q_rs, q_nw"
    if fm == 1 and (not f.Q or not f.qkv or f.Vt or f.q_rs or f.q_nw):
        return "form 1 takes Q, Kt, qkv and no Vt, q_rs, q_nw"
    if fm == 2 and (not f.qkv or not f.q_rs or not f.q_nw or f.Q or f.Vt):
        return "form 2 takes qkv, Kt, q_rs, q_nw and no Q, Vt"
    if min(f.B, f.S, f.H) < 1:
        return "B, S, H >= 1"
    if f.Dr not in (72, 80, 88):
        return "Dr 72, 80 or 88 (a padded head on the D = 96 kernels: the ones row needs D > Dr)"
    if fm == 2 and f.Dr != 88:
        return "form 2 needs Dr == 88"
    if fm == 2 and f.pipe not in (0, 1, 2):
        return "pipe 0, 1 or 2"
    if fm == 2 and f.pipe_rows not in (0, 256):
        return "pipe_rows 0 or 256"
    if fm and (f.ld % 8 or f.ld < 3 * f.H * f.Dr):
        return "ld % 8 == 0, ld >= 3 H Dr"
    v16 = (low(f.qkv) + 4 * f.H * f.Dr) % 16 == 0              # V sits 2 H Dr elements behind q in a row of qkv
    ok = f.S <= 256 * 64 and not low(f.out) and (not fm or (v16 and 128 * f.ld < 0xffffffff)) and (fm != 2 or not (low(f.qkv) or low(f.q_nw)))
    if not ok:
        return "attn_plan does not serve this launch (at most 256 key tiles, out / qkv / q_nw 16-byte aligned, a 64-row tile of qkv below 4 GiB)"
    return None


RULES = dict(patch_embed=patch_embed, decode_proj=decode_proj, decode_attention=decode_attention, qkv_post=qkv_post, prefill_attention=prefill_attention, iv2_attention=iv2_attention)


def expect(entry, fields, host, **kw):
    text = RULES[entry](D(fields), host or {}, **kw)
    return (ARG, f"gvl_op_{entry}: {text}") if text else (0, "")


# ---- valid descriptors, and every rule broken ---------------------------------------------------------------------------------------------------------------------------
def ptrs(*names):
    return {k: P0 for k in names}


PATCH = dict(mode=1, path=0, n=2, T=2, image=28, patch=14, C=64, Kp=592, **ptrs("px", "W", "bias", "cls", "pos", "out"))
PATCH_CLIP = dict(PATCH, mode=0, T=1, bias=None, **ptrs("lnw", "lnb"))
PROJ = dict(N=48, K=1024, batch=4, **ptrs("W", "x", "out_f32"))
ROPE = dict(N=48, K=1024, batch=4, rope_on=1, H=2, KV=1, Dr=12, D=16, max_pos=8, n_pages=2, table_stride=1, q_stride=32, **ptrs("W", "x", "cos_s", "sin_s", "pos", "tables", "Q", "Kt", "Vt"))
ROPE_H = dict(pos=[0, 1, 2, 3], tables=[0, 0, 0, 0])
DATT = dict(q_stride=256, n_pages=9, table_stride=6, out_stride=256, batch=2, H=4, KV=2, D=64, Dout=64, nsplit=16, **ptrs("q", "Kt", "Vt", "tables", "pos", "part", "counters", "out"))
DATT_H = dict(pos=[256, 64], tables=[0, 1, 2, 3, 4, 0, 5, 6, 0, 0, 0, 0])
QKV = dict(ld=96, B=2, S=65, H=2, KV=2, Dr=16, D=24, mode=2, pos0=64, max_pages=4, n_pages=8, max_pos=200, ones_row=1, k_ones=1, **ptrs("qkv", "Q", "Kt", "Vt", "cos", "sin", "block_table"))
QKV_H = dict(block_table=[7, 0, 1, 7, 7, 2, 3, 7])
QKV_PLAIN = dict(ld=96, B=2, S=65, H=2, KV=2, Dr=16, D=16, mode=0, n_pages=4, **ptrs("qkv", "Q", "Kt", "Vt"))
QKV_NORM = dict(ld=96, B=1, S=5, H=2, KV=2, Dr=16, D=24, mode=1, n_pages=1, k_ones=1, **ptrs("qkv", "Kt", "Vt", "qn", "kn", "q_rs"))
QKV_EXT = dict(ld=96, B=1, H=2, KV=2, Dr=16, D=16, mode=2, n_pages=8, max_pos=200, ext=1, vl_n=3, vl_rows=[0, 3, 68, 70], vl_tables=[P0, P0, P0], vl_pos0=[64, 0, 128], table_len=[2, 2, 3],
               **ptrs("qkv", "Q", "Kt", "Vt", "cos", "sin"))
QKV_EXT_H = dict(vl_tables=[[-9, 0], [1, 2], [-9, -9, 3]])
PRE = dict(max_pages=4, B=2, H=4, KV=2, S=65, D=96, Dout=80, Sk=129, qpos0=64, causal=1, n_pages=8, **ptrs("Q", "Kt", "Vt", "O", "block_table"))
PRE_H = dict(block_table=[0, 1, 2, -5, 3, 4, 5, 99])
PRE_EXT = dict(B=1, H=4, KV=4, S=129, D=64, Dout=64, causal=1, n_pages=12, ext=1, vl_n=3, vl_rows=[0, 65, 96, 225], vl_tables=[P0, P0, P0], vl_pos0=[64, 0, 192], table_len=[3, 2, 7],
               **ptrs("Q", "Kt", "Vt", "O"))
PRE_EXT_H = dict(vl_tables=[[0, 1, 2], [3, 99], [4, 5, 6, 7, 8, 9, -1]])
IV2 = {0: dict(form=0, B=2, S=129, H=2, Dr=88, **ptrs("Q", "Kt", "Vt", "out")), 1: dict(form=1, B=2, S=129, H=2, Dr=80, ld=480, **ptrs("Q", "Kt", "qkv", "out")),
       2: dict(form=2, B=2, S=129, H=2, Dr=88, ld=536, pipe=1, **ptrs("qkv", "Kt", "q_rs", "q_nw", "out"))}

# (entry, valid fields, host arrays, [(changed fields or host arrays, the text behind "gvl_op_<entry>: ")]) -- every rule of the entry's contract, in the entry's order
BREAKS = [
    ("patch_embed", PATCH, None, [
        (dict(mode=2), "mode is 0 (CLIP) or 1 (InternVideo2)"), (dict(path=2), "path is 0 (fused) or 1 (three passes)"), (dict(n=0), "n, T, image, patch, C and Kp must be positive"),
        (dict(C=-8), "n, T, image, patch, C and Kp must be positive"), (dict(image=30), "image must be a multiple of patch"), (dict(Kp=580), "Kp must be a multiple of 8 and hold 3 patch^2 columns"),
        (dict(Kp=584), "Kp must be a multiple of 8 and hold 3 patch^2 columns"), (dict(out=None), "px, W, cls, pos and out are required"), (dict(px=None), "px, W, cls, pos and out are required"),
        (dict(bias=None), "InternVideo2 needs the conv bias"), (dict(im2col=P0), "the fused path forms no im2col matrix"),
        (dict(path=1), "the three passes need Kp % 64 == 0 and C % 8 == 0 (CLIP: C <= 4096)"), (dict(path=1, Kp=640, C=68), "the three passes need Kp % 64 == 0 and C % 8 == 0 (CLIP: C <= 4096)"),
        (dict(n=1 << 20, T=1 << 9), "too many patch rows"), (dict(C=72), "geometry outside the fused kernel"), (dict(patch=7, Kp=152), "geometry outside the fused kernel"),
        (dict(patch=28, Kp=2352), "geometry outside the fused kernel")]),
    ("patch_embed", PATCH_CLIP, None, [
        (dict(lnw=None), "CLIP needs lnw and lnb"), (dict(lnb=None), "CLIP needs lnw and lnb"), (dict(T=2), "CLIP has one frame per image (T = 1)"),
        (dict(path=1, Kp=640, C=4104), "the three passes need Kp % 64 == 0 and C % 8 == 0 (CLIP: C <= 4096)")]),
    ("decode_proj", PROJ, None, [
        (dict(N=0), "N, K > 0 and W, x set"), (dict(x=None), "N, K > 0 and W, x set"), (dict(batch=0), "1 <= batch <= 16"), (dict(batch=17), "1 <= batch <= 16"),
        (dict(path=2), "path 0 / 1, w_fmt 0 / 1 / 2"), (dict(w_fmt=3), "path 0 / 1, w_fmt 0 / 1 / 2"), (dict(K=1040), "K % 32 == 0 (tile order; the VALU GEMV: K % 8 == 0)"),
        (dict(path=1, K=1028), "K % 32 == 0 (tile order; the VALU GEMV: K % 8 == 0)"), (dict(act=1), "act is NONE or SILU_MUL"),
        (dict(x_is_tiled=1, norm_w=P0), "a tiled x feeds the skinny GEMM without norm_w only"), (dict(x_is_tiled=1, path=1), "a tiled x feeds the skinny GEMM without norm_w only"),
        (dict(path=1, variant=1), "the VALU GEMV has no variants, quantised weights, tiled outputs or fused-norm sums"),
        (dict(path=1, sq_out=P0), "the VALU GEMV has no variants, quantised weights, tiled outputs or fused-norm sums"), (dict(out_stride=-4), "out_stride >= the output row length"),
        (dict(out_stride=44), "out_stride >= the output row length"), (dict(out_f32=None), "an output buffer"), (dict(out_stride=50), "out_stride % 4 == 0 for batch > 1 (8- and 16-byte epilogue stores)"),
        (dict(N=50), "out_stride % 4 == 0 for batch > 1 (8- and 16-byte epilogue stores)"), (dict(w_fmt=1, K=768), "FP8 needs K % 512 == 0, MXFP4 K % 1024 == 0"),
        (dict(w_fmt=2, K=1536), "FP8 needs K % 512 == 0, MXFP4 K % 1024 == 0")]),
    ("decode_proj", ROPE, ROPE_H, [
        (dict(Dr=11), "rope: Dr even, D >= Dr, N == (H + 2 KV) Dr"), (dict(D=8), "rope: Dr even, D >= Dr, N == (H + 2 KV) Dr"), (dict(H=1), "rope: Dr even, D >= Dr, N == (H + 2 KV) Dr"),
        (dict(cos_s=None), "rope: tables, pos, page tables, Q, Kt, Vt set"), (dict(Vt=None), "rope: tables, pos, page tables, Q, Kt, Vt set"),
        (dict(rope_switch=4), "rope: long tables set when rope_switch > 0"), (dict(max_pos=0), "rope: max_pos, n_pages, table_stride >= 1, q_stride >= H D"),
        (dict(q_stride=31), "rope: max_pos, n_pages, table_stride >= 1, q_stride >= H D"), (dict(bias=P0), "rope: no other epilogue"),
        (dict(w_fmt=1, K=768), "FP8 needs K % 512 == 0, MXFP4 K % 1024 == 0"), (dict(pos=[0, 1, 2, 8]), "position outside the tables"), (dict(pos=[-1, 1, 2, 3]), "position outside the tables"),
        (dict(max_pos=100, pos=[0, 1, 2, 64]), "position outside the tables"), (dict(tables=[0, 1, 2, 0]), PAGE), (dict(tables=[0, -1, 0, 0]), PAGE)]),
    ("decode_attention", DATT, DATT_H, [
        (dict(part=None), "q, Kt, Vt, tables, pos, part, counters, out set"), (dict(batch=0), "1 <= batch <= 16"), (dict(batch=17), "1 <= batch <= 16"),
        (dict(KV=3), "the launch plan does not serve this geometry (H % KV == 0, D 64 / 96 / 128, 1 <= nsplit <= 16)"),
        (dict(D=80, Dout=80), "the launch plan does not serve this geometry (H % KV == 0, D 64 / 96 / 128, 1 <= nsplit <= 16)"),
        (dict(nsplit=17), "the launch plan does not serve this geometry (H % KV == 0, D 64 / 96 / 128, 1 <= nsplit <= 16)"),
        (dict(nsplit=0), "the launch plan does not serve this geometry (H % KV == 0, D 64 / 96 / 128, 1 <= nsplit <= 16)"), (dict(Dout=65), "1 <= Dout <= D"), (dict(Dout=0), "1 <= Dout <= D"),
        (dict(q_stride=248), "q_stride >= H D, q rows 16-byte aligned"), (dict(q_stride=260), "q_stride >= H D, q rows 16-byte aligned"), (dict(q={"set": 2}), "q_stride >= H D, q rows 16-byte aligned"),
        (dict(out_stride=255), "out_stride >= H Dout"), (dict(n_pages=0), "n_pages, table_stride >= 1"), (dict(table_stride=0), "n_pages, table_stride >= 1"),
        (dict(pos=[256, -1]), "position outside the tables"), (dict(pos=[384, 64]), "position outside the tables"), (dict(tables=[0, 1, 2, 3, 9, 0, 5, 6, 0, 0, 0, 0]), PAGE),
        (dict(tables=[0, 1, 2, 3, 4, 0, 5, -1, 0, 0, 0, 0]), PAGE),
        (dict(gsplit=1, cpb=1), "gsplit * cpb is smaller than the longest sequence's split count (the ticket would never complete)")]),
    ("qkv_post", QKV, QKV_H, [
        (dict(Kt=None), "qkv, Kt and Q (or q_rs) set"), (dict(Q=None), "qkv, Kt and Q (or q_rs) set"), (dict(mode=3), "mode 0, 1 or 2"), (dict(n_pages=0), "H, KV, B, n_pages >= 1"),
        (dict(B=0), "H, KV, B, n_pages >= 1"), (dict(Dr=8), "Dr % 8 == 0 (mode 2: % 16), 8 <= Dr <= 128, D % 8 == 0, D >= Dr"), (dict(D=28), "Dr % 8 == 0 (mode 2: % 16), 8 <= Dr <= 128, D % 8 == 0, D >= Dr"),
        (dict(D=8), "Dr % 8 == 0 (mode 2: % 16), 8 <= Dr <= 128, D % 8 == 0, D >= Dr"), (dict(Dr=144, D=144, ld=864), "Dr % 8 == 0 (mode 2: % 16), 8 <= Dr <= 128, D % 8 == 0, D >= Dr"),
        (dict(ld=100), "ld % 8 == 0, ld >= (H + 2 KV) Dr"), (dict(ld=88), "ld % 8 == 0, ld >= (H + 2 KV) Dr"), (dict(cos=None), "mode 2 needs cos, sin and max_pos"),
        (dict(max_pos=0), "mode 2 needs cos, sin and max_pos"), (dict(q_rs=P0), "q_rs is a mode 1 form"), (dict(D=16), "ones_row / k_ones need D > Dr"), (dict(vl_n=9), "0 <= vl_n <= 8"),
        (dict(vl_n=-1), "0 <= vl_n <= 8"), (dict(ext=1), "ext needs a ragged group, Vt and no q_rs"), (dict(S=0), "S >= 1, pos0 >= 0"), (dict(pos0=-64), "S >= 1, pos0 >= 0"),
        (dict(pos0=32), "Vt needs pos0 % 64 == 0 (V^T pages are written whole)"), (dict(block_table=None), "pos0 > 0 needs a block table"), (dict(max_pages=0), "max_pages >= 1"),
        (dict(max_pos=128), "a position outside the cos / sin tables"), (dict(max_pages=2, block_table=[7, 0, 7, 2]), "a block table shorter than ceil((pos0 + S) / 64)"),
        (dict(block_table=[7, 0, 8, 7, 7, 2, 3, 7]), PAGE), (dict(block_table=[7, -1, 1, 7, 7, 2, 3, 7]), PAGE), (dict(block_table=[7, 0, 1, 7, 7, 1, 3, 7]), TWICE),
        (dict(block_table=[7, 0, 0, 7, 7, 2, 3, 7]), TWICE)]),
    ("qkv_post", QKV_PLAIN, None, [(dict(n_pages=3), PAGE), (dict(pos0=64), "pos0 > 0 needs a block table"), (dict(ones_row=1), "ones_row / k_ones need D > Dr"), (dict(Dr=8, D=8, ld=48), None)]),
    ("qkv_post", QKV_NORM, None, [(dict(qn=None), "mode 1 needs qn and kn"), (dict(kn=None), "mode 1 needs qn and kn"), (dict(k_ones=0), "q_rs needs k_ones")]),
    ("qkv_post", QKV_EXT, QKV_EXT_H, [
        (dict(Vt=None), "ext needs a ragged group, Vt and no q_rs"), (dict(mode=0), "a ragged group needs mode 2, B == 1, pos0 == 0 and no block_table"),
        (dict(B=2), "a ragged group needs mode 2, B == 1, pos0 == 0 and no block_table"), (dict(pos0=64), "a ragged group needs mode 2, B == 1, pos0 == 0 and no block_table"),
        (dict(block_table=P0, max_pages=8), "a ragged group needs mode 2, B == 1, pos0 == 0 and no block_table"), (dict(vl_rows=[1, 3, 68, 70]), "vl_rows[0] must be 0"),
        (dict(vl_rows=[0, 3, 3, 70]), "an empty ragged member"), (dict(vl_rows=[0, 68, 3, 70]), "an empty ragged member"), (dict(vl_tables=[None, P0, P0]), "every ragged member needs a block table"),
        (dict(table_len=[2, 0, 3]), "every ragged member needs a block table"), (dict(vl_pos0=[64, 0, 100]), "vl_pos0 must be a multiple of 64"), (dict(vl_pos0=[-64, 0, 128]), "vl_pos0 must be a multiple of 64"),
        (dict(max_pos=129), "a position outside the cos / sin tables"), (dict(table_len=[2, 1, 3]), "a block table shorter than ceil((pos0 + S) / 64)"),
        (dict(vl_tables=[[-9, 0], [1, 8], [-9, -9, 3]]), PAGE), (dict(vl_tables=[[-9, 0], [1, 2], [-9, -9, 2]]), TWICE), (dict(vl_tables=[[-9, 0], [1, 1], [-9, -9, 3]]), TWICE),
        (dict(ext=0, vl_tables=[[4, 0], [1, 2], [5, -9, 3]]), None), (dict(ext=0), PAGE)]),
    ("prefill_attention", PRE, PRE_H, [
        (dict(O=None), "Q, Kt, Vt, O set"), (dict(n_pages=0), "n_pages >= 1"), (dict(vl_n=9), "0 <= vl_n <= 8"), (dict(ext=1), "ext needs a ragged group"),
        (dict(block_table=None), "the single form needs a block table (implicit pages: gvl_op_attention)"), (dict(max_pages=0), "the single form needs a block table (implicit pages: gvl_op_attention)"),
        (dict(ring=4), "ring 0, 2 or 3"), (dict(D=80), ATTN_PLAN), (dict(Dout=76), ATTN_PLAN), (dict(Dout=104), ATTN_PLAN), (dict(KV=3), ATTN_PLAN), (dict(S=0), ATTN_PLAN), (dict(Sk=128), ATTN_PLAN),
        (dict(Sk=0), ATTN_PLAN), (dict(qpos0=-64), ATTN_PLAN), (dict(O={"set": 8}), ATTN_PLAN), (dict(B=0), ATTN_PLAN), (dict(Sk=256 * 64 + 1), ATTN_PLAN),
        (dict(max_pages=2, block_table=[0, 1, 3, 4]), "a block table shorter than the key tiles the launch reads"), (dict(block_table=[0, 1, 2, -5, 3, 4, 8, 99]), PAGE),
        (dict(block_table=[-1, 1, 2, -5, 3, 4, 5, 99]), PAGE), (dict(causal=0, Sk=200), PAGE), (dict(causal=0, Sk=192), None), (dict(block_table=[0, 0, 0, -5, 0, 0, 0, 99]), None)]),
    ("prefill_attention", PRE_EXT, PRE_EXT_H, [
        (dict(causal=0), EXT_PLAN), (dict(B=2), EXT_PLAN), (dict(Sk=200), EXT_PLAN), (dict(qpos0=64), EXT_PLAN), (dict(block_table=P0, max_pages=2), EXT_PLAN), (dict(vl_rows=[1, 65, 96, 225]), EXT_PLAN),
        (dict(vl_tables=[None, P0, P0]), EXT_PLAN), (dict(vl_rows=[0, 65, 65, 225]), EXT_PLAN), (dict(vl_pos0=[64, 0, 100]), EXT_PLAN), (dict(vl_pos0=[-64, 0, 192]), EXT_PLAN),
        (dict(vl_pos0=[64, 0, 256 * 64]), EXT_PLAN), (dict(table_len=[3, 0, 7]), "table_len >= 1"), (dict(table_len=[3, 2, 5]), "a block table shorter than the key tiles the launch reads"),
        (dict(vl_tables=[[0, 1, 2], [3, 99], [12, 5, 6, 7, 8, 9, -1]]), PAGE), (dict(vl_tables=[[0, 1, 2], [-1, 99], [4, 5, 6, 7, 8, 9, -1]]), PAGE),
        (dict(ext=0, causal=0), ATTN_PLAN), (dict(ext=0, S=128), ATTN_PLAN), (dict(ext=0, vl_rows=[0, 65, 65, 225]), ATTN_PLAN), (dict(ext=0, vl_rows=[1, 65, 96, 225]), ATTN_PLAN), (dict(ext=0), None)]),
] + [("iv2_attention", IV2[fm], None, br) for fm, br in (
    (0, [(dict(form=3), "form 0, 1 or 2"), (dict(form=-1), "form 0, 1 or 2"), (dict(Kt=None), "Kt and out set"), (dict(out=None), "Kt and out set"), (dict(Q=None), "form 0 takes Q, Kt, Vt and no qkv, q_rs, q_nw"),
         (dict(q_nw=P0), "form 0 takes Q, Kt, Vt and no qkv, q_rs, q_nw"), (dict(H=0), "B, S, H >= 1"), (dict(Dr=64), "Dr 72, 80 or 88 (a padded head on the D = 96 kernels: the ones row needs D > Dr)"),
         (dict(Dr=84), "Dr 72, 80 or 88 (a padded head on the D = 96 kernels: the ones row needs D > Dr)"), (dict(Dr=96), "Dr 72, 80 or 88 (a padded head on the D = 96 kernels: the ones row needs D > Dr)"),
         (dict(S=256 * 64 + 1), "attn_plan does not serve this launch (at most 256 key tiles, out / qkv / q_nw 16-byte aligned, a 64-row tile of qkv below 4 GiB)"),
         (dict(out={"set": 2}), "attn_plan does not serve this launch (at most 256 key tiles, out / qkv / q_nw 16-byte aligned, a 64-row tile of qkv below 4 GiB)"), (dict(Dr=72), None)]),
    (1, [(dict(qkv=None), "form 1 takes Q, Kt, qkv and no Vt, q_rs, q_nw"), (dict(Vt=P0), "form 1 takes Q, Kt, qkv and no Vt, q_rs, q_nw"), (dict(S=0), "B, S, H >= 1"), (dict(ld=484), "ld % 8 == 0, ld >= 3 H Dr"),
         (dict(ld=472), "ld % 8 == 0, ld >= 3 H Dr"), (dict(qkv={"set": 2}), "attn_plan does not serve this launch (at most 256 key tiles, out / qkv / q_nw 16-byte aligned, a 64-row tile of qkv below 4 GiB)"),
         (dict(ld=1 << 25), "attn_plan does not serve this launch (at most 256 key tiles, out / qkv / q_nw 16-byte aligned, a 64-row tile of qkv below 4 GiB)"), (dict(pipe=7, pipe_rows=3), None)]),
    (2, [(dict(q_rs=None), "form 2 takes qkv, Kt, q_rs, q_nw and no Q, Vt"), (dict(Q=P0), "form 2 takes qkv, Kt, q_rs, q_nw and no Q, Vt"), (dict(B=0), "B, S, H >= 1"), (dict(Dr=80), "form 2 needs Dr == 88"),
         (dict(pipe=3), "pipe 0, 1 or 2"), (dict(pipe=-1), "pipe 0, 1 or 2"), (dict(pipe_rows=128), "pipe_rows 0 or 256"), (dict(ld=532), "ld % 8 == 0, ld >= 3 H Dr"),
         (dict(q_nw={"set": 2}), "attn_plan does not serve this launch (at most 256 key tiles, out / qkv / q_nw 16-byte aligned, a 64-row tile of qkv below 4 GiB)"),
         (dict(qkv={"set": 2}), "attn_plan does not serve this launch (at most 256 key tiles, out / qkv / q_nw 16-byte aligned, a 64-row tile of qkv below 4 GiB)"), (dict(pipe_rows=256), None)]))]


def changed(fields, host, ch):
    f, h = dict(fields), dict(host or {})
    for k, v in ch.items():
        if k in HOST_ARRAYS and isinstance(v, list) or (k == "vl_tables" and v and isinstance(v[0], list)):
            h[k] = v
        else:
            f[k] = v
    return f, h


def broken_cases():
    """-> [(entry, fields, host, text or None)]: the valid descriptors, then every rule broken"""
    out = []
    for entry, fields, host, breaks in BREAKS:
        out.append((entry, fields, host, None))
        out += [(entry,) + changed(fields, host, ch) + (text,) for ch, text in breaks]
    return out


def pair_cases():
    """two changes at once, of different fields"""
    out = []
    for entry, fields, host, breaks in BREAKS:
        for (a, _), (b, _) in itertools.combinations(breaks, 2):
            if not set(a) & set(b):
                out.append((entry,) + changed(fields, host, dict(a, **b)))
    return out


def test_every_rule_broken_alone_gets_its_text():
    cases = broken_cases()
    out = run(script([c[:3] for c in cases]))
    for (entry, f, h, text), got in zip(cases, out):
        want = (ARG, f"gvl_op_{entry}: {text}") if text else (0, "")
        assert got == want, (entry, f, h, got, want)
        assert expect(entry, f, h) == want, (entry, f, h, expect(entry, f, h), want)
    texts = {c[3] for c in cases} - {None}
    with open(os.path.join(CSRC, "gvl_op_check.h")) as fh:
        src = fh.read()
    for t in texts:
        assert src.count('"' + t + '"') == 1, t
    # every text of the header is reached, but the one no descriptor reaches: Dr 72 / 80 / 88 always plans a ONES kernel
    in_header = set(re.findall(r'(?:return|\?|=|,) "([^"]+)"', src))
    assert len(cases) > 200 and in_header - texts == {"the plan chose no ONES kernel for this launch"}, (sorted(in_header - texts), sorted(texts - in_header))


def test_two_faults_get_the_check_that_stands_first():
    cases = pair_cases()
    out = run(script(cases))
    for (entry, f, h), got in zip(cases, out):
        assert got == expect(entry, f, h), (entry, f, h, got, expect(entry, f, h))
    assert len(cases) > 1500
    # the order, spelled out where it matters most
    first = [("decode_proj", dict(ROPE, w_fmt=1, K=768), dict(ROPE_H, pos=[0, 1, 2, 8]), "FP8 needs K % 512 == 0, MXFP4 K % 1024 == 0"),     # the quantised K in front of the read-back
             ("decode_proj", dict(ROPE), dict(pos=[0, 1, 2, 8], tables=[5, 0, 0, 0]), PAGE),                                                # sequence 0's page in front of sequence 3's position
             ("decode_attention", dict(DATT, gsplit=1, cpb=1), dict(DATT_H, tables=[0, 1, 2, 3, 9, 0, 5, 6, 0, 0, 0, 0]), PAGE),            # the pages in front of the launch shape
             ("qkv_post", dict(QKV, max_pos=128), dict(block_table=[7, 8, 1, 7, 7, 2, 3, 7]), "a position outside the cos / sin tables"),
             ("qkv_post", dict(QKV_EXT, max_pos=129), dict(vl_tables=[[-9, 9], [1, 2], [-9, -9, 3]]), PAGE),                                # member 0's page in front of member 2's position
             ("qkv_post", dict(QKV, max_pages=2), dict(block_table=[7, 9, 7, 2]), "a block table shorter than ceil((pos0 + S) / 64)"),      # the length in front of the member's pages
             ("prefill_attention", dict(PRE_EXT, table_len=[3, 0, 7]), dict(vl_tables=[[0, 1, 12], [3, 99], [4, 5, 6, 7, 8, 9, -1]]), PAGE),   # member 0's page in front of member 1's length
             ("prefill_attention", dict(PRE_EXT, table_len=[3, 0, 7], causal=0), PRE_EXT_H, EXT_PLAN)]
    for (entry, f, h, text), got in zip(first, run(script([c[:3] for c in first]))):
        assert got == (ARG, f"gvl_op_{entry}: {text}") == expect(entry, f, h), (entry, f, h, got)


# ---- the walk at its edges and on random tables -----------------------------------------------------------------------------------------------------------------------
def edge_cases():
    ts = 3                                           # table_stride
    da = lambda pos, tab, **kw: ("decode_attention", dict(dict(DATT, batch=1, table_stride=ts, nsplit=1), **kw), dict(pos=[pos], tables=tab))   # noqa: E731
    dp = lambda pos, tab, **kw: ("decode_proj", dict(dict(ROPE, batch=1, table_stride=ts, max_pos=1 << 20, n_pages=9), **kw), dict(pos=[pos], tables=tab))   # noqa: E731
    out = [da(ts * 64 - 1, [0, 1, 8]), da(ts * 64, [0, 1, 8]), da(ts * 64 - 1, [0, 1, 9]), da(ts * 64 - 1, [0, -1, 8]), da(127, [0, 1, 9]), da(128, [0, 1, 9]), da(0, [8, 9, 9]), da(0, [9, 0, 0]),
           dp(ts * 64 - 1, [9, 9, 8]), dp(ts * 64, [0, 0, 0]), dp(ts * 64 - 1, [0, 0, 9]), dp(ts * 64 - 1, [0, 0, -1]), dp(64, [9, 8, 9]), dp(63, [9, 8, 9]), dp(7, [0, 0, 0], max_pos=8), dp(8, [0, 0, 0], max_pos=8)]
    q = lambda S, pos0, tab, **kw: ("qkv_post", dict(dict(QKV, B=1, S=S, pos0=pos0, max_pages=len(tab), max_pos=1 << 20), **kw), dict(block_table=tab))   # noqa: E731
    out += [q(64, 64, [-1, 7]), q(65, 64, [-1, 7]), q(65, 64, [-1, 7, 8]), q(65, 64, [-1, 7, 7]), q(128, 0, [6, 7]), q(129, 0, [6, 7]), q(1, 128, [9, 9, 0]), q(1, 128, [9, 9, -1]),
            q(192, 0, [3, 4, 3]), q(64, 0, [7], n_pages=7), q(64, 0, [6], n_pages=7)]
    out += [("qkv_post", dict(QKV_EXT), dict(vl_tables=[[-9, 3], [1, 2], [-9, -9, 3]])), ("qkv_post", dict(QKV_EXT), dict(vl_tables=[[3, 0], [1, 2], [0, 1, 3]])),
            ("qkv_post", dict(QKV_EXT, n_pages=4), QKV_EXT_H), ("qkv_post", dict(QKV_EXT, n_pages=3), QKV_EXT_H)]
    p = lambda S, q0, tab, **kw: ("prefill_attention", dict(dict(PRE, B=1, S=S, qpos0=q0, Sk=q0 + S, max_pages=len(tab)), **kw), dict(block_table=tab))   # noqa: E731
    out += [p(64, 64, [0, 7]), p(65, 64, [0, 7]), p(65, 64, [0, 7, 8]), p(65, 64, [0, 7, 7]), p(1, 128, [0, 1, -1]), p(64, 64, [0, 7, 99]), p(64, 64, [8, 7]), p(64, 0, [0], causal=0, Sk=65),
            p(64, 0, [0, 8], causal=0, Sk=65), p(64, 0, [0, 7], causal=0, Sk=128), p(64, 0, [0, 7], causal=0, Sk=129)]
    return out


def test_the_walk_at_its_edges():
    cases = edge_cases()
    out = run(script(cases))
    for (entry, f, h), got in zip(cases, out):
        assert got == expect(entry, f, h), (entry, f, h, got, expect(entry, f, h))
    texts = [t.split(": ", 1)[-1] for _, t in out]
    assert texts.count("") >= 15 and texts.count(PAGE) >= 14 and texts.count(TWICE) >= 3 and texts.count("position outside the tables") >= 3
    assert texts.count("a block table shorter than ceil((pos0 + S) / 64)") >= 2 and texts.count("a block table shorter than the key tiles the launch reads") >= 3


def random_cases(seed=7, n=2500):
    """small tables: at most 4 members, 6 tiles, 8 pages; a fault of every kind is frequent"""
    r = random.Random(seed)
    out = []
    page = lambda n_pages: r.choice([r.randrange(n_pages), r.randrange(n_pages), r.randrange(n_pages), -1, n_pages, n_pages - 1, 0])   # noqa: E731
    for _ in range(n):
        B, ts, n_pages = r.randint(1, 4), r.randint(1, 6), r.randint(1, 8)
        pos = [r.choice([r.randrange(ts * 64), ts * 64 - 1, ts * 64, -1, 0, 63, 64]) for _ in range(B)]
        tabs = [page(n_pages) for _ in range(B * ts)]
        out.append(("decode_attention", dict(DATT, batch=B, table_stride=ts, n_pages=n_pages, nsplit=r.choice([1, 2, 16]), gsplit=r.choice([0, 1, 2]), cpb=r.choice([0, 1, 2])), dict(pos=pos, tables=tabs)))
        out.append(("decode_proj", dict(ROPE, batch=B, table_stride=ts, n_pages=n_pages, max_pos=r.choice([ts * 64, 65, 1 << 20])), dict(pos=pos, tables=tabs)))
        S, pos0 = r.randint(1, 200), 64 * r.randint(0, 3)
        mp = r.randint(1, 6)
        tab = [r.sample(range(-1, n_pages + 1), 1)[0] if r.random() < 0.3 else r.randrange(n_pages) for _ in range(B * mp)]
        out.append(("qkv_post", dict(QKV, B=B, S=S, pos0=pos0, max_pages=mp, n_pages=n_pages, max_pos=r.choice([pos0 + S, pos0 + S - 1, 1 << 20])), dict(block_table=tab)))
        out.append(("qkv_post", dict(QKV_PLAIN, B=B, S=S, n_pages=n_pages), None))
        out.append(("prefill_attention", dict(PRE, B=B, S=S, qpos0=pos0, Sk=pos0 + S + r.choice([0, 0, 70]), causal=r.randint(0, 1), max_pages=mp, n_pages=n_pages), dict(block_table=tab)))
        n_m = r.randint(1, 4)
        lens = [r.randint(1, 130) for _ in range(n_m)]
        rows = [sum(lens[:u]) for u in range(n_m + 1)]
        p0 = [64 * r.randint(0, 3) for _ in range(n_m)]
        tl = [r.randint(1, 6) for _ in range(n_m)]
        vt = [[page(n_pages) for _ in range(x)] for x in tl]
        ext = r.randint(0, 1)
        grp = dict(vl_n=n_m, vl_rows=rows, vl_tables=[P0] * n_m, vl_pos0=p0, table_len=tl, ext=ext, n_pages=n_pages)
        out.append(("qkv_post", dict(QKV_EXT, max_pos=r.choice([1 << 20, 130]), **grp), dict(vl_tables=vt)))
        out.append(("prefill_attention", dict(PRE_EXT, S=max(lens), **dict(grp, table_len=[x - (r.random() < 0.05) for x in tl])), dict(vl_tables=vt)))
    return out


def test_random_small_tables_agree_with_the_restatement():
    cases = random_cases()
    out = run(script(cases))
    seen = {}
    for (entry, f, h), got in zip(cases, out):
        assert got == expect(entry, f, h), (entry, f, h, got, expect(entry, f, h))
        seen.setdefault(entry, set()).add(got[1].split(": ", 1)[-1])
    assert len(cases) >= 4 * 2500
    for entry, texts in seen.items():                      # per entry: admitted, and every refusal of its walk
        assert "" in texts and PAGE in texts and len(texts) >= (3 if entry == "decode_proj" else 4), (entry, texts)
    assert TWICE in seen["qkv_post"] and "table_len >= 1" in seen["prefill_attention"]


# ---- the comparison can fail -----------------------------------------------------------------------------------------------------------------------------------------
def test_a_wrong_page_bound_a_dropped_once_only_rule_and_a_swapped_order_are_reported():
    cases = [c[:3] for c in broken_cases()] + edge_cases() + random_cases(n=300)
    out = run(script(cases))

    def differing(**kw):
        return [(e, f, h) for (e, f, h), got in zip(cases, out) if got != expect(e, f, h, **kw)]
    assert differing() == []
    off_by_one = differing(page_ok=lambda page, n: 0 <= page <= n)          # page n_pages let through
    assert len(off_by_one) >= 20 and {e for e, _, _ in off_by_one} == {"decode_proj", "decode_attention", "qkv_post", "prefill_attention"}
    no_once = [(e, f, h) for (e, f, h), got in zip(cases, out) if e == "qkv_post" and got != expect(e, f, h, once=False)]
    assert len(no_once) >= 10 and all(expect(e, f, h)[1].endswith(TWICE) for e, f, h in no_once)
    swapped = differing(short_first=False)                                  # a member's pages in front of its table's length
    assert len(swapped) >= 5 and all("shorter" in expect(e, f, h)[1] for e, f, h in swapped)
