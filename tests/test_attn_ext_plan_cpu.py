"""CPU: attn_ext_plan (csrc/gvl_attn_plan.h) -- the launch of the ragged EXTEND prefill (attn_fwd_kernel<D, 4, 2, 0, 0, 2>: a ragged causal group whose members
each sit behind their own cached prefix) -- built with the host compiler through tests/c/attn_ext_plan_dump.cc.  The form is bit-identical to per-sequence launches by
design, so no result test can tell a wrong grid that still covers every block from a right one, or notice a launch the kernel's assumptions do not hold for; this can.
Checked: the grid formula, block and LDS against the ragged form of attn_plan (tests/attn_plan.py) for the same rows, every refusal, and that the new list and the four
pinned ones are what the dispatch switches are built from."""
import functools
import os
import subprocess
import tempfile
from collections import namedtuple

import pytest

import attn_plan as A

Launch = namedtuple("Launch", "D NWAVES NS grid block lds lazy")
BASE = dict(H=32, KV=32, D=96, Dout=96, causal=1, rows=(100, 37, 200), pos0=(3456, 0, 64), tables=None, O16=1, lazy=8.0)


@functools.lru_cache(maxsize=None)
def dumper():
    exe = os.path.join(tempfile.mkdtemp(prefix="gvl_ext_plan_"), "attn_ext_plan_dump")
    cmd = ["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", A.CSRC, os.path.join(A.ROOT, "tests", "c", "attn_ext_plan_dump.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def line(**kw):
    c = dict(BASE, **kw)
    n = c.get("vl_n", len(c["rows"]))
    offs = [0]
    for r in c["rows"]:
        offs.append(offs[-1] + r)
    offs += [0] * (9 - len(offs))
    pos0 = list(c["pos0"]) + [0] * (8 - len(c["pos0"]))
    tables = (1 << len(c["rows"])) - 1 if c["tables"] is None else c["tables"]
    return f"{c['H']} {c['KV']} {c['D']} {c['Dout']} {c['causal']} {n} " + " ".join(map(str, offs[:9])) + " " + " ".join(map(str, pos0[:8])) + f" {tables} {c['O16']} {c['lazy']!r}"


def plans(lines):
    r = subprocess.run([dumper()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    got = r.stdout.splitlines()
    assert len(got) == len(lines)
    return [None if g == "-1" else Launch(*[int(x) for x in g.split()[:6]], float(g.split()[6])) for g in got]


def plan(**kw):
    return plans([line(**kw)])[0]


def ragged(rows, **kw):
    """attn_plan's ragged launch for the same rows (no prefixes)"""
    offs = [0]
    for r in rows:
        offs.append(offs[-1] + r)
    c = dict(BASE, **kw)
    got = A.plans([A.prefill_line(B=1, H=c["H"], KV=c["KV"], S=max(rows), D=c["D"], Dout=c["Dout"], causal=1, vl_n=len(rows), vl_rows=tuple(offs), vl_tables=(1 << len(rows)) - 1,
                                  lazy=c["lazy"])])[0]
    assert got is not None and len(got) == 1 and got[0].VL == 1
    return got[0]


def test_list_is_one_form_per_head_dim_and_the_pinned_lists_did_not_move():
    r = subprocess.run([dumper(), "list"], capture_output=True, text=True)
    assert r.returncode == 0
    assert [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()] == [(64, 4, 2), (96, 4, 2), (128, 4, 2)]
    assert len(A.lists()) == 15 + 2 + 12 + 9
    with open(os.path.join(A.CSRC, "gvl_attn_plan.h")) as f:
        text = f.read()
    assert "#include <hip" not in text and "getenv" not in text and "static " not in text.replace("static_assert", "")


@pytest.mark.parametrize("D,Dout", [(64, 64), (96, 96), (96, 88), (128, 128)])
@pytest.mark.parametrize("H,KV", [(32, 32), (32, 8), (8, 2), (4, 1), (24, 24), (9, 9)])
def test_grid_block_lds(D, Dout, H, KV):
    for rows, pos0 in (((100, 37, 200), (3456, 0, 64)), ((1,), (64,)), ((128, 129, 127, 1, 256, 257, 64, 65), (64, 128, 192, 320, 0, 64, 3456, 16000)), ((16384 - 64,), (64,))):
        l = plan(D=D, Dout=Dout, H=H, KV=KV, rows=rows, pos0=pos0)
        assert l is not None, (rows, pos0)
        blocks = sum(-(-r // 128) for r in rows)
        assert l.grid == blocks * (H // KV) * (-(-KV // 8) * 8), (rows, l)          # sum_u ceil(S_u / 128) x H / KV x (KV padded to 8)
        assert (l.D, l.NWAVES, l.NS, l.block, l.lazy) == (D, 4, 2, 256, 8.0)
        want = ragged(rows, D=D, Dout=Dout, H=H, KV=KV)
        assert (l.grid, l.block, l.lds) == (want.grid, want.block, want.lds) and l.lds == 2 * 2 * 64 * D * 2 + 1024     # the ragged form's, whatever the prefixes are


def test_all_prefixes_zero_is_the_ragged_launch():
    for rows in ((5,), (100, 37, 200), (128,) * 8, (1, 2049, 300)):
        for kw in (dict(D=64, Dout=64), dict(D=96, Dout=96, H=32, KV=8), dict(D=128, Dout=128, H=8, KV=2)):
            l, want = plan(rows=rows, pos0=(0,) * len(rows), **kw), ragged(rows, **kw)
            assert (l.D, l.NWAVES, l.NS, l.grid, l.block, l.lds, l.lazy) == (want.D, want.NWAVES, want.NS, want.grid, want.block, want.lds, want.lazy)


def test_refusals():
    assert plan() is not None
    bad = dict(
        pos0_not_whole_pages=dict(pos0=(3456, 0, 65)), pos0_32=dict(pos0=(32, 0, 0)), pos0_negative=dict(pos0=(-64, 0, 0)),
        empty_member=dict(rows=(100, 0, 200)), empty_first=dict(rows=(0, 5, 5)), negative_member=dict(rows=(100, -1, 200)),
        nine_members=dict(rows=(10,) * 8, pos0=(0,) * 8, vl_n=9), no_members=dict(vl_n=0), negative_count=dict(vl_n=-1),
        missing_table=dict(tables=0b101), missing_last_table=dict(tables=0b011), no_tables=dict(tables=0),
        not_causal=dict(causal=0),
        too_many_key_tiles=dict(rows=(100, 37, 65), pos0=(3456, 0, 16384 - 64)), query_rows_alone_too_many=dict(rows=(16385,), pos0=(0,)),
        head_dim=dict(D=80, Dout=80), dout_above_d=dict(D=64, Dout=72), dout_not_8=dict(D=96, Dout=90), dout_zero=dict(Dout=0),
        heads_not_grouped=dict(H=32, KV=5), no_heads=dict(H=0), no_kv_heads=dict(KV=0), o_unaligned=dict(O16=0))
    got = plans([line(**kw) for kw in bad.values()])
    assert [k for k, g in zip(bad, got) if g is not None] == []
    # the edges that ARE served: the last key tile of the page-id table, Dout below D, 8 members
    ok = [dict(rows=(100, 37, 64), pos0=(3456, 0, 16384 - 64)), dict(D=96, Dout=88), dict(rows=(10,) * 8, pos0=(64,) * 8), dict(rows=(16384,), pos0=(0,))]
    assert all(g is not None for g in plans([line(**kw) for kw in ok]))


def test_lazy_knob_is_clamped_like_the_other_forms():
    assert [plan(lazy=v).lazy for v in (0.0, 3.5, 64.0, -1.0, 65.0)] == [0.0, 3.5, 64.0, 8.0, 8.0]
