"""-m gpu: the two decode-attention kernels (gvl_attn.hip: decode_attn_kernel<D, 1, PH>, decode_attn_gqa_kernel<D, GM, STG>) through gvl_op_decode_attention, one launch at a
time on caller-owned tensors, against an INDEPENDENT reference (tests/decode_attn_ref.py) -- where test_gpu_llm.py sees them through a 2-layer random model at a 1e-2 class
tolerance (near-uniform attention: a lost page, a mask off by one key or a dropped split all stay below it) and compares launch shapes that share the mask, the split rule,
the record format and the merge with each other.

  exact cases    one-hot attention (decode_attn_ref.onehot_case): the output must equal the target's V row BIT FOR BIT.  THE list is decode_attn_ref.exact_cases(): per geometry
                 every context length of LENS alone, a batch of 3 (one split / merging / clamped split count) and a batch of 16 mixed lengths where two sequences share their
                 prefix pages; cpb 1 / 2 / 3 / 4 / 16, gsplit 0 / the exact minimum, out_tiled 0 / 1 and padded q / out strides walk through the list.  Per case every page
                 of every sequence is some head's target, and so are key 0, the last key, the one before it and the first and last key of every split: one FRESH launch per
                 set of targets (decode_attn_ref.target_sets), nothing is retried.  A failure names sequence, head, the target key with its page, split, wave and trip,
                 and the key whose V row came out instead.
  bounded cases  dense data with the mass where the kernels are fragile (late_heavy, early_heavy, spike, split_skew, plain) against a float64 softmax: ZERO elements outside
                 decode_attn_ref.elementwise_bound (derived there, no fitted factor).
  workspace      asserted on EVERY launch: the tickets are zero afterwards; the partial records start as decoys that would win any merge (m = 1e4, l = 1, acc = 7) and the
                 records the sequence does not use are still those decoys afterwards; nothing behind [batch][H][nsplit][D + 2], behind the tickets, in the guard rows and
                 columns of out (out_tiled: in the slots of absent sequences and columns) is written; q's guard columns are NaN.
  bit identity   fixed data, within a kernel family: every cpb, gsplit and hpb, a sequence alone against the same sequence at any slot of a batch, a repeated launch, out_tiled
                 against rows.
  instantiations the union of the planned kernels (tests/attn_plan.py) over the list is EXACTLY the twelve reachable without lab knobs: ("head", D, 0 | 1) and
                 ("gqa", 64 | 128, 4 | 16, 1), ("gqa", 96, 4 | 16, 0).  PH = 2 (the round-1 grid for groups) and STG = 0 at D = 64 / 128 (operands from global memory where
                 the staged form exists) are planned only under the GVL_LAB knobs; no lab library is built for them here.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, bf, tiny_geo  # noqa: E402
from grounded_video_llm_amd import engine as E, lib as L  # noqa: E402
import attn_plan as A  # noqa: E402
import decode_attn_ref as R  # noqa: E402
from attn_ref import SENT, _bits  # noqa: E402
from decode_proj_ref import xt_index  # noqa: E402

EXACT, BOUNDED = R.exact_cases(), R.bounded_cases()
TICKET_FILL = 0x5a5a5a5
GUARD_ROWS = 2


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(tiny_geo(), DEV, towers=())
    yield e
    e.close()


class Workspace:
    """part: decoy records + 1024 guard words; counters: zero tickets + 64 guard words"""

    def __init__(self, c):
        self.n, self.nt = c.B * c.H * c.nsplit * (c.D + 2), c.B * c.H
        self.part = R.decoy_part(c, extra=1024, device=DEV)
        self.counters = torch.cat([torch.zeros(self.nt, dtype=torch.int32), torch.full((64,), TICKET_FILL, dtype=torch.int32)]).to(DEV)

    def check(self, c, what, fresh=True):
        assert bool((self.counters[:self.nt] == 0).all()), f"{what}: {int((self.counters[:self.nt] != 0).sum())} tickets are not zero after the launch"
        assert bool((self.counters[self.nt:] == TICKET_FILL).all()), f"{what}: words behind the tickets written"
        assert bool((self.part[self.n:] == SENT).all()), f"{what}: words behind [batch][H][nsplit][D + 2] written"
        if fresh:                                      # the records a sequence does not use (all of them when it has one split) are still the decoys
            rec = self.part[:self.n].view(c.B, c.H, c.nsplit, c.D + 2)
            for b, Lb in enumerate(c.lens):
                ns = R.split_rule(Lb, c.nsplit)[1]
                lo = 0 if ns == 1 else ns
                stale = rec[b, :, lo:]
                assert bool((stale[..., c.D] == R.DECOY_M).all()) and bool((stale[..., :c.D] == R.DECOY_ACC).all()), f"{what}: sequence {b} ({ns} splits) wrote a record it does not own"


def launch(eng, c, cpb=0, gsplit=0, hpb=0, out_tiled=0, pad=False, ws=None, fresh=True, what=""):
    """ONE launch of gvl_op_decode_attention -> out bf16 [B, H * Dr]; the guards and the workspace discipline are asserted here, for every launch of this file"""
    what = what or f"{c} cpb {cpb} gsplit {gsplit} hpb {hpb} tiled {out_tiled} pad {pad}"
    B, H, D, Dr = c.B, c.H, c.D, c.Dr
    cols = H * Dr
    q_stride = H * D + (16 if pad else 0)
    q = torch.full((B, q_stride), float("nan"), dtype=bf, device=DEV)
    q[:, :H * D] = c.q.view(B, H * D)
    ws = ws or Workspace(c)
    if out_tiled:
        out_stride, n_out = cols, 16 * ((cols + 31) // 32) * 32
        out = torch.full((n_out + 256,), SENT, dtype=bf, device=DEV)
    else:
        out_stride = cols + (R.GUARD_COLS if pad else 0)
        out = torch.full((B + GUARD_ROWS, out_stride), SENT, dtype=bf, device=DEV)
    c.last = (out, ws)
    eng.op_decode_attention(q=q, Kt=c.Kt, Vt=c.Vt, tables=c.tables, pos=c.pos, part=ws.part, counters=ws.counters, out=out, q_stride=q_stride, n_pages=c.n_pages,
                            table_stride=c.table_stride, out_stride=out_stride, out_tiled=out_tiled, batch=B, H=H, KV=c.KV, D=D, Dout=Dr, nsplit=c.nsplit, hpb=hpb, cpb=cpb,
                            gsplit=gsplit, scale=c.scale)
    torch.cuda.synchronize()
    ws.check(c, what, fresh)
    if out_tiled:                                      # placement: the tiled index that decode_proj_ref states; every other slot keeps its fill
        idx = torch.stack([xt_index(b, torch.arange(cols)) for b in range(B)]).to(DEV)
        rows = out[idx]
        rest = torch.ones(out.shape, dtype=torch.bool, device=DEV)
        rest[idx.flatten()] = False
        assert bool((out[rest] == SENT).all()), f"{what}: tile-order slots of absent sequences / columns, or words behind the tile, written"
    else:
        rows = out[:B, :cols]
        assert bool((out[B:] == SENT).all()) and bool((out[:B, cols:] == SENT).all()), f"{what}: guard rows / columns of out written"
    return rows.contiguous()


def shape_of(c, e):
    return dict(cpb=e["cpb"], gsplit=R.min_gsplit(c, e["cpb"]) if e["gsplit_min"] else 0, hpb=e["hpb"], out_tiled=e["out_tiled"], pad=e["pad"])


def plan_of(c, s):
    (l,) = A.plans([A.decode_line(H=c.H, KV=c.KV, D=c.D, nsplit=c.nsplit, batch=c.B, hpb=s["hpb"], cpb=s["cpb"], gsplit=s["gsplit"])])
    assert l is not None, f"{c} {s}: refused by the plan"
    return l


# ---- exact family --------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_list_reaches_exactly_the_twelve_instantiations_of_the_shipped_build():
    reached, odd_units = set(), set()
    for e in EXACT + BOUNDED:
        c = R.Case("plan", e["lens"], e["H"], e["KV"], e["Dr"], 1.0, R.NSPLIT, "cpu")
        s = shape_of(c, e)
        l = plan_of(c, s)
        assert A.kernel_of(l) == R.GEOS[e["geo"]][4], f"{c} {s}: planned {A.kernel_of(l)}"
        reached.add(A.kernel_of(l))
        if l.family == A.HEAD and l.t1 == 1 and (c.KV * l.gsplit * l.batch) % 8:
            odd_units.add(e["geo"])                     # the XCD-aware grid with a last row of 8 that is partly empty
    assert reached == R.REACHABLE, f"the list misses {sorted(R.REACHABLE - reached)} / reaches unexpected {sorted(reached - R.REACHABLE)}"
    assert reached <= A.lists() and odd_units == {18, 19, 20}


@pytest.mark.parametrize("geo", range(len(R.GEOS)))
def test_onehot_cases_bit_for_bit(eng, geo):
    n = 0
    for e in (e for e in EXACT if e["geo"] == geo):
        c = R.onehot_case(e["lens"], e["H"], e["KV"], e["Dr"], e["seed"], share=e["share"], device=DEV)
        s = shape_of(c, e)
        pages = {(b, p): False for b, Lb in enumerate(c.lens) for p in range((Lb + 63) // 64)}
        for i, t in enumerate(R.target_sets(c)):
            c.set_targets(t)
            what = f"{c} {s} [{A.kernel_of(plan_of(c, s))}] target set {i}"
            msg = R.onehot_mismatch(launch(eng, c, what=what, **s), c, what)
            assert msg is None, msg
            for b in range(c.B):
                for x in t[b].tolist():
                    pages[(b, x // 64)] = True
            n += 1
        assert all(pages.values()), f"{c}: pages {[k for k, v in pages.items() if not v]} were nobody's target"
    print(f"[parity] decode attention one-hot {R.GEOS[geo][:4]} {R.GEOS[geo][4]}: {n} launches, every one bit for bit")


def test_a_shorter_context_right_after_a_longer_one_on_the_same_workspace(eng):
    """the second launch finds the longer context's records in the slots it does not use (and everything else the first one left): it must read its own ns only"""
    for H, KV, Dr, hpb in ((4, 4, 64, 0), (8, 2, 64, 0), (8, 2, 96, 2), (32, 1, 64, 0)):
        long = R.onehot_case([4097, 8256, 833], H, KV, Dr, 71, device=DEV)
        short = R.onehot_case([257, 65, 700], H, KV, Dr, 72, device=DEV)
        ws = Workspace(long)
        for c in (long, short, long):
            msg = R.onehot_mismatch(launch(eng, c, hpb=hpb, ws=ws, fresh=False), c, f"{c} on a used workspace")
            assert msg is None, msg


def test_onehot_with_page_offsets_beyond_2_to_the_31_elements(eng):
    """K and V^T pools of just over 2^31 elements each, uninitialised; the tables point at the last pages: every element offset is above 2^31.  One geometry per kernel
    family (per-head grid, grouped-query, XCD-aware grid), all on KV = 2, D = 64: the same pools"""
    n_pages = (1 << 31) // (2 * 64 * 64) + 16
    pools = (torch.empty((n_pages, 2, 64, 64), dtype=bf, device=DEV), torch.empty((n_pages, 2, 64, 64), dtype=bf, device=DEV))
    lens = [257, 65]
    T = sum((x + 63) // 64 for x in lens) + len(lens)
    for H, want in ((2, ("head", 64, 0)), (4, ("gqa", 64, 4, 1)), (34, ("head", 64, 1))):
        c = R.onehot_case(lens, H, 2, 64, 5, device=DEV, pools=pools, first_page=n_pages - T)
        assert int(c.tables.min()) * 2 * 64 * 64 >= 1 << 31 and A.kernel_of(plan_of(c, dict(hpb=0, cpb=0, gsplit=0))) == want
        for i, t in enumerate(R.target_sets(c)):
            c.set_targets(t)
            msg = R.onehot_mismatch(launch(eng, c), c, f"{c} above 2^31, target set {i}")
            assert msg is None, msg


# ---- bounded family ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(len(BOUNDED)))
def test_bounded_cases_inside_the_elementwise_bound(eng, n):
    e = BOUNDED[n]
    c = R.bounded_case(e["kind"], e["lens"], e["H"], e["KV"], e["Dr"], e["seed"], device=DEV)
    s = shape_of(c, e)
    out = launch(eng, c, **s)
    ref, bound, Abs = R.elementwise_bound(c)
    msg, worst = R.bound_violations(out, ref, bound, c, f"{c} {s} [{A.kernel_of(plan_of(c, s))}]")
    print(f"[parity] decode attention bounded {e['kind']} {R.GEOS[e['geo']][:4]} {R.GEOS[e['geo']][4]}: worst err / bound {worst:.3f}")
    assert msg is None, msg


# ---- bit identity --------------------------------------------------------------------------------------------------------------------------------------------------
def sub_batch(c, order):
    """the sequences `order` of case c as a case of their own, on the same pools"""
    d = copy.copy(c)
    d.lens, d.B = [c.lens[b] for b in order], len(order)
    idx = torch.tensor(order, device=DEV)
    d.q, d.tables, d.pos = c.q[idx].contiguous(), c.tables[idx].contiguous(), c.pos[idx].contiguous()
    return d


@pytest.mark.parametrize("geo", R.BOUNDED_GEOS)
def test_no_launch_shape_changes_an_output_bit(eng, geo):
    H, KV, Dr, hpb, _ = R.GEOS[geo]
    c = R.bounded_case("plain", [1025, 65, 4097, 257, 8256], H, KV, Dr, 40 + geo, device=DEV)
    base = launch(eng, c)
    G = H // KV
    hpbs = [h for h in range(1, G + 1) if G % h == 0] if 1 < G <= 16 else [0]
    i = 0
    for cpb in R.CPBS:
        for gs in (0, R.min_gsplit(c, cpb)):
            s = dict(cpb=cpb, gsplit=gs, hpb=hpbs[i % len(hpbs)], out_tiled=i % 2, pad=i % 3 == 0)
            i += 1
            assert torch.equal(_bits(launch(eng, c, **s)), _bits(base)), f"{c} {s} [{A.kernel_of(plan_of(c, s))}]: not bit-identical to the default launch shape"
    for h in hpbs:
        assert torch.equal(_bits(launch(eng, c, hpb=h)), _bits(base)), f"{c} hpb {h}: not bit-identical to the default launch shape"
    assert torch.equal(_bits(launch(eng, c)), _bits(base)), f"{c}: a repeated launch differs"
    for b in range(c.B):                               # a sequence alone against the same sequence in the batch
        assert torch.equal(_bits(launch(eng, sub_batch(c, [b]))[0]), _bits(base[b])), f"{c}: sequence {b} alone differs from slot {b} of the batch"
    order = [3, 0, 4, 2, 1]                            # ... and at another slot
    assert torch.equal(_bits(launch(eng, sub_batch(c, order))), _bits(base[order])), f"{c}: a sequence's result depends on its slot in the batch"


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_a_good_launch_follows(eng):
    c = R.onehot_case([257, 65], 4, 2, 64, 9, device=DEV)
    assert R.onehot_mismatch(launch(eng, c), c) is None
    good = dict(q=c.q.view(2, 256).contiguous(), Kt=c.Kt, Vt=c.Vt, tables=c.tables, pos=c.pos, q_stride=256, n_pages=c.n_pages, table_stride=c.table_stride, out_stride=256,
                out_tiled=0, batch=2, H=4, KV=2, D=64, Dout=64, nsplit=16, hpb=0, cpb=0, gsplit=0, scale=1.0)
    tab_hi, tab_neg = c.tables.clone(), c.tables.clone()
    tab_hi[0, 4], tab_neg[1, 1] = c.n_pages, -1
    beyond = c.tables.clone()
    beyond[1, 2:] = c.n_pages + 5                      # entries BEHIND a sequence's pages are never read: no refusal
    refused = {
        "the plan: H % KV": dict(KV=3), "the plan: head dim": dict(D=80, Dout=80), "the plan: nsplit 17": dict(nsplit=17), "the plan: nsplit 0": dict(nsplit=0),
        "batch 17": dict(batch=17), "batch 0": dict(batch=0),
        "position -1": dict(pos=torch.tensor([256, -1], dtype=torch.int32, device=DEV)),
        "position behind the tables": dict(pos=torch.tensor([c.table_stride * 64, 64], dtype=torch.int32, device=DEV)),
        "page n_pages": dict(tables=tab_hi), "page -1": dict(tables=tab_neg),
        "gsplit * cpb below the split count": dict(gsplit=1, cpb=1),
        "Dout > D": dict(Dout=65), "Dout 0": dict(Dout=0), "q_stride short": dict(q_stride=248), "out_stride short": dict(out_stride=255),
        "no workspace": dict(part=None),
    }
    for name, kw in refused.items():
        ws = Workspace(c)
        out = torch.full((2 + GUARD_ROWS, 256), SENT, dtype=bf, device=DEV)
        with pytest.raises(L.GvlError) as ei:
            eng.op_decode_attention(**dict(dict(good, part=ws.part, counters=ws.counters, out=out), **kw))
        torch.cuda.synchronize()
        assert "gvl_op_decode_attention" in str(ei.value), (name, str(ei.value))
        assert bool((out == SENT).all()), f"{name}: a refused launch wrote to the output"
        assert torch.equal(ws.part, R.decoy_part(c, extra=1024, device=DEV)) and bool((ws.counters[:ws.nt] == 0).all()), f"{name}: a refused launch wrote to the workspace"
    ws = Workspace(c)
    out = torch.full((2 + GUARD_ROWS, 256), SENT, dtype=bf, device=DEV)
    eng.op_decode_attention(**dict(good, part=ws.part, counters=ws.counters, out=out, tables=beyond, gsplit=2, cpb=1))
    torch.cuda.synchronize()
    assert R.onehot_mismatch(out[:2].contiguous(), c, "after the refusals, gsplit at the exact minimum") is None
    ws.check(c, "after the refusals")
    assert R.onehot_mismatch(launch(eng, c), c) is None
