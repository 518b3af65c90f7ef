"""-m gpu: the qkv_post family (gvl_elem.hip: qkv_post_kernel, v_transpose_kernel, qkv_post_ext_kernel, v_transpose_ext_kernel) through gvl_op_qkv_post, one launch at a time
on caller-owned tensors, against an INDEPENDENT reference (tests/qkv_post_ref.py) -- where the model-level tests see these kernels through goldens at model tolerances and
the form-against-form tests (test_gpu_extend_varlen.py, test_prefix_sharing_fork_and_extend_prefill) run the same address arithmetic on both sides.

  every launch   Q, the K pool, the V^T pool and q_rs start as a NaN-pattern sentinel and are oversized: pages no table names, 4096 guard elements behind Q, 64 behind q_rs;
                 table entries in front of and behind a sequence's new tiles are no pages at all.  The WHOLE image of every buffer is compared: what nobody may write must
                 still be the sentinel, the slots the kernels are specified to zero or one-fill are expected exactly.  qkv is the prefix of an allocation whose next 64
                 rows, and whose columns behind the row where ld is padded, are NaN.
  modes 0, 2     bit for bit (RoPE: two bf16 roundings before the add, emulated on bit patterns).
  mode 1         ZERO elements outside the float64 bound of qkv_post_ref.norm_expect (derived there, no fitted factor); q_rs against its own relative bound; pads, V^T and
                 sentinels bit for bit.
  THE list       qkv_post_ref.cases(): per geometry and mode every length 1 / 3 / 4 / 5 / 63 / 64 / 65 / 130 on implicit pages (B 1 / 3) and on a permuted table with
                 pos0 0 / 64 / 192 (Vt NULL in a quarter of them, then also pos0 % 64 != 0); ragged and ragged-extend groups of 1 / 2 / 8 members whose 4-row blocks
                 straddle two and three members.  test_qkv_post_ref_cpu.py proves on this list that seventeen wrong kernels are reported by the comparison used here.
  bit identity   a ragged / extend member against its own single-sequence launch at pos0 = vl_pos0[u]; implicit pages against an identity table.
  refusals       every refusal of the contract in include/gvl.h, with every output all-sentinel afterwards.
  above 2^31     qkv_post_ref.relocated_cases(): cases of THE list on pages whose element offsets inside 4.3 GB pools lie above 2^31 (one: above 2^30, where the byte offsets
                 pass 2^31) -- the same expectations, the rest of both pools all sentinel (checked whole, on the device), bit-identical to the case at first_page = 0.

A failure names the count, the first (buffer, page / row, head, slot, d), the member and the source row.

Largest err / bound observed on an MI355X (mode 1; the assertion is zero elements outside the bound, never a ratio of these):
  Q 1.000, Kt 1.000 in every geometry -- exact ties of the store's rounding (the product of two 8-bit significands lies halfway between two bf16 numbers about once in
  256 elements; the bound is half an ulp there and round-to-nearest meets it with equality), nothing above;  q_rs 0.005 (rsqrtf and the wave sum use a small part of
  the n 2^-24 their bound allows).  Modes 0 and 2: zero differing bits in 404 launches.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, bf, big_pool_pair, count_other, tiny_geo  # noqa: E402
from grounded_video_llm_amd import engine as E, lib as L  # noqa: E402
import qkv_post_ref as R  # noqa: E402

SPECS = R.cases()
GROUPS = sorted({(s["form"] == "single", s["geo"], s["mode"], bool(s["q_rs"])) for s in SPECS}, key=str)


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(tiny_geo(), DEV, towers=())
    yield e
    e.close()


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(DEV).view(bf)


class Buffers:
    """the device side of one launch: sentinel-filled outputs (qkv_post_ref.Images) and the uploaded operands"""

    def __init__(self, c):
        im = R.Images(c)
        self.Q, self.Kt, self.Vt = _dev16(im.Q), _dev16(im.Kt), _dev16(im.Vt)
        self.q_rs = torch.from_numpy(im.q_rs.view(np.int32)).to(DEV).view(torch.float32)
        self.qkv = _dev16(c.qkv)
        self.cos, self.sin = (torch.from_numpy(t).to(DEV) for t in (c.cos, c.sin)) if c.mode == 2 else (None, None)
        self.qn, self.kn = (_dev16(c.qn), _dev16(c.kn)) if c.mode == 1 else (None, None)
        self.block_table = torch.from_numpy(c.block_table).to(DEV) if c.block_table is not None else None
        self.vl_tables = [torch.tensor(m.table, dtype=torch.int32, device=DEV) for m in c.members] if c.form != "single" else None

    def images(self):
        torch.cuda.synchronize()
        im = type("Got", (), {})()
        for name in ("Q", "Kt", "Vt"):
            setattr(im, name, getattr(self, name).view(torch.int16).cpu().numpy().view(np.uint16))
        im.q_rs = self.q_rs.view(torch.int32).cpu().numpy().view(np.uint32)
        return im

    def untouched(self, c):
        return R.mismatch(c, self.images(), R.Expect(R.Images(c))) is None


def fields(c, b):
    """every field of gvl_qkv_post for case c on the buffers b"""
    kw = dict(qkv=b.qkv, ld=c.ld, Q=b.Q, Kt=b.Kt, Vt=b.Vt if c.vt else None, block_table=b.block_table, max_pages=c.max_pages, B=c.B, S=c.S, H=c.H, KV=c.KV, Dr=c.Dr, D=c.D,
              mode=c.mode, qn=b.qn, kn=b.kn, eps=c.eps, cos=b.cos, sin=b.sin, pos0=c.pos0, ones_row=c.ones_row, k_ones=c.k_ones, q_rs=b.q_rs if c.q_rs else None,
              n_pages=c.n_pages, max_pos=c.max_pos, ext=int(c.form == "ext"))
    if c.form != "single":
        kw.update(vl_n=len(c.members), vl_rows=[m.row0 for m in c.members] + [c.rows], vl_tables=b.vl_tables, vl_pos0=[m.pos0 for m in c.members])
    return kw


def launch(eng, c):
    b = Buffers(c)
    eng.op_qkv_post(**fields(c, b))
    return b.images()


@pytest.mark.parametrize("single,geo,mode,q_rs", GROUPS)
def test_every_case_of_the_list(eng, single, geo, mode, q_rs):
    """exact: the whole image of every buffer bit for bit; mode 1: zero elements outside the derived bound"""
    stats, n = {}, 0
    for s in SPECS:
        if (s["form"] == "single", s["geo"], s["mode"], bool(s["q_rs"])) != (single, geo, mode, q_rs):
            continue
        c = R.build(s)
        msg = R.mismatch(c, launch(eng, c), R.expect(c), stats)
        assert msg is None, msg
        n += 1
    assert n >= 8
    what = "bit for bit" if mode != 1 else "zero elements outside the bound, largest err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(stats.items()))
    print(f"[parity] qkv_post {'single' if single else 'ragged + extend'} mode {mode} {geo}{' q_rs' if q_rs else ''}: {n} launches, {what}")


@pytest.mark.parametrize("geo", R.GEOS)
def test_a_group_member_is_bit_identical_to_its_own_single_sequence_launch(eng, geo):
    n = 0
    for s in (s for s in SPECS if s["form"] != "single" and s["geo"] == geo and s["vt"] and len(s["lens"]) in (2, 8)):
        c = R.build(s)
        whole = launch(eng, c)
        for u, m in enumerate(c.members):
            d = R.single_launch_of(c, u)
            one = launch(eng, d)
            what = f"{c}: member {u} (rows {m.rows}, pos0 {m.pos0})"
            assert np.array_equal(one.Q[:d.q_elems], whole.Q[m.row0 * c.H * c.D:(m.row0 + m.rows) * c.H * c.D]), f"{what}: Q differs from its single-sequence launch"
            pages = [m.table[t] for t in range(m.pos0 >> 6, (m.pos0 + m.rows + 63) >> 6)]
            assert np.array_equal(one.Kt[pages], whole.Kt[pages]), f"{what}: K pages differ from its single-sequence launch"
            assert np.array_equal(one.Vt[pages], whole.Vt[pages]), f"{what}: V^T pages differ from its single-sequence launch"
            rest = np.setdiff1d(np.arange(c.n_pages), pages)
            assert (one.Kt[rest] == R.SENT).all() and (one.Vt[rest] == R.SENT).all() and (one.Q[d.q_elems:] == R.SENT).all(), f"{what}: the single-sequence launch wrote elsewhere"
            n += 1
    assert n >= 20


def test_implicit_pages_are_bit_identical_to_an_identity_block_table(eng):
    n = 0
    for s in (s for s in SPECS if s["form"] == "single" and not s["table"] and s["S"] in (5, 64, 130)):
        a, b = R.build(s), R.build(dict(s, table=True, identity=True))
        assert a.n_pages == b.n_pages and np.array_equal(a.qkv, b.qkv) and b.block_table[:, :(a.S + 63) // 64].reshape(-1).tolist() == list(range(a.B * ((a.S + 63) // 64)))
        x, y = launch(eng, a), launch(eng, b)
        for name in ("Q", "Kt", "Vt", "q_rs"):
            assert np.array_equal(getattr(x, name), getattr(y, name)), f"{a}: {name} differs between implicit pages and the identity table"
        n += 1
    assert n >= 50


def test_refusals_write_nothing_and_a_good_launch_follows(eng):
    single = R.build(dict(form="single", geo=(6, 2, 80, 96), mode=2, seed=901, B=2, S=65, pos0=64, table=True, vt=True, k_ones=1, ones_row=1, q_rs=False, ld_pad=16))
    plain = R.build(dict(form="single", geo=(4, 4, 64, 64), mode=0, seed=902, B=2, S=65, pos0=0, table=False, vt=True, k_ones=0, ones_row=0, q_rs=False, ld_pad=0))
    norm = R.build(dict(form="single", geo=(4, 4, 88, 96), mode=1, seed=903, B=1, S=5, pos0=0, table=False, vt=True, k_ones=1, ones_row=0, q_rs=True, ld_pad=0))
    group = R.build(dict(form="ext", geo=(4, 4, 64, 64), mode=2, seed=904, lens=(3, 65, 2), vl_pos0=(64, 0, 128), vt=True, k_ones=0, ones_row=0, q_rs=False, ld_pad=0))
    ragged = R.build(dict(form="ragged", geo=(4, 4, 64, 64), mode=2, seed=905, lens=(3, 65, 2), vl_pos0=None, vt=True, k_ones=0, ones_row=0, q_rs=False, ld_pad=0))

    def tab(c, r, i, v):
        t = c.block_table.copy()
        t[r, i] = v
        return torch.from_numpy(t).to(DEV)

    def vtab(c, u, i, v):
        ts = [torch.tensor(m.table, dtype=torch.int32, device=DEV) for m in c.members]
        ts[u][i] = v
        return ts

    one_tile = torch.tensor(group.members[1].table[:1], dtype=torch.int32, device=DEV)
    refused = [
        # what the launchers refuse
        ("Dr % 8", single, dict(Dr=76)), ("mode 2: Dr % 16", single, dict(Dr=72)), ("D % 8", single, dict(D=100)), ("D < Dr", single, dict(D=72)), ("Dr > 128", plain, dict(Dr=136, D=136, H=1, KV=1)),
        ("ld % 8", single, dict(ld=single.ld + 4)), ("ld short", single, dict(ld=single.width - 8)), ("q_rs outside mode 1", plain, dict(q_rs=True, k_ones=1, D=72)),
        ("ragged: mode", ragged, dict(mode=0)), ("ragged: B", ragged, dict(B=2)), ("ragged: pos0", ragged, dict(pos0=64)), ("ragged: 9 members", ragged, dict(vl_n=9)),
        ("ext: no group", single, dict(ext=1)), ("ext: no Vt", group, dict(Vt=None)), ("ext: block_table", group, dict(block_table=torch.zeros(8, dtype=torch.int32, device=DEV), max_pages=8)),
        ("ext: vl_pos0 % 64", group, dict(vl_pos0=[64, 0, 100])), ("ext: vl_pos0 < 0", group, dict(vl_pos0=[-64, 0, 128])), ("ext: a member without a table", group, dict(vl_tables=[None] + vtab(group, 0, 0, 0)[1:], table_len=[2, 2, 4])),
        # what the entry adds
        ("page n_pages", single, dict(block_table=tab(single, 1, 2, single.n_pages))), ("page -1", single, dict(block_table=tab(single, 0, 1, -1))),
        ("implicit pages outside the pool", plain, dict(n_pages=3)),
        ("group: page n_pages", group, dict(vl_tables=vtab(group, 2, 2, group.n_pages))), ("ragged: page -1", ragged, dict(vl_tables=vtab(ragged, 1, 1, -1))),
        ("a page named twice", ragged, dict(vl_tables=vtab(ragged, 2, 0, ragged.members[1].table[1]))),
        ("position >= max_pos", single, dict(max_pos=single.pos0 + single.S - 1)), ("group: position >= max_pos", group, dict(max_pos=129)),
        ("table shorter than ceil((pos0 + S) / 64)", single, dict(max_pages=2)), ("group: table shorter", group, dict(vl_tables=[vtab(group, 0, 0, 0)[0], one_tile, vtab(group, 0, 0, 0)[2]])),
        ("Vt with pos0 % 64", single, dict(pos0=32)), ("pos0 > 0 without a table", plain, dict(pos0=64)), ("pos0 < 0", single, dict(pos0=-64)),
        ("vl_rows[0] != 0", ragged, dict(vl_rows=[1, 3, 68, 70])), ("an empty member", ragged, dict(vl_rows=[0, 3, 3, 70])), ("a member of negative length", group, dict(vl_rows=[0, 68, 3, 70])),
        ("q_rs without k_ones", norm, dict(k_ones=0)), ("ones_row with D == Dr", plain, dict(ones_row=1)), ("k_ones with D == Dr", plain, dict(k_ones=1)),
        ("mode 1 without qn", norm, dict(qn=None)), ("mode 1 without kn", norm, dict(kn=None)), ("mode 2 without cos", single, dict(cos=None)), ("mode 3", plain, dict(mode=3)),
        ("no Kt", plain, dict(Kt=None)), ("no Q and no q_rs", plain, dict(Q=None)), ("S 0", plain, dict(S=0)), ("n_pages 0", plain, dict(n_pages=0)),
    ]
    for name, c, kw in refused:
        b = Buffers(c)
        f = fields(c, b)
        if kw.get("q_rs") is True:
            kw = dict(kw, q_rs=b.q_rs)
        with pytest.raises(L.GvlError) as ei:
            eng.op_qkv_post(**dict(f, **kw))
        assert ei.value.status == L.ERR_ARG and "qkv_post" in str(ei.value), (name, str(ei.value))
        assert b.untouched(c), f"{name}: a refused launch wrote to an output"
    for c in (single, plain, norm, group, ragged):
        msg = R.mismatch(c, launch(eng, c), R.expect(c))
        assert msg is None, "after the refusals: " + msg


# ---- page offsets that need more than 32 bits ----------------------------------------------------------------------------------------------------------------------------
RELOCATED = R.relocated_cases()


@pytest.fixture(scope="module")
def big_pools():
    """K and V^T pools of qkv_post_ref.POOL_ELEMS (just over 2^31) bf16 elements each, 4.3 GB apiece, shared by every relocated case and freed with the module"""
    pools = big_pool_pair(R.POOL_ELEMS)
    yield pools
    pools.clear()
    torch.cuda.empty_cache()


class BigBuffers(Buffers):
    """Buffers whose pools are views [n_pages][KV][64][D] of the big ones, sentinel-filled on the device before the launch"""

    def __init__(self, c, pools):
        Buffers.__init__(self, c)
        self.flat, n = pools, c.n_pages * c.page_elems
        for p in pools:
            p.fill_(R.SENT)
        self.Kt, self.Vt = pools[0][:n].view(bf).view(c.n_pages, c.KV, 64, c.D), pools[1][:n].view(bf).view(c.n_pages, c.KV, c.D, 64)
        self.win = (c.page0 * c.page_elems, (c.page0 + c.win) * c.page_elems)

    def images(self):
        torch.cuda.synchronize()
        im = type("Got", (), {})()
        im.Q = self.Q.view(torch.int16).cpu().numpy().view(np.uint16)
        for name, p, shape in (("Kt", self.flat[0], self.Kt.shape[1:]), ("Vt", self.flat[1], self.Vt.shape[1:])):   # the case's pages, as qkv_post_ref.Images holds them
            setattr(im, name, p[self.win[0]:self.win[1]].cpu().numpy().view(np.uint16).reshape((-1,) + tuple(shape)))
        im.q_rs = self.q_rs.view(torch.int32).cpu().numpy().view(np.uint32)
        return im


@pytest.mark.parametrize("n", range(len(RELOCATED)))
def test_pages_above_2_to_the_31_elements_of_the_pools(eng, big_pools, n):
    """a case of THE list on pages from the first one at or above 2^31 (the last case: 2^30) elements of 4.3 GB pools: the named pages and Q / q_rs against the same
    expectation as on the small pools (bit for bit; mode 1 inside its bound), EVERY other element of both pools still the sentinel -- the low part never holds the case's
    data, so a wrapped write cannot land on the right values -- and every buffer bit-identical to the same case on its small pools at first_page = 0"""
    s, k = RELOCATED[n]
    c, small = R.build_relocated(s, k), R.build(s)
    named = [m.table[t] for m in c.members for t in range(m.pos0 >> 6, (m.pos0 + m.rows + 63) >> 6)]
    assert min(named) * c.page_elems >= 1 << k and (k == 31 or max(named) * c.page_elems < 1 << 31), "the pages of this case do not lie where the test says"
    b = BigBuffers(c, big_pools)
    eng.op_qkv_post(**fields(c, b))
    got = b.images()
    stats = {}
    msg = R.mismatch(c, got, R.expect(c), stats)
    assert msg is None, msg
    for name, p in (("K", big_pools[0]), ("V^T", big_pools[1])):
        bad = count_other(p, R.SENT, *b.win)
        assert bad == 0, f"{c}: {bad} elements of the {name} pool outside pages {c.page0} .. {c.page0 + c.win - 1} are no longer the sentinel"
    low = launch(eng, small)
    for name in ("Q", "Kt", "Vt", "q_rs"):
        assert np.array_equal(getattr(got, name).reshape(-1), getattr(low, name).reshape(-1)), f"{c}: {name} differs from the same case at first_page = 0"
    print(f"[parity] qkv_post on pages {min(named)} .. {max(named)} (element offsets from {min(named) * c.page_elems}, 2^{k} = {1 << k}): "
          + ("bit for bit" if c.mode != 1 else "zero elements outside the bound, largest err / bound " + ", ".join(f"{a} {v:.3f}" for a, v in sorted(stats.items()))))
