"""-m gpu: the paged forms of attn_fwd_kernel (gvl_attn.hip) behind a cached prefix, through gvl_op_prefill_attention on caller-owned pages -- a block table with qpos0 / Sk,
the ragged grid (VL = 1) and the ragged-extend grid (VL = 2, gvl_launch_attention_ext) -- against tests/prefill_attn_ref.py.  test_gpu_attn_exact.py runs qpos0 = Sk = 0 on
implicit pages only; the model-level tests see these forms through goldens at model tolerances and compare forms that share the address arithmetic with each other.

  pools          built by the reference on the host (NOT by gvl_op_qkv_post: a fault there can neither mask nor mimic one here): pages no table names are NaN, K slots >= Sk
                 of a last partial page are NaN, V^T slots >= Sk are +-1e30, tables are permuted and carry a spare entry that is no page; Q is followed by NaN rows.
  exact cases    one-hot attention (prefill_attn_ref.onehot_case): the output must equal the target's V row BIT FOR BIT.  Targets: the last visible key qpos0 + i, key 0, the
                 first key of the query's own tile, the last cached key qpos0 - 1, the first new key qpos0, a hash over all visible keys (non-causal: last / perm / edges).
                 A failure names member, query block, wave, key tile with its page and the key whose V row came out.
  bounded cases  attn_ref's KINDS over the longer context against the float64 softmax: ZERO elements outside attn_ref.elementwise_bound (per visible key count; no new constant).
  shapes         (qpos0, S) = (64, 1) (64, 31) (64, 33) (64, 64) (64, 65) (128, 129) (192, 130) (0, 130) (960, 65), a causal case with 70 keys beyond every query and a
                 non-causal one with Sk > S; D 64 / 96 / 128 with Dout 64 / 32 / 80 / 128, (H, KV) (4, 4) (4, 2) (8, 1), B 1 / 2, ring 0 / 2 / 3; groups of 1 / 2 / 8
                 members of 1 / 65 / 128 / 129 / 31 rows, ragged and ragged-extend with prefixes 0 / 64 / 192, one where two members share their prefix pages.
  bit identity   a group member against its own single-sequence launch at (qpos0, Sk) = (vl_pos0[u], vl_pos0[u] + S_u); the all-zero extend group against the VL = 1 launch;
                 ring 0 / 2 / 3.
  every launch   160 sentinel guard rows behind O.
  refusals       what the plans refuse, a page outside the pools, a table shorter than the key tiles read: nothing written.
  above 2^31     prefill_attn_ref.relocated_cases(): cases of the lists on pages whose element offsets inside 4.3 GB all-NaN pools lie above 2^31 (one: above 2^30,
                 where the byte offsets pass 2^31) -- the same expectations, the pools unchanged (checked whole, on the device), bit-identical to the case at first_page = 0.
  joined         gvl_op_qkv_post then gvl_op_prefill_attention on the same buffers for one extend group: page layout, D padding and 64-slot pages of the two contracts meet.
test_prefill_attn_ref_cpu.py proves on these lists that twelve wrong kernels are reported by the comparisons used here.

Largest err / bound observed on an MI355X (the assertion is zero elements outside the bound, never a ratio of these):
  block table with qpos0 / Sk   late_heavy 0.824, early_heavy 0.761, spike 0.706, scaled_rows 0.854, plain 0.800
  ragged / ragged-extend        D 64: 0.784, D 64 Dout 32: 0.797, D 96 Dout 80: 0.902, D 128: 0.856
The exact families: zero differing bits in 252 + 222 launches.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, bf, big_pool_pair, count_other, tiny_geo  # noqa: E402
from grounded_video_llm_amd import engine as E, lib as L  # noqa: E402
import prefill_attn_ref as P  # noqa: E402
from attn_ref import SENT, _bits  # noqa: E402

EXACT, GROUPS_EXACT, BOUNDED, GROUPS_BOUNDED = P.exact_cases(), P.group_cases("exact"), P.bounded_cases(), P.group_cases("bounded")


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(tiny_geo(), DEV, towers=())
    yield e
    e.close()


def fields(c, O, ring=None):
    kw = dict(Q=c.Q, Kt=c.Kt, Vt=c.Vt, O=O, B=c.B, H=c.H, KV=c.KV, S=c.S, D=c.D, Dout=c.Dr, Sk=c.Sk, qpos0=c.qpos0, scale=c.scale, causal=c.causal,
              ring=c.ring if ring is None else ring, n_pages=c.n_pages, ext=int(c.form == "ext"))
    if c.form == "single":
        kw.update(block_table=c.block_table, max_pages=c.block_table.shape[1])
    else:
        kw.update(vl_n=len(c.members), vl_rows=[m.row0 for m in c.members] + [c.rows], vl_tables=c.tables, vl_pos0=[m.qpos0 for m in c.members])
    return kw


def launch(eng, c, ring=None, what=""):
    """ONE launch -> O bf16 [rows, H Dout]; the 160 guard rows are asserted here, for every launch of this file"""
    O = torch.full((c.rows + P.GUARD_ROWS, c.H * c.Dr), SENT, dtype=bf, device=DEV)
    eng.op_prefill_attention(**fields(c, O, ring))
    torch.cuda.synchronize()
    assert bool((O[c.rows:] == SENT).all()), f"{what or c}: guard rows behind O written"
    return O[:c.rows]


# ---- exact family --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,Dout", P.DGEOS)
def test_onehot_behind_a_prefix_bit_for_bit(eng, D, Dout):
    n = 0
    for s in (s for s in EXACT if (s["D"], s["Dout"]) == (D, Dout)):
        c = P.make(s, DEV)
        msg = P.onehot_mismatch(launch(eng, c), c)
        assert msg is None, msg
        n += 1
    assert n >= 60
    print(f"[parity] prefill attention one-hot, block table with qpos0 / Sk, D {D} Dout {Dout}: {n} launches, every one bit for bit")


@pytest.mark.parametrize("D,Dout", P.DGEOS)
def test_onehot_ragged_and_ragged_extend_groups_bit_for_bit(eng, D, Dout):
    n = 0
    for s in (s for s in GROUPS_EXACT if (s["D"], s["Dout"]) == (D, Dout)):
        c = P.make(s, DEV)
        msg = P.onehot_mismatch(launch(eng, c), c)
        assert msg is None, msg
        n += 1
    assert n >= 54
    print(f"[parity] prefill attention one-hot, ragged / ragged-extend groups, D {D} Dout {Dout}: {n} launches, every one bit for bit")


# ---- bounded family ------------------------------------------------------------------------------------------------------------------------------------------------
def bounded_sweep(eng, specs, what):
    worst = 0.0
    for s in specs:
        c = P.make(s, DEV)
        ref, bound = P.elementwise_bound(c)
        msg, w = P.bound_violations(launch(eng, c), ref, bound, c)
        print(f"[parity] prefill attention bounded {c}: worst err / bound {w:.3f}")
        assert msg is None, msg
        worst = max(worst, w)
    print(f"[parity] prefill attention bounded, {what}: {len(specs)} launches, zero elements outside the bound, largest err / bound {worst:.3f}")


@pytest.mark.parametrize("kind", P.KINDS)
def test_bounded_behind_a_prefix_inside_the_elementwise_bound(eng, kind):
    specs = [s for s in BOUNDED if s["kind"] == kind]
    assert len(specs) == 11
    bounded_sweep(eng, specs, f"block table with qpos0 / Sk, {kind}")


@pytest.mark.parametrize("D,Dout", P.DGEOS)
def test_bounded_groups_inside_the_elementwise_bound(eng, D, Dout):
    specs = [s for s in GROUPS_BOUNDED if (s["D"], s["Dout"]) == (D, Dout)]
    assert len(specs) == 9
    bounded_sweep(eng, specs, f"ragged / ragged-extend groups, D {D} Dout {Dout}")


# ---- bit identity --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,Dout", P.DGEOS)
def test_a_group_member_is_bit_identical_to_its_own_single_sequence_launch(eng, D, Dout):
    n = 0
    for s in (s for s in GROUPS_BOUNDED if (s["D"], s["Dout"]) == (D, Dout)):
        c = P.make(s, DEV)
        whole = launch(eng, c)
        for u, m in enumerate(c.members):
            d = P.single_launch_of(c, u)
            assert (d.qpos0, d.Sk) == (m.qpos0, m.qpos0 + m.S)
            one = launch(eng, d)
            assert torch.equal(_bits(one), _bits(whole[m.row0:m.row0 + m.S])), f"{c}: member {u} (rows {m.S}, prefix {m.qpos0}) differs from its own single-sequence launch"
            n += 1
        if c.form == "ext" and not any(m.qpos0 for m in c.members):
            r = P.make(dict(s, form="ragged"), DEV)               # the same seed: the same data, tables and pools
            assert torch.equal(_bits(r.Q), _bits(c.Q)) and torch.equal(_bits(r.Kt), _bits(c.Kt)) and [m.table for m in r.members] == [m.table for m in c.members]
            assert torch.equal(_bits(launch(eng, r)), _bits(whole)), f"{c}: the all-zero extend group differs from the VL = 1 launch"
            n += 1
    assert n >= 30


def test_the_ring_depth_changes_no_bit(eng):
    n = 0
    for s in BOUNDED[::2]:
        c = P.make(s, DEV)
        base = launch(eng, c, ring=0)
        for ring in (2, 3):
            assert torch.equal(_bits(launch(eng, c, ring=ring)), _bits(base)), f"{c}: ring {ring} differs from ring 0"
        n += 1
    assert n >= 25


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_a_good_launch_follows(eng):
    single = P.make(dict(form="single", B=2, S=65, qpos0=64, Sk=129, H=4, KV=2, D=96, Dout=80, causal=1, ring=0, target="hash", seed=41), DEV)
    full = P.make(dict(form="single", B=1, S=65, qpos0=0, Sk=200, H=4, KV=2, D=64, Dout=64, causal=0, ring=0, target="perm", seed=42), DEV)
    group = P.make(dict(form="ext", lens=(65, 31, 129), vl_pos0=(64, 0, 192), H=4, KV=4, D=64, Dout=64, causal=1, seed=43, target="hash"), DEV)
    ragged = P.make(dict(form="ragged", lens=(65, 31, 129), vl_pos0=None, H=4, KV=4, D=64, Dout=64, causal=1, seed=44, target="hash"), DEV)

    def tab(c, r, i, v):
        t = c.block_table.clone()
        t[r, i] = v
        return t

    def vtab(c, u, i, v):
        ts = [t.clone() for t in c.tables]
        ts[u][i] = v
        return ts

    refused = [
        # what attn_plan / attn_ext_plan refuse
        ("D 80", single, dict(D=80)), ("Dout % 8", single, dict(Dout=76)), ("Dout > D", single, dict(Dout=104)), ("H % KV", single, dict(KV=3)), ("S 0", single, dict(S=0)),
        ("Sk < qpos0 + S", single, dict(Sk=128)), ("qpos0 without Sk", single, dict(Sk=0)), ("qpos0 < 0", single, dict(qpos0=-64)), ("more than 256 key tiles", full, dict(Sk=256 * 64 + 1)),
        ("ragged: not causal", ragged, dict(causal=0)), ("ragged: B 2", ragged, dict(B=2)), ("ragged: Sk", ragged, dict(Sk=200)), ("ragged: qpos0", ragged, dict(qpos0=64)),
        ("ragged: block_table", ragged, dict(block_table=ragged.tables[0], max_pages=2)), ("ragged: a member longer than S", ragged, dict(S=128)),
        ("ragged: an empty member", ragged, dict(vl_rows=[0, 65, 65, 225])), ("ragged: vl_rows[0] != 0", ragged, dict(vl_rows=[1, 65, 96, 225])), ("9 members", ragged, dict(vl_n=9)),
        ("ext: not causal", group, dict(causal=0)), ("ext: vl_pos0 % 64", group, dict(vl_pos0=[64, 0, 100])), ("ext: vl_pos0 < 0", group, dict(vl_pos0=[-64, 0, 192])),
        ("ext: a member without a table", group, dict(vl_tables=[None] + group.tables[1:], table_len=[3, 2, 7])), ("ext: no group", single, dict(ext=1)),
        ("ext: vl_rows[0] != 0", group, dict(vl_rows=[1, 65, 96, 225])), ("ext: more than 256 key tiles", group, dict(vl_pos0=[64, 0, 256 * 64])),
        # what the entry adds
        ("single: no block table", single, dict(block_table=None)), ("ring 4", single, dict(ring=4)), ("no O", single, dict(O=None)), ("n_pages 0", single, dict(n_pages=0)),
        ("page n_pages", single, dict(block_table=tab(single, 1, 2, single.n_pages))), ("page -1", single, dict(block_table=tab(single, 0, 0, -1))),
        ("non-causal: page of the last tile", full, dict(block_table=tab(full, 0, 3, full.n_pages))),
        ("group: page n_pages in the prefix", group, dict(vl_tables=vtab(group, 2, 0, group.n_pages))), ("ragged: page -1", ragged, dict(vl_tables=vtab(ragged, 1, 0, -1))),
        ("table shorter than the key tiles", single, dict(max_pages=2)), ("non-causal: table shorter than ceil(Sk / 64)", full, dict(max_pages=3)),
        ("group: table shorter", group, dict(vl_tables=[group.tables[0], group.tables[1], group.tables[2][:5].contiguous()])),
    ]
    for name, c, kw in refused:
        O = torch.full((c.rows + P.GUARD_ROWS, c.H * c.Dr), SENT, dtype=bf, device=DEV)
        with pytest.raises(L.GvlError) as ei:
            eng.op_prefill_attention(**dict(fields(c, O), **kw))
        torch.cuda.synchronize()
        assert ei.value.status == L.ERR_ARG and "gvl_op_prefill_attention" in str(ei.value), (name, str(ei.value))
        assert bool((O == SENT).all()), f"{name}: a refused launch wrote to the output"
    beyond = tab(single, 1, 3, -5)                     # the spare entry behind a sequence's tiles is never read: no refusal
    O = torch.full((single.rows + P.GUARD_ROWS, single.H * single.Dr), SENT, dtype=bf, device=DEV)
    eng.op_prefill_attention(**dict(fields(single, O), block_table=beyond))
    assert P.onehot_mismatch(O[:single.rows], single, "after the refusals") is None
    for c in (single, full, group, ragged):
        msg = P.onehot_mismatch(launch(eng, c), c)
        assert msg is None, "after the refusals: " + msg


# ---- joined: gvl_op_qkv_post writes what gvl_op_prefill_attention reads --------------------------------------------------------------------------------------------------
def test_qkv_post_then_prefill_attention_on_the_same_buffers(eng):
    """one ragged-extend group, padded head dim (80 -> 96), grouped-query.  The prefix pages come from the host; the new tokens' Q rows, K slots and V^T pages are written by
    gvl_op_qkv_post_ext from a fused qkv matrix (cos = 1, sin = 0: the rotation is the identity and exact on this data, which has no zeros) into buffers that held NaN
    there.  The attention output on them must be BIT-IDENTICAL to the one on the host-built pools, and inside the float64 bound."""
    s = dict(form="ext", lens=(65, 31, 129), vl_pos0=(64, 0, 192), H=4, KV=2, D=96, Dout=80, causal=1, seed=77, kind="plain")
    c = P.make(s, DEV)
    want = launch(eng, c)
    H, KV, D, Dr = c.H, c.KV, c.D, c.Dr
    qkv = torch.cat([torch.cat([q.reshape(m.S, H * Dr), k[m.qpos0:].reshape(m.S, KV * Dr), v[m.qpos0:].reshape(m.S, KV * Dr)], 1) for m, q, k, v in zip(c.members, c.q, c.k, c.v)])
    qkv = torch.cat([qkv, torch.full((64, qkv.shape[1]), float("nan"), dtype=bf, device=DEV)]).contiguous()
    assert bool((qkv[:c.rows] != 0).all())
    Q = torch.full_like(c.Q, float("nan"))
    Kt, Vt = c.Kt.clone(), c.Vt.clone()
    for m in c.members:                                # the pages of the new tokens: wiped
        for t in range(m.qpos0 // 64, (m.Sk + 63) // 64):
            Kt[m.table[t]], Vt[m.table[t]] = float("nan"), float("nan")
    max_pos = max(m.Sk for m in c.members)
    cos, sin = torch.ones((max_pos, Dr // 2), device=DEV), torch.zeros((max_pos, Dr // 2), device=DEV)
    eng.op_qkv_post(qkv=qkv, ld=qkv.shape[1], Q=Q, Kt=Kt, Vt=Vt, B=1, S=c.S, H=H, KV=KV, Dr=Dr, D=D, mode=2, cos=cos, sin=sin, vl_n=len(c.members),
                    vl_rows=[m.row0 for m in c.members] + [c.rows], vl_tables=c.tables, vl_pos0=[m.qpos0 for m in c.members], n_pages=c.n_pages, max_pos=max_pos, ext=1)
    torch.cuda.synchronize()
    assert torch.equal(_bits(Q[:c.rows * H * D]), _bits(c.Q[:c.rows * H * D])), "Q as gvl_op_qkv_post writes it is not the layout gvl_op_prefill_attention reads"
    for m in c.members:
        for t in range((m.Sk + 63) // 64):
            n = min(64, m.Sk - t * 64)
            pg = m.table[t]
            assert torch.equal(_bits(Kt[pg, :, :n]), _bits(c.Kt[pg, :, :n])) and torch.equal(_bits(Vt[pg, :, :, :n]), _bits(c.Vt[pg, :, :, :n])), f"member with prefix {m.qpos0}: page {pg} (tile {t})"
    c.Q, c.Kt, c.Vt = Q, Kt, Vt
    got = launch(eng, c)
    assert torch.equal(_bits(got), _bits(want)), "the attention output on the pages gvl_op_qkv_post wrote differs from the one on the host-built pages"
    ref, bound = P.elementwise_bound(c)
    msg, w = P.bound_violations(got, ref, bound, c)
    assert msg is None, msg


# ---- page offsets that need more than 32 bits ----------------------------------------------------------------------------------------------------------------------------
RELOCATED = P.relocated_cases()
NAN_BITS = 0x7FC0                                       # the bf16 NaN the pools are filled with: what torch.full(..., nan) holds


@pytest.fixture(scope="module")
def big_pools():
    """K and V^T pools of prefill_attn_ref.POOL_ELEMS (just over 2^31) bf16 elements each, 4.3 GB apiece, shared by every relocated case and freed with the module"""
    pools = big_pool_pair(P.POOL_ELEMS)
    yield pools
    pools.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n", range(len(RELOCATED)))
def test_pages_above_2_to_the_31_elements_of_the_pools(eng, big_pools, n):
    """a case of the lists on pages from the first one at or above 2^31 (the last case: 2^30) elements of 4.3 GB pools that are NaN everywhere else -- the low part never
    holds the case's data, so a wrapped read finds NaN: O against the same expectation as on the small pools (one-hot: bit for bit; dense: zero elements outside the
    float64 bound), the pools unchanged (outside the case's pages all NaN, checked whole; the case's pages as the reference wrote them), and O bit-identical to the same
    case on its small pools at first_page = 0"""
    s, k = RELOCATED[n]
    for p in big_pools:
        p.fill_(NAN_BITS)
    c = P.make_relocated(s, k, DEV, [p.view(bf) for p in big_pools])
    small = P.make(s, DEV)
    named = [m.table[t] for m in c.members for t in range((m.Sk + 63) // 64)]
    assert min(named) * c.page_elems >= 1 << k and (k == 31 or (max(named) + 1) * c.page_elems <= 1 << 31), "the pages of this case do not lie where the test says"
    assert c.Kt.data_ptr() == big_pools[0].data_ptr() and c.Vt.data_ptr() == big_pools[1].data_ptr() and c.n_pages * c.page_elems <= P.POOL_ELEMS
    got = launch(eng, c)
    if "target" in s:
        msg, what = P.onehot_mismatch(got, c), "bit for bit"
    else:
        ref, bound = P.elementwise_bound(c)
        msg, w = P.bound_violations(got, ref, bound, c)
        what = f"zero elements outside the bound, worst err / bound {w:.3f}"
    assert msg is None, msg
    lo, hi = c.page0 * c.page_elems, (c.page0 + c.win) * c.page_elems
    for name, p, mine, ref_pool in (("K", big_pools[0], c.Kt, small.Kt), ("V^T", big_pools[1], c.Vt, small.Vt)):
        bad = count_other(p, NAN_BITS, lo, hi)
        assert bad == 0, f"{c}: {bad} elements of the {name} pool outside pages {c.page0} .. {c.page0 + c.win - 1} are no longer NaN"
        assert torch.equal(_bits(mine[c.page0:c.page0 + c.win]), _bits(ref_pool)), f"{c}: the case's pages of the {name} pool changed, or were not laid out as on the small pools"
    assert torch.equal(_bits(got), _bits(launch(eng, small))), f"{c}: O differs from the same case at first_page = 0"
    print(f"[parity] prefill attention on pages {min(named)} .. {max(named)} (element offsets from {min(named) * c.page_elems}, 2^{k} = {1 << k}): {what}")
