"""tests/decode_proj_ref.py checked on its own, without a GPU: the exact cases are exact, the quantiser restatements agree with torch.float8_e4m3fn and with the
oracle's de-quantisers (on random data and on the edge set the GPU test feeds the kernels), the coverage claims hold, and the bounded references evaluated in
float32 stay well inside their own bounds.  The relocated rope cases (decode_proj_ref.rope_relocated_cases): a float32 emulation of the epilogue over sparse
pools passes, and three wrong kernels that form a page's offset in 32 bits are reported."""
import numpy as np
import pytest
import torch

import decode_proj_ref as R
import gemm_ref as G
import gvl_oracle as O

bf = torch.bfloat16

# (N, K, batch, form, w_fmt, wide) -- the shapes of the GPU test, at the small N (the arithmetic does not depend on N)
EXACT = [(50, 1024, 5, "resid", 0, False), (50, 1024, 4, "bf16", 1, False), (50, 1024, 3, "bias", 2, True), (48, 256, 5, "plain", 0, False), (52, 1024, 16, "bias", 0, False), (48, 3072, 3, "bf16", 0, False), (64, 11008, 4, "resid", 0, False),
         (64, 2048, 16, "producer", 0, False), (48, 1024, 4, "consumer", 0, False), (48, 4096, 16, "consumer", 0, False),
         (52, 5632, 16, "plain", 1, True), (52, 1024, 5, "bias", 1, True), (48, 1024, 4, "resid", 1, False), (64, 512, 16, "producer", 1, False),
         (52, 1024, 16, "plain", 2, True), (48, 2048, 3, "bias", 2, True), (48, 1024, 4, "resid", 2, False), (64, 1024, 16, "producer", 2, False)]
ROPE_GEOS = [(8, 8, 96, 128), (8, 2, 128, 128), (4, 4, 64, 64)]


@pytest.mark.parametrize("N,K,B,form,w_fmt,wide", EXACT)
def test_exact_cases_are_exact(N, K, B, form, w_fmt, wide):
    """the float64 accumulator equals the fp32 one under two different summation orders bit for bit, and every epilogue value is representable where it is formed"""
    c = R.exact_case(N, K, B, form, seed=1, w_fmt=w_fmt, wide=wide)
    acc64 = c.x.double().numpy() @ c.W.double().numpy().T
    fwd = R.recompute_fp32(c, range(K))
    rev = R.recompute_fp32(c, np.random.RandomState(0).permutation(K))
    assert (fwd.astype(np.float64) == acc64).all() and (rev.astype(np.float64) == acc64).all()
    assert fwd.tobytes() == rev.tobytes()
    # every 16-row block has a non-zero expected output for every sequence
    e = c.expect.double().abs()
    pad = (-N) % 16
    blocks = torch.nn.functional.pad(e, (0, pad)).view(B, -1, 16).sum(-1)
    assert bool((blocks > 0).all())
    # rows differ: no two sequences expect the same output
    assert len({c.expect[b].double().numpy().tobytes() for b in range(B)}) == B
    if form == "producer":
        assert bool((c.expect_sq.double() == (c.expect.double() ** 2).view(B, N // 16, 16).sum(-1)).all()) and float(c.expect_sq.max()) < 2 ** 24 * float(e[e > 0].min()) ** 2 * 4
    if form == "consumer":
        for b in range(B):                                  # the kernel's order adds the partials without rounding; another association does not
            want = K * 4.0 ** ((b + 1) % 3 - 1)
            assert float(R.sq_in_sum(c.sq_in[b].numpy(), 8)) == want
            assert float(R.sq_in_sum(c.sq_in[b].numpy(), 8, "fold")) != want


@pytest.mark.parametrize("geo", ROPE_GEOS)
@pytest.mark.parametrize("form", ["rope10", "rope01", "rope_switch"])
@pytest.mark.parametrize("w_fmt", [0, 1, 2])
def test_exact_rope_cases(geo, form, w_fmt):
    """(building the case also asserts that no expected value equals the sentinel, for every weight format)"""
    H, KV, Dr, D = geo
    N = (H + 2 * KV) * Dr
    c = R.exact_case(N, (256, 512, 1024)[w_fmt], 5, form, seed=0, w_fmt=w_fmt, rope_geo=geo)
    assert sorted(set(c.pos.tolist())) == [0, 63, 64, 130]
    # the written pages differ and no page table is the identity
    pages = [int(c.tables[b, int(c.pos[b]) >> 6]) for b in range(5)]
    assert len(set(pages)) == 5 and all(c.tables[b].tolist() != list(range(c.tables.shape[1])) for b in range(5))
    # what is not a target holds the sentinel: the D - Dr padding, every other slot, every other page
    Q = c.expect_Q.view(5, H, D)
    assert bool((Q[:, :, Dr:] == R.SENTINEL).all()) and bool((Q[:, :, :Dr] != R.SENTINEL).all())
    assert int((c.expect_Kt != R.SENTINEL).sum()) == 5 * KV * Dr == int((c.expect_Vt != R.SENTINEL).sum())
    # against the plain model order: y = x W^T, heads of Dr, rotate-half with the case's tables
    y = (c.x.double() @ c.W.double().T).view(5, H + 2 * KV, Dr)
    half = Dr // 2
    for b in range(5):
        p = int(c.pos[b])
        co, si = (c.cos_l, c.sin_l) if p + 1 > R.ROPE_SWITCH else (c.cos_s, c.sin_s)
        rot = torch.cat([-y[b, :, half:], y[b, :, :half]], -1)
        want = y[b] * torch.cat([co[p], co[p]]).double() + rot * torch.cat([si[p], si[p]]).double()
        assert bool((Q[b, :, :Dr].double() == want[:H]).all())
        page, slot = int(c.tables[b, p >> 6]), p & 63
        assert bool((c.expect_Kt[page, :, slot, :Dr].double() == want[H:H + KV]).all())
        assert bool((c.expect_Vt[page, :, :Dr, slot].double() == y[b, H + KV:]).all())
    if form == "rope_switch":                               # the boundary is visible: pos 63 and pos 64 rotate differently
        assert not bool((c.cos_s == c.cos_l).all())


def test_logical_rows_is_the_rotate_half_pairing():
    perm = R.logical_rows(3 * 8 + 8, Dr=8, n_qk=3)
    assert perm[:8].tolist() == [0, 4, 1, 5, 2, 6, 3, 7] and perm[8:10].tolist() == [8, 12] and perm[24:].tolist() == list(range(24, 32))
    assert sorted(perm.tolist()) == list(range(32))


@pytest.mark.parametrize("K,B", [(256, 1), (1024, 16), (1024, 4), (3072, 16), (5632, 16), (11008, 16), (8192, 16)])
def test_x_rows_cover_every_chunk(K, B):
    rounds = R.rounds_to_cover(K, B)
    hit = torch.zeros(K // 8, dtype=torch.bool)
    for s in range(rounds):
        x = R.exact_x(K, B, s)
        assert bool((x.float().abs().sum(1) >= 1).all()) and bool((x[:, K - 1] != 0).all())
        hit |= (x.float().view(B, K // 8, 8) != 0).any(-1).any(0)
    assert bool(hit.all())


def test_tile_order_round_trip():
    t = torch.arange(5 * 96, dtype=torch.float32).view(5, 96)
    tiled = R.to_tiled(t)
    assert tiled.numel() == 16 * 96 and bool((R.from_tiled(tiled, 5, 96) == t).all())
    assert R.xt_index(3, 41) == (1 * 64 + (1 * 16 + 3)) * 8 + 1


# ---- quantisers ------------------------------------------------------------------------------------------------------------------------------------
def _data_rows():
    g = torch.Generator().manual_seed(5)
    return (torch.randn((40, 1024), generator=g) * torch.exp2(torch.rand((40, 1), generator=g) * 30 - 15)).to(bf)


@pytest.mark.parametrize("which", ["random", "edges"])
def test_fp8_restatement_matches_torch_float8_and_the_oracle(which):
    W = _data_rows() if which == "random" else R.fp8_edge_rows()
    deq, s, _ = R.fp8_quant(W)
    w = W.double().numpy()
    assert ((np.abs(w).max(1) <= 448 * s) & ((np.abs(w).max(1) > 224 * s) | (np.abs(w).max(1) == 0))).all() and (np.log2(s) % 1 == 0).all()
    rt = (torch.from_numpy(w / s[:, None]).float().to(torch.float8_e4m3fn).double().numpy()) * s[:, None]
    assert (deq == rt).all() and (np.signbit(deq) == np.signbit(w)).all()
    assert (deq == O.fp8_pow2_dequant(W).double().numpy()).all()
    if which == "edges":                                    # the edge set holds what it claims
        t = np.abs(w) / s[:, None]
        assert (np.abs(w).max(1) == 448 * s).sum() >= 3 and (t == 2.0 ** -10).any() and (t == 3 * 2.0 ** -10).any()     # exact maxima; sub-normal ties
        mx = set(np.abs(w).max(1).tolist())
        for k in (-12, 0, 12):                              # 448 * 2^k, its bf16 neighbours on each side, and the same at 224 * 2^k
            for m, sc in ((446, 1), (448, 1), (450, 2), (223, 0.5), (224, 0.5), (225, 1)):
                assert m * 2.0 ** k in mx, (m, k)
                assert s[np.abs(w).max(1) == m * 2.0 ** k].tolist()[0] == sc * 2.0 ** k


@pytest.mark.parametrize("which", ["random", "edges"])
def test_mxfp4_restatement_matches_the_oracle(which):
    W = _data_rows() if which == "random" else R.mxfp4_edge_rows()
    deq, _, e8 = R.mxfp4_quant(W)
    assert (deq == O.mxfp4_dequant(W).double().numpy()).all()
    # from the definition: every de-quantised value is a grid point times the block's scale and no other grid point is closer
    N, K = W.shape
    w = W.double().numpy().reshape(N, K // 32, 32)
    X = np.ldexp(1.0, e8.astype(np.int64) - 127)[..., None]
    live = (e8 > 0)[..., None] & np.ones_like(w, dtype=bool)
    d = np.abs(deq.reshape(w.shape))
    grid = R.E2M1[None, :] * X[..., None]
    best = np.abs(np.abs(w)[..., None] - grid).min(-1)
    assert (np.abs(np.abs(w) - d)[live] == best[live]).all() and (deq.reshape(w.shape)[~live] == 0).all()
    m = np.abs(w).max(2)
    assert ((m[e8 > 0] >= 4 * X[e8 > 0, 0]) & (m[e8 > 0] < 8 * X[e8 > 0, 0])).all()
    if which == "edges":
        t = (np.abs(w) / X)[live]
        for tie in R.E2M1_TIES:
            assert (t == tie).any()
        assert ((m > 0) & (e8 == 0)).any() and (m == 0).any()                   # tiny blocks that become zeros; all-zero blocks
        words = R.mxfp4_scale_words(e8)
        assert words.shape == ((N + 15) // 16, K // 128, 16) and int(words[0, 1, 3]) == int.from_bytes(bytes(e8[3, 4:8].tolist()), "little")


def test_e2m1_ties_go_to_the_even_code():
    t = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 0.2500001, 0.7499999, 6.0, 100.0, 0.0])
    assert R.e2m1_code(t).tolist() == [0, 2, 2, 4, 4, 6, 6, 1, 1, 7, 7, 0]


def test_quantising_an_exact_case_is_the_identity():
    for w_fmt in (1, 2):
        for wide in (False, True):
            c = R.exact_case(52, 1024, 4, "plain" if wide else "bf16", seed=3, w_fmt=w_fmt, wide=wide)
            assert bool((R.quant(c.W, w_fmt) == c.W).all())
            if w_fmt == 1:
                assert len(set(c.scale.tolist())) >= 3
            else:
                assert len(set(c.e8.reshape(-1).tolist())) >= (8 if wide else 2)


# ---- bounded references: float32 evaluation inside a fraction of the bound --------------------------------------------------------------------------
def _rb(t):
    return t.to(bf).float()


@pytest.mark.parametrize("K,w_fmt", [(K, f) for K in (256, 1024, 4096) for f in (0, 1, 2) if K % (32, 512, 1024)[f] == 0])
def test_norm_prologue_reference_in_fp32(K, w_fmt):
    x, W, Wq = R.bounded_data(48, K, 4, 11, w_fmt)
    nw = (torch.randn(K, generator=torch.Generator().manual_seed(3)) * 0.1 + 1.0).to(bf)
    ref, bound = R.norm_prologue_bound(x, nw, 1e-5, Wq)
    xf = x.float()
    rs = torch.rsqrt((xf * xf).sum(1, keepdim=True) / K + 1e-5)
    got = _rb(nw.float() * _rb(xf * rs)) @ Wq.float().T
    r, bad = R.max_ratio(got, ref, bound)
    print(f"norm prologue K={K} w_fmt={w_fmt}: fp32 emulation max err / bound {r:.3f}, bound / scale {float((bound / ref.abs().max()).max()):.2e}")
    assert bad == 0 and r < 0.5


@pytest.mark.parametrize("w_fmt", [0, 1, 2])
def test_swiglu_reference_in_fp32(w_fmt):
    x, W, Wq = R.bounded_data(2 * 52, 1024, 5, 12, w_fmt)
    ref, bound = R.swiglu_bound(x, Wq)
    v = _rb(x.float() @ Wq.float().T)
    g, u = v[:, 0::2], v[:, 1::2]
    got = (u * _rb(g * torch.sigmoid(g))).to(bf)
    r, bad = R.max_ratio(got, ref, bound)
    assert bad == 0 and r < 0.5


@pytest.mark.parametrize("K", [512, 1024, 3072, 4096])
def test_chain_reference_in_fp32(K):
    g = torch.Generator().manual_seed(K)
    a, W1, _ = R.bounded_data(K, 256, 4, 13)
    resid = (torch.randn((4, K), generator=g) * 2).to(bf)
    gamma = (torch.randn(K, generator=g) * 0.1 + 1.0).to(bf)
    W2 = (torch.randn((48, K), generator=g) * K ** -0.5).to(bf)
    Wf = (W2.float() * gamma.float()[None, :]).to(bf)
    h, sq = R.producer_bound(a, W1, resid)
    ref, bound = R.consumer_bound(h, sq, Wf, 1e-5)
    hf = (resid.float() + _rb(a.float() @ W1.float().T)).to(bf)
    sqf = (hf.float() ** 2).view(4, K // 16, 16).sum(-1)
    assert R.max_ratio(hf, h.x, h.e)[1] == 0 and R.max_ratio(sqf, sq.x, sq.e)[1] == 0
    got = (hf.float() @ Wf.float().T) * torch.rsqrt(sqf.sum(1, keepdim=True) / K + 1e-5)
    r, bad = R.max_ratio(got, ref, bound)
    assert bad == 0 and r < 0.5
    # and the chain is the RMSNorm it replaces, up to the folded weight's rounding: float64 rmsnorm(resid + y) W2^T
    full = (h.x * torch.rsqrt((h.x ** 2).mean(1, keepdim=True) + 1e-5) * gamma.double()[None, :]) @ W2.double().T
    assert float((ref - full).abs().max() / full.abs().max()) < 2e-2


@pytest.mark.parametrize("geo", ROPE_GEOS)
def test_rope_reference_in_fp32(geo):
    H, KV, Dr, D = geo
    N = (H + 2 * KV) * Dr
    x, W, Wq = R.bounded_data(N, 256, 4, 14)
    tabs = R.longrope_tables(132, Dr)
    pos = torch.tensor([0, 63, 64, 130])
    q, k, v = R.rope_bound(x, Wq, geo, pos, tabs, 64)
    y = _rb(x.float() @ Wq.float().T).view(4, H + 2 * KV, Dr)
    half = Dr // 2
    for b in range(4):
        p = int(pos[b])
        co, si = (tabs[2][p], tabs[3][p]) if p >= 64 else (tabs[0][p], tabs[1][p])
        x1, x2 = y[b, :H + KV, :half], y[b, :H + KV, half:]
        o = torch.cat([(_rb(x1 * co) + _rb(-x2 * si)), (_rb(x2 * co) + _rb(x1 * si))], -1).to(bf)
        r, bad = R.max_ratio(o[:H], q.x[b], q.e[b])
        assert bad == 0 and r < 0.6
        assert R.max_ratio(o[H:], k.x[b], k.e[b])[1] == 0 and R.max_ratio(y[b, H + KV:].to(bf), v.x[b], v.e[b])[1] == 0
    assert not bool((tabs[0][100] == tabs[2][100]).all())


# ---- the relocated rope cases ----------------------------------------------------------------------------------------------------------------------------------------
RELOCATED = R.rope_relocated_cases()


def test_the_relocated_rope_cases_are_what_the_issue_of_page_offsets_needs():
    hi = [r for r in RELOCATED if r[6] == 31]
    assert sorted(r[6] for r in RELOCATED) == [30] + [31] * len(hi)
    assert {r[4] for r in hi if r[5] == 1} == {1, 2, 4} and 16 in {r[4] for r in hi if r[5] == 0} and {r[2] for r in hi if r[5] == 0} == {0, 1, 2} and all(r[2] == 0 for r in hi if r[5] == 1)
    assert {r[0] for r in RELOCATED} == set(ROPE_GEOS) and {r[1] for r in RELOCATED} == {"rope10", "rope01", "rope_switch"}
    for r in RELOCATED:
        geo, form, w_fmt, K, B, path, k = r
        c = R.rope_relocated_case(*r)
        small = R.exact_case(c.N, K, B, form, seed=0, w_fmt=w_fmt, rope_geo=geo)
        pe = geo[1] * 64 * geo[3]
        written = [int(c.tables[b, int(c.pos[b]) >> 6]) for b in range(B)]
        assert c.page_elems == pe and c.n_pages == R.POOL_ELEMS // pe == c.kw["n_pages"] and c.page0 + c.win <= c.n_pages and (c.page0 - 1) * pe < 1 << k
        assert int(c.tables.min()) * pe >= 1 << k and min(written) * pe >= 1 << k and (k == 31 or (int(c.tables.max()) + 1) * pe * 2 <= 1 << 32)
        assert torch.equal(c.tables - c.page0, small.tables) and torch.equal(c.pos, small.pos) and small.page0 == 0 and small.n_pages == small.win == c.win
        for name in ("expect_Q", "expect_Kt", "expect_Vt"):   # the expectation does not depend on first_page
            assert torch.equal(getattr(c, name).view(torch.int16), getattr(small, name).view(torch.int16))


@pytest.mark.parametrize("n", range(len(RELOCATED)))
def test_page_offsets_formed_in_32_bits_are_caught_on_every_relocated_rope_case(n):
    """the float32 emulation over sparse pools passes; a page offset taken mod 2^31 elements or mod 2^32 bytes is reported on every case above 2^31 elements.  On the
    case above 2^30 those two ARE the identity (every offset is below 2^31 elements = 2^32 bytes) -- what that placement catches is the SIGNED 32-bit byte offset"""
    r = RELOCATED[n]
    c = R.rope_relocated_case(*r)
    ok = R.rope_emulate(c)
    assert R.rope_mismatch(c, ok) is None and len(ok["Kt"]) == c.batch == len(ok["Vt"])
    for mut in R.MUTATIONS:
        got = R.rope_emulate(c, mut)
        msg = R.rope_mismatch(c, got)
        if r[6] == 30 and mut != "page_byte_int32":
            assert msg is None
            continue
        assert msg is not None and "Kt: page" in msg and "Vt: page" in msg and "not written" in msg and "written outside pages" in msg and "Q differs" not in msg, (mut, msg)
        assert all(k[0] == "stray" and k[1] + c.page_elems <= c.page0 * c.page_elems for k in got["Kt"]), "the wrapped writes land in front of the case's pages"
    small = R.exact_case(c.N, r[3], r[4], r[1], seed=0, w_fmt=r[2], rope_geo=r[0])
    for mut in (None,) + R.MUTATIONS:                         # on the small pools the three are the identity
        assert R.rope_mismatch(small, R.rope_emulate(small, mut)) is None
