"""The decode projections, form by form, through gvl_op_decode_proj: dgemm_kernel (gvl_decode.hip, path 0) and gemv_kernel (gvl_elem.hip, path 1) with every
prologue / epilogue, the three weight formats and the four quantiser kernels -- against tests/decode_proj_ref.py (checked on its own by
test_decode_proj_ref_cpu.py).

  exact      operands on which every number is representable: outputs, sums of squares, tiled copies, Q / K-page / V-page placement BIT FOR BIT, the untouched
             rest of every buffer included; column j of a batch == the same sequence alone
  quantisers every finite bf16 pattern in range of its row / block scale plus the edge set (decode_proj_ref.fp8_edge_rows / mxfp4_edge_rows): de-quantised
             weight, scales and -- through one-hot activations -- the tile stream, bit for bit against the numpy restatements
  bounded    dense data, float64 reference, per-element derived bound (decode_proj_ref: nothing fitted); the largest err / bound per form is printed
  above 2^31 decode_proj_ref.rope_relocated_cases(): rope cases of the sweep whose tables name pages above 2^31 elements (one: above 2^30) of 4.3 GB pools -- the same
             expectation, the rest of both pools all sentinel (checked whole, on the device), bit-identical to the case at first_page = 0
  refusals   every documented precondition comes back as GVL_ERR_ARG and leaves the outputs untouched

What the launchers refuse (asserted, not skipped): path 1 serves batch 1, 2, 4 only and no quantised weights, fused-norm sums or tiled buffers; sq_in needs
bf16 weights; MXFP4 needs K % 1024, FP8 K % 512; SwiGLU needs N % 4 == 0.
Not covered, because no call the launcher accepts reaches it: the `nr + 1 < N` branch of the SwiGLU epilogue (N % 4 != 0).  The scalar tail of the plain /
residual epilogue (N % 4 != 0) IS covered: N = 50 in the exact sweeps of every form and weight format, and in the norm-prologue cases.

Largest err / bound printed on an MI355X (gfx950), per bounded form (0: every element equals the rounded float64 reference -- the bound itself is 0 wherever no
bf16 tie point lies within the error interval, so these are not slack):
  swiglu      bf16 weights 0.152 (bf16 out) / 0.177 (f32 out) / 0.151 (VALU kernel); FP8 3.3e-37; MXFP4 0
  rope        Q, K pages, V pages: 0 for bf16 / FP8 / MXFP4 on the skinny GEMM and for the VALU kernel
  norm_w      bf16 7.6e-4 (skinny GEMM, one and two row blocks per workgroup alike) / 6.5e-4 (VALU kernel); FP8 1.0e-4; MXFP4 7.9e-5   (the bound is 1e-3 .. 7e-3 of the output scale: it allows every normalised
              activation whose rounding interval holds a tie to flip at once, for all K of them)
  chain       producer h 0, producer sq_out 0.094, consumer 1.1e-4
The whole file takes 14 s on that machine.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_proj_ref as R  # noqa: E402
import gemm_ref as G  # noqa: E402
from gpu_util import DEV, bf, big_pool_pair, check, count_other, tiny_geo  # noqa: E402
from grounded_video_llm_amd import engine as E, lib as L  # noqa: E402

FILL = -7776.0                                              # a bf16 number no exact case produces
FMT_K = {0: (256, 1024, 2048, 3072, 11008), 1: (512, 1024, 2048, 3072, 5632), 2: (1024, 2048, 3072)}
FMT_NAME = {0: "bf16", 1: "fp8", 2: "mxfp4"}


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(tiny_geo(), DEV, towers=())
    yield e
    e.close()


def dev(t):
    return None if t is None else t.to(DEV)


def refused(eng, W, x, outs, **kw):
    """the call must come back as ERR_ARG and leave every output tensor as it was"""
    before = [o.clone() for o in outs]
    with pytest.raises(L.GvlError) as ei:
        eng.op_decode_proj(W, x, **kw)
    assert ei.value.status == L.ERR_ARG, ei.value
    torch.cuda.synchronize()
    for o, b in zip(outs, before):
        assert torch.equal(o.view(torch.uint8), b.view(torch.uint8)), "a refused call wrote to an output"


def run_case(eng, c, path=0, variant=0, guard=0, rows=None, tiled_x=False, pools=None):
    """one call for an exact case (rows: a subset of its sequences, run as their own batch).  -> dict of the output tensors, on the CPU.  pools (rope): the flat K and
    V^T buffers to view as [c.n_pages][KV][64][D], sentinel-filled by the caller; of them the pages c.page0 .. c.page0 + c.win - 1 come back"""
    sel = list(range(c.batch)) if rows is None else rows
    B, N, f = len(sel), c.N, c.f
    kw = dict(c.kw, path=path, variant=variant)
    x = c.x[sel]
    out = {}
    if "rope" in f:
        H, KV, Dr, D = c.geo
        out["Q"] = torch.full((B, H * D), R.SENTINEL, dtype=bf, device=DEV)
        if pools is None:
            out["Kt"] = torch.full((c.n_pages, KV, 64, D), R.SENTINEL, dtype=bf, device=DEV)
            out["Vt"] = torch.full((c.n_pages, KV, D, 64), R.SENTINEL, dtype=bf, device=DEV)
        else:
            n = c.n_pages * c.page_elems
            out["Kt"], out["Vt"] = pools[0][:n].view(bf).view(c.n_pages, KV, 64, D), pools[1][:n].view(bf).view(c.n_pages, KV, D, 64)
        kw.update(out, cos_s=dev(c.cos_s), sin_s=dev(c.sin_s), cos_l=dev(c.cos_l), sin_l=dev(c.sin_l), pos=dev(c.pos[sel].contiguous()), tables=dev(c.tables[sel].contiguous()))
    else:
        stride = N + guard
        if guard:
            kw["out_stride"] = stride
        key = "out_f32" if f["out"] == "f32" else "out_bf16"
        out[key] = torch.full((B, stride), FILL, dtype=torch.float32 if f["out"] == "f32" else bf, device=DEV)
        kw[key] = out[key]
        if f.get("bias"):
            kw["bias"] = dev(c.bias)
        if f.get("resid"):
            r = torch.zeros((B, stride), dtype=bf)
            r[:, :N] = c.resid[sel]
            kw["resid"] = dev(r)
        if f.get("producer"):
            out["sq_out"] = torch.full((B, N // 16), FILL, dtype=torch.float32, device=DEV)
            out["out_tiled2"] = torch.full((16 * N,), FILL, dtype=bf, device=DEV)
            kw.update(sq_out=out["sq_out"], out_tiled2=out["out_tiled2"])
        if f.get("consumer"):
            kw["sq_in"] = dev(c.sq_in[sel].contiguous())
    if tiled_x:
        x = R.to_tiled(x)
        kw.update(x_is_tiled=1, batch=B)
    eng.op_decode_proj(dev(c.W), dev(x), **kw)
    if "rope" in f:                                         # the case's pages: all of the pool on the small pools
        out["Kt"], out["Vt"] = out["Kt"][c.page0:c.page0 + c.win], out["Vt"][c.page0:c.page0 + c.win]
    return {k: v.cpu() for k, v in out.items()}


def assert_case(c, got, what, rows=None, guard=0):
    sel = list(range(c.batch)) if rows is None else rows
    N = c.N
    if "rope" in c.f:
        H, KV, Dr, D = c.geo
        eq, ek, ev = c.expect_Q.view(c.batch, H, D)[sel], c.expect_Kt, c.expect_Vt
        if rows is not None:                                # only these sequences' slots are written
            ek, ev = torch.full_like(ek, R.SENTINEL), torch.full_like(ev, R.SENTINEL)
            for b in sel:
                p = int(c.pos[b]); page, slot = int(c.tables[b, p >> 6]) - c.page0, p & 63
                ek[page, :, slot] = c.expect_Kt[page, :, slot]
                ev[page, :, :, slot] = c.expect_Vt[page, :, :, slot]
        for name, g, w in (("Q", got["Q"].view(len(sel), H, D), eq), ("Kt", got["Kt"], ek), ("Vt", got["Vt"], ev)):
            bad = (g.float() != w.float()).nonzero()
            assert bad.numel() == 0, f"{what}: {name}: {bad.shape[0]} elements wrong (sentinel {R.SENTINEL} = must stay untouched); first at {bad[0].tolist()}: got {float(g[tuple(bad[0])])}, expected {float(w[tuple(bad[0])])}"
        return
    key = "out_f32" if c.f["out"] == "f32" else "out_bf16"
    msg = G.exact_mismatch(got[key][:, :N], c.expect[sel], f"{what}: {key}")
    assert msg is None, msg
    if guard:
        assert bool((got[key][:, N:] == FILL).all()), f"{what}: the guard columns past N were written"
    if c.f.get("producer"):
        msg = G.exact_mismatch(got["sq_out"], c.expect_sq[sel], f"{what}: sq_out")
        assert msg is None, msg
        want = torch.full((16 * N,), FILL, dtype=bf)
        k = torch.arange(N)
        for j, b in enumerate(sel):
            want[R.xt_index(j, k)] = c.expect[b]
        assert torch.equal(got["out_tiled2"], want), f"{what}: out_tiled2 is not the row-major output in tile order (or slots of absent sequences were written)"


def sweep(eng, form, w_fmt, Ns, Ks, batches, path=0, variant=0, wide=None, single=True, max_rounds=1, **kw):
    """every (N, K, batch); at batch 16 up to max_rounds seeds (rounds_to_cover of them hit every weight chunk); at the second K, sequences 0 and batch - 1 alone
    == their column of the batch"""
    for K in Ks:
        for N in Ns:
            for B in batches:
                rounds = min(max_rounds, R.rounds_to_cover(K, B)) if B == 16 else 1
                for seed in range(rounds):
                    wd = (R.EXACT_FORMS[form].get("out") == "f32" and w_fmt != 0) if wide is None else wide
                    c = R.exact_case(N, K, B, form, seed=seed, w_fmt=w_fmt, wide=wd, **kw)
                    what = f"{form} {FMT_NAME[w_fmt]} path {path} variant {variant} N={N} K={K} batch={B} seed={seed}"
                    guard = 16 + (-N) % 4 if N % 16 else 0      # 16 or more guard columns; the row stride stays a multiple of 4
                    got = run_case(eng, c, path, variant, guard=guard)
                    assert_case(c, got, what, guard=guard)
                    if single and seed == 0 and B > 1 and K == Ks[min(1, len(Ks) - 1)]:
                        for j in {0, B - 1}:
                            assert_case(c, run_case(eng, c, path, variant, rows=[j]), what + f" sequence {j} alone", rows=[j])


# ---- exact: every form x weight format on the skinny GEMM --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w_fmt", [0, 1, 2])
@pytest.mark.parametrize("form", ["plain", "bias", "bf16", "resid"])
def test_exact_epilogues(eng, form, w_fmt):
    """K: 256 no full load group, 1024 one, 2048 the two-group trip, 3072 an odd group count, 11008 (bf16) 10 groups + 3 remainder steps, 5632 (FP8) 5 groups + 2
    remainder steps -- the (s0 & 1) * 8 branch no shipped geometry runs.  N = 52: a partial last row block.  N = 50: a partial last LANE as well (nr = 48 owns
    rows 48, 49 only): the scalar tail of the epilogue with its per-element bias, resid + rbf(y), bf16 and f32 stores, and the FP8 scale clamp at N - 1."""
    sweep(eng, form, w_fmt, (48, 50, 52), FMT_K[w_fmt], (1, 3, 4, 5, 16), max_rounds=99 if form == "bias" else 2)


@pytest.mark.parametrize("w_fmt", [0, 1, 2])
def test_exact_producer(eng, w_fmt):
    """the residual epilogue that feeds the fused norm: sq_out = the exact integer sums per 16-row block, out_tiled2 = the output permuted by gvl_xt_index"""
    sweep(eng, "producer", w_fmt, (48, 64), FMT_K[w_fmt][:4], (1, 3, 4, 5, 16))


def test_exact_consumer(eng):
    """sq_in: partial sums whose only rounding-free order is the kernel's, totals K * 4^m (rs = 2, 1, 1/2 by sequence); x arrives row-major and as a tiled stream"""
    sweep(eng, "consumer", 0, (48, 50), (512, 1024, 3072, 4096), (1, 3, 5, 16))
    for K in (512, 4096):
        c = R.exact_case(52, K, 5, "consumer", seed=2)
        assert_case(c, run_case(eng, c, tiled_x=True), f"consumer, tiled x, K={K}")
        c4 = R.exact_case(52, K, 5, "consumer", seed=2, nw=4)                   # the 4-wave variant splits the partials differently
        assert_case(c4, run_case(eng, c4, variant=1441), f"consumer, variant 1441, K={K}")


@pytest.mark.parametrize("variant", [1841, 2841, 1441, 2441, 1821, 2821, 1881])
def test_exact_plain_variants(eng, variant):
    """every instantiated plain variant by name: 4 / 8 waves, 2 / 4 / 8 steps per load group, one / two row blocks per workgroup (N = 48: an odd block count under RB = 2)"""
    sweep(eng, "bias", 0, (48, 50), (256, 1024, 2048, 3072, 11008, 8192), (1, 5, 16), variant=variant, single=False, max_rounds=2)
    if variant in (1841, 2841):
        for w_fmt in (1, 2):
            sweep(eng, "resid", w_fmt, (48, 50), FMT_K[w_fmt][-3:], (5,), variant=variant, single=False)


def test_default_variant_for_few_rows_and_long_k(eng):
    """N <= 3072, K >= 8192, K % 2048 == 0: the launcher picks 1881 by itself"""
    sweep(eng, "resid", 0, (64,), (8192,), (1, 16))


@pytest.mark.parametrize("N", [16384, 16400])
def test_exact_two_row_blocks_at_large_N(eng, N):
    """N >= 16384: RB = 2.  16400 = 1025 blocks: the last workgroup's second row block is clamped to the last block and must store nothing -- outputs, sq_out and
    the columns past N (16 guard columns per row) are checked"""
    cases = (("plain", 0, False), ("producer", 0, False), ("bias", 1, True), ("resid", 1, False), ("plain", 2, True)) if N == 16400 else (("producer", 0, False), ("plain", 1, True))
    for form, w_fmt, wide in cases:
        c = R.exact_case(N, (256, 512, 1024)[w_fmt], 5, form, seed=1, w_fmt=w_fmt, wide=wide)
        assert_case(c, run_case(eng, c, guard=16), f"{form} {FMT_NAME[w_fmt]} N={N}", guard=16)


# ---- exact: the VALU GEMV ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "bias", "bf16", "resid"])
def test_exact_gemv(eng, form):
    """path 1, batch 1 / 2 / 4"""
    sweep(eng, form, 0, (48, 50, 52), (256, 1024, 11008), (1, 2, 4), path=1)          # 50: a partial last block of 4 waves x R rows, rows past N - 1 clamped


def test_exact_gemv_rows_per_wave(eng):
    """N chosen so that every rows-per-wave instantiation of the VALU kernel runs: R = 2, 3, 4, 6, 8 at one sequence, 2, 3, 4 at four"""
    sweep(eng, "resid", 0, (4100, 8204, 12300, 20004, 30004), (256,), (1,), path=1, single=False)
    sweep(eng, "resid", 0, (4100, 8204, 12300), (256,), (4,), path=1, single=False)


def test_gemv_refuses_what_it_does_not_serve(eng):
    c = R.exact_case(48, 1024, 5, "plain")
    W, out = dev(c.W), torch.full((16, 48), FILL, dtype=torch.float32, device=DEV)
    for B in (3, 5, 16):
        refused(eng, W, dev(c.x[:1].repeat(B, 1)), [out], path=1, out_f32=out)
    x = dev(c.x[:4])
    sq = torch.ones((4, 64), dtype=torch.float32, device=DEV)
    t = torch.full((16 * 48,), FILL, dtype=bf, device=DEV)
    ob = torch.full((4, 48), FILL, dtype=bf, device=DEV)
    for kw in (dict(w_fmt=1), dict(w_fmt=2), dict(variant=1841), dict(sq_in=sq, sq_n=64), dict(sq_out=sq, out_bf16=ob), dict(out_tiled2=t, out_bf16=ob),
               dict(out_tiled=1, act=R.ACT_SILU_MUL, out_bf16=ob), dict(x_is_tiled=1)):
        refused(eng, W, x, [out, sq, t, ob], path=1, out_f32=out, **kw)


# ---- exact: RoPE + Q + paged KV append -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", [(8, 8, 96, 128), (8, 2, 128, 128), (4, 4, 64, 64)])
@pytest.mark.parametrize("form", ["rope10", "rope01", "rope_switch"])
def test_exact_rope_placement(eng, geo, form):
    """positions 0 / 63 / 64 / 130 mixed across the batch, permuted page tables, rope_switch = 64 (pos 63: short tables, pos 64: long): Q rows, K page slots
    and transposed V page slots hold exactly the expected values and EVERYTHING else -- the D - Dr padding, other slots, other pages -- keeps its sentinel"""
    H, KV, Dr, D = geo
    N = (H + 2 * KV) * Dr
    for w_fmt, K in ((0, 256), (1, 512), (2, 1024)):
        sweep(eng, form, w_fmt, (N,), (K,), (5, 16) if w_fmt == 0 else (5,), rope_geo=geo)
    sweep(eng, form, 0, (N,), (256,), (1, 2, 4), path=1, rope_geo=geo)


# ---- exact: RoPE + Q + paged KV append on pages whose offsets need more than 32 bits ------------------------------------------------------------------------
RELOCATED = R.rope_relocated_cases()
SENT_BITS = int(torch.tensor(R.SENTINEL, dtype=bf).view(torch.int16))


@pytest.fixture(scope="module")
def big_pools():
    """K and V^T pools of decode_proj_ref.POOL_ELEMS (just over 2^31) bf16 elements each, 4.3 GB apiece, shared by every relocated case and freed with the module"""
    pools = big_pool_pair(R.POOL_ELEMS)
    yield pools
    pools.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n", range(len(RELOCATED)))
def test_exact_rope_placement_above_2_to_the_31_elements_of_the_pools(eng, big_pools, n):
    """decode_rope_pair (gvl_decode_epi.h) from both kernels: a case of the rope sweep whose page tables name pages from the first one at or above 2^31 (the last case:
    2^30) elements of 4.3 GB pools.  Q, the K page slots and the V^T page slots bit for bit; EVERY other element of both pools still the sentinel (the low part never
    holds the case's data: a wrapped write cannot produce the right pages); every output bit-identical to the same case on its small pools at first_page = 0"""
    geo, form, w_fmt, K, B, path, k = RELOCATED[n]
    c = R.rope_relocated_case(*RELOCATED[n])
    small = R.exact_case(c.N, K, B, form, seed=0, w_fmt=w_fmt, rope_geo=geo)
    assert int(c.tables.min()) * c.page_elems >= 1 << k and (k == 31 or (int(c.tables.max()) + 1) * c.page_elems <= 1 << 31), "the pages of this case do not lie where the test says"
    for p in big_pools:
        p.fill_(SENT_BITS)
    what = f"{form} {FMT_NAME[w_fmt]} path {path} {geo} K={K} batch={B} pages from {int(c.tables.min())} (2^{k} elements)"
    got = run_case(eng, c, path, pools=big_pools)
    assert_case(c, got, what)
    lo, hi = c.page0 * c.page_elems, (c.page0 + c.win) * c.page_elems
    for name, p in (("K", big_pools[0]), ("V^T", big_pools[1])):
        bad = count_other(p, SENT_BITS, lo, hi)
        assert bad == 0, f"{what}: {bad} elements of the {name} pool outside pages {c.page0} .. {c.page0 + c.win - 1} are no longer the sentinel"
    low = run_case(eng, small, path)
    for name in ("Q", "Kt", "Vt"):
        assert torch.equal(bits(got[name]), bits(low[name])), f"{what}: {name} differs from the same case at first_page = 0"


# ---- quantisers ----------------------------------------------------------------------------------------------------------------------------------------
def one_hot_products(eng, W, w_fmt, first_kw):
    """[N, K] float32: column k from the call whose sequence b has x = e_k, k = 16 c + b -- what the TILE STREAM holds, element by element"""
    N, K = W.shape
    Wd = dev(W)
    cols = []
    for c0 in range(0, K, 16):
        x = torch.zeros((16, K), dtype=bf)
        x[torch.arange(16), c0 + torch.arange(16)] = 1.0
        y = torch.full((16, N + (-N) % 4), FILL, dtype=torch.float32, device=DEV)
        eng.op_decode_proj(Wd, dev(x), w_fmt=w_fmt, out_f32=y, out_stride=y.shape[1], **(first_kw if c0 == 0 else {}))
        cols.append(y.cpu()[:, :N])
    return torch.cat(cols).T.contiguous()


def bits(t):
    return t.contiguous().view(torch.int16)


def test_fp8_quantiser_on_every_bf16_input(eng):
    W = R.fp8_edge_rows()
    N, K = W.shape
    deq_ref, s_ref, _ = R.fp8_quant(W)
    want = torch.from_numpy(deq_ref).to(bf)
    assert bool((want.double().numpy() == deq_ref).all())
    w_deq = torch.zeros((N, K), dtype=bf, device=DEV)
    w_scale = torch.zeros((N,), dtype=torch.float32, device=DEV)
    prod = one_hot_products(eng, W, 1, dict(w_deq=w_deq, w_scale=w_scale))
    assert torch.equal(w_scale.cpu().double(), torch.from_numpy(s_ref)), "fp8_row_scale"
    bad = (bits(w_deq.cpu()) != bits(want)).nonzero()
    assert bad.numel() == 0, f"fp8_requant_retile: {bad.shape[0]} de-quantised values differ (signed zeros count); first {bad[0].tolist()}: {float(W[tuple(bad[0])])} -> {float(w_deq.cpu()[tuple(bad[0])])}, expected {float(want[tuple(bad[0])])}"
    bad = (prod.double() != want.double()).nonzero()
    assert bad.numel() == 0, f"FP8 tile stream x wscale: {bad.shape[0]} elements differ; first {bad[0].tolist()}"


def test_mxfp4_quantiser_on_every_bf16_input(eng):
    W = R.mxfp4_edge_rows()
    N, K = W.shape
    deq_ref, _, e8 = R.mxfp4_quant(W)
    want = torch.from_numpy(deq_ref).to(bf)
    assert bool((want.double().numpy() == deq_ref).all())
    words_ref = R.mxfp4_scale_words(e8)
    w_deq = torch.zeros((N, K), dtype=bf, device=DEV)
    w_scale = torch.zeros(words_ref.shape, dtype=torch.int32, device=DEV)
    prod = one_hot_products(eng, W, 2, dict(w_deq=w_deq, w_scale=w_scale))
    got_words = w_scale.cpu().numpy().view(np.uint32)
    assert (got_words == words_ref).all(), f"mxfp4_scale: {(got_words != words_ref).sum()} scale words differ"
    bad = (bits(w_deq.cpu()) != bits(want)).nonzero()
    assert bad.numel() == 0, f"mxfp4_requant_retile: {bad.shape[0]} de-quantised values differ (signed zeros count); first {bad[0].tolist()}: {float(W[tuple(bad[0])])} -> {float(w_deq.cpu()[tuple(bad[0])])}, expected {float(want[tuple(bad[0])])}"
    bad = (prod.double() != want.double()).nonzero()
    assert bad.numel() == 0, f"MXFP4 tile stream: {bad.shape[0]} elements differ; first {bad[0].tolist()}"


@pytest.mark.parametrize("w_fmt", [1, 2])
def test_quantisers_follow_the_rotate_half_row_order(eng, w_fmt):
    """with rope_on the scales are per LOGICAL row and the de-quantised weight comes back in the model's row order"""
    H, KV, Dr, D = 4, 4, 64, 64
    N, K = (H + 2 * KV) * Dr, 1024
    _, W, _ = R.bounded_data(N, K, 1, 21)
    W = (W.float() * torch.exp2(torch.arange(N) % 7 - 3.0)[:, None]).to(bf)     # rows of different scales: a wrong permutation shows in the scales
    c = R.exact_case(N, 256, 1, "rope10", rope_geo=(H, KV, Dr, D))
    deq, s, e8 = (R.fp8_quant if w_fmt == 1 else R.mxfp4_quant)(W, Dr, H + KV)
    w_deq = torch.zeros((N, K), dtype=bf, device=DEV)
    w_scale = torch.zeros((N,) if w_fmt == 1 else R.mxfp4_scale_words(e8).shape, dtype=torch.float32 if w_fmt == 1 else torch.int32, device=DEV)
    Q = torch.zeros((1, H * D), dtype=bf, device=DEV); Kt = torch.zeros((c.n_pages, KV, 64, D), dtype=bf, device=DEV); Vt = torch.zeros((c.n_pages, KV, D, 64), dtype=bf, device=DEV)
    kw = dict(c.kw, w_fmt=w_fmt)
    eng.op_decode_proj(dev(W), dev(torch.ones((1, K), dtype=bf)), Q=Q, Kt=Kt, Vt=Vt, cos_s=dev(c.cos_s), sin_s=dev(c.sin_s), cos_l=dev(c.cos_l), sin_l=dev(c.sin_l),
                       pos=dev(c.pos), tables=dev(c.tables), w_deq=w_deq, w_scale=w_scale, **kw)
    assert bool((torch.from_numpy(R.logical_rows(N, Dr, H + KV)) != torch.arange(N)).any())
    assert torch.equal(bits(w_deq.cpu()), bits(R.quant(W, w_fmt, Dr, H + KV)))
    if w_fmt == 1:
        assert torch.equal(w_scale.cpu().double(), torch.from_numpy(s))
    else:
        assert (w_scale.cpu().numpy().view(np.uint32) == R.mxfp4_scale_words(e8)).all()


# ---- bounded -------------------------------------------------------------------------------------------------------------------------------------------
RATIOS = {}


def report(form, got, ref, bound, gross=2e-2):
    r, bad = R.max_ratio(got.cpu(), ref, bound)
    RATIOS[form] = max(RATIOS.get(form, 0.0), r)
    print(f"[decode-proj bound] {form}: max err / bound = {r:.3g} ({bad} of {ref.numel()} outside); worst so far for this form: {RATIOS[form]:.3g}")
    check(got.cpu(), ref, gross, form)                      # and not grossly wrong either
    assert bad == 0, f"{form}: {bad} elements outside the per-element bound, worst err / bound {r:.3f}"


@pytest.mark.parametrize("w_fmt", [0, 1, 2])
def test_bounded_swiglu(eng, w_fmt):
    """N = 2 I, I = 52 and 26: neither a multiple of two 16-row blocks of (gate, up) pairs, so the last row block is partial; tile-order and plain output, f32
    output.  The launcher refuses SILU_MUL with N % 4 != 0 (asserted at I = 27), so every lane that stores takes the nr + 3 < N branch: the nr + 1 < N branch of
    the SwiGLU epilogue cannot be reached through the launcher and is not covered here or anywhere else."""
    for I, B in ((52, 5), (26, 16), (27, 3)):
        N, K = 2 * I, 1024
        x, W, Wq = R.bounded_data(N, K, B, 31 + I, w_fmt)
        ref, bound = R.swiglu_bound(x, Wq)
        ref32, bound32 = R.swiglu_bound(x, Wq, out_f32=True)
        Is = I + (-I) % 4                                   # row stride: a multiple of 4; the columns past I are guards
        ob = torch.full((B, Is), FILL, dtype=bf, device=DEV); of = torch.full((B, Is), FILL, dtype=torch.float32, device=DEV)
        if N % 4:                                           # the launcher wants whole lanes of (gate, up) pairs
            refused(eng, dev(W), dev(x), [ob], w_fmt=w_fmt, act=R.ACT_SILU_MUL, out_bf16=ob, out_stride=Is)
            continue
        eng.op_decode_proj(dev(W), dev(x), w_fmt=w_fmt, act=R.ACT_SILU_MUL, out_bf16=ob, out_f32=of, out_stride=Is)
        assert bool((ob[:, I:] == FILL).all()) and bool((of[:, I:] == FILL).all()), "columns past N / 2 were written"
        ob, of = ob[:, :I].contiguous(), of[:, :I].contiguous()
        report(f"swiglu {FMT_NAME[w_fmt]} bf16 out", ob, ref, bound)
        report(f"swiglu {FMT_NAME[w_fmt]} f32 out", of, ref32, bound32)
        ot = torch.full((16 * ((I + 31) // 32) * 32,), FILL, dtype=bf, device=DEV)
        eng.op_decode_proj(dev(W), dev(x), w_fmt=w_fmt, act=R.ACT_SILU_MUL, out_bf16=ot, out_tiled=1)
        assert torch.equal(R.from_tiled(ot.cpu(), B, I), ob.cpu()), "the tile-order SwiGLU output is not the row-major one permuted by gvl_xt_index"
        mask = torch.ones_like(ot.cpu(), dtype=torch.bool)
        for b in range(B):
            mask[R.xt_index(b, torch.arange(I))] = False
        assert bool((ot.cpu()[mask] == FILL).all()), "tile slots of absent sequences / columns were written"
    if w_fmt == 0:                                          # the VALU kernel's own SwiGLU epilogue
        x, W, Wq = R.bounded_data(104, 1024, 4, 77)
        ref, bound = R.swiglu_bound(x, Wq)
        ob = torch.full((4, 52), FILL, dtype=bf, device=DEV)
        eng.op_decode_proj(dev(W), dev(x), path=1, act=R.ACT_SILU_MUL, out_bf16=ob)
        report("swiglu bf16 gemv", ob, ref, bound)


@pytest.mark.parametrize("geo", [(8, 8, 96, 128), (8, 2, 128, 128), (4, 4, 64, 64)])
def test_bounded_rope(eng, geo):
    """LongRoPE-like tables, both sets, positions either side of the switch; both kernels and the FP8 stream"""
    H, KV, Dr, D = geo
    N = (H + 2 * KV) * Dr
    tabs = R.longrope_tables(132, Dr)
    for path, w_fmt, K, B in ((0, 0, 256, 8), (0, 1, 512, 4), (0, 2, 1024, 4), (1, 0, 256, 4)):
        x, W, Wq = R.bounded_data(N, K, B, 41 + path, w_fmt, Dr, H + KV)
        pos, tables, n_pages = R.rope_layout(B, 0)
        q, k, v = R.rope_bound(x, Wq, geo, pos, tabs, R.ROPE_SWITCH)
        refQ, refK, refV = R.rope_place(q.x, k.x, v.x, pos, tables, n_pages, geo, torch.float64, R.SENTINEL)
        bQ, bK, bV = R.rope_place(q.e, k.e, v.e, pos, tables, n_pages, geo, torch.float64, 0.0)       # bound 0 off target: the sentinel must survive exactly
        Q = torch.full((B, H * D), R.SENTINEL, dtype=bf, device=DEV); Kt = torch.full((n_pages, KV, 64, D), R.SENTINEL, dtype=bf, device=DEV)
        Vt = torch.full((n_pages, KV, D, 64), R.SENTINEL, dtype=bf, device=DEV)
        eng.op_decode_proj(dev(W), dev(x), path=path, w_fmt=w_fmt, rope_on=1, rope_switch=R.ROPE_SWITCH, cos_s=dev(tabs[0]), sin_s=dev(tabs[1]), cos_l=dev(tabs[2]),
                           sin_l=dev(tabs[3]), max_pos=132, n_pages=n_pages, pos=dev(pos), tables=dev(tables), table_stride=tables.shape[1], q_stride=H * D, Q=Q, Kt=Kt, Vt=Vt,
                           H=H, KV=KV, Dr=Dr, D=D)
        tag = f"rope {FMT_NAME[w_fmt]} path {path}"
        report(tag + " Q", Q, refQ, bQ)
        report(tag + " K pages", Kt, refK, bK)
        report(tag + " V pages", Vt, refV, bV)


@pytest.mark.parametrize("K,w_fmt", [(K, f) for K in (256, 1024, 4096) for f in (0, 1, 2) if K % (32, 512, 1024)[f] == 0])
def test_bounded_norm_prologue(eng, K, w_fmt):
    """the in-block RMSNorm (XN): batch 1 .. 4 with one row block per workgroup (default) and two (variant 2841), and the VALU kernel's own prologue; N = 50: a
    partial last lane; batch 5 is refused"""
    N, Ns = 50, 52
    nw = (torch.randn(K, generator=torch.Generator().manual_seed(3)) * 0.1 + 1.0).to(bf)
    for B in (1, 2, 3, 4):
        x, W, Wq = R.bounded_data(N, K, B, 50 + B, w_fmt)
        bias = torch.randn(N, generator=torch.Generator().manual_seed(B)) * 0.5
        ref, bound = R.norm_prologue_bound(x, nw, 1e-5, Wq, bias)
        for path, variant in ((0, 0), (0, 2841), (1, 0)):
            if path == 1 and (w_fmt or B == 3):
                continue
            y = torch.full((B, Ns), FILL, dtype=torch.float32, device=DEV)
            eng.op_decode_proj(dev(W), dev(x), path=path, variant=variant, w_fmt=w_fmt, norm_w=dev(nw), eps=1e-5, bias=dev(bias), out_f32=y, out_stride=Ns)
            assert bool((y[:, N:] == FILL).all()), "columns past N were written"
            report(f"norm prologue {FMT_NAME[w_fmt]} path {path}" + (f" variant {variant}" if variant else ""), y[:, :N].contiguous(), ref, bound)
    x, W, _ = R.bounded_data(N, K, 5, 55, w_fmt)
    y = torch.full((5, Ns), FILL, dtype=torch.float32, device=DEV)
    refused(eng, dev(W), dev(x), [y], w_fmt=w_fmt, norm_w=dev(nw), eps=1e-5, out_f32=y, out_stride=Ns)


@pytest.mark.parametrize("K", [512, 1024, 3072, 4096])
def test_bounded_producer_consumer_chain(eng, K):
    """o_proj / down_proj -> next projection as the decode step runs them: the producer (resid + sq_out + out_tiled2), a weight folded with the norm weight by
    gvl_op_fold_gamma, the consumer reading the producer's tiled stream and partial sums (sq_n = K / 16) -- against float64 rmsnorm(resid + y) W^T"""
    B, K1, N2 = 5, 256, 52
    g = torch.Generator().manual_seed(K)
    a, W1, _ = R.bounded_data(K, K1, B, 61)
    resid = (torch.randn((B, K), generator=g) * 2).to(bf)
    gamma = (torch.randn(K, generator=g) * 0.1 + 1.0).to(bf)
    W2 = (torch.randn((N2, K), generator=g) * K ** -0.5).to(bf)
    Wf = eng.op_fold_gamma(dev(W2), dev(gamma))
    assert torch.equal(Wf.cpu(), (W2.float() * gamma.float()[None, :]).to(bf)), "gvl_op_fold_gamma"
    h_ref, sq_ref = R.producer_bound(a, W1, resid)
    ref, bound = R.consumer_bound(h_ref, sq_ref, Wf.cpu(), 1e-5)
    h = torch.full((B, K), FILL, dtype=bf, device=DEV); sq = torch.full((B, K // 16), FILL, dtype=torch.float32, device=DEV); ht = torch.zeros((16 * K,), dtype=bf, device=DEV)
    eng.op_decode_proj(dev(W1), dev(a), resid=dev(resid), out_bf16=h, sq_out=sq, out_tiled2=ht)
    report("chain: producer h", h, h_ref.x, h_ref.e)
    report("chain: producer sq_out", sq, sq_ref.x, sq_ref.e)
    assert torch.equal(R.from_tiled(ht.cpu(), B, K), h.cpu())
    y = torch.full((B, N2), FILL, dtype=torch.float32, device=DEV)
    eng.op_decode_proj(Wf, ht, x_is_tiled=1, batch=B, sq_in=sq, sq_n=K // 16, eps=1e-5, out_f32=y)
    report("chain: consumer", y, ref, bound)
    full = (h_ref.x * torch.rsqrt((h_ref.x ** 2).mean(1, keepdim=True) + 1e-5) * gamma.double()[None, :]) @ W2.double().T
    check(y.cpu(), full, 2e-2, f"chain K={K} vs float64 rmsnorm(resid + y) W^T")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_documented_preconditions_are_refused(eng):
    """bad arguments only: nothing here reaches a kernel"""
    N = 48
    mk = lambda K, B=4: (dev(torch.ones((N, K), dtype=bf)), dev(torch.ones((B, K), dtype=bf)))
    y = torch.full((16, N), FILL, dtype=torch.float32, device=DEV)
    ob = torch.full((16, N), FILL, dtype=bf, device=DEV)
    sq = torch.full((16, 64), FILL, dtype=torch.float32, device=DEV)
    t = torch.full((16 * N,), FILL, dtype=bf, device=DEV)
    outs = [y, ob, sq, t]
    W, x = mk(1024)
    refused(eng, *mk(128), outs, out_f32=y)                                     # K % 256
    refused(eng, *mk(384), outs, out_f32=y)
    refused(eng, *mk(2560), outs, w_fmt=2, out_f32=y)                           # MXFP4: K % 1024
    refused(eng, *mk(768), outs, w_fmt=1, out_f32=y)                            # FP8: K % 512
    refused(eng, W, x, outs, w_fmt=1, sq_in=sq, sq_n=64, out_f32=y)             # sq_in needs bf16 weights
    refused(eng, W, x, outs, w_fmt=2, sq_in=sq, sq_n=64, out_f32=y)
    refused(eng, W, x, outs, sq_in=sq, sq_n=48, out_f32=y)                      # sq_n % 32
    refused(eng, W, x, outs, sq_in=sq, sq_n=64, norm_w=dev(torch.ones(1024, dtype=bf)), out_f32=y)
    refused(eng, W, x, outs, out_tiled=1, out_bf16=ob)                          # out_tiled without SwiGLU
    refused(eng, W, x, outs, sq_out=sq, out_f32=y)                              # the producer needs the bf16 output
    refused(eng, W, x, outs, sq_out=sq, out_bf16=ob, act=R.ACT_SILU_MUL)
    refused(eng, W, x, outs, variant=1234, out_f32=y)                           # no such kernel
    refused(eng, W, dev(torch.ones((17, 1024), dtype=bf)), outs, out_f32=y)     # batch > 16
    refused(eng, W, x, outs)                                                    # no output at all
    refused(eng, W, x, outs, out_f32=y, out_stride=50)                          # batch > 1: rows of the outputs a multiple of 4 apart
    # rope: odd Dr, N that is not (H + 2 KV) Dr, a position past the tables, a page past the pools
    H, KV, D = 2, 1, 16
    tabs = [dev(torch.ones((8, 6), dtype=torch.float32)) for _ in range(4)]
    Q = torch.full((4, H * D), FILL, dtype=bf, device=DEV); Kt = torch.full((2, KV, 64, D), FILL, dtype=bf, device=DEV); Vt = torch.full((2, KV, D, 64), FILL, dtype=bf, device=DEV)
    pos = dev(torch.tensor([0, 1, 2, 3], dtype=torch.int32)); tables = dev(torch.zeros((4, 1), dtype=torch.int32))
    rk = dict(rope_on=1, cos_s=tabs[0], sin_s=tabs[1], cos_l=tabs[2], sin_l=tabs[3], max_pos=8, n_pages=2, pos=pos, tables=tables, table_stride=1, q_stride=H * D, Q=Q, Kt=Kt, Vt=Vt,
              H=H, KV=KV, D=D)
    refused(eng, W, x, [Q, Kt, Vt], Dr=11, **rk)                                # odd Dr (N = 44 would not match either)
    refused(eng, W, x, [Q, Kt, Vt], Dr=10, **rk)                                # N = 48 != 4 * 10
    refused(eng, W, x, [Q, Kt, Vt], Dr=12, **dict(rk, pos=dev(torch.tensor([0, 1, 2, 8], dtype=torch.int32))))
    refused(eng, W, x, [Q, Kt, Vt], Dr=12, **dict(rk, tables=dev(torch.tensor([[0], [1], [2], [0]], dtype=torch.int32))))
    Wodd = dev(torch.ones((2 * 1 * 11 * 2, 256), dtype=bf))                     # N = (H + 2 KV) Dr with Dr = 11: the launcher's own odd-Dr check is behind the entry's
    refused(eng, Wodd, dev(torch.ones((4, 256), dtype=bf)), [Q, Kt, Vt], Dr=11, **rk)
