"""-m gpu: the vision front end and the glue of the visual prefix, kernel by kernel through the C ABI (gvl_op_patch_embed, gvl_op_patchify, gvl_op_hd_merge, gvl_op_pool_*,
gvl_op_strip_cls, gvl_op_bcast_row, gvl_op_gemm_grouped, gvl_op_layernorm / rmsnorm) against the float64 references of tests/vision_ref.py: exact integer cases that must
be reproduced bit for bit, and bounded cases with a derived per-element bound that ZERO elements may exceed (tests/test_vision_ref_cpu.py proves on the CPU that a correct
implementation meets every check used here and that the bugs these tests exist for do not).  Outputs live inside sentinel-filled allocations: nothing around them may
change.  Each test prints the largest |err| / bound it saw and the number of elements that differ bitwise from the rounded reference."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_plan as GP  # noqa: E402
import vision_ref as V  # noqa: E402
from gpu_util import DEV, bf, tiny_geo  # noqa: E402
from grounded_video_llm_amd import engine as E, lib as L, synth, weights as Wt  # noqa: E402

CASES = V.patch_cases()
IDS = [c.name() for c in CASES]
GRID_CAP = 8192 * 256            # threads of the largest grid the glue launchers start: more items than this and the grid-stride loop wraps
_dev, _fused = {}, {}


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(tiny_geo(), DEV, towers=())
    yield e
    e.close()
    _dev.clear()
    _fused.clear()


def report(what, worst, ndiff, total):
    print(f"[parity] {what}: max |err| / bound = {worst:.3g}, {ndiff} of {total} elements differ bitwise from the rounded reference")


def refused(fn, status=L.ERR_ARG):
    with pytest.raises(L.GvlError) as ei:
        fn()
    assert ei.value.status == status, ei.value
    torch.cuda.synchronize()


def rnd(shape, seed, std=1.0):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randn(shape, generator=g, device=DEV) * std


# ---- patch embedding ------------------------------------------------------------------------------------------------------------------------------------------------
def operands(c):
    if c.name() not in _dev:
        _dev[c.name()] = {k: (None if getattr(c, k) is None else getattr(c, k).to(DEV)) for k in ("px", "W", "bias", "cls", "pos", "lnw", "lnb")}
    return _dev[c.name()]


def run_patch(eng, c, path, im2col=None):
    d = operands(c)
    buf, out = V.guarded(c.n * c.S, c.C, c.out_dtype(), DEV)
    eng.op_patch_embed(c.mode, path, d["px"], d["W"], d["cls"], d["pos"], out, c.patch, bias=d["bias"], lnw=d["lnw"], lnb=d["lnb"], eps=c.eps, im2col=im2col)
    torch.cuda.synchronize()
    host = buf.cpu()
    return host, host[V.PAD_ROWS:V.PAD_ROWS + c.n * c.S]


def fused(eng, c):
    if c.name() not in _fused:
        _fused[c.name()] = run_patch(eng, c, 0)
    return _fused[c.name()]


def assert_patch(c, buf, out, what):
    msg, worst, ndiff = V.check_patch(c, out, what)
    report(what, worst, ndiff, out.numel())
    assert msg is None, msg
    # the bytes before the output and after it -- for a tail tile: the rows that follow row M - 1 -- keep the sentinel
    assert V.guard_damage(buf, c.n * c.S) == 0, f"{what}: wrote outside its output"


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_patch_embed_fused(eng, c):
    buf, out = fused(eng, c)
    assert_patch(c, buf, out, f"patch_embed fused {c.name()}")


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_patch_embed_three_pass(eng, c):
    """the same bounds for the three passes; their im2col matrix is bit-exact, zero columns included; InternVideo2's exact cases are bit-equal between the two paths"""
    abuf, A = V.guarded(c.M, c.Kp, bf, DEV)
    buf, out = run_patch(eng, c, 1, im2col=A)
    assert_patch(c, buf, out, f"patch_embed three-pass {c.name()}")
    assert torch.equal(A.cpu(), V.patchify_ref(c.px, c.patch, c.Kp)), "im2col differs from the reference"
    assert V.guard_damage(abuf, c.M) == 0, "im2col wrote outside its matrix"
    ndiff = int((out != fused(eng, c)[1]).sum())
    print(f"[parity] patch_embed {c.name()}: {ndiff} of {out.numel()} elements differ bitwise between the fused and the three-pass path")
    if c.kind == "exact" and c.mode == 1:
        assert ndiff == 0


@pytest.mark.parametrize("patch,image,n,T,Kp", [(4, 8, 2, 2, 48), (4, 8, 2, 2, 64), (16, 32, 2, 1, 768), (14, 28, 1, 3, 592), (4, 8, 87400, 1, 48)])
def test_patchify_alone(eng, patch, image, n, T, Kp):
    """any patch size the launcher accepts; the last case has more items (n T g^2 Kp / 8) than the largest grid has threads: the grid-stride loop wraps"""
    g = image // patch
    if n > 1000:
        assert n * T * g * g * (Kp // 8) > GRID_CAP
    px = rnd((n, 3, T, image, image), 5)
    abuf, A = V.guarded(n * T * g * g, Kp, bf, DEV)
    eng.op_patchify(px, A, patch)
    torch.cuda.synchronize()
    assert torch.equal(A, V.patchify_ref(px, patch, Kp)) and V.guard_damage(abuf, A.shape[0]) == 0


def test_iv2_embed_grid_wraps(eng):
    """iv2_embed_kernel is reached through the three passes only: an exact case with more items (n S C / 8) than its largest grid has threads.  Every value is a small
    integer, so the expectation is an fp32 matmul of the (bit-exact, tested above) im2col matrix -- exact in any order -- plus bias and pos"""
    n, C = 131073, 64
    c = V.patch_case(1, 14, 1, n, C, "exact", device=DEV)
    assert n * c.S * (C // 8) > GRID_CAP
    abuf, A = V.guarded(c.M, c.Kp, bf, DEV)
    buf, out = V.guarded(n * c.S, C, bf, DEV)
    eng.op_patch_embed(1, 1, c.px, c.W, c.cls, c.pos, out, c.patch, bias=c.bias, im2col=A)
    torch.cuda.synchronize()
    im2col = V.patchify_ref(c.px, c.patch, c.Kp)
    assert torch.equal(A, im2col)
    acc = im2col[:, :V.KREAL].float() @ c.W[:, :V.KREAL].float().T
    pos, cls = c.pos.float(), c.cls.float()
    want = torch.stack([(cls + pos[0]).expand(n, C), acc + c.bias + pos[1]], 1)
    assert float(want.abs().max()) <= 256 and bool((want == want.round()).all())
    assert torch.equal(out.view(n, 2, C), want.to(bf))
    assert V.guard_damage(buf, n * c.S) == 0 and V.guard_damage(abuf, c.M) == 0


def test_patch_embed_refusals(eng):
    """the fused path refuses what its launcher does not implement -- no fall-back -- and writes nothing"""
    def attempt(mode, path, C, patch, image, T, Kp, status=L.ERR_ARG, n=1, **kw):
        g = image // patch
        S = 1 + T * g * g
        dt = torch.float32 if mode == 0 else bf
        buf, out = V.guarded(n * S, C, dt, DEV)
        z = lambda *s: torch.zeros(s, device=DEV)
        args = dict(bias=z(C) if mode == 1 else None, lnw=z(C) if mode == 0 else None, lnb=z(C) if mode == 0 else None)
        args.update(kw)
        refused(lambda: eng.op_patch_embed(mode, path, z(n, 3, T, image, image), z(C, Kp).to(bf), z(C).to(dt), z(S, C).to(dt), out, patch, **args), status)
        assert bool((buf == V.SENT).all()), "a refused call wrote to its output"
    attempt(1, 0, 768, 14, 14, 1, 640)                       # C = 768: no fused kernel
    attempt(1, 0, 1024, 16, 32, 1, 768)                      # patch 16
    attempt(0, 0, 1024, 14, 14, 2, 640)                      # CLIP has no frames
    attempt(0, 0, 1408, 14, 14, 1, 640)                      # CLIP at InternVideo2's width
    attempt(1, 1, 1024, 14, 14, 1, 592)                      # three passes: the GEMM needs Kp % 64 == 0
    attempt(1, 0, 1024, 14, 14, 1, 640, im2col=torch.zeros((1, 640), dtype=bf, device=DEV))
    attempt(1, 1, 1024, 14, 14, 1, 640, bias=None)
    attempt(1, 1, 1024, 14, 14, 1, 640, status=L.ERR_OOM, n=40000)      # 40000 x 1024 bf16 GEMM output: more than the workspace arena of this engine holds


# ---- glue -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C", [(1, 8), (3, 8), (1, 1024), (3, 1024), (3362, 4)])
def test_hd_merge(eng, n, C):
    if n > 1000:
        assert n * 156 * C > GRID_CAP
    f, sub = rnd((n, 576, C), 1, 3.0), rnd((4 * C,), 2)
    buf, out = V.guarded(n * 156, 4 * C, bf, DEV)
    eng.op_hd_merge(f, sub, out)
    torch.cuda.synchronize()
    assert torch.equal(out.view(n, 156, 4 * C), V.hd_merge_ref(f, sub)) and V.guard_damage(buf, n * 156) == 0


@pytest.mark.parametrize("n,C", [(2, 4), (2, 1024), (32769, 4)])
def test_pool_spatial(eng, n, C):
    if n > 1000:
        assert n * 64 * (C // 4) > GRID_CAP
    else:
        f = rnd((n, 576, C), 3, 3.0)
        buf, out = V.guarded(n * 64, C, bf, DEV)
        eng.op_pool_spatial(f, out)
        torch.cuda.synchronize()
        v = V.pool_spatial_ref(f)
        msg, worst = V.bound_violations(out, v.x.reshape(-1, C), v.e.reshape(-1, C), f"pool_spatial n{n} C{C}")
        report(f"pool_spatial n{n} C{C}", worst, int((out != v.x.reshape(-1, C).to(bf)).sum()), out.numel())
        assert msg is None, msg
        assert V.guard_damage(buf, n * 64) == 0
    f, want = V.pool_spatial_exact_input(n, C, 7, DEV)               # integers whose windows sum to 9 times their mean: exact in any order
    buf, out = V.guarded(n * 64, C, bf, DEV)
    eng.op_pool_spatial(f, out)
    torch.cuda.synchronize()
    assert torch.equal(out.view(n, 64, C), want) and V.guard_damage(buf, n * 64) == 0


@pytest.mark.parametrize("n,T,C", [(2, 1, 8), (2, 3, 8), (2, 1, 1408), (2, 3, 1408), (131073, 1, 8)])
def test_pool_temporal(eng, n, T, C):
    if n > 1000:
        assert n * T * 16 * (C // 8) > GRID_CAP
    else:
        f = rnd((n, T, 256, C), 4, 2.0).to(bf)
        buf, out = V.guarded(n * T * 16, C, bf, DEV)
        eng.op_pool_temporal(f, out)
        torch.cuda.synchronize()
        v = V.pool_temporal_ref(f)
        msg, worst = V.bound_violations(out, v.x.reshape(-1, C), v.e.reshape(-1, C), f"pool_temporal n{n} T{T} C{C}")
        report(f"pool_temporal n{n} T{T} C{C}", worst, int((out != v.x.reshape(-1, C).to(bf)).sum()), out.numel())
        assert msg is None, msg
        assert V.guard_damage(buf, n * T * 16) == 0
    f = V.int_field((n, T, 256, C), -8, 8, 11, DEV).to(bf)           # sixteen integers: exact in any order
    buf, out = V.guarded(n * T * 16, C, bf, DEV)
    eng.op_pool_temporal(f, out)
    torch.cuda.synchronize()
    want = (f.float().view(n, T, 4, 4, 4, 4, C).sum((3, 5)) / 16).reshape(n * T * 16, C).to(bf)
    assert torch.equal(out, want) and V.guard_damage(buf, n * T * 16) == 0


@pytest.mark.parametrize("dtype,n,S,C", [(torch.float32, 3, 2, 5), (torch.float32, 3, 10, 5), (bf, 3, 2, 6), (bf, 3, 10, 6), (bf, 2, 10, 1408), (torch.float32, 2097153, 2, 1)])
def test_strip_cls(eng, dtype, n, S, C):
    """C = 5 (f32) and C = 6 (bf16): rows of 20 and 12 bytes, multiples of 4 and of nothing larger"""
    if n > 1000:
        assert n * (S - 1) * C > GRID_CAP
    x = V.int_field((n, S, C), -100, 100, 3, DEV).to(dtype)
    buf, out = V.guarded(n * (S - 1), C, dtype, DEV)
    eng.op_strip_cls(x, out)
    torch.cuda.synchronize()
    assert torch.equal(out.view(n, S - 1, C), x[:, 1:]) and V.guard_damage(buf, n * (S - 1)) == 0
    if C == 6:
        refused(lambda: eng.op_strip_cls(x[:, :, :5].contiguous(), out))         # 10-byte rows


@pytest.mark.parametrize("n,stride,cols", [(3, 7, 10), (3, 181, 64), (131073, 2, 8)])
def test_bcast_row(eng, n, stride, cols):
    """row_off = the last row of the stride; every other row keeps the sentinel"""
    if n > 1000:
        assert n * cols > 4096 * 256
    row = V.int_field((cols,), -100, 100, 8, DEV).to(bf)
    buf, out = V.guarded(n * stride, cols, bf, DEV)
    eng.op_bcast_row(row, out, n, stride, stride - 1)
    torch.cuda.synchronize()
    o = out.view(n, stride, cols)
    assert torch.equal(o[:, stride - 1], row.expand(n, cols)) and bool((o[:, :stride - 1] == V.SENT).all()) and V.guard_damage(buf, n * stride) == 0
    refused(lambda: eng.op_bcast_row(row, out, n, stride, stride))


# ---- the row-remapping GEMM store -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grp", V.GROUPINGS, ids=[f"rows{a}-stride{b}-off{c}" for a, b, c in V.GROUPINGS])
@pytest.mark.parametrize("N", [64, 72])
def test_gemm_grouped(eng, N, grp):
    """rows inside the groups: bit-equal to op_gemm of the same operands; every other row keeps its sentinel; every tile_cfg of test_gemm_plain the plan accepts"""
    gr, gs, off = grp
    K, M = 64, 4 * gr + (gr + 1) // 2                                # five groups, the last one partial (grp_rows = 1: five whole ones)
    A, W, bias = rnd((M, K), 21).to(bf), rnd((N, K), 22, K ** -0.5).to(bf), rnd((N,), 23, 0.5)
    _, total = V.grouped_rows(M, gr, gs, off)
    ran = 0
    for cfg in (1, 0, 21, 22, 82, 85):
        for kw, dt in ((dict(), bf), (dict(bias=bias), bf), (dict(bias=bias), torch.float32)):
            f32 = dt == torch.float32
            buf, out = V.guarded(total, N, dt, DEV)
            call = lambda: eng.op_gemm_grouped(A, W, out, gr, gs, off, tile_cfg=cfg, **kw)
            if GP.plans([GP.case(M, N, K, GP.epi_of(out_f32=f32, **kw), cfg, grp_rows=gr)], GP.device_cus())[0] is None:
                refused(call)
                assert bool((buf == V.SENT).all())
                continue
            call()
            dense = eng.op_gemm(A, W, out_f32=f32, tile_cfg=cfg, **kw)
            torch.cuda.synchronize()
            wrong, lost = V.check_grouped(out, dense, gr, gs, off)
            assert (wrong, lost) == (0, 0), f"cfg {cfg} {sorted(kw)} {dt}: {wrong} elements inside the groups differ from op_gemm, {lost} outside lost the sentinel"
            assert V.guard_damage(buf, total) == 0
            ran += 1
    assert ran >= 3
    print(f"[parity] gemm_grouped N{N} {grp}: {ran} (tile_cfg, epilogue) combinations bit-equal to op_gemm, 0 sentinel rows changed")


def test_gemm_grouped_refusals(eng):
    M, N, K = 200, 64, 64
    A, W = rnd((M, K), 31).to(bf), rnd((N, K), 32).to(bf)
    buf, out = V.guarded(2 * 181, N, bf, DEV)
    sq = torch.full((M, 1), float("nan"), device=DEV)
    refused(lambda: eng.op_gemm_grouped(A, W, out, 156, 181, 0, rowsq=sq))          # row statistics + remap: no kernel (gvl_gemm_plan.h)
    refused(lambda: eng.op_gemm_grouped(A, W, out, 156, 181, 26))                   # the groups would overlap
    refused(lambda: eng.op_gemm_grouped(A, W, out, 0, 181, 0))
    assert bool((buf == V.SENT).all()) and bool(torch.isnan(sq).all())


# ---- norms ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", V.LN_COLS)
@pytest.mark.parametrize("rows", V.NORM_ROWS)
def test_layernorm_bound(eng, rows, cols):
    """both sides of the MAXV switch-over (1024 / 1028), a row count that is no multiple of 4, a row of 1000 + noise, an all-zero row, a single nonzero element"""
    x, w, b = V.norm_rows(rows, cols, 1, torch.float32)
    got = eng.op_layernorm(x.to(DEV), w.to(DEV), b.to(DEV), 1e-5).cpu()
    v = V.layernorm_bound(x.double(), torch.zeros((rows, cols), dtype=torch.float64), w.double(), b.double(), 1e-5, out_bf16=True, depth=V.wave_sum_depth(cols))
    msg, worst = V.bound_violations(got, v.x, v.e, f"layernorm {rows}x{cols}")
    report(f"layernorm {rows}x{cols}", worst, int((got != v.x.to(bf)).sum()), got.numel())
    assert msg is None, msg
    if rows == 5:
        assert torch.equal(got[2], b.to(bf)), "an all-zero row gives the bias exactly"


@pytest.mark.parametrize("cols", V.RMS_COLS)
@pytest.mark.parametrize("rows", V.NORM_ROWS)
def test_rmsnorm_bound(eng, rows, cols):
    x, w, _ = V.norm_rows(rows, cols, 2, bf)
    got = eng.op_rmsnorm(x.to(DEV), w.to(DEV), 1e-6).cpu()
    v = V.rmsnorm_bound(x.double(), torch.zeros((rows, cols), dtype=torch.float64), w.double(), 1e-6, depth=V.wave_sum_depth(cols))
    msg, worst = V.bound_violations(got, v.x, v.e, f"rmsnorm {rows}x{cols}")
    report(f"rmsnorm {rows}x{cols}", worst, int((got != v.x.to(bf)).sum()), got.numel())
    assert msg is None, msg
    if rows == 5:
        assert not bool(got[2].any()), "an all-zero row gives 0"


def test_norm_refusals(eng):
    for cols in (6, 4100):
        refused(lambda: eng.op_layernorm(torch.zeros((2, cols), device=DEV), torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV), 1e-5))
    for cols in (12, 8200):
        refused(lambda: eng.op_rmsnorm(torch.zeros((2, cols), device=DEV, dtype=bf), torch.zeros(cols, device=DEV, dtype=bf), 1e-6))


# ---- the fixed geometry of the glue ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("llm", ["phi3.5", "llama3"])
def test_build_visual_refuses_towers_the_glue_does_not_implement(llm):
    """hd_merge / pool_spatial hard-code CLIP's 24 x 24 grid and pool_temporal InternVideo2's 16 x 16: a context whose towers have another grid (here 2 x 2) never
    reaches them -- gvl_build_visual and gvl_encode_segments refuse"""
    geo = tiny_geo(llm=llm)
    eng = E.Engine(geo, DEV, towers=("clip", "iv2", "proj"))
    try:
        eng.load_packed(Wt.pack_clip(synth.clip_weights(geo.clip_hidden, geo.clip_inter, geo.clip_layers, 28, 14, seed="vo.clip"), geo.clip_layers - 1))
        eng.load_packed(Wt.pack_iv2(synth.iv2_weights(geo.iv2_dim, geo.iv2_inter, geo.iv2_depth, geo.frames_per_seg, 28, 14, seed="vo.iv2"), geo.iv2_depth - 1,
                                    geo.frames_per_seg))
        eng.load_packed(Wt.pack_projectors(synth.projector_weights(llm, geo.hidden, geo.clip_hidden, geo.iv2_dim, seed="vo.proj"), llm))
        eng.finalize()
        cf = torch.zeros((1, 4, geo.clip_hidden), device=DEV)
        vf = torch.zeros((1, geo.frames_per_seg * 4, geo.iv2_dim), dtype=bf, device=DEV)
        refused(lambda: eng.build_visual(cf, vf))
        refused(lambda: eng.encode_segments(torch.zeros((1, 3, 28, 28), device=DEV), torch.zeros((1, 3, geo.frames_per_seg, 28, 28), device=DEV)))
    finally:
        eng.close()
