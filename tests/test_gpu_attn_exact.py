"""-m gpu: gvl_op_attention (attn_fwd_kernel, every result-neutral form the operator reaches) against an INDEPENDENT reference (tests/attn_ref.py) -- where
test_gpu_ops.py judges it by max|err| / max|ref| on std-1 data and the other attention tests compare forms that share the mask, kperm, the lazy reference and the epilogue.

Attention checks
  exact cases    one-hot attention (attn_ref.onehot_case): keys are +-1 binary codes of their index (XOR a per-(batch, KV head) mask), a query is 64 x the code of its
                 target, scale 1.0 -- integer scores <= 896, the target >= 128 raw = 184 log2 units ahead of every other key, so every other probability is 0 in fp32, the lazy
                 reference must move (alpha = 0) when the target tile arrives, and the output must equal the target's V row BIT FOR BIT.  V is hashed bf16 bit patterns limited
                 to normal values of 2^-100 ... 2^100: keys that tie at p = 1 before the target arrives are summed, unrestricted exponents overflow that sum and the alpha = 0
                 that follows makes inf 0 = NaN; subnormals are flushed by the MFMA pipe.  A failure names the count, (b, h, i, d), target key, query block, wave, key tile and
                 the key whose V row came out instead.
  bounded cases  dense data with the mass where the kernel is fragile (late_heavy, early_heavy, spike, scaled_rows; plain = the old data) against a float64 softmax computed on
                 the GPU in chunks of 256 query rows: ZERO elements outside attn_ref.elementwise_bound -- leading term 2 . 2^-8 . (p @ |v|): one bf16 rounding of each
                 probability entering P.V (the row sum runs over the unrounded ones) and one of the stored output; plus fp32 score accumulation, the fmaf / v_exp_f32 /
                 reference moves, fp32 accumulation of O and l, the reciprocal and product of the epilogue, all derived there with no fitted factor.
Forms: vision_in_place 1 / 0 / 2 (non-causal, head dim <= 96: Q, K, V in place at head dim 64 -- VROW = 2 --, V in place -- VROW = 1 --, pages; causal or head dim > 96: always
pages) and attn_ring 0 / 2 / 3 on the paged forms.  gvl.h: none of them may change an output bit, so the bounded cases must also be bit-identical across forms.
The output buffer carries 160 guard rows (more than a 128-row query block's overhang) that must keep their fill; qkv is the prefix of an allocation whose next 64 rows are
NaN: the in-place forms must re-read the last real key row for the tail tile's pad keys -- a DMA past the end shows up as NaN (0 . NaN) without any out-of-bounds access.
The folded softmax / ones-row sum of InternVideo2 (VROW = 3, ONES, attn_iv2_pipe_kernel) is not reachable through gvl_op_attention: gvl_op_iv2_attention, test_gpu_iv2_attn.py."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, bf, tiny_geo  # noqa: E402
from grounded_video_llm_amd import engine as E, lib as L  # noqa: E402
import attn_ref as R  # noqa: E402
import attn_plan as A  # noqa: E402

GUARD = 160
NAN_ROWS = 64


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(tiny_geo(), DEV, towers=())
    yield e
    e.close()


def stage(c):
    """qkv as the prefix of an allocation whose next NAN_ROWS rows are NaN"""
    rows = c.B * c.S
    c.alloc = torch.full((rows + NAN_ROWS, c.qkv.shape[1]), float("nan"), dtype=bf, device=DEV)
    c.alloc[:rows] = c.qkv
    return c


def run(eng, c, S=None):
    """one launch of gvl_op_attention into a guarded buffer -> out [B*S, H*Dr]; asserts that the guard rows kept their fill"""
    if getattr(c, "alloc", None) is None:
        stage(c)
    S = S or c.S
    rows = c.B * c.S
    buf = torch.full((rows + GUARD, c.H * c.Dr), R.SENT, dtype=bf, device=DEV)
    base = c.alloc.data_ptr()
    rc = eng.lib.gvl_op_attention(eng.ctx, C.c_void_p(base), C.c_void_p(base + 2 * c.H * c.Dr), C.c_void_p(base + 2 * (c.H + c.KV) * c.Dr), E._ptr(buf),
                                  c.B, S, c.H, c.KV, c.Dr, float(c.scale), int(c.causal), eng.stream)
    c.last_buf = buf
    eng._chk(rc, f"gvl_op_attention {c}")
    torch.cuda.synchronize()
    touched = (buf[rows:] != R.SENT).nonzero()
    assert touched.numel() == 0, f"{c}: {touched.shape[0]} elements of the rows BEYOND B*S written, first at row {rows + int(touched[0][0])}, column {int(touched[0][1])}"
    return buf[:rows]


def forms(c):
    """(label, vision_in_place, attn_ring) of every form the operator reaches for this case.  What each setting claims -- its operand mode, and ring depth 3 wherever
    a depth-3 kernel exists (paged operands, head dim > 64) -- is asserted against the library's own plan for gvl_op_attention's launch (tests/attn_plan.py), and the
    label names the instantiation that plan gives"""
    paged_only = c.causal or c.Dr > 96
    out = []
    for vip in ((1,) if paged_only else (1, 0, 2)):
        mode = A.PAGED if paged_only or vip == 0 else (A.QKV_ROWS if vip == 1 and c.Dr == 64 else A.V_ROWS)
        for ring in ((0, 2, 3) if mode == A.PAGED else (0,)):
            (l,) = A.op_attention(c.B, c.S, c.H, c.KV, c.Dr, int(c.causal), vip, ring)
            assert l.family == A.FWD and l.mode == mode and l.NS == (3 if ring == 3 and l.D > 64 else 2) and l.ONES == 0, f"{c} vision_in_place {vip} attn_ring {ring}: the plan is {l}"
            out.append((f"vision_in_place {vip} attn_ring {ring} ({A.MODE_NAMES[l.mode]}: attn_fwd_kernel<{l.D}, {l.NWAVES}, {l.NS}, {l.ONES}, {l.VROW}, {l.VL}>)", vip, ring))
    return out


def kernels(c):
    return {A.kernel_of(A.op_attention(c.B, c.S, c.H, c.KV, c.Dr, int(c.causal), vip, ring)[0]) for _, vip, ring in forms(c)}


# every attn_fwd_kernel instantiation that gvl_op_attention can reach (it sets neither ones_row nor a ragged group): (D, NWAVES, NS, ONES, VROW, VL)
REACHABLE = {0: {("fwd", 64, 4, 2, 0, v, 0) for v in (0, 1, 2)} | {("fwd", 96, 4, 2, 0, v, 0) for v in (0, 1)} | {("fwd", 96, 4, 3, 0, 0, 0), ("fwd", 128, 4, 2, 0, 0, 0), ("fwd", 128, 4, 3, 0, 0, 0)},
             1: {("fwd", 64, 4, 2, 0, 0, 0)} | {("fwd", D, 4, ns, 0, 0, 0) for D in (96, 128) for ns in (2, 3)}}


def for_every_form(eng, c, judge):
    try:
        for label, vip, ring in forms(c):
            eng.debug_set("vision_in_place", vip)
            eng.debug_set("attn_ring", ring)
            judge(label, run(eng, c))
    finally:
        eng.debug_set("vision_in_place", 1)
        eng.debug_set("attn_ring", 0)


# ---- exact family --------------------------------------------------------------------------------------------------------------------------------------------------
S_LIST = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 193, 257, 577]          # one wave, one tile, one query block, tail tiles of 1 and 63 keys, a last block with 1 real row
DRS = [16, 32, 64, 72, 88, 96, 104, 128]                                          # padded and unpadded on each template; 72 / 104: the smallest on the 96 / 128 templates
BHKV = [(1, 2, 2), (3, 4, 2), (1, 4, 1), (3, 2, 2), (1, 4, 2), (3, 4, 1)]         # B KV = 3: 5 of the 8 XCD groups of the grid are padding


def pairs(maps):
    """a FIXED list of 56 + 4 (shape, map): every S four times, every head dim seven times, every (B, H, KV) and every map about evenly, no full product"""
    out = []
    for i in range(4 * len(S_LIST)):
        r = i // len(S_LIST)
        B, H, KV = BHKV[(i + r) % len(BHKV)]
        out.append((B, S_LIST[i % len(S_LIST)], H, KV, DRS[(3 * i + r) % len(DRS)], maps[(i + 2 * r) % len(maps)]))
    # B KV = 9 and 10: the group index wraps past the 8 XCDs
    out += [(3, 129, 3, 3, 64, maps[0]), (3, 193, 6, 3, 96, maps[1]), (5, 65, 4, 2, 128, maps[2]), (3, 257, 3, 3, 88, maps[-1])]
    return out


def exact_sweep(eng, causal):
    maps = R.CAUSAL_MAPS if causal else R.FULL_MAPS
    n, reached = 0, set()
    for B, S, H, KV, Dr, target in pairs(maps):
        c = R.onehot_case(B, S, H, KV, Dr, causal, target, seed=S + Dr + B, device=DEV)
        reached |= kernels(c)

        def judge(label, out, c=c):
            msg = R.onehot_mismatch(out, c, f"{c} [{label}]")
            assert msg is None, msg

        for_every_form(eng, c, judge)
        n += len(forms(c))
    assert reached == REACHABLE[causal], f"the sweep misses {sorted(REACHABLE[causal] - reached)} / reaches unexpected {sorted(reached - REACHABLE[causal])}"
    print(f"[parity] attention one-hot causal{causal}: {len(pairs(maps))} cases, {n} launches, every one bit for bit")


def test_onehot_cases_bit_for_bit_noncausal(eng):
    exact_sweep(eng, 0)


def test_onehot_cases_bit_for_bit_causal(eng):
    exact_sweep(eng, 1)


@pytest.mark.parametrize("Dr,causal,target", [(64, 0, "perm"), (128, 1, "diag"), (128, 1, "hash")])
def test_onehot_at_the_page_table_limit(eng, Dr, causal, target):
    """S = 16384 = 256 pages, the most the kernel's LDS page table holds; the expectation is a gather -- no S^2 reference"""
    c = R.onehot_case(1, 16384, 1, 1, Dr, causal, target, seed=3, device=DEV)

    def judge(label, out):
        msg = R.onehot_mismatch(out, c, f"{c} [{label}]")
        assert msg is None, msg

    for_every_form(eng, c, judge)


def test_one_key_beyond_the_page_table_is_an_error(eng):
    c = R.Case(1, 16385, 1, 1, 64, 1.0, 0, "S = 16385")
    c.qkv = torch.zeros((16385, 3 * 64), dtype=bf, device=DEV)
    for causal in (0, 1):
        c.causal = causal
        with pytest.raises(L.GvlError):
            run(eng, c)
        torch.cuda.synchronize()
        assert bool((c.last_buf == R.SENT).all()), "an unsupported launch wrote to the output"


# ---- bounded family ------------------------------------------------------------------------------------------------------------------------------------------------
BOUNDED_SHAPES = [(1, 1000, 4, 2, 96, 1), (2, 333, 4, 1, 128, 1), (3, 193, 2, 2, 64, 0), (1, 577, 4, 2, 88, 0), (1, 257, 2, 1, 16, 0), (2, 200, 4, 4, 72, 1), (1, 129, 4, 2, 104, 0),
                  (1, 641, 2, 2, 64, 1)]


@pytest.mark.parametrize("B,S,H,KV,Dr,causal", BOUNDED_SHAPES)
def test_bounded_cases_inside_the_elementwise_bound(eng, B, S, H, KV, Dr, causal):
    for kind in R.KINDS:
        c = R.bounded_case(B, S, H, KV, Dr, causal, kind, seed=S + Dr, device=DEV)
        ref, bound, Abs = R.elementwise_bound(c, chunk=256)
        worst, first = {}, []

        def judge(label, out):
            msg, w = R.bound_violations(out, ref, bound, c, f"{c} [{label}]")
            worst[label] = w
            if not first:
                first.append(out.clone())
                print(f"[parity] attention {c}: worst err / bound {w:.3f}; old statistic max|err| / max|ref| {R.old_stat(out, ref):.2e}, per-row statistic "
                      f"{R.row_stat(out, ref, Abs, Dr):.2e}")
            assert msg is None, msg
            assert torch.equal(R._bits(out), R._bits(first[0])), f"{c} [{label}]: not bit-identical to [{forms(c)[0][0]}]"

        for_every_form(eng, c, judge)
        assert len(worst) == len(forms(c))


# ---- the scratch arena ---------------------------------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_what_the_scratch_arena_held(eng):
    """Q, K pages and V^T pages live in the engine's scratch arena; the rows of the last K page behind key S - 1 are never written (their keys are masked) and the V^T pad
    columns are zero-filled.  After one attention on an all-NaN qkv of a larger shape (its NaN output is expected and not looked at) every form must return the bits it
    returned before: a NaN that reaches an unmasked key or the P.V product's pad columns comes out as NaN (0 . NaN)."""
    cases = [R.bounded_case(2, 193, 4, 2, 88, 0, "plain", 1, DEV), R.bounded_case(1, 129, 2, 2, 72, 1, "late_heavy", 2, DEV), R.bounded_case(3, 65, 2, 1, 16, 0, "late_heavy", 3, DEV),
             R.onehot_case(1, 191, 2, 2, 104, 0, "last", 4, DEV), R.onehot_case(2, 65, 4, 2, 64, 1, "diag", 5, DEV), R.onehot_case(1, 33, 2, 2, 64, 0, "edges", 6, DEV)]
    before = {}
    for i, c in enumerate(cases):
        for_every_form(eng, c, lambda label, out, i=i: before.__setitem__((i, label), out.clone()))
    nan = torch.full((3 * 700, 12 * 128), float("nan"), dtype=bf, device=DEV)
    try:
        for vip in (0, 1):
            eng.debug_set("vision_in_place", vip)
            eng.op_attention(nan[:, :12 * 64], 3, 700, 4, 4, 64, 0.125, 0)
            eng.op_attention(nan[:, :12 * 96].contiguous(), 3, 700, 4, 4, 96, 0.1, 0)
            eng.op_attention(nan, 3, 700, 4, 4, 128, 0.09, 0)
    finally:
        eng.debug_set("vision_in_place", 1)
    torch.cuda.synchronize()
    for i, c in enumerate(cases):
        def judge(label, out, i=i, c=c):
            assert bool(torch.isfinite(out.float()).all()), f"{c} [{label}]: NaN from the dirtied arena reached the output"
            assert torch.equal(R._bits(out), R._bits(before[(i, label)])), f"{c} [{label}]: the result depends on what the arena held"
            if c.expect is not None:
                assert R.onehot_mismatch(out, c) is None

        for_every_form(eng, c, judge)
