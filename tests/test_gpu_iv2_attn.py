"""-m gpu: the attention launch of an InternVideo2 block, one launch at a time through gvl_op_iv2_attention on caller-owned buffers, against an INDEPENDENT reference
(tests/iv2_attn_ref.py) -- the ONES instantiations of attn_fwd_kernel (<96, 4, 2, 1, 0 | 1 | 3, 0>), the q-normalised-on-load operand mode and attn_iv2_pipe_kernel with 4
and 8 waves: its normal pass, the safe re-pass of a query block and the idle-wave loop.  test_gpu_towers.py compares these forms with each other (they share the q
prologue, the K pad column, the ones-column row sum, the tail mask, kperm, the V-image pad logic and the epilogue) and sees them through whole towers at 1.2e-2 .. 1.5e-2
of the output's maximum; this file names the (batch, head, row, d) that went wrong.

  list        iv2_attn_ref.cases(), built on the CPU -- the very data test_iv2_attn_ref_cpu.py judged with the emulation (passes predicted per 128-row block, late gaps
              realised, 15 mutations reported) -- and moved to the device.  Key tiles 1 .. 6 and 8, whole-tile lengths, tails of 1 / 32 / 33 / 40 / 63 keys, one real row in
              the last block (S = 129, 257: three idle waves), B x H = 1 x 3, 3 x 5, 2 x 8 (fewer than, not a multiple of, a multiple of the 8 XCD groups).  Dr = 88 runs
              form 2 under pipe 0 / 1 / 2 -- S >= 256: pipe 1 / 2 also with pipe_rows 256 (257, 321: 8-wave + 4-wave; 512: 8-wave alone) -- and forms 0 and 1; Dr = 72 / 80
              forms 0 and 1.  Every launch asserts the kernels it ran against the library's own plan (attn_plan.op_iv2_attention).
  exact       one-hot rows must equal the target's V row BIT FOR BIT: overflow (the target >= 185 log2 units above the first tile: exp2 overflows, the block repeats in the
              safe pass; blocks where every row, one row and no row needs it) and survive (p = 2^92 < 2^100: the normal pass keeps its result).
  bounded     dense data, float64 softmax on the rounded operands, ZERO elements outside iv2_attn_ref.elementwise_bound (derived there, no fitted factor).
  identities  a second run of the same launch; pipe 0 against pipe 2; pipe_rows 256 against 0; forms 0 against 1; pipe 1 against pipe 0 wherever the reference says no
              tile exceeds the first tile's maximum by more than 2^8 -- each bit for bit.
  buffers     out carries 160 guard rows of a sentinel that must survive; qkv is the prefix of an allocation whose next 64 rows are NaN, its k columns are NaN (no form
              reads them), ld is wider than 3 H Dr in half the cases with NaN in the extra columns; q_rs has NaN behind it; K slots behind the last key hold NaN (masked by
              index).  A V pad-chunk DMA or a tail tile that reads past the last real row comes out as 0 x NaN or NaN + 1, without any out-of-bounds access.
  joined      gvl_op_qkv_post (mode 1, q_rs, k_ones, ones_row) then gvl_op_iv2_attention on the same buffers: the pages are bit-identical to the reference's, so is the output.
  refusals    every documented precondition comes back as ERR_ARG naming the entry, with every output byte still the sentinel.

Observed on an MI355X: 99 tests, 1100 launches, zero differing bits, zero elements outside the bound, every identity and refusal clean.  Largest err / bound over the
bounded cases: form 0 0.991, form 1 0.991, form 2 pipe 0 0.991, pipe 1 0.991 (pipe_rows 256: 0.987), pipe 2 0.991 (0.987) -- the rows near 1 are late_gap / mixed_block rows
whose output is one or two V rows: the bound there is half a bf16 ulp of the store plus a little, and a store's rounding error reaches half an ulp.  Wall time of the file
5.9 s on its own, engine set-up included (in the same suite run the tests of test_gpu_attn_exact.py that show among the 60 slowest add up to 1.7 s; no test here does).
Passes the reference predicts for pipe 1, per 128-row query block over the list (2243 blocks of form 2): 996 repeat in the safe pass -- 439 because every row asks for it
(one-hot last / perm / edges, late_heavy at S >= 193, late_gap 104 / 126 / 150), 220 for one or two rows of the block (one_late, mixed_block, and scaled_rows: rows whose q is
scaled by 2^6) -- and 1247 keep the normal pass, among them all 158 blocks of the survive map "near" (p = 2^92) and every late_gap 4 / 12 / 40 / 96 block.
Found by this file: with pipe_rows 256 the 8-wave form voted the re-pass per 256-row block, the 4-wave form per 128 rows, so a row whose own sum was sane but whose
reference moves in the safe pass (a later tile 2^8 .. 2^100 above the first) came out of a different pass -- different roundings -- depending on pipe_rows: scaled_rows at
S = 257 and S = 512 differed in bits between pipe_rows 0 and 256 (first seen on the emulation, then on the GPU).  The 8-wave form now votes per 128-row half."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, bf, tiny_geo  # noqa: E402
from grounded_video_llm_amd import engine as E, lib as L  # noqa: E402
import attn_plan as A  # noqa: E402
import iv2_attn_ref as R  # noqa: E402
import qkv_post_ref as QP  # noqa: E402

T0 = time.time()
SPECS = R.cases()
NAN_ROWS = 64
WORST = {}            # (form, pipe, pipe_rows) -> largest err / bound
LAUNCHES = [0]
FWD = {0: ("fwd", 96, 4, 2, 1, 0, 0), 1: ("fwd", 96, 4, 2, 1, 1, 0), 2: ("fwd", 96, 4, 2, 1, 3, 0)}


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(tiny_geo(), DEV, towers=())
    yield e
    e.close()


def _bits(t):
    return t.contiguous().view(torch.int16)


def dev_bf(a):
    """numpy uint16 bit patterns -> bf16 tensor on the device"""
    return torch.from_numpy(a.view(np.int16).copy()).to(DEV).view(bf)


class Staged:
    """the device buffers of one case: built once, read by every launch of it"""

    def __init__(self, c_cpu):
        self.c = c = R.to_device(c_cpu, DEV)
        B, S, H, Dr = c.B, c.S, c.H, c.Dr
        self.rows = rows = B * S
        self.alloc = torch.full((rows + NAN_ROWS, c.ld), float("nan"), dtype=bf, device=DEV)
        self.alloc[:rows, :H * Dr] = c.x.reshape(rows, H * Dr)
        self.alloc[:rows, 2 * H * Dr:3 * H * Dr] = c.v.reshape(rows, H * Dr)
        self.rs = torch.full((rows + NAN_ROWS,), float("nan"), dtype=torch.float32, device=DEV)
        self.rs[:rows] = c.q_rs.reshape(-1)
        pg = R.pages(c_cpu)
        self.Q, self.Kt, self.Vt = dev_bf(pg["Q"]), dev_bf(pg["Kt"]), dev_bf(pg["Vt"])
        self.nw = c.q_nw.contiguous()

    def fields(self, form, pipe=0, pipe_rows=0):
        c = self.c
        kw = dict(Kt=self.Kt, B=c.B, S=c.S, H=c.H, Dr=c.Dr, scale=c.scale, form=form)
        if form == 0:
            kw.update(Q=self.Q, Vt=self.Vt)
        elif form == 1:
            kw.update(Q=self.Q, qkv=self.alloc[:self.rows], ld=c.ld)
        else:
            kw.update(qkv=self.alloc[:self.rows], ld=c.ld, q_rs=self.rs[:self.rows], q_nw=self.nw, pipe=pipe, pipe_rows=pipe_rows)
        return kw


def expected_kernels(c, form, pipe, pipe_rows):
    if form != 2 or pipe == 0:
        return [FWD[form]]
    rows8 = (c.S // 256) * 256 if pipe_rows == 256 else 0
    return ([("iv2_pipe", 8)] if rows8 else []) + ([("iv2_pipe", 4)] if c.S > rows8 else [])


def launch(eng, st, form, pipe=0, pipe_rows=0, **over):
    """one gvl_op_iv2_attention into a guarded buffer -> [B*S + GUARD, H*Dr] (iv2_attn_ref.judge looks at the guard rows); asserts which kernels the plan says it ran"""
    c = st.c
    plan = A.op_iv2_attention(c.B, c.S, c.H, c.Dr, form, pipe, pipe_rows, c.ld)
    assert plan is not None and [A.kernel_of(l) for l in plan] == expected_kernels(c, form, pipe, pipe_rows), f"{c} form {form} pipe {pipe} pipe_rows {pipe_rows}: the plan is {plan}"
    assert sum(l.q_rows for l in plan) == c.S and all(l.ONES == 1 for l in plan)
    buf = torch.full((st.rows + R.GUARD, c.H * c.Dr), R.SENT, dtype=bf, device=DEV)
    eng.op_iv2_attention(out=buf, **dict(st.fields(form, pipe, pipe_rows), **over))
    torch.cuda.synchronize()
    LAUNCHES[0] += 1
    return buf


@pytest.mark.parametrize("n", range(len(SPECS)), ids=lambda n: "%02d-%s-S%d" % (n, SPECS[n]["what"], SPECS[n]["S"]))
def test_every_case_every_launch(eng, n):
    c_cpu = R.build(SPECS[n])
    st = Staged(c_cpu)
    c = st.c
    bounds = {}
    if c.family == "bounded":
        for f in {2 if f == 2 else 0 for f in c.forms}:
            bounds[f] = R.elementwise_bound(c, f)
    outs = {}
    for f, pipe, pr in R.launches(c):
        what = f"{c} [form {f} pipe {pipe} pipe_rows {pr}: {expected_kernels(c, f, pipe, pr)}]"
        out = launch(eng, st, f, pipe, pr)
        ref, bound, _ = bounds.get(2 if f == 2 else 0, (None, None, None))
        msg, w = R.judge(c, f, out, ref, bound, what)
        if c.family == "bounded":
            WORST[f, pipe, pr] = max(WORST.get((f, pipe, pr), 0.0), w)
            print(f"[parity] iv2 attention {what}: worst err / bound {w:.3f}")
        assert msg is None, msg
        again = launch(eng, st, f, pipe, pr)
        assert torch.equal(_bits(again), _bits(out)), f"{what}: a second run of the same launch differs"
        outs[f, pipe, pr] = out
    eq = lambda a, b: torch.equal(_bits(outs[a]), _bits(outs[b]))
    assert eq((0, 0, 0), (1, 0, 0)), f"{c}: forms 0 and 1 differ"
    if 2 in c.forms:
        assert eq((2, 0, 0), (2, 2, 0)), f"{c}: pipe 0 (attn_fwd_kernel) and pipe 2 (the safe pass of attn_iv2_pipe_kernel) differ"
        if c.S >= 256:
            assert eq((2, 2, 0), (2, 2, 256)), f"{c}: pipe 2, pipe_rows 256 against 0"
            assert eq((2, 1, 0), (2, 1, 256)), f"{c}: pipe 1, pipe_rows 256 against 0"
        if R.pipe1_equals_pipe0(c):
            assert eq((2, 1, 0), (2, 0, 0)), f"{c}: no tile exceeds the first tile's maximum by 2^8, yet pipe 1 and pipe 0 differ"


def test_qkv_post_then_iv2_attention_on_the_same_buffers(eng):
    """gvl_op_qkv_post (mode 1 with q_rs, k_ones, ones_row; then once more without q_rs for the Q pages) writes what gvl_op_iv2_attention reads.  The data makes the norm
    EXACT: every element of a q / k row is +-2^e with one e per token, eps = 0, so the mean square is 4^e, rs = 2^-e and bf16(w * bf16(x * rs)) = +-w with no rounding
    anywhere.  The pages and q_rs must then be bit-identical to the reference's, and so must the attention output of every form on them."""
    B, S, H, Dr = 2, 129, 3, 88
    g = torch.Generator().manual_seed(99)
    sign = lambda *s: torch.where(torch.rand(s, generator=g) < 0.5, -1.0, 1.0)
    e_q, e_k = torch.randint(-1, 2, (B, S), generator=g).float(), torch.randint(-1, 2, (B, S), generator=g).float()
    c = R.Case(B, S, H, Dr, Dr ** -0.5, "joined", "bounded")
    c.x = (sign(B, S, H, Dr) * torch.exp2(e_q)[:, :, None, None]).to(bf)
    kraw = (sign(B, S, H, Dr) * torch.exp2(e_k)[:, :, None, None]).to(bf)
    c.q_rs = torch.exp2(-e_q)
    c.q_nw = (sign(H, Dr) * torch.exp2(torch.rand((H, Dr), generator=g) * 2 - 1)).to(bf)
    kn = (sign(H, Dr) * torch.exp2(torch.rand((H, Dr), generator=g) * 2 - 1)).to(bf)
    c.k = (kn.float()[None, None] * (kraw.float() * torch.exp2(-e_k)[:, :, None, None]).to(bf).float()).to(bf)
    c.v = torch.randn((B, S, H, Dr), generator=g).to(bf)
    c.forms, c.ld = (2, 0, 1), 3 * H * Dr + 16
    want_st = Staged(c)                                                    # the reference's pages, fed directly
    rows, nt = B * S, (S + 63) // 64
    qkv = want_st.alloc.clone()
    qkv[:rows, H * Dr:2 * H * Dr] = kraw.reshape(rows, H * Dr).to(DEV)
    sent = lambda shape: dev_bf(np.full(shape, QP.SENT, dtype=np.uint16))
    Q, Kt, Vt = sent((B * H * S * R.D,)), sent((B * nt, H, 64, R.D)), sent((B * nt, H, R.D, 64))
    rs = torch.full((rows + NAN_ROWS,), float("nan"), dtype=torch.float32, device=DEV)
    common = dict(qkv=qkv[:rows], ld=c.ld, Kt=Kt, B=B, S=S, H=H, KV=H, Dr=Dr, D=R.D, mode=1, qn=c.q_nw.to(DEV), kn=kn.to(DEV), eps=0.0, ones_row=1, k_ones=1, n_pages=B * nt)
    eng.op_qkv_post(Vt=Vt, q_rs=rs[:rows], **common)
    torch.cuda.synchronize()
    assert torch.equal(rs[:rows], want_st.rs[:rows]) and bool(torch.isnan(rs[rows:]).all()), "q_rs as gvl_op_qkv_post writes it"
    assert bool((_bits(Q) == _bits(sent((1,)))).all()), "q_rs set: Q is not written"
    eng.op_qkv_post(Q=Q, **common)                                         # the Q pages of forms 0 / 1 (K rewritten with the same bits; Vt NULL: not touched)
    torch.cuda.synchronize()
    assert torch.equal(_bits(Q), _bits(want_st.Q)), "Q as gvl_op_qkv_post writes it is not what gvl_op_iv2_attention reads"
    assert torch.equal(_bits(Vt), _bits(want_st.Vt)), "V^T pages"
    for b in range(B):
        for t in range(nt):
            m = min(64, S - t * 64)
            assert torch.equal(_bits(Kt[b * nt + t, :, :m]), _bits(want_st.Kt[b * nt + t, :, :m])), f"K page of batch {b}, tile {t}"
    got_st = Staged.__new__(Staged)
    got_st.__dict__.update(want_st.__dict__)
    got_st.alloc, got_st.rs, got_st.Q, got_st.Kt, got_st.Vt = qkv, rs, Q, Kt, Vt
    cd = want_st.c
    b2, b0 = R.elementwise_bound(cd, 2), R.elementwise_bound(cd, 0)
    for f, pipe, pr in R.launches(cd):
        want, got = launch(eng, want_st, f, pipe, pr), launch(eng, got_st, f, pipe, pr)
        assert torch.equal(_bits(got), _bits(want)), f"form {f} pipe {pipe}: the output on the pages gvl_op_qkv_post wrote differs from the one on the reference's pages"
        ref, bound, _ = b2 if f == 2 else b0
        msg, _ = R.judge(cd, f, got, ref, bound)
        assert msg is None, msg


def test_refusals_write_nothing_and_a_good_launch_follows(eng):
    spec = next(s for s in SPECS if s["what"] == "perm" and s["S"] == 129)
    st = Staged(R.build(spec))
    c = st.c
    rows = st.rows
    flat = lambda t: t.reshape(-1)[8:]                                      # 16 bytes in is fine ...
    odd = lambda t: t.reshape(-1)[1:]                                       # ... 2 bytes in is not
    refused = [
        ("form 3", 2, dict(form=3)), ("form -1", 2, dict(form=-1)), ("no Kt", 2, dict(Kt=None)), ("no out", 2, dict(out=None)),
        ("form 0 without Q", 0, dict(Q=None)), ("form 0 without Vt", 0, dict(Vt=None)), ("form 0 with qkv", 0, dict(qkv=st.alloc[:rows], ld=c.ld)),
        ("form 0 with q_rs", 0, dict(q_rs=st.rs[:rows])), ("form 0 with q_nw", 0, dict(q_nw=st.nw)),
        ("form 1 without Q", 1, dict(Q=None)), ("form 1 without qkv", 1, dict(qkv=None)), ("form 1 with Vt", 1, dict(Vt=st.Vt)), ("form 1 with q_rs", 1, dict(q_rs=st.rs[:rows])),
        ("form 1 with q_nw", 1, dict(q_nw=st.nw)),
        ("form 2 without qkv", 2, dict(qkv=None)), ("form 2 without q_rs", 2, dict(q_rs=None)), ("form 2 without q_nw", 2, dict(q_nw=None)), ("form 2 with Q", 2, dict(Q=st.Q)),
        ("form 2 with Vt", 2, dict(Vt=st.Vt)),
        ("B 0", 2, dict(B=0)), ("S 0", 1, dict(S=0)), ("H 0", 0, dict(H=0)), ("Dr 64", 0, dict(Dr=64)), ("Dr 96", 1, dict(Dr=96)), ("Dr 84", 0, dict(Dr=84)), ("form 2 at Dr 80", 2, dict(Dr=80)),
        ("pipe 3", 2, dict(pipe=3)), ("pipe -1", 2, dict(pipe=-1)), ("pipe_rows 128", 2, dict(pipe=1, pipe_rows=128)), ("pipe_rows 512", 2, dict(pipe=1, pipe_rows=512)),
        ("ld % 8", 2, dict(ld=c.ld + 4)), ("ld < 3 H Dr", 1, dict(ld=3 * c.H * c.Dr - 8)), ("more than 256 key tiles", 2, dict(S=256 * 64 + 1)),
        ("more than 256 key tiles, form 0", 0, dict(S=256 * 64 + 1)), ("qkv 2 bytes off", 2, dict(qkv=odd(st.alloc))), ("q_nw 2 bytes off", 2, dict(q_nw=odd(st.nw))),
        ("V rows 2 bytes off", 1, dict(qkv=odd(st.alloc))), ("out 2 bytes off", 2, "odd"),
    ]
    for name, form, kw in refused:
        buf = torch.full((rows + R.GUARD, c.H * c.Dr), R.SENT, dtype=bf, device=DEV)
        out = odd(buf) if kw == "odd" else buf
        with pytest.raises(L.GvlError) as ei:
            eng.op_iv2_attention(**dict(dict(st.fields(form, 1, 0), out=out), **({} if kw == "odd" else kw)))
        torch.cuda.synchronize()
        assert ei.value.status == L.ERR_ARG and "gvl_op_iv2_attention" in str(ei.value), (name, str(ei.value))
        assert bool((buf == R.SENT).all()), f"{name}: a refused launch wrote to the output"
    # 16-byte aligned views into larger allocations are served
    for f, pipe, pr in R.launches(c):
        msg, _ = R.judge(c, f, launch(eng, st, f, pipe, pr))
        assert msg is None, "after the refusals: " + msg
    shifted = torch.full((8 + st.alloc.numel(),), float("nan"), dtype=bf, device=DEV)
    shifted[8:] = st.alloc.reshape(-1)
    msg, _ = R.judge(c, 2, launch(eng, st, 2, 1, 0, qkv=flat(shifted)))
    assert msg is None, "qkv 16 bytes into its allocation: " + msg


def test_zz_report():
    """the figures for this file's docstring"""
    for f in (0, 1, 2):
        w = {k: v for k, v in WORST.items() if k[0] == f}
        print(f"[report] form {f}: largest err / bound " + ", ".join(f"pipe {k[1]} pipe_rows {k[2]}: {v:.3f}" for k, v in sorted(w.items())))
    print(f"[report] {LAUNCHES[0]} launches, wall time of the file {time.time() - T0:.1f} s")
