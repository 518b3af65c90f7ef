"""Independent reference for the attention launch of an InternVideo2 block (gvl_attn.hip: the ONES instantiations of attn_fwd_kernel, the q-normalised-on-load operand mode
and attn_iv2_pipe_kernel with 4 and 8 waves, reached one launch at a time through gvl_op_iv2_attention) -- plain torch / numpy, no GPU needed to import or run this file.

Non-causal self attention, B sequences of S tokens, H heads of Dr (72 / 80 / 88) padded to D = 96.  The softmax row sum is the ones row / column of V: it runs over the
bf16-ROUNDED probabilities.  Three forms (gvl_iv2_attn.form):
  0   Q, K pages, V^T pages with the ones row                 attn_fwd_kernel<96, 4, 2, 1, 0, 0>
  1   Q, K pages, V read in place from the token rows          attn_fwd_kernel<96, 4, 2, 1, 1, 0>
  2   q read in place and normalised on load, K pages whose pad column holds 1.0, V in place (Dr = 88): pipe 0 attn_fwd_kernel<96, 4, 2, 1, 3, 0>, pipe 1 attn_iv2_pipe_kernel
      <4> (pipe_rows 256: <8> for whole 256-row blocks, <4> for the rest), pipe 2 its safe pass only.
The page layouts are qkv_post_ref's (pages()): nothing about a layout is restated here.

Operand contract, in float32, bit for bit
  forms 0 / 1   the Q pages hold qn = bf16(w * bf16(fl32(x * rs))) (what gvl_op_qkv_post mode 1 writes); score s_j = fp32 sum of qn_d k_jd; p~_j = exp2(fmaf(s_j, sc, -fl(m sc))),
                sc = fl32(scale * log2(e)), m = a running maximum moved by the lazy rule (more than 2^8 above it, per 32-row wave) -- attn_ref.emulate's arithmetic
  form 2        the q fragment is qf_d = bf16( fl32( fl32( w_d * bf16(fl32(x_d * rs)) ) * sc ) ), d < 88: the scale rides in q.  Element 88 of q is MINUS the reference m (a bf16
                number, 0 at the start) and multiplies the 1.0 in K's pad column, so the MFMAs deliver s_j - m in log2 units and p~_j = exp2(that), a bare v_exp_f32.
                First tile: m = bf16(its row maximum).  Later tiles: pipe 1's normal pass never moves m; pipe 0 / 2 and the safe re-pass move it by the lazy rule to
                bf16(m + max(tile maximum - m, 0)) with alpha = exp2(m_old - m_new) on O AND on the row sum (it is a column of O).
  all forms     P rounded to bf16 for P.V; O and l = sum_j bf16(p~_j) accumulate in fp32; out = bf16(O * fl32(1 / l)).
  pipe 1        after the normal pass a row sum that is not in (0, 2^100) sends the WHOLE 128-row query block (the 8-wave form: that half of its block) through the safe pass.
The float64 softmax of reference() runs on these rounded operands (qn, or qf with the scale inside); the norm's own distance from the real-number norm is qkv_post_ref's subject.

Exact family: one-hot (onehot_case).  attn_ref.onehot_case's codes at Dr = 88: k_j = the +-1 code of j XOR mask(b, h) in nb = bit_length(S - 1) coordinates, q = mult x the
code of the target, scale = 1, q_rs = 1, q_nw = 1.  Worked out afresh for the folded form:
  mult 64   bf16(64) = 64, 64 sc = 92.33 -> the stored fragment is bf16(92.33) = 92.5 (bf16 spacing 0.5 in [64, 128)).  Scores are 92.5 x an integer of magnitude <= nb <= 9 minus
            a bf16 reference of magnitude <= 832.5: multiples of 0.25 below 2^11, exact in fp32 in any order.  The target scores 92.5 nb, every other key differs in >= 1 bit:
            92.5 (nb - 2), i.e. >= 185 log2 units behind.
    reference = bf16 of a row maximum, so the target's probability is exp2(92.5 nb - bf16(92.5 nb)): a number in [2^-2, 2^2] -- nb = 9: 832.5 -> 832, p = 2^0.5, bf16 1.4140625 --
            whose bf16 rounding p~ is what BOTH the product and the ones column see: l = p~ exactly, O = p~ v exactly (8 x 8 significand bits), every other key adds
            exp2(<= -185 + 2) = 0.  O * fl(1 / l) is within 2^-22 relative of v, whose bf16 neighbours are 2^-8 away: the store rounds back to the target's V row BIT FOR BIT.
    overflow  a target outside the first tile sits >= 185 log2 units above the first tile's maximum: pipe 1's normal pass computes exp2(185) = inf, the row sum is not sane
            and the block repeats in the safe pass, where the lazy rule must move the reference with alpha = exp2(-185) = 0.  Maps: attn_ref.FULL_MAPS (every block redone where
            S > 64), "first_tile" (targets < 64: no block redone) and "one_late" (first_tile, but one row per 128 rows targets key S - 1: the decision is block-wide, so the
            other 127 rows are recomputed although their own sums were sane).  V as attn_ref.onehot_v: normal bf16 of 2^-100 ... 2^100 (tied keys before the target are summed).
  mult 32   survive: the stored fragment is bf16(46.17) = 46.25, one bit of Hamming distance is 92.5 log2 units.  Map "near": every target is 64 * 2^k + r (r < 64), one bit away from
            key r of the first tile, so the first tile's maximum is 46.25 (nb - 2), the reference its bf16 rounding and the target's probability exp2(92.5 -+ rounding) ~ 2^92 <
            2^100: the normal pass MUST keep its result -- the one regime where attn_iv2_pipe_kernel's arithmetic is not attn_fwd_kernel's (pipe 0 / 2 move the reference there).
            V range: every other key has p <= exp2(0 + 2) = 4 (at or below the first tile's maximum, plus the reference's rounding), at most 2^9 of them, |v| <= 2^E: their sum
            is below 2^(11 + E), the target's term is at least 2^(91 - E) with an fp32 ulp of 2^(68 - E); absorbed in any summation order when 2^(11 + E) < 2^(67 - E), E <= 27.
            survive_v takes E = 20.  The ones column: 2^11 against an ulp of 2^68.  test_iv2_attn_ref_cpu.py asserts O == l v and l == bf16(l) > 2^90 on the emulation.
  The per-(batch, head) XOR mask makes a wrong head or batch a wrong target.  expect = a gather of V rows, no matmul.  attn_ref.onehot_mismatch names a failure.

Bounded family (bounded_case + elementwise_bound): dense data, float64 softmax on the rounded operands, a PER-ELEMENT bound, zero elements outside it.  Kinds: attn_ref.KINDS,
  late_gap(g)   plain data whose coordinate 0 is reserved: k_0 = 1 on ONE key j* >= 64 per (batch, head) and 0 elsewhere, q_0 chosen per row so that key j* scores g log2 units
                above the row's first-tile maximum (asserted on the rounded operands of form 2 to within one unit).  Where S > 65 the neighbour of j* is a copy of it moved by
                1.0 in coordinate 1 (a fraction of a unit in score, asserted within two units of g) with its own V row: the output is a mixture of two V rows at P ~ 2^g, not
                a one-hot row that any rounding would leave alone.  |v| reaches 2^10.  g in GAPS: both sides of the lazy rule's
                2^8, of the 2^100 sanity threshold and of fp32 overflow (2^128).
  mixed_block   one row per 128 rows at g = 150, the others plain: the block is redone for one row
  ragged_rs     q_rs spanning 2^-6 ... 2^6 over the tokens, q_nw 2^-1 ... 2^1 with both signs over (head, d), x = plain / rs: a wrong index into either is a wrong row

emulate(case, form, pipe, pipe_rows, mut)   the arithmetic above in plain torch: the CPU stand-in for a correct kernel, and with mut = one of MUTATIONS for wrong ones.
  Not a mutation: "the re-pass decided per wave instead of per block".  Both passes are correct arithmetic for a row whose own sum is sane, and they differ only by roundings
  inside the bound (or not at all: the exact family, rows whose reference never moves), so no comparison of VALUES can see which one computed a row.  What the block-wide
  decision protects is the barrier count of the block, not a value.
"""
import math

import numpy as np
import torch

import attn_ref as A
import qkv_post_ref as QP
from gemm_ref import U32, _mix, bf16_ulp

bf = torch.bfloat16
D = 96
LOG2E = np.float32(1.4426950408889634)
LAZY = 8.0
SANE = 2.0 ** 100
SENT = A.SENT
GUARD = 160
GAPS = (4, 12, 40, 96, 104, 126, 150)
EXACT_MAPS = A.FULL_MAPS + ("first_tile", "one_late", "near")
KINDS = A.KINDS + tuple(f"late_gap{g}" for g in GAPS) + ("mixed_block", "ragged_rs")
MUTATIONS = ("no_repass", "mask_plus", "mask_minus", "skip_kb2_at_33", "pad_dup", "vlast_no_ones", "k_pad_zero", "q_rs_prev", "q_rs_batch0", "q_nw_no_head", "scale_twice",
             "xcd_swap", "rows8_neither", "rows8_both", "alpha_split")


class Case:
    """x bf16 [B, S, H, Dr] (the raw q of the token rows), q_rs f32 [B, S], q_nw bf16 [H, Dr], k bf16 [B, S, H, Dr] (the K pages' content), v bf16 [B, S, H, Dr]; exact
    family: target [B, H, S], expect [B*S, H*Dr]"""

    def __init__(self, B, S, H, Dr, scale, what, family):
        self.B, self.S, self.H, self.KV, self.Dr, self.scale, self.what, self.family, self.causal = B, S, H, H, Dr, float(scale), what, family, 0
        self.target = self.expect = None

    def __str__(self):
        return f"{self.what} B{self.B} S{self.S} H{self.H} Dr{self.Dr}"


def _sc(c):
    return np.float32(c.scale) * LOG2E


def qn_of(c, mut=None):
    """bf16(w * bf16(fl32(x * rs))) as float32 [B, H, S, Dr]: the Q pages of forms 0 / 1, and the inner part of form 2's fragment"""
    B, S, H, Dr = c.B, c.S, c.H, c.Dr
    rs = c.q_rs
    if mut == "q_rs_prev":
        rs = rs.reshape(-1)[(torch.arange(B * S, device=rs.device) - 1).clamp_min(0)].view(B, S)
    if mut == "q_rs_batch0":
        rs = rs[:1].expand(B, S)
    w = c.q_nw.float()
    if mut == "q_nw_no_head":
        w = w[:1].expand(H, Dr)
    inner = (c.x.float() * rs[:, :, None, None]).to(bf).float()
    return (w[None, None] * inner).to(bf).float().permute(0, 2, 1, 3)


def qf_of(c, mut=None):
    """form 2's q fragment, elements 0 .. Dr - 1, float32 [B, H, S, Dr]"""
    B, S, H, Dr = c.B, c.S, c.H, c.Dr
    rs = c.q_rs
    if mut == "q_rs_prev":
        rs = rs.reshape(-1)[(torch.arange(B * S, device=rs.device) - 1).clamp_min(0)].view(B, S)
    if mut == "q_rs_batch0":
        rs = rs[:1].expand(B, S)
    w = c.q_nw.float()
    if mut == "q_nw_no_head":
        w = w[:1].expand(H, Dr)
    sc = torch.tensor(_sc(c), dtype=torch.float32, device=c.x.device)
    inner = (c.x.float() * rs[:, :, None, None]).to(bf).float()
    t = (w[None, None] * inner) * sc
    if mut == "scale_twice":
        t = t * sc
    return t.to(bf).float().permute(0, 2, 1, 3)


def pages(c):
    """-> dict of numpy uint16 arrays in qkv_post_ref's layouts on implicit pages (block_table NULL): Q [B H S D] flat (forms 0 / 1), Kt [n_pages, H, 64, D] with 1.0 in
    column Dr, Vt [n_pages, H, D, 64] with the ones row; K slots of keys >= S hold qkv_post_ref.SENT (a NaN: nobody writes them, the kernel masks by index).  Built by
    qkv_post_ref.emulate in mode 0 (copies) from qn, k and v: the layout is its, not this file's."""
    B, S, H, Dr = c.B, c.S, c.H, c.Dr
    p = QP.build(dict(form="single", geo=(H, H, Dr, D), mode=0, seed=0, B=B, S=S, pos0=0, table=False, vt=True, k_ones=1, ones_row=1, q_rs=False, ld_pad=0))
    bits = lambda t: t.contiguous().cpu().view(torch.int16).numpy().view(np.uint16)
    qn = qn_of(c).permute(0, 2, 1, 3).to(bf)
    p.qkv[:B * S, :3 * H * Dr] = np.concatenate([bits(qn).reshape(B * S, H * Dr), bits(c.k).reshape(B * S, H * Dr), bits(c.v).reshape(B * S, H * Dr)], 1)
    im = QP.emulate(p)
    nt = (S + 63) // 64
    return dict(Q=im.Q[:p.q_elems].copy(), Kt=im.Kt[:B * nt].copy(), Vt=im.Vt[:B * nt].copy())


# ---- exact family ----------------------------------------------------------------------------------------------------------------------------------------------------
def survive_v(B, S, H, Dr, seed, device="cpu"):
    """attn_ref.onehot_v with the exponent folded into 2^-20 ... 2^20 (see the module docstring)"""
    bits = A.onehot_v(B, S, H, Dr, seed, device).view(torch.int16).to(torch.int64) & 0xFFFF
    e = (bits >> 7) & 0xFF
    bits = (bits & 0x807F) | ((107 + (e - 27) % 41) << 7)
    return torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16).view(bf)


def exact_targets(B, S, H, target, seed, device="cpu"):
    i = torch.arange(S, device=device, dtype=torch.int64)[None, None, :]
    b = torch.arange(B, device=device, dtype=torch.int64)[:, None, None]
    h = torch.arange(H, device=device, dtype=torch.int64)[None, :, None]
    if target in A.FULL_MAPS:
        return A.targets(B, S, H, target, seed, device)
    hsh = _mix(b * 7919 + h * 104729 + i * 31 + seed * 13 + 3)
    first = hsh % min(S, 64)
    if target == "first_tile":
        return first
    if target == "one_late":
        late = (i % 128 == (37 + 11 * h + 5 * b) % 128) | ((i == S - 1) & ((S - 1) % 128 < (37 + 11 * h + 5 * b) % 128) & (b + h == 0))
        return torch.where(late, torch.full_like(first, S - 1), first)
    assert target == "near" and S > 64
    ks = [k for k in range(8) if 64 << k < S]                              # 64 * 2^k + r must be a key
    t = torch.zeros((B, H, S), dtype=torch.int64, device=device)
    r = hsh % 64
    pick = (hsh >> 7) % len(ks)
    for n, k in enumerate(ks):
        cand = (64 << k) + r
        cand = torch.where(cand < S, cand, torch.full_like(cand, 64 << k))      # r too large for the last, partial stretch: key 64 * 2^k itself (r = 0)
        t = torch.where(pick == n, cand, t)
    return t


def onehot_case(B, S, H, Dr, target, seed, device="cpu"):
    """see the module docstring.  target "near" is the survive sub-family (mult 32, survive_v), every other map the overflow sub-family (mult 64, attn_ref.onehot_v)"""
    assert target in EXACT_MAPS and Dr % 8 == 0
    nb = max(1, (S - 1).bit_length())
    assert nb <= 9 and nb <= Dr
    mult = 32.0 if target == "near" else 64.0
    c = Case(B, S, H, Dr, 1.0, f"one-hot {target}", "exact")
    c.mult = mult
    mask = _mix(torch.arange(B, device=device, dtype=torch.int64)[:, None] * 131 + torch.arange(H, device=device, dtype=torch.int64)[None, :] * 17 + seed + 7) % (1 << nb)
    j = torch.arange(S, device=device, dtype=torch.int64)
    c.k = A._code(j[None, :, None] ^ mask[:, None, :], nb, Dr).to(bf)                          # [B, S, H, Dr]
    c.target = exact_targets(B, S, H, target, seed, device)
    assert bool(((c.target >= 0) & (c.target < S)).all())
    c.x = (mult * A._code(c.target ^ mask[:, :, None], nb, Dr).permute(0, 2, 1, 3)).to(bf)     # [B, S, H, Dr]
    c.q_rs = torch.ones((B, S), dtype=torch.float32, device=device)
    c.q_nw = torch.ones((H, Dr), dtype=bf, device=device)
    c.v = survive_v(B, S, H, Dr, seed, device) if target == "near" else A.onehot_v(B, S, H, Dr, seed, device)
    vh = c.v.permute(0, 2, 1, 3)
    c.expect = torch.gather(vh, 2, c.target[..., None].expand(B, H, S, Dr)).permute(0, 2, 1, 3).reshape(B * S, H * Dr).contiguous()
    return c


# ---- bounded family --------------------------------------------------------------------------------------------------------------------------------------------------
def _scores2(c):
    """form 2's scores in log2 units on the rounded operands, float64 [B, H, S, S]"""
    return qf_of(c).double() @ c.k.permute(0, 2, 3, 1).double()


def bounded_case(B, S, H, Dr, kind, seed, device="cpu"):
    assert kind in KINDS
    base = kind if kind in A.KINDS else "plain"
    a = A.bounded_case(B, S, H, H, Dr, 0, base, seed, device)
    q, k, v = (t.clone() for t in a.split())
    c = Case(B, S, H, Dr, a.scale, kind, "bounded")
    c.x, c.k, c.v = q.contiguous(), k.contiguous(), v.contiguous()
    c.q_rs = torch.ones((B, S), dtype=torch.float32, device=device)
    c.q_nw = torch.ones((H, Dr), dtype=bf, device=device)
    g = torch.Generator(device=device)
    g.manual_seed(seed + 4711)
    if kind == "ragged_rs":
        c.q_rs = torch.exp2(torch.rand((B, S), device=device, generator=g) * 12 - 6)
        sign = torch.where(torch.rand((H, Dr), device=device, generator=g) < 0.5, -1.0, 1.0)
        c.q_nw = (sign * torch.exp2(torch.rand((H, Dr), device=device, generator=g) * 2 - 1)).to(bf)
        c.x = (q.float() / c.q_rs[:, :, None, None]).to(bf)
    gap = int(kind[8:]) if kind.startswith("late_gap") else 150 if kind == "mixed_block" else None
    if gap is not None:
        assert S > 64
        c.v = (v.float() * torch.exp2(torch.rand((1, 1, H, Dr), device=device, generator=g) * 10)).to(bf)
        bb = torch.arange(B, device=device)[:, None]
        hh = torch.arange(H, device=device)[None, :]
        c.jstar = 64 + (17 * hh + 29 * bb + seed) % (S - 64)                                    # [B, H]
        c.k[..., 0] = 0
        c.k[bb, c.jstar, hh, 0] = 1
        if S > 65:                                                                              # a second late key one step in coordinate 1 away: a MIXTURE at P ~ 2^g, not a one-hot row
            c.j2 = torch.where(c.jstar + 1 < S, c.jstar + 1, c.jstar - 1)
            c.k[bb, c.j2, hh] = c.k[bb, c.jstar, hh]
            c.k[bb, c.j2, hh, 1] = (c.k[bb, c.jstar, hh, 1].float() + 1).to(bf)
        c.x[..., 0] = 0
        s = _scores2(c)
        rest = torch.gather(s, 3, c.jstar[:, :, None, None].expand(B, H, S, 1))[..., 0]        # the score of j* without coordinate 0
        want = s[..., :64].amax(-1) + gap - rest                                                # what qf_0 should be, [B, H, S]
        rows = torch.ones((B, H, S), dtype=torch.bool, device=device)
        if kind == "mixed_block":
            i = torch.arange(S, device=device)[None, None, :]
            rows = (i % 128 == (53 + 7 * hh[..., None] + 3 * bb[..., None]) % 128) | (i == S - 1) & (bb[..., None] + hh[..., None] == 0)
        sc = float(_sc(c))
        x0 = want / sc
        best, err = torch.zeros_like(want), torch.full_like(want, float("inf"))
        for n in range(-4, 5):                                                                  # the neighbouring bf16 values of x0: two roundings lie between x_0 and qf_0
            cand = (x0 * (1 + n * 2.0 ** -8)).float().to(bf)
            qf0 = ((cand.float() * torch.tensor(sc, dtype=torch.float32, device=device)).to(bf)).double()
            e = (qf0 - want).abs()
            best, err = torch.where(e < err, cand.double(), best), torch.minimum(e, err)
        c.x[..., 0] = torch.where(rows, best, torch.zeros_like(best)).permute(0, 2, 1).to(bf)
        c.gap_rows, c.gap = rows, gap
        s = _scores2(c)
        got = torch.gather(s, 3, c.jstar[:, :, None, None].expand(B, H, S, 1))[..., 0] - s[..., :64].amax(-1)
        assert bool(((got - gap).abs()[rows] <= 1.0).all()), f"{c}: realised gap {float(got[rows].min())} .. {float(got[rows].max())}, wanted {gap}"
        top = s[..., 64:].amax(-1) - s[..., :64].amax(-1)                                       # the row's largest gap: j* or its neighbour (q_1 x 1 away: +-0.15 sigma)
        assert bool(((top - gap).abs()[rows] <= 2.0).all()), f"{c}: the largest gap of a row {float(top[rows].min())} .. {float(top[rows].max())}, wanted {gap}"
    return c


def max_gap(c):
    """the largest (maximum of a later tile - maximum of the first tile) over the rows, form 2's log2 units, and the largest |score|"""
    s = _scores2(c)
    late = s[..., 64:].amax(-1) if c.S > 64 else torch.full(s.shape[:-1], -float("inf"), dtype=torch.float64, device=s.device)
    return float((late - s[..., :64].amax(-1)).max()), float(s.abs().max())


def pipe1_equals_pipe0(c):
    """True when the reference says no tile exceeds the first tile's maximum by more than 2^8 -- with the margin the kernel's own reference needs: it is the bf16 ROUNDING
    of the first tile's maximum (2^-8 M away at most) -- so attn_fwd_kernel's lazy rule never fires after tile 0 and pipe 1 must equal pipe 0 bit for bit"""
    g, M = max_gap(c)
    return g <= LAZY - 2.0 ** -8 * M - 0.01


def reference(c, form):
    """float64 on the rounded operands -> x [B, H, S, S] scores in log2 units, Aq [B, H, S, S] = sum_d |q_d k_jd| in the same units"""
    kT = c.k.permute(0, 2, 3, 1).double()
    if form == 2:
        q = qf_of(c).double()
        return q @ kT, q.abs() @ kT.abs()
    q = qn_of(c).double()
    sc = c.scale * math.log2(math.e)
    return (q @ kT) * sc, (q.abs() @ kT.abs()) * sc


def elementwise_bound(c, form):
    """-> (ref, bound, Abs), float64 [B*S, H*Dr]: the float64 softmax attention on the form's rounded operands, a per-element bound on |kernel output - ref| that every
    pass of every kernel of the form meets, and Abs = p @ |v|.

    Derivation (no fitted factor; U = 2^-24, b = 2^-8).  One row; x_j its exact scores in log2 units, p = softmax_2(x), O* = sum_j p_j v_j, T = ceil(S / 64) key tiles,
    n = S + T, M = max_j |x_j|, A_j = sum_d |q_d k_jd| (>= |x_j|), m = the kernel's reference: a bf16 rounding of a partial row maximum, |m| <= (1 + 2^-6) M' with
    M' = max_j (|x_j| + (Dr + 2) U A_j) (one bf16 rounding of a computed maximum; 2^-6 instead of 2^-8 pays for the second-order terms).
      exponent, form 2    the MFMAs accumulate Dr products and 1.0 * (-m) in fp32 in some order: (Dr + 1) U (A_j + |m|) on s_j - m (running-sum bound).  A tile that was
                          computed against an older reference (tile 0; the tile pending at a move) is shifted by ONE fp32 subtraction of de = m_new - m_old, which is exact
                          itself (two bf16 numbers): U (|x_j| + |m|).  Together dx_j <= (Dr + 2) U (A_j + (1 + 2^-6) M').  A move multiplies what was accumulated by alpha =
                          exp2(-de) on the SAME exponent scale, so no rounding of the exponent comes with it.
      exponent, forms 0/1 attn_ref.elementwise_bound's: scale (Dr U A_j + 4 T U M') / ln 2 in log2 units (fp32 score, the fmaf, sc = fl(scale fl(log2 e)), T - 1 moves).
      v_exp_f32           1 ulp = 2 U relative, once for p~_j and once per move for alpha (at most T - 1 moves): (1 + 2 U)^T.
                          eps_j = 2^dx_j (1 + 2 U)^T - 1: the relative error of the probability BEFORE its rounding to bf16.
      P                   p^_j = p~_j (1 + d_j), |d_j| <= b, is what BOTH the product and the row sum see (the ones column).  With c_j = (1 + eps_j)(1 + d_j) - 1 common to both,
                            O_acc / W = sum_j p_j (1 + c_j)(1 + th_j) v_j,   l_acc / W = sum_j p_j (1 + c_j)(1 + th'_j),   W = sum_j 2^(x_j - m)
                          th, th': fp32 accumulation of n terms including the T rescales, |th| <= n U =: gam -- the running-sum bound holds for any order and covers absorption
                          (a key at P ~ 2^92 swallowing the rest IS rounding error of these additions).  Then
                            O_acc / l_acc - O* = [ sum_j p_j c_j (v_j - O*)  +  sum_j p_j (1 + c_j)(th_j v_j - th'_j O*) ] / (1 + sum_j p_j ((1 + c_j)(1 + th'_j) - 1))
                          The leading term: the rounding of a probability moves the output only as far as that key's V row is from the output.  With cb = (1 + max_j eps_j)
                          (1 + b) - 1 and Jensen,  sum_j p_j |v_j - O*| <= sqrt(sum_j p_j v_j^2 - O*^2) =: sig  (+ the float64 cancellation of that difference, 2^-50 p @ v^2):
                            e1 = ( cb sig + gam (1 + cb)(Abs + |O*|) ) / (1 - ((1 + cb)(1 + gam) - 1))
      epilogue            one fp32 reciprocal (2 U) and one product (U): e2 = e1 + 3 U (|O*| + e1);  store: half a bf16 ulp at |O*| + e2.
      flush               probabilities (and an alpha) below 2^-126 are flushed.  Against l_acc / W >= 2^(-2^-6 M') (the key that set the reference) and at most S 2^8 of
                          accumulated mass per unit of |v| before a move: S 2^8 2^-126 2^(2^-6 M') <= 2^-93 < 2^-90 max_j |v_jd| for S <= 2^9 and M' <= 1024 -- asserted.
    The same bound serves the normal pass (no moves), the safe pass and attn_fwd_kernel: it charges every pass the T moves."""
    B, S, H, Dr = c.B, c.S, c.H, c.Dr
    x, Aq = reference(c, form)
    v = c.v.permute(0, 2, 1, 3).double()
    va = v.abs()
    T = float((S + 63) // 64)
    n = S + T
    b8 = 2.0 ** -8
    if form == 2:
        Mp = (x.abs() + (Dr + 2) * U32 * Aq).amax(-1, keepdim=True)
        dx = (Dr + 2) * U32 * (Aq + (1 + 2.0 ** -6) * Mp)
    else:
        Mp = (x.abs() + Dr * U32 * Aq).amax(-1, keepdim=True)
        dx = Dr * U32 * Aq + 4 * T * U32 * Mp
    assert S <= 512 and float(Mp.max()) <= 1024, (S, float(Mp.max()))
    eps = (torch.exp2(dx) * (1 + 2 * U32) ** T - 1).amax(-1, keepdim=True)                    # [B, H, S, 1]
    cb = (1 + eps) * (1 + b8) - 1
    p = torch.softmax(x * math.log(2.0), -1)
    o, Ab, sq = p @ v, p @ va, p @ (v * v)
    sig = torch.sqrt((sq - o * o).clamp_min(0) + 2.0 ** -50 * sq)
    gam = n * U32
    e1 = (cb * sig + gam * (1 + cb) * (Ab + o.abs())) / (1 - ((1 + cb) * (1 + gam) - 1))
    e2 = e1 + 3 * U32 * (o.abs() + e1)
    bound = e2 + 0.5 * bf16_ulp(o.abs() + e2) + 2.0 ** -90 * va.amax(2, keepdim=True)
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(B * S, H * Dr)
    return flat(o), flat(bound), flat(Ab)


# ---- the kernels' arithmetic in plain torch ----------------------------------------------------------------------------------------------------------------------------
def _ftz(t):
    return torch.where(t.abs() < 2.0 ** -126, torch.zeros_like(t), t)


def _rbf(t):
    return t.to(bf).float()


def blocks_of(S):
    """the units of attn_iv2_pipe_kernel's re-pass vote as (first row, one past the last): 128 query rows -- a block of the 4-wave form, HALF a block of the 8-wave form,
    so that the pass which computes a row does not depend on pipe_rows"""
    return [(r, min(S, r + 128)) for r in range(0, S, 128)]


def emulate(c, form=2, pipe=1, pipe_rows=0, mut=None, guard=GUARD, info=None):
    """-> bf16 [B*S + guard, H*Dr], the guard rows SENT.  info (dict): "redo" = [(b, h, first row, rows whose sum is not sane, real rows)] of the blocks pipe 1 repeats in the safe pass, "blocks" =
    their number in all, "moved" = whether a reference moved after tile 0, "O" / "l" = the accumulators [B, H, S, Dr] / [B, H, S] before the division.
    mut (MUTATIONS) -- a WRONG kernel:
      no_repass            pipe 1 keeps the normal pass whatever the row sum is
      mask_plus / _minus   the tail mask lets key S through (the K slot behind the last key: modelled as a duplicate of key S - 1, as the in-place V image's pad rows are) /
                           hides key S - 1
      skip_kb2_at_33       the second 32-key block of the last tile is skipped when the tail holds <= 33 keys instead of <= 32 (pipe 1 / 2, more than one tile)
      pad_dup              no tail mask at all, K and V pad rows duplicate key S - 1 (forms 1 / 2: the in-place V image)
      vlast_no_ones        the V slot of a partial last tile has no ones column: its keys are missing from the row sum (pipe 1 / 2)
      k_pad_zero           K's pad column reads 0: the reference is never subtracted inside the MFMAs (form 2)
      q_rs_prev, q_rs_batch0, q_nw_no_head, scale_twice     q_rs of token i - 1 / of batch 0, q_nw of head 0, q multiplied by sc twice (form 2)
      xcd_swap             the group decode takes (batch, head) of group g = b H + h as (g % B, g // B) for K and V, while q and the output keep (b, h)
      rows8_neither / _both   pipe_rows 256 with 0 < rows8 < S: the rows >= rows8 are written by no launch / the 8-wave launch runs on past rows8 and writes the
                           (B - 1, S - 1) result into the rows behind the output (the same VALUES written twice over real rows cannot be seen)
      alpha_split          a reference move rescales O but not the row sum"""
    assert mut is None or mut in MUTATIONS
    B, S, H, Dr = c.B, c.S, c.H, c.Dr
    dev = c.x.device
    k = c.k.permute(0, 2, 1, 3).float()
    v = c.v.permute(0, 2, 1, 3).float()
    if mut == "xcd_swap":
        g = torch.arange(B * H, device=dev)
        k = k.reshape(B * H, S, Dr)[(g % B) * H + (g // B) % H].view(B, H, S, Dr)
        v = v.reshape(B * H, S, Dr)[(g % B) * H + (g // B) % H].view(B, H, S, Dr)
    nt = (S + 63) // 64
    pad = nt * 64 - S
    tail = S - (nt - 1) * 64
    unmask = mut in ("pad_dup", "mask_plus")
    if pad:
        dup = lambda t: t[:, :, S - 1:S].expand(B, H, pad, Dr)
        k = torch.cat([k, dup(k) if unmask else torch.zeros((B, H, pad, Dr), device=dev)], 2)
        v = torch.cat([v, dup(v) if unmask and form else torch.zeros((B, H, pad, Dr), device=dev)], 2)
    v1 = torch.cat([v, torch.ones((B, H, nt * 64, 1), device=dev)], -1)                        # the ones column: O[..., Dr] is the row sum
    if mut == "vlast_no_ones" and pad and form == 2 and pipe:
        v1[:, :, (nt - 1) * 64:, Dr] = 0
    G = (S + 31) // 32
    limit = S + 1 if mut == "mask_plus" else S - 1 if mut == "mask_minus" else nt * 64 if mut == "pad_dup" else S
    sc32 = torch.tensor(_sc(c), dtype=torch.float32, device=dev)
    q = qf_of(c, mut) if form == 2 else qn_of(c)
    moved = [False]

    def wave_any(t):
        t = torch.cat([t, torch.zeros((B, H, G * 32 - S), dtype=torch.bool, device=dev)], -1).view(B, H, G, 32).any(-1)
        return t.repeat_interleave(32, dim=-1)[..., :S]

    def one_pass(lazy):
        m = torch.zeros((B, H, S), dtype=torch.float32, device=dev) if form == 2 else torch.full((B, H, S), -1e30, dtype=torch.float32, device=dev)
        O = torch.zeros((B, H, S, Dr + 1), dtype=torch.float32, device=dev)
        for t in range(nt):
            keys = torch.arange(t * 64, t * 64 + 64, device=dev)
            raw = q.double() @ k[:, :, t * 64:t * 64 + 64].transpose(-1, -2).double()
            dead = keys >= limit
            if mut == "skip_kb2_at_33" and form == 2 and pipe and nt > 1 and t == nt - 1 and tail <= 33:
                dead = dead | (keys >= t * 64 + 32)
            if form == 2:
                s = raw.float() if mut == "k_pad_zero" else (raw - m.double()[..., None]).float()
                s = torch.where(dead, torch.full_like(s, -1e30), s)
                mx = s.amax(-1)
                if t == 0:
                    m_new, alpha = _rbf(m + mx), None
                elif lazy:
                    vote = wave_any(mx > LAZY)
                    moved[0] = moved[0] or bool(vote.any())
                    m_new = torch.where(vote, _rbf(m + mx.clamp_min(0)), m)
                    alpha = _ftz(torch.exp2(-(m_new - m).double()).float())
                else:
                    m_new, alpha = m, None
                s = s - (m_new - m)[..., None]
                m = m_new
                p = _ftz(torch.exp2(s.double()).float())
            else:
                s = torch.where(dead, torch.full_like(raw.float(), -1e30), raw.float())
                mx = s.amax(-1)
                vote = wave_any((mx - m) * sc32 > LAZY)
                moved[0] = moved[0] or (t > 0 and bool(vote.any()))
                m_new = torch.where(vote, torch.maximum(m, mx), m)
                alpha = _ftz(torch.exp2(((m - m_new) * sc32).double()).float())
                m = m_new
                p = _ftz(torch.exp2(s.double() * float(sc32) + (-m * sc32).double()[..., None]).float())
            if alpha is not None:
                if mut == "alpha_split":
                    O = torch.cat([O[..., :Dr] * alpha[..., None], O[..., Dr:]], -1)
                else:
                    O = O * alpha[..., None]
            O = O + p.to(bf).float() @ v1[:, :, t * 64:t * 64 + 64]
        return O

    redo_list, blocks = [], blocks_of(S)
    if form != 2 or pipe != 1:
        O = one_pass(True)
    else:
        O = one_pass(False)
        l = O[..., Dr]
        sane = (l > 0) & (l < SANE)
        redo = torch.zeros((B, H, S), dtype=torch.bool, device=dev)
        for r0, r1 in blocks:
            blk = ~sane[..., r0:r1].all(-1)                                                      # [B, H]: block-wide
            redo[..., r0:r1] = blk[..., None]
            bad = (~sane[..., r0:r1]).sum(-1)
            redo_list += [(int(b), int(h), r0, int(bad[b, h]), r1 - r0) for b, h in blk.nonzero().tolist()]
        if mut == "no_repass":
            redo[:] = False
        if bool(redo.any()):
            O = torch.where(redo[..., None], one_pass(True), O)
    l = O[..., Dr]
    out = (O[..., :Dr] * (1.0 / l)[..., None]).to(bf).permute(0, 2, 1, 3).reshape(B * S, H * Dr)
    out = torch.cat([out, torch.full((guard, H * Dr), SENT, dtype=bf, device=dev)])
    rows8 = (S // 256) * 256 if (pipe_rows == 256 and form == 2 and pipe) else 0
    if 0 < rows8 < S:
        if mut == "rows8_neither":
            out.view(-1, H * Dr)[:B * S].view(B, S, H * Dr)[:, rows8:] = SENT
        if mut == "rows8_both":
            out[B * S:B * S + min(guard, rows8 + 256 - S)] = out[B * S - 1]
    if info is not None:
        info.update(redo=redo_list, blocks=B * H * len(blocks), moved=moved[0], O=O[..., :Dr], l=l)
    return out


def judge(c, form, got, ref=None, bound=None, what=""):
    """THE comparison of both tests: got [B*S + guard, H*Dr].  -> (message or None, worst err / bound or 0.0): the guard rows must hold SENT; exact family: bit for bit
    (attn_ref.onehot_mismatch); bounded family: zero elements outside the bound (attn_ref.bound_violations)"""
    what = what or f"{c} form {form}"
    rows = c.B * c.S
    if got.shape[0] < rows or got.shape[1] != c.H * c.Dr:
        return f"{what}: shape {tuple(got.shape)}", float("inf")
    touched = (got[rows:] != SENT).nonzero()
    if touched.numel():
        return f"{what}: {touched.shape[0]} elements of the rows BEYOND B*S written, first at row {rows + int(touched[0][0])}, column {int(touched[0][1])}", float("inf")
    if c.family == "exact":
        return A.onehot_mismatch(got[:rows], c, what), 0.0
    return A.bound_violations(got[:rows], ref, bound, c, what)


# ---- THE list of test_gpu_iv2_attn.py --------------------------------------------------------------------------------------------------------------------------------
BH = ((1, 3), (3, 5), (2, 8))            # fewer than, not a multiple of, a multiple of the 8 XCD groups
# key tiles 1 .. 6 and 8, whole-tile lengths, tails of 1 / 32 / 33 / 63 keys, one real row in the last query block (129, 257), 8-wave + 4-wave (257, 321) and 8-wave alone (512)
S_LIST = (40, 64, 65, 96, 97, 127, 128, 129, 161, 192, 193, 257, 321, 512)


def cases():
    """-> list of dict(family, B, S, H, Dr, what (map / kind), seed, forms, ld_pad).  Dr = 88 runs every form; Dr = 72 / 80 forms 0 / 1 only (form 2 takes 88 alone)"""
    out = []

    def add(family, S, what, Dr=88):
        n = len(out)
        B, H = BH[n % 3]
        out.append(dict(family=family, B=B, S=S, H=H, Dr=Dr, what=what, seed=n + 1, forms=(2, 0, 1) if Dr == 88 else (0, 1), ld_pad=(0, 16)[n % 2]))

    for n, S in enumerate(S_LIST):                                           # overflow: every S twice over the three full maps
        add("exact", S, A.FULL_MAPS[n % 3])
        add("exact", S, A.FULL_MAPS[(n + 1) % 3])
    for S in (65, 129, 193, 257, 321, 512):                                  # survive; sane blocks; one non-sane row per block
        add("exact", S, "near")
    for S in (64, 129, 257, 321, 512):
        add("exact", S, "first_tile")
    for S in (129, 257, 321, 512):
        add("exact", S, "one_late")
    add("exact", 193, "perm", 72)
    add("exact", 97, "last", 80)
    for n, kind in enumerate(A.KINDS):
        for S in ((40, 97, 193, 321), (65, 129, 257, 512))[n % 2]:
            add("bounded", S, kind)
    for n, g in enumerate(GAPS):
        for S in ((65, 161, 321), (129, 257, 512))[n % 2]:
            add("bounded", S, f"late_gap{g}")
    for S in (129, 257, 321, 512):
        add("bounded", S, "mixed_block")
    for S in (40, 129, 257, 321):
        add("bounded", S, "ragged_rs")
    add("bounded", 193, "late_heavy", 72)
    add("bounded", 129, "plain", 80)
    return out


def build(spec, device="cpu"):
    f = onehot_case if spec["family"] == "exact" else bounded_case
    c = f(spec["B"], spec["S"], spec["H"], spec["Dr"], spec["what"], spec["seed"], device)
    c.spec, c.forms, c.ld = spec, spec["forms"], 3 * spec["H"] * spec["Dr"] + spec["ld_pad"]
    return c


def to_device(c, device):
    """the same case (built on the CPU: the data test_iv2_attn_ref_cpu.py judged) with its tensors on `device`"""
    d = Case.__new__(Case)
    d.__dict__.update({k: (v.to(device) if torch.is_tensor(v) else v) for k, v in c.__dict__.items()})
    return d


def launches(c):
    """(form, pipe, pipe_rows) of every launch a case gets: forms 0 / 1 once; form 2 under pipe 0, 1, 2 and -- S >= 256 -- pipe 1, 2 with pipe_rows 256"""
    out = []
    for f in c.forms:
        if f != 2:
            out.append((f, 0, 0))
        else:
            out += [(2, 0, 0), (2, 1, 0), (2, 2, 0)] + ([(2, 1, 256), (2, 2, 256)] if c.S >= 256 else [])
    return out
