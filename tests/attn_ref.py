"""Independent references for the flash-attention kernel (attn_fwd_kernel in gvl_attn.hip, reached through gvl_op_attention) -- no GPU needed to import or run this file.

Why: gpu_util.check() is max|got - ref| / max|ref| over the whole output against fp32 torch.  A causal output's scale is set by its first rows (row 0 is v[0], ~4 on std-1
data) while a long row's output is ~0.1, so anything confined to a few long rows, one key or one query block's last wave disappears; and on dense random data one key of
a long row carries less mass than one bf16 rounding of the output, so no tolerance can say "this key was counted exactly once".  The other attention tests compare kernel
forms that share the mask, kperm, the lazy reference point and the epilogue with each other.  Two families of cases replace the statistic, as gemm_ref.py does for the GEMM:

onehot_case(B, S, H, KV, Dr, causal, target, seed)   every query row attends to EXACTLY one key and the output must equal that key's V row BIT FOR BIT.
    k[b, kvh, j]  the +-1 binary code of j XOR mask(b, kvh) in the first nb = bit_length(S - 1) coordinates, 0 elsewhere (nb <= 14 <= Dr for every supported S); the
                  per-(batch, KV head) mask turns a wrong head or batch mapping into a wrong target
    q[b, h, i]    64 code(t XOR mask), t = target(b, h, i); called with scale = 1.0
    scores        integers of magnitude <= 64 nb <= 896: exact in fp32 in any order.  The target scores 64 nb, every other key differs in >= 1 bit: <= 64 (nb - 2), i.e. 128 raw
                  units = 184 log2 units behind -> every other probability is exp2(<= -184) = 0 in fp32 and P is one-hot.
    l             1 up to the residual of fmaf(m, sc, -fl(m sc)): |m sc| < 2^11, so the residual is below half an fp32 ulp of it, 2^-14 ~ 6e-5, p(target) = exp2(that) is
                  within 5e-5 of 1 and rounds to bf16 1.0 for the product.  O = v[t] exactly, and v[t] / l is within 5e-5 relative of a bf16 number whose neighbours are
                  >= 2^-8 relative away: the residual cannot move the bf16 rounding of the store.
    reference     before a row's target tile arrives its reference point sits >= 184 log2 units below the target, so the lazy rule (a.lazy = 8) MUST move it, with alpha =
                  exp2(<= -184) = 0: the rescale path runs on every row whose target is not in its first tile, and whatever was accumulated before is wiped.
    V             bf16 bit patterns hashed from (b, kvh, j, d): both signs, the 7 mantissa bits distinct over d within a row, NORMAL values with 2^-100 <= |v| < 2^101 only:
                  before the target tile arrives several keys of one tile can tie at p = 1 and their V rows are summed (<= 2^14 2^101, finite); with unrestricted exponents
                  that sum overflows and the following alpha = 0 gives inf 0 = NaN.  Subnormals are excluded because the MFMA pipe flushes them.
    expect        v[b, kvh(h), t] -- a gather, no matmul.
  A one-hot row cannot see a duplicated key whose V row is duplicated too: (1 + n) v / (1 + n) rounds back to v.  That defect (unmasked pad keys of the in-place forms) belongs
  to the bounded kind late_heavy; the exact family sees it where the pad V is not the duplicate (V^T pages: zeros).

bounded_case(B, S, H, KV, Dr, causal, kind, seed) + elementwise_bound(case)   dense data that puts each row's mass where the kernel is fragile (KINDS below), a float64
  softmax on the bf16 operands and a PER-ELEMENT bound that is derived, not measured -- see elementwise_bound.

emulate(case)   the kernel's documented arithmetic in plain torch: the CPU stand-in for a correct kernel (and, with mut=..., for eight wrong ones: test_attn_ref_cpu.py).
"""
import math

import numpy as np
import torch

from gemm_ref import U32, _mix, bf16_ulp

bf = torch.bfloat16
LOG2E = np.float32(1.4426950408889634)
LAZY = 8.0                      # a.lazy (gvl_launch_attention)
SENT = -7.0                     # fill of output rows / columns nobody may write
CAUSAL_MAPS = ("diag", "prev", "tile_first", "zero", "hash")
FULL_MAPS = ("last", "perm", "edges")
KINDS = ("late_heavy", "early_heavy", "spike", "scaled_rows", "plain")
MUTATIONS = ("mask_plus", "mask_minus", "drop_diag", "pad_dup", "pad_dup_vzero", "swap_pv", "gqa_mod", "no_rescale_O", "skip_last8", "rows_shift")


class Case:
    """qkv bf16 [B*S, (H+2KV)*Dr] (the fused layout gvl_op_attention requires) + how to call; expect / target / v (exact family) or nothing more (bounded family)"""

    def __init__(self, B, S, H, KV, Dr, scale, causal, what):
        self.B, self.S, self.H, self.KV, self.Dr, self.scale, self.causal, self.what = B, S, H, KV, Dr, float(scale), int(causal), what
        self.qkv = self.expect = self.target = None

    def split(self):
        """-> q [B, S, H, Dr], k [B, S, KV, Dr], v [B, S, KV, Dr] (views of qkv)"""
        t = self.qkv.view(self.B, self.S, self.H + 2 * self.KV, self.Dr)
        return t[:, :, :self.H], t[:, :, self.H:self.H + self.KV], t[:, :, self.H + self.KV:]

    def __str__(self):
        return f"{self.what} B{self.B} S{self.S} H{self.H}/{self.KV} D{self.Dr} causal{self.causal}"


def _fuse(c, q, k, v):
    c.qkv = torch.cat([q, k, v], dim=2).reshape(c.B * c.S, (c.H + 2 * c.KV) * c.Dr).to(bf).contiguous()
    return c


# ---- exact family --------------------------------------------------------------------------------------------------------------------------------------------------
def _code(x, nb, Dr):
    """x int64 [...] -> [..., Dr] float: +-1 by bit c of x for c < nb, 0 beyond"""
    bits = (x[..., None] >> torch.arange(nb, device=x.device, dtype=torch.int64)) & 1
    out = torch.zeros(x.shape + (Dr,), dtype=torch.float32, device=x.device)
    out[..., :nb] = (2 * bits - 1).float()
    return out


def _coprime(a, S):
    a = max(1, a % S) if S > 1 else 1
    while math.gcd(a, S) != 1:
        a += 1
    return a


def targets(B, S, H, target, seed, device="cpu"):
    """-> int64 [B, H, S]: the one key row (b, h, i) attends to"""
    i = torch.arange(S, device=device, dtype=torch.int64)[None, None, :]
    b = torch.arange(B, device=device, dtype=torch.int64)[:, None, None]
    h = torch.arange(H, device=device, dtype=torch.int64)[None, :, None]
    z = torch.zeros((B, H, S), dtype=torch.int64, device=device)
    if target == "diag":
        return z + i
    if target == "prev":
        return z + (i - 1).clamp_min(0)
    if target == "tile_first":
        return z + (i - i % 64)
    if target == "zero":
        return z
    if target == "hash":
        return _mix(b * 7919 + h * 104729 + i * 31 + seed * 13 + 3) % (i + 1)
    if target == "last":
        return z + (S - 1)
    if target == "perm":                      # (a i + c) mod S, a coprime to S: a bijection per (b, h); a and c move with the head, so over the heads every key is hit
        t = z.clone()                         # from every query block
        for bb in range(B):
            for hh in range(H):
                a = _coprime(37 + 64 * hh + 2 * bb + seed, S)
                t[bb, hh] = (a * i[0, 0] + 29 * hh + 11 * bb + seed) % S
        return t
    if target == "edges":
        e = sorted({x for x in (0, 31, 32, 63, 64, 65, S - 2, S - 1) if 0 <= x < S})
        return torch.tensor(e, device=device, dtype=torch.int64)[(i + h + 3 * b) % len(e)] + z
    raise ValueError(target)


def onehot_v(B, S, KV, Dr, seed, device="cpu"):
    """bf16 [B, S, KV, Dr]: hashed bit patterns, sign | exponent 27 ... 227 (2^-100 ... 2^100) | 7 mantissa bits that are distinct over d within a row"""
    b, j, g, d = (torch.arange(n, device=device, dtype=torch.int64).view(s) for n, s in ((B, (-1, 1, 1, 1)), (S, (1, -1, 1, 1)), (KV, (1, 1, -1, 1)), (Dr, (1, 1, 1, -1))))
    row = _mix(b * 1000003 + g * 50021 + j * 97 + seed * 7 + 1)
    h = _mix(row + d * 40503 + 5)
    bits = ((h >> 20) & 1) << 15 | (27 + h % 201) << 7 | (d + row) % 128
    bits = torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16)
    return bits.view(bf)


def onehot_case(B, S, H, KV, Dr, causal, target, seed, device="cpu"):
    """see the module docstring.  -> Case with qkv, scale = 1.0, target [B, H, S], v [B, S, KV, Dr] and expect [B*S, H*Dr] (bf16)"""
    assert H % KV == 0 and Dr % 8 == 0 and target in (CAUSAL_MAPS if causal else FULL_MAPS)
    nb = max(1, (S - 1).bit_length())
    assert nb <= 14 and nb <= Dr
    c = Case(B, S, H, KV, Dr, 1.0, causal, f"one-hot {target}")
    rep = H // KV
    mask = _mix(torch.arange(B, device=device, dtype=torch.int64)[:, None] * 131 + torch.arange(KV, device=device, dtype=torch.int64)[None, :] * 17 + seed + 7) % (1 << nb)   # [B, KV]
    j = torch.arange(S, device=device, dtype=torch.int64)
    k = _code(j[None, :, None] ^ mask[:, None, :], nb, Dr)                                       # [B, S, KV, Dr]
    c.target = targets(B, S, H, target, seed, device)
    if causal:
        assert bool((c.target <= j[None, None, :]).all())
    assert bool(((c.target >= 0) & (c.target < S)).all())
    qmask = mask.repeat_interleave(rep, dim=1)                                                   # [B, H]: query head h belongs to KV head h // (H / KV)
    q = 64.0 * _code(c.target ^ qmask[:, :, None], nb, Dr).permute(0, 2, 1, 3)                   # [B, S, H, Dr]
    c.v = onehot_v(B, S, KV, Dr, seed, device)
    _fuse(c, q.to(bf), k.to(bf), c.v)
    vh = c.v.permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)                                   # [B, H, S, Dr]
    exp = torch.gather(vh, 2, c.target[..., None].expand(B, H, S, Dr))
    c.expect = exp.permute(0, 2, 1, 3).reshape(B * S, H * Dr).contiguous()
    return c


def _bits(t):
    return t.contiguous().view(torch.int16)


def _where(c, r, col):
    b, i, h, d = r // c.S, r % c.S, col // c.Dr, col % c.Dr
    return b, h, i, d


def onehot_mismatch(got, c, what=""):
    """None when got [B*S, H*Dr] equals the expectation bit for bit (NaN never does), else the message the tests fail with: the count of wrong elements and, for the first
    and the last one, (b, h, i, d), the target key, the query block (i // 128), the wave ((i % 128) // 32), the key tile (t // 64) and -- where it can tell -- which other
    key's V row the output row equals instead."""
    what = what or str(c)
    if got.shape != c.expect.shape or got.dtype != c.expect.dtype:
        return f"{what}: shape / dtype {tuple(got.shape)} {got.dtype}, expected {tuple(c.expect.shape)} {c.expect.dtype}"
    bad = (_bits(got) != _bits(c.expect)).nonzero()
    if bad.numel() == 0:
        return None
    rep = c.H // c.KV

    def describe(rc):
        b, h, i, d = _where(c, *rc)
        t = int(c.target[b, h, i])
        row = _bits(got[rc[0], h * c.Dr:(h + 1) * c.Dr])
        hit = (_bits(c.v).view(c.B * c.S * c.KV, c.Dr) == row[None, :]).all(1).nonzero()
        if hit.numel():
            x = int(hit[0])
            b2, j2, g2 = x // (c.S * c.KV), x // c.KV % c.S, x % c.KV
            same = " -- the whole output row equals the V row of key %d (batch %d, KV head %d; expected key %d, batch %d, KV head %d)" % (j2, b2, g2, t, b, h // rep)
        else:
            same = " -- the output row equals no key's V row"
        return (f"(b {b}, h {h}, i {i}, d {d}): got {float(got[rc[0], rc[1]]):.6g}, expected {float(c.expect[rc[0], rc[1]]):.6g}; target key {t}, query block {i // 128}, "
                f"wave {i % 128 // 32}, key tile {t // 64}{same}")

    rows = bad[:, 0].unique().numel()
    return f"{what}: {bad.shape[0]} of {got.numel()} elements wrong in {rows} rows; first {describe(bad[0].tolist())}; last {describe(bad[-1].tolist())}"


# ---- bounded family ------------------------------------------------------------------------------------------------------------------------------------------------
def bounded_case(B, S, H, KV, Dr, causal, kind, seed, device="cpu"):
    """dense data, scale = Dr^-0.5:
      late_heavy   scores grow by ~1 natural unit per key (k_0 = j // 16, k_1 = j % 16, q_0 = 16 sqrt(Dr), q_1 = sqrt(Dr)) plus std-1 noise: a causal row's mass sits on its diagonal and
                   the two or three keys before it, a non-causal row's on the last real keys of the tail tile -- a leaked key i + 1 or an unmasked pad key takes > half the mass
      early_heavy  k_0 = +1 in the first tile, -1 after it, q_0 = 12 sqrt(Dr): the first tile holds every row's maximum, later tiles sit 24 units below the reference
      spike        one row r_w per 32-row wave has q = 30 k[j_w] / sqrt(Dr) (score ~30 on that key, the others stay ~N(0, 30^2 / Dr)): the wave-uniform rescale fires for
                   31 rows that did not ask for it; causal: j_w = r_w (the diagonal, the row's last tile), non-causal: a key of the later tiles
      scaled_rows  q rows scaled by 2^-6 ... 2^6, V columns by 2^-6 ... 2^6
      plain        std-1 data, as tests/test_gpu_ops.py::test_attention"""
    assert kind in KINDS and H % KV == 0
    c = Case(B, S, H, KV, Dr, Dr ** -0.5, causal, kind)
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    rnd = lambda *s: torch.randn(s, device=device, generator=g)
    q, k, v = rnd(B, S, H, Dr), rnd(B, S, KV, Dr), rnd(B, S, KV, Dr)
    j = torch.arange(S, device=device)
    rep = H // KV
    if kind == "late_heavy":
        k[..., 0] = (j // 16).float()[None, :, None]
        k[..., 1] = (j % 16).float()[None, :, None]
        q[..., 0], q[..., 1] = 16.0 * Dr ** 0.5, Dr ** 0.5
    elif kind == "early_heavy":
        k[..., 0] = torch.where(j < 64, 1.0, -1.0)[None, :, None]
        q[..., 0] = 12.0 * Dr ** 0.5
    elif kind == "spike":
        for w in range((S + 31) // 32):
            r = min(S - 1, 32 * w + (7 * w + 5 + seed) % 32)
            jw = r if causal else (S - 1 - 5 * w) % S
            q[:, r] = k[:, jw].repeat_interleave(rep, dim=1) * (30.0 / Dr ** 0.5)
    elif kind == "scaled_rows":
        q = q * torch.exp2(torch.rand((B, S, 1, 1), device=device, generator=g) * 12 - 6)
        v = v * torch.exp2(torch.rand((1, 1, KV, Dr), device=device, generator=g) * 12 - 6)
    return _fuse(c, q.to(bf), k.to(bf), v.to(bf))


def elementwise_bound(c, chunk=256):
    """-> (ref, bound, Abs), float64 [B*S, H*Dr]: the float64 softmax attention of case c on its bf16 operands, a per-element bound on |kernel output - ref| that any
    implementation with the documented arithmetic meets, and Abs = p @ |v|.  Computed in chunks of <= `chunk` query rows: nothing of size S^2 H is held.

    Derivation (no fitted factor; U32 = 2^-24, b = 2^-8 = the largest relative error of one round-to-nearest to bf16).  Row i of head h, visible keys j, scores s_j =
    q . k_j (raw), p = softmax(scale s), T = key tiles the row walks through (causal: i // 64 + 1, else ceil(S / 64)), n = visible keys + T.
      exponent   the kernel forms p~_j = exp2(fmaf(s~_j, sc, -fl(m sc))) against a reference m that is some earlier maximum of the row, and carries earlier tiles along with
                 alpha = exp2((m_old - m_new) sc) at each move of m (at most once per tile).  In log2 units, relative to the row's final reference:
                   fp32 accumulation of the score   sc Dr U32 sum_d |q_d k_jd|                                  (running-sum bound, any order)
                   the fmaf's one rounding          U32 |s_j sc - m sc| <= 2 U32 M sc,  M = max_j |s_j| + the accumulation term  (every m is one of the row's own maxima)
                   sc = fl(scale fl(log2 e))        2 U32 M sc
                   each move of the reference       fl(m_new sc) - fl(m_old sc) against fl((m_old - m_new) sc): 4 U32 M sc, T - 1 moves that matter (the first acts on O = 0)
                 times ln 2 (sc ln 2 = scale) it is a RELATIVE error of p~_j;  v_exp_f32 is good to 1 ulp = 2 U32, once for p and once per alpha:
                   delta_j = scale (Dr U32 sum_d |q_d k_jd| + 4 T U32 M) + 2 T U32
      P . V      each p~_j is rounded to bf16 for the MFMA (relative b), the products are exact in fp32 and are summed, with the T rescales, in fp32:
                   numerator / L = o + nu,  |nu| <= sum_j p_j (delta_j + b + delta_j b) |v_jd| + n U32 (1 + b) sum_j p_j (1 + delta_j) |v_jd|
      row sum    over the UNROUNDED p~_j (the non-ONES path, the only one gvl_op_attention reaches): l / L = (1 + zeta)(1 + gamma), |zeta| <= sum_j p_j delta_j, |gamma| <= n U32
      quotient   |num / l - o| <= (|nu| + |o| (|zeta| + |gamma| + |zeta gamma|)) / ((1 - |zeta|)(1 - |gamma|)) = e1
      epilogue   one fp32 reciprocal (1 ulp = 2 U32) and one fp32 product (U32): e2 = e1 + 3 U32 (|o| + e1)
      store      round to nearest bf16: half a bf16 ulp at magnitude |o| + e2 (<= b (|o| + e2))
      flush      a p~_j below 2^-126 is flushed: <= S 2^-126 max_j |v_jd| against l >= 1 -- S <= 2^14: 2^-112 max_j |v_jd|
    With delta -> 0 this is b Abs + b |o| <= 2 . 2^-8 Abs, the leading term."""
    B, S, H, KV, Dr = c.B, c.S, c.H, c.KV, c.Dr
    dev = c.qkv.device
    q, k, v = (t.permute(0, 2, 1, 3).double() for t in c.split())                   # [B, heads, S, Dr]
    rep = H // KV
    k, v = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
    kT, kaT, va = k.transpose(-1, -2), k.abs().transpose(-1, -2), v.abs()
    vmax = va.amax(2, keepdim=True)                                                  # [B, H, 1, Dr]
    b8 = 2.0 ** -8
    keys = torch.arange(S, device=dev)
    ref, bound, Abs = (torch.empty((B, H, S, Dr), dtype=torch.float64, device=dev) for _ in range(3))
    for r0 in range(0, S, chunk):
        rows = torch.arange(r0, min(S, r0 + chunk), device=dev)
        qc = q[:, :, r0:r0 + chunk]
        s = qc @ kT                                                                  # [B, H, R, S]
        es = Dr * U32 * (qc.abs() @ kaT)
        if c.causal:
            vis = keys[None, :] <= rows[:, None]
            T = (rows // 64 + 1).double()
        else:
            vis = torch.ones((rows.numel(), S), dtype=torch.bool, device=dev)
            T = torch.full((rows.numel(),), float((S + 63) // 64), dtype=torch.float64, device=dev)
        T = T[None, None, :, None]
        n = vis.sum(-1).double()[None, None, :, None] + T
        M = torch.where(vis, s.abs() + es, torch.zeros_like(s)).amax(-1, keepdim=True)
        delta = c.scale * (es + 4 * T * U32 * M) + 2 * T * U32
        p = torch.softmax(torch.where(vis, s * c.scale, torch.full_like(s, float("-inf"))), -1)
        o, A = p @ v, p @ va
        Ad = (p * delta) @ va
        zeta = (p * delta).sum(-1, keepdim=True)
        gamma = n * U32
        nu = Ad * (1 + b8) + b8 * A + gamma * (1 + b8) * (A + Ad)
        e1 = (nu + o.abs() * (zeta + gamma + zeta * gamma)) / ((1 - zeta) * (1 - gamma))
        e2 = e1 + 3 * U32 * (o.abs() + e1)
        ref[:, :, r0:r0 + chunk], Abs[:, :, r0:r0 + chunk] = o, A
        bound[:, :, r0:r0 + chunk] = e2 + 0.5 * bf16_ulp(o.abs() + e2) + 2.0 ** -112 * vmax
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(B * S, H * Dr)
    return flat(ref), flat(bound), flat(Abs)


def old_stat(got, ref):
    """gpu_util.check()'s statistic (restated: gpu_util imports the GPU package)"""
    return float((got.double() - ref).abs().max() / ref.abs().max())


def row_stat(got, ref, Abs, Dr):
    """max_d |err| / max_d Abs per (row, head), maximum over them: the statistic that does not let the first rows set the scale for the long ones"""
    err = (got.double() - ref).abs().view(ref.shape[0], -1, Dr).amax(-1)
    return float((err / Abs.view(ref.shape[0], -1, Dr).amax(-1)).max())


def bound_violations(got, ref, bound, c, what=""):
    """-> (message or None, largest |got - ref| / bound): zero elements may lie outside the per-element bound; the message names the count, the worst ratio and the first
    and last offending (b, h, i, d) with query block, wave and -- causal -- the diagonal's key tile"""
    what = what or str(c)
    g = got.double()
    if g.shape != ref.shape:
        return f"{what}: shape {tuple(g.shape)}, expected {tuple(ref.shape)}", float("inf")
    err = (g - ref).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = (err > bound).nonzero()
    if bad.numel() == 0:
        return None, worst

    def d(rc):
        b, h, i, dd = _where(c, *rc)
        return (f"(b {b}, h {h}, i {i}, d {dd}): got {float(g[rc[0], rc[1]]):.6g}, reference {float(ref[rc[0], rc[1]]):.6g}, bound {float(bound[rc[0], rc[1]]):.3g}; query block "
                f"{i // 128}, wave {i % 128 // 32}" + (f", diagonal key {i} in key tile {i // 64}" if c.causal else f", last key {c.S - 1} in key tile {(c.S - 1) // 64}"))

    return f"{what}: {bad.shape[0]} of {g.numel()} elements outside the bound (worst err / bound {worst:.3g}); first {d(bad[0].tolist())}; last {d(bad[-1].tolist())}", worst


# ---- the kernel's arithmetic in plain torch ------------------------------------------------------------------------------------------------------------------------
def emulate(c, mut=None, mut_rows=None, guard=0):
    """attn_fwd_kernel's documented arithmetic: 64-key tiles, fp32 scores from the bf16 operands, -1e30 masking, the lazy reference point (it moves, for all 32 rows of a
    wave, to each row's own running maximum only when SOME row of the wave sees a tile maximum more than 8 log2 units above its reference), p = exp2(fmaf(s, sc, -m sc)),
    P rounded to bf16 for the product, l from the unrounded p, one fp32 reciprocal, bf16 store.  -> bf16 [B*S + guard, H*Dr], the guard rows filled with SENT.
    (Rows >= S of the last wave load query S - 1 and see the same keys: their vote is row S - 1's, so they are left out.  A causal tile that a wave skips is a tile whose
    keys are all masked for it: p = 0, no vote -- the same.)

    mut: one of MUTATIONS -- a WRONG kernel (test_attn_ref_cpu.py):
      mask_plus / mask_minus   causal: key i + 1 is visible / key i is hidden
      drop_diag                causal: the diagonal key is hidden for the rows mut_rows (default: the last row of every 128-row query block)
      pad_dup, pad_dup_vzero   the pad keys of the tail tile are not masked and their K rows duplicate key S - 1 (the in-place forms' re-read); V pad: the duplicate / zeros
      swap_pv                  keys 3 and 5 of every 16-key group are swapped in the P.V product but not in the scores
      gqa_mod                  query head h reads KV head h % KV
      no_rescale_O             when the reference moves alpha is applied to l but not to O
      skip_last8               the last 8 columns of every head stay unwritten
      rows_shift               the rows >= S of the last query block are written: row S (the next batch's row 0, or the first row behind the output) takes query S - 1's result"""
    assert mut is None or mut in MUTATIONS
    B, S, H, KV, Dr = c.B, c.S, c.H, c.KV, c.Dr
    dev = c.qkv.device
    q, k, v = (t.permute(0, 2, 1, 3).float() for t in c.split())
    rep = H // KV
    hk = torch.arange(H, device=dev) % KV if mut == "gqa_mod" else torch.arange(H, device=dev) // rep
    k, v = k[:, hk], v[:, hk]                                                       # [B, H, S, Dr]
    nt = (S + 63) // 64
    pad = nt * 64 - S
    unmask_pad = mut in ("pad_dup", "pad_dup_vzero")
    if pad:
        kp = k[:, :, S - 1:S].expand(B, H, pad, Dr) if unmask_pad else torch.zeros((B, H, pad, Dr), device=dev)
        vp = v[:, :, S - 1:S].expand(B, H, pad, Dr) if mut == "pad_dup" else torch.zeros((B, H, pad, Dr), device=dev)
        k, v = torch.cat([k, kp], 2), torch.cat([v, vp], 2)
    G = (S + 31) // 32
    qi = torch.arange(S, device=dev)
    sc = np.float32(c.scale) * LOG2E
    sc32, sc64 = torch.tensor(sc, dtype=torch.float32, device=dev), float(sc)
    m_run = torch.full((B, H, S), -1e30, dtype=torch.float32, device=dev)
    l_run = torch.zeros((B, H, S), dtype=torch.float32, device=dev)
    O = torch.zeros((B, H, S, Dr), dtype=torch.float32, device=dev)
    if mut == "drop_diag" and mut_rows is None:
        mut_rows = qi[qi % 128 == 127]
    for t in range(nt):
        if c.causal and t * 64 > S - 1 + (1 if mut == "mask_plus" else 0):
            break
        keys = torch.arange(t * 64, t * 64 + 64, device=dev)
        s = q @ k[:, :, t * 64:t * 64 + 64].transpose(-1, -2)                       # [B, H, S, 64]
        dead = (keys >= S)[None, :].expand(S, 64)
        if unmask_pad:
            dead = torch.zeros_like(dead)
        if c.causal:
            lim = qi + 1 if mut == "mask_plus" else qi - 1 if mut == "mask_minus" else qi
            dead = dead | (keys[None, :] > lim[:, None])
            if mut == "drop_diag":
                sel = torch.zeros(S, dtype=torch.bool, device=dev)
                sel[mut_rows] = True
                dead = dead | ((keys[None, :] == qi[:, None]) & sel[:, None])
        s = torch.where(dead, torch.full_like(s, -1e30), s)
        mx = s.amax(-1)
        vote = (mx - m_run) * sc32 > LAZY
        vote = torch.cat([vote, torch.zeros((B, H, G * 32 - S), dtype=torch.bool, device=dev)], -1).view(B, H, G, 32).any(-1)
        vote = vote.repeat_interleave(32, dim=-1)[..., :S]
        m_new = torch.where(vote, torch.maximum(m_run, mx), m_run)
        alpha = torch.exp2(((m_run - m_new) * sc32).double()).float()
        m_run = m_new
        if mut != "no_rescale_O":
            O = O * alpha[..., None]
        nm = -m_run * sc32
        p = torch.exp2(s.double() * sc64 + nm.double()[..., None]).float()          # fmaf: the float64 product of two fp32 numbers is exact
        l_run = l_run * alpha + p.sum(-1)
        vt = v[:, :, t * 64:t * 64 + 64]
        if mut == "swap_pv":
            perm = torch.arange(64, device=dev)
            for g0 in range(0, 64, 16):
                if t * 64 + g0 + 5 < S:
                    perm[g0 + 3], perm[g0 + 5] = g0 + 5, g0 + 3
            vt = vt[:, :, perm]
        O = O + p.to(bf).float() @ vt
    out = (O * (1.0 / l_run)[..., None]).to(bf)
    if mut == "skip_last8":
        out[..., Dr - 8:] = SENT
    out = out.permute(0, 2, 1, 3).reshape(B * S, H * Dr)
    out = torch.cat([out, torch.full((guard, H * Dr), SENT, dtype=bf, device=dev)])
    if mut == "rows_shift":
        assert guard >= 1
        for b in range(B):
            out[b * S + S] = out[b * S + S - 1]
    return out
