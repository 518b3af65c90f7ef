"""Independent references for the bf16 MFMA GEMM family (gvl_gemm.hip, gvl_gemm4.hip, gvl_gemm4p.hip) -- no GPU needed to import or run this file.

Why: the bit-identity tests compare the kernels with each other (they share gvl_gemm_epi.h and the k order: a common error passes), and gpu_util.check() is
max|got - ref| / max|ref| over the whole matrix against fp32 torch: blind to one wrong tile at the tolerance and to any row whose scale is far below the largest.
Two families of cases replace it:

exact_case(M, N, K, epi, seed)   operands on which EVERY number the kernel forms is exactly representable, so the expected output comes from integer arithmetic
  and must be reproduced BIT FOR BIT.
    A   8 entries of +-1 per row (scatter-added: a collision gives 0 / +-2), one at the LAST k, seven at chunk (7 m + j + seed) mod K / 8, a hashed element of the chunk: every
        8-element chunk of every k-tile is hit within any K / 56 + 1 consecutive rows (test_gemm_ref_cpu.py asserts it per 128-row block)
    W   integers in [-6, 6], hashed asymmetrically from (n, k)  ->  any partial sum, in any order, is an integer of magnitude <= 48: exact in fp32
    bias      integers in [-16, 16]                   acc + bias: integer, <= 64 -- exact in bf16 (8 significant bits: every integer up to 256, every half-integer
    gamma     +-{0.5, 1, 2}                            up to 128, every quarter up to 64)
    resid     integers in [-60, 60]                   bf16(v) gamma: <= 128, a half-integer only when <= 32; + resid: integer <= 188 or half-integer <= 92 -- exact
    rowscale  {0.25, 0.5, 1, 2, 4}                    acc * rs: an integer <= 48 times a power of two -- exact
    rowsq     64 squares of multiples of 1/2 below 256: a sum of quarter units below 2^24 -- exact in fp32 in any order
  fp32 accumulation, every bf16 rounding the kernels document (gvl_gemm_epi.h) and the bf16 / f32 store are therefore the identity on these values.

bounded_case(M, N, K, epi, seed) + elementwise_bound(case)   dense random data check() is blind to (row scales 2^-6 ... 2^6, a few outlier columns of A ~100 x the rest,
  K^-0.5 weights), a float64 reference with the roundings where gvl_gemm_epi.h and test_gemm_epilogues place them, and a PER-ELEMENT tolerance that is derived, not
  measured -- see elementwise_bound.
"""
import math

import torch

bf = torch.bfloat16
ACT_NONE, ACT_QUICK_GELU, ACT_GELU, ACT_SILU_MUL = 0, 1, 2, 3      # gvl.h
U32 = 2.0 ** -24                                                     # unit roundoff of fp32

# name -> operands of the epilogue (what the case carries) -- the exact family: every epilogue whose arithmetic is exact on integer data
EXACT_EPIS = {
    "plain": (), "bias": ("bias",), "resid": ("resid",), "bias_resid_f32": ("bias", "resid", "f32"), "bias_gamma_resid": ("bias", "gamma", "resid"),
    "rowscale": ("rowscale",), "rowsq": ("rowsq",), "rowsq_resid": ("rowsq", "resid"), "rowsq_bias_gamma_resid": ("rowsq", "bias", "gamma", "resid"), "f32": ("f32",),
}
# the bounded family: every activation with and without bias and row scale AS FAR AS THE LIBRARY SERVES THE COMBINATION (row scale exists in the staged epilogues 64 / 67 /
# 98 only: alone, with SwiGLU, with bias + erf-GELU -- gvl_launch_gemm returns -1 for the others), and the residual / LayerScale forms
BOUNDED_EPIS = {
    "plain": (), "rowscale": ("rowscale",),
    "qgelu": ("qgelu",), "bias_qgelu": ("bias", "qgelu"),
    "gelu": ("gelu",), "bias_gelu": ("bias", "gelu"), "rowscale_bias_gelu": ("rowscale", "bias", "gelu"),
    "silu": ("silu",), "bias_silu": ("bias", "silu"), "rowscale_silu": ("rowscale", "silu"),
    "resid": ("resid",), "bias_resid": ("bias", "resid"), "gamma": ("gamma",), "bias_gamma_resid": ("bias", "gamma", "resid"), "bias_resid_f32": ("bias", "resid", "f32"),
    "rowsq_bias_gamma_resid": ("rowsq", "bias", "gamma", "resid"),
}
NNZ = 8


class Case:
    """operands + how to call the library: kwargs() for Engine.op_gemm / op_gemm_rows (rows: needs op_gemm_rows)"""

    def __init__(self, M, N, K, epi, flags):
        self.M, self.N, self.K, self.epi, self.flags = M, N, K, epi, flags
        self.A = self.W = self.bias = self.gamma = self.resid = self.rowscale = None
        self.expect = self.expect_rowsq = None
        self.act = ACT_QUICK_GELU if "qgelu" in flags else ACT_GELU if "gelu" in flags else ACT_SILU_MUL if "silu" in flags else ACT_NONE
        self.out_f32 = "f32" in flags
        self.rows = "rowscale" in flags or "rowsq" in flags

    def kwargs(self):
        kw = {k: getattr(self, k) for k in ("bias", "gamma", "resid") if getattr(self, k) is not None}
        if self.act:
            kw["act"] = self.act
        if self.rows:
            if self.rowscale is not None:
                kw["rowscale"] = self.rowscale
            if "rowsq" in self.flags:
                kw["want_rowsq"] = True
        elif self.out_f32:
            kw["out_f32"] = True
        return kw


def _mix(x):
    """a 31-bit integer hash, elementwise on int64 tensors (xorshift-multiply; every intermediate stays below 2^62)"""
    x = (x ^ (x >> 15)) * 0x2C1B3C6D % (1 << 31)
    x = (x ^ (x >> 12)) * 0x297A2D39 % (1 << 31)
    return x ^ (x >> 15)


def exact_A_entries(rows, K, seed):
    """-> (idx [R, 8] int64, sign [R, 8] int64) of the +-1 entries of the given rows (int64 tensor of row numbers)"""
    j = torch.arange(NNZ, device=rows.device, dtype=torch.int64)[None, :]
    m = rows[:, None]
    h = _mix(m * 1315423911 % (1 << 31) + j * 2654435 + seed * 97 + 1)
    chunk = (m * (NNZ - 1) + (j - 1) + seed) % (K // 8)
    idx = chunk * 8 + h % 8
    idx = torch.where(idx == K - 1, idx - 1, idx)                  # the last k belongs to entry 0 alone: nothing can cancel it
    idx = torch.where(j == 0, torch.full_like(idx, K - 1), idx)
    sign = 1 - 2 * ((h >> 9) & 1)
    return idx, sign


def exact_A(rows, K, seed):
    idx, sign = exact_A_entries(rows, K, seed)
    A = torch.zeros((rows.numel(), K), dtype=torch.float32, device=rows.device)
    A.scatter_add_(1, idx, sign.float())
    return A.to(bf)


def exact_W_int(rows, cols, seed):
    """W[n, k] for the given n (rows) and k (cols), int64 in [-6, 6]; asymmetric in (n, k)"""
    n, k = rows[:, None], cols[None, :]
    return _mix(n * 40503 + k * 9973 + (n >> 3) * (k & 63) + seed * 7919) % 13 - 6


def exact_vectors(M_rows, N_cols, seed, flags):
    """the epilogue operands of the given output rows / columns (int64 tensors): dict of float tensors"""
    out = {}
    if "bias" in flags:
        out["bias"] = (_mix(N_cols * 7 + seed + 11) % 33 - 16).float()
    if "gamma" in flags:
        g = _mix(N_cols * 13 + seed + 5)
        out["gamma"] = torch.tensor([0.5, 1.0, 2.0], device=N_cols.device)[g % 3] * (1 - 2 * ((g >> 7) & 1)).float()
    if "rowscale" in flags:
        out["rowscale"] = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0], device=M_rows.device)[_mix(M_rows * 3 + seed + 17) % 5]
    if "resid" in flags:
        out["resid"] = (_mix(M_rows[:, None] * 50021 + N_cols[None, :] * 31 + seed) % 121 - 60).float()
    return out


def exact_expected(rows, cols, K, seed, flags, W_int=None):
    """the expected output block [rows x cols] (float64; exactly representable in the output type) and, with "rowsq", nothing else: the statistics come from
    exact_rowsq on whole 64-column blocks.  No matmul: 8 gathered columns of W per row."""
    idx, sign = exact_A_entries(rows, K, seed)
    acc = torch.zeros((rows.numel(), cols.numel()), dtype=torch.int64, device=rows.device)
    for j in range(NNZ):
        w = exact_W_int(cols, idx[:, j], seed).T if W_int is None else W_int[cols][:, idx[:, j]].T
        acc += sign[:, j:j + 1] * w
    v = acc.double()
    ev = exact_vectors(rows, cols, seed, flags)
    if "rowscale" in flags:
        v = v * ev["rowscale"].double()[:, None]
    if "bias" in flags:
        v = v + ev["bias"].double()[None, :]
    if "gamma" in flags:
        v = v * ev["gamma"].double()[None, :]
    if "resid" in flags:
        v = v + ev["resid"].double()
    assert float(v.abs().max()) <= 256 and bool((v * 4 == (v * 4).round()).all())
    return v


def exact_case(M, N, K, epi, seed, device="cpu"):
    """see the module docstring.  -> Case with A, W (bf16), the epilogue operands, expect (output dtype) and expect_rowsq ([M, N / 64] f32, or None)"""
    flags = EXACT_EPIS[epi]
    assert K % 64 == 0 and N % 4 == 0 and ("rowsq" not in flags or N % 64 == 0)
    c = Case(M, N, K, epi, flags)
    rows, cols, ks = (torch.arange(n, device=device, dtype=torch.int64) for n in (M, N, K))
    c.A = exact_A(rows, K, seed)
    Wi = exact_W_int(cols, ks, seed)
    c.W = Wi.to(bf)
    ev = exact_vectors(rows, cols, seed, flags)
    c.bias, c.gamma, c.rowscale = ev.get("bias"), ev.get("gamma"), ev.get("rowscale")
    if "resid" in flags:
        c.resid = ev["resid"] if c.out_f32 else ev["resid"].to(bf)
    R = 8192
    exp = torch.cat([exact_expected(rows[r:r + R], cols, K, seed, flags, W_int=Wi) for r in range(0, M, R)])
    c.expect = exp.float() if c.out_f32 else exp.to(bf)
    assert bool((c.expect.double() == exp).all()), "the expected values are not representable in the output type"
    if "rowsq" in flags:
        c.expect_rowsq = exp.pow(2).view(M, N // 64, 64).sum(-1).float()
    return c


def tile_of(r, c):
    return f"256 x 256 tile (row {r // 256}, column {c // 256}), element ({r % 256}, {c % 256}) of it"


def exact_mismatch(got, want, what, row0=0, col0=0):
    """None when got == want bit for bit (shape, dtype and every element; NaN never equals), else the message the tests fail with: the number of wrong elements, the
    first and the last one, and the 256 x 256 tile each falls in."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{what}: shape / dtype {tuple(got.shape)} {got.dtype}, expected {tuple(want.shape)} {want.dtype}"
    bad = (got != want).nonzero()
    if bad.numel() == 0:
        return None
    (r0, c0), (r1, c1) = bad[0].tolist(), bad[-1].tolist()
    g = lambda r, c: f"({r + row0}, {c + col0}): got {float(got[r, c])}, expected {float(want[r, c])}, {tile_of(r + row0, c + col0)}"
    return f"{what}: {bad.shape[0]} of {got.numel()} elements wrong; first {g(r0, c0)}; last {g(r1, c1)}"


# ---- bounded family ------------------------------------------------------------------------------------------------------------------------------------------------
def bounded_case(M, N, K, epi, seed, device="cpu"):
    flags = BOUNDED_EPIS[epi]
    c = Case(M, N, K, epi, flags)
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    rnd = lambda *s: torch.randn(s, device=device, generator=g)
    scale = torch.exp2(torch.rand((M, 1), device=device, generator=g) * 12 - 6)          # row scales 2^-6 ... 2^6
    A = rnd(M, K)
    out_cols = torch.randperm(K, device=device, generator=g)[:max(1, K // 128)]
    A[:, out_cols] *= 100.0                                                              # a few outlier columns ~100 x the rest
    c.A = (A * scale).to(bf)
    c.W = (rnd(N, K) * K ** -0.5).to(bf)
    n_out = N // 2 if "silu" in flags else N
    if "bias" in flags:
        c.bias = rnd(N) * 0.5
    if "gamma" in flags:
        c.gamma = rnd(N) * 0.05 + 0.1
    if "rowscale" in flags:
        c.rowscale = torch.rand((M,), device=device, generator=g) + 0.5
    if "resid" in flags:
        r = rnd(M, n_out) * 2.0 * scale
        c.resid = r if c.out_f32 else r.to(bf)
    return c


def bf16_ulp(x):
    """spacing of bf16 at magnitude |x| (8 significant bits): 2^(floor(log2 |x|) - 7); the smallest normal's below it"""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))               # |x| = m 2^e, m in [0.5, 1)
    return torch.exp2((e - 8).double())


def _rbf(x):
    """float64 -> nearest bf16 (RNE), as float64.  Through fp32: exact for every bf16-representable target unless x sits within 2^-24 relative of a bf16 tie -- on such
    an element the double rounding can pick the other neighbour, which the ulp term of the bound covers"""
    return x.float().to(bf).double()


class _V:
    """a float64 intermediate x of the reference and a bound e >= |the kernel's value - x|"""

    def __init__(self, x, e):
        self.x, self.e = x, e

    def f32(self, n=1):             # n fp32 roundings of a value within e of x: each <= U32 (|x| + e)
        return _V(self.x, self.e + n * U32 * (self.x.abs() + self.e))

    def round_bf16(self):           # |rbf(xk) - rbf(x)| <= |rbf(xk) - xk| + |xk - x| + |x - rbf(x)| <= e + one bf16 ulp at magnitude |x| + e
        return _V(_rbf(self.x), self.e + bf16_ulp(self.x.abs() + self.e))

    def scale(self, s):             # exact factor s known to both sides, one fp32 rounding of the product
        return _V(self.x * s, self.e * s.abs()).f32()

    def add(self, o):               # o: exact operand, one fp32 rounding
        return _V(self.x + o, self.e).f32()


def _sigmoid(v):
    """fast_sigmoid (gvl_internal.h): rcp(1 + exp(-x)) with the hardware's 1-ulp exp2 / rcp.  Relative error of the result, counted: the product x log2(e) rounded to fp32
    moves the exponent by |x| log2(e) U32, i.e. the power by a relative |x| U32; exp2 1 ulp (2 U32); the sum (U32); rcp 1 ulp (2 U32)  ->  (|x| + 5) U32, plus 2^-126
    absolute for a flushed denormal.  Lipschitz constant of the sigmoid: 1 / 4."""
    s = torch.sigmoid(v.x)
    return _V(s, 0.25 * v.e + s * (v.x.abs() + v.e + 5) * U32 + 2.0 ** -126)


def _mul(a, b):                     # product of two uncertain values, one fp32 rounding
    return _V(a.x * b.x, a.x.abs() * b.e + b.x.abs() * a.e + a.e * b.e).f32()


GELU_LIP = 1.13                     # max |d/dx x Phi(x)| = 1.1290 (at x = sqrt 2)
SILU_LIP = 1.10                     # max |d/dx x sigmoid(x)| = 1.0998 (at x = 2.3994)


def elementwise_bound(c):
    """-> (ref, bound, rowsq_ref, rowsq_bound): the float64 reference of case c and, per element, a bound on |kernel output - ref| that any implementation with the documented
    arithmetic meets.  Derivation (no fitted factor; U32 = 2^-24):
      accumulator   the kernel sums K exact products in fp32 in SOME order: |acc32 - acc| <= K U32 sum_k |a_k w_k|  (standard running-sum bound, gamma_K ~ K U32)
      fp32 step     every fp32 operation on a value within e of x adds U32 (|x| + e)                       (row scale, bias, LayerScale, residual, products)
      bf16 point    where gvl_gemm_epi.h rounds to bf16 -- acc (* rs) (+ bias); 1.702 x and the sigmoid of quick-GELU; g sigmoid(g) of SwiGLU; the LayerScale
                    product; the value added to the residual; the stored output -- the reference rounds its float64 intermediate too, and the two rounded values differ
                    by at most e + ONE bf16 ulp at magnitude |x| + e
      Lipschitz     an error e entering a function leaves multiplied by its largest slope: x Phi(x) 1.13, x sigmoid(x) 1.10, sigmoid 1 / 4, a product a b by
                    |a| e_b + |b| e_a + e_a e_b, a known factor by its magnitude
      erf-GELU      Phi comes from an fp32 table at bf16 points (gvl_gemm_epi.h): one fp32 rounding of Phi and one of the product (2 U32 |y|); below 2^-12 the table
                    clamps (Phi off by <= 2e-4 relative: |x| 2e-4), above 5.5 it returns Phi(5.5) = 1 - 1.9e-8 resp. exactly 0 (|x| 1.9e-8, resp. |x Phi(x)| <= 1.1e-7)
      sigmoid       see _sigmoid
      row statistics  the sum of squares of the 64 STORED outputs y: |y_k^2 - y^2| <= e (2 |y| + e) per term, plus 64 U32 sum y_k^2 for the fp32 summation
    """
    flags = c.flags
    A, W = c.A.double(), c.W.double()
    acc = A @ W.T
    v = _V(acc, c.K * U32 * (A.abs() @ W.abs().T))
    if c.rowscale is not None:
        v = v.scale(c.rowscale.double()[:, None])
    if c.bias is not None:
        v = v.add(c.bias.double()[None, :])
    if c.out_f32 and c.resid is None and c.gamma is None and not c.act:
        return v.x, v.e, None, None                                   # f32 store of the fp32 value
    v = v.round_bf16()
    if "qgelu" in flags:
        t = v.scale(torch.tensor(1.702, dtype=torch.float64, device=acc.device)).round_bf16()
        v = _mul(v, _sigmoid(t).round_bf16())
    elif "gelu" in flags:
        x = v.x
        y = x * 0.5 * torch.erfc(-x * math.sqrt(0.5))
        tab = 2 * U32 * y.abs() + torch.where(x.abs() < 2.0 ** -12, x.abs() * 2e-4, torch.zeros_like(x)) + \
            torch.where(x.abs() > 5.5, torch.maximum(x.abs() * 1.9e-8, torch.full_like(x, 1.1e-7)), torch.zeros_like(x))
        v = _V(y, GELU_LIP * v.e + tab)
    elif "silu" in flags:
        g, u = _V(v.x[:, 0::2], v.e[:, 0::2]), _V(v.x[:, 1::2], v.e[:, 1::2])
        s = _sigmoid(g)
        t = _V(g.x * s.x, SILU_LIP * g.e + g.x.abs() * (s.e - 0.25 * g.e)).f32().round_bf16()      # slope of x sigmoid(x) on g's error + the sigmoid's own error times |g|
        v = _mul(u, t)
    if c.gamma is not None:
        v = v.scale(c.gamma.double()[None, :])
    if c.resid is not None:
        if c.gamma is not None or c.act:
            v = v.round_bf16()                                        # round_pre_resid = 1 (gvl_op_gemm): what is added to the residual stream is a bf16 value
        v = v.add(c.resid.double())
    if not c.out_f32:
        v = v.round_bf16()
    if "rowsq" in flags:
        y2 = v.x.pow(2).view(c.M, c.N // 64, 64).sum(-1)
        e2 = (v.e * (2 * v.x.abs() + v.e)).view(c.M, c.N // 64, 64).sum(-1)
        return v.x, v.e, y2, e2 + 64 * U32 * (y2 + e2)
    return v.x, v.e, None, None


def bound_violations(got, ref, bound, what):
    """-> (message or None, largest |got - ref| / bound): zero elements may lie outside the per-element bound; the message names the count, the worst element and the
    first and last offending (row, column) with their tiles"""
    g = got.double()
    if g.shape != ref.shape:
        return f"{what}: shape {tuple(g.shape)}, expected {tuple(ref.shape)}", float("inf")
    err = (g - ref).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    ratio = err / bound
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = (err > bound).nonzero()
    if bad.numel() == 0:
        return None, worst
    d = lambda rc: f"({rc[0]}, {rc[1]}): got {float(g[rc[0], rc[1]]):.6g}, reference {float(ref[rc[0], rc[1]]):.6g}, bound {float(bound[rc[0], rc[1]]):.3g}, {tile_of(rc[0], rc[1])}"
    return f"{what}: {bad.shape[0]} of {g.numel()} elements outside the bound (worst err / bound {worst:.3g}); first {d(bad[0].tolist())}; last {d(bad[-1].tolist())}", worst


def emulate(c):
    """what the kernels document, in plain torch: bf16 operands, an fp32 matmul, fp32 epilogue arithmetic with the bf16 rounding points of gvl_gemm_epi.h.
    -> (output in the output dtype, rowsq or None).  The CPU stand-in for a correct kernel: it must pass both families of checks."""
    rb = lambda t: t.to(bf).float()
    v = c.A.float() @ c.W.float().T
    if c.rowscale is not None:
        v = v * c.rowscale[:, None]
    if c.bias is not None:
        v = v + c.bias[None, :]
    if c.act == ACT_QUICK_GELU:
        x = rb(v)
        v = x * rb(torch.sigmoid(rb(1.702 * x)))
    elif c.act == ACT_GELU:
        v = torch.nn.functional.gelu(rb(v))
    elif c.act == ACT_SILU_MUL:
        x = rb(v)
        g, u = x[:, 0::2], x[:, 1::2]
        v = u * rb(g * torch.sigmoid(g))
    if c.gamma is not None:
        v = rb(v) * c.gamma[None, :]
    if c.resid is not None:
        v = c.resid.float() + rb(v)
    out = v if c.out_f32 else v.to(bf)
    sq = out.float().pow(2).view(c.M, c.N // 64, 64).sum(-1) if "rowsq" in c.flags else None
    return out, sq
