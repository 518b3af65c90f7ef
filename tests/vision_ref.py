"""Independent references for the vision front end and the glue of the visual prefix (gvl_patch.hip, the vision half of gvl_elem.hip, the row-remapping GEMM store of
gvl_gemm_epi.h) -- no GPU needed to import or run this file.

Why: these kernels are reached only through clip_encode / iv2_encode / encode_segments, whose outputs are compared after two or more transformer layers, on strided
samples, at 6e-3 ... 1.8e-2 of the output's max-abs: a one-row or one-column mistake passes.  Here every kernel gets a plain float64 reference of the SAME operation,
whose index arithmetic comes from the model's definition (a convolution of stride = kernel over [c][py][px]; cat(cls, patches) + pos; the reshape / permute forms of
the glue) and never from the kernels, and two families of cases, as tests/gemm_ref.py has them:

exact     patch_case(..., kind="exact"): pixels are sparse +-1 (eight per patch, at positions that differ from patch to patch and sweep every (c, py, px)), weights
          integers in [-6, 6] hashed asymmetrically from (column, k), bias integers in [-16, 16], cls and pos integers in [-40, 40] that differ from row to row.
          Every partial sum of the convolution, in any order, is an integer of magnitude <= 48, the sum with the bias <= 64 and with pos <= 104: all exact in fp32
          AND in bf16 (8 significant bits: every integer up to 256).  InternVideo2's output must then equal the
          reference BIT FOR BIT; CLIP's pre-LayerNorm rows are exact and only the fp32 LayerNorm carries error (layernorm_bound with e = 0).  A wrong row, column,
          frame, image or pixel changes the integer.
bounded   seeded gaussian data, the float64 reference with the documented rounding points and a PER-ELEMENT bound that is derived, not measured (patch_reference,
          layernorm_bound, rmsnorm_bound, pool_*_ref).  Zero elements may lie outside it.

The glue kernels patchify, iv2_embed, hd_merge, strip_cls and bcast_row are gathers with at most one round-to-nearest-even to bf16: bit-exact.  The pools sum 9 / 16
terms in fp32: a float64 mean with a derived bound, plus integer cases that are exact in any order.

emulate_*: the documented arithmetic in fp32 / bf16 torch -- the CPU stand-in for a correct kernel.  tests/test_vision_ref_cpu.py proves that it stays inside every bound
on every input the GPU tests use, and that each of its deliberate mutations (MUTATIONS) is caught.
"""
import torch
import torch.nn.functional as F

from gemm_ref import U32, _V, _mix, _rbf, bf, bf16_ulp, bound_violations, exact_W_int, exact_mismatch  # noqa: F401  (re-exported for the tests)

PATCH, KREAL, KP = 14, 588, 640
PE_BM = 48                                                           # patch rows per block of the fused kernel: only the SHAPES below are chosen by it
SENT = -7776.0                                                       # sentinel: representable in bf16 (243 * 32) and f32, outside every test's value range
PAD_ROWS = 64                                                        # sentinel rows before and after an output: more than one 48-row tile
# (image, T, n): the smallest shapes at which each path of the fused kernel can still go wrong
CLIP_SHAPES = [(14, 1, 1),       # M = 1: one real row in a tail tile
               (14, 1, 9),       # two CLS blocks, the second with one live wave
               (42, 1, 11),      # M = 99 = 2 * 48 + 3: tiles straddle images, a tail of 3 rows
               (98, 1, 2)]       # L = 49: the second tile starts at row 48 of image 0
IV2_SHAPES = [(28, 3, 5),        # M = 60: straddles frames and segments, a tail of 12
              (56, 2, 3),        # M = 96: whole tiles only
              (14, 1, 1)]
IV2_DIMS = (1408, 1024)
CLIP_DIM = 1024
GROUPINGS = [(156, 181, 0), (16, 181, 156), (64, 97, 0), (1, 3, 2)]  # (grp_rows, grp_stride, row_off)
LN_COLS, RMS_COLS, NORM_ROWS = (4, 1024, 1028, 4096), (8, 2048, 2056, 8192), (1, 5)
MUTATIONS = ("drop_px13", "pos_off1", "frame_prev", "dup_tail", "cls_pos1", "sub_gn_col0", "dydx_swap", "window_shift", "one_pass_var", "stride_is_rows")


# ---- sentinel-guarded outputs ---------------------------------------------------------------------------------------------------------------------------------------
def guarded(rows, cols, dtype, device="cpu", pad=PAD_ROWS):
    """-> (buf [pad + rows + pad, cols] filled with SENT, the [rows, cols] view in its middle)"""
    buf = torch.full((pad + rows + pad, cols), SENT, dtype=dtype, device=device)
    return buf, buf[pad:pad + rows]


def guard_damage(buf, rows, pad=PAD_ROWS):
    """number of elements before and after the output that no longer hold the sentinel"""
    return int((buf[:pad] != SENT).sum()) + int((buf[pad + rows:] != SENT).sum())


# ---- patch embedding ------------------------------------------------------------------------------------------------------------------------------------------------
class PatchCase:
    """operands of one gvl_op_patch_embed call: mode 0 CLIP (cls, pos f32; lnw, lnb) / 1 InternVideo2 (cls, pos bf16; bias)"""

    def __init__(self, mode, image, T, n, C, kind):
        self.mode, self.image, self.T, self.n, self.C, self.kind, self.patch, self.Kp, self.eps = mode, image, T, n, C, kind, PATCH, KP, 1e-5
        self.g = image // PATCH
        self.L = self.g * self.g
        self.TL = T * self.L
        self.S = 1 + self.TL
        self.M = n * self.TL
        self.px = self.W = self.bias = self.cls = self.pos = self.lnw = self.lnb = None
        self._ref = None

    def out_dtype(self):
        return torch.float32 if self.mode == 0 else bf

    def name(self):
        return f"{'clip' if self.mode == 0 else 'iv2'} C{self.C} image{self.image} T{self.T} n{self.n} {self.kind}"

    def to(self, device):
        for k in ("px", "W", "bias", "cls", "pos", "lnw", "lnb"):
            if getattr(self, k) is not None:
                setattr(self, k, getattr(self, k).to(device))
        return self


def patch_case(mode, image, T, n, C, kind, seed=0, device="cpu"):
    """device: where an EXACT case is built (hashes of index tensors: the same values anywhere) -- for the one case that is large enough to wrap a grid"""
    assert kind == "exact" or device == "cpu"
    c = PatchCase(mode, image, T, n, C, kind)
    S, p = c.S, PATCH
    cols, ks, rows = (torch.arange(k, dtype=torch.int64, device=device) for k in (C, KP, S))
    g = torch.Generator()
    g.manual_seed(1000 * seed + 7 * image + 3 * T + n + C)
    rnd = lambda *s: torch.randn(s, generator=g)
    if kind == "exact":
        # patch row m carries +-1 at k = 37 (8 m + j + seed) mod 588, j < 8 (37 and 588 are coprime: any 74 consecutive rows hit every (c, py, px), no two rows
        # share a position set), folded back into the pixel layout [n][3][T][image][image]
        m = torch.arange(c.M, dtype=torch.int64, device=device)[:, None]
        j = torch.arange(8, dtype=torch.int64, device=device)[None, :]
        k = 37 * (8 * m + j + seed) % KREAL
        sign = 1 - 2 * ((_mix(m * 1315423911 % (1 << 31) + j * 2654435 + seed * 97 + 1) >> 9) & 1)
        A = torch.zeros((c.M, KREAL), device=device).scatter_(1, k, sign.float())
        c.px = A.view(n, T, c.g, c.g, 3, p, p).permute(0, 4, 1, 2, 5, 3, 6).reshape(n, 3, T, image, image).contiguous()
        nnz = c.px.abs().view(n, 3, T, c.g, p, c.g, p).sum((1, 4, 6)).max()
        assert float(nnz) == 8 and 6 * float(nnz) + 16 + 40 <= 256, "a patch has too many nonzero pixels for exact bf16 sums"
        c.W = exact_W_int(cols, ks, seed).to(bf)                                     # the pad columns [588, Kp) are nonzero too: nothing may read them
        c.bias = (_mix(cols * 7 + seed + 11) % 33 - 16).float() if mode == 1 else None
        cls = (_mix(cols * 13 + seed + 5) % 81 - 40).float()
        pos = (_mix(rows[:, None] * 50021 + cols[None, :] * 31 + seed) % 81 - 40).float()
        assert S < 2 or not bool((pos[1:] == pos[:-1]).all(1).any()), "two neighbouring pos rows are equal"
    else:
        c.px = rnd(n, 3, T, image, image)
        c.W = (rnd(C, KP) * KREAL ** -0.5).to(bf)
        c.bias = (rnd(C) * 0.5).to(bf).float() if mode == 1 else None       # InternVideo2 is a bf16 model: its f32 bias holds bf16 values
        cls, pos = rnd(C) * 0.5, rnd(S, C) * 0.5
    c.cls, c.pos = (cls, pos) if mode == 0 else (cls.to(bf), pos.to(bf))
    if mode == 0:
        c.lnw, c.lnb = 1.0 + 0.2 * rnd(C), 0.2 * rnd(C)
    return c


def patch_cases():
    """every (case) the GPU tests run, exact and bounded: built once per process"""
    out = []
    for kind in ("exact", "bounded"):
        out += [patch_case(0, im, T, n, CLIP_DIM, kind) for im, T, n in CLIP_SHAPES]
        out += [patch_case(1, im, T, n, C, kind) for C in IV2_DIMS for im, T, n in IV2_SHAPES]
    return out


def _conv(px, W, p, n, T, L):
    """the model's patch convolution: stride = kernel = (1, p, p), weight [C][c][py][px] -> [n, T L, C] (flatten(3).permute: patches of a frame row-major, frames in
    order -- internvideo2.py:721-725; with T = 1 it is CLIP's conv2d + flatten(2).transpose(1, 2), modeling_clip.py:185-188)"""
    C = W.shape[0]
    w = W[:, :3 * p * p].reshape(C, 3, 1, p, p)
    y = F.conv3d(px, w, stride=(1, p, p))                            # [n, C, T, g, g]
    return y.flatten(3).permute(0, 2, 3, 1).reshape(n, T * L, C)


def patch_reference(c):
    """-> (ref [n, S, C] float64, bound [n, S, C]) of case c; cached.  Rounding points (gvl_patch.hip, and the three passes alike):
      operands      the f32 pixels are rounded to bf16 (RNE: the same value on both sides, no error term); products of bf16 operands are exact in fp32 and are summed in
                    fp32 in SOME order: |acc32 - acc| <= K U32 sum |a w|, K = 588  (exact cases: every partial sum is a small integer -- no error at all)
      InternVideo2  bf16(acc + bias) [one fp32 add, one bf16 rounding], then the bf16 add of pos [one fp32 add, one bf16 rounding]; the CLS row bf16(cls + pos[0])
      CLIP          bf16(acc) + pos in fp32 [one bf16 rounding, one fp32 add]; the CLS row cls + pos[0] [one fp32 add]; then LayerNorm in fp32 (layernorm_bound), f32 out
    """
    if c._ref is not None:
        return c._ref
    px, W = c.px.to(bf).double(), c.W.double()
    acc = _conv(px, W, c.patch, c.n, c.T, c.L)
    exact = c.kind == "exact"
    e = torch.zeros_like(acc) if exact else KREAL * U32 * _conv(px.abs(), W.abs(), c.patch, c.n, c.T, c.L)
    cls, pos = c.cls.double(), c.pos.double()
    if exact:                                                        # every step is the identity on these integers (asserted)
        v = acc + (c.bias.double() if c.mode == 1 else 0.0) + pos[None, 1:]
        x = torch.cat([(cls + pos[0]).expand(c.n, 1, -1), v], 1)
        assert bool((x == x.round()).all()) and float(x.abs().max()) <= 256 and float(acc.abs().max()) <= 48
        x = _V(x, torch.zeros_like(x))
    elif c.mode == 1:
        v = _V(acc, e).add(c.bias.double()).round_bf16().add(pos[None, 1:]).round_bf16()
        k = _V((cls + pos[0]).expand(c.n, 1, -1), torch.zeros((c.n, 1, c.C), dtype=torch.float64)).f32().round_bf16()
        x = _V(torch.cat([k.x, v.x], 1), torch.cat([k.e, v.e], 1))
    else:
        v = _V(acc, e).round_bf16().add(pos[None, 1:])
        k = _V((cls + pos[0]).expand(c.n, 1, -1), torch.zeros((c.n, 1, c.C), dtype=torch.float64)).f32()
        x = _V(torch.cat([k.x, v.x], 1), torch.cat([k.e, v.e], 1))
    if c.mode == 0:
        x = layernorm_bound(x.x, x.e, c.lnw.double(), c.lnb.double(), c.eps, out_bf16=False)
    c._ref = (x.x, x.e)
    return c._ref


def check_patch(c, out, what):
    """out [n S, C] in the output dtype -> (message or None, largest |err| / bound, number of elements that differ from the rounded reference bitwise).
    InternVideo2 exact cases: bit for bit.  Everything else: zero elements outside the bound."""
    ref, bound = patch_reference(c)
    ref, bound = ref.reshape(-1, c.C).to(out.device), bound.reshape(-1, c.C).to(out.device)
    want = ref.to(out.dtype)
    ndiff = int((out != want).sum()) if out.shape == want.shape else -1
    if c.kind == "exact" and c.mode == 1:
        return exact_mismatch(out, want, what), 0.0 if ndiff == 0 else float("inf"), ndiff
    msg, worst = bound_violations(out, ref, bound, what)
    return msg, worst, ndiff


def emulate_patch(c, mutate=None, pad=PAD_ROWS):
    """the documented arithmetic in fp32 / bf16 torch, written into a guarded buffer as the kernels write theirs -> (buf, out view [n S, C])"""
    px = c.px.to(bf).float()
    p, n, T, L, TL, S, C = c.patch, c.n, c.T, c.L, c.TL, c.S, c.C
    if mutate == "drop_px13":
        px = px.clone()
        px[..., 13::p] = 0
    acc = _conv(px, c.W.float(), p, n, T, L)
    if mutate == "frame_prev":                                       # rows of a 48-row block that holds more than one frame read frame t - 1
        prev = _conv(torch.cat([px[:, :, :1], px[:, :, :-1]], 2), c.W.float(), p, n, T, L).reshape(-1, C)
        m = torch.arange(c.M)
        frame = m // L
        lo = (m // PE_BM) * PE_BM
        straddles = frame[lo] != frame[torch.clamp(lo + PE_BM - 1, max=c.M - 1)]
        acc = torch.where(straddles[:, None], prev, acc.reshape(-1, C)).reshape(n, TL, C)
    pos = c.pos.float()
    prow = pos[1:]
    if mutate == "pos_off1":
        prow = torch.roll(prow, -1, 0)
    k = c.cls.float() + (pos[1] if mutate == "cls_pos1" else pos[0])
    if c.mode == 1:
        v = ((acc + c.bias).to(bf).float() + prow[None]).to(bf)
        x = torch.cat([k.to(bf).expand(n, 1, -1), v], 1)
    else:
        x = torch.cat([k.expand(n, 1, -1), acc.to(bf).float() + prow[None]], 1)
        x = emulate_layernorm(x, c.lnw, c.lnb, c.eps, out_bf16=False)
    buf, out = guarded(n * S, C, c.out_dtype(), pad=pad)
    out.copy_(x.reshape(-1, C))
    if mutate == "dup_tail" and c.M % PE_BM:                         # the tail tile's duplicate of the last row, stored where row M would be
        buf[pad + n * S] = out[-1]
    return buf, out


# ---- norms ----------------------------------------------------------------------------------------------------------------------------------------------------------
def layernorm_bound(x, e, w, b, eps, out_bf16, depth=None):
    """float64 LayerNorm of x over its last dimension and a bound on |kernel - reference| for a kernel that holds values x~ with |x~ - x| <= e and works in fp32
    (two passes: mean, then the sum of squared differences) -> _V.  Derivation (first order in e; U32 = 2^-24; C = columns):
      sums      D = the longest chain of fp32 additions a term of a C-term sum passes through: C - 1 < C for an unknown order (the default); wave_sum_depth(C) for the
                norm kernels, which document one wave per row.  Such a sum is off by at most D U32 sum |terms|
      mean      m~ = fl(sum x~ / C): |mean(x~) - mean(x)| <= mean(e), and the fp32 sum plus the division add (D + 1) U32 mean(|x| + e)                     =: s1
      centred   d~ = fl(x~ - m~): |d~_j - d_j| <= e_j + mean(e) + s1 + U32 |d_j|                                                                          =: e'_j
      variance  v = mean(d^2): dv = (2 / C) sum d_j dd_j <= 2 sqrt(mean d^2) sqrt(mean e'^2) (Cauchy-Schwarz) = 2 sigma E,  E = sqrt(mean_j e'_j^2)
      rstd      r = (v + eps)^-1/2: |dr| / r = dv / (2 (v + eps)) <= sigma E / (v + eps) <= r E   (sigma / (v + eps) <= (v + eps)^-1/2)
                fp32: C squares and their sum (positive terms), the division and the add of eps: (D + 4) U32 relative on v + eps, half of it on r; rsqrt 1 ulp =
                2 U32  ->  relative ((D + 4) / 2 + 2) U32                                                                                                 =: f
      output    y = d r w + b, xh = d r:  |dy_i| <= r |w_i| (e'_i + |xh_i| E) + |xh_i w_i| f + 3 U32 (|xh_i w_i| + |y_i|)   (two products, one sum)
    With e'_j = e_j + mean_k e_k this is  r |w_i| (e'_i + |xh_i| sqrt(mean_j e'_j^2))  plus the fp32 terms of the two C-term sums, the rsqrt and the final arithmetic."""
    C = x.shape[-1]
    D = C if depth is None else depth
    mean = lambda t: t.mean(-1, keepdim=True)
    mu = mean(x)
    d = x - mu
    r = torch.rsqrt(mean(d * d) + eps)
    s1 = (D + 1) * U32 * mean(x.abs() + e)
    e1 = e + mean(e) + s1 + U32 * d.abs()
    E = mean(e1 * e1).sqrt()
    f = ((D + 4) / 2 + 2) * U32
    xh = d * r
    y = xh * w + b
    v = _V(y, r * w.abs() * (e1 + xh.abs() * E) + (xh * w).abs() * f + 3 * U32 * ((xh * w).abs() + y.abs()))
    return v.round_bf16() if out_bf16 else v


def rmsnorm_bound(x, e, w, eps, depth=None):
    """float64 RMSNorm y = bf16(w bf16(x r)), r = (mean x^2 + eps)^-1/2 (internvideo2.py:443-448) -> _V.  The same form as layernorm_bound without the mean subtraction
    (e'_j = e_j): d(mean x^2) <= 2 sqrt(mean x^2) E, E = sqrt(mean e^2), so |dr| / r <= r E; fp32: the squares of bf16 values are exact, a C-term sum, the division, the
    add of eps and the rsqrt: ((D + 3) / 2 + 2) U32 relative on r (D as in layernorm_bound).  x r: one fp32 product, rounded to bf16; times the bf16 weight: one fp32 product, rounded to bf16."""
    C = x.shape[-1]
    mean = lambda t: t.mean(-1, keepdim=True)
    r = torch.rsqrt(mean(x * x) + eps)
    E = mean(e * e).sqrt()
    f = (((C if depth is None else depth) + 3) / 2 + 2) * U32
    xr = x * r
    v = _V(xr, r * e + xr.abs() * (r * E + f)).f32().round_bf16()
    return v.scale(w).round_bf16()


def wave_sum_depth(cols):
    """the norm kernels run one wave per row (gvl_elem.hip): a lane adds its ceil(cols / 64) values in turn, six butterfly steps add the 64 lanes"""
    return (cols + 63) // 64 + 6


def emulate_layernorm(x, w, b, eps, out_bf16, one_pass=False):
    x = x.float()
    mu = x.mean(-1, keepdim=True)
    var = (x * x).mean(-1, keepdim=True) - mu * mu if one_pass else ((x - mu) ** 2).mean(-1, keepdim=True)
    y = (x - mu) * torch.rsqrt(var + eps) * w.float() + b.float()
    return y.to(bf) if out_bf16 else y


def emulate_rmsnorm(x, w, eps):
    xf = x.float()
    r = torch.rsqrt((xf * xf).mean(-1, keepdim=True) + eps)
    return (w.float() * (xf * r).to(bf).float()).to(bf)


def norm_rows(rows, cols, seed, dtype):
    """rows = 1: the row with a large common offset (1000 + noise: a one-pass variance loses it).  rows = 5: a gaussian row, 1000 + noise, an all-zero row, a row with
    a single nonzero element, a small gaussian row.  bf16 rows: the noise is scaled by 8 (the spacing of bf16 at 1000 is 4)."""
    g = torch.Generator()
    g.manual_seed(100 * seed + cols + rows)
    noise = 8.0 if dtype == bf else 1.0
    offset = lambda: 1000.0 + noise * torch.randn(cols, generator=g)
    if rows == 1:
        x = offset()[None]
    else:
        assert rows == 5
        single = torch.zeros(cols)
        single[cols // 3] = 3.5
        x = torch.stack([torch.randn(cols, generator=g) * 2.0, offset(), torch.zeros(cols), single, torch.randn(cols, generator=g) * 0.01])
    w, b = 1.0 + 0.2 * torch.randn(cols, generator=g), 0.2 * torch.randn(cols, generator=g)
    return x.to(dtype), w.to(dtype), b.to(dtype)


# ---- glue -----------------------------------------------------------------------------------------------------------------------------------------------------------
def patchify_ref(px, p, Kp):
    """im2col of a convolution with stride = kernel: row (img, t, gy, gx), column (c, py, px); bf16(px), zero in [3 p^2, Kp) -- bit-exact"""
    n, _, T, H, _ = px.shape
    g = H // p
    A = px.view(n, 3, T, g, p, g, p).permute(0, 2, 3, 5, 1, 4, 6).reshape(n * T * g * g, 3 * p * p).to(bf)
    return torch.cat([A, torch.zeros((A.shape[0], Kp - 3 * p * p), dtype=bf, device=px.device)], 1)


def hd_merge_ref(f, sub_gn):
    """reshape_hd_patches_2x2merge + add_image_newline (llava_next_video.py:454-489): [n, 24 x 24, C] -> [n, 12 x 13, 4 C], channel chunks (dy, dx); bf16 -- bit-exact"""
    n, _, C = f.shape
    x = f.view(n, 12, 2, 12, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(n, 12, 12, 4 * C)
    nl = sub_gn.view(1, 1, 1, 4 * C).expand(n, 12, 1, 4 * C)
    return torch.cat([x, nl], 2).reshape(n, 156, 4 * C).to(bf)


def emulate_hd_merge(f, sub_gn, mutate=None):
    """the same gather written per output element (row = h * 13 + w, chunk = 2 dy + dx)"""
    n, _, C = f.shape
    out = torch.empty((n, 12, 13, 4, C), dtype=torch.float32)
    g = f.view(n, 24, 24, C)
    col_nl = 0 if mutate == "sub_gn_col0" else 12
    cols = [w for w in range(13) if w != col_nl]
    for dy in range(2):
        for dx in range(2):
            out[:, :, cols, 2 * dy + dx] = g[:, dx::2, dy::2] if mutate == "dydx_swap" else g[:, dy::2, dx::2]
    out[:, :, col_nl] = sub_gn.view(4, C)
    return out.reshape(n, 156, 4 * C).to(bf)


def pool_spatial_ref(f):
    """AdaptiveAvgPool [24, 24] -> [8, 8] == the mean of each 3 x 3 block (llava_next_video.py:509-517), float64 -> _V: nine terms summed in fp32 in some order
    (9 U32 sum |x|, i.e. 9 U32 mean |x| on the mean), the division by 9 (two fp32 ulps = 4 U32), one rounding to bf16"""
    n, _, C = f.shape
    x = f.double().view(n, 8, 3, 8, 3, C)
    m, am = x.mean((2, 4)).reshape(n, 64, C), x.abs().mean((2, 4)).reshape(n, 64, C)
    return _V(m, 9 * U32 * am).f32(4).round_bf16()


def emulate_pool_spatial(f, mutate=None):
    g = f.float().view(f.shape[0], 24, 24, -1)
    if mutate == "window_shift":
        g = torch.roll(g, -1, 2)
    acc = torch.zeros((f.shape[0], 8, 8, f.shape[2]))
    for dy in range(3):
        for dx in range(3):
            acc = acc + g[:, dy::3, dx::3]
    return (acc / 9.0).reshape(f.shape[0], 64, -1).to(bf)


def pool_temporal_ref(f):
    """AdaptiveAvgPool [T, 16, 16] -> [T, 4, 4] == the mean of each 4 x 4 block per frame (llava_next_video.py:543-549), f bf16 [n, T, 256, C], float64 -> _V: sixteen bf16
    values summed in fp32 in some order (16 U32 mean |x| on the mean), times 2^-4 (exact), one rounding to bf16"""
    n, T, _, C = f.shape
    x = f.double().view(n, T, 4, 4, 4, 4, C)
    m, am = x.mean((3, 5)).reshape(n, T, 16, C), x.abs().mean((3, 5)).reshape(n, T, 16, C)
    return _V(m, 16 * U32 * am).round_bf16()


def emulate_pool_temporal(f):
    n, T, _, C = f.shape
    g = f.float().view(n, T, 16, 16, C)
    acc = torch.zeros((n, T, 4, 4, C))
    for dy in range(4):
        for dx in range(4):
            acc = acc + g[:, :, dy::4, dx::4]
    return (acc * 0.0625).reshape(n, T, 16, C).to(bf)


def int_field(shape, lo, hi, seed, device="cpu"):
    """seeded integers in [lo, hi] as f32 (device-side for the cases that are large enough to wrap a grid)"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, device=device).float()


def pool_spatial_exact_input(n, C, seed, device="cpu"):
    """f32 [n, 576, C] of integers whose 3 x 3 windows each sum to 9 times an integer mean in [-20, 20]: the window holds mean + (a, -a, b, -b, c, -c, d, -d, 0) rolled by a
    per-window offset; every partial sum, in any order, is an integer below 256 and the division by 9 is exact -> the output is the mean, bit for bit.  A window
    shifted by one sums other values."""
    mean = int_field((n, 8, 8, 1, C), -20, 20, seed, device)
    a = int_field((n, 8, 8, 4, C), -5, 5, seed + 1, device)
    d = torch.cat([torch.stack([a, -a], 4).reshape(n, 8, 8, 8, C), torch.zeros_like(mean)], 3)            # [n, 8, 8, 9, C], sums to 0
    roll = (torch.arange(9, device=device)[None, :] + torch.arange(64, device=device)[:, None]) % 9         # window-dependent order
    d = torch.gather(d, 3, roll.view(1, 8, 8, 9, 1).expand(n, 8, 8, 9, C))
    w = (mean + d).view(n, 8, 8, 3, 3, C).permute(0, 1, 3, 2, 4, 5)                                         # [n, ph, dy, pw, dx, C]
    return w.reshape(n, 576, C).contiguous(), mean.reshape(n, 64, C).to(bf)


# ---- the row-remapping GEMM store -----------------------------------------------------------------------------------------------------------------------------------
def grouped_rows(M, grp_rows, grp_stride, row_off, device="cpu"):
    """destination row of GEMM row m: m -> (m / grp_rows) * grp_stride + m % grp_rows + row_off, and the number of rows of the output buffer"""
    m = torch.arange(M, device=device)
    groups = (M + grp_rows - 1) // grp_rows
    return (m // grp_rows) * grp_stride + m % grp_rows + row_off, groups * grp_stride


def scatter_groups(dense, grp_rows, grp_stride, row_off, mutate=None):
    """what the grouped store leaves in a sentinel-filled buffer, given the dense GEMM's output [M, N]"""
    M = dense.shape[0]
    dst, total = grouped_rows(M, grp_rows, grp_stride, row_off, dense.device)
    if mutate == "stride_is_rows":
        dst, _ = grouped_rows(M, grp_rows, grp_rows, row_off, dense.device)
    buf = torch.full((total, dense.shape[1]), SENT, dtype=dense.dtype, device=dense.device)
    buf[dst] = dense
    return buf


def check_grouped(buf, dense, grp_rows, grp_stride, row_off):
    """-> (wrong elements inside the groups, elements outside the groups that lost the sentinel)"""
    dst, total = grouped_rows(dense.shape[0], grp_rows, grp_stride, row_off, dense.device)
    assert buf.shape == (total, dense.shape[1])
    inside = torch.zeros(total, dtype=torch.bool, device=buf.device)
    inside[dst] = True
    return int((buf[dst] != dense).sum()), int((buf[~inside] != SENT).sum())
