"""Independent references for the decode projections (gvl_decode.hip dgemm_kernel, gvl_elem.hip gemv_kernel, reached through gvl_op_decode_proj) and for
the four weight quantiser kernels -- no GPU needed to import or run this file.  Companion of gemm_ref.py (same two families, same bound machinery).

Quantiser restatements   fp8_quant / mxfp4_quant, plain numpy float64 + integer arithmetic from the format definitions (OCP e4m3fn: 3 mantissa bits, normals
  2^-6 .. 448, subnormals k 2^-9; OCP MX v1.0: E2M1 elements {0, .5, 1, 1.5, 2, 3, 4, 6}, one E8M0 scale per 32 consecutive k).  They do not call the oracle's
  fp8_pow2_dequant / mxfp4_dequant; test_decode_proj_ref_cpu.py compares the two, and both with torch.float8_e4m3fn.
  MXFP4 scale byte 0: the library's convention (include/gvl.h) -- a block whose largest magnitude has an fp32 exponent field <= 2 (below 2^-124) gets scale
  byte 0 and de-quantises to +0 everywhere.  Kernel, this restatement and oracle.mxfp4_dequant agree on it.

exact_case(N, K, batch, form, seed, w_fmt, wide)   operands on which every number the kernel forms is exactly representable: the expected output comes from
  a float64 product that involves no rounding and must be reproduced BIT FOR BIT, whatever the k-slice split, the group order or the wave reduction.
    x     rows of gemm_ref.exact_A: 8 entries of +-1, one at the LAST k, seven in chunks (7 m + j) mod K / 8 of row m = seed * batch + b; the rows
          0 .. rounds_to_cover(K, batch) * batch - 1 hit every 8-element chunk of every 32-k step (the CPU test asserts it); rows differ
    W     w_fmt 0: integers in [-6, 6] (gemm_ref.exact_W_int).
          w_fmt 1: narrow  64 * 2^r * integer in [-6, 6], r in [-2, 2] per 16-row block, one |integer| = 6 planted per row: e4m3 values under the row scale 2^r
                   wide    2^r * i * 2^j with r per ROW, j in [-9, 3] per element (|i 2^j| on the 2^-9 grid, sub-normals of e4m3 included) and +-448 planted
                           once per row: partial sums of 8 stay below 784 * 4 on a 2^-11 grid -- under 2^24 units
          w_fmt 2: narrow  2^e * E2M1 grid value, e per 16-row block, +-4 or +-6 planted in every block of 32
                   wide    the same with e in [0, 11] per (row, block of 32): partial sums of 8 below 8 * 6 * 2^11 on a grid of 1/2 -- under 2^24 units
          Quantising such W is the identity (asserted when the case is built), so the GPU test isolates the stream layout and the widening.
    bias, resid   integers times the row's unit: acc + bias <= 64 units, + resid <= 124 units (248 half units for MXFP4): exact in bf16
    sq_out        16 squares of at most 124 units each (one unit per 16-row block): exact in fp32 in any order
    sq_in         partial sums that the kernel's order adds without rounding while other associations round (see exact_sq_in); the total is K * 4^m per
                  sequence, so rsqrt gives 2, 1 or 1/2 and the scaled accumulators stay exact
    rope          tables (cos, sin) = (1, 0), (0, 1), or (1, 0) short / (0, -1) long: rotation sign, partner and placement, no arithmetic.
                  first_page / n_pages: the page tables name first_page + (the same pages) in caller-owned pools of n_pages pages; expect_Kt / expect_Vt hold the 24
                  pages first_page .. first_page + 23 only (c.page0, c.win).  rope_relocated_cases(): cases of the GPU test's rope sweep on pages whose element
                  offsets lie above 2^31 (one above 2^30); rope_emulate / rope_mismatch: the epilogue in float32 over SPARSE pools (page id -> array), and the
                  comparison the GPU test makes, for test_decode_proj_ref_cpu.py
  SwiGLU is not exact (the sigmoid): it belongs to the bounded family.

bounded_*(...)   dense data (row scales 2^-6 .. 2^6, K^-0.5 weights), a float64 reference with the bf16 roundings where the kernels place them and a PER-ELEMENT
  bound derived as in gemm_ref.elementwise_bound (fp32 accumulation over K terms, a bf16 rounding whose input may differ, each error carried through what
  follows).  One refinement over gemm_ref: where a value within e of x is rounded to bf16, the bound is the distance from rbf(x) to the roundings of x - e and
  x + e (_round: rounding is monotone) rather than e + one ulp -- zero unless a tie point lies inside the interval.  The norm prologue needs it: K normalised
  activations feed every output, and one ulp on each of them would allow 5 % of the output scale.  Hardware approximations: fast_sigmoid through gemm_ref._sigmoid (the constant test_sigmoid_epilogues_on_every_bf16_input pins);
  rsqrtf at RSQRT_ULP = 1 ulp, the figure the HIP math API documents for rsqrtf.
"""
import functools

import numpy as np
import torch

import gemm_ref as G
from kv_page_ref import PAGE_MUTATIONS, POOL_ELEMS, first_page_above, wrap_page_offset

bf = torch.bfloat16
MUTATIONS = PAGE_MUTATIONS          # wrong kernels of rope_emulate: a page's base address formed in 32 bits (kv_page_ref.wrap_page_offset)
U32 = G.U32
ACT_NONE, ACT_SILU_MUL = 0, 3
RSQRT_ULP = 1.0                     # HIP math API: rsqrtf, maximum error 1 ulp
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
E2M1_TIES = (E2M1[:-1] + E2M1[1:]) / 2            # 0.25 0.75 1.25 1.75 2.5 3.5 5.0


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------------------
def xt_index(j, k):
    """gvl_xt_index: element (sequence j < 16, column k) of the decode activation tile order"""
    return ((k >> 5) * 64 + (((k >> 3) & 3) * 16 + j)) * 8 + (k & 7)


def to_tiled(rows):
    """[B, cols] -> the 16 * cols elements of the tile order (slots of absent sequences: 0)"""
    B, n = rows.shape
    out = torch.zeros((16 * ((n + 31) // 32) * 32,), dtype=rows.dtype)
    k = torch.arange(n)
    for b in range(B):
        out[xt_index(b, k)] = rows[b]
    return out


def from_tiled(t, B, n):
    k = torch.arange(n)
    return torch.stack([t[xt_index(b, k)] for b in range(B)])


def logical_rows(N, Dr=0, n_qk=0):
    """perm[n] = the weight row that LOGICAL row n of the decode copy reads: with Dr > 0 the q and k heads are visited in rotate-half partner pairs,
    logical (2 j, 2 j + 1) = weight rows (hd Dr + d, hd Dr + d + Dr / 2), j = hd Dr / 2 + d"""
    n = np.arange(N)
    if Dr <= 0:
        return n
    half = Dr // 2
    j = n >> 1
    hd, d = j // half, j % half
    return np.where(j < n_qk * half, hd * Dr + d + (n & 1) * half, n)


def _f64(W):
    return W.to(bf).float().numpy().astype(np.float64) if isinstance(W, torch.Tensor) else np.asarray(W, dtype=np.float64)


# ---- quantiser restatements ------------------------------------------------------------------------------------------------------------------------
def fp8_quant(W, Dr=0, n_qk=0):
    """-> (deq [N, K] float64 in LOGICAL row order, scale [N] float64 by logical row, None).  scale = the smallest power of two >= max|row| / 448 (1 for an
    all-zero row); element = RNE of w / scale to e4m3fn, times scale; the sign survives a zero result"""
    w = _f64(W)[logical_rows(W.shape[0], Dr, n_qk)]
    m = np.abs(w).max(1)
    f, ex = np.frexp(m)                                      # m = f 2^ex, f in [0.5, 1); 448 = 0.875 * 2^9
    k = np.where(f <= 0.875, ex - 9, ex - 8)
    s = np.where(m > 0, np.ldexp(1.0, k), 1.0)
    t = np.abs(w) / s[:, None]                               # exact
    _, e = np.frexp(t)
    step = np.ldexp(1.0, np.maximum(e - 1, -6) - 3)          # spacing of e4m3 at t: 2^(floor(log2 t) - 3), 2^-9 below the smallest normal
    q = np.minimum(np.rint(t / step) * step, 448.0)          # rint: to nearest, ties to even
    return np.copysign(q * s[:, None], w), s, None


def e2m1_code(t):
    """t >= 0 (float64) -> the E2M1 code 0 .. 7 nearest to t, ties to the even code, saturating at 6.0"""
    code = (t[..., None] > E2M1_TIES).sum(-1)
    for i, tie in enumerate(E2M1_TIES):
        code = np.where(t == tie, i if i % 2 == 0 else i + 1, code)
    return code


def mxfp4_quant(W, Dr=0, n_qk=0):
    """-> (deq [N, K] float64 in logical row order, None, e8 [N, K / 32] uint8 by logical row).  e8 = (fp32 exponent field of the block's max|w|) - 2, clamped to
    [0, 254]; 0 for an all-zero block, and e8 == 0 means a block of zeros"""
    N, K = W.shape
    w = _f64(W)[logical_rows(N, Dr, n_qk)].reshape(N, K // 32, 32)
    m = np.abs(w).max(2)
    _, ex = np.frexp(m)                                      # normal fp32: exponent field = floor(log2 m) + 127 = ex + 126
    field = np.where(m >= 2.0 ** -126, ex + 126, 0)
    e8 = np.where(m > 0, np.clip(field - 2, 0, 254), 0)
    X = np.ldexp(1.0, e8 - 127)[..., None]
    q = E2M1[e2m1_code(np.abs(w) / X)] * X
    deq = np.where(e8[..., None] > 0, np.copysign(q, w), 0.0)
    return deq.reshape(N, K), None, e8.astype(np.uint8)


def mxfp4_scale_words(e8):
    """[N, K / 32] scale bytes -> the library's scale words [ceil(N / 16)][K / 128][16] uint32 (byte j of a word: k step 4 (k / 128) + j); rows past N: 0"""
    N, nkt = e8.shape
    nb = (N + 15) // 16
    p = np.zeros((nb * 16, nkt), dtype=np.uint8)
    p[:N] = e8
    return np.ascontiguousarray(p.reshape(nb, 16, nkt // 4, 4).transpose(0, 2, 1, 3)).view("<u4").reshape(nb, nkt // 4, 16)


def quant(W, w_fmt, Dr=0, n_qk=0):
    """the de-quantised weight in W's OWN row order, as a bf16 tensor (w_fmt 0: W itself)"""
    if not w_fmt:
        return W
    deq = (fp8_quant if w_fmt == 1 else mxfp4_quant)(W, Dr, n_qk)[0]
    out = np.empty_like(deq)
    out[logical_rows(W.shape[0], Dr, n_qk)] = deq
    t = torch.from_numpy(out)
    r = t.to(bf)
    assert bool((r.double() == t).all()), "a de-quantised value is not a bf16 number"
    return r


# ---- exact family ----------------------------------------------------------------------------------------------------------------------------------
# form -> what the call carries.  out: "f32" / "bf16"
EXACT_FORMS = {
    "plain": dict(out="f32"), "bias": dict(out="f32", bias=1), "bf16": dict(out="bf16", bias=1), "resid": dict(out="bf16", bias=1, resid=1),
    "producer": dict(out="bf16", resid=1, producer=1), "consumer": dict(out="f32", bias=1, consumer=1),
    "rope10": dict(rope=((1, 0), (1, 0))), "rope01": dict(rope=((0, 1), (0, 1))), "rope_switch": dict(rope=((1, 0), (0, -1))),
}
ROPE_POS = (0, 63, 64, 130)
ROPE_SWITCH = 64
SENTINEL = -1.75                                            # what Q / Kt / Vt are filled with before the call: no exact output (integers, multiples of 16 for FP8, of 1 / 2 for
                                                            # MXFP4) can equal it -- _rope_expect asserts that for every case it builds


class Case:
    pass


def rounds_to_cover(K, batch):
    """x rows 0 .. rounds * batch - 1 hit every 8-element chunk: row m covers chunks 7 m .. 7 m + 6 (mod K / 8)"""
    rows = -(-(K // 8) // 7)
    return -(-rows // batch)


def exact_x(K, batch, seed):
    rows = seed * batch + torch.arange(batch, dtype=torch.int64)
    return G.exact_A(rows, K, 0)


@functools.lru_cache(maxsize=4)
def exact_W(N, K, w_fmt, wide, seed):
    """-> (W float64 [N, K] in LOGICAL row order, unit [N] float64: bias / resid are integers times it).  Cached: callers must not write to the arrays"""
    n, k = torch.arange(N, dtype=torch.int64), torch.arange(K, dtype=torch.int64)
    wi = G.exact_W_int(n, k, seed).numpy().astype(np.float64)
    h = G._mix(n[:, None] * 7919 + k[None, :] * 104729 + seed * 31 + 3).numpy()
    hn = G._mix((n if wide else n >> 4) * 613 + seed * 17 + 9).numpy()
    rows = np.arange(N)
    if w_fmt == 0:
        return wi, np.ones(N)
    if w_fmt == 1:
        r = hn % 5 - 2
        plant = G._mix(n * 37 + seed + 1).numpy() % (K - 1)                     # never the last k: x's entry there must meet an ordinary value too
        sgn = 1.0 - 2.0 * ((hn >> 8) & 1)
        if wide:
            v = wi * np.ldexp(1.0, h % 13 - 9)
            v[rows, plant] = 448.0 * sgn
            return v * np.ldexp(1.0, r)[:, None], np.ldexp(1.0, r)
        v = wi.copy()
        v[rows, plant] = 6.0 * sgn
        return v * np.ldexp(64.0, r)[:, None], np.ldexp(64.0, r)
    g = E2M1[h % 8] * (1.0 - 2.0 * ((h >> 5) & 1))
    blk = np.arange(K // 32)
    hb = G._mix(n[:, None] * 131 + torch.arange(K // 32, dtype=torch.int64)[None, :] * 977 + seed * 5 + 2).numpy()
    g = g.reshape(N, K // 32, 32)
    slot = np.where(blk[None, :] == K // 32 - 1, hb % 31, hb % 32)               # the last block: not at the last k
    g[rows[:, None], blk[None, :], slot] = np.where((hb >> 7) & 1, 4.0, 6.0) * (1.0 - 2.0 * ((hb >> 9) & 1))
    e = (hb >> 11) % 12 if wide else np.broadcast_to((hn % 12)[:, None], hb.shape)
    return (g * np.ldexp(1.0, e)[..., None]).reshape(N, K), (np.ones(N) if wide else np.ldexp(1.0, hn % 12))


def exact_sq_in(batch, sq_n, K, nw, seed):
    """-> (sq [batch, sq_n] float32, rs [batch] float64).  The kernel adds sequence b's partials as: lane (w, g) left-folds its per = sq_n / (4 nw) partials
    [(4 w + g) per, ...) from 0; wave w forms (s0 + s1) + (s2 + s3); the waves are left-folded in order.  Data: the four lane sums of wave w are
    (A, a - A, A, c - A) with A = 2^24, a = 1 or 5 and c odd: the kernel's pairs cancel exactly, while a left fold ((s0 + s1) + s2) + s3 forms a + A, an
    odd number above 2^24 that 24 bits cannot hold, and comes out 1 short in every wave.  The lane sum sits at a hashed index of the lane's partials, zeros elsewhere
    (a skipped index loses it).  Total = K * 4^m, m in {-1, 0, 1} by sequence: rsqrt(total / K) = 2, 1, 1/2."""
    per = sq_n // (4 * nw)
    A = 2.0 ** 24
    sq = np.zeros((batch, sq_n), dtype=np.float64)
    rs = np.zeros(batch)
    for b in range(batch):
        m = (b + seed) % 3 - 1
        target = K * 4.0 ** m
        h = G._mix(torch.arange(2 * nw, dtype=torch.int64) * 71 + b * 1009 + seed * 13 + 4).numpy()
        small = (h % 4) * 2 + 1.0                                              # odd, 1 .. 7: the first 2 nw - 1 sum to at most 105 < K / 4
        small[0::2] = (h[0::2] % 2) * 4 + 1.0                                  # a = 1 or 5: A + a is a tie that goes DOWN every time (no wave can cancel another's miss)
        small[-1] = target - small[:-1].sum()                                  # odd as well: target is even, 2 nw - 1 odd numbers sum to an odd number
        assert small[-1] % 2 == 1 and 0 < small[-1] < 2 ** 20
        for w in range(nw):
            lane = (A, small[2 * w] - A, A, small[2 * w + 1] - A)
            for g in range(4):
                j = int(G._mix(torch.tensor(b * 97 + w * 11 + g * 5 + seed)).item()) % per
                sq[b, (4 * w + g) * per + j] = lane[g]
        rs[b] = 2.0 ** -m
    out = sq.astype(np.float32)
    assert (out.astype(np.float64) == sq).all()
    return torch.from_numpy(out), rs


def sq_in_sum(sq_row, nw, order="kernel"):
    """float32 emulation of the consumer's reduction of one sequence's partials; order "kernel" or a deliberately different association ("fold")"""
    f = np.float32
    per = sq_row.shape[0] // (4 * nw)
    tot = f(0)
    for w in range(nw):
        s = []
        for g in range(4):
            a = f(0)
            for j in range(per):
                a = f(a + f(sq_row[(4 * w + g) * per + j]))
            s.append(a)
        ws = f(f(s[0] + s[1]) + f(s[2] + s[3])) if order == "kernel" else f(f(f(s[0] + s[1]) + s[2]) + s[3])
        tot = f(tot + ws)
    return tot


def exact_case(N, K, batch, form, seed=0, w_fmt=0, wide=False, rope_geo=None, nw=8, first_page=0, n_pages=None):
    """see the module docstring.  rope forms: rope_geo = (H, KV, Dr, D), N = (H + 2 KV) Dr.  -> Case: W, x (bf16), the epilogue operands, kwargs for
    Engine.op_decode_proj without the output buffers, and the expected outputs (expect / expect_sq / expect_Q / expect_Kt / expect_Vt)"""
    f = EXACT_FORMS[form]
    c = Case()
    c.N, c.K, c.batch, c.form, c.w_fmt, c.f = N, K, batch, form, w_fmt, f
    assert not wide or f.get("out") == "f32"
    Dr, n_qk = 0, 0
    if "rope" in f:
        H, KV, Dr, D = rope_geo
        assert N == (H + 2 * KV) * Dr
        n_qk = H + KV
    perm = logical_rows(N, Dr, n_qk)
    Wl, unit_l = exact_W(N, K, w_fmt, wide, seed % 3)               # three weight matrices per shape: the x rows are what changes with every seed
    Wd = np.empty_like(Wl)
    Wd[perm] = Wl
    unit = np.empty_like(unit_l)
    unit[perm] = unit_l
    c.W = torch.from_numpy(Wd).to(bf)
    assert bool((c.W.double().numpy() == Wd).all())
    if w_fmt:                                               # quantising this W changes nothing, and the scales are the designed ones
        deq, s, e8 = (fp8_quant if w_fmt == 1 else mxfp4_quant)(c.W, Dr, n_qk)
        assert (deq == Wl).all(), "exact_W: quantisation is not the identity"
        c.scale, c.e8 = s, e8
    c.x = exact_x(K, batch, seed)
    acc = c.x.double().numpy() @ Wd.T                       # [batch, N], weight-row order; integers times a grid unit: no rounding in float64
    c.kw = dict(w_fmt=w_fmt)
    n_t, b_t = torch.arange(N, dtype=torch.int64), torch.arange(batch, dtype=torch.int64) + seed * batch
    if "rope" in f:
        _rope_expect(c, acc, rope_geo, f["rope"], seed, first_page, n_pages)
        return c
    v = acc
    if f.get("consumer"):
        c.sq_in, rs = exact_sq_in(batch, K // 16, K, nw, seed)
        c.kw.update(sq_n=K // 16, eps=0.0)
        v = v * rs[:, None]
    if f.get("bias"):
        bi = (G._mix(n_t * 7 + seed + 11) % 33 - 16).numpy() * unit
        c.bias = torch.from_numpy(bi).float()
        v = v + bi[None, :]
    if f.get("resid"):
        ri = (G._mix(b_t[:, None] * 50021 + n_t[None, :] * 31 + seed) % 121 - 60).numpy() * unit[None, :]
        c.resid = torch.from_numpy(ri).to(bf)
        v = v + ri
    out = torch.from_numpy(v)
    c.expect = out.float() if f["out"] == "f32" else out.to(bf)
    assert bool((c.expect.double() == out).all()), "the expected values are not representable in the output type"
    if f.get("producer"):
        assert N % 16 == 0
        c.expect_sq = torch.from_numpy((v ** 2).reshape(batch, N // 16, 16).sum(-1)).float()
        assert bool((c.expect_sq.double().numpy() == (v ** 2).reshape(batch, N // 16, 16).sum(-1)).all())
    return c


def rope_tables(max_pos, half, cs):
    return torch.full((max_pos, half), float(cs[0])), torch.full((max_pos, half), float(cs[1]))


def rope_layout(batch, seed, table_stride=4, n_pages=24, first_page=0):
    """positions ROPE_POS mixed across the batch and a page table per sequence: a non-identity permutation of distinct pages first_page .. first_page + n_pages - 1"""
    pos = torch.tensor([ROPE_POS[(b + seed) % len(ROPE_POS)] for b in range(batch)], dtype=torch.int32)
    assert batch <= n_pages                                 # every sequence writes a page of its own
    g = torch.Generator().manual_seed(1234 + seed)
    tables = torch.stack([torch.randperm(n_pages, generator=g)[:table_stride] for _ in range(batch)]).to(torch.int32)
    # the pages that are WRITTEN (one per sequence) must differ, or two sequences with equal slots would collide
    used = set()
    for b in range(batch):
        pg = int(pos[b]) >> 6
        while int(tables[b, pg]) in used:
            tables[b, pg] = (int(tables[b, pg]) + 1) % n_pages
        used.add(int(tables[b, pg]))
    return pos, tables + first_page, n_pages


def rope_place(q, k, v, pos, tables, n_pages, geo, dtype=bf, fill=SENTINEL):
    """q [B, H, Dr], k / v [B, KV, Dr] -> (Q [B, H * D], Kt [pages, KV, 64, D], Vt [pages, KV, D, 64]) with `fill` everywhere else"""
    H, KV, Dr, D = geo
    B = q.shape[0]
    Q = torch.full((B, H, D), fill, dtype=dtype)
    Kt = torch.full((n_pages, KV, 64, D), fill, dtype=dtype)
    Vt = torch.full((n_pages, KV, D, 64), fill, dtype=dtype)
    for b in range(B):
        p = int(pos[b])
        page, slot = int(tables[b, p >> 6]), p & 63
        Q[b, :, :Dr] = q[b].to(dtype)
        Kt[page, :, slot, :Dr] = k[b].to(dtype)
        Vt[page, :, :Dr, slot] = v[b].to(dtype)
    return Q.reshape(B, H * D), Kt, Vt


def _rope_expect(c, acc, geo, cs, seed, first_page=0, n_pages=None):
    H, KV, Dr, D = geo
    half = Dr // 2
    B = c.batch
    c.geo = geo
    c.pos, c.tables, c.win = rope_layout(B, seed, first_page=first_page)
    c.page0, c.page_elems, c.n_pages = first_page, KV * 64 * D, n_pages or first_page + c.win
    assert first_page + c.win <= c.n_pages
    c.max_pos = max(ROPE_POS) + 2
    (c.cos_s, c.sin_s), (c.cos_l, c.sin_l) = rope_tables(c.max_pos, half, cs[0]), rope_tables(c.max_pos, half, cs[1])
    y = torch.from_numpy(acc).reshape(B, H + 2 * KV, Dr)
    qk = y[:, :H + KV]
    out = torch.empty_like(qk)
    for b in range(B):
        co, si = cs[1] if int(c.pos[b]) + 1 > ROPE_SWITCH else cs[0]
        x1, x2 = qk[b, :, :half], qk[b, :, half:]
        out[b, :, :half] = x1 * co - x2 * si
        out[b, :, half:] = x2 * co + x1 * si
    c.expect_Q, c.expect_Kt, c.expect_Vt = rope_place(out[:, :H], out[:, H:], y[:, H + KV:], c.pos, c.tables - c.page0, c.win, geo)
    want = torch.cat([out, y[:, H + KV:]], 1)
    assert bool((want.to(bf).double() == want).all()), "rope: expected values not representable in bf16"
    assert not bool((want == SENTINEL).any()), "rope: an expected value equals the sentinel and could not be told from an unwritten element"
    c.kw.update(rope_on=1, rope_switch=ROPE_SWITCH, max_pos=c.max_pos, n_pages=c.n_pages, table_stride=c.tables.shape[1], q_stride=H * D, H=H, KV=KV, Dr=Dr, D=D)


# (geo, form, w_fmt, K, batch, path, k): cases of test_gpu_decode_proj.py's rope sweep, pages from the first one at or above 2^k elements of POOL_ELEMS pools
def rope_relocated_cases():
    """the VALU kernel at batch 1, 2 and 4, the skinny GEMM at batch 16 and at 5 with the three weight formats; k = 30: byte offsets between 2^31 and 2^32"""
    g = ((8, 8, 96, 128), (8, 2, 128, 128), (4, 4, 64, 64))
    return [(g[0], "rope_switch", 0, 256, 16, 0, 31), (g[1], "rope01", 1, 512, 5, 0, 31), (g[2], "rope10", 2, 1024, 5, 0, 31), (g[1], "rope_switch", 0, 256, 5, 0, 31),
            (g[0], "rope01", 0, 256, 1, 1, 31), (g[2], "rope_switch", 0, 256, 2, 1, 31), (g[1], "rope10", 0, 256, 4, 1, 31), (g[1], "rope_switch", 0, 256, 16, 0, 30)]


def rope_relocated_case(geo, form, w_fmt, K, batch, path, k, seed=0):
    H, KV, Dr, D = geo
    pe = KV * 64 * D
    return exact_case((H + 2 * KV) * Dr, K, batch, form, seed=seed, w_fmt=w_fmt, rope_geo=geo, first_page=first_page_above(1 << k, pe), n_pages=POOL_ELEMS // pe)


def rope_emulate(c, mut=None):
    """the rope epilogue of an exact case in float32, writing THROUGH the page tables into sparse pools -> dict(Q = bf16 [B, H D], Kt / Vt = {page id: bf16 page over the
    sentinel}).  mut (MUTATIONS): the page's offset wraps, the write lands at ("stray", element offset) instead"""
    H, KV, Dr, D = c.geo
    half, B = Dr // 2, c.batch
    y = (c.x.float() @ c.W.float().T).view(B, H + 2 * KV, Dr)          # exact in fp32 (test_exact_cases_are_exact)
    Q = torch.full((B, H, D), SENTINEL, dtype=bf)
    Kt, Vt = {}, {}
    for b in range(B):
        p = int(c.pos[b])
        co, si = (c.cos_l[p], c.sin_l[p]) if p + 1 > ROPE_SWITCH else (c.cos_s[p], c.sin_s[p])
        x1, x2 = y[b, :H + KV, :half], y[b, :H + KV, half:]
        qk = torch.cat([x1 * co - x2 * si, x2 * co + x1 * si], -1).to(bf)
        page, slot = int(c.tables[b, p >> 6]), p & 63
        off = page * c.page_elems
        key = page if wrap_page_offset(off, mut) == off else ("stray", wrap_page_offset(off, mut))
        Q[b, :, :Dr] = qk[:H]
        Kt.setdefault(key, torch.full((KV, 64, D), SENTINEL, dtype=bf))[:, slot, :Dr] = qk[H:]
        Vt.setdefault(key, torch.full((KV, D, 64), SENTINEL, dtype=bf))[:, :Dr, slot] = y[b, H + KV:].to(bf)
    return dict(Q=Q.reshape(B, H * D), Kt=Kt, Vt=Vt)


def rope_mismatch(c, got):
    """None when Q and the pages c.page0 .. c.page0 + c.win - 1 of sparse pools equal the expectation bit for bit and nothing else was written, else the message"""
    msgs = []
    if not torch.equal(got["Q"].view(torch.int16), c.expect_Q.view(torch.int16)):
        msgs.append("Q differs")
    for name, exp in (("Kt", c.expect_Kt), ("Vt", c.expect_Vt)):
        for w in range(c.win):
            page = got[name].get(c.page0 + w)
            page = torch.full_like(exp[w], SENTINEL) if page is None else page
            bad = (page.view(torch.int16) != exp[w].view(torch.int16)).nonzero()
            if bad.numel():
                i = tuple(bad[0].tolist())
                msgs.append(f"{name}: page {c.page0 + w}: {bad.shape[0]} elements wrong; first at {list(i)}: got {float(page[i])}, expected {float(exp[w][i])} (sentinel {SENTINEL} = not written)")
                break
        other = [k for k in got[name] if not (isinstance(k, int) and c.page0 <= k < c.page0 + c.win)]
        if other:
            msgs.append(f"{name}: {len(other)} pages written outside pages {c.page0} .. {c.page0 + c.win - 1}: {other[:2]}")
    return "; ".join(msgs) if msgs else None


def recompute_fp32(c, order):
    """the accumulator of an exact case in float32 under a given summation order over k (a permutation): must equal the float64 product bit for bit"""
    W, x = c.W.float().numpy(), c.x.float().numpy()
    acc = np.zeros((c.batch, c.N), dtype=np.float32)
    for k in order:
        if x[:, k].any():
            acc = (acc + x[:, k:k + 1] * W[None, :, k]).astype(np.float32)
    return acc


# ---- bounded family --------------------------------------------------------------------------------------------------------------------------------
def bounded_data(N, K, batch, seed, w_fmt=0, Dr=0, n_qk=0):
    """-> (x bf16 [batch, K] with row scales 2^-6 .. 2^6, W bf16 [N, K] ~ K^-0.5, Wq: the weight the kernel evaluates -- W itself or its de-quantised form)"""
    g = torch.Generator().manual_seed(seed)
    scale = torch.exp2(torch.rand((batch, 1), generator=g) * 12 - 6)
    x = (torch.randn((batch, K), generator=g) * scale).to(bf)
    W = (torch.randn((N, K), generator=g) * K ** -0.5).to(bf)
    return x, W, quant(W, w_fmt, Dr, n_qk)


def _round(v):
    """bf16 rounding of a value known to lie in [x - e, x + e]: rounding is monotone, so the kernel's rounded value lies between the roundings of the two ends --
    far sharper than e + one ulp where e is small against the ulp (the two sides then round alike unless a tie point sits in the interval).  The ends are
    widened by one fp32 ulp first: _rbf goes through fp32, whose own rounding may move an end across a tie."""
    lo, hi = v.x - v.e, v.x + v.e
    pad = lambda t: U32 * t.abs() + 2.0 ** -140
    r, rl, rh = G._rbf(v.x), G._rbf(lo - pad(lo)), G._rbf(hi + pad(hi))
    return G._V(r, torch.maximum(rh - r, r - rl))


def _acc(xv, W):
    """xv: _V of the B operand [batch, K] (e = 0 when both sides hold the same bf16 values) -> _V of the fp32 accumulator: K-term running-sum error on top of
    the operand error carried through |W|"""
    Wd = W.double()
    e_in = xv.e @ Wd.abs().T if torch.is_tensor(xv.e) else 0.0
    return G._V(xv.x @ Wd.T, e_in + W.shape[1] * U32 * ((xv.x.abs() + xv.e) @ Wd.abs().T))


def swiglu_bound(x, Wq, out_f32=False):
    """SwiGLU epilogue on interleaved (gate, up) rows: gemm_ref's bound for the same arithmetic (rbf(acc); u * rbf(g sigmoid(g)); the store)"""
    c = G.Case(x.shape[0], Wq.shape[0], Wq.shape[1], "silu", ("silu", "f32") if out_f32 else ("silu",))
    c.A, c.W = x, Wq
    ref, bound, _, _ = G.elementwise_bound(c)
    return ref, bound


def _rstd(ss, K, eps):
    """ss: _V of a sum of squares -> _V of rsqrtf(ss / K + eps): two fp32 roundings of the argument, RSQRT_ULP ulps (2 U32 each) of the function; d rs / d arg = rs / (2 arg)"""
    arg = ss.x / K + eps
    rs = arg.rsqrt()
    e_arg = ss.e / K + 2 * U32 * arg
    return G._V(rs, 0.5 * rs * e_arg / (arg - e_arg).clamp_min(1e-300) + 2 * RSQRT_ULP * U32 * rs)


def norm_prologue_bound(x, norm_w, eps, Wq, bias=None):
    """xn = rbf(w * rbf(x * rs)), rs = rsqrtf(mean x^2 + eps) with fp32 statistics; then the plain f32 projection of xn"""
    K = x.shape[1]
    xd = x.double()
    # sum of squares in fp32, in the documented orders: gvl_decode.hip adds 8 squares per lane, a 6-level wave sum and 3 levels of slice sums (18 roundings on any
    # path from a square to the total); gvl_elem.hip adds K / 256 chunks of 8 per thread, a 6-level wave sum and 3 more adds -- the deeper of the two, plus the square
    depth = K // 32 + 10
    ss = G._V((xd ** 2).sum(1, keepdim=True), depth * U32 * (xd ** 2).sum(1, keepdim=True))
    rs = _rstd(ss, K, eps)
    t = _round(G._V(xd * rs.x, xd.abs() * rs.e).f32())
    xn = _round(t.scale(norm_w.double()[None, :]))
    v = _acc(xn, Wq)
    if bias is not None:
        v = v.add(bias.double()[None, :])
    return v.x, v.e


def producer_bound(x, Wq, resid, bias=None):
    """h = bf16(resid + rbf(acc + bias)) and the sums of squares of the stored h per 16 columns -> (_V h, _V sq [batch, N / 16])"""
    v = _acc(G._V(x.double(), 0.0), Wq)
    if bias is not None:
        v = v.add(bias.double()[None, :])
    h = _round(_round(v).add(resid.double()))
    B, N = h.x.shape
    y2 = (h.x ** 2).view(B, N // 16, 16).sum(-1)
    e2 = (h.e * (2 * h.x.abs() + h.e)).view(B, N // 16, 16).sum(-1)
    return h, G._V(y2, e2 + 17 * U32 * (y2 + e2))


def consumer_bound(h, sq, Wf, eps):
    """out = rsqrtf(sum(sq) / K + eps) * (h Wf^T): h, sq = producer_bound's (the kernel reads ITS OWN h and sq, within those bounds of the reference's)"""
    K = Wf.shape[1]
    n = sq.x.shape[1]
    ss = G._V(sq.x.sum(1, keepdim=True), sq.e.sum(1, keepdim=True) + n * U32 * (sq.x + sq.e).sum(1, keepdim=True))
    rs = _rstd(ss, K, eps)
    v = G._mul(_acc(h, Wf), rs)
    return v.x, v.e


def rope_bound(x, Wq, geo, pos, tabs, switch):
    """the rotation with its three roundings, at each sequence's position and table set: -> (_V q [B, H, Dr], _V k [B, KV, Dr], _V v [B, KV, Dr]).
    tabs = (cos_s, sin_s, cos_l, sin_l), f32 [max_pos, Dr / 2]: exact factors known to both sides"""
    H, KV, Dr, D = geo
    half = Dr // 2
    B = x.shape[0]
    a = _acc(G._V(x.double(), 0.0), Wq)
    y = G._V(a.x.view(B, H + 2 * KV, Dr), a.e.view(B, H + 2 * KV, Dr))
    lng = (pos.long() + 1 > switch)[:, None]
    co = torch.where(lng, tabs[2][pos.long()], tabs[0][pos.long()]).double()[:, None, :]
    si = torch.where(lng, tabs[3][pos.long()], tabs[1][pos.long()]).double()[:, None, :]
    r = _round(G._V(y.x[:, :H + KV], y.e[:, :H + KV]))
    x1, x2 = G._V(r.x[..., :half], r.e[..., :half]), G._V(r.x[..., half:], r.e[..., half:])
    def rot(p, q, sgn):                                     # bf16(rbf(p c) + rbf(sgn q s))
        u, w = _round(p.scale(co)), _round(q.scale(sgn * si))
        return _round(G._V(u.x + w.x, u.e + w.e).f32())
    o1, o2 = rot(x1, x2, -1.0), rot(x2, x1, 1.0)
    qk = G._V(torch.cat([o1.x, o2.x], -1), torch.cat([o1.e, o2.e], -1))
    v = _round(G._V(y.x[:, H + KV:], y.e[:, H + KV:]))
    return G._V(qk.x[:, :H], qk.e[:, :H]), G._V(qk.x[:, H:], qk.e[:, H:]), v


def longrope_tables(max_pos, Dr, theta=10000.0, seed=0):
    """LongRoPE-like tables (Phi-3.5 style): per-frequency rescale factors, short near 1, long up to 64, and the attention factor on cos / sin; f32, rounded
    to bf16 values as the library's tables are"""
    half = Dr // 2
    g = torch.Generator().manual_seed(77 + seed)
    inv = theta ** (-torch.arange(half, dtype=torch.float64) * 2 / Dr)
    short = 1.0 + 0.1 * torch.rand(half, generator=g, dtype=torch.float64)
    long_ = 1.0 + 63.0 * (torch.arange(half, dtype=torch.float64) / half) ** 2
    p = torch.arange(max_pos, dtype=torch.float64)[:, None]
    mk = lambda fac, m: ((torch.cos(p * inv / fac) * m).float().to(bf).float(), (torch.sin(p * inv / fac) * m).float().to(bf).float())
    (cs, ss), (cl, sl) = mk(short, 1.0), mk(long_, 1.19)
    return cs, ss, cl, sl


def max_ratio(got, ref, bound):
    """-> (largest |got - ref| / bound, number of elements outside the bound); NaN / inf in got count as outside"""
    g = got.double()
    err = (g - ref).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max()), int((err > bound).sum())


# ---- the quantisers' edge set (shared by the CPU test of the restatements and the GPU test of the kernels) --------------------------------------------------
def all_bf16_upto(limit):
    """every finite bf16 value with |v| <= limit, both signs, both zeros (float32 tensor)"""
    bits = torch.arange(0, 0x7F80, dtype=torch.int32)
    v = (bits << 16).view(torch.float32)
    v = v[v <= limit]
    return torch.cat([v, -v])


def fp8_edge_rows(K=512):
    """rows for the three scales 2^-12, 1, 2^12 holding every bf16 pattern in range, plus: a maximum of exactly 448 * 2^k with its two bf16 neighbours (446, 450) and
    the same one binade down (223, 224, 225: the other side of the fr == 0.5 decision), an all-zero row, a row of negative zeros"""
    rows = []
    for k in (-12, 0, 12):
        top = 448.0 * 2.0 ** k
        vals = all_bf16_upto(top)
        per = K - 1
        for i in range(0, vals.numel(), per):
            r = torch.zeros(K)
            chunk = vals[i:i + per]
            r[:chunk.numel()] = chunk
            r[K - 1] = top if (i // per) % 2 == 0 else -top
            rows.append(r)
        u = 2.0 ** k                                        # bf16 spacing is 2 u at 448 u (in [256, 512) u) and u at 224 u: the maxima 446 / 448 / 450 and 223 / 224 / 225 u
        for mx in (top, top + 2 * u, top - 2 * u, top / 2, top / 2 + u, top / 2 - u):
            r = torch.linspace(-1, 1, K) * mx
            r[7] = -mx
            rows.append(r)
    rows.append(torch.zeros(K))
    rows.append(-torch.zeros(K))
    return torch.stack(rows).to(bf)


def mxfp4_edge_rows(K=1024):
    """blocks of 32 holding: every E2M1 tie value (and its bf16 neighbours) at several block scales with both signs; every bf16 pattern within a block's range
    (blocks whose maximum pins the scale); an all-zero block, a block of negative zeros, blocks of tiny values whose maximum has an exponent field of 0 .. 3"""
    blocks = []
    for e in (-120, -9, 0, 1, 7, 100):
        X = 2.0 ** e
        pts = []
        for tie in E2M1_TIES.tolist() + E2M1.tolist():
            for d in (-2.0 ** -8, 0.0, 2.0 ** -7):
                pts.append(tie * (1 + d) * X)
        pts = torch.tensor(pts, dtype=torch.float64)
        pts = torch.cat([pts, -pts]).float()
        for mx in (4.0, 6.0, 7.96875, -5.0):
            for i in range(0, pts.numel(), 31):
                b = torch.zeros(32)
                ch = pts[i:i + 31]
                b[:ch.numel()] = ch
                b[31] = mx * X
                blocks.append(b)
    vals = all_bf16_upto(7.96875)                           # every pattern under a block maximum in [4, 8): scale 1
    vals = vals[vals.abs() >= 2.0 ** -20]                   # (below: far under the first tie, covered by the tiny blocks)
    for i in range(0, vals.numel(), 31):
        b = torch.zeros(32)
        ch = vals[i:i + 31]
        b[:ch.numel()] = ch
        b[31] = 6.0 if (i // 31) % 2 else -4.0
        blocks.append(b)
    blocks.append(torch.zeros(32))
    blocks.append(-torch.zeros(32))
    for field in (0, 1, 2, 3, 4):                           # maxima with an fp32 exponent field 0 (bf16 sub-normal) .. 4
        for mant in (0, 0x40, 0x7F):
            top = torch.tensor([(field << 7 | mant) << 16 if field else (mant or 1) << 16], dtype=torch.int32).view(torch.float32)
            b = torch.linspace(-1, 1, 32) * top
            b[5] = top
            blocks.append(b)
    pad = (-len(blocks)) % (K // 32)
    blocks += [torch.zeros(32)] * pad
    return torch.stack(blocks).view(-1, K).to(bf)
