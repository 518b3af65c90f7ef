"""Independent reference for the qkv_post family (gvl_elem.hip: qkv_post_kernel, v_transpose_kernel, qkv_post_ext_kernel, v_transpose_ext_kernel, reached one launch at a
time through gvl_op_qkv_post) -- plain numpy, no GPU needed, no code shared with the kernels, with decode_proj_ref's RoPE or with torch's bf16 conversion.

What a launch must do is restated from the contract of gvl_qkv_post in include/gvl.h, per member (sequence) u with S_u new rows at positions pos0_u + i:
  Q    [H][S_u][D] at element row0_u H D;  K  slot p % 64 of page table_u[p / 64];  V^T  whole pages table_u[pos0_u / 64 + t], slots of tokens >= S_u zero;  the pad
       columns / rows Dr .. D - 1 zero, but 1.0 in K column Dr (k_ones) and in every slot of V^T row Dr (ones_row);  q_rs: rs of q stored, Q untouched.
  mode 0   copies.   mode 2   bf16(bf16(x cos) + bf16(+-partner sin)), emulated on integer bit patterns with round_bf16_bits (round to nearest even).   Both EXACT.
  mode 1   the full-width RMSNorm: judged by a per-element bound against float64, derived in norm_expect, no fitted factor.

emulate(case, mut=None) -> Images   every output buffer over its sentinel fill.  With mut=... one of MUTATIONS: a WRONG kernel (test_qkv_post_ref_cpu.py proves that
                                    mismatch() catches each on the list the GPU test runs).
expect(case)            -> Expect   the images of emulate for modes 0 / 2 (bit for bit); for mode 1 the float64 reference and bound of every normalised element, every other
                                    element (pads, V^T, sentinels) bit for bit.
mismatch(case, images, expect)      None, or the message the tests fail with: the count, the first (buffer, page / row, head, slot, d), the member and the source row.
cases()                 THE list test_gpu_qkv_post.py runs; build(spec) -> Case.
relocated_cases()       cases of that list to be run on pages whose element offsets inside the pools lie above 2^31 (one above 2^30): build(spec, first_page, n_pages) names
                        the pages first_page + (the same permutation) in caller-owned pools; the Images hold those pages only (image index = page - first_page), and
                        what a wrong kernel writes anywhere else is kept sparsely (Images.stray).  Expectations do not depend on first_page.

Inputs are hashed bf16 bit patterns (data_bits): modes 0 / 2 normal values 2^-30 ... 2^30 of both signs plus signed zeros, no subnormal, inf or NaN, hashed per (row, column) so
that a misplaced 16-byte chunk cannot equal the right one; mode 1 2^-4 ... 2^4.  cos / sin are hashed per (pos, j) over +-[1/4, 2) -- not a rotation: a wrong position
or a wrong j is a wrong number.  The qkv matrix is the prefix of an allocation whose following 64 rows (and whose columns behind the row, where ld is padded) are NaN.
The sentinel of every output is a NaN pattern no bf16 arithmetic on this data produces (0x7FA5), so an unwritten element can never pass for a written one.
"""
import numpy as np

from kv_page_ref import PAGE_MUTATIONS, POOL_ELEMS, first_page_above, wrap_page_offset

U32 = 2.0 ** -24                    # unit roundoff of fp32
RSQRT_REL = 2.0 ** -23              # HIP math API: rsqrtf, maximum error 1 ulp -- at most 2^-23 relative
SENT = 0x7FA5                       # bf16 NaN with a payload: what every output element holds before a launch
SENT_F32 = 0x7FA55A5A               # the same for q_rs
NAN_BITS = 0x7FC0
ONE = 0x3F80
GUARD = 4096                        # sentinel elements behind Q: 32 guard rows at D = 128 (the pools carry whole pages no table names instead)
TAIL_ROWS = 64
MUTATIONS = ("rope_sign", "partner_same_half", "cos_stride_Dr", "pos_plus_1", "slot_ignores_pos0", "one_rounding", "neighbour_table", "member_off_by_one", "q_row0_dropped",
             "pad_not_zeroed", "k_ones_missing", "k_ones_col_plus_1", "ones_row_missing", "v_tail_not_zeroed", "v_ext_tile_at_64t", "q_rs_writes_Q", "rms_per_head")
MUTATIONS += PAGE_MUTATIONS         # a page's base address formed in 32 bits (kv_page_ref.wrap_page_offset): the identity on cases(), wrong on relocated_cases()
GEOS = ((4, 4, 64, 64), (6, 2, 80, 96), (2, 2, 128, 128), (8, 1, 32, 64), (3, 3, 16, 64))          # every mode
GEO_IV2, GEO_WIDE = (4, 4, 88, 96), (13, 13, 128, 128)                                             # modes 0 / 1: in_regs (44 chunks) with and without q_rs;  mode 1: 208 chunks, streaming
LENS = (1, 3, 4, 5, 63, 64, 65, 130)
GROUPS = ((65,), (3,), (3, 65), (64, 130), (1, 1, 2, 3, 64, 65, 130, 1), (130, 1, 65, 2, 1, 3, 64, 1))
# (1, 1, 2, ...): the 4-row block 0 holds members 0, 1 and 2, block 1 members 3 and 4; member 5 ends at row 136, a block boundary.  (64, 130): member 0 ends on one.
EXT_POS0 = ((0, 64, 128, 64, 0, 128, 64, 0), (0,) * 8, (128, 0, 64, 0, 128, 64, 0, 128))


# ---- bf16 on bit patterns ----------------------------------------------------------------------------------------------------------------------------------------------
def f32_of_bits(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def round_bf16_bits(x):
    """float32 -> bf16 bit patterns, round to nearest, ties to even (finite input)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def round_bf16_f64(t):
    """float64 -> the nearest number with an 8-bit significand (ties to even), as float64; normal range only"""
    m, e = np.frexp(t)
    return np.ldexp(np.rint(m * 256.0) / 256.0, e)


def ulp_bf16(x):
    """spacing of the bf16 numbers in the binade of |x| (float64)"""
    _, e = np.frexp(np.abs(x))
    return np.ldexp(1.0, e - 8)


def _mix(x):
    x = np.asarray(x, dtype=np.int64)
    x = (x ^ (x >> 15)) * 0x2C1B3C6D % (1 << 31)
    x = (x ^ (x >> 12)) * 0x297A2D39 % (1 << 31)
    return x ^ (x >> 15)


def data_bits(rows, cols, seed, narrow):
    """uint16 [rows, cols]: sign | exponent | 7 mantissa bits hashed per (row, column); narrow: 2^-4 ... 2^4 without zeros, else 2^-30 ... 2^30 and one signed zero in 37"""
    r, c = np.arange(rows, dtype=np.int64)[:, None], np.arange(cols, dtype=np.int64)[None, :]
    h = _mix(r * 1000003 + c * 40503 + seed * 7919 + 1)
    g = _mix(h + c * 97 + 5)
    ex = 123 + g % 9 if narrow else 97 + g % 61
    bits = ((h >> 20) & 1) << 15 | ex << 7 | (h >> 8) & 127
    if not narrow:
        bits = np.where((g >> 9) % 37 == 0, ((h >> 20) & 1) << 15, bits)
    return bits.astype(np.uint16)


def trig_tables(max_pos, half, seed):
    """-> cos, sin float32 [max_pos, half]: bf16-representable values +-(1 + m / 128) 2^e, e in -2 .. 0, hashed per (pos, j)"""
    p, j = np.arange(max_pos, dtype=np.int64)[:, None], np.arange(half, dtype=np.int64)[None, :]
    out = []
    for k in (11, 23):
        h = _mix(p * 65599 + j * 8191 + seed * 131 + k)
        out.append(f32_of_bits((((h >> 20) & 1) << 15 | (125 + h % 3) << 7 | (h >> 8) & 127).astype(np.uint16)))
    return out[0], out[1]


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------------------------------
class Member:
    def __init__(self, row0, rows, pos0, table, b=0):
        self.row0, self.rows, self.pos0, self.table, self.b = row0, rows, pos0, [int(x) for x in table], b


class Case:
    """form: "single" (vl_n = 0: B sequences of S rows at pos0; table None = implicit pages), "ragged", "ext".  members: what the launch means, one per sequence."""

    def __str__(self):
        s = self.spec
        return (f"{s['form']} mode {s['mode']} H{self.H}/{self.KV} Dr{self.Dr} D{self.D} " + (f"B{s['B']} S{s['S']} pos0 {s['pos0']} table {s['table']}" if s["form"] == "single"
                else f"members {s['lens']} pos0 {s.get('vl_pos0')}") + f" vt {int(self.vt)} k_ones {self.k_ones} ones_row {self.ones_row} q_rs {int(self.q_rs)} ld {self.ld}")


def build(spec, first_page=0, n_pages=None):
    """spec: dict(form, geo, mode, seed, and -- single: B, S, pos0, table (bool) -- ragged / ext: lens, vl_pos0) + vt, k_ones, ones_row, q_rs, ld_pad.
    first_page, n_pages: the case's pages are first_page + (the same permutation) in caller-owned pools of n_pages pages (default: pools that end behind the case's
    pages, as before).  c.page0 = first_page, c.win = the pages the case lays out; Images hold the pages page0 .. page0 + win - 1, image index = page - page0."""
    c = Case()
    c.spec = dict(spec)
    c.H, c.KV, c.Dr, c.D = spec["geo"]
    c.mode, c.form, c.seed = spec["mode"], spec["form"], spec["seed"]
    c.vt, c.k_ones, c.ones_row, c.q_rs = bool(spec.get("vt", True)), int(spec.get("k_ones", 0)), int(spec.get("ones_row", 0)), bool(spec.get("q_rs", False))
    c.width = (c.H + 2 * c.KV) * c.Dr
    c.ld = c.width + spec.get("ld_pad", 0)
    c.eps = 1e-6
    rng = np.random.RandomState(1000 + c.seed)
    c.members, c.block_table, c.max_pages = [], None, 0
    if c.form == "single":
        B, S, pos0 = spec["B"], spec["S"], spec["pos0"]
        c.B, c.S, c.pos0, c.rows = B, S, pos0, B * S
        nt, need = (S + 63) // 64, (pos0 + S + 63) // 64
        if spec["table"]:
            c.max_pages = need + 2                                   # max_pages > the tiles a sequence has
            c.win = B * need + 3                                     # pages no table names
            c.n_pages = n_pages or first_page + c.win
            perm = rng.permutation(c.win)
            c.block_table = np.full((B, c.max_pages), c.n_pages + 7, dtype=np.int32)     # entries behind a sequence's tiles are never read
            c.block_table[:, :need] = first_page + perm[:B * need].reshape(B, need)
            c.block_table[:, :pos0 // 64] = -3                       # ... nor the prefix pages this launch does not write
            if spec.get("identity"):
                c.win = B * nt + 3
                c.n_pages = n_pages or first_page + c.win
                c.block_table = np.full((B, c.max_pages), c.n_pages + 7, dtype=np.int32)
                c.block_table[:, :nt] = first_page + np.arange(B * nt).reshape(B, nt)
            tabs = [c.block_table[b] for b in range(B)]
        else:
            assert pos0 == 0 and first_page == 0 and n_pages is None, "implicit pages start at page 0"
            c.win = c.n_pages = B * nt + 3
            tabs = [np.arange(b * nt, (b + 1) * nt) for b in range(B)]
        c.members = [Member(b * S, S, pos0, tabs[b], b) for b in range(B)]
    else:
        lens = list(spec["lens"])
        p0 = [int(x) for x in spec["vl_pos0"][:len(lens)]] if c.form == "ext" else [0] * len(lens)
        c.B, c.S, c.pos0, c.rows = 1, max(lens), 0, sum(lens)
        need = [(p + s + 63) // 64 for p, s in zip(p0, lens)]
        new = [n - p // 64 for n, p in zip(need, p0)]
        c.win = sum(new) + 5
        c.n_pages = n_pages or first_page + c.win
        perm = [first_page + int(x) for x in rng.permutation(c.win)[:sum(new)]]
        r0 = 0
        for u, s in enumerate(lens):
            tab = np.full(need[u] + 1 + u % 2, c.n_pages + 7, dtype=np.int32)
            tab[:p0[u] // 64] = -3
            tab[p0[u] // 64:need[u]] = [perm.pop() for _ in range(new[u])]
            c.members.append(Member(r0, s, p0[u], tab))
            r0 += s
    c.max_pos = max(m.pos0 + m.rows for m in c.members) + 2
    c.qkv = np.full((c.rows + TAIL_ROWS, c.ld), NAN_BITS, dtype=np.uint16)
    c.qkv[:c.rows, :c.width] = data_bits(c.rows, c.width, c.seed, narrow=c.mode == 1)
    c.cos, c.sin = trig_tables(c.max_pos, c.Dr // 2, c.seed) if c.mode == 2 else (None, None)
    c.qn = data_bits(1, c.H * c.Dr, c.seed + 101, True)[0] if c.mode == 1 else None
    c.kn = data_bits(1, c.KV * c.Dr, c.seed + 202, True)[0] if c.mode == 1 else None
    c.q_elems = c.rows * c.H * c.D
    c.page0, c.page_elems = first_page, c.KV * 64 * c.D
    assert c.page0 + c.win <= c.n_pages
    return c


def single_launch_of(c, u):
    """member u of a ragged / ext case as a single-sequence case on the same table: spec-less Case sharing c's data (rows of qkv, tables, pools' size)"""
    m = c.members[u]
    d = Case()
    d.__dict__.update(c.__dict__)
    d.spec = dict(form="single", mode=c.mode, B=1, S=m.rows, pos0=m.pos0, table=True)
    d.form, d.B, d.S, d.pos0, d.rows = "single", 1, m.rows, m.pos0, m.rows
    d.qkv = np.concatenate([c.qkv[m.row0:m.row0 + m.rows], np.full((TAIL_ROWS, c.ld), NAN_BITS, dtype=np.uint16)])
    d.block_table, d.max_pages = np.asarray(m.table, dtype=np.int32)[None, :].copy(), len(m.table)
    d.members = [Member(0, m.rows, m.pos0, m.table)]
    d.q_elems = m.rows * c.H * c.D
    return d


class Images:
    def __init__(self, c):
        self.Q = np.full(c.q_elems + GUARD, SENT, dtype=np.uint16)
        self.Kt = np.full((c.win, c.KV, 64, c.D), SENT, dtype=np.uint16)     # pages c.page0 .. c.page0 + c.win - 1 of the pool
        self.Vt = np.full((c.win, c.KV, c.D, 64), SENT, dtype=np.uint16)
        self.q_rs = np.full(c.rows + 64, SENT_F32, dtype=np.uint32)          # float32 bit patterns
        self.stray = {}                                                      # (buffer, element offset in the pool) -> what was written OUTSIDE those pages: a sparse pool


# ---- the pass in plain numpy -------------------------------------------------------------------------------------------------------------------------------------------
def rope(xb, pos, cos, sin, mut=None):
    """xb uint16 [S, heads, Dr], pos int [S] -> uint16 [S, heads, Dr]: bf16(bf16(x cos[pos]) + bf16(+-partner sin[pos])), the partner Dr / 2 away, minus in the first half"""
    S, _, Dr = xb.shape
    half = Dr // 2
    x = f32_of_bits(xb)
    j = np.arange(Dr) % half
    first = np.arange(Dr) < half
    partner = np.where(first, np.arange(Dr) + half, np.arange(Dr) - half)
    if mut == "partner_same_half":
        partner = np.arange(Dr)
    if mut == "pos_plus_1":
        pos = pos + 1
    if mut == "cos_stride_Dr":                                               # flat index pos Dr + j into the [max_pos][half] table
        flat = (pos[:, None] * Dr + j[None, :]) % cos.size
        cc, ss = cos.reshape(-1)[flat], sin.reshape(-1)[flat]
    else:
        cc, ss = cos[pos][:, j], sin[pos][:, j]                              # [S, Dr]
    sg = np.where(first, np.float32(-1), np.float32(1))
    if mut == "rope_sign":
        sg = -sg
    a = x * cc[:, None, :]                                                    # 8 x 8 significand bits: exact in fp32
    b = (sg[None, None, :] * x[:, :, partner]) * ss[:, None, :]
    if mut == "one_rounding":
        return round_bf16_bits(a + b)
    return round_bf16_bits(f32_of_bits(round_bf16_bits(a)) + f32_of_bits(round_bf16_bits(b)))


def rope_f64(xb, pos, cos, sin):
    """the same formula in float64 with NO rounding step -> (y, |x cos|, |partner sin|): the anchor of the emulation (test_qkv_post_ref_cpu.py)"""
    Dr = xb.shape[-1]
    half = Dr // 2
    x = f32_of_bits(xb).astype(np.float64)
    c, s = cos[pos].astype(np.float64)[:, None, :], sin[pos].astype(np.float64)[:, None, :]
    x1, x2 = x[..., :half], x[..., half:]
    y = np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    return y, np.concatenate([np.abs(x1 * c), np.abs(x2 * c)], -1), np.concatenate([np.abs(x2 * s), np.abs(x1 * s)], -1)


def norm_f32(xb, wb, eps, per_head=0):
    """mode 1 in fp32: xb uint16 [S, n] (the full q or k width), wb uint16 [n] -> (uint16 [S, n], rs float32 [S])"""
    x = f32_of_bits(xb)
    n = x.shape[1]
    if per_head:                                                              # mutation: the statistics of one head instead of the full width
        sq = np.repeat((x * x).reshape(x.shape[0], -1, per_head).sum(-1, dtype=np.float32), per_head, 1) / np.float32(per_head)
    else:
        sq = ((x * x).sum(1, dtype=np.float32) / np.float32(n))[:, None]
    rs = (np.float32(1) / np.sqrt(sq + np.float32(eps), dtype=np.float32)).astype(np.float32)
    inner = f32_of_bits(round_bf16_bits(x * rs))
    return round_bf16_bits(f32_of_bits(wb)[None, :] * inner), rs[:, 0]


def emulate(c, mut=None):
    assert mut is None or mut in MUTATIONS
    H, KV, Dr, D = c.H, c.KV, c.Dr, c.D
    im = Images(c)
    ragged = c.form != "single"
    n = len(c.members)
    p0 = c.page0
    for u, m in enumerate(c.members):
        S, r0 = m.rows, m.row0
        x = c.qkv[r0:r0 + S, :c.width]
        q, k, v = x[:, :H * Dr], x[:, H * Dr:(H + KV) * Dr], x[:, (H + KV) * Dr:]
        i = np.arange(S)
        pos = m.pos0 + i
        if c.mode == 2:
            qo, ko = (rope(t.reshape(S, -1, Dr), pos, c.cos, c.sin, mut).reshape(S, -1) for t in (q, k))
        elif c.mode == 1:
            ph = Dr if mut == "rms_per_head" else 0
            (qo, rs), (ko, _) = norm_f32(q, c.qn, c.eps, ph), norm_f32(k, c.kn, c.eps, ph)
            if c.q_rs:
                im.q_rs[r0:r0 + S] = rs.view(np.uint32)
        else:
            qo, ko = q, k
        rows_ok = np.ones(S, dtype=bool)
        if mut == "member_off_by_one" and ragged and u > 0:                  # the member's first row is taken for the previous member's row S_(u-1): its own places stay unwritten
            rows_ok[0] = False
        # Q
        if not c.q_rs or mut == "q_rs_writes_Q":
            q0 = 0 if (mut == "q_row0_dropped" and ragged) else r0 * H * D
            Qm = im.Q[q0:q0 + S * H * D].reshape(H, S, D)
            Qm[:, rows_ok, :Dr] = qo.reshape(S, H, Dr).transpose(1, 0, 2)[:, rows_ok]
            if mut != "pad_not_zeroed":
                Qm[:, rows_ok, Dr:] = 0
        # K
        kpos = i if mut == "slot_ignores_pos0" else pos
        table = c.members[(u + 1) % n].table if mut == "neighbour_table" else m.table
        tile = kpos >> 6
        if mut in ("neighbour_table", "slot_ignores_pos0"):                  # a wrong table entry may be no page at all: that write is dropped here (the GPU would fault)
            tile = np.minimum(tile, len(table) - 1)
            page = np.asarray(table)[tile]
            rows_ok = rows_ok & (page >= p0) & (page < p0 + c.win)
        page, slot = np.asarray(table)[tile] - p0, kpos & 63
        page, slot, kk = page[rows_ok], slot[rows_ok], ko.reshape(S, KV, Dr)[rows_ok]
        g = np.arange(KV)[None, :]
        im.Kt[page[:, None], g, slot[:, None], :Dr] = kk
        if D > Dr:
            if mut != "pad_not_zeroed":
                im.Kt[page[:, None], g, slot[:, None], Dr:] = 0
            if c.k_ones and mut != "k_ones_missing":
                col = Dr + 1 if mut == "k_ones_col_plus_1" else Dr
                if mut == "k_ones_col_plus_1":
                    im.Kt[page[:, None], g, slot[:, None], Dr] = 0
                im.Kt[page[:, None], g, slot[:, None], col] = ONE
        if mut == "member_off_by_one" and ragged and u > 0:                  # ... and its key lands behind the previous member's last key
            pm = c.members[u - 1]
            pp = pm.pos0 + pm.rows
            if pp >> 6 < len(pm.table) and p0 <= pm.table[pp >> 6] < p0 + c.win:
                im.Kt[pm.table[pp >> 6] - p0, :, pp & 63, :Dr] = ko.reshape(S, KV, Dr)[0]
        # V^T: whole pages
        if c.vt:
            for t in range((S + 63) // 64):
                tt = t if (mut == "v_ext_tile_at_64t" and c.form == "ext") else (m.pos0 >> 6) + t
                pg = m.table[tt] - p0
                if not 0 <= pg < c.win:                                      # only under the mutation: no page at all, the write is dropped here
                    continue
                blk = np.zeros((KV, D, 64), dtype=np.uint16)
                cnt = min(64, S - t * 64)
                take = 64 if mut == "v_tail_not_zeroed" else cnt             # the mutation reads on into the next member's rows / the NaN tail
                src = c.qkv[r0 + t * 64:r0 + t * 64 + take, (H + KV) * Dr:c.width]
                blk[:, :Dr, :take] = src.reshape(take, KV, Dr).transpose(1, 2, 0)
                if c.ones_row and mut != "ones_row_missing":
                    blk[:, Dr, :] = ONE
                im.Vt[pg] = blk
    if mut in PAGE_MUTATIONS:                                                # every written page lands where the wrapped offset points: outside the case's pages
        for name in ("Kt", "Vt"):
            img = getattr(im, name)
            for w in np.nonzero((img != SENT).reshape(c.win, -1).any(1))[0]:
                off = (p0 + int(w)) * c.page_elems
                if wrap_page_offset(off, mut) != off:
                    im.stray[(name, wrap_page_offset(off, mut))] = img[w].copy()
                    img[w] = SENT
    return im


# ---- mode 1: float64 reference and derived bound -----------------------------------------------------------------------------------------------------------------------
def norm_expect(xb, wb, eps):
    """-> (ref, bound, rs, rs_bound), float64: xb uint16 [S, n], wb uint16 [n].

    The kernel forms, in fp32, ss = the sum of the row's n squares (each exact: 8 x 8 significand bits) in some order, m~ = ss / n + eps, rs~ = rsqrtf(m~), and stores
    bf16(w * bf16(x * rs~)).  With u = 2^-24:
      ss        n - 1 additions of non-negative terms in any order: relative error <= g = n u / (1 - n u)
      m~        one division and one addition of positive terms: (1 + g)(1 + u)^2 - 1 = dm relative
      rs~       |(1 + e)^-1/2 - 1| <= |e| for |e| < 1/2, and rsqrtf is good to 1 ulp (<= 2^-23 relative): drs = (1 + dm)(1 + 2^-23) - 1; this is q_rs's own bound, rs drs
      x * rs~   one fp32 rounding: t~ = t (1 + dt), |dt| <= (1 + drs)(1 + u) - 1, t = x rs in float64
      inner     rounding to bf16 is monotone, so bf16(t~) lies between bf16(t (1 - dt)) and bf16(t (1 + dt)): it equals bf16(t) unless a rounding boundary lies that
                close to t, and is then ONE neighbour away -- flip = the larger distance of the two ends from bf16(t), zero for almost every element
      w * inner 8 x 8 bits, exact in fp32; the store rounds to nearest: half a bf16 ulp at the largest magnitude the product can have
    ref = w bf16(t),  bound = |w| flip + ulp_bf16(|w| (|bf16(t)| + flip)) / 2."""
    x, w = f32_of_bits(xb).astype(np.float64), f32_of_bits(wb).astype(np.float64)[None, :]
    n = x.shape[1]
    m = (x * x).sum(1) / n + float(np.float32(eps))
    rs = m ** -0.5
    g = n * U32 / (1 - n * U32)
    dm = (1 + g) * (1 + U32) ** 2 - 1
    drs = (1 + dm) * (1 + RSQRT_REL) - 1
    dt = (1 + drs) * (1 + U32) - 1
    t = x * rs[:, None]
    inner = round_bf16_f64(t)
    flip = np.maximum(np.abs(round_bf16_f64(t * (1 - dt)) - inner), np.abs(round_bf16_f64(t * (1 + dt)) - inner))
    ref = w * inner
    bound = np.abs(w) * flip + 0.5 * ulp_bf16(np.abs(w) * (np.abs(inner) + flip))
    return ref, bound, rs, rs * drs


class Expect:
    """bits: the Images every exact element must equal; for mode 1 additionally, per buffer name, (index arrays, ref, bound) of the elements judged by a bound -- those
    elements are excluded from the bit comparison"""

    def __init__(self, images):
        self.bits, self.bounded = images, {}


def expect(c):
    e = Expect(emulate(c))
    if c.mode != 1:
        return e
    H, KV, Dr, D = c.H, c.KV, c.Dr, c.D
    qi, qr, qb, ki, kr, kb, ri, rr, rb = ([] for _ in range(9))
    for m in c.members:
        S, r0 = m.rows, m.row0
        x = c.qkv[r0:r0 + S, :c.width]
        ref, bound, rs, rsb = norm_expect(x[:, :H * Dr], c.qn, c.eps)
        if c.q_rs:
            ri.append(r0 + np.arange(S)), rr.append(rs), rb.append(rsb)
        else:
            idx = r0 * H * D + (np.arange(H)[None, :, None] * S + np.arange(S)[:, None, None]) * D + np.arange(Dr)[None, None, :]       # [S, H, Dr]
            qi.append(idx.reshape(-1)), qr.append(ref.reshape(-1)), qb.append(bound.reshape(-1))
        ref, bound, _, _ = norm_expect(x[:, H * Dr:(H + KV) * Dr], c.kn, c.eps)
        pos = m.pos0 + np.arange(S)
        page, slot = np.asarray(m.table)[pos >> 6], pos & 63
        idx = (((page - c.page0)[:, None, None] * KV + np.arange(KV)[None, :, None]) * 64 + slot[:, None, None]) * D + np.arange(Dr)[None, None, :]
        ki.append(idx.reshape(-1)), kr.append(ref.reshape(-1)), kb.append(bound.reshape(-1))
    cat = lambda a: np.concatenate(a) if a else np.zeros(0)
    e.bounded = {"Q": (cat(qi).astype(np.int64), cat(qr), cat(qb)), "Kt": (cat(ki).astype(np.int64), cat(kr), cat(kb)), "q_rs": (cat(ri).astype(np.int64), cat(rr), cat(rb))}
    return e


# ---- the comparison of both tests --------------------------------------------------------------------------------------------------------------------------------------
def locate(c, name, flat):
    """where element `flat` of buffer `name` belongs: (page / row, head, slot, d), the member that owns it and the qkv row it comes from"""
    H, KV, Dr, D = c.H, c.KV, c.Dr, c.D
    if name == "q_rs":
        u = [k for k, m in enumerate(c.members) if m.row0 <= flat < m.row0 + m.rows]
        return f"(q_rs, row {flat}): member {u[0] if u else None}, source row {flat if u else None}"
    if name == "Q":
        if flat >= c.q_elems:
            return f"(Q, guard element {flat - c.q_elems} behind the last row): nobody's"
        row_block, d = flat // D, flat % D
        for k, m in enumerate(c.members):
            lo = m.row0 * H
            if lo <= row_block < lo + m.rows * H:
                h, i = (row_block - lo) // m.rows, (row_block - lo) % m.rows
                return f"(Q, row {i} of member {k}, head {h}, d {d}): member {k}, source row {m.row0 + i}"
    page, rest = c.page0 + flat // (KV * 64 * D), flat % (KV * 64 * D)
    g, rest = rest // (64 * D), rest % (64 * D)
    slot, d = (rest // D, rest % D) if name == "Kt" else (rest % 64, rest // 64)
    for k, m in enumerate(c.members):
        for t in range(m.pos0 >> 6, (m.pos0 + m.rows + 63) >> 6):
            if m.table[t] == page:
                i = t * 64 + slot - m.pos0
                src = m.row0 + i if 0 <= i < m.rows else None
                return f"({name}, page {page} = tile {t} of member {k}, KV head {g}, slot {slot}, d {d}): member {k}, source row {src}"
    return f"({name}, page {page}, KV head {g}, slot {slot}, d {d}): a page no table of this launch names"


def mismatch(c, got, e, stats=None):
    """got: an Images-like object (numpy arrays of the same shapes / dtypes).  None when every exact element equals e.bits bit for bit and ZERO bounded elements lie outside
    their bound (a non-finite one always does); else the message.  stats (dict): the largest err / bound per buffer is recorded there."""
    msgs = []
    for name in ("Q", "Kt", "Vt", "q_rs"):
        g, x = getattr(got, name).reshape(-1), getattr(e.bits, name).reshape(-1)
        if g.shape != x.shape or g.dtype != x.dtype:
            return f"{c}: {name} has shape / dtype {g.shape} {g.dtype}, expected {x.shape} {x.dtype}"
        ne = g != x
        if name in e.bounded and e.bounded[name][0].size:
            idx, ref, bound = e.bounded[name]
            ne[idx] = False
            with np.errstate(invalid="ignore"):
                val = (g[idx].view(np.float32) if name == "q_rs" else f32_of_bits(g[idx])).astype(np.float64)
                err = np.where(np.isfinite(val), np.abs(val - ref), np.inf)
            if stats is not None:
                stats[name] = max(stats.get(name, 0.0), float((err / bound).max()))
            out = np.nonzero(err > bound)[0]
            if out.size:
                o = out[0]
                msgs.append(f"{name}: {out.size} of {idx.size} elements outside the bound (worst err / bound {float((err / bound).max()):.3g}); first {locate(c, name, int(idx[o]))} got "
                            f"{val[o]:.8g}, reference {ref[o]:.8g}, bound {bound[o]:.3g}")
        bad = np.nonzero(ne)[0]
        if bad.size:
            f = int(bad[0])
            msgs.append(f"{name}: {bad.size} of {g.size} elements differ; first {locate(c, name, f)} got 0x{int(g[f]):04x}, expected 0x{int(x[f]):04x}"
                        + (" (the sentinel: nobody may write here)" if int(x[f]) in (SENT, SENT_F32) else " (still the sentinel: not written)" if int(g[f]) in (SENT, SENT_F32) else ""))
    for (name, off), _ in sorted(getattr(got, "stray", {}).items())[:1]:
        msgs.append(f"{name}: {len(got.stray)} pages written outside pages {c.page0} .. {c.page0 + c.win - 1}; first at element offset {off} of the pool (the sentinel: nobody may write here)")
    return f"{c}: " + "; ".join(msgs) if msgs else None


# ---- THE list of test_gpu_qkv_post.py ----------------------------------------------------------------------------------------------------------------------------------
def cases():
    out, n = [], 0

    def flags(geo, mode, n, q_rs=False):
        pad = geo[3] > geo[2]
        return dict(k_ones=int(pad and (q_rs or n % 2 == 0)), ones_row=int(pad and n % 4 < 2), q_rs=q_rs, ld_pad=(0, 16)[n % 2])

    singles = [(g, m) for g in GEOS for m in (0, 1, 2)] + [(GEO_IV2, 0), (GEO_IV2, 1), (GEO_IV2, "q_rs"), (GEO_WIDE, 1)]
    for gi, (geo, mode) in enumerate(singles):
        q_rs, mode = mode == "q_rs", 1 if mode == "q_rs" else mode
        for si, S in enumerate(LENS):
            n += 1
            k = si + gi
            f = flags(geo, mode, n, q_rs)
            out.append(dict(form="single", geo=geo, mode=mode, seed=n, B=(1, 3)[k % 2], S=S, pos0=0, table=False, vt=True, **f))              # implicit pages
            novt = k % 4 == 3                                                                                                             # Vt NULL: K and Q only; pos0 need not be whole pages
            out.append(dict(form="single", geo=geo, mode=mode, seed=n + 500, B=(3, 1)[k % 2], S=S, pos0=(0, 64, 192)[k % 3] + (37 if novt and k % 8 == 3 else 0), table=True,
                            vt=not novt, **f))
    for gi, geo in enumerate(GEOS):
        for li, lens in enumerate(GROUPS):
            n += 1
            f = flags(geo, 2, n)
            out.append(dict(form="ragged", geo=geo, mode=2, seed=n, lens=lens, vl_pos0=None, vt=(gi + li) % 5 != 4, **f))
            for pi, p0 in enumerate(EXT_POS0):
                if pi == 2 and len(lens) < 8:
                    continue
                out.append(dict(form="ext", geo=geo, mode=2, seed=n + 700 + pi, lens=lens, vl_pos0=p0, vt=True, **f))
    return out


# ---- the relocated cases: the same launches on pages whose offsets inside the pool need more than 32 bits ----------------------------------------------------------------
def relocated_cases():
    """-> [(spec, k)]: specs TAKEN FROM cases() (no new shape), to be laid out from the first page at or above 2^k elements of a POOL_ELEMS pool (build_relocated).
    k = 31: every page offset is above 2^31 elements.  Between them: all four kernels (single with a table: qkv_post_kernel + v_transpose_kernel, also in their
    ragged form; extend: the two _ext kernels), modes 0 / 1 / 2, q_rs, Vt NULL, head dims 64, 128 and the padded 80 -> 96 and 88 -> 96 (page sizes that are not powers of
    two: a wrapped offset is not even page aligned).  k = 30: one more, byte offsets between 2^31 and 2^32."""
    sp = cases()

    def pick(**kw):
        test = kw.pop("test", lambda s: True)
        return next(s for s in sp if all(s.get(k) == v for k, v in kw.items()) and test(s))

    table = dict(form="single", table=True)
    out = [(pick(geo=GEOS[0], mode=0, S=65, vt=True, **table), 31),
           (pick(geo=GEOS[2], mode=2, S=65, vt=True, test=lambda s: s["pos0"] > 0, **table), 31),
           (pick(geo=GEOS[1], mode=2, S=130, vt=True, k_ones=1, ones_row=1, **table), 31),
           (pick(geo=GEO_IV2, mode=1, q_rs=False, S=65, vt=True, **table), 31),
           (pick(geo=GEO_IV2, mode=1, q_rs=True, S=130, vt=True, **table), 31),
           (pick(geo=GEOS[2], mode=0, vt=False, test=lambda s: s["pos0"] & 63, **table), 31),
           (pick(form="ragged", geo=GEOS[1], lens=GROUPS[4], vt=True), 31),
           (pick(form="ragged", geo=GEOS[2], lens=GROUPS[3], vt=True), 31),
           (pick(form="ext", geo=GEOS[2], lens=GROUPS[5], vl_pos0=EXT_POS0[2]), 31),
           (pick(form="ext", geo=GEOS[1], lens=GROUPS[2], vl_pos0=EXT_POS0[0]), 31),
           (pick(form="ext", geo=GEOS[0], lens=GROUPS[4], vl_pos0=EXT_POS0[0]), 30)]
    return out


def build_relocated(spec, k):
    """build(spec) with its pages from the first one at or above 2^k elements of a pool of POOL_ELEMS elements"""
    pe = spec["geo"][1] * 64 * spec["geo"][3]
    return build(spec, first_page=first_page_above(1 << k, pe), n_pages=POOL_ELEMS // pe)
