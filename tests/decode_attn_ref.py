"""Independent references for the two decode-attention kernels (decode_attn_kernel<D, 1, PH> and decode_attn_gqa_kernel<D, GM, STG> in gvl_attn.hip, reached through
gvl_op_decode_attention) -- no GPU needed to import or run this file.  Companion of attn_ref.py (same two families, same bound machinery).

Layout (include/gvl.h, restated here and not taken from the library): token t of sequence b is slot t % 64 of page tables[b][t // 64]; K pool [n_pages][KV][64][D] (key rows),
V^T pool [n_pages][KV][D][64]; q [B][H][D].  Every case lays its pages out itself through a NON-IDENTITY page table (a seeded permutation of the pool), and
  * the slots past pos in a sequence's last page hold decoys: K rows that would win (exact family: the code of a head's target; bounded family: a copy of the last real
    key), V columns with distinct finite values -- a mask that lets one key too many through changes the result;
  * the table entries beyond the sequence's pages point at a valid poison page of its own, full of such keys;
  * the V^T pad rows Dr <= d < D hold +-1e30 (large, finite), the K and q pad columns are zero, as the page writers leave them;
  * the pages of the pool that no sequence owns are NaN.

Split rule (gvl.h): n = ceil((pos + 1) / 64) pages, ns = min(nsplit, ceil(n / 4)) splits of pps = ceil(n / ns) pages; split c is pages [c pps, min((c + 1) pps, n)) and
may be empty; wave w of its block takes pages c pps + w, + 4, ...; one record [D acc, m, l] per split; the merge runs over the ns records in split order.

onehot_case(lens, H, KV, Dr, seed)   keys are the +-1 code of their token index XOR a per-(sequence, KV head) mask, the query of (b, h) is 64 x the code of its target, scale 1.0:
    integer scores, the target >= 128 raw = 184 log2 units ahead of every other key, so every other probability is exp2(<= -184) = 0 in fp32 in both kernels, the target's is
    exp2(0) = 1, l = 1, and the wave combine and the split merge multiply everything but the target's record by exp2(<= -184) = 0.  The output must equal the target's V row
    BIT FOR BIT.  V is attn_ref.onehot_v (normal values of 2^-100 .. 2^100: what ties before the target arrives is summed and must stay finite for the 0 that follows).
    Case.set_targets(t) installs one [B, H] set of targets (q, expect and the decoy K rows); target_sets(c) lists the sets a test goes through: per case every page of every
    sequence is some head's target, and so are key 0, the last real key, the one before it, and the first and last key of every split.
bounded_case(kind, lens, H, KV, Dr, seed) + elementwise_bound(case)   dense data with the mass where these kernels are fragile (KINDS), a float64 softmax on the bf16
    operands and a PER-ELEMENT bound that is derived, not measured -- see elementwise_bound.
emulate(case, shape, mut)   the kernels' documented arithmetic in plain torch, reading the pools through the tables: the CPU stand-in for a correct kernel and, with mut=...,
    for twelve wrong ones (test_decode_attn_ref_cpu.py).
exact_cases() / bounded_cases()   THE fixed lists test_gpu_decode_attn_exact.py runs (no full products); the CPU test runs the emulation over the same lists.
"""
import numpy as np
import torch

from gemm_ref import U32, _mix, bf16_ulp
from attn_ref import _code, onehot_v, _bits, SENT

bf = torch.bfloat16
LOG2E = np.float32(1.4426950408889634)
NSPLIT = 16                     # gvl_ctx::nsplit
VPAD = 1e30                     # V^T pad rows
DECOY_M, DECOY_L, DECOY_ACC = 1.0e4, 1.0, 7.0      # a stale partial record that would win any merge
GUARD_COLS = 8
KINDS = ("late_heavy", "early_heavy", "spike", "split_skew", "plain")
MUTATIONS = ("mask_plus", "mask_minus", "drop_second_trip", "pps_floor", "drop_last_split", "merge_all_nsplit", "no_rescale_wave", "no_rescale_merge", "gqa_mod",
             "table_identity", "table_of_seq0", "dout_stride")


def pad_head(dr):
    return 64 if dr <= 64 else 96 if dr <= 96 else 128


def split_rule(L, nsplit=NSPLIT):
    """context length (pos + 1) -> (pages, splits, pages per split)"""
    n = (L + 63) // 64
    ns = max(1, min(nsplit, (n + 3) // 4))
    return n, ns, (n + ns - 1) // ns


def place(L, t, nsplit=NSPLIT):
    """key t of a context of L -> (page, split, wave, trip)"""
    n, ns, pps = split_rule(L, nsplit)
    page = t // 64
    split = page // pps
    return page, split, (page - split * pps) % 4, (page - split * pps) // 4


class Case:
    """q bf16 [B, H, D]; Kt bf16 [n_pages, KV, 64, D]; Vt bf16 [n_pages, KV, D, 64]; tables int32 [B, table_stride]; pos int32 [B]; k / v: per sequence the logical
    operands [L, KV, Dr] (bf16); exact family: target [B, H], expect bf16 [B, H * Dr]"""

    def __init__(self, what, lens, H, KV, Dr, scale, nsplit, device):
        assert H % KV == 0
        self.what, self.lens, self.B, self.H, self.KV, self.Dr, self.D = what, [int(x) for x in lens], len(lens), H, KV, Dr, pad_head(Dr)
        self.scale, self.nsplit, self.device = float(scale), nsplit, device
        self.target = self.expect = None

    def set_targets(self, t):
        """exact family: install one [B, H] set of targets -- q, expect and the decoy K rows"""
        return _set_targets(self, t)

    def __str__(self):
        return f"{self.what} lens {self.lens} H{self.H}/{self.KV} D{self.Dr}"


def _lay_out(c, ks, vs, seed, share=None, pools=None, first_page=0):
    """pages, tables and pos of case c from the logical operands ks / vs (per sequence [L, KV, Dr]); share = (src, dst, pages): sequence dst owns no copy of its first
    `pages` pages, its table names src's (the operands of the two must agree there); pools = (Kt, Vt): write into these (uninitialised) pools, pages first_page ..."""
    dev, B, KV, Dr, D = c.device, c.B, c.KV, c.Dr, c.D
    npg = [(L + 63) // 64 for L in c.lens]
    c.table_stride = max(npg) + 3
    owned = [(b, i) for b in range(B) for i in range(npg[b]) if not (share and b == share[1] and i < share[2])] + [(b, -1) for b in range(B)]     # -1: the poison page
    T = len(owned)
    perm = np.random.RandomState(seed * 7 + 11).permutation(T)
    if T > 1 and bool((perm == np.arange(T)).all()):
        perm = np.roll(perm, 1)
    ident = {key: first_page + int(perm[i]) for i, key in enumerate(owned)}
    if share:
        src, dst, sp = share
        assert sp * 64 < min(c.lens[src], c.lens[dst]) and bool((ks[src][:sp * 64] == ks[dst][:sp * 64]).all()) and bool((_bits(vs[src][:sp * 64]) == _bits(vs[dst][:sp * 64])).all())
        for i in range(sp):
            ident[(dst, i)] = ident[(src, i)]
    if pools is None:
        c.n_pages = first_page + T + 2
        c.Kt = torch.full((c.n_pages, KV, 64, D), float("nan"), dtype=bf, device=dev)
        c.Vt = torch.full((c.n_pages, KV, D, 64), float("nan"), dtype=bf, device=dev)
    else:
        c.Kt, c.Vt = pools
        c.n_pages = c.Kt.shape[0]
        assert c.Kt.shape == (c.n_pages, KV, 64, D) and c.Vt.shape == (c.n_pages, KV, D, 64) and first_page + T <= c.n_pages
    tables = torch.zeros((B, c.table_stride), dtype=torch.int64)
    vdec = onehot_v(B, 128, KV, Dr, seed + 4099, dev)                            # [B, 128, KV, Dr]: decoy V, slots 0 .. 63 for the last page, 64 .. 127 for the poison page
    sign = torch.where(torch.arange(D - Dr, device=dev) % 2 == 0, VPAD, -VPAD).to(bf)[None, None, :, None]
    c.last_page, c.poison, c.rem = [], [], []
    for b in range(B):
        L, n = c.lens[b], npg[b]
        ids = torch.tensor([ident[(b, i)] for i in range(n)], dtype=torch.int64)
        tables[b, :n], tables[b, n:] = ids, ident[(b, -1)]
        rem = L - (n - 1) * 64
        k = torch.zeros((n * 64, KV, D), dtype=bf, device=dev)
        v = torch.zeros((n * 64, KV, Dr), dtype=bf, device=dev)
        k[:L, :, :Dr], v[:L] = ks[b].to(bf), vs[b]
        v[L:] = vdec[b, rem:64]
        ids_d = ids.to(dev)
        c.Kt[ids_d] = k.view(n, 64, KV, D).permute(0, 2, 1, 3)
        c.Vt[ids_d, :, :Dr] = v.view(n, 64, KV, Dr).permute(0, 2, 3, 1)
        c.Vt[ids_d, :, Dr:] = sign.expand(n, KV, D - Dr, 64)
        p = ident[(b, -1)]
        c.Kt[p] = 0
        c.Vt[p, :, :Dr] = vdec[b, 64:].permute(1, 2, 0)
        c.Vt[p, :, Dr:] = sign[0].expand(KV, D - Dr, 64)
        c.last_page.append(int(ids[-1])), c.poison.append(p), c.rem.append(rem)
    c.tables = tables.to(torch.int32).to(dev)
    c.pos = torch.tensor([L - 1 for L in c.lens], dtype=torch.int32, device=dev)
    c.k, c.v = [x.to(bf) for x in ks], vs
    return c


def _set_decoys(c, kdec):
    """kdec [B, KV, 64, Dr]: the K rows of the poison pages and of the slots past pos in the last pages"""
    for b in range(c.B):
        c.Kt[c.poison[b], :, :, :c.Dr] = kdec[b].to(bf)
        if c.rem[b] < 64:
            c.Kt[c.last_page[b], :, c.rem[b]:, :c.Dr] = kdec[b, :, c.rem[b]:].to(bf)


# ---- exact family --------------------------------------------------------------------------------------------------------------------------------------------------
def onehot_case(lens, H, KV, Dr, seed, share=None, nsplit=NSPLIT, device="cpu", pools=None, first_page=0):
    """see the module docstring; the case comes with the targets of target_sets(c)[0] installed"""
    c = Case("one-hot", lens, H, KV, Dr, 1.0, nsplit, device)
    c.nb = max(1, (max(c.lens) - 1).bit_length())
    assert c.nb <= 14 and c.nb <= Dr
    bm = torch.arange(c.B, dtype=torch.int64)
    if share:
        bm[share[1]] = share[0]                                                  # the two sequences of a shared prefix have the same keys there: the same mask
    c.mask = (_mix(bm[:, None] * 131 + torch.arange(KV, dtype=torch.int64)[None, :] * 17 + seed + 7) % (1 << c.nb)).to(device)                    # [B, KV]
    ks, vs = [], []
    for b, L in enumerate(c.lens):
        j = torch.arange(L, dtype=torch.int64, device=device)
        ks.append(_code(j[:, None] ^ c.mask[b][None, :], c.nb, Dr))              # [L, KV, Dr]
        vs.append(onehot_v(1, L, KV, Dr, seed + 977 * int(bm[b]), device)[0])
        if share and b == share[1]:
            vs[b] = torch.cat([vs[share[0]][:share[2] * 64], onehot_v(1, L, KV, Dr, seed + 977 * b + 3, device)[0][share[2] * 64:]])
    _lay_out(c, ks, vs, seed, share, pools, first_page)
    c.q = torch.zeros((c.B, H, c.D), dtype=bf, device=device)
    c.set_targets(target_sets(c)[0])
    return c


def _set_targets(c, t):
    t = t.to(c.device)
    assert t.shape == (c.B, c.H) and all(bool(((t[b] >= 0) & (t[b] < L)).all()) for b, L in enumerate(c.lens))
    rep = c.H // c.KV
    c.target = t
    qmask = c.mask.repeat_interleave(rep, dim=1)                                 # [B, H]: query head h belongs to KV head h // (H / KV)
    c.q[:, :, :c.Dr] = (64.0 * _code(t ^ qmask, c.nb, c.Dr)).to(bf)
    heads = torch.arange(c.KV, device=c.device)[:, None] * rep + torch.arange(64, device=c.device)[None, :] % rep                               # [KV, 64]: slot s of KV head g
    _set_decoys(c, _code(t[:, heads] ^ c.mask[:, :, None], c.nb, c.Dr))          # holds the winning code of head g rep + s % rep
    c.expect = torch.stack([c.v[b][t[b], torch.arange(c.H, device=c.device) // rep] for b in range(c.B)]).reshape(c.B, c.H * c.Dr).contiguous()
    return c


def wanted_keys(L, nsplit=NSPLIT, seed=0):
    """the keys of one sequence that must each be some head's target: one per page, key 0, the last two, the first and last key of every (non-empty) split"""
    n, ns, pps = split_rule(L, nsplit)
    keys = [min(L - 1, p * 64 + int(_mix(torch.tensor(p * 31 + seed + 5))) % 64) for p in range(n)] + [0, L - 1, max(0, L - 2)]
    for s in range(ns):
        if s * pps < n:
            keys += [s * pps * 64, min(L, min(n, (s + 1) * pps) * 64) - 1]
    return sorted(set(keys))


def target_sets(c):
    """-> list of int64 [B, H]: the sets of targets a test of case c goes through, one fresh launch each (the longest sequence's wanted keys, H at a time; a
    sequence that has run out starts over)"""
    want = [wanted_keys(L, c.nsplit, b) for b, L in enumerate(c.lens)]
    n = max((len(w) + c.H - 1) // c.H for w in want)
    return [torch.tensor([[w[(s * c.H + h) % len(w)] for h in range(c.H)] for w in want], dtype=torch.int64) for s in range(n)]


def onehot_mismatch(out, c, what=""):
    """None when out [B, H * Dr] equals the expectation bit for bit, else the failure message: count, and for the first wrong element sequence, head, the target key with
    its page, split, wave and trip, and the key whose V row came out instead, if any"""
    what = what or str(c)
    if out.shape != c.expect.shape or out.dtype != c.expect.dtype:
        return f"{what}: shape / dtype {tuple(out.shape)} {out.dtype}, expected {tuple(c.expect.shape)} {c.expect.dtype}"
    bad = (_bits(out) != _bits(c.expect)).nonzero()
    if bad.numel() == 0:
        return None
    rep = c.H // c.KV

    def describe(rc):
        b, h, d = rc[0], rc[1] // c.Dr, rc[1] % c.Dr
        t, L = int(c.target[b, h]), c.lens[b]
        page, split, wave, trip = place(L, t, c.nsplit)
        row = _bits(out[b, h * c.Dr:(h + 1) * c.Dr])
        same = " -- the output row equals no key's V row"
        for b2 in range(c.B):
            hit = (_bits(c.v[b2]).reshape(-1, c.Dr) == row[None, :]).all(1).nonzero()
            if hit.numel():
                x = int(hit[0])
                same = f" -- the whole output row equals the V row of key {x // c.KV} (sequence {b2}, KV head {x % c.KV}; expected key {t}, sequence {b}, KV head {h // rep})"
                break
        return (f"(sequence {b}, head {h}, d {d}): got {float(out[rc[0], rc[1]]):.6g}, expected {float(c.expect[rc[0], rc[1]]):.6g}; context {L} = {split_rule(L, c.nsplit)[0]} pages "
                f"in {split_rule(L, c.nsplit)[1]} splits, target key {t} in page {page}, split {split}, wave {wave}, trip {trip}{same}")

    return f"{what}: {bad.shape[0]} of {out.numel()} elements wrong in {bad[:, 0].unique().numel()} sequences; first {describe(bad[0].tolist())}; last {describe(bad[-1].tolist())}"


# ---- bounded family ------------------------------------------------------------------------------------------------------------------------------------------------
def bounded_case(kind, lens, H, KV, Dr, seed, nsplit=NSPLIT, device="cpu"):
    """dense data, scale = Dr^-0.5 (t = tokens from the end of the context):
      late_heavy   the score grows by ~1 natural unit per key over the last 96 keys (k_0, k_1 count them, q_0 = 16 sqrt(Dr), q_1 = sqrt(Dr)): the mass sits on the last real
                   keys of the last, partial page -- a masked last key or a decoy let through takes most of it
      early_heavy  k_0 = +1 in the first page, -1 after it, q_0 = 12 sqrt(Dr): the first page of the first split holds the mass, everything later sits 24 units below
      spike        q = 30 k[j*] / sqrt(Dr) for one key j* per head inside a middle split: one page's wave and one split's record carry the result
      split_skew   k_0 = the split index, q_0 = +-20 sqrt(Dr) by head: every split's maximum is 20 natural units (29 log2 units) from its neighbour's, the first or the last
                   split wins and the merge weights matter
      plain        std-1 data"""
    assert kind in KINDS
    c = Case(kind, lens, H, KV, Dr, Dr ** -0.5, nsplit, device)
    g = torch.Generator()
    g.manual_seed(seed)
    rnd = lambda *s: torch.randn(s, generator=g)
    q = rnd(c.B, H, Dr)
    rep = H // KV
    ks, vs = [], []
    for b, L in enumerate(c.lens):
        k, v = rnd(L, KV, Dr), rnd(L, KV, Dr)
        j = torch.arange(L)
        n, ns, pps = split_rule(L, nsplit)
        if kind == "late_heavy":
            t = (j - (L - 96)).clamp_min(0)
            k[..., 0], k[..., 1] = (t // 16).float()[:, None], (t % 16).float()[:, None]
            q[b, :, 0], q[b, :, 1] = 16.0 * Dr ** 0.5, Dr ** 0.5
        elif kind == "early_heavy":
            k[..., 0] = torch.where(j < 64, 1.0, -1.0)[:, None]
            q[b, :, 0] = 12.0 * Dr ** 0.5
        elif kind == "spike":
            for h in range(H):
                js = min(L - 1, (ns // 2) * pps * 64 + (37 * h + 11 * b + seed) % (pps * 64))
                q[b, h] = k[js, h // rep] * (30.0 / Dr ** 0.5)
        elif kind == "split_skew":
            k[..., 0] = (j // (pps * 64)).float()[:, None]
            q[b, :, 0] = 20.0 * Dr ** 0.5 * torch.where(torch.arange(H) % 2 == 0, 1.0, -1.0)
        ks.append(k.to(bf).float().to(device)), vs.append(v.to(bf).to(device))
    _lay_out(c, ks, vs, seed)
    c.q = torch.zeros((c.B, H, c.D), dtype=bf, device=device)
    c.q[:, :, :Dr] = q.to(bf).to(device)
    _set_decoys(c, torch.stack([k[-1][:, None, :].expand(KV, 64, Dr) for k in ks]))
    return c


def elementwise_bound(c):
    """-> (ref, bound, Abs), float64 [B, H * Dr]: the float64 softmax attention of case c on its bf16 operands (the logical ones: this function does not read the pages), a
    per-element bound on |kernel output - ref| that any implementation with the documented arithmetic meets, and Abs = p @ |v|.

    Derivation (no fitted factor; U32 = 2^-24, b = 2^-8 = the largest relative error of one round-to-nearest to bf16).  Head h of sequence b, L keys, raw scores s_j = q . k_j,
    p = softmax(scale s), n pages in ns splits of pps, R = ceil(pps / 4) + 2 = the rescales a term can pass through: one per trip of its wave (alpha = exp2(m_old - m_new)),
    one in the wave combine and one in the split merge (exp2(m_w - mm), exp2(m_s - gm)); N = L + n + R.
      exponent   the kernels form sv = fl(fl(s~) sc), sc = fl(scale fl(log2 e)), and p~_j = exp2(fl(sv - m)) against the running maximum m of the wave.  In log2 units,
                 relative to the head's final maximum, with M = max_j |s_j| + the accumulation term:
                   fp32 accumulation of the score   sc D U32 sum_d |q_d k_jd|                                   (running-sum bound, any order; the MFMA's is smaller)
                   the product s sc                 U32 M sc
                   sc itself                        2 U32 M sc
                   the difference sv - m            U32 |sv - m| <= 2 U32 M sc
                   each rescale's difference        2 U32 M sc, R of them
                 times ln 2 (sc ln 2 = scale) it is a RELATIVE error of p~_j; v_exp_f32 is good to 1 ulp = 2 U32, once for p and once per rescale, and each rescale is one
                 more fp32 product (U32):
                   delta_j = scale (D U32 sum_d |q_d k_jd| + (5 + 2 R) U32 M) + (2 + 3 R) U32
      P . V      each p~_j is rounded to bf16 (relative b); the products are rounded (per-head kernel: fp32 VALU) or exact (MFMA) and summed in fp32, over the keys of a page,
                 the trips, the waves and the splits: at most N roundings on any path
                   numerator / Lsum = o + nu,  |nu| <= sum_j p_j (delta_j + b + delta_j b) |v_jd| + N U32 (1 + b) sum_j p_j (1 + delta_j) |v_jd|
      row sum    over the UNROUNDED p~_j: l / Lsum = (1 + zeta)(1 + gamma), |zeta| <= sum_j p_j delta_j, |gamma| <= N U32
      quotient   |num / l - o| <= (|nu| + |o| (|zeta| + |gamma| + |zeta gamma|)) / ((1 - |zeta|)(1 - |gamma|)) = e1
      division   one fp32 division, <= 1 ulp = 2 U32: e2 = e1 + 2 U32 (|o| + e1)
      store      round to nearest bf16: half a bf16 ulp at magnitude |o| + e2
      flush      a p~_j below 2^-126 is flushed: <= L 2^-126 max_j |v_jd| against l >= 1 -- L <= 2^14: 2^-112 max_j |v_jd|
    With delta -> 0 this is b Abs + b |o| <= 2 . 2^-8 Abs, the leading term: the bf16 rounding of each probability entering P . V plus that of the stored output."""
    rep = c.H // c.KV
    b8 = 2.0 ** -8
    refs, bounds, Abss = [], [], []
    for b, L in enumerate(c.lens):
        n, ns, pps = split_rule(L, c.nsplit)
        R = (pps + 3) // 4 + 2
        N = L + n + R
        q = c.q[b, :, :c.Dr].double()                                            # [H, Dr]
        k = c.k[b].double().repeat_interleave(rep, dim=1).permute(1, 0, 2)       # [H, L, Dr]
        v = c.v[b].double().repeat_interleave(rep, dim=1).permute(1, 0, 2)
        s = torch.einsum("hd,hjd->hj", q, k)
        es = c.D * U32 * torch.einsum("hd,hjd->hj", q.abs(), k.abs())
        M = (s.abs() + es).amax(-1, keepdim=True)
        delta = c.scale * (es + (5 + 2 * R) * U32 * M) + (2 + 3 * R) * U32
        p = torch.softmax(s * c.scale, -1)
        va = v.abs()
        o, A, Ad = torch.einsum("hj,hjd->hd", p, v), torch.einsum("hj,hjd->hd", p, va), torch.einsum("hj,hjd->hd", p * delta, va)
        zeta = (p * delta).sum(-1, keepdim=True)
        gamma = N * U32
        nu = Ad * (1 + b8) + b8 * A + gamma * (1 + b8) * (A + Ad)
        e1 = (nu + o.abs() * (zeta + gamma + zeta * gamma)) / ((1 - zeta) * (1 - gamma))
        e2 = e1 + 2 * U32 * (o.abs() + e1)
        refs.append(o.reshape(-1)), Abss.append(A.reshape(-1))
        bounds.append((e2 + 0.5 * bf16_ulp(o.abs() + e2) + 2.0 ** -112 * va.amax(1)).reshape(-1))
    return torch.stack(refs), torch.stack(bounds), torch.stack(Abss)


def bound_violations(out, ref, bound, c, what=""):
    """-> (message or None, largest |out - ref| / bound): zero elements may lie outside the per-element bound"""
    what = what or str(c)
    g = out.double()
    if g.shape != ref.shape:
        return f"{what}: shape {tuple(g.shape)}, expected {tuple(ref.shape)}", float("inf")
    err = (g - ref).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max())
    bad = (err > bound).nonzero()
    if bad.numel() == 0:
        return None, worst

    def d(rc):
        b, h, dd = rc[0], rc[1] // c.Dr, rc[1] % c.Dr
        n, ns, pps = split_rule(c.lens[b], c.nsplit)
        return (f"(sequence {b}, head {h}, d {dd}): got {float(g[rc[0], rc[1]]):.6g}, reference {float(ref[rc[0], rc[1]]):.6g}, bound {float(bound[rc[0], rc[1]]):.3g}; "
                f"context {c.lens[b]} = {n} pages in {ns} splits of {pps}")

    return f"{what}: {bad.shape[0]} of {g.numel()} elements outside the bound (worst err / bound {worst:.3g}); first {d(bad[0].tolist())}; last {d(bad[-1].tolist())}", worst


# ---- the kernels' arithmetic in plain torch ------------------------------------------------------------------------------------------------------------------------
def decoy_part(c, extra=0, device=None):
    """the workspace f32 [B * H * nsplit * (D + 2) + extra] full of records that would win any merge (acc = 7, m = 1e4, l = 1); the extra words hold SENT"""
    rec = torch.full((c.D + 2,), DECOY_ACC, dtype=torch.float32)
    rec[c.D], rec[c.D + 1] = DECOY_M, DECOY_L
    return torch.cat([rec.repeat(c.B * c.H * c.nsplit), torch.full((extra,), SENT, dtype=torch.float32)]).to(device or c.device)


def min_gsplit(c, cpb):
    """the smallest gsplit that serves case c at cpb splits per block"""
    return max((split_rule(L, c.nsplit)[1] + cpb - 1) // cpb for L in c.lens)


def emulate(c, shape=None, mut=None, part=None):
    """The documented arithmetic of both kernels: per (sequence, head) the split rule above; wave w of a split walks its pages with a running (m, l, acc): sv = fl(s sc),
    keys >= pos + 1 at -1e30, alpha = exp2(m - m_new), p = exp2(sv - m_new), l = l alpha + sum p, acc = acc alpha + bf16(p) . V; the four waves are combined against their
    common maximum in wave order; one split: out = acc / l; otherwise one record per split and a merge over the ns records against their maximum in split order.
    shape = (cpb, gsplit, hpb): the launch shape changes no arithmetic -- it is only checked against the rule gvl_op_decode_attention enforces (gsplit * cpb >= splits).
    part: the workspace [B, H, nsplit, D + 2] to publish into (default: decoy_part).
    -> (out bf16 [B, H * Dr + GUARD_COLS] on a SENT fill, part)

    mut: one of MUTATIONS -- a WRONG kernel:
      mask_plus / mask_minus   key pos + 1 is visible / key pos is hidden
      drop_second_trip         a wave's second page (pg += 4) is skipped
      pps_floor                pps = floor(pages / ns): the pages behind ns pps are never read
      drop_last_split          the merge runs over ns - 1 records
      merge_all_nsplit         the merge runs over nsplit records: it picks up whatever the workspace held
      no_rescale_wave          the wave combine adds the four waves without exp2(m_w - mm)
      no_rescale_merge         the merge adds the records without exp2(m_s - gm)
      gqa_mod                  query head h reads KV head h % KV
      table_identity           page i of a sequence is taken to be page i of the pool
      table_of_seq0            every sequence reads sequence 0's table
      dout_stride              head h's output goes to column h D instead of h Dr"""
    assert mut is None or mut in MUTATIONS
    B, H, KV, Dr, D, dev = c.B, c.H, c.KV, c.Dr, c.D, c.device
    if shape is not None:
        cpb, gsplit, _ = shape
        cpb = max(1, cpb)
        assert (gsplit if 0 < gsplit <= c.nsplit else (c.nsplit + cpb - 1) // cpb) * cpb >= max(split_rule(L, c.nsplit)[1] for L in c.lens)
    rep = H // KV
    hk = torch.arange(H, device=dev) % KV if mut == "gqa_mod" else torch.arange(H, device=dev) // rep
    sc = torch.tensor(np.float32(c.scale) * LOG2E, dtype=torch.float32, device=dev)
    part = (decoy_part(c) if part is None else part.clone())[:B * H * c.nsplit * (D + 2)].view(B, H, c.nsplit, D + 2)
    stride = H * Dr + GUARD_COLS
    flat = torch.full((B * stride + H * D,), SENT, dtype=bf, device=dev)
    tables = c.tables.cpu()
    lane = torch.arange(64, device=dev)
    for b in range(B):
        L = c.lens[b]
        n, ns, pps = split_rule(L, c.nsplit)
        if mut == "pps_floor":
            pps = max(1, n // ns)
        tab = tables[0 if mut == "table_of_seq0" else b]
        lim = L + (1 if mut == "mask_plus" else -1 if mut == "mask_minus" else 0)
        q = c.q[b].float()
        for s in range(ns):
            p_begin, p_end = s * pps, min(s * pps + pps, n)
            red = []
            for w in range(4):
                m = torch.full((H,), -1e30, dtype=torch.float32, device=dev)
                l = torch.zeros((H,), dtype=torch.float32, device=dev)
                acc = torch.zeros((H, D), dtype=torch.float32, device=dev)
                for trip, pg in enumerate(range(p_begin + w, p_end, 4)):
                    if mut == "drop_second_trip" and trip == 1:
                        continue
                    page = pg if mut == "table_identity" else int(tab[pg])
                    K, V = c.Kt[page, hk].float(), c.Vt[page, hk].float()                          # [H, 64, D], [H, D, 64]
                    sv = torch.einsum("hkd,hd->hk", K, q) * sc
                    sv = torch.where((pg * 64 + lane >= lim)[None, :], torch.full_like(sv, -1e30), sv)
                    m_new = torch.maximum(m, sv.amax(1))
                    alpha = torch.exp2(m - m_new)
                    p = torch.exp2(sv - m_new[:, None])
                    l = l * alpha + p.sum(1)
                    acc = acc * alpha[:, None] + torch.einsum("hk,hdk->hd", p.to(bf).float(), V)
                    m = m_new
                red.append((acc, m, l))
            mm = torch.stack([r[1] for r in red]).amax(0)
            racc, rl = torch.zeros_like(red[0][0]), torch.zeros_like(red[0][2])
            for acc, m, l in red:
                wgt = torch.ones_like(m) if mut == "no_rescale_wave" else torch.exp2(m - mm)
                racc, rl = racc + acc * wgt[:, None], rl + l * wgt
            if ns > 1:                                                                             # the one-split path publishes nothing
                part[b, :, s, :D], part[b, :, s, D], part[b, :, s, D + 1] = racc, mm, rl
        if ns == 1:
            o = racc / rl[:, None]
        else:
            nm = ns - 1 if mut == "drop_last_split" else c.nsplit if mut == "merge_all_nsplit" else ns
            gm = part[b, :, :nm, D].amax(1)
            ml, macc = torch.zeros((H,), dtype=torch.float32, device=dev), torch.zeros((H, D), dtype=torch.float32, device=dev)
            for s in range(nm):
                wgt = torch.ones_like(gm) if mut == "no_rescale_merge" else torch.exp2(part[b, :, s, D] - gm)
                ml, macc = ml + part[b, :, s, D + 1] * wgt, macc + part[b, :, s, :D] * wgt[:, None]
            o = macc / ml[:, None]
        for h in range(H):
            col = b * stride + h * (D if mut == "dout_stride" else Dr)
            flat[col:col + Dr] = o[h, :Dr].to(bf)
    return flat[:B * stride].view(B, stride), part


# ---- THE lists of test_gpu_decode_attn_exact.py ----------------------------------------------------------------------------------------------------------------------
LENS = [1, 2, 63, 64, 65, 255, 256, 257, 833, 1025, 4096, 4097, 5185, 8256]
CPBS = [1, 2, 3, 4, 16]
# (H, KV, Dr, hpb, what the plan must give: kernel_of)
GEOS = [(4, 4, 64, 0, ("head", 64, 0)), (2, 2, 96, 0, ("head", 96, 0)), (2, 2, 128, 0, ("head", 128, 0)), (4, 4, 32, 0, ("head", 64, 0)), (2, 2, 80, 0, ("head", 96, 0)),
        (2, 2, 104, 0, ("head", 128, 0)),
        (8, 2, 64, 1, ("gqa", 64, 4, 1)), (8, 2, 64, 2, ("gqa", 64, 4, 1)), (8, 2, 64, 4, ("gqa", 64, 4, 1)), (6, 2, 128, 0, ("gqa", 128, 4, 1)), (4, 2, 32, 0, ("gqa", 64, 4, 1)),
        (8, 1, 64, 0, ("gqa", 64, 16, 1)), (16, 1, 128, 16, ("gqa", 128, 16, 1)), (16, 1, 128, 8, ("gqa", 128, 16, 1)),
        (8, 2, 96, 1, ("gqa", 96, 4, 0)), (8, 2, 96, 2, ("gqa", 96, 4, 0)), (8, 2, 96, 4, ("gqa", 96, 4, 0)), (8, 1, 80, 0, ("gqa", 96, 16, 0)),
        (32, 1, 64, 0, ("head", 64, 1)), (32, 1, 96, 0, ("head", 96, 1)), (64, 2, 128, 0, ("head", 128, 1))]
REACHABLE = ({("head", D, ph) for D in (64, 96, 128) for ph in (0, 1)} | {("gqa", D, gm, 1) for D in (64, 128) for gm in (4, 16)} | {("gqa", 96, gm, 0) for gm in (4, 16)})
LENS3 = [256, 833, 4097]                                                          # a one-split sequence, a merging one and a clamped one
LENS16 = [65, 1, 257, 64, 1025, 833, 2, 4097, 63, 1000, 255, 256, 4096, 130, 700, 3000]
SHARE16 = (5, 9, 10)                                                              # sequences 5 and 9 share their first 10 pages
# one geometry per group of instantiations for the bounded family and the bit-identity tests
BOUNDED_GEOS = [0, 4, 7, 9, 13, 15, 17, 19, 20]
BOUNDED_LENS = [65, 257, 1025, 4097]


def exact_cases():
    """-> list of dict(geo, lens, H, KV, Dr, hpb, cpb, gsplit_min, out_tiled, pad, share, seed): per geometry every length alone, the batch of 3 and the batch of 16;
    cpb, gsplit (0 or the exact minimum), out_tiled and padded strides walk through their values with the case index -- no full product"""
    out = []
    for i, (H, KV, Dr, hpb, _) in enumerate(GEOS):
        rows = [([L], None) for L in LENS] + [(LENS3, None), (LENS16, SHARE16)]
        for j, (lens, share) in enumerate(rows):
            out.append(dict(geo=i, lens=lens, H=H, KV=KV, Dr=Dr, hpb=hpb, cpb=CPBS[(i + j) % 5], gsplit_min=(i + j // 5) % 2, out_tiled=(i + j // 2) % 2, pad=(i + j) % 3 == 0,
                            share=share, seed=100 * i + j))
    return out


def bounded_cases():
    """-> list of dict(geo, kind, lens, H, KV, Dr, hpb, cpb, gsplit_min, out_tiled, pad, seed): every kind on one geometry per group of instantiations, a batch of four lengths"""
    out = []
    for n, i in enumerate(BOUNDED_GEOS):
        H, KV, Dr, hpb, _ = GEOS[i]
        for j, kind in enumerate(KINDS):
            out.append(dict(geo=i, kind=kind, lens=BOUNDED_LENS, H=H, KV=KV, Dr=Dr, hpb=hpb, cpb=CPBS[(n + j) % 5], gsplit_min=(n + j) % 2, out_tiled=(n + j // 2) % 2,
                            pad=(n + j) % 3 == 0, seed=1000 + 10 * i + j))
    return out
