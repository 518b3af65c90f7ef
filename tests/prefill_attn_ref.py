"""References for the paged forms of attn_fwd_kernel behind a cached prefix (gvl_attn.hip, reached through gvl_op_prefill_attention): a caller-supplied block table with
qpos0 / Sk, the ragged grid (VL = 1) and the ragged-extend grid (VL = 2).  attn_ref.py generalised to a key context: query i of a sequence sits at position qpos0 + i of
Sk keys, and a launch holds several sequences (members).  It imports attn_ref's primitives and leaves that file alone; no GPU needed to import or run this file.

Both families are attn_ref's, per member:
  exact     one-hot attention with attn_ref's construction over the Sk keys of the context (codes of j XOR mask(member, KV head), q = 64 code(target XOR mask), scale 1):
            the output must equal the target's V row BIT FOR BIT.  Target maps (causal): diag = the last visible key qpos0 + i, zero = key 0, tile_first = the first key of
            the query's own tile, prefix_last = the last cached key qpos0 - 1, first_new = qpos0, hash = over all visible keys; (full) last / perm / edges over Sk.
  bounded   a member's data is attn_ref.bounded_case over its WHOLE context (B = 1, S = Sk) of which the launch computes the rows qpos0 .. qpos0 + S - 1 -- so reference and
            bound are attn_ref.elementwise_bound of that case, rows qpos0 .. : the derivation is per visible key count and tile count of the row, nothing new is needed.
The pools are built HERE, on the host, not by gvl_op_qkv_post: K and V^T pages no table names are NaN, K slots >= Sk of a last partial page are NaN (nobody ever writes
them and the kernel masks by index), V^T slots >= Sk hold +-1e30 (finite: P = 0 there), block tables are permuted and longer than needed.

emulate(case, mut=None)   the kernel's documented arithmetic reading the pages THROUGH the tables (attn_ref.emulate's, plus the per-wave causal tile skip, the per-block
                          tile count and the need_mask predicate, which a correct kernel cannot tell from masking everything -- the mutations can); mut: MUTATIONS.
exact_cases() / bounded_cases() / group_cases()   THE lists test_gpu_prefill_attn.py runs; make(spec) -> Case.
relocated_cases()         cases of those lists on pages whose element offsets inside the pools lie above 2^31 (one above 2^30): make(spec, first_page=, pools=) names the
                          pages first_page + (the same permutation) in caller-owned, all-NaN pools and writes the named pages only; on the CPU the pools are sparse
                          (SparsePools: page id -> array).  Data, targets, expectation and bound do not depend on first_page.
"""
import copy

import numpy as np
import torch

import attn_ref as A
from attn_ref import SENT, LAZY, LOG2E, KINDS, _bits, _code, onehot_v
from gemm_ref import _mix
from kv_page_ref import PAGE_MUTATIONS, POOL_ELEMS, first_page_above, wrap_page_offset

bf = torch.bfloat16
VPAD = 1e30
GUARD_ROWS = 160
CAUSAL_MAPS = ("diag", "zero", "tile_first", "prefix_last", "first_new", "hash")
FULL_MAPS = ("last", "perm", "edges")
MUTATIONS = ("mask_plus", "mask_minus", "skip_no_qpos0", "mask_no_qpos0", "n_tiles_from_S", "no_tail_mask", "wrong_member_table", "prefix_offset_dropped", "member_off_by_one",
             "gqa_mod", "no_rescale_O", "skip_last8") + PAGE_MUTATIONS           # the last three: a page's base address formed in 32 bits (kv_page_ref.wrap_page_offset)
BENIGN = ("need_mask_pred_no_qpos0",)   # qpos0 dropped from the need_mask PREDICATE alone makes it true on a superset of the tiles: masks are applied where none is needed, no bit changes
SHAPES = ((64, 1), (64, 31), (64, 33), (64, 64), (64, 65), (128, 129), (192, 130), (0, 130), (960, 65))      # (qpos0, S), Sk = qpos0 + S
DGEOS = ((64, 64), (64, 32), (96, 80), (128, 128))                                                            # (D, Dout)
HKV = ((4, 4), (4, 2), (8, 1))
GROUPS = ((129,), (65, 31), (1, 65, 128, 129, 31, 128, 65, 1))
EXT_POS0 = ((64, 0, 192, 64, 0, 192, 64, 0), (0,) * 8)


class Member:
    def __init__(self, row0, S, qpos0, Sk, table, mask_id, share=None):
        self.row0, self.S, self.qpos0, self.Sk, self.table, self.mask_id, self.share = row0, S, qpos0, Sk, [int(x) for x in table], mask_id, share


class Case:
    def __str__(self):
        s = self.spec
        body = f"B{s['B']} S{s['S']} qpos0 {s['qpos0']} Sk {s['Sk']}" if self.form == "single" else f"members {tuple(s['lens'])} pos0 {tuple(m.qpos0 for m in self.members)}"
        return f"{self.what} {self.form} {body} H{self.H}/{self.KV} D{self.D} Dout{self.Dr} causal{self.causal} ring{self.ring}"


class SparsePools:
    """a pool as page id -> [KV, ., .] array, for the CPU: a page nobody wrote reads as NaN, which is what the GPU test fills its pools with"""

    def __init__(self, n_pages, shape, device):
        self.shape, self.page_shape, self.device, self.pages = (n_pages,) + tuple(shape), tuple(shape), device, {}

    def __getitem__(self, pg):
        assert 0 <= pg < self.shape[0]
        if pg not in self.pages:
            self.pages[pg] = torch.full(self.page_shape, float("nan"), dtype=bf, device=self.device)
        return self.pages[pg]


def layout(spec, first_page=0, n_pages=None):
    """-> Case with members, tables (permuted, one spare entry that is no page, behind each), n_pages (4 pages nobody names); no data yet.  first_page / n_pages: the
    case's pages are first_page + (the same permutation) in pools of n_pages pages; c.page0 = first_page, c.win = the pages laid out (the named ones and the 4 spares)"""
    c = Case()
    c.spec = dict(spec)
    c.form, c.H, c.KV, c.D, c.Dr, c.causal, c.ring, c.seed = spec["form"], spec["H"], spec["KV"], spec["D"], spec["Dout"], int(spec["causal"]), spec.get("ring", 0), spec["seed"]
    rng = np.random.RandomState(77 + c.seed)
    if c.form == "single":
        B, S, q0 = spec["B"], spec["S"], spec["qpos0"]
        Sk = spec["Sk"] or S
        trip = [(S, q0, Sk, None)] * B
        c.B, c.S, c.qpos0, c.Sk = B, S, q0, spec["Sk"]
    else:
        lens = list(spec["lens"])
        p0 = list(spec["vl_pos0"][:len(lens)]) if c.form == "ext" else [0] * len(lens)
        share = spec.get("share")                                        # (u, w): member u's prefix pages are member w's
        trip = [(s, p, p + s, share[1] if share and share[0] == u else None) for u, (s, p) in enumerate(zip(lens, p0))]
        c.B, c.S, c.qpos0, c.Sk = 1, max(lens), 0, 0
    tiles = [(Sk + 63) // 64 for _, _, Sk, _ in trip]
    own = [t - (q0 // 64 if sh is not None else 0) for t, (_, q0, _, sh) in zip(tiles, trip)]
    c.page0, c.win, c.page_elems = first_page, sum(own) + 4, c.KV * 64 * c.D
    c.n_pages = n_pages or first_page + c.win
    assert first_page + c.win <= c.n_pages
    perm = [first_page + int(x) for x in rng.permutation(c.win)[:sum(own)]]
    c.members, row0 = [], 0
    for u, (S, q0, Sk, sh) in enumerate(trip):
        head = c.members[sh].table[:q0 // 64] if sh is not None else []
        tab = head + [int(perm.pop()) for _ in range(own[u])] + [c.n_pages + 9]
        c.members.append(Member(row0, S, q0, Sk, tab, c.members[sh].mask_id if sh is not None else u, sh))
        row0 += S
    c.rows = row0
    c.max_pages = max(tiles) + 1
    c.block_table = torch.tensor([m.table for m in c.members], dtype=torch.int32) if c.form == "single" else None
    return c


def place(c, device="cpu", pools=None):
    """members' q / k / v (bf16 [S, H, Dr], [Sk, KV, Dr] x 2) -> Q [rows H D + a NaN tail], Kt, Vt pools as the docstring describes.  pools = (Kt, Vt): the caller's
    [n_pages, KV, 64, D] / [n_pages, KV, D, 64] tensors, all NaN already -- only the named pages are written; pools = "sparse": SparsePools (CPU)"""
    H, KV, D, Dr = c.H, c.KV, c.D, c.Dr
    c.Q = torch.full((c.rows * H * D + 64 * D,), float("nan"), dtype=bf, device=device)
    if pools is None:
        c.Kt = torch.full((c.n_pages, KV, 64, D), float("nan"), dtype=bf, device=device)
        c.Vt = torch.full((c.n_pages, KV, D, 64), float("nan"), dtype=bf, device=device)
    elif pools == "sparse":
        c.Kt, c.Vt = SparsePools(c.n_pages, (KV, 64, D), device), SparsePools(c.n_pages, (KV, D, 64), device)
    else:
        c.Kt, c.Vt = pools
        assert tuple(c.Kt.shape) == (c.n_pages, KV, 64, D) and tuple(c.Vt.shape) == (c.n_pages, KV, D, 64)
    pad = torch.where(torch.arange(64, device=device) % 2 == 0, VPAD, -VPAD).to(bf)
    for m, q, k, v in zip(c.members, c.q, c.k, c.v):
        Qm = c.Q[m.row0 * H * D:(m.row0 + m.S) * H * D].view(H, m.S, D)
        Qm[:, :, :Dr], Qm[:, :, Dr:] = q.permute(1, 0, 2), 0
        for t in range((m.Sk + 63) // 64):
            n = min(64, m.Sk - t * 64)
            kp, vp = c.Kt[m.table[t]], c.Vt[m.table[t]]
            kp[:, :n, :Dr], kp[:, :n, Dr:] = k[t * 64:t * 64 + n].permute(1, 0, 2), 0
            vp[:, :Dr, :n], vp[:, Dr:, :] = v[t * 64:t * 64 + n].permute(1, 2, 0), 0
            vp[:, :Dr, n:] = pad[n:]
    c.tables = [torch.tensor(m.table, dtype=torch.int32, device=device) for m in c.members]
    if c.block_table is not None:
        c.block_table = c.block_table.to(device)
    return c


# ---- exact family ----------------------------------------------------------------------------------------------------------------------------------------------------
def targets(m, H, target, seed, u, device="cpu"):
    """-> int64 [H, S]: the one key query (h, i) of member m attends to"""
    i = torch.arange(m.S, device=device, dtype=torch.int64)[None, :]
    h = torch.arange(H, device=device, dtype=torch.int64)[:, None]
    z = torch.zeros((H, m.S), dtype=torch.int64, device=device)
    p = m.qpos0 + i
    if target == "diag":
        return z + p
    if target == "zero":
        return z
    if target == "tile_first":
        return z + (p - p % 64)
    if target == "prefix_last":
        return z + max(m.qpos0 - 1, 0)
    if target == "first_new":
        return z + m.qpos0
    if target == "hash":
        return _mix(u * 7919 + h * 104729 + i * 31 + seed * 13 + 3) % (p + 1)
    if target in FULL_MAPS:                                              # attn_ref's maps over the Sk keys of the context
        return A.targets(1, m.Sk, H, target, seed + u, device)[0][:, m.qpos0:m.qpos0 + m.S]
    raise ValueError(target)


def onehot_case(spec, device="cpu", first_page=0, pools=None, n_pages=None):
    c = layout(spec, first_page, n_pages if pools is None or pools == "sparse" else pools[0].shape[0])
    c.what, c.scale, c.target_map = f"one-hot {spec['target']}", 1.0, spec["target"]
    assert spec["target"] in (CAUSAL_MAPS if c.causal else FULL_MAPS)
    H, KV, Dr = c.H, c.KV, c.Dr
    Skm = max(m.Sk for m in c.members)
    nb = max(1, (Skm - 1).bit_length())
    assert nb <= 14 and nb <= Dr
    rep = H // KV
    n = len(c.members)
    mask = _mix(torch.arange(n, device=device, dtype=torch.int64)[:, None] * 131 + torch.arange(KV, device=device, dtype=torch.int64)[None, :] * 17 + c.seed + 7) % (1 << nb)
    vall = onehot_v(n, Skm, KV, Dr, c.seed, device)
    c.q, c.k, c.v, c.target, exp = [], [], [], [], []
    for u, m in enumerate(c.members):
        j = torch.arange(m.Sk, device=device, dtype=torch.int64)
        k = _code(j[:, None] ^ mask[m.mask_id][None, :], nb, Dr).to(bf)                      # [Sk, KV, Dr]
        v = vall[u, :m.Sk].clone()
        if m.share is not None:
            v[:m.qpos0] = c.v[m.share][:m.qpos0]                                              # the same physical pages
        t = targets(m, H, spec["target"], c.seed, u, device)
        assert bool(((t >= 0) & (t < m.Sk)).all()) and (not c.causal or bool((t <= m.qpos0 + torch.arange(m.S, device=device)[None, :]).all()))
        qmask = mask[m.mask_id].repeat_interleave(rep)                                        # [H]
        q = (64.0 * _code(t ^ qmask[:, None], nb, Dr)).permute(1, 0, 2).to(bf)               # [S, H, Dr]
        vh = v.permute(1, 0, 2).repeat_interleave(rep, dim=0)                                 # [H, Sk, Dr]
        exp.append(torch.gather(vh, 1, t[..., None].expand(H, m.S, Dr)).permute(1, 0, 2).reshape(m.S, H * Dr))
        c.q.append(q), c.k.append(k), c.v.append(v), c.target.append(t)
    c.expect = torch.cat(exp).contiguous()
    return place(c, device, pools)


def where_of(c, row):
    u = max(k for k, m in enumerate(c.members) if m.row0 <= row)
    return u, row - c.members[u].row0


def onehot_mismatch(got, c, what=""):
    """None when got [rows, H Dout] equals the expectation bit for bit, else the message: the count and, for the first wrong element, member, (h, i, d), the target key with
    its page, query block, wave, key tile, and the key whose V row came out instead"""
    what = what or str(c)
    if got.shape != c.expect.shape:
        return f"{what}: shape {tuple(got.shape)}, expected {tuple(c.expect.shape)}"
    bad = (_bits(got) != _bits(c.expect)).nonzero()
    if bad.numel() == 0:
        return None
    r, col = bad[0].tolist()
    u, i = where_of(c, r)
    m, h, d = c.members[u], col // c.Dr, col % c.Dr
    t = int(c.target[u][h, i])
    row = _bits(got[r, h * c.Dr:(h + 1) * c.Dr])
    same = " -- the output row equals no key's V row of any member"
    for w, v in enumerate(c.v):
        hit = (_bits(v).view(-1, c.Dr) == row[None, :]).all(1).nonzero()
        if hit.numel():
            x = int(hit[0])
            same = f" -- the whole output row equals the V row of key {x // c.KV} of member {w}, KV head {x % c.KV} (expected key {t} of member {u}, KV head {h // (c.H // c.KV)})"
            break
    return (f"{what}: {bad.shape[0]} of {got.numel()} elements wrong in {bad[:, 0].unique().numel()} rows; first member {u} (h {h}, i {i}, d {d}): got {float(got[r, col]):.6g}, expected "
            f"{float(c.expect[r, col]):.6g}; target key {t} (position of the query {m.qpos0 + i}) in key tile {t // 64} = page {m.table[t // 64]}, query block {i // 128}, wave {i % 128 // 32}{same}")


# ---- bounded family ----------------------------------------------------------------------------------------------------------------------------------------------------
def bounded_case(spec, device="cpu", first_page=0, pools=None, n_pages=None):
    """per member attn_ref.bounded_case over the whole context; -> Case with .full (the attn_ref cases) for elementwise_bound"""
    c = layout(spec, first_page, n_pages if pools is None or pools == "sparse" else pools[0].shape[0])
    c.what, c.scale = spec["kind"], c.Dr ** -0.5
    c.q, c.k, c.v, c.full = [], [], [], []
    for u, m in enumerate(c.members):
        f = A.bounded_case(1, m.Sk, c.H, c.KV, c.Dr, c.causal, spec["kind"], c.seed * 16 + u, device)
        q, k, v = (t[0] for t in f.split())
        c.q.append(q[m.qpos0:m.qpos0 + m.S].contiguous()), c.k.append(k.contiguous()), c.v.append(v.contiguous()), c.full.append(f)
    return place(c, device, pools)


def elementwise_bound(c):
    """-> (ref, bound), float64 [rows, H Dout]: attn_ref.elementwise_bound of each member's whole context, the rows the launch computes"""
    ref, bound = [], []
    for m, f in zip(c.members, c.full):
        r, b, _ = A.elementwise_bound(f)
        ref.append(r[m.qpos0:m.qpos0 + m.S]), bound.append(b[m.qpos0:m.qpos0 + m.S])
    return torch.cat(ref), torch.cat(bound)


def bound_violations(got, ref, bound, c, what=""):
    """-> (message or None, largest |got - ref| / bound): zero elements may lie outside the bound"""
    what = what or str(c)
    g = got.double()
    err = (g - ref).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max())
    bad = (err > bound).nonzero()
    if bad.numel() == 0:
        return None, worst
    r, col = bad[0].tolist()
    u, i = where_of(c, r)
    m = c.members[u]
    return (f"{what}: {bad.shape[0]} of {g.numel()} elements outside the bound (worst err / bound {worst:.3g}); first member {u} (h {col // c.Dr}, i {i}, d {col % c.Dr}): got "
            f"{float(g[r, col]):.6g}, reference {float(ref[r, col]):.6g}, bound {float(bound[r, col]):.3g}; query position {m.qpos0 + i} of {m.Sk} keys, query block {i // 128}, "
            f"wave {i % 128 // 32}, diagonal key tile {(m.qpos0 + i) // 64}"), worst


# ---- the kernel's arithmetic, reading the pages through the tables -------------------------------------------------------------------------------------------------------
def _run(c, q, table, qpos0, Sk, mut):
    """one sequence: q bf16 [S, H, Dr] against the context (table, qpos0, Sk) in the pools -> bf16 [S, H Dr]"""
    H, KV, Dr = c.H, c.KV, c.Dr
    dev = q.device
    S = q.shape[0]
    rep = H // KV
    hk = torch.arange(H, device=dev) % KV if mut == "gqa_mod" else torch.arange(H, device=dev) // rep
    qf = q.permute(1, 0, 2).float()                                                  # [H, S, Dr]
    i = torch.arange(S, device=dev)
    qw = (i // 32) * 32
    last_q = torch.clamp((i // 128) * 128 + 127, max=S - 1)
    tiles_all = (Sk + 63) // 64
    n_tiles = ((0 if mut == "n_tiles_from_S" else qpos0) + last_q) // 64 + 1 if c.causal else torch.full((S,), tiles_all, device=dev)
    sc = np.float32(c.scale) * LOG2E
    sc32, sc64 = torch.tensor(sc, dtype=torch.float32, device=dev), float(sc)
    G = (S + 31) // 32
    m_run = torch.full((H, S), -1e30, dtype=torch.float32, device=dev)
    l_run = torch.zeros((H, S), dtype=torch.float32, device=dev)
    O = torch.zeros((H, S, Dr), dtype=torch.float32, device=dev)
    lim = qpos0 + i + (1 if mut == "mask_plus" else -1 if mut == "mask_minus" else 0)
    if mut == "mask_no_qpos0":
        lim = i
    for t in range(int(n_tiles.max())):
        tt = t - qpos0 // 64 if (mut == "prefix_offset_dropped" and t >= qpos0 // 64) else t
        pg = table[tt] if tt < len(table) else -1
        wrapped = mut in PAGE_MUTATIONS and wrap_page_offset(pg * c.page_elems, mut) != pg * c.page_elems
        if 0 <= pg < c.n_pages and not wrapped:
            kt, vt = c.Kt[pg][:, :, :Dr].float()[hk], c.Vt[pg][:, :Dr, :].float().transpose(-1, -2)[hk]     # [H, 64, Dr] each
        else:     # no page at all (only under a mutation): the GPU would read foreign memory.  A wrapped offset points in front of the case's pages, where the pools hold NaN
            kt = vt = torch.full((H, 64, Dr), float("nan"), device=dev)
        keys = torch.arange(t * 64, t * 64 + 64, device=dev)
        active = t < n_tiles
        if c.causal:
            active = active & ~(t * 64 > (0 if mut == "skip_no_qpos0" else qpos0) + qw + 31)                # the wave-uniform causal tile skip
        s = qf @ kt.transpose(-1, -2)                                                # [H, S, 64]
        need = torch.full((S,), bool(t == tiles_all - 1 and Sk & 63), device=dev)
        if c.causal:
            need = need | (t * 64 + 63 > (0 if mut == "need_mask_pred_no_qpos0" else qpos0) + qw)
        dead = (keys >= Sk)[None, :].expand(S, 64) & (mut != "no_tail_mask")
        if c.causal:
            dead = dead | (keys[None, :] > lim[:, None])
        dead = (dead & need[:, None]) | ~active[:, None]
        s = torch.where(dead[None], torch.full_like(s, -1e30), s)
        mx = s.amax(-1)
        vote = ((mx - m_run) * sc32 > LAZY) & active[None]
        vote = torch.cat([vote, torch.zeros((H, G * 32 - S), dtype=torch.bool, device=dev)], -1).view(H, G, 32).any(-1).repeat_interleave(32, dim=-1)[..., :S]
        m_new = torch.where(vote & active[None], torch.maximum(m_run, mx), m_run)
        alpha = torch.exp2(((m_run - m_new) * sc32).double()).float()
        m_run = m_new
        if mut != "no_rescale_O":
            O = O * alpha[..., None]
        p = torch.exp2(s.double() * sc64 + (-m_run * sc32).double()[..., None]).float()
        p = torch.where(active[None, :, None], p, torch.zeros_like(p))
        l_run = l_run * alpha + p.sum(-1)
        pv = p.to(bf).float() @ vt                                                   # 0 x (+-1e30 behind Sk) = 0; a NaN page poisons every row that multiplies it, as on the matrix pipe
        O = O + torch.where(active[None, :, None], pv, torch.zeros_like(pv))         # a wave that skips the tile does not multiply it
    out = (O * (1.0 / l_run)[..., None]).to(bf)
    if mut == "skip_last8":
        out[..., Dr - 8:] = SENT
    return out.permute(1, 0, 2).reshape(S, H * Dr)


def emulate(c, mut=None):
    assert mut is None or mut in MUTATIONS + BENIGN
    n = len(c.members)
    outs = []
    for u, m in enumerate(c.members):
        ctx = c.members[(u + 1) % n] if mut == "wrong_member_table" else m
        out = _run(c, c.q[u], ctx.table, m.qpos0, m.Sk, mut)
        if mut == "member_off_by_one" and u > 0:                                     # the member's first query block is decoded as the previous member's
            w = c.members[u - 1]
            out[:128] = _run(c, c.q[u], w.table, w.qpos0, w.Sk, None)[:128]
        outs.append(out)
    return torch.cat(outs + [torch.full((GUARD_ROWS, c.H * c.Dr), SENT, dtype=bf, device=c.Q.device)])


def single_launch_of(c, u):
    """member u of a group as a single-sequence launch at (qpos0, Sk) = (vl_pos0[u], vl_pos0[u] + S_u) on the same pools and its own table"""
    m = c.members[u]
    d = copy.copy(c)
    d.form, d.B, d.S, d.qpos0, d.Sk, d.rows = "single", 1, m.S, m.qpos0, m.Sk, m.S
    d.spec = dict(c.spec, B=1, S=m.S, qpos0=m.qpos0, Sk=m.Sk)
    d.members = [Member(0, m.S, m.qpos0, m.Sk, m.table, m.mask_id)]
    d.block_table, d.max_pages = c.tables[u][None, :].contiguous(), len(m.table)
    d.tables = [c.tables[u]]
    d.Q = torch.cat([c.Q[m.row0 * c.H * c.D:(m.row0 + m.S) * c.H * c.D], c.Q[-64 * c.D:]]).contiguous()
    for name in ("q", "k", "v", "target", "full"):
        if hasattr(c, name):
            setattr(d, name, [getattr(c, name)[u]])
    if hasattr(c, "expect") and c.expect is not None:
        d.expect = c.expect[m.row0:m.row0 + m.S]
    return d


# ---- THE lists of test_gpu_prefill_attn.py -----------------------------------------------------------------------------------------------------------------------------
def _single_shapes():
    out = [dict(S=S, qpos0=q0, Sk=q0 + S, causal=1) for q0, S in SHAPES]
    out.append(dict(S=65, qpos0=64, Sk=64 + 65 + 70, causal=1))          # keys beyond every query: a partial last tile that is entirely future
    out.append(dict(S=65, qpos0=0, Sk=200, causal=0))                    # non-causal with a longer context in a table
    return out


def exact_cases():
    out, n = [], 0
    for si, sh in enumerate(_single_shapes()):
        for gi, (D, Dout) in enumerate(DGEOS):
            H, KV = HKV[(si + gi) % 3]
            for ti, target in enumerate(CAUSAL_MAPS if sh["causal"] else FULL_MAPS):
                n += 1
                out.append(dict(form="single", B=1 + (si + gi + ti) % 2, H=H, KV=KV, D=D, Dout=Dout, ring=(0, 2, 3)[(si + gi + ti) % 3], target=target, seed=n, **sh))
    return out


def group_cases(kind_or_target):
    """ragged (VL = 1) and ragged-extend (VL = 2) groups; kind_or_target: "exact" -> every causal map, "bounded" -> the kinds cycle"""
    out, n = [], 0
    for gi, (D, Dout) in enumerate(DGEOS):
        for li, lens in enumerate(GROUPS):
            H, KV = HKV[(gi + li) % 3]
            forms = [("ragged", None)] + [("ext", p0) for p0 in EXT_POS0]
            for fi, (form, p0) in enumerate(forms):
                names = CAUSAL_MAPS if kind_or_target == "exact" else (KINDS[(gi + li + fi) % len(KINDS)],)
                for name in names:
                    n += 1
                    out.append(dict(form=form, lens=lens, vl_pos0=p0, H=H, KV=KV, D=D, Dout=Dout, causal=1, seed=300 + n, **{"target" if kind_or_target == "exact" else "kind": name}))
    if kind_or_target == "exact":                                      # two members share their prefix pages
        for ti, target in enumerate(CAUSAL_MAPS):
            out.append(dict(form="ext", lens=(65, 31, 129), vl_pos0=(192, 192, 64), share=(1, 0), H=4, KV=2, D=96, Dout=80, causal=1, seed=900 + ti, target=target))
    return out


def bounded_cases():
    out, n = [], 0
    for si, sh in enumerate(_single_shapes()):
        for ki, kind in enumerate(KINDS):
            n += 1
            D, Dout = DGEOS[(si + ki) % 4]
            H, KV = HKV[(si + 2 * ki) % 3]
            out.append(dict(form="single", B=1 + (si + ki) % 2, H=H, KV=KV, D=D, Dout=Dout, ring=(0, 2, 3)[(si + ki) % 3], kind=kind, seed=n, **sh))
    return out


def make(spec, device="cpu", **kw):
    return onehot_case(spec, device, **kw) if "target" in spec else bounded_case(spec, device, **kw)


# ---- the relocated cases: the same launches on pages whose offsets inside the pools need more than 32 bits ---------------------------------------------------------------
def relocated_cases():
    """-> [(spec, k)]: specs TAKEN FROM the lists above, to be laid out from the first page at or above 2^k elements of POOL_ELEMS pools (make_relocated).  k = 31: the
    caller's block table causal (ring 0 and 3) and full, a VL = 1 group of 8, VL = 2 groups of 8 and with a shared prefix, a dense bounded case; D 64 / 96 / 128 (page
    sizes that are and are not powers of two).  The hash / perm targets reach every page of every member.  k = 30: one more, byte offsets between 2^31 and 2^32."""
    ex, gr, bd = exact_cases(), group_cases("exact"), bounded_cases()

    def pick(lst, test=lambda s: True, **kw):
        return next(s for s in lst if all(s.get(k) == v for k, v in kw.items()) and test(s))

    return [(pick(ex, D=64, target="hash", qpos0=192, ring=0), 31),
            (pick(ex, D=128, target="hash", qpos0=960, test=lambda s: s["ring"] != 0), 31),
            (pick(ex, D=96, causal=0, target="perm"), 31),
            (pick(gr, form="ragged", D=128, lens=GROUPS[2], target="hash"), 31),
            (pick(gr, form="ext", D=64, Dout=32, lens=GROUPS[2], vl_pos0=EXT_POS0[0], target="hash"), 31),
            (pick(gr, share=(1, 0), target="hash"), 31),
            (pick(bd, D=96, kind="late_heavy", test=lambda s: s["qpos0"] >= 128), 31),
            (pick(gr, form="ext", D=128, lens=GROUPS[2], vl_pos0=EXT_POS0[0], target="diag"), 30)]


def make_relocated(spec, k, device="cpu", pools="sparse"):
    """make(spec) with its pages from the first one at or above 2^k elements of pools of POOL_ELEMS elements: pools = (Kt, Vt) flat bf16 tensors of that size, all NaN
    (they are viewed as [n_pages][KV][64][D]), or "sparse" (CPU)"""
    pe = spec["KV"] * 64 * spec["D"]
    n = POOL_ELEMS // pe
    if pools != "sparse":
        pools = (pools[0][:n * pe].view(n, spec["KV"], 64, spec["D"]), pools[1][:n * pe].view(n, spec["KV"], spec["D"], 64))
    return make(spec, device, first_page=first_page_above(1 << k, pe), pools=pools, n_pages=n)
