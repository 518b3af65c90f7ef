"""What the six descriptor entries of the operator level (gvl_op_patch_embed, gvl_op_decode_proj, gvl_op_decode_attention, gvl_op_qkv_post, gvl_op_prefill_attention,
gvl_op_iv2_attention) refuse and admit, as a plain list: per entry the refusals its own operator test already exercises (test_gpu_vision_ops.py, test_gpu_decode_proj.py,
test_gpu_decode_attn_exact.py, test_gpu_qkv_post.py, test_gpu_prefill_attn.py, test_gpu_iv2_attn.py -- the same base cases, the same one changed field each), then one
admitted launch of each base case.  tools/make_op_refusals.py runs the list against whichever libgvl.so is built and writes tests/golden/op_refusals.json: per case the
descriptor as the library saw it (a pointer as null or set with its low four address bits, the host copies of pos and the block tables), the status and the text behind
`failed (status N): `.  tests/test_gpu_op_refusals.py replays it on the GPU, tests/test_op_check_cpu.py replays the recorded descriptors against csrc/gvl_op_check.h
without one.

A case is (entry, name, keywords of the engine's op_* method, the tensors nothing may write when the call is refused).  Refusals write nothing, so every case of a base
shares the base's buffers; the admitted launches come last."""
import numpy as np
import torch

DEV = "cuda:0"
bf = torch.bfloat16
ENTRIES = ("patch_embed", "decode_proj", "decode_attention", "qkv_post", "prefill_attention", "iv2_attention")
HOST = {"decode_proj": ("pos", "tables"), "decode_attention": ("pos", "tables"), "qkv_post": ("block_table",), "prefill_attention": ("block_table",)}   # read back by the entry


def dev(t):
    return None if t is None else t.to(DEV)


# ---- gvl_op_patch_embed: test_gpu_vision_ops.py::test_patch_embed_refusals -------------------------------------------------------------------------------------------
def patch_embed_cases():
    import vision_ref as V
    out = []

    def attempt(name, mode, path, C, patch, image, T, Kp, n=1, **kw):
        g = image // patch
        S = 1 + T * g * g
        dt = torch.float32 if mode == 0 else bf
        buf, o = V.guarded(n * S, C, dt, DEV)
        z = lambda *s: torch.zeros(s, device=DEV)   # noqa: E731
        args = dict(bias=z(C) if mode == 1 else None, lnw=z(C) if mode == 0 else None, lnb=z(C) if mode == 0 else None)
        args.update(kw)
        out.append(("patch_embed", name, dict(mode=mode, path=path, px=z(n, 3, T, image, image), W=z(C, Kp).to(bf), cls=z(C).to(dt), pos=z(S, C).to(dt), out=o, patch=patch, **args), [buf]))
    attempt("C 768: no fused kernel", 1, 0, 768, 14, 14, 1, 640)
    attempt("patch 16", 1, 0, 1024, 16, 32, 1, 768)
    attempt("CLIP has no frames", 0, 0, 1024, 14, 14, 2, 640)
    attempt("CLIP at InternVideo2's width", 0, 0, 1408, 14, 14, 1, 640)
    attempt("three passes: Kp % 64", 1, 1, 1024, 14, 14, 1, 592)
    attempt("fused with im2col", 1, 0, 1024, 14, 14, 1, 640, im2col=torch.zeros((1, 640), dtype=bf, device=DEV))
    attempt("InternVideo2 without bias", 1, 1, 1024, 14, 14, 1, 640, bias=None)
    c = V.patch_cases()[0]                                   # the first case of the operator test's own list, by either path
    for path in (0, 1):
        buf, o = V.guarded(c.n * c.S, c.C, c.out_dtype(), DEV)
        d = {k: dev(getattr(c, k)) for k in ("px", "W", "bias", "cls", "pos", "lnw", "lnb")}
        im2col = V.guarded(c.M, c.Kp, bf, DEV)[1] if path else None
        out.append(("patch_embed", f"admitted: {c.name()} path {path}", dict(mode=c.mode, path=path, out=o, patch=c.patch, eps=c.eps, im2col=im2col, **d), None))
    return out


# ---- gvl_op_decode_proj: test_gemv_refuses_what_it_does_not_serve, test_documented_preconditions_are_refused -----------------------------------------------------
def decode_proj_cases():
    import decode_proj_ref as R
    FILL = -7776.0
    out = []
    c = R.exact_case(48, 1024, 5, "plain")
    W, o16 = dev(c.W), torch.full((16, 48), FILL, dtype=torch.float32, device=DEV)
    for B in (3, 5, 16):
        out.append(("decode_proj", f"gemv: batch {B}", dict(W=W, x=dev(c.x[:1].repeat(B, 1)), path=1, out_f32=o16), [o16]))
    x = dev(c.x[:4])
    sq = torch.ones((4, 64), dtype=torch.float32, device=DEV)
    t = torch.full((16 * 48,), FILL, dtype=bf, device=DEV)
    ob = torch.full((4, 48), FILL, dtype=bf, device=DEV)
    for name, kw in (("w_fmt 1", dict(w_fmt=1)), ("w_fmt 2", dict(w_fmt=2)), ("variant", dict(variant=1841)), ("sq_in", dict(sq_in=sq, sq_n=64)), ("sq_out", dict(sq_out=sq, out_bf16=ob)),
                     ("out_tiled2", dict(out_tiled2=t, out_bf16=ob)), ("out_tiled", dict(out_tiled=1, act=R.ACT_SILU_MUL, out_bf16=ob)), ("x_is_tiled", dict(x_is_tiled=1))):
        out.append(("decode_proj", "gemv: " + name, dict(W=W, x=x, path=1, out_f32=o16, **kw), [o16, sq, t, ob]))
    N = 48
    mk = lambda K, B=4: (dev(torch.ones((N, K), dtype=bf)), dev(torch.ones((B, K), dtype=bf)))   # noqa: E731
    y = torch.full((16, N), FILL, dtype=torch.float32, device=DEV)
    ob = torch.full((16, N), FILL, dtype=bf, device=DEV)
    sq = torch.full((16, 64), FILL, dtype=torch.float32, device=DEV)
    t = torch.full((16 * N,), FILL, dtype=bf, device=DEV)
    outs = [y, ob, sq, t]
    W, x = mk(1024)

    def add(name, Wx, **kw):
        out.append(("decode_proj", name, dict(W=Wx[0], x=Wx[1], **kw), outs))
    add("K 128", mk(128), out_f32=y)
    add("K 384", mk(384), out_f32=y)
    add("MXFP4: K % 1024", mk(2560), w_fmt=2, out_f32=y)
    add("FP8: K % 512", mk(768), w_fmt=1, out_f32=y)
    add("sq_in with FP8 weights", (W, x), w_fmt=1, sq_in=sq, sq_n=64, out_f32=y)
    add("sq_in with MXFP4 weights", (W, x), w_fmt=2, sq_in=sq, sq_n=64, out_f32=y)
    add("sq_n % 32", (W, x), sq_in=sq, sq_n=48, out_f32=y)
    add("sq_in with norm_w", (W, x), sq_in=sq, sq_n=64, norm_w=dev(torch.ones(1024, dtype=bf)), out_f32=y)
    add("out_tiled without SwiGLU", (W, x), out_tiled=1, out_bf16=ob)
    add("sq_out without the bf16 output", (W, x), sq_out=sq, out_f32=y)
    add("sq_out with SwiGLU", (W, x), sq_out=sq, out_bf16=ob, act=R.ACT_SILU_MUL)
    add("variant 1234", (W, x), variant=1234, out_f32=y)
    add("batch 17", (W, dev(torch.ones((17, 1024), dtype=bf))), out_f32=y)
    add("no output", (W, x))
    add("out_stride 50", (W, x), out_f32=y, out_stride=50)
    H, KV, D = 2, 1, 16
    tabs = [dev(torch.ones((8, 6), dtype=torch.float32)) for _ in range(4)]
    Q = torch.full((4, H * D), FILL, dtype=bf, device=DEV)
    Kt = torch.full((2, KV, 64, D), FILL, dtype=bf, device=DEV)
    Vt = torch.full((2, KV, D, 64), FILL, dtype=bf, device=DEV)
    pos, tables = dev(torch.tensor([0, 1, 2, 3], dtype=torch.int32)), dev(torch.zeros((4, 1), dtype=torch.int32))
    rk = dict(rope_on=1, cos_s=tabs[0], sin_s=tabs[1], cos_l=tabs[2], sin_l=tabs[3], max_pos=8, n_pages=2, pos=pos, tables=tables, table_stride=1, q_stride=H * D, Q=Q, Kt=Kt, Vt=Vt,
              H=H, KV=KV, D=D)
    rope = lambda name, Wx=(W, x), **kw: out.append(("decode_proj", "rope: " + name, dict(dict(rk, W=Wx[0], x=Wx[1]), **kw), [Q, Kt, Vt]))   # noqa: E731
    rope("odd Dr", Dr=11)
    rope("N != (H + 2 KV) Dr", Dr=10)
    rope("a position past the tables", Dr=12, pos=dev(torch.tensor([0, 1, 2, 8], dtype=torch.int32)))
    rope("a page past the pools", Dr=12, tables=dev(torch.tensor([[0], [1], [2], [0]], dtype=torch.int32)))
    rope("odd Dr with a matching N", (dev(torch.ones((2 * 1 * 11 * 2, 256), dtype=bf)), dev(torch.ones((4, 256), dtype=bf))), Dr=11)
    out.append(("decode_proj", "admitted: plain, N 48, K 1024, batch 4", dict(W=W, x=x, out_f32=y), None))
    return out


# ---- gvl_op_decode_attention: test_gpu_decode_attn_exact.py::test_refusals_write_nothing_and_a_good_launch_follows --------------------------------------------------
def decode_attention_cases():
    import decode_attn_ref as R
    from attn_ref import SENT
    c = R.onehot_case([257, 65], 4, 2, 64, 9, device=DEV)
    part = R.decoy_part(c, extra=1024, device=DEV)
    counters = torch.cat([torch.zeros(c.B * c.H, dtype=torch.int32), torch.full((64,), 0x5a5a5a5, dtype=torch.int32)]).to(DEV)
    o = torch.full((2 + 2, 256), SENT, dtype=bf, device=DEV)
    good = dict(q=c.q.view(2, 256).contiguous(), Kt=c.Kt, Vt=c.Vt, tables=c.tables, pos=c.pos, part=part, counters=counters, out=o, q_stride=256, n_pages=c.n_pages,
                table_stride=c.table_stride, out_stride=256, out_tiled=0, batch=2, H=4, KV=2, D=64, Dout=64, nsplit=16, hpb=0, cpb=0, gsplit=0, scale=1.0)
    tab_hi, tab_neg = c.tables.clone(), c.tables.clone()
    tab_hi[0, 4], tab_neg[1, 1] = c.n_pages, -1
    beyond = c.tables.clone()
    beyond[1, 2:] = c.n_pages + 5                      # entries BEHIND a sequence's pages are never read: no refusal
    refused = {
        "the plan: H % KV": dict(KV=3), "the plan: head dim": dict(D=80, Dout=80), "the plan: nsplit 17": dict(nsplit=17), "the plan: nsplit 0": dict(nsplit=0),
        "batch 17": dict(batch=17), "batch 0": dict(batch=0),
        "position -1": dict(pos=torch.tensor([256, -1], dtype=torch.int32, device=DEV)),
        "position behind the tables": dict(pos=torch.tensor([c.table_stride * 64, 64], dtype=torch.int32, device=DEV)),
        "page n_pages": dict(tables=tab_hi), "page -1": dict(tables=tab_neg),
        "gsplit * cpb below the split count": dict(gsplit=1, cpb=1),
        "Dout > D": dict(Dout=65), "Dout 0": dict(Dout=0), "q_stride short": dict(q_stride=248), "out_stride short": dict(out_stride=255),
        "no workspace": dict(part=None),
    }
    out = [("decode_attention", name, dict(good, **kw), [o, part, counters]) for name, kw in refused.items()]
    out.append(("decode_attention", "admitted: pages behind a sequence's own, gsplit at the exact minimum", dict(good, tables=beyond, gsplit=2, cpb=1), None))
    return out


# ---- gvl_op_qkv_post: test_gpu_qkv_post.py::test_refusals_write_nothing_and_a_good_launch_follows -------------------------------------------------------------------
def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(DEV).view(bf)


def qkv_post_cases():
    import qkv_post_ref as R

    def fields(c):
        im = R.Images(c)
        Q, Kt, Vt = _dev16(im.Q), _dev16(im.Kt), _dev16(im.Vt)
        q_rs = torch.from_numpy(im.q_rs.view(np.int32)).to(DEV).view(torch.float32)
        cos, sin = (torch.from_numpy(t).to(DEV) for t in (c.cos, c.sin)) if c.mode == 2 else (None, None)
        qn, kn = (_dev16(c.qn), _dev16(c.kn)) if c.mode == 1 else (None, None)
        kw = dict(qkv=_dev16(c.qkv), ld=c.ld, Q=Q, Kt=Kt, Vt=Vt if c.vt else None, block_table=torch.from_numpy(c.block_table).to(DEV) if c.block_table is not None else None,
                  max_pages=c.max_pages, B=c.B, S=c.S, H=c.H, KV=c.KV, Dr=c.Dr, D=c.D, mode=c.mode, qn=qn, kn=kn, eps=c.eps, cos=cos, sin=sin, pos0=c.pos0, ones_row=c.ones_row,
                  k_ones=c.k_ones, q_rs=q_rs if c.q_rs else None, n_pages=c.n_pages, max_pos=c.max_pos, ext=int(c.form == "ext"))
        if c.form != "single":
            kw.update(vl_n=len(c.members), vl_rows=[m.row0 for m in c.members] + [c.rows], vl_tables=[torch.tensor(m.table, dtype=torch.int32, device=DEV) for m in c.members],
                      vl_pos0=[m.pos0 for m in c.members])
        return kw, [Q, Kt, Vt, q_rs]

    single = R.build(dict(form="single", geo=(6, 2, 80, 96), mode=2, seed=901, B=2, S=65, pos0=64, table=True, vt=True, k_ones=1, ones_row=1, q_rs=False, ld_pad=16))
    plain = R.build(dict(form="single", geo=(4, 4, 64, 64), mode=0, seed=902, B=2, S=65, pos0=0, table=False, vt=True, k_ones=0, ones_row=0, q_rs=False, ld_pad=0))
    norm = R.build(dict(form="single", geo=(4, 4, 88, 96), mode=1, seed=903, B=1, S=5, pos0=0, table=False, vt=True, k_ones=1, ones_row=0, q_rs=True, ld_pad=0))
    group = R.build(dict(form="ext", geo=(4, 4, 64, 64), mode=2, seed=904, lens=(3, 65, 2), vl_pos0=(64, 0, 128), vt=True, k_ones=0, ones_row=0, q_rs=False, ld_pad=0))
    ragged = R.build(dict(form="ragged", geo=(4, 4, 64, 64), mode=2, seed=905, lens=(3, 65, 2), vl_pos0=None, vt=True, k_ones=0, ones_row=0, q_rs=False, ld_pad=0))
    base = {id(c): fields(c) for c in (single, plain, norm, group, ragged)}

    def tab(c, r, i, v):
        t = c.block_table.copy()
        t[r, i] = v
        return torch.from_numpy(t).to(DEV)

    def vtab(c, u, i, v):
        ts = [torch.tensor(m.table, dtype=torch.int32, device=DEV) for m in c.members]
        ts[u][i] = v
        return ts

    one_tile = torch.tensor(group.members[1].table[:1], dtype=torch.int32, device=DEV)
    refused = [
        # what the launchers refuse
        ("Dr % 8", single, dict(Dr=76)), ("mode 2: Dr % 16", single, dict(Dr=72)), ("D % 8", single, dict(D=100)), ("D < Dr", single, dict(D=72)), ("Dr > 128", plain, dict(Dr=136, D=136, H=1, KV=1)),
        ("ld % 8", single, dict(ld=single.ld + 4)), ("ld short", single, dict(ld=single.width - 8)), ("q_rs outside mode 1", plain, dict(q_rs=True, k_ones=1, D=72)),
        ("ragged: mode", ragged, dict(mode=0)), ("ragged: B", ragged, dict(B=2)), ("ragged: pos0", ragged, dict(pos0=64)), ("ragged: 9 members", ragged, dict(vl_n=9)),
        ("ext: no group", single, dict(ext=1)), ("ext: no Vt", group, dict(Vt=None)), ("ext: block_table", group, dict(block_table=torch.zeros(8, dtype=torch.int32, device=DEV), max_pages=8)),
        ("ext: vl_pos0 % 64", group, dict(vl_pos0=[64, 0, 100])), ("ext: vl_pos0 < 0", group, dict(vl_pos0=[-64, 0, 128])), ("ext: a member without a table", group, dict(vl_tables=[None] + vtab(group, 0, 0, 0)[1:], table_len=[2, 2, 4])),
        # what the entry adds
        ("page n_pages", single, dict(block_table=tab(single, 1, 2, single.n_pages))), ("page -1", single, dict(block_table=tab(single, 0, 1, -1))),
        ("implicit pages outside the pool", plain, dict(n_pages=3)),
        ("group: page n_pages", group, dict(vl_tables=vtab(group, 2, 2, group.n_pages))), ("ragged: page -1", ragged, dict(vl_tables=vtab(ragged, 1, 1, -1))),
        ("a page named twice", ragged, dict(vl_tables=vtab(ragged, 2, 0, ragged.members[1].table[1]))),
        ("position >= max_pos", single, dict(max_pos=single.pos0 + single.S - 1)), ("group: position >= max_pos", group, dict(max_pos=129)),
        ("table shorter than ceil((pos0 + S) / 64)", single, dict(max_pages=2)), ("group: table shorter", group, dict(vl_tables=[vtab(group, 0, 0, 0)[0], one_tile, vtab(group, 0, 0, 0)[2]])),
        ("Vt with pos0 % 64", single, dict(pos0=32)), ("pos0 > 0 without a table", plain, dict(pos0=64)), ("pos0 < 0", single, dict(pos0=-64)),
        ("vl_rows[0] != 0", ragged, dict(vl_rows=[1, 3, 68, 70])), ("an empty member", ragged, dict(vl_rows=[0, 3, 3, 70])), ("a member of negative length", group, dict(vl_rows=[0, 68, 3, 70])),
        ("q_rs without k_ones", norm, dict(k_ones=0)), ("ones_row with D == Dr", plain, dict(ones_row=1)), ("k_ones with D == Dr", plain, dict(k_ones=1)),
        ("mode 1 without qn", norm, dict(qn=None)), ("mode 1 without kn", norm, dict(kn=None)), ("mode 2 without cos", single, dict(cos=None)), ("mode 3", plain, dict(mode=3)),
        ("no Kt", plain, dict(Kt=None)), ("no Q and no q_rs", plain, dict(Q=None)), ("S 0", plain, dict(S=0)), ("n_pages 0", plain, dict(n_pages=0)),
    ]
    out = []
    for name, c, kw in refused:
        f, outs = base[id(c)]
        if kw.get("q_rs") is True:
            kw = dict(kw, q_rs=outs[3])
        out.append(("qkv_post", name, dict(f, **kw), outs))
    for what, c in (("single", single), ("plain", plain), ("norm", norm), ("group", group), ("ragged", ragged)):
        out.append(("qkv_post", "admitted: " + what, base[id(c)][0], None))
    return out


# ---- gvl_op_prefill_attention: test_gpu_prefill_attn.py::test_refusals_write_nothing_and_a_good_launch_follows ------------------------------------------------------
def prefill_attention_cases():
    import prefill_attn_ref as P
    from attn_ref import SENT

    def fields(c):
        O = torch.full((c.rows + P.GUARD_ROWS, c.H * c.Dr), SENT, dtype=bf, device=DEV)
        kw = dict(Q=c.Q, Kt=c.Kt, Vt=c.Vt, O=O, B=c.B, H=c.H, KV=c.KV, S=c.S, D=c.D, Dout=c.Dr, Sk=c.Sk, qpos0=c.qpos0, scale=c.scale, causal=c.causal, ring=c.ring, n_pages=c.n_pages,
                  ext=int(c.form == "ext"))
        if c.form == "single":
            kw.update(block_table=c.block_table, max_pages=c.block_table.shape[1])
        else:
            kw.update(vl_n=len(c.members), vl_rows=[m.row0 for m in c.members] + [c.rows], vl_tables=c.tables, vl_pos0=[m.qpos0 for m in c.members])
        return kw, [O]

    single = P.make(dict(form="single", B=2, S=65, qpos0=64, Sk=129, H=4, KV=2, D=96, Dout=80, causal=1, ring=0, target="hash", seed=41), DEV)
    full = P.make(dict(form="single", B=1, S=65, qpos0=0, Sk=200, H=4, KV=2, D=64, Dout=64, causal=0, ring=0, target="perm", seed=42), DEV)
    group = P.make(dict(form="ext", lens=(65, 31, 129), vl_pos0=(64, 0, 192), H=4, KV=4, D=64, Dout=64, causal=1, seed=43, target="hash"), DEV)
    ragged = P.make(dict(form="ragged", lens=(65, 31, 129), vl_pos0=None, H=4, KV=4, D=64, Dout=64, causal=1, seed=44, target="hash"), DEV)
    base = {id(c): fields(c) for c in (single, full, group, ragged)}

    def tab(c, r, i, v):
        t = c.block_table.clone()
        t[r, i] = v
        return t

    def vtab(c, u, i, v):
        ts = [t.clone() for t in c.tables]
        ts[u][i] = v
        return ts

    refused = [
        # what attn_plan / attn_ext_plan refuse
        ("D 80", single, dict(D=80)), ("Dout % 8", single, dict(Dout=76)), ("Dout > D", single, dict(Dout=104)), ("H % KV", single, dict(KV=3)), ("S 0", single, dict(S=0)),
        ("Sk < qpos0 + S", single, dict(Sk=128)), ("qpos0 without Sk", single, dict(Sk=0)), ("qpos0 < 0", single, dict(qpos0=-64)), ("more than 256 key tiles", full, dict(Sk=256 * 64 + 1)),
        ("ragged: not causal", ragged, dict(causal=0)), ("ragged: B 2", ragged, dict(B=2)), ("ragged: Sk", ragged, dict(Sk=200)), ("ragged: qpos0", ragged, dict(qpos0=64)),
        ("ragged: block_table", ragged, dict(block_table=ragged.tables[0], max_pages=2)), ("ragged: a member longer than S", ragged, dict(S=128)),
        ("ragged: an empty member", ragged, dict(vl_rows=[0, 65, 65, 225])), ("ragged: vl_rows[0] != 0", ragged, dict(vl_rows=[1, 65, 96, 225])), ("9 members", ragged, dict(vl_n=9)),
        ("ext: not causal", group, dict(causal=0)), ("ext: vl_pos0 % 64", group, dict(vl_pos0=[64, 0, 100])), ("ext: vl_pos0 < 0", group, dict(vl_pos0=[-64, 0, 192])),
        ("ext: a member without a table", group, dict(vl_tables=[None] + group.tables[1:], table_len=[3, 2, 7])), ("ext: no group", single, dict(ext=1)),
        ("ext: vl_rows[0] != 0", group, dict(vl_rows=[1, 65, 96, 225])), ("ext: more than 256 key tiles", group, dict(vl_pos0=[64, 0, 256 * 64])),
        # what the entry adds
        ("single: no block table", single, dict(block_table=None)), ("ring 4", single, dict(ring=4)), ("no O", single, dict(O=None)), ("n_pages 0", single, dict(n_pages=0)),
        ("page n_pages", single, dict(block_table=tab(single, 1, 2, single.n_pages))), ("page -1", single, dict(block_table=tab(single, 0, 0, -1))),
        ("non-causal: page of the last tile", full, dict(block_table=tab(full, 0, 3, full.n_pages))),
        ("group: page n_pages in the prefix", group, dict(vl_tables=vtab(group, 2, 0, group.n_pages))), ("ragged: page -1", ragged, dict(vl_tables=vtab(ragged, 1, 0, -1))),
        ("table shorter than the key tiles", single, dict(max_pages=2)), ("non-causal: table shorter than ceil(Sk / 64)", full, dict(max_pages=3)),
        ("group: table shorter", group, dict(vl_tables=[group.tables[0], group.tables[1], group.tables[2][:5].contiguous()])),
    ]
    out = [("prefill_attention", name, dict(base[id(c)][0], **kw), base[id(c)][1]) for name, c, kw in refused]
    out.append(("prefill_attention", "admitted: single, a spare entry behind a sequence's tiles", dict(base[id(single)][0], block_table=tab(single, 1, 3, -5)), None))
    for what, c in (("single", single), ("full", full), ("group", group), ("ragged", ragged)):
        out.append(("prefill_attention", "admitted: " + what, base[id(c)][0], None))
    return out


# ---- gvl_op_iv2_attention: test_gpu_iv2_attn.py::test_refusals_write_nothing_and_a_good_launch_follows --------------------------------------------------------------
def iv2_attention_cases():
    import iv2_attn_ref as R
    spec = next(s for s in R.cases() if s["what"] == "perm" and s["S"] == 129)
    c_cpu = R.build(spec)
    c = R.to_device(c_cpu, DEV)
    B, S, H, Dr = c.B, c.S, c.H, c.Dr
    rows = B * S
    alloc = torch.full((rows + 64, c.ld), float("nan"), dtype=bf, device=DEV)
    alloc[:rows, :H * Dr] = c.x.reshape(rows, H * Dr)
    alloc[:rows, 2 * H * Dr:3 * H * Dr] = c.v.reshape(rows, H * Dr)
    rs = torch.full((rows + 64,), float("nan"), dtype=torch.float32, device=DEV)
    rs[:rows] = c.q_rs.reshape(-1)
    pg = R.pages(c_cpu)
    Q, Kt, Vt = (torch.from_numpy(pg[k].view(np.int16).copy()).to(DEV).view(bf) for k in ("Q", "Kt", "Vt"))
    nw = c.q_nw.contiguous()
    buf = torch.full((rows + R.GUARD, H * Dr), R.SENT, dtype=bf, device=DEV)

    def fields(form, pipe=0, pipe_rows=0):
        kw = dict(Kt=Kt, B=B, S=S, H=H, Dr=Dr, scale=c.scale, form=form, out=buf)
        if form == 0:
            kw.update(Q=Q, Vt=Vt)
        elif form == 1:
            kw.update(Q=Q, qkv=alloc[:rows], ld=c.ld)
        else:
            kw.update(qkv=alloc[:rows], ld=c.ld, q_rs=rs[:rows], q_nw=nw, pipe=pipe, pipe_rows=pipe_rows)
        return kw

    odd = lambda t: t.reshape(-1)[1:]                                       # 2 bytes in   # noqa: E731
    refused = [
        ("form 3", 2, dict(form=3)), ("form -1", 2, dict(form=-1)), ("no Kt", 2, dict(Kt=None)), ("no out", 2, dict(out=None)),
        ("form 0 without Q", 0, dict(Q=None)), ("form 0 without Vt", 0, dict(Vt=None)), ("form 0 with qkv", 0, dict(qkv=alloc[:rows], ld=c.ld)),
        ("form 0 with q_rs", 0, dict(q_rs=rs[:rows])), ("form 0 with q_nw", 0, dict(q_nw=nw)),
        ("form 1 without Q", 1, dict(Q=None)), ("form 1 without qkv", 1, dict(qkv=None)), ("form 1 with Vt", 1, dict(Vt=Vt)), ("form 1 with q_rs", 1, dict(q_rs=rs[:rows])),
        ("form 1 with q_nw", 1, dict(q_nw=nw)),
        ("form 2 without qkv", 2, dict(qkv=None)), ("form 2 without q_rs", 2, dict(q_rs=None)), ("form 2 without q_nw", 2, dict(q_nw=None)), ("form 2 with Q", 2, dict(Q=Q)),
        ("form 2 with Vt", 2, dict(Vt=Vt)),
        ("B 0", 2, dict(B=0)), ("S 0", 1, dict(S=0)), ("H 0", 0, dict(H=0)), ("Dr 64", 0, dict(Dr=64)), ("Dr 96", 1, dict(Dr=96)), ("Dr 84", 0, dict(Dr=84)), ("form 2 at Dr 80", 2, dict(Dr=80)),
        ("pipe 3", 2, dict(pipe=3)), ("pipe -1", 2, dict(pipe=-1)), ("pipe_rows 128", 2, dict(pipe=1, pipe_rows=128)), ("pipe_rows 512", 2, dict(pipe=1, pipe_rows=512)),
        ("ld % 8", 2, dict(ld=c.ld + 4)), ("ld < 3 H Dr", 1, dict(ld=3 * H * Dr - 8)), ("more than 256 key tiles", 2, dict(S=256 * 64 + 1)),
        ("more than 256 key tiles, form 0", 0, dict(S=256 * 64 + 1)), ("qkv 2 bytes off", 2, dict(qkv=odd(alloc))), ("q_nw 2 bytes off", 2, dict(q_nw=odd(nw))),
        ("V rows 2 bytes off", 1, dict(qkv=odd(alloc))), ("out 2 bytes off", 2, dict(out=odd(buf))),
    ]
    out = [("iv2_attention", name, dict(fields(form, 1, 0), **kw), [buf]) for name, form, kw in refused]
    for f, pipe, pr in R.launches(c):
        out.append(("iv2_attention", f"admitted: form {f} pipe {pipe} pipe_rows {pr}", fields(f, pipe, pr), None))
    return out


def cases():
    """-> [(entry, name, keywords, outputs or None)] on the GPU; outputs None: a launch the operator tests run, expected to be admitted"""
    return patch_embed_cases() + decode_proj_cases() + decode_attention_cases() + qkv_post_cases() + prefill_attention_cases() + iv2_attention_cases()


# ---- the descriptor as the library sees it, and the call ------------------------------------------------------------------------------------------------------------
def describe(entry, kw):
    """-> (fields, host): ints as they are, floats left out (no entry refuses one), a pointer {"set": low four address bits} (null: absent), vl_tables a list of those
    or None; host: the int32 arrays the entry reads back, flat"""
    kw = dict(kw)
    if entry == "decode_proj":
        W, x = kw["W"], kw["x"]
        kw.update(N=W.shape[0], K=W.shape[1], batch=int(kw.get("batch", x.shape[0])))
    if entry == "patch_embed":
        n, _, T, image, _ = kw["px"].shape
        kw.update(n=n, T=T, image=image, C=kw["W"].shape[0], Kp=kw["W"].shape[1])
    if kw.get("vl_tables") is not None and "table_len" not in kw:
        kw["table_len"] = [int(t.numel()) for t in kw["vl_tables"]]
    ptr = lambda t: None if t is None else {"set": t.data_ptr() & 15}   # noqa: E731
    fields, host = {}, {}
    for k, v in kw.items():
        if v is None or isinstance(v, float):
            continue
        if k == "vl_tables":
            fields[k] = [ptr(t) for t in v]
            host[k] = [None if t is None else t.cpu().reshape(-1).tolist() for t in v]
        elif torch.is_tensor(v):
            fields[k] = ptr(v)
            if k in HOST.get(entry, ()):
                host[k] = v.cpu().reshape(-1).tolist()
        elif isinstance(v, (list, tuple)):
            fields[k] = [int(x) for x in v]
        else:
            fields[k] = int(v)
    return fields, host


def call(eng, entry, kw):
    """-> (status, text behind `failed (status N): `)"""
    from grounded_video_llm_amd import lib as L
    kw = dict(kw)
    try:
        if entry == "patch_embed":
            a = [kw.pop(k) for k in ("mode", "path", "px", "W", "cls", "pos", "out", "patch")]
            eng.op_patch_embed(*a, **kw)
        elif entry == "decode_proj":
            eng.op_decode_proj(kw.pop("W"), kw.pop("x"), **kw)
        else:
            getattr(eng, "op_" + entry)(**kw)
    except L.GvlError as e:
        torch.cuda.synchronize()
        return e.status, str(e).split("): ", 1)[1]
    torch.cuda.synchronize()
    return 0, ""


def replay(eng, on_case):
    """every case in order; on_case(index, entry, name, fields, host, status, text, untouched) -- untouched: None for an admitted call, else whether every output of a
    refused call still holds the bytes it held"""
    for i, (entry, name, kw, outs) in enumerate(cases()):
        fields, host = describe(entry, kw)
        before = [o.clone() for o in outs] if outs else []
        status, text = call(eng, entry, kw)
        same = None if status == 0 else all(torch.equal(o.view(torch.uint8), b.view(torch.uint8)) for o, b in zip(outs or [], before))
        on_case(i, entry, name, fields, host, status, text, same)
