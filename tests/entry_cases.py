"""What the sequence entries of include/gvl.h refuse and admit, as a plain list: one small LLM, one set of sequence states, and every prefill / decode entry, the three
searches, gvl_seq_fork / gvl_seq_clone / gvl_seq_fanout called on each of them.  tools/make_entry_refusals.py runs the list against whichever libgvl.so is built and
writes tests/golden/entry_refusals.json (status and whole message of every call); tests/test_gpu_entry_refusals.py replays it on the GPU, tests/test_admit_cpu.py
replays the same states against the pure admission function (csrc/gvl_admit.h) without one.

Every case runs against a freshly built SETUP (a call that was admitted is followed by a teardown and a rebuild), so one description of the table serves all cases.
Sequence ids are the slot numbers the table hands out in SETUP's order; NAMES gives them names.

The pool holds 288 pages, not a few dozen: "one slot too few" needs 254 live sequences, and every live sequence owns at least one page."""
import ctypes as C

GEO = dict(llm="phi3.5", hidden=64, inter=128, layers=2, heads=4, kv_heads=4, vocab=100, max_seq=512, max_prefill=128, kv_pages=288)
MAX_SEQS, OUTLIST_CAP, VOCAB = 256, 8192, GEO["vocab"]

# ---- the states: (op, args...) in order; alloc / fork take the next free slot, which is the id written behind `#`
SETUP = [
    ("alloc", 256),                 # 0 empty
    ("alloc", 256),                 # 1 p64: 64 rows, a whole page
    ("prefill", 1, 64),
    ("alloc", 256),                 # 2 p70: 70 rows, a partial page
    ("prefill", 2, 70),
    ("fork", 1, 64, 256),           # 3 fork64: pos 64, n_gen 0
    ("alloc", 128),                 # 4 lead
    ("prefill", 4, 8),
    ("alloc", 128),                 # 5 foll
    ("prefill", 5, 8),
    ("guide", 4, 5),
    ("alloc", 128),                 # 6 kh_empty: keeps its hidden states, empty
    ("keep_hidden", 6),
    ("alloc", 128),                 # 7 kh_pre: keeps its hidden states, 20 rows
    ("keep_hidden", 7),
    ("prefill", 7, 20),
    ("alloc", 256),                 # 8 empty2: a good first member of the prefill entries
    ("alloc", 256),                 # 9 p64b: a good first member of the decode entries
    ("prefill", 9, 64),
    ("fork", 9, 64, 256),           # 10 fork64b: a good first member of the extend entries
    ("alloc", 64),                  # 11 p8: 8 rows in a capacity of 64
    ("prefill", 11, 8),
    ("alloc", 64),                  # 12 e64: empty, capacity 64 < max_prefill
    ("fork", 1, 64, 128),           # 13 fork_small: pos 64 in a capacity of 128
    ("alloc", 8),                   # 14 full: 8 rows in a capacity of 8
    ("prefill", 14, 8),
    ("alloc", 64),                  # 15 freed
    ("free", 15),
]
NAMES = dict(empty=0, p64=1, p70=2, fork64=3, lead=4, foll=5, kh_empty=6, kh_pre=7, empty2=8, p64b=9, fork64b=10, p8=11, e64=12, fork_small=13, full=14, freed=15,
             minus1=-1, id77=77)
# the states every entry meets as its only member and behind a good first one
STATES = ["empty", "p64", "p70", "fork64", "lead", "foll", "kh_empty", "kh_pre", "freed", "minus1", "id77"]
# further set-ups for the all-or-nothing opens: SETUP, then the pool or the slots filled until `n` are free
SETUPS = {"base": SETUP}
for _what in ("pages", "slots"):
    for _n in (2, 3):
        SETUPS[f"{_what}_free_{_n}"] = SETUP + [(f"fill_{_what}", _n)]

SINGLE = {"prefill": 8, "prefill_extend": 8, "forward_loss": 8, "decode_step_logits": 5}          # entry -> the length / token of a plain call
BATCH = {"prefill_varlen": ("empty2", 8), "prefill_extend_varlen": ("fork64b", 8), "score_extend_varlen": ("fork64b", 8), "decode_greedy_batch": ("p64b", 3),
         "decode_steps": ("p64b", 2), "decode_step_logits_batch": ("p64b", 5)}                    # entry -> (a good first member, the length / count / token)
PER_MEMBER = ("prefill_varlen", "prefill_extend_varlen", "score_extend_varlen", "decode_step_logits_batch")   # batch entries whose number is per member
SEARCHES = ("beam_search", "group_beam_search", "contrastive_search")


def _batch(fn, names, x):
    return (fn, list(names), list(x) if isinstance(x, (list, tuple)) else ([x] * len(names) if fn in PER_MEMBER else x))


def cases():
    """-> [(setup name, call)]; a call is (entry, seq name or [names], number or [numbers], ...)"""
    out = []
    for fn, x in SINGLE.items():
        out += [("base", (fn, s, x)) for s in STATES]
    for fn, (good, x) in BATCH.items():
        out += [("base", _batch(fn, [s], x)) for s in STATES]
        out += [("base", _batch(fn, [good, s], x)) for s in STATES]
        out.append(("base", _batch(fn, [good, good], x)))
    # ---- the length edges: 0, max_prefill + 1, capacity + 1, pos + n_new one past the capacity (and the last length that fits)
    for fn in ("prefill", "forward_loss"):
        out += [("base", (fn, "empty", n)) for n in (0, 129, 128)] + [("base", (fn, "e64", n)) for n in (65, 64)]
    out += [("base", ("prefill_extend", "fork64", n)) for n in (0, 129, 128)] + [("base", ("prefill_extend", "fork_small", n)) for n in (65, 64)]
    out += [("base", ("prefill_varlen", ["empty"], [n])) for n in (0, 129, 128)] + [("base", ("prefill_varlen", ["e64"], [n])) for n in (65, 64)]
    out += [("base", ("prefill_varlen", ["empty2", "e64"], [8, 65])), ("base", ("prefill_varlen", ["empty2", "empty"], [8, 0]))]
    for fn in ("prefill_extend_varlen", "score_extend_varlen"):
        out += [("base", (fn, ["fork64"], [n])) for n in (0, 129, 128)] + [("base", (fn, ["fork_small"], [n])) for n in (65, 64)]
        out += [("base", (fn, ["e64"], [n])) for n in (65, 64)] + [("base", (fn, ["fork64b", "fork_small"], [8, 65]))]
    out += [("base", ("decode_greedy_batch", ["p64b"], n)) for n in (0, OUTLIST_CAP + 1)]
    out += [("base", ("decode_steps", ["p8"], n)) for n in (0, 57, 56)] + [("base", ("decode_steps", ["p64b", "p8"], 57)), ("base", ("decode_steps", ["full"], 1))]
    out += [("base", ("decode_greedy_batch", ["full"], 3))]
    for tok in (-1, VOCAB, VOCAB - 1):
        out += [("base", ("decode_step_logits", "p64", tok)), ("base", ("decode_step_logits_batch", ["p64b", "p64"], [5, tok]))]
    out += [("base", ("decode_step_logits", "full", 5)), ("base", ("decode_step_logits_batch", ["p64b", "full"], [5, 5]))]
    # ---- two faults in one call: which check wins
    out += [("base", ("prefill_extend", "p70", 0)), ("base", ("prefill_extend", "foll", 0)), ("base", ("prefill_extend", "kh_pre", 0)),
            ("base", ("prefill", "p64", 0)), ("base", ("forward_loss", "kh_pre", 0)), ("base", ("forward_loss", "p64", 129)),
            ("base", ("prefill_varlen", ["empty2", "empty2"], [8, 0])), ("base", ("prefill_varlen", ["p64", "p64"], [8, 8])), ("base", ("prefill_varlen", ["kh_empty"], [0])),
            ("base", ("prefill_varlen", ["p64"], [129])), ("base", ("prefill_varlen", ["id77", "empty"], [0, 0])),
            ("base", ("prefill_extend_varlen", ["fork64b", "fork64b"], [8, 0])), ("base", ("prefill_extend_varlen", ["p70", "p70"], [8, 8])),
            ("base", ("prefill_extend_varlen", ["foll", "kh_pre"], [0, 0])), ("base", ("score_extend_varlen", ["p70"], [0])),
            ("base", ("score_extend_varlen", ["fork64b", "lead", "lead"], [8, 8, 8])),
            ("base", ("decode_greedy_batch", ["empty", "empty"], 3)), ("base", ("decode_greedy_batch", ["foll"], OUTLIST_CAP + 1)), ("base", ("decode_greedy_batch", ["kh_empty"], 3)),
            ("base", ("decode_steps", ["fork64"], 500)), ("base", ("decode_steps", ["p8", "p8"], 57)), ("base", ("decode_steps", ["kh_pre", "foll"], 2)),
            ("base", ("decode_step_logits", "lead", -1)), ("base", ("decode_step_logits", "foll", VOCAB)), ("base", ("decode_step_logits", "kh_empty", 5)),
            ("base", ("decode_step_logits_batch", ["p64", "p64"], [5, -1])), ("base", ("decode_step_logits_batch", ["empty", "empty"], [5, 5])),
            ("base", ("decode_step_logits_batch", ["kh_pre", "kh_pre"], [5, 5]))]
    # ---- the searches, the copies and the fan-out on every state
    for fn in SEARCHES:
        out += [("base", (fn, s)) for s in STATES]
    out += [("base", ("seq_fork", s, 64, 256)) for s in STATES] + [("base", ("seq_fork", "p64", n, 256)) for n in (0, 32, 128)] + [("base", ("seq_fork", "p64", 64, m)) for m in (64, 513)]
    out += [("base", ("seq_clone", s, 256)) for s in STATES] + [("base", ("seq_clone", "p70", m)) for m in (70, 71, 513)]
    out += [("base", ("seq_fanout", s, 2, 256)) for s in STATES] + [("base", ("seq_fanout", "p70", n, 256)) for n in (0, 16, 15)] + [("base", ("seq_fanout", "p70", 2, m)) for m in (70, 513)]
    # ---- all or nothing: 3 siblings / 1 + 3 clones of a search with one page or one slot too few, and with exactly enough
    for what in ("pages", "slots"):
        out += [(f"{what}_free_2", ("seq_fanout", "p70", 3, 128)), (f"{what}_free_3", ("seq_fanout", "p70", 3, 128))]
        out += [(f"{what}_free_3", ("contrastive_search", "kh_pre")), (f"{what}_free_3", ("beam_search", "p70"))]
    return out


# ---- running the list on an engine -------------------------------------------------------------------------------------------------------------------------
def make_engine():
    import torch  # noqa: F401
    from grounded_video_llm_amd import engine as E, synth, weights as Wt
    kw = dict(GEO)
    kw["rope_short"], kw["rope_long"] = synth.longrope_factors(GEO["hidden"] // GEO["heads"])
    geo = E.TowerGeometry(clip_hidden=64, clip_inter=128, clip_layers=3, clip_heads=4, clip_image=28, clip_patch=14, iv2_dim=64, iv2_inter=128, iv2_depth=4, iv2_heads=4,
                          iv2_image=28, iv2_patch=14, frames_per_seg=2, max_segs=2, **kw)
    W = synth.llm_weights("phi3", GEO["hidden"], GEO["inter"], GEO["layers"], GEO["heads"], GEO["kv_heads"], GEO["vocab"], True, seed="t.entries", device="cuda:0")
    eng = E.Engine(geo, "cuda:0", towers=("llm",))
    eng.load_packed(Wt.pack_llm(W, geo.kind, geo.layers, geo.heads, geo.kv_heads, geo.max_seq, geo.rope_theta, geo.rope_short, geo.rope_long, geo.rope_max_pos, geo.rope_orig_max_pos))
    eng.finalize()
    return eng


class Runner:
    """builds a set-up on `eng`, runs calls through the raw ABI -> (status, text behind `failed (status N): `), tears down"""

    def __init__(self, eng):
        import torch
        self.eng, self.live, self.setup = eng, [], None
        g = torch.Generator().manual_seed(11)
        self.x = (torch.randn((129, GEO["hidden"]), generator=g) * 0.5).to(torch.bfloat16).to(eng.device)
        self.row = torch.linspace(-2.0, 2.0, VOCAB, dtype=torch.float32, device=eng.device)
        self.total = eng.kv_info()["total_pages"]

    def build(self, name):
        import torch
        eng = self.eng
        assert not self.live and eng.kv_info()["free_pages"] == self.total
        lg = {}
        for op, *a in SETUPS[name]:
            if op == "alloc":
                self.live.append(eng.seq_alloc(a[0]))
            elif op == "fork":
                self.live.append(eng.seq_fork(*a))
            elif op == "prefill":
                lg[a[0]] = eng.prefill(a[0], self.x[:a[1]], want_logits=True)
            elif op == "keep_hidden":
                eng.seq_keep_hidden(a[0])
            elif op == "guide":
                eng.seq_set_guidance(a[0], a[1], 1.5, lg[a[0]], lg[a[1]])
            elif op == "free":
                eng.seq_free(a[0])
                self.live.remove(a[0])
            elif op == "fill_pages":                    # sequences of up to 8 pages until a[0] pages are free
                while (free := eng.kv_info()["free_pages"]) > a[0]:
                    self.live.append(eng.seq_alloc(64 * min(free - a[0], 8)))
            elif op == "fill_slots":                    # one-page sequences until a[0] slots are free
                while MAX_SEQS - len(self.live) > a[0]:
                    self.live.append(eng.seq_alloc(64))
            else:
                raise ValueError(op)
        assert self.live[:15] == list(range(15)), self.live[:15]
        torch.cuda.synchronize()
        self.setup = name

    def teardown(self, extra=()):
        for s in sorted(set(self.live) | set(extra)):   # a leader goes before its follower: its id is the smaller one
            self.eng.seq_free(s)
        self.live, self.setup = [], None
        assert self.eng.kv_info()["free_pages"] == self.total

    def members(self, call):
        """the live sequences a call names"""
        names = call[1] if isinstance(call[1], list) else [call[1]]
        return sorted({NAMES[n] for n in names} & set(self.live))

    def snapshot(self, ids):
        return self.eng.kv_info(), {s: (self.eng.seq_pages(s), self.eng.seq_read(s)) for s in ids}

    def run(self, call):
        """-> (status, text, ids of the sequences the call opened)"""
        from grounded_video_llm_amd import lib as L
        from grounded_video_llm_amd.engine import _ptr
        eng, lib, st, x = self.eng, self.eng.lib, self.eng.stream, self.x
        fn = call[0]
        opened = []
        if isinstance(call[1], list):
            n = len(call[1])
            ids = (C.c_int * n)(*[NAMES[s] for s in call[1]])
            nums = call[2] if isinstance(call[2], list) else None
            ptrs = (C.c_void_p * n)(*[x.data_ptr()] * n)
            lens = (C.c_int * n)(*nums) if nums else None
        if fn == "prefill":
            rc = lib.gvl_prefill(eng.ctx, NAMES[call[1]], _ptr(x), call[2], None, st)
        elif fn == "prefill_extend":
            rc = lib.gvl_prefill_extend(eng.ctx, NAMES[call[1]], _ptr(x), call[2], None, st)
        elif fn == "forward_loss":
            lab, nll, nv = (C.c_int64 * max(call[2], 1))(*[1] * max(call[2], 1)), C.c_double(0.0), C.c_int(0)
            rc = lib.gvl_forward_loss(eng.ctx, NAMES[call[1]], _ptr(x), call[2], lab, C.byref(nll), C.byref(nv), st)
        elif fn == "prefill_varlen":
            rc = lib.gvl_prefill_varlen(eng.ctx, ids, n, ptrs, lens, st)
        elif fn == "prefill_extend_varlen":
            rc = lib.gvl_prefill_extend_varlen(eng.ctx, ids, n, ptrs, lens, None, st)
        elif fn == "score_extend_varlen":
            import torch
            tg = [(C.c_int32 * max(m, 1))(*[1] * max(m, 1)) for m in nums]
            tgp = (C.POINTER(C.c_int32) * n)(*[C.cast(t, C.POINTER(C.c_int32)) for t in tg])
            room = max(sum(max(m, 0) for m in nums), 1)
            lp, rank, got = torch.empty((room,), dtype=torch.float32, device=eng.device), torch.empty((room,), dtype=torch.int32, device=eng.device), C.c_int(-1)
            rc = lib.gvl_score_extend_varlen(eng.ctx, ids, n, ptrs, lens, tgp, 0, _ptr(lp), _ptr(rank), None, None, C.byref(got), None, st)
        elif fn == "decode_greedy_batch":
            buf, nout = (C.c_int32 * (n * max(min(call[2], 16), 1)))(), (C.c_int * n)()
            assert call[2] <= 16 or call[2] > OUTLIST_CAP            # (the room handed over is for an admitted call)
            rc = lib.gvl_decode_greedy_batch(eng.ctx, ids, n, call[2], -1, buf, nout, st)
        elif fn == "decode_steps":
            rc = lib.gvl_decode_steps(eng.ctx, ids, n, call[2], st)
        elif fn == "decode_step_logits":
            rc = lib.gvl_decode_step_logits(eng.ctx, NAMES[call[1]], call[2], None, st)
        elif fn == "decode_step_logits_batch":
            rc = lib.gvl_decode_step_logits_batch(eng.ctx, ids, n, (C.c_int32 * n)(*nums), None, st)
        elif fn in SEARCHES:
            k, max_new = (4, 2) if fn == "contrastive_search" else (2, 2)
            out, no, score, ts = (C.c_int32 * max_new)(), (C.c_int * 1)(), (C.c_double * 1)(), (C.c_float * max_new)()
            base = L.GvlBeamParams(k, max_new, -1, 1.0, 0, 1.0, 0, 0, -1, -1)
            if fn == "beam_search":
                rc = lib.gvl_beam_search_n(eng.ctx, NAMES[call[1]], _ptr(self.row), C.byref(base), 1, out, max_new, no, score, ts, st)
            elif fn == "group_beam_search":
                prm = L.GvlGroupBeamParams(base, 2, 1.0, -1)
                rc = lib.gvl_group_beam_search(eng.ctx, NAMES[call[1]], _ptr(self.row), C.byref(prm), 1, out, max_new, no, score, ts, st)
            else:
                prm = L.GvlContrastiveParams(k, 0.6, max_new, -1, 1.0, 0, 0, -1, -1)
                rc = lib.gvl_contrastive_search(eng.ctx, NAMES[call[1]], _ptr(self.row), C.byref(prm), out, max_new, no, None, None, None, None, None, None, st)
        elif fn == "seq_fork":
            sid = C.c_int(-1)
            rc = lib.gvl_seq_fork(eng.ctx, NAMES[call[1]], call[2], call[3], C.byref(sid))
            opened = [sid.value] if rc == 0 else []
        elif fn == "seq_clone":
            sid = C.c_int(-1)
            rc = lib.gvl_seq_clone(eng.ctx, NAMES[call[1]], call[2], C.byref(sid), st)
            opened = [sid.value] if rc == 0 else []
        elif fn == "seq_fanout":
            m = max(call[2], 1)
            sids, streams, first = (C.c_int * m)(), (C.c_uint32 * m)(*range(1, m + 1)), self.row.clone()
            rc = lib.gvl_seq_fanout(eng.ctx, NAMES[call[1]], call[2], call[3], streams, _ptr(first), sids, st)
            opened = [int(sids[i]) for i in range(call[2])] if rc == 0 else []
        else:
            raise ValueError(fn)
        msg = lib.gvl_last_error(eng.ctx)
        if rc == 0:
            import torch
            torch.cuda.synchronize()
        return rc, (msg.decode() if msg and rc != 0 else ""), opened

    def replay(self, on_case):
        """every case on its set-up; on_case(index, setup, call, status, text, before, after) with the snapshots of a refused call's members (None when admitted)"""
        for i, (setup, call) in enumerate(cases()):
            if self.setup != setup:
                if self.setup is not None:
                    self.teardown()
                self.build(setup)
            ids = self.members(call)
            before = self.snapshot(ids)
            rc, text, opened = self.run(call)
            if rc == 0:
                on_case(i, setup, call, rc, text, None, None)
                self.teardown(opened)
            else:
                on_case(i, setup, call, rc, text, before, self.snapshot(ids))
        if self.setup is not None:
            self.teardown()
