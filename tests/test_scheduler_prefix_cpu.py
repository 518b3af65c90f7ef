"""CPU: ClipScheduler's shared prefixes (add_prefix / submit(prefix=) / drop_prefix) on a scripted engine with seq_fork, prefill_extend_batch and reference-counted
KV pages.  The double's token t of a request is a pure function of (the rows its sequence holds, t): a request that forks a holder and prefills only its tail gets the
ids of its full prompt exactly when the scheduler cut the prompt where the holder ends -- any other cut, a wrong holder or a tail prefilled twice changes them."""
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from grounded_video_llm_amd import lib as L
from grounded_video_llm_amd import serve


class Emb:
    """a spliced prompt: row i is the integer rows[i]"""

    def __init__(self, rows):
        self.rows = tuple(int(r) for r in rows)
        self.shape = (len(self.rows), 8)

    def __getitem__(self, sl):
        assert isinstance(sl, slice)
        return Emb(self.rows[sl])


class Engine:
    """Engine double with a page pool whose pages are reference counted: a fork shares the pages of its source's first n_tokens."""

    def __init__(self, pages, vocab=50, max_seq=4096, rope_orig_max_pos=0):
        self.total, self.vocab = pages, vocab
        self.geo = SimpleNamespace(max_seq=max_seq, rope_orig_max_pos=rope_orig_max_pos, rope_long=object() if rope_orig_max_pos else None)
        self.refs = {}                       # page id -> holders
        self.seqs, self.log, self._next, self._page = {}, [], 0, 0
        self.min_free = pages

    @property
    def free(self):
        return self.total - len(self.refs)

    def _oom(self):
        e = L.GvlError("KV pages exhausted")
        e.status = L.ERR_OOM
        return e

    def _open(self, shared, max_tokens):
        need = (max_tokens + 63) // 64 - len(shared)
        if need > self.free:
            raise self._oom()
        own = []
        for _ in range(need):
            self._page += 1
            own.append(self._page)
            self.refs[self._page] = 0
        for p in list(shared) + own:
            self.refs[p] += 1
        self.min_free = min(self.min_free, self.free)
        self._next += 1
        self.seqs[self._next] = dict(pages=list(shared) + own, cap=max_tokens, rows=(), out=[])
        return self._next

    def seq_alloc(self, max_tokens):
        return self._open([], max_tokens)

    def seq_fork(self, src, n_tokens, max_tokens):
        q = self.seqs[src]
        assert n_tokens > 0 and n_tokens % 64 == 0 and n_tokens <= len(q["rows"]) and max_tokens > n_tokens
        self.log.append(("fork", src, n_tokens))
        s = self._open(q["pages"][:n_tokens // 64], max_tokens)
        self.seqs[s]["rows"] = q["rows"][:n_tokens]
        return s

    def seq_free(self, seq):
        for p in self.seqs.pop(seq)["pages"]:
            self.refs[p] -= 1
            if not self.refs[p]:
                del self.refs[p]

    def _tok(self, rows, t):
        return zlib.crc32(f"{hash(rows)}:{t}".encode()) % self.vocab

    def _prefill(self, seqs, embs, extend):
        assert len(set(seqs)) == len(seqs) == len(embs)
        for s, e in zip(seqs, embs):
            q = self.seqs[s]
            assert (extend or not q["rows"]) and len(q["rows"]) % 64 == 0 and not q["out"] and e.shape[0] >= 1 and len(q["rows"]) + e.shape[0] <= q["cap"]
            q["rows"] = q["rows"] + e.rows
            q["out"].append(self._tok(q["rows"], 0))

    def prefill_batch(self, seqs, embs):
        self.log.append(("prefill", [e.shape[0] for e in embs]))
        self._prefill(seqs, embs, False)

    def prefill_extend_batch(self, seqs, embs, want_logits=False):
        self.log.append(("extend", [e.shape[0] for e in embs], [len(self.seqs[s]["rows"]) for s in seqs]))
        self._prefill(seqs, embs, True)

    def decode_steps(self, seqs, k):
        assert len(set(seqs)) == len(seqs) and k >= 1
        for s in seqs:
            q = self.seqs[s]
            assert len(q["rows"]) + len(q["out"]) - 1 + k <= q["cap"], "scheduler overran a sequence's KV capacity"
            for _ in range(k):
                q["out"].append(self._tok(q["rows"], len(q["out"])))

    def seq_read(self, seq, first=0, cap=4096):
        return self.seqs[seq]["out"][first:first + cap]

    def alone(self, emb, max_new, eos):
        out = []
        for t in range(min(max_new, self.geo.max_seq - emb.shape[0] + 1)):
            out.append(self._tok(emb.rows, t))
            if eos is not None and out[-1] == eos:
                break
        return out


def clips(rng, n_clips=3, n_req=23):
    """n_clips visual prefixes and n_req prompts: two thirds ask about a clip (prefix rows + a tail of their own), the rest are unrelated"""
    bases = [rng.integers(0, 10**6, int(rng.integers(130, 600))) for _ in range(n_clips)]
    reqs = []
    for i in range(n_req):
        c = int(rng.integers(0, n_clips)) if i % 3 else None
        tail = rng.integers(0, 10**6, int(rng.integers(1, 150)))
        reqs.append((c, Emb(np.concatenate([bases[c], tail]) if c is not None else tail)))
    return [Emb(b) for b in bases], reqs


@pytest.mark.parametrize("max_active,chunk,pages", [(1, 1, 80), (4, 8, 80), (3, 5, 34), (8, 16, 1000), (5, 3, 60)])
def test_ids_equal_one_at_a_time_for_mixes_of_prefixed_and_plain_requests(max_active, chunk, pages):
    eng = Engine(pages)
    rng = np.random.default_rng(max_active * 100 + chunk)
    bases, reqs = clips(rng)
    eos, max_new = 7, 40
    want = [eng.alone(e, max_new, eos) for _, e in reqs]
    assert any(len(w) < max_new for w in want) and any(len(w) == max_new for w in want)
    sch = serve.ClipScheduler(eng, eos, max_active=max_active, chunk=chunk, max_prefill_rows=400)
    pids = [sch.add_prefix(b) for b in bases]
    held = sum(b.shape[0] // 128 * 128 // 64 for b in bases)
    assert eng.free == pages - held                                   # a prefix's pages are held ONCE, whatever follows
    rids = [sch.submit(e, max_new, prefix=None if c is None else pids[c]) for c, e in reqs]
    out = sch.run()
    assert [out[r] for r in rids] == want
    assert sch.stats["max_concurrent"] <= max_active
    assert sch.stats["prefix_rows_saved"] == sum(bases[c].shape[0] // 128 * 128 for c, _ in reqs if c is not None)
    # every admitted request prefilled only its tail: tail rows + prefix rows = its prompt, and tail rows alone count against max_prefill_rows
    ext = [op for op in eng.log if op[0] == "extend"]
    assert ext and all(sum(op[1]) <= 400 or len(op[1]) == 1 for op in ext)
    passes = [op for op in eng.log if op[0] in ("prefill", "extend")][len(bases):]           # the first len(bases) are add_prefix's own
    assert sum(sum(op[1]) for op in passes) == sum(e.shape[0] for _, e in reqs) - sch.stats["prefix_rows_saved"]
    assert sorted([a + b for op in ext for a, b in zip(op[1], op[2])] + [n for op in passes if op[0] == "prefill" for n in op[1]]) == sorted(e.shape[0] for _, e in reqs)
    if max_active > 1 and pages >= 80:
        assert any(0 in op[2] and any(op[2]) for op in ext), "prefixed and plain newcomers never shared a pass"
    # shared pages are counted once: the low-water mark is what one copy of each prefix + the concurrent tails need, far above per-request copies
    assert eng.free == pages - held and len(eng.seqs) == len(bases)
    for p in pids:
        sch.drop_prefix(p)
    assert eng.free == pages and not eng.seqs and not eng.refs, "pages leaked"


def test_shared_pages_are_counted_once():
    eng = Engine(64)
    base = Emb(range(1000, 1000 + 1280))                        # 20 pages
    sch = serve.ClipScheduler(eng, None, max_active=8, chunk=4)
    pid = sch.add_prefix(base)
    reqs = [Emb(base.rows + (i, i + 1, i + 2)) for i in range(8)]
    rids = [sch.submit(e, 50, prefix=pid) for e in reqs]
    sch.step()
    assert len(sch.active) == 8                                   # 8 x 21 pages would not fit 64; 20 + 8 x 1 does
    assert eng.free == 64 - 20 - 8 and eng.min_free == 64 - 28
    out = sch.run()
    assert [out[r] for r in rids] == [eng.alone(e, 50, None) for e in reqs]
    assert [op for op in eng.log if op[0] == "extend"] == [("extend", [3] * 8, [1280] * 8)]
    sch.drop_prefix(pid)
    assert eng.free == 64 and not eng.seqs


def test_drop_prefix_while_requests_are_queued_and_in_flight():
    eng = Engine(200)
    base = Emb(range(300))                                       # P = 256: 4 pages
    sch = serve.ClipScheduler(eng, None, max_active=2, chunk=2)
    pid = sch.add_prefix(base)
    holder = sch.prefixes[pid].seq
    reqs = [Emb(base.rows + (900 + i,)) for i in range(5)]
    rids = [sch.submit(e, 9, prefix=pid) for e in reqs]
    sch.step()                                                   # two in flight, three queued
    assert len(sch.active) == 2 and len(sch.queue) == 3
    sch.drop_prefix(pid)
    assert holder in eng.seqs, "the holder must live while queued requests name it"
    with pytest.raises(KeyError):
        sch.submit(reqs[0], 3, prefix=pid)                       # no new submissions
    with pytest.raises(KeyError):
        sch.drop_prefix(pid)
    seen_free_with_forks_alive = False
    while sch.pending():
        sch.step()
        if holder not in eng.seqs and sch.active:
            seen_free_with_forks_alive = True                    # admitted forks keep the pages alive through their references
            assert all(eng.seqs[r.seq]["rows"][:256] == base.rows[:256] for r in sch.active)
        assert (holder in eng.seqs) == bool(sum(r.prefix == pid for r in sch.queue))      # freed as soon as no queued request names it
    assert seen_free_with_forks_alive
    assert [sch.done[r] for r in rids] == [eng.alone(e, 9, None) for e in reqs]
    assert eng.free == 200 and not eng.seqs and pid not in sch.prefixes
    # with nothing queued the holder goes at once
    pid2 = sch.add_prefix(base)
    assert eng.free == 196
    sch.drop_prefix(pid2)
    assert eng.free == 200


def test_oom_on_a_fork_waits_for_a_retirement_then_proceeds():
    eng = Engine(4 + 3)                                          # the holder's 4 pages + 3
    base = Emb(range(256))
    sch = serve.ClipScheduler(eng, None, max_active=4, chunk=4)
    pid = sch.add_prefix(base)
    reqs = [Emb(base.rows + tuple(range(i, i + 10))) for i in (1000, 2000, 3000)]
    plain = Emb(range(5000, 5020))
    rids = [sch.submit(reqs[0], 60, prefix=pid), sch.submit(reqs[1], 60, prefix=pid), sch.submit(plain, 6), sch.submit(reqs[2], 6, prefix=pid)]
    sch.step()                                                   # 266 + 60 tokens = 6 pages, 4 shared: 2 own pages each -> the second fork does not fit
    assert [r.rid for r in sch.active] == [rids[0]] and len(sch.queue) == 3, "FIFO: nobody overtakes the waiting fork"
    out = sch.run()
    assert [out[r] for r in rids] == [eng.alone(e, n, None) for e, n in ((reqs[0], 60), (reqs[1], 60), (plain, 6), (reqs[2], 6))]
    sch.drop_prefix(pid)
    assert eng.free == 7 and not eng.seqs
    # a fork that can never fit is a loud error, as for seq_alloc
    eng = Engine(5)
    sch = serve.ClipScheduler(eng, None)
    pid = sch.add_prefix(base)
    sch.submit(Emb(base.rows + (1,)), 200, prefix=pid)
    with pytest.raises(L.GvlError, match="does not fit"):
        sch.run()


def test_argument_rules():
    eng = Engine(100)
    sch = serve.ClipScheduler(eng, None)
    with pytest.raises(ValueError):
        sch.add_prefix(Emb(range(127)))
    assert eng.free == 100
    pid = sch.add_prefix(Emb(range(200)))                        # P = 128
    assert sch.prefixes[pid].rows == 128 and eng.free == 98
    with pytest.raises(ValueError):
        sch.submit(Emb(range(128)), 4, prefix=pid)               # no row of its own
    with pytest.raises(KeyError):
        sch.submit(Emb(range(300)), 4, prefix=pid + 1)
    assert not sch.queue
    r = sch.submit(Emb(range(129)), 4, prefix=pid)
    assert sch.run()[r] == eng.alone(Emb(range(129)), 4, None)
    assert [op for op in eng.log if op[0] == "extend"] == [("extend", [1], [128])]
    sch.drop_prefix(pid)
    assert eng.free == 100


def test_longrope_rule_ignores_the_prefix():
    """P <= rope_orig_max_pos < len(embeds): a full prefill of that prompt ropes the shared rows with the long factors -- the request is served without the prefix"""
    eng = Engine(100, rope_orig_max_pos=300)
    sch = serve.ClipScheduler(eng, None)
    pid = sch.add_prefix(Emb(range(256)))
    long_, short = Emb(range(301)), Emb(range(300))
    a, b = sch.submit(long_, 3, prefix=pid), sch.submit(short, 3, prefix=pid)
    assert [r.prefix for r in sch.queue] == [None, pid]
    out = sch.run()
    assert out[a] == eng.alone(long_, 3, None) and out[b] == eng.alone(short, 3, None)
    assert [op for op in eng.log if op[0] == "extend"] == [("extend", [301, 44], [0, 256])]
    assert sch.stats["prefix_rows_saved"] == 256
    sch.drop_prefix(pid)
    assert eng.free == 100


def test_no_new_engine_method_is_called_when_no_request_names_a_prefix():
    eng = Engine(64)
    eng.seq_fork = eng.prefill_extend_batch = None               # calling either raises TypeError
    embs = [Emb(range(i * 1000, i * 1000 + 20 + 7 * i)) for i in range(9)]
    assert serve.generate_many(eng, embs, 12, 7, max_active=4, chunk=5) == [eng.alone(e, 12, 7) for e in embs]
    assert {op[0] for op in eng.log} == {"prefill"} and eng.free == 64
    # ... also not with a prefix registered that nobody names
    sch = serve.ClipScheduler(eng, None)
    pid = sch.add_prefix(Emb(range(128)))
    r = sch.submit(embs[0], 3)
    assert sch.run()[r] == eng.alone(embs[0], 3, None)
    sch.drop_prefix(pid)
    assert eng.free == 64
