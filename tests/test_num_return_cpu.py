"""CPU: the host logic of num_return_sequences.  generate()'s argument errors (HF's three, and the guidance refusal) come before any work; the stream numbering gives
the prefix property; ClipScheduler.submit(num_return_sequences = n) on the scripted engine of test_host_logic.py: n request ids, ONE prefill, a fan-out at admission
that counts as n toward max_active, answers that do not depend on max_active or chunk, all-or-nothing admission, nothing leaked."""
import pytest
import torch

from grounded_video_llm_amd import lib as L, model as M, serve
from test_host_logic import _Emb, _ScriptedEngine


class _NoEngine:
    """generate()'s argument errors must come before any work: every engine call fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} reached")


def test_generate_argument_errors():
    from types import SimpleNamespace
    m = M.LLAVA_NEXT_VIDEO.__new__(M.LLAVA_NEXT_VIDEO)
    m.engine, m.geo = _NoEngine(), SimpleNamespace(vocab=640)
    samples = {"prompts": ["a", "b"], "video_ids": ["x", "y"], "spatial_pixel_values": torch.zeros((2, 1))}
    with pytest.raises(ValueError, match="Greedy methods without beam search do not support `num_return_sequences` different than 1"):
        m.generate(samples, num_return_sequences=2)
    with pytest.raises(ValueError, match="Greedy methods without beam search do not support `num_return_sequences` different than 1"):
        m.generate(samples, do_sample=False, num_beams=1, num_return_sequences=3)
    with pytest.raises(ValueError, match=r"`num_return_sequences` \(4\) has to be smaller or equal to `num_beams` \(3\)"):
        m.generate(samples, num_beams=3, num_return_sequences=4)
    with pytest.raises(ValueError, match=r"`num_return_sequences` \(4\) has to be smaller or equal to `num_beams` \(3\)"):
        m.generate(samples, num_beams=3, do_sample=True, num_return_sequences=4)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="`num_return_sequences` has to be a strictly positive integer"):
            m.generate(samples, do_sample=True, num_return_sequences=bad)
    with pytest.raises(ValueError, match="guidance_scale with num_return_sequences > 1 is not supported"):
        m.generate(samples, do_sample=True, num_return_sequences=2, guidance_scale=2.0, negative_prompts=["n", "n"])
    with pytest.raises(ValueError, match="generate_shared.*num_return_sequences > 1 is built for sampling"):
        m.generate_shared({"spatial_pixel_values": torch.zeros((1, 1))}, ["a"], num_beams=3, num_return_sequences=2)
    with pytest.raises(ValueError, match="Greedy methods"):
        m.generate_shared({"spatial_pixel_values": torch.zeros((1, 1))}, ["a"], num_return_sequences=2)
    assert M.num_return_sequences(dict()) == 1 and M.num_return_sequences(dict(num_return_sequences=None)) == 1
    assert M.num_return_sequences(dict(num_return_sequences=1, guidance_scale=2.0)) == 1     # one answer: nothing else is looked at
    assert M.num_return_sequences(dict(num_return_sequences=3, num_beams=3)) == 3 and M.num_return_sequences(dict(num_return_sequences=5, do_sample=True)) == 5


def test_stream_numbering_does_not_depend_on_n():
    seen = {M.fanout_stream(p, j) for p in range(40) for j in range(40)}
    assert len(seen) == 1600 and all(0 <= s < 2 ** 32 for s in seen)              # distinct, and a uint32
    assert M.fanout_stream(3, 0) == 3 and M.fanout_stream(3, 2) == 2 * 65536 + 3   # the documented function of (prompt index, member index)
    for p, j in ((65536, 0), (0, 65536), (-1, 0)):
        with pytest.raises(ValueError):
            M.fanout_stream(p, j)


# ---- the scheduler on a scripted engine -----------------------------------------------------------------------------------------------------
class _FanEngine(_ScriptedEngine):
    """token t of answer j of a request is a pure function of (the prompt's seed, j, t); a sibling costs the pages behind the prompt's whole pages"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.sampling, self.fanouts = {}, []

    def seq_set_sampling(self, seq, sampling=None, **kw):
        self.sampling[seq] = sampling

    def prefill(self, seq, emb, want_logits=False):
        q = self.seqs[seq]
        assert q["seed"] is None and emb.shape[0] <= q["cap"] and want_logits
        self.log.append(("prefill", [emb.shape[0]]))
        q["seed"], q["pos"] = f"{emb.seed}/0", emb.shape[0]
        q["out"].append(self._tok(q["seed"], 0))
        return ("logits", seq)

    def seq_fanout(self, seq, n_new, max_tokens, streams, first_logits):
        src = self.seqs[seq]
        assert first_logits == ("logits", seq) and len(src["out"]) == 1 and len(streams) == n_new and 1 <= n_new <= 15
        need = (max_tokens + 63) // 64 - src["pos"] // 64
        if need * n_new > self.free:
            e = L.GvlError("KV pages exhausted")
            e.status = L.ERR_OOM
            raise e
        self.fanouts.append((seq, list(streams)))
        out = []
        for st in streams:
            self.free -= need
            self._next += 1
            seed = src["seed"].split("/")[0] + f"/{st}"
            self.seqs[self._next] = dict(pages=need, cap=max_tokens, seed=seed, pos=src["pos"], out=[self._tok(seed, 0)])
            out.append(self._next)
        return out

    def answer(self, emb, j, max_new, eos):
        out = []
        for t in range(max_new):
            out.append(self._tok(f"{emb.seed}/{j}", t))
            if eos is not None and out[-1] == eos:
                break
        return out


@pytest.mark.parametrize("max_active,chunk", [(3, 1), (3, 8), (8, 1), (8, 8), (20, 5)])
def test_scheduler_fans_a_request_out(max_active, chunk):
    eng = _FanEngine(400)
    sch = serve.ClipScheduler(eng, 7, max_active=max_active, chunk=chunk)
    a, b, c = _Emb(70, 1), _Emb(130, 2), _Emb(20, 3)
    r_plain = sch.submit(a, 12)
    r_fan = sch.submit(b, 12, num_return_sequences=3, temperature=0.7, seed=5)
    r_tail = sch.submit(c, 12, do_sample=False)
    big = sch.submit(c, 9, num_return_sequences=max_active, do_sample=True, seed=1) if max_active <= 16 else None
    assert isinstance(r_plain, int) and isinstance(r_fan, list) and len(r_fan) == 3 and len(set(r_fan + [r_plain, r_tail])) == 5
    out = sch.run()
    assert [out[r] for r in r_fan] == [eng.answer(b, j, 12, 7) for j in range(3)]          # answer j: stream j, whatever max_active and chunk are
    assert out[r_plain] == eng.alone(a, 12, 7) and out[r_tail] == eng.alone(c, 12, 7)
    if big is not None:
        assert [out[r] for r in big] == [eng.answer(c, j, 9, 7) for j in range(max_active)]
    assert sum(1 for op in eng.log if op == ("prefill", [130])) == 1                         # ONE prefill for the three answers
    assert eng.fanouts[0][1] == [1, 2] and sch.stats["max_concurrent"] <= max_active
    src = eng.fanouts[0][0]
    assert eng.sampling[src] == dict(do_sample=True, temperature=0.7, top_k=50, top_p=None, seed=5, stream=0, min_p=None, typical_p=None,
                                     epsilon_cutoff=None, eta_cutoff=None)
    assert eng.free == 400 and not eng.seqs, "pages leaked"


def test_fan_out_waits_for_slots_and_pages():
    eng = _FanEngine(12)                                        # 4 pages per plain request below; the fan-out needs 3 + 2 * 1
    sch = serve.ClipScheduler(eng, None, max_active=4, chunk=4)
    r0, r1 = sch.submit(_Emb(200, 1), 8), sch.submit(_Emb(200, 2), 8)
    fan = sch.submit(_Emb(130, 3), 8, num_return_sequences=3, seed=2)
    sch.step()
    assert len(sch.active) == 2 and len(sch.queue) == 1         # two slots are free, three are needed: the fan-out waits as a whole
    out = sch.run()
    assert [out[r] for r in fan] == [eng.answer(_Emb(130, 3), j, 8, None) for j in range(3)]
    assert out[r0] == eng.alone(_Emb(200, 1), 8, None) and eng.free == 12 and not eng.seqs
    # pages: slots are there, the siblings' pages are not -- the source goes back, nothing half-admitted stays behind, and the request runs once pages are free
    eng = _FanEngine(9)
    sch = serve.ClipScheduler(eng, None, max_active=8, chunk=4)
    r0 = sch.submit(_Emb(200, 1), 8)                            # 4 pages
    fan = sch.submit(_Emb(60, 3), 80, num_return_sequences=3, seed=2)    # 3 pages each, nothing shared: 9 in all
    sch.step()
    assert len(sch.active) == 1 and len(sch.queue) == 1 and eng.free == 5 and len(eng.seqs) == 1
    out = sch.run()
    assert [out[r] for r in fan] == [eng.answer(_Emb(60, 3), j, 80, None) for j in range(3)] and eng.free == 9 and not eng.seqs


def test_submit_validation():
    sch = serve.ClipScheduler(_FanEngine(64), 7, max_active=4)
    with pytest.raises(ValueError, match="Greedy methods without beam search do not support `num_return_sequences` different than 1"):
        sch.submit(_Emb(5, 1), 4, num_return_sequences=2)
    with pytest.raises(ValueError, match="Greedy methods"):
        sch.submit(_Emb(5, 1), 4, num_return_sequences=2, do_sample=False)
    with pytest.raises(ValueError, match="strictly positive integer"):
        sch.submit(_Emb(5, 1), 4, num_return_sequences=0, do_sample=True)
    with pytest.raises(ValueError, match="guidance_scale with num_return_sequences > 1"):
        sch.submit(_Emb(5, 1), 4, num_return_sequences=2, do_sample=True, guidance_scale=2.0, negative=_Emb(3, 2))
    with pytest.raises(ValueError, match="counts as 5 toward max_active"):
        sch.submit(_Emb(5, 1), 4, num_return_sequences=5, do_sample=True)
    assert sch.pending() == 0
    assert isinstance(sch.submit(_Emb(5, 1), 4, num_return_sequences=1), int)       # one answer: today's request, today's return value
