"""CPU: ClipScheduler.submit's sampling arguments on the scripted engine of test_host_logic.py: a request's own setting reaches Engine.seq_set_sampling at its
admission (before its prefill, stream 0, HF's defaults for what is absent), a request without one never touches it, and bad values raise at submit."""
import pytest

from grounded_video_llm_amd import serve
from test_host_logic import _Emb, _ScriptedEngine


class _SamplingEngine(_ScriptedEngine):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.sampling = {}

    def seq_set_sampling(self, seq, sampling=None, **kw):
        assert self.seqs[seq]["seed"] is None, "the setting must be in place before the sequence's prefill"
        self.sampling[seq] = sampling
        self.log.append(("sampling", seq))


def test_submit_sampling_reaches_the_engine():
    eng = _SamplingEngine(64)
    sch = serve.ClipScheduler(eng, 7, max_active=2, chunk=4)
    embs = [_Emb(10 + i, 100 + i) for i in range(4)]
    r0 = sch.submit(embs[0], 6)                                                     # follows the engine's setting
    r1 = sch.submit(embs[1], 6, do_sample=False)                                    # greedy whatever the engine samples
    r2 = sch.submit(embs[2], 6, temperature=0.7, top_p=0.9, min_p=0.05, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=2e-3, seed=11)
    r3 = sch.submit(embs[3], 6, do_sample=True, top_k=0, typical_p=1.0)
    want = {r: eng.alone(e, 6, 7) for r, e in zip((r0, r1, r2, r3), embs)}
    assert sch.run() == want                                                         # the double's tokens do not depend on settings: the plumbing changes no ids
    got = sorted(eng.sampling.items())
    assert len(got) == 3                                                             # r0 never reached seq_set_sampling
    assert [s for _, s in got] == [
        dict(do_sample=False),
        dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9, seed=11, stream=0, min_p=0.05, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=2e-3),
        dict(do_sample=True, temperature=1.0, top_k=0, top_p=None, seed=0, stream=0, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None)]
    assert eng.free == 64 and not eng.seqs


@pytest.mark.parametrize("kw,msg", [(dict(min_p=2.0), r"`min_p` has to be a float in the \[0, 1\] interval, but is 2.0"),
                                    (dict(typical_p=0.0), r"`typical_p` has to be a float > 0 and < 1, but is 0.0"),
                                    (dict(epsilon_cutoff=1.0), r"`epsilon_cutoff` has to be a float > 0 and < 1, but is 1.0"),
                                    (dict(eta_cutoff=-0.5), r"`eta_cutoff` has to be a float > 0 and < 1, but is -0.5"),
                                    (dict(temperature=0.0), "strictly positive float"), (dict(top_k=-3), "top_k"), (dict(top_p=1.2), "top_p")])
def test_submit_sampling_is_validated(kw, msg):
    eng = _SamplingEngine(64)
    sch = serve.ClipScheduler(eng, 7)
    with pytest.raises(ValueError, match=msg):
        sch.submit(_Emb(5, 1), 4, **kw)
    assert sch.pending() == 0 and not eng.sampling                                   # nothing was queued


def test_admission_failure_frees_the_sequence():
    class _Refusing(_SamplingEngine):
        def seq_set_sampling(self, seq, sampling=None, **kw):
            raise ValueError("refused")
    eng = _Refusing(64)
    sch = serve.ClipScheduler(eng, 7)
    sch.submit(_Emb(5, 1), 4, do_sample=False)
    with pytest.raises(ValueError, match="refused"):
        sch.step()
    assert eng.free == 64 and not eng.seqs
