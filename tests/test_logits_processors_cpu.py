"""HF generate()'s logits processors (repetition_penalty, no_repeat_ngram_size, min_new_tokens / min_length) as the product resolves them
(grounded_video_llm_amd/logits.py) and as the device kernel applies them (csrc/gvl_logits.hip, restated below in torch) -- pinned against the
installed transformers' own generate(inputs_embeds=...) on a tiny LlamaForCausalLM, greedy and beam search.  No GPU."""
import math
import warnings

import pytest
import torch

from grounded_video_llm_amd import logits as LP
from grounded_video_llm_amd.beam import beam_search


def restate(scores: torch.Tensor, hist, penalty=1.0, ngram=0, min_new=0, eos=-1) -> torch.Tensor:
    """The kernel's arithmetic on one fp32 row (CPU torch: IEEE multiply / divide): penalty on every distinct generated id (gather -> scatter),
    then the n-gram bans, then the eos ban while fewer than min_new ids were generated."""
    s = scores.clone().float()
    L = len(hist)
    if penalty != 1.0 and L:
        h = torch.tensor(hist, dtype=torch.long)
        g = s.gather(0, h)
        s.scatter_(0, h, torch.where(g < 0, g * penalty, g / penalty))
    if ngram > 0 and L >= ngram:
        suf = list(hist[L - ngram + 1:])
        for i in range(L - ngram + 1):
            if list(hist[i:i + ngram - 1]) == suf:
                s[hist[i + ngram - 1]] = -math.inf
    if eos >= 0 and L < min_new:
        s[eos] = -math.inf
    return s


def _tiny():
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=50, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      max_position_embeddings=256)
    m = LlamaForCausalLM(cfg).eval()
    return m, m.get_input_embeddings().weight


def _hf(m, emb, **kw):
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        return m.generate(inputs_embeds=emb, pad_token_id=0, **kw)[0].tolist()


def _fwd(m, E, emb, ids):
    with torch.no_grad():
        x = torch.cat([emb, E[torch.tensor(ids, dtype=torch.long)][None]], 1) if ids else emb
        return m(inputs_embeds=x).logits[0, -1].float()


def _greedy(m, E, emb, mx, eos, procs):
    ids = []
    while len(ids) < mx:
        s = restate(_fwd(m, E, emb, ids), ids, *procs.args())
        t = int(torch.argmax(s))
        ids.append(t)
        if eos is not None and t == eos:
            break
    return ids


def _has_repeated_ngram(ids, n):
    seen = set()
    for i in range(len(ids) - n + 1):
        g = tuple(ids[i:i + n])
        if g in seen:
            return True
        seen.add(g)
    return False


def test_greedy_with_processors_equals_hf_generate():
    m, E = _tiny()
    hits = {"pen": 0, "ngram": 0, "min": 0}
    for seed in range(5):
        emb = torch.randn((1, 7, 32), generator=torch.Generator().manual_seed(seed)) * 2.0
        plain = _hf(m, emb, do_sample=False, max_new_tokens=24, eos_token_id=None)
        eos = plain[0]                                       # an eos the model really produces -- as its very first token
        cases = [dict(repetition_penalty=1.3), dict(repetition_penalty=0.7), dict(no_repeat_ngram_size=2), dict(no_repeat_ngram_size=1),
                 dict(no_repeat_ngram_size=3, repetition_penalty=1.2), dict(min_new_tokens=5), dict(min_length=7 + 4),
                 dict(min_new_tokens=3, min_length=40), dict(min_length=5), dict(repetition_penalty=1.1, no_repeat_ngram_size=2, min_new_tokens=6)]
        for kw in cases:
            for e in (eos, plain[3], None):
                ref = _hf(m, emb, do_sample=False, max_new_tokens=20, eos_token_id=e, **kw)
                procs = LP.resolve(kw, e, emb.shape[1])
                got = _greedy(m, E, emb, 20, e, procs)
                assert got == ref, (seed, kw, e, got, ref)
                hits["pen"] += int("repetition_penalty" in kw and got != _hf(m, emb, do_sample=False, max_new_tokens=20, eos_token_id=e))
                hits["ngram"] += int("no_repeat_ngram_size" in kw and _has_repeated_ngram(plain[:20], kw["no_repeat_ngram_size"]))
                hits["min"] += int(e == eos and procs.min_new > 0)
    assert all(v > 0 for v in hits.values()), hits          # every processor changed an answer somewhere


def test_beam_search_with_processors_equals_hf_generate():
    m, E = _tiny()
    checked = 0
    for seed in range(4):
        emb = torch.randn((1, 7, 32), generator=torch.Generator().manual_seed(seed)) * 2.0
        free = _hf(m, emb, num_beams=3, do_sample=False, max_new_tokens=8, eos_token_id=None)
        for k, kw, eos, mx in ((3, dict(no_repeat_ngram_size=2), free[2], 10), (2, dict(repetition_penalty=1.5), free[1], 9),
                               (4, dict(min_new_tokens=4), free[0], 8), (3, dict(repetition_penalty=0.8, no_repeat_ngram_size=2, min_length=7 + 3), free[0], 10)):
            ref = _hf(m, emb, num_beams=k, do_sample=False, max_new_tokens=mx, eos_token_id=eos, length_penalty=1.0, early_stopping=False, **kw)
            procs = LP.resolve(kw, eos, emb.shape[1])
            beams = [[] for _ in range(k)]

            def step(parents, toks):
                beams[:] = [beams[p_] + [t] for p_, t in zip(parents, toks)]
                return torch.stack([_fwd(m, E, emb, b) for b in beams])

            def process(hists, lp):
                return torch.stack([restate(lp[j], hists[j], *procs.args()) for j in range(lp.shape[0])])
            got = beam_search(step, _fwd(m, E, emb, []), k, mx, eos, 1.0, False, process=process)
            while ref and ref[-1] == 0 and len(ref) > len(got):
                ref = ref[:-1]
            assert got == ref, (seed, k, kw, got, ref)
            if "no_repeat_ngram_size" in kw:
                assert not _has_repeated_ngram(got, 2)
            checked += 1
    assert checked == 16


def test_kwarg_validation_matches_hf():
    for kw, msg in ((dict(repetition_penalty=2), "`penalty` has to be a strictly positive float, but is 2"),
                    (dict(repetition_penalty=0.0), "strictly positive float"), (dict(repetition_penalty=-1.0), "strictly positive float"),
                    (dict(no_repeat_ngram_size=2.5), "`ngram_size` has to be a strictly positive integer"),
                    (dict(no_repeat_ngram_size=2.0), "`ngram_size` has to be a strictly positive integer"),
                    (dict(min_new_tokens=2.5), "`min_length` has to be a non-negative integer, but is 2.5")):
        with pytest.raises(ValueError, match=msg.replace("`", ".")):
            LP.resolve(kw, 2, 10)
    # what HF leaves silently off: penalty exactly 1 (int or bool), non-positive n-gram sizes, non-positive / absorbed minimum lengths, any min without eos
    for kw in (dict(repetition_penalty=1), dict(repetition_penalty=True), dict(no_repeat_ngram_size=0), dict(no_repeat_ngram_size=-1),
               dict(no_repeat_ngram_size=None), dict(min_new_tokens=0), dict(min_new_tokens=-1), dict(min_length=-1), dict(min_length=2.5), dict(min_length=10)):
        assert not LP.resolve(kw, 2, 10).active, kw
    assert not LP.resolve(dict(min_new_tokens=5, min_length=50), None, 10).active
    assert LP.resolve(dict(min_new_tokens=2.5), None, 10) == LP.OFF            # no eos: HF never builds the min-length processors, so nothing is checked
    # the C ABI's argument order
    assert LP.resolve(dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=4), 7, 10).args() == (1.2, 3, 4, 7)


def test_min_length_uses_the_padded_batch_length_and_min_new_tokens_wins():
    from grounded_video_llm_amd import prompts as P
    ids = [[1, 5, 6, -200, 7], [1, 5, -200, 7, 8, 9, 10, 11]]
    ids_arr, mask = P.left_pad_truncate(ids, 0, 64)
    n_vis = 30
    L = LP.padded_embed_len(ids_arr.shape[1], n_vis)
    assert L == 8 - 1 + 30                                    # the reference stacks both rows at the padded width: 7 text rows + 30 visual rows
    for row_kw in (dict(min_length=L + 6), dict(min_length=L + 6, no_repeat_ngram_size=0)):
        p = LP.resolve(row_kw, 2, L)
        assert p.min_new == 6 and p.eos == 2                 # the SAME value for both rows, whatever each row's own length
    assert LP.resolve(dict(min_length=L - 3), 2, L).min_new == 0
    # generate_shared: every prompt is its own reference call -> its own (un-padded) length
    assert LP.resolve(dict(min_length=45), 2, LP.padded_embed_len(5, n_vis)).min_new == 45 - 34
    assert LP.resolve(dict(min_length=45), 2, LP.padded_embed_len(8, n_vis)).min_new == 45 - 37
    # min_new_tokens takes precedence over min_length (GenerationMixin._prepare_generated_length)
    assert LP.resolve(dict(min_new_tokens=3, min_length=L + 20), 2, L).min_new == 3
    assert LP.resolve(dict(min_new_tokens=0, min_length=L + 20), 2, L).min_new == 0


def test_min_length_adjustment_equals_hf_with_inputs_embeds():
    """HF itself: min_length counts the embedding rows -- min_length = rows + k bans eos exactly for the first k new ids."""
    m, E = _tiny()
    emb = torch.randn((1, 9, 32), generator=torch.Generator().manual_seed(3)) * 2.0
    eos = _hf(m, emb, do_sample=False, max_new_tokens=4, eos_token_id=None)[0]
    for k in (0, 1, 3, 6):
        ref = _hf(m, emb, do_sample=False, max_new_tokens=12, eos_token_id=eos, min_length=9 + k)
        assert eos not in ref[:k] and ref == _greedy(m, E, emb, 12, eos, LP.resolve(dict(min_length=9 + k), eos, 9))
    assert _hf(m, emb, do_sample=False, max_new_tokens=12, eos_token_id=eos, min_length=9)[0] == eos


def test_restatement_is_duplicate_safe_and_ordered():
    s = torch.tensor([2.0, -2.0, 0.0, 4.0, -0.0, 1.0])
    out = restate(s, [0, 0, 1, 1, 1, 3], penalty=2.0)
    assert out.tolist() == [1.0, -4.0, 0.0, 2.0, -0.0, 1.0]          # penalised ONCE per distinct id
    out = restate(s, [0, 3, 5, 0, 3], penalty=2.0, ngram=3)            # suffix (0, 3) seen at 0 -> bans 5; the penalty never overwrites a ban
    assert out[5] == -math.inf and out[0] == 1.0 and out[3] == 2.0
    out = restate(s, [1, 2], min_new=3, eos=4)
    assert out[4] == -math.inf
    assert restate(s, [1, 2, 3], min_new=3, eos=4)[4] == -0.0


class _ScriptedEngine:
    """The ClipScheduler's engine surface on the CPU: every sequence emits its own seq id forever; records processor settings."""

    def __init__(self):
        self.n, self.live, self.gen, self.procs = 0, set(), {}, {}

    def seq_alloc(self, cap):
        self.n += 1
        self.live.add(self.n)
        self.gen[self.n] = 0
        return self.n

    def seq_free(self, s):
        self.live.discard(s)

    def seq_set_processors(self, s, *a):
        assert s in self.live
        self.procs[s] = a

    def prefill_batch(self, seqs, embeds):
        for s in seqs:
            self.gen[s] = 1

    def decode_steps(self, seqs, k):
        for s in seqs:
            self.gen[s] += k

    def seq_read(self, s, first, cap):
        return [100 + s] * max(0, min(self.gen[s] - first, cap))


def test_scheduler_sets_per_request_processors():
    from grounded_video_llm_amd.serve import ClipScheduler
    eng = _ScriptedEngine()
    sch = ClipScheduler(eng, eos_id=2, max_active=4, chunk=3)
    emb = torch.zeros((5, 4))
    a = sch.submit(emb, 6, repetition_penalty=1.3)
    b = sch.submit(emb, 6)
    c = sch.submit(emb, 6, no_repeat_ngram_size=2, min_new_tokens=4)
    out = sch.run()
    assert [len(out[r]) for r in (a, b, c)] == [6, 6, 6]
    assert eng.procs == {1: (1.3, 0, 0, 2), 3: (1.0, 2, 4, 2)}          # request b keeps the engine's default: no call
    with pytest.raises(ValueError):
        sch.submit(emb, 4, repetition_penalty=0.0)
    with pytest.raises(ValueError):
        sch.submit(emb, 4, no_repeat_ngram_size=1.5)
