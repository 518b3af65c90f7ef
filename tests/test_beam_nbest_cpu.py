"""The n best hypotheses of a beam search (HF generate(num_beams = k, num_return_sequences = n); transformers 4.40.1 BeamSearchScorer.finalize with
num_beam_hyps_to_keep = n) on the CPU: BeamState::finalize_n of csrc/gvl_beam.h (tests/c/beam_nbest_check.cc, host compiler) against beam.py's num_return on the
candidate lists beam.py saw -- the approach of tests/test_beam_host_cpu.py, whose synthetic model and recording hook are used here --, hand-written lists for the order
among equal scores and the eos rule, and beam.py against the installed transformers' generate(num_return_sequences = n) on a tiny Llama."""
import atexit
import functools
import itertools
import os
import shutil
import subprocess
import tempfile
import zlib

import pytest
import torch

import conftest  # noqa: F401  (puts the package on sys.path)
from grounded_video_llm_amd.beam import beam_search
from test_beam_host_cpu import EARLY, EOS_MODES, V, model, topk_hook

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grounded-video-llm_amd", "csrc")


@functools.lru_cache(maxsize=None)
def checker():
    tmp = tempfile.mkdtemp(prefix="gvl_nbest_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "beam_nbest_check")
    cmd = ["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", CSRC, os.path.join(ROOT, "tests", "c", "beam_nbest_check.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def replay(k, vocab, max_new, eos, lp, early, n, record):
    """-> (the n results finalize_n gave, the one finalize gave), each (ids, score, transition scores)"""
    lines = [f"{k} {vocab} {max_new} {-1 if eos is None else eos} {float(lp).hex()} {EARLY[early]} {n}"]
    for cands in record:
        lines.append(" ".join([str(len(cands))] + [f"{float(v).hex()} {int(i)} {float(p).hex()}" for v, i, p in cands]))
    r = subprocess.run([checker()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = r.stdout.splitlines()
    assert out and out[0].split()[0] == "count", out
    m = int(out[0].split()[1])

    def parse(ln):
        head, ids, ts = ln.split("|")
        return [int(x) for x in ids.split()], float(head.split()[1]), [float(x) for x in ts.split()]   # %.17g round-trips a double
    assert len(out) == m + 2 and out[-1].startswith("best") and all(ln.startswith("final") for ln in out[1:-1])
    return [parse(ln) for ln in out[1:-1]], parse(out[-1])


def python_side(k, max_new, eos, lp, early, hook, logits_of, n, vocab=V):
    beams = [[] for _ in range(k)]

    def step(parents, toks):
        beams[:] = [beams[p] + [t] for p, t in zip(parents, toks)]
        return torch.stack([logits_of(b) for b in beams])
    res = beam_search(step, logits_of([]), k, max_new, eos, lp, early, None, None, True, candidates=hook, num_return=n)
    return [res] if n == 1 else res


@pytest.mark.parametrize("k", [2, 3, 4])
def test_finalize_n_equals_beam_py(k):
    runs = by_eos = 0
    for early, lp, (mode, (eos, bias)), max_new in itertools.product((False, True), (0.0, 1.0, 2.0), EOS_MODES.items(), (1, 2, 12)):
        seed = zlib.crc32(repr((k, early, lp, mode, max_new, "nbest")).encode())
        logits_of = model(seed, eos, bias)
        full = None
        for n in range(1, k + 1):
            record = []
            py = python_side(k, max_new, eos, lp, early, topk_hook(k, record), logits_of, n)
            got, best = replay(k, V, max_new, eos, lp, early, n, record)
            assert [tuple(map(_t, r)) for r in got] == [tuple(map(_t, r)) for r in py], (k, n, early, lp, mode, max_new)
            assert best == got[0]                                            # finalize == finalize_n(1)'s entry, whatever n is
            assert len(py) == n and all(a[1] >= b[1] for a, b in zip(py, py[1:]))   # best first
            if n == k:
                full = py
            by_eos += any(eos is not None and r[0] and r[0][-1] == eos for r in py)
            runs += 1
        for n in range(1, k):                                                # fewer returned = a prefix of more returned
            assert python_side(k, max_new, eos, lp, early, topk_hook(k, []), logits_of, n) == full[:n]
    assert runs == 54 * k and by_eos > 0


def _t(x):
    return tuple(x) if isinstance(x, list) else x


def scripted(k, vocab, max_new, eos, lp, early, n, script):
    it = iter(script)

    def hook(rows, scores):
        c = next(it)
        return [v for v, _, _ in c], [i for _, i, _ in c], [p for _, _, p in c]
    py = python_side(k, max_new, eos, lp, early, hook, lambda hist: torch.zeros(vocab), n, vocab)
    got, best = replay(k, vocab, max_new, eos, lp, early, n, script)
    assert got == py and best == got[0]
    return py


def test_equal_scores_the_later_added_comes_first():
    cands = [[(-1.0, 3, -1.0), (-1.0, 5, -1.0), (-1.0, 1, -1.0), (-3.0, 2, -3.0)]]
    assert scripted(3, 8, 1, None, 1.0, False, 3, cands) == [([1], -1.0, [-1.0]), ([5], -1.0, [-1.0]), ([3], -1.0, [-1.0])]
    assert scripted(3, 8, 1, None, 1.0, False, 2, cands) == [([1], -1.0, [-1.0]), ([5], -1.0, [-1.0])]
    # a strictly better one in the middle goes first, the equal pair keeps "later first"
    cands = [[(-0.5, 3, -0.5), (-1.0, 5, -1.0), (-1.0, 1, -1.0), (-3.0, 2, -3.0), (-4.0, 4, -4.0), (-5.0, 6, -5.0)]]
    assert [r[0] for r in scripted(3, 8, 1, None, 1.0, False, 3, cands)] == [[3], [1], [5]]


def test_eos_is_appended_only_while_there_is_room():
    # step 2: the eos of rank 0 closes [1] -> [1, eos] (2 ids = max_new: room for exactly the eos); the open beams [1, 3] and [2, 4] follow without one
    s = [[(-0.125, 1, -0.125), (-0.25, 2, -0.25), (-1.0, 3, -1.0), (-2.0, 4, -2.0)],
         [(-0.15625, 7, -0.03125), (-0.5, 3, -0.375), (-0.625, 8 + 4, -0.375), (-1.0, 5, -0.875)]]
    py = scripted(2, 8, 2, 7, 1.0, False, 2, s)
    assert py == [([1, 7], -0.15625 / 2, [-0.125, -0.03125]), ([1, 3], -0.25, [-0.125, -0.375])]
    # max_new 3 with early stopping: two hypotheses close at step 2 by eos, one after 1 id and ... both get their eos, both are shorter than max_new
    s = [[(-0.125, 1, -0.125), (-0.25, 2, -0.25), (-1.0, 3, -1.0), (-2.0, 4, -2.0)],
         [(-0.25, 7, -0.125), (-0.5, 8 + 7, -0.25), (-0.625, 3, -0.5), (-1.0, 8 + 5, -0.75)]]
    py = scripted(2, 8, 3, 7, 1.0, True, 2, s)
    assert py == [([1, 7], -0.125, [-0.125, -0.125]), ([2, 7], -0.25, [-0.25, -0.25])]
    # max_new 1: an eos hypothesis holds no id before its eos; the open beam that fills max_new gets none
    py = scripted(2, 8, 1, 7, 1.0, False, 2, [[(-0.5, 7, -0.5), (-1.0, 3, -1.0), (-2.0, 4, -2.0), (-3.0, 5, -3.0)]])
    assert py == [([7], -0.5, [-0.5]), ([3], -1.0, [-1.0])]


def test_num_return_is_checked():
    for n in (0, 4):
        with pytest.raises(ValueError, match="num_return"):
            beam_search(lambda p, t: torch.zeros((3, 8)), torch.zeros(8), 3, 2, None, num_return=n)


def test_num_return_equals_hf_generate():
    """The same tiny LlamaForCausalLM drives beam.py (num_return = n) and the installed transformers' generate(num_return_sequences = n): equal sequences, in order, for
    k = 2, 3, 4 and every n in 1 .. k.  The vectorised 5.x scorer and the 4.40.1 one differ only in the order among equal scores, so the seeds are ones whose k final
    hypothesis scores are pairwise distinct -- asserted."""
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=50, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, max_position_embeddings=256)
    m = LlamaForCausalLM(cfg).eval()
    E = m.get_input_embeddings().weight
    n_eos_hits = 0
    for seed in range(3):
        emb = torch.randn((1, 7, 32), generator=torch.Generator().manual_seed(seed)) * 2.0
        with torch.no_grad():
            free = m.generate(inputs_embeds=emb, num_beams=3, do_sample=False, max_new_tokens=8, eos_token_id=None, pad_token_id=0)[0].tolist()

        def fwd(x):
            with torch.no_grad():
                return m(inputs_embeds=x).logits[0, -1]
        for k, eos, mx, lp in ((3, free[2], 9, 1.0), (4, None, 6, 1.0), (2, free[2], 12, 1.0), (4, free[3], 10, 0.5)):
            def ours(n):
                beams = [[] for _ in range(k)]

                def step(parents, toks):
                    beams[:] = [beams[p_] + [t] for p_, t in zip(parents, toks)]
                    return torch.stack([fwd(torch.cat([emb, E[torch.tensor(b)][None]], 1)) for b in beams])
                res = beam_search(step, fwd(emb), k, mx, eos, lp, False, with_scores=True, num_return=n)
                return [res] if n == 1 else res
            full = ours(k)
            scores = [r[1] for r in full]
            assert len(set(scores)) == k, (seed, k, scores)                  # pairwise distinct: the two scorers' tie orders cannot matter
            for n in range(1, k + 1):
                got = ours(n)
                assert got == full[:n]
                with torch.no_grad():
                    ref = m.generate(inputs_embeds=emb, num_beams=k, num_return_sequences=n, do_sample=False, max_new_tokens=mx, eos_token_id=eos, pad_token_id=0,
                                     length_penalty=lp, early_stopping=False, output_scores=True, return_dict_in_generate=True)
                assert ref.sequences.shape[0] == n
                for r in range(n):
                    want = ref.sequences[r].tolist()
                    m_ = len(got[r][0])                                          # HF pads the rows to the longest hypothesis: with pad, or with eos repeated
                    assert got[r][0] == want[:m_] and all(t in (0, eos) for t in want[m_:]), (seed, k, n, r, eos, mx, lp, got[r][0], want)
                    assert not want[m_:] or (eos is not None and got[r][0][-1] == eos)   # only a hypothesis that ended by eos is padded
                    assert abs(got[r][1] - float(ref.sequences_scores[r])) < 1e-4
                    n_eos_hits += int(eos is not None and eos in got[r][0])
    assert n_eos_hits >= 1, "no hypothesis ended by eos"
