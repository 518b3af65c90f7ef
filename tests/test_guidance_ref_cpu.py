"""Classifier-free guidance on the CPU: tests/guidance_ref.py pinned against the installed transformers (the processor class and generate(guidance_scale=...,
negative_prompt_ids=...) of a tiny LlamaForCausalLM), the tolerance bound of the GPU operator test shown to hold for a plain fp32 evaluation, the grouping rule
decode_parts_paired (csrc/gvl_decode_plan.h) through a small C++ dump, and logits.resolve_guidance / generate()'s argument errors.  No GPU."""
import itertools
import math
import os
import subprocess
import warnings

import pytest
import torch

import guidance_ref as GR
from grounded_video_llm_amd import logits as LP
from test_logits_processors_cpu import _tiny, restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grounded-video-llm_amd", "csrc")


# ---- the restatements against transformers ----------------------------------------------------------------------------------------------
def test_guided_row_equals_the_hf_processor():
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor as CFG

    class _Model:                                            # what the processor asks of a model: logits for the unconditional ids
        def __init__(self, rows):
            self.rows = rows

        def __call__(self, input_ids, **kw):
            return _Out(self.rows[:, None, :])

    class _Out(dict):
        def __init__(self, logits):
            super().__init__(logits=logits)
            self.logits = logits

    g = torch.Generator().manual_seed(5)
    x = GR.rows(g, 8, 1025)
    cond, neg = x[:4], x[4:]
    for s in GR.SCALES:
        got = CFG(s, _Model(neg), unconditional_ids=torch.zeros((4, 1), dtype=torch.long))(torch.zeros((4, 1), dtype=torch.long), cond.clone())
        for b in range(4):
            ref, _, _ = GR.guided_row(cond[b], neg[b], s)
            assert (got[b].double() - ref).abs().le(GR.bound(cond[b], neg[b], s)).all(), (s, b)
            mine = s * (torch.log_softmax(cond[b], -1) - torch.log_softmax(neg[b], -1)) + torch.log_softmax(neg[b], -1)
            assert torch.equal(got[b], mine), (s, b)         # the loop's fp32 expression is HF's, bit for bit


def _hf_guided(m, prompt, neg, **kw):
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        return m.generate(input_ids=torch.tensor([prompt]), negative_prompt_ids=torch.tensor([neg]), pad_token_id=0, do_sample=False, **kw)


def _stream(m, prompt):
    """one teacher-forced stream over the tiny model: (first logits, step(tok) -> logits), by full recomputation"""
    ids = list(prompt)

    def fwd():
        with torch.no_grad():
            return m(input_ids=torch.tensor([ids])).logits[0, -1].float()

    def step(t):
        ids.append(int(t))
        return fwd()
    return fwd(), step


@pytest.mark.parametrize("kw", [dict(), dict(repetition_penalty=1.4, min_new_tokens=5)], ids=["plain", "penalty+min_new"])
def test_guided_loop_equals_hf_generate(kw):
    m, _ = _tiny()
    changed = 0
    for seed in range(4):
        g = torch.Generator().manual_seed(100 + seed)
        prompt = torch.randint(1, 50, (6,), generator=g).tolist()
        neg = torch.randint(1, 50, (4,), generator=g).tolist()
        plain = m.generate(input_ids=torch.tensor([prompt]), pad_token_id=0, do_sample=False, max_new_tokens=12, eos_token_id=None)[0, 6:].tolist()
        eos = plain[2] if kw else None                       # an eos the model produces early: the min-length ban has something to do
        ref = _hf_guided(m, prompt, neg, guidance_scale=1.5, max_new_tokens=12, eos_token_id=eos, **kw)[0, 6:].tolist()
        while eos is not None and ref and ref[-1] == 0 and (len(ref) < 2 or eos in ref[:-1]):
            ref = ref[:-1]                                   # HF pads behind eos
        gen = []

        def select(i, G):
            # HF's order: guidance FIRST, then the penalty (over prompt + generated ids: this call has input_ids), then the min-new-tokens ban
            s = restate(G, prompt + gen, penalty=kw.get("repetition_penalty", 1.0))
            if eos is not None and len(gen) < kw.get("min_new_tokens", 0):
                s[eos] = -math.inf
            gen.append(int(torch.argmax(s)))
            return gen[-1]
        fc, sc = _stream(m, prompt)
        fu, su = _stream(m, neg)
        got = GR.generate(sc, su, fc, fu, 1.5, 12, eos, select)
        assert got == ref, (seed, kw, got, ref)
        changed += got != plain[:len(got)]
    assert changed > 0                                        # guidance changed an answer somewhere


def test_first_token_is_guided_output_scores():
    m, _ = _tiny()
    prompt, neg = [3, 17, 9, 41, 5], [3, 8]
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        out = m.generate(input_ids=torch.tensor([prompt]), negative_prompt_ids=torch.tensor([neg]), pad_token_id=0, do_sample=False, guidance_scale=1.5,
                         max_new_tokens=3, eos_token_id=None, output_scores=True, return_dict_in_generate=True)
    fc, _ = _stream(m, prompt)
    fu, _ = _stream(m, neg)
    G, _, _ = GR.guided_row(fc, fu, 1.5)
    assert (out.scores[0][0].double() - G).abs().le(GR.bound(fc, fu, 1.5)).all()
    assert int(out.sequences[0, len(prompt)]) == int(torch.argmax(out.scores[0][0]))
    raw = torch.log_softmax(fc, -1)
    assert not torch.allclose(out.scores[0][0], raw, atol=1e-3)      # ... and it is not the unguided row


# ---- the tolerance of the GPU operator test -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,pairs", GR.op_cases())
def test_fp32_torch_stays_inside_the_bound(n, pairs):
    x = GR.op_rows(n, pairs)
    worst = 0.0
    for p in range(pairs):
        s = GR.SCALES[p % 4]
        c, u = x[p], x[pairs + p]
        lc, lu = torch.log_softmax(c, -1), torch.log_softmax(u, -1)
        got = s * (lc - lu) + lu
        G, _, _ = GR.guided_row(c, u, s)
        ratio = ((got.double() - G).abs() / GR.bound(c, u, s)).max()
        worst = max(worst, float(ratio))
    print(f"[guidance] n {n} pairs {pairs}: fp32 torch uses {worst:.3f} of the bound")
    assert worst <= 1.0


# ---- the grouping rule ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs_dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gvl_pairs") / "decode_pairs_dump")
    r = subprocess.run(["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", CSRC, os.path.join(ROOT, "tests", "c", "decode_pairs_dump.cc"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def ask(cases):
        text = "".join(f"{int(mf)} {len(rows)} {' '.join(map(str, rows))}\n" for mf, rows in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == len(cases)
        return [[int(t) for t in ln.split()] for ln in lines]
    return ask


def _arrangements(p, s):
    """orders of p pairs and s singles: pairs first, singles first, interleaved from either end"""
    a = [2] * p + [1] * s
    inter = [v for t in itertools.zip_longest([2] * p, [1] * s) for v in t if v is not None]
    return {tuple(a), tuple(reversed(a)), tuple(inter), tuple(reversed(inter))}


def test_decode_parts_paired(pairs_dump):
    cases = [(mf, list(rows)) for mf in (True, False) for p in range(9) for s in range(17 - 2 * p) if p + s > 0 for rows in sorted(_arrangements(p, s))]
    for (mf, rows), units in zip(cases, pairs_dump(cases)):
        assert sum(units) == len(rows) and all(u >= 1 for u in units), (mf, rows, units)     # every unit once, in order: a pair is one unit and cannot be split
        o = 0
        for u in units:
            total = sum(rows[o:o + u])
            assert (1 <= total <= 16) if mf else total in (1, 2, 4), (mf, rows, units)      # every step has an admitted size
            # ... and takes the longest admitted run: no longer run from the same start is admitted
            for v in range(u + 1, len(rows) - o + 1):
                t = sum(rows[o:o + v])
                assert not ((t <= 16) if mf else t in (1, 2, 4)), (mf, rows, units, o, v)
            o += u
        if mf:
            assert len(units) == 1, (rows, units)                                           # up to 8 pairs, or any mix that fits 16 rows, share one step
    assert pairs_dump([(False, [2, 1]), (False, [1, 2]), (False, [1, 2, 1]), (False, [2, 2, 2])]) == [[1, 1], [1, 1], [3], [2, 1]]
    # without pairs the cut is decode_parts'
    import decode_plan as DP
    plain = [(mf, [1] * n) for mf in (True, False) for n in range(0, 41)]
    want = DP.ask([f"G {int(mf)} {len(rows)}" for mf, rows in plain])
    assert [tuple(u) for u in pairs_dump(plain)] == [tuple(w) for w in want]


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------------
def test_resolve_guidance():
    for off in (dict(), dict(guidance_scale=None), dict(guidance_scale=1), dict(guidance_scale=1.0)):
        assert LP.resolve_guidance(off) is None
    assert LP.resolve_guidance(dict(guidance_scale=2)) == 2.0 and isinstance(LP.resolve_guidance(dict(guidance_scale=2)), float)
    assert LP.resolve_guidance(dict(guidance_scale=-0.5)) == -0.5 and LP.resolve_guidance(dict(guidance_scale=0)) == 0.0
    for bad in (float("inf"), float("nan"), "2", True, [1.5]):
        with pytest.raises(ValueError, match="guidance_scale"):
            LP.resolve_guidance(dict(guidance_scale=bad))
    assert LP.negative_id_rows(torch.tensor([[0, 4, 5], [7, 8, 9]]), torch.tensor([[0, 1, 1], [1, 1, 1]])) == [[4, 5], [7, 8, 9]]
    assert LP.negative_id_rows([4, 5]) == [[4, 5]]
    for ids, mask in (([[4, -1]], None), ([[]], None), ([[4, 5]], [[0, 0]]), ([[4, 5]], [[1]])):
        with pytest.raises(ValueError, match="negative_prompt"):
            LP.negative_id_rows(ids, mask)


class _NoEngine:
    """generate()'s argument errors must come before any work: every engine call fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} reached")


def test_generate_argument_errors():
    from types import SimpleNamespace
    from grounded_video_llm_amd.model import LLAVA_NEXT_VIDEO
    m = LLAVA_NEXT_VIDEO.__new__(LLAVA_NEXT_VIDEO)
    m.engine, m.geo = _NoEngine(), SimpleNamespace(vocab=640)
    samples = {"prompts": ["a", "b"], "video_ids": ["x", "y"], "spatial_pixel_values": torch.zeros((2, 1))}
    with pytest.raises(ValueError, match="needs the negative prompt"):
        m.generate(samples, guidance_scale=2.0)
    with pytest.raises(ValueError, match="exactly one"):
        m.generate(samples, guidance_scale=2.0, negative_prompts=["n", "n"], negative_prompt_ids=[[1], [2]])
    with pytest.raises(ValueError, match="2 samples need 2 negative prompts"):
        m.generate(samples, guidance_scale=2.0, negative_prompts=["n"])
    with pytest.raises(ValueError, match="list of strings"):
        m.generate(samples, guidance_scale=2.0, negative_prompts="n")
    with pytest.raises(ValueError, match="outside the vocabulary"):
        m.generate(samples, guidance_scale=2.0, negative_prompt_ids=[[1], [640]])
    with pytest.raises(ValueError, match="num_beams > 1 is not supported"):
        m.generate(samples, guidance_scale=2.0, negative_prompts=["n", "n"], num_beams=2)
    with pytest.raises(ValueError, match="guidance_scale"):
        m.generate(samples, guidance_scale=float("nan"), negative_prompts=["n", "n"])
    with pytest.raises(ValueError, match="generate_shared.*not supported"):
        m.generate_shared({"spatial_pixel_values": torch.zeros((1, 1))}, ["a"], guidance_scale=2.0, negative_prompts=["n"])
    assert m._check_guidance(dict(guidance_scale=1, num_beams=4), 2) is None              # off: nothing else is looked at, as in HF
