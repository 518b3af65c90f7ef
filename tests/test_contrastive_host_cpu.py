"""Contrastive search on the host, without a GPU:
  1. logits.resolve_contrastive picks the mode exactly where HF's _get_generation_mode does, and validates penalty_alpha / top_k;
  2. generate(penalty_alpha=0.6, top_k=4) on a stub engine reaches Engine.contrastive_search with those values (before this mode existed the call decoded greedily);
     the combinations that are not built raise ValueError before any engine work;
  3. csrc/gvl_contrastive.h (host-only; tests/c/contrastive_check.cc includes it alone and is built with the host C++ compiler): winner / loser lists, eos, max_new,
     the limits;
  4. the prefill plan: keep_hidden switches the last-layer tail off and changes nothing else."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile
from types import SimpleNamespace

import pytest
import torch

import conftest  # noqa: F401  (puts the package on sys.path)
from grounded_video_llm_amd import logits as LP, logprobs as LPR, model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grounded-video-llm_amd", "csrc")


# ---- 1. the mode table -------------------------------------------------------------------------------------------------------------------
def test_resolve_contrastive_mode_table():
    on = dict(penalty_alpha=0.6, top_k=4)
    assert LP.resolve_contrastive(on) == (4, 0.6)
    assert LP.resolve_contrastive(dict(on, do_sample=False, num_beams=1)) == (4, 0.6)
    assert LP.resolve_contrastive(dict(on, num_beams=None)) == (4, 0.6)
    assert LP.resolve_contrastive(dict(penalty_alpha=1, top_k=2)) == (2, 1.0)
    assert LP.resolve_contrastive(dict(penalty_alpha=0.6, top_k=16)) == (16, 0.6)
    # every condition HF names, one at a time
    assert LP.resolve_contrastive(dict()) is None
    assert LP.resolve_contrastive(dict(top_k=4)) is None
    assert LP.resolve_contrastive(dict(penalty_alpha=None, top_k=4)) is None
    assert LP.resolve_contrastive(dict(penalty_alpha=0.0, top_k=4)) is None
    assert LP.resolve_contrastive(dict(penalty_alpha=0.6)) is None
    assert LP.resolve_contrastive(dict(penalty_alpha=0.6, top_k=None)) is None
    assert LP.resolve_contrastive(dict(penalty_alpha=0.6, top_k=1)) is None
    assert LP.resolve_contrastive(dict(on, do_sample=True)) is None
    assert LP.resolve_contrastive(dict(on, num_beams=2)) is None
    assert LP.resolve_contrastive(dict(on, do_sample=True, top_k=50)) is None            # top_k is the sampling warper there: any size


def test_resolve_contrastive_errors():
    for a in (-0.1, 1.5, float("nan"), "0.6", True):
        with pytest.raises(ValueError, match="penalty_alpha"):
            LP.resolve_contrastive(dict(penalty_alpha=a, top_k=4))
    with pytest.raises(ValueError, match="penalty_alpha"):                                # validated whatever the mode
        LP.resolve_contrastive(dict(penalty_alpha=2.0, do_sample=True))
    with pytest.raises(ValueError, match=r"at most 16"):
        LP.resolve_contrastive(dict(penalty_alpha=0.6, top_k=17))
    with pytest.raises(ValueError, match="top_k"):
        LP.resolve_contrastive(dict(penalty_alpha=0.6, top_k=4.0))
    assert LP.MAX_CONTRASTIVE_TOP_K == 16


# ---- 2. generate() on a stub engine ---------------------------------------------------------------------------------------------------------
class _StubEngine:
    """Records every call; the ones that generate(), generate_shared() and score() read a value from return one.  Sequence ids are the lowest free slot from 5 up, so
    an alloc / free pair at a time always sees 5 and sequences that live together are told apart.  logits=True: prefills and teacher-forced steps hand back real
    (deterministic) rows, for the searches that compute on them on the host.  pool=n: the KV pool holds n sequences, one more is refused with ERR_OOM."""
    def __init__(self, logits=False, vocab=640, pool=None):
        self.calls = []
        self.device = "cpu"
        self._logits, self._vocab, self._live, self._pool = logits, vocab, set(), pool

    def _need(self, n):
        if self._pool is not None and len(self._live) + n > self._pool:
            from grounded_video_llm_amd import lib as L
            e = L.GvlError("gvl_seq_alloc failed (status %d): the KV pool is exhausted" % L.ERR_OOM)
            e.status = L.ERR_OOM
            raise e

    def _alloc(self):
        self._need(1)
        sid = next(i for i in range(5, 4096) if i not in self._live)
        self._live.add(sid)
        return sid

    def _row(self, tok):
        return torch.sin(torch.arange(self._vocab, dtype=torch.float32) * (0.37 * (int(tok) % 97 + 1)))

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append((name, a, kw))
            if name == "splice":
                return torch.zeros((len(a[0]) - 1 + a[1].shape[0], 8))
            if name == "embed_ids":
                return torch.zeros((len(a[0]), 8))
            if name in ("seq_alloc", "seq_fork", "seq_clone"):
                return self._alloc()
            if name == "seq_fanout":
                self._need(a[1])                             # all or nothing, as gvl_seq_fanout is
                return [self._alloc() for _ in range(a[1])]
            if name == "seq_free":
                self._live.discard(a[0])
                return None
            if name in ("rules_create", "grammar_create"):
                return 7 if name == "rules_create" else 9
            if name == "decode_group_info":
                return dict(max_group=16, any_size=1)
            if name == "prefill":
                if not kw.get("want_logits"):
                    return None
                return self._row(0) if self._logits else "FIRST"
            if name == "prefill_extend_batch":
                return torch.stack([self._row(0) for _ in a[0]]) if kw.get("want_logits") else None
            if name == "decode_step_logits":
                return self._row(a[1])
            if name == "decode_step_logits_batch":
                return torch.stack([self._row(t) for t in a[1]])
            if name == "op_logits_process":
                return a[0]
            if name in ("beam_search", "group_beam_search"):      # (..., with_scores, num_return=n) are the last two arguments of both
                res = ([11, 2], -0.25, [-0.125, -0.125]) if a[-1] else [11, 2]
                return [res] * kw["num_return"] if kw.get("num_return", 1) > 1 else res
            if name == "seq_read_logprobs":
                n = a[2]
                return [-0.5] * n, ([[(1, -0.5)] for _ in range(n)] if kw.get("top") else None)
            if name == "score_extend_batch":
                n = sum(1 for ids in a[2] for t in ids if t != -100)
                top = a[3] if len(a) > 3 else kw.get("top_n", 0)
                return (torch.full((n,), -0.5), torch.zeros((n,), dtype=torch.int32), torch.ones((n, 8), dtype=torch.int32) if top else None,
                        torch.full((n, 8), -0.5) if top else None)
            if name == "generate_ids":
                lp = kw.get("logprobs")
                return [1, 2] if lp is None else ([1, 2], ([-0.5, -0.5], [[(1, -0.5)], [(2, -0.5)]] if lp > 0 else None))
            if name == "contrastive_search":
                ids = [11, 12, 2]
                tr = dict(ids=[[11, 7, 8, 9], [6, 12, 8, 9], [2, 7, 8, 9]], p=[[.5, .2, .1, .1], [.4, .3, .1, .1], [.9, .05, .01, .01]],
                          pen=[[.25, .5, .5, .5], [.75, .125, .5, .5], [.5, .5, .5, .5]], sel=[0, 1, 0])
                return (ids, tr) if kw.get("with_trace") else ids
            if name in ("decode_greedy",):
                return [1, 2]
            if name == "decode_greedy_batch":
                return [[1, 2] for _ in a[0]]
            return None
        return call


class _Tok:
    eos_token_id, pad_token_id, bos_token_id = 2, 0, 1

    def batch_decode(self, ids, skip_special_tokens=True):
        return [" ".join(str(i) for i in row) for row in ids]


def _stub_model(logits=False, n_visual=6, pool=None):
    m = M.LLAVA_NEXT_VIDEO.__new__(M.LLAVA_NEXT_VIDEO)
    m.engine, m.tokenizer, m.max_txt_len = _StubEngine(logits, pool=pool), _Tok(), 64
    m.geo = SimpleNamespace(vocab=640, max_seq=4096, max_prefill=4096, rope_long=None, rope_orig_max_pos=0)
    m.tokenizer_image_token = lambda text: [1, 20, -200, 21, 22]
    m.encode_images = lambda samples: torch.zeros((len(samples.get("prompts", "v")), n_visual, 8))     # one video when the call names no prompts of its own
    m._n_visual = lambda samples: n_visual
    return m


SAMPLES = {"prompts": ["a", "b"], "video_ids": ["x", "y"], "spatial_pixel_values": torch.zeros((2, 1))}


def test_generate_routes_penalty_alpha_and_top_k_to_contrastive_search():
    m = _stub_model()
    texts = m.generate(SAMPLES, penalty_alpha=0.6, top_k=4, max_new_tokens=16)
    names = [c[0] for c in m.engine.calls]
    searches = [c for c in m.engine.calls if c[0] == "contrastive_search"]
    assert len(searches) == 2 and texts == ["11 12 2", "11 12 2"]                          # one search per sample, like beams
    for _, a, kw in searches:
        assert a[0] == 5 and a[1] == "FIRST" and a[2:6] == (4, 0.6, 16, 2)                 # seq, first logits, top_k, penalty_alpha, max_new, eos
    assert names.count("seq_keep_hidden") == 2 and names.count("seq_free") == 2
    assert names.index("seq_keep_hidden") < names.index("prefill") < names.index("contrastive_search")
    assert not any(n.startswith("decode_greedy") for n in names)                           # no fall-through to greedy
    # the search processes its own rows: the engine-wide defaults are off for the call, as for beams
    assert ("set_logits_processors", LP.OFF.args(), {}) in m.engine.calls and ("set_sampling", (False,), {}) in m.engine.calls


def test_generate_without_the_mode_stays_greedy():
    for kw in (dict(top_k=4), dict(penalty_alpha=0.0, top_k=4), dict(penalty_alpha=0.6, top_k=1)):
        m = _stub_model()
        m.generate(SAMPLES, max_new_tokens=4, **kw)
        assert not any(c[0] == "contrastive_search" for c in m.engine.calls)


def test_generate_returns_p_and_the_degeneration_penalty_with_output_scores():
    m = _stub_model()
    out = m.generate(SAMPLES, penalty_alpha=0.6, top_k=4, max_new_tokens=16, return_dict_in_generate=True, output_scores=True)
    assert isinstance(out, LPR.GenerateOutput) and out.sequences == [[11, 12, 2]] * 2
    assert out.transition_scores == [[.5, .3, .9]] * 2 and out.degeneration_penalties == [[.25, .125, .5]] * 2
    plain = m.generate(SAMPLES, penalty_alpha=0.6, top_k=4, max_new_tokens=16, return_dict_in_generate=True)
    assert plain.transition_scores is None and plain.degeneration_penalties is None and plain.sequences == [[11, 12, 2]] * 2


def test_unsupported_combinations_raise_before_any_engine_work():
    class _NoEngine:
        def __getattr__(self, name):
            raise AssertionError(f"engine.{name} reached")
    m = _stub_model()
    m.engine = _NoEngine()
    on = dict(penalty_alpha=0.6, top_k=4)
    bad = [(dict(on, guidance_scale=2.0, negative_prompts=["n", "n"]), "guidance_scale"),
           (dict(on, num_return_sequences=2), "num_return_sequences"),
           (dict(on, top_logprobs=2, return_dict_in_generate=True), "top_logprobs"),
           (dict(on, top_k=17), "at most 16"),
           (dict(penalty_alpha=1.5, top_k=4), "penalty_alpha"),
           (dict(penalty_alpha=-1.0), "penalty_alpha")]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            m.generate(SAMPLES, **kw)
    with pytest.raises(ValueError, match="generate_shared.*contrastive"):
        m.generate_shared({"spatial_pixel_values": torch.zeros((1, 1))}, ["a"], **on)


def test_the_scheduler_refuses_contrastive_search():
    from grounded_video_llm_amd import serve
    from test_host_logic import _Emb, _ScriptedEngine
    sch = serve.ClipScheduler(_ScriptedEngine(64), 2, max_active=2)
    with pytest.raises(ValueError, match="contrastive"):
        sch.submit(_Emb(4, 1), 4, penalty_alpha=0.6, top_k=4)
    with pytest.raises(ValueError, match="penalty_alpha"):
        sch.submit(_Emb(4, 1), 4, penalty_alpha=3.0)


# ---- 3. gvl_contrastive.h ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def checker():
    tmp = tempfile.mkdtemp(prefix="gvl_contrastive_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "contrastive_check")
    cmd = ["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", CSRC, os.path.join(ROOT, "tests", "c", "contrastive_check.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run(lines):
    r = subprocess.run([checker()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return [ln.split("|") for ln in r.stdout.splitlines()]


def test_header_keeps_the_winner_and_frees_the_losers_in_candidate_order():
    out = run(["init 4 8 -1",
               "step 2  30 31 32 33  7 9 11 13",        # rank 2 wins: sequence 11 lives on, 7 9 13 go back
               "step 0  40 41 42 43  11 3 7 9",         # the current sequence itself wins
               "step 3  50 51 52 53  11 3 7 9",
               "end"])
    assert out[0] == ["init 0"]
    assert out[1] == ["step 0", "11", "7 9 13"] and out[2] == ["step 0", "11", "3 7 9"] and out[3] == ["step 0", "9", "11 3 7"]
    assert out[4] == ["ids", "32 40 53", "2 0 3", "0"]


def test_header_stops_behind_eos_and_at_max_new():
    out = run(["init 2 5 41", "step 1  40 41  1 2", "end"])                       # the chosen id is eos at step 0: finished, eos is part of the output
    assert out[1] == ["step 1", "2", "1"] and out[2] == ["ids", "41", "1", "1"]
    out = run(["init 2 5 41", "step 0  40 41  1 2", "step 0  7 8  1 2", "end"])   # eos among the candidates but not chosen: the search goes on
    assert [o[0] for o in out[1:3]] == ["step 0", "step 0"] and out[3][3] == "0"
    out = run(["init 2 2 -1", "step 0  5 6  1 2", "step 1  5 6  1 3", "step 0  5 6  3 4", "end"])
    assert out[1][0] == "step 0" and out[2] == ["step 1", "3", "1"]               # the max_new-th id finishes
    assert out[3][0] == "step -1" and out[4] == ["ids", "5 6", "0 1", "1"]        # a step behind the end is refused and changes nothing


def test_header_refuses_bad_steps_and_limits():
    out = run(["init 3 4 -1", "step 3  1 2 3  4 5 6", "step -1  1 2 3  4 5 6", "step 0  1 2 3  4 4 6", "end"])
    assert [o[0] for o in out[1:4]] == ["step -1"] * 3 and out[4] == ["ids", "", "", "0"]
    assert run(["init 1 4 -1"]) == [["init -1"]] and run(["init 17 4 -1"]) == [["init -1"]] and run(["init 2 0 -1"]) == [["init -1"]]
    ok = "refusal 4 0.6 16 8192 16 640 3072"
    assert run([ok]) == [["refusal", "-"]]
    for line, word in (("refusal 1 0.6 16 8192 16 640 3072", "top_k"), ("refusal 17 0.6 16 8192 16 640 3072", "top_k"), ("refusal 4 1.5 16 8192 16 640 3072", "penalty_alpha"),
                       ("refusal 4 -0.1 16 8192 16 640 3072", "penalty_alpha"), ("refusal 4 nan 16 8192 16 640 3072", "penalty_alpha"), ("refusal 4 0.6 0 8192 16 640 3072", "max_new_tokens"),
                       ("refusal 4 0.6 9000 8192 9000 640 3072", "max_new_tokens"), ("refusal 4 0.6 16 8192 15 640 3072", "cap"), ("refusal 16 0.6 16 8192 16 15 3072", "vocabulary"),
                       ("refusal 2 0.6 16 8192 16 3 3072", "vocabulary")):
        assert word in run([line])[0][1], line
    assert run(["refusal 16 0 16 8192 16 16 3072", "refusal 2 1 1 8192 1 4 3072"]) == [["refusal", "-"]] * 2
    # the candidate rows must fit the ranking kernel's LDS: rows (4 / 8 / 16) x hidden x 2 bytes <= 128 KiB
    fits = ["refusal 16 0.6 16 8192 16 640 4096", "refusal 8 0.6 16 8192 16 640 8192", "refusal 9 0.6 16 8192 16 640 4096", "refusal 4 0.6 16 8192 16 640 8192"]
    assert run(fits) == [["refusal", "-"]] * 4
    for line in ("refusal 9 0.6 16 8192 16 640 4160", "refusal 16 0.6 16 8192 16 640 8192", "refusal 8 0.6 16 8192 16 640 8256"):
        assert "LDS" in run([line])[0][1], line
    for line in ("refusal 4 0.6 16 8192 16 640 96", "refusal 4 0.6 16 8192 16 640 0"):
        assert "multiple of 64" in run([line])[0][1], line


# ---- 4. the prefill plan ---------------------------------------------------------------------------------------------------------------------
PLAN_SRC = r"""
#include <cstdio>
#include <cstring>
#include "gvl_prefill_plan.h"
int main() {
  int S, nf_ok, tail_knob, keep;
  while (std::scanf("%d %d %d %d", &S, &nf_ok, &tail_knob, &keep) == 4) {
    PrefillGeometry g{};
    g.nb = 1; g.lens[0] = S; g.rope_orig_max_pos = 4096; g.long_table = true; g.page_id_cap = 256;
    g.hidden = 3072; g.qkv_width = 9216; g.gate_up_width = 16384; g.fused_weights = nf_ok != 0; g.keep_hidden = keep != 0;
    PrefillKnobs k{1, true, tail_knob != 0, true};
    PrefillPlan p;
    const int rc = prefill_plan(g, k, &p);
    if (rc) { std::printf("refused %d\n", rc); continue; }
    std::printf("%d %d|%d %d %d|%d|", p.tail ? 1 : 0, p.last_rows, p.M, p.nf ? 1 : 0, p.batched_table ? 1 : 0, p.n_steps);
    for (int i = 0; i < p.n_steps; ++i) { const PrefillStep& s = p.steps[i]; std::printf("%d.%d.%d.%d.%d.%d.%d.%d.%d ", s.kind, s.form, s.first, s.count, s.B, s.S, s.pos0, s.Sk, s.use_long ? 1 : 0); }
    std::printf("|%d", p.n_chunks);
    for (int i = 0; i < p.n_chunks; ++i) std::printf(" %d", p.chunks[i]);
    std::printf("\n");
  }
  // what a keep-hidden member cannot be part of: a group, a cached prefix, a loss tail, a score tail
  PrefillGeometry g{}; PrefillKnobs k{1, true, true, true}; PrefillPlan p;
  g.page_id_cap = 256; g.hidden = 3072; g.keep_hidden = true;
  g.nb = 2; g.lens[0] = g.lens[1] = 10; std::printf("group %d\n", prefill_plan(g, k, &p));
  g.nb = 1; g.pos0[0] = 64; std::printf("prefix %d\n", prefill_plan(g, k, &p));
  g.pos0[0] = 0; g.loss = true; std::printf("loss %d\n", prefill_plan(g, k, &p));
  g.loss = false; g.score = true; std::printf("score %d\n", prefill_plan(g, k, &p));
  g.score = false; std::printf("alone %d\n", prefill_plan(g, k, &p));
  return 0;
}
"""


def test_keep_hidden_turns_the_last_layer_tail_off_and_nothing_else():
    tmp = tempfile.mkdtemp(prefix="gvl_plan_keep_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    src, exe = os.path.join(tmp, "plan_keep.cc"), os.path.join(tmp, "plan_keep")
    with open(src, "w") as f:
        f.write(PLAN_SRC)
    r = subprocess.run(["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = [(S, nf, knob) for S in (1, 63, 129, 3520, 5000) for nf in (0, 1) for knob in (0, 1)]
    lines = [f"{S} {nf} {knob} {keep}" for S, nf, knob in cases for keep in (0, 1)]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rows = [ln.split("|") for ln in out.stdout.splitlines()]
    body, tailrows = rows[:len(lines)], rows[len(lines):]
    for i, (S, nf, knob) in enumerate(cases):
        plain, keep = body[2 * i], body[2 * i + 1]
        assert plain[0] == (f"{knob} {2 if knob else 0}"), (S, nf, knob, plain)        # without keep_hidden the knob decides (GVL_PREFILL_LAST_TAIL = 2, STRIDED = 0)
        assert keep[0] == "0 0", (S, nf, knob, keep)                                   # with it: no tail, the last row is read in place
        assert keep[1:] == plain[1:], (S, nf, knob)                                    # every other field as without it
    assert [r[0] for r in tailrows] == ["group -6", "prefix -6", "loss -6", "score -6", "alone 0"]
