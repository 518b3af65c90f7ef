"""CPU: the fp64 restatement of the sampling stages (tests/warpers_ref.py) against the installed transformers' warper classes chained in
GenerationMixin._get_logits_processor's order, and beam.warp_scores (min_tokens_to_keep = 2) against the same classes; logits.resolve_sampling /
request_sampling raise HF's messages.  top-p stays off in the HF comparison: the device keeps a tie at its cut where HF splits it by position
(a documented decision, include/gvl.h), so its rule is checked on its own."""
import math

import numpy as np
import pytest
import torch

import warpers_ref as WR
from grounded_video_llm_amd import beam as B, logits as LP

LPW = pytest.importorskip("transformers.generation.logits_process")

SCALES = (0.5, 2.0, 4.0, 30.0)


def make_row(rng, n, scale):
    x = rng.standard_normal(n).astype(np.float32) * np.float32(scale)
    x[5::97] = x[0]                                                 # ties with entry 0
    if rng.integers(2):
        x[7::13] = -np.inf                                          # -inf entries
    x[11] = x.max()                                                 # a tie at the maximum
    x[3] = x[11]
    if rng.integers(4) == 0:
        x[20:28] = x[20]                                            # a block of tied scores somewhere in the body
    return x


def hf_chain(x, T, top_k, min_p, typical_p, eps, eta, min_keep=1, top_p=None, dtype=torch.float64):
    chain = [LPW.TemperatureLogitsWarper(float(T))] if T != 1.0 else []
    if top_k:
        chain.append(LPW.TopKLogitsWarper(top_k=int(top_k), min_tokens_to_keep=min_keep))
    if top_p is not None and top_p < 1.0:
        chain.append(LPW.TopPLogitsWarper(top_p=float(top_p), min_tokens_to_keep=min_keep))
    if min_p is not None:
        chain.append(LPW.MinPLogitsWarper(min_p=float(min_p), min_tokens_to_keep=min_keep))
    if typical_p is not None and typical_p < 1.0:
        chain.append(LPW.TypicalLogitsWarper(mass=float(typical_p), min_tokens_to_keep=min_keep))
    if eps is not None and 0.0 < eps < 1.0:
        chain.append(LPW.EpsilonLogitsWarper(epsilon=float(eps), min_tokens_to_keep=min_keep))
    if eta is not None and 0.0 < eta < 1.0:
        chain.append(LPW.EtaLogitsWarper(epsilon=float(eta), min_tokens_to_keep=min_keep))
    s = torch.as_tensor(x, dtype=dtype)[None, :]
    ids = torch.zeros((1, 1), dtype=torch.long)
    for w in chain:
        s = w(ids, s)
    return s[0]


def settings(rng, i):
    """every warper on in half of the rows, independently (bit j of i), with parameters spread over their useful ranges"""
    return dict(T=(0.5, 0.7, 1.0, 1.3)[int(rng.integers(4))], top_k=(0, 5, 50, 400)[int(rng.integers(4))],
                min_p=(float(rng.choice([0.02, 0.1, 0.3, 0.7])) if i & 1 else None),
                typical_p=(float(rng.choice([0.2, 0.5, 0.9, 0.97])) if i & 2 else None),
                eps=(float(rng.choice([3e-4, 1e-3, 9e-3, 0.05])) if i & 4 else None),
                eta=(float(rng.choice([3e-4, 2e-3, 0.02, 0.3])) if i & 8 else None))


@pytest.mark.parametrize("n,rows", [(64, 496), (1000, 496), (32064, 208)])
def test_restatement_matches_transformers(n, rows):
    rng = np.random.default_rng(1000 + n)
    seen = set()
    for i in range(rows):
        x = make_row(rng, n, SCALES[i % 4])
        st = settings(rng, i // 4)
        seen.add((i // 4) & 15)
        want = torch.isfinite(hf_chain(x, **st)).numpy()
        got = WR.keep_mask(x, st["T"], st["top_k"], None, st["min_p"], st["typical_p"], st["eps"], st["eta"])
        assert np.array_equal(got, want), (n, i, st, int(got.sum()), int(want.sum()))
        assert got.any()
    assert len(seen) == 16                                          # every on / off combination of the four warpers ran


def test_restatement_edge_cases():
    x = np.array([1.0, 1.0, 0.0, -np.inf, -2.0], dtype=np.float32)
    assert WR.keep_mask(x, min_p=1.0).tolist() == [True, True, False, False, False]            # min_p 1: the maximum and its ties
    assert WR.keep_mask(x, epsilon_cutoff=0.99).tolist() == [True, True, False, False, False]  # nothing reaches the cut: the largest score stays
    assert WR.keep_mask(x, eta_cutoff=0.99).tolist() == [True, True, False, False, False]
    # typical_p may drop the maximum: one likely token among many equally unlikely ones
    y = np.full(2001, 0.0, dtype=np.float32); y[0] = 7.0
    keep = WR.keep_mask(y, typical_p=0.3)
    assert not keep[0] and keep[1:].all()
    assert torch.equal(torch.as_tensor(keep), torch.isfinite(hf_chain(y, 1.0, 0, None, 0.3, None, None)))
    # the top-p rule of the device: kept iff the mass of strictly larger scores is < top_p; the tie at the cut stays whole
    z = np.log(np.array([0.4, 0.2, 0.2, 0.1, 0.1], dtype=np.float64)).astype(np.float32)
    assert WR.keep_mask(z, top_p=0.5).tolist() == [True, True, True, False, False]
    rep = {}
    WR.keep_mask(z, top_p=0.5, report=rep)
    assert abs(rep["top_p"] - 0.1) < 1e-6
    # a greedy selection keeps every finite entry and takes the first maximum
    tok, margin, keep = WR.select(x, None)
    assert tok == 0 and margin == math.inf and keep.tolist() == [True, True, True, False, True]
    tok, margin, keep = WR.select(x, dict(do_sample=True, temperature=0.7, top_k=0, min_p=0.5, seed=3, stream=1), step=4)
    assert keep.tolist() == [True, True, False, False, False] and tok in (0, 1) and margin > 0


def test_report_margins():
    rng = np.random.default_rng(5)
    x = make_row(rng, 1000, 2.0)
    rep = {}
    keep = WR.keep_mask(x, 0.7, 50, None, 0.1, 0.9, 1e-3, 2e-3, report=rep)
    assert set(rep) == {"min_p", "typical_p", "epsilon_cutoff", "eta_cutoff"}
    below, upto, gap = rep["typical_p"]
    assert below < 0.9 <= upto and gap > 0
    assert (rep["min_p"] >= 0).all() and keep.sum() >= 1


@pytest.mark.parametrize("n", [64, 1000])
def test_beam_warp_scores_matches_transformers(n):
    """beam-sample's host warpers: the same seven stages with min_tokens_to_keep = 2, as HF sets it for num_beams > 1, on fp32 log-probability rows"""
    rng = np.random.default_rng(77 + n)
    for i in range(160):
        x = torch.log_softmax(torch.as_tensor(make_row(rng, n, SCALES[i % 4])), dim=-1)
        st = settings(rng, i // 2)
        top_p = (None, 0.9, 0.5)[i % 3]
        want = hf_chain(x, st["T"], st["top_k"], st["min_p"], st["typical_p"], st["eps"], st["eta"], min_keep=2, top_p=top_p, dtype=torch.float32)
        got = B.warp_scores(x[None, :], st["T"], st["top_k"], top_p, 2, st["min_p"], st["typical_p"], st["eps"], st["eta"])[0]
        assert torch.equal(torch.isfinite(got), torch.isfinite(want)), (n, i, st, top_p)
        assert torch.equal(got, want)
        assert int(torch.isfinite(got).sum()) >= 2
    base = torch.log_softmax(torch.randn(3, 50, generator=torch.Generator().manual_seed(1)), dim=-1)
    assert torch.equal(B.warp_scores(base, 0.7, 10, 0.9), B.warp_scores(base, 0.7, 10, 0.9, 2, None, None, None, None))    # the new stages default to off


def test_resolve_sampling_messages():
    assert LP.resolve_sampling({}) == dict(min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None)
    assert LP.resolve_sampling(dict(min_p=0.1, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=2e-3)) == dict(min_p=0.1, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=2e-3)
    assert LP.resolve_sampling(dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0)) == dict(min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None)
    for kw, cls, arg in ((dict(min_p=2.0), LPW.MinPLogitsWarper, dict(min_p=2.0)), (dict(min_p=-0.1), LPW.MinPLogitsWarper, dict(min_p=-0.1)),
                         (dict(typical_p=0.0), LPW.TypicalLogitsWarper, dict(mass=0.0)), (dict(typical_p=1.5), LPW.TypicalLogitsWarper, dict(mass=1.5)),
                         (dict(epsilon_cutoff=1.0), LPW.EpsilonLogitsWarper, dict(epsilon=1.0)), (dict(epsilon_cutoff=-1e-3), LPW.EpsilonLogitsWarper, dict(epsilon=-1e-3)),
                         (dict(eta_cutoff=1.0), LPW.EtaLogitsWarper, dict(epsilon=1.0))):
        with pytest.raises(ValueError) as hf:
            cls(**arg)
        with pytest.raises(ValueError) as ours:
            LP.resolve_sampling(kw)
        assert str(ours.value) == str(hf.value)


def test_request_sampling():
    assert LP.request_sampling() is ...
    assert LP.request_sampling(do_sample=False, temperature=0.3) == dict(do_sample=False)
    got = LP.request_sampling(temperature=0.7, min_p=0.1, seed=9)
    assert got == dict(do_sample=True, temperature=0.7, top_k=50, top_p=None, seed=9, stream=0, min_p=0.1, typical_p=None, epsilon_cutoff=None, eta_cutoff=None)
    assert LP.request_sampling(do_sample=True)["temperature"] == 1.0 and LP.request_sampling(do_sample=True, top_k=0)["top_k"] == 0
    for kw in (dict(temperature=0.0), dict(temperature=float("nan")), dict(top_k=-1), dict(top_p=1.5), dict(min_p=2.0), dict(typical_p=0.0), dict(eta_cutoff=3.0),
               dict(do_sample=False, epsilon_cutoff=1.0)):
        with pytest.raises(ValueError):
            LP.request_sampling(**kw)
    with pytest.raises(ValueError, match="strictly positive float"):
        LP.request_sampling(temperature=-1.0)
