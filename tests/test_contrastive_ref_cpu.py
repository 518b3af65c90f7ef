"""tests/contrastive_ref.py -- the float64 restatement of HF contrastive search that the GPU tests are built on -- against a literal torch transcription of
transformers 4.40.1's `_ranking_fast` [ext], on random inputs whose scores are separated, and its tie rules on hand-made inputs."""
import numpy as np
import pytest
import torch

import contrastive_ref as R


def _ranking_fast(context_hidden, next_hidden, next_top_k_probs, alpha, beam_width):
    """transformers 4.40.1 generation/utils.py `_ranking_fast`, line for line (context_hidden [B*K, S, D], next_hidden [B*K, 1, D], next_top_k_probs [B, K])."""
    norm_context_hidden = context_hidden / context_hidden.norm(dim=2, keepdim=True)
    norm_next_hidden = next_hidden / next_hidden.norm(dim=2, keepdim=True)
    cosine_matrix = torch.matmul(norm_context_hidden, norm_next_hidden.transpose(1, 2)).squeeze(-1)  # [B*K, S]
    degeneration_penalty, _ = torch.max(cosine_matrix, dim=-1)  # [B*K]
    next_top_k_probs = next_top_k_probs.view(-1)  # [B*K]
    contrastive_score = (1.0 - alpha) * next_top_k_probs - alpha * degeneration_penalty
    contrastive_score = torch.stack(torch.split(contrastive_score, beam_width))  # [B, K]
    _, selected_idx = contrastive_score.max(dim=-1)  # [B]
    return selected_idx, degeneration_penalty, contrastive_score


@pytest.mark.parametrize("k,S,D", [(2, 1, 8), (4, 63, 128), (5, 65, 96), (16, 300, 64)])
@pytest.mark.parametrize("alpha", [0.0, 0.3, 0.6, 1.0])
def test_ranking_equals_the_transcription_of_ranking_fast(k, S, D, alpha):
    checked = 0
    for seed in range(12):
        g = torch.Generator().manual_seed(101 * seed + 7 * k + S)
        ctx = torch.randn((S, D), generator=g, dtype=torch.float64)
        cand = torch.randn((k, D), generator=g, dtype=torch.float64)
        row = 2.0 * torch.randn((max(3 * k, 40),), generator=g, dtype=torch.float64)
        ids, p, p_all = R.top_k_candidates(row.numpy(), k)
        tv, ti = torch.topk(torch.softmax(row, dim=-1), k)                       # HF: top_k_probs, top_k_ids = torch.topk(next_probs, dim=-1, k=top_k)
        assert ids.tolist() == ti.tolist() and np.allclose(p, tv.numpy(), rtol=0, atol=1e-15)
        sel_hf, pen_hf, sc_hf = _ranking_fast(ctx[None].expand(k, S, D), cand[:, None, :], tv[None], alpha, k)
        pen, _ = R.degeneration_penalty(cand.numpy(), ctx.numpy())
        sel, sc = R.select(p, pen, alpha)
        assert np.abs(pen - pen_hf.numpy()).max() <= 1e-12 and np.abs(sc - sc_hf.numpy()[0]).max() <= 1e-12
        if R.margin(sc) >= 1e-9:                                                 # separated scores: the choice is the same
            assert sel == int(sel_hf[0])
            checked += 1
    assert checked >= 6


def test_tie_rules():
    # equal probabilities: the lower token id is the better candidate
    ids, p, _ = R.top_k_candidates([0.0, 1.0, 1.0, -1.0, 1.0], 3)
    assert ids.tolist() == [1, 2, 4] and p[0] == p[1] == p[2]
    # equal scores: the lower rank wins
    assert R.select([0.25, 0.25, 0.125], [0.5, 0.5, 0.5], 0.5)[0] == 0
    assert R.select([0.125, 0.25, 0.25], [0.75, 0.5, 0.5], 0.5)[0] == 1
    # alpha = 0 is the most probable candidate, alpha = 1 the least similar one
    assert R.select([0.5, 0.25], [0.9, 0.1], 0.0)[0] == 0 and R.select([0.5, 0.25], [0.9, 0.1], 1.0)[0] == 1


def test_the_penalty_is_the_maximum_over_every_context_row_and_scale_free():
    g = np.random.default_rng(3)
    ctx, cand = g.standard_normal((9, 16)), g.standard_normal((3, 16))
    ctx[5] = 4.0 * cand[1]                                                        # a parallel row: cosine exactly 1 whatever its length
    pen, arg = R.degeneration_penalty(cand, ctx)
    assert abs(pen[1] - 1.0) <= 1e-15 and arg[1] == 5
    pen2, _ = R.degeneration_penalty(3.0 * cand, 0.5 * ctx)
    assert np.abs(pen - pen2).max() <= 1e-15
    assert np.allclose(R.degeneration_penalty(cand, ctx[:1])[0], R.cosine_matrix(cand, ctx)[:, 0])


def test_the_loop_appends_the_winner_to_the_context_and_stops_behind_eos():
    D, V = 8, 12
    g = np.random.default_rng(11)
    E, W = g.standard_normal((V, D)), g.standard_normal((V, D))

    def step(ids, tok):
        h = E[tok] + 0.1 * len(ids)
        return h, W @ h
    ctx = g.standard_normal((4, D))
    out, trace = R.contrastive_search(step, W @ ctx[-1], ctx, 3, 0.6, 6)
    assert len(out) == 6 and all(t["ids"][t["sel"]] == o for t, o in zip(trace, out))
    # replay by hand: step t's penalties see the prompt rows and the t winners before it
    hist = list(ctx)
    for t, tr in enumerate(trace):
        hs = np.stack([step(out[:t], i)[0] for i in tr["ids"]])
        assert np.allclose(tr["pen"], R.degeneration_penalty(hs, np.stack(hist))[0])
        hist.append(hs[tr["sel"]])
    eos = out[2]
    cut, _ = R.contrastive_search(step, W @ ctx[-1], ctx, 3, 0.6, 6, eos=eos)
    assert cut == out[:out.index(eos) + 1]
    banned = out[0]
    proc, _ = R.contrastive_search(step, W @ ctx[-1], ctx, 3, 0.6, 4, process=lambda ids, row: np.where(np.arange(V) == banned, -np.inf, row))
    assert banned not in proc
