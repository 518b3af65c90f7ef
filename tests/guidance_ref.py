"""Classifier-free guidance against a negative sequence (HF generate(guidance_scale=s, negative_prompt_ids=...); transformers'
UnbatchedClassifierFreeGuidanceLogitsProcessor) restated for the tests: the guided row in float64, the tolerance an fp32 evaluation of it is allowed, and the
generation loop -- two teacher-forced streams, one selection.  tests/test_guidance_ref_cpu.py pins both against the installed transformers; the GPU tests compare
the library (guidance_rows_kernel / follow_commit_kernel, csrc/gvl_pick.hip) against them."""
import torch

SCALES = (1.5, 3.0, 0.5, -1.0)


def guided_row(cond, neg, scale):
    """float64: scale * (log_softmax(cond) - log_softmax(neg)) + log_softmax(neg); also returns the two log-softmax rows."""
    c = torch.log_softmax(torch.as_tensor(cond, dtype=torch.float64), -1)
    u = torch.log_softmax(torch.as_tensor(neg, dtype=torch.float64), -1)
    return float(scale) * (c - u) + u, c, u


def e(x):
    """the project's per-entry log-softmax tolerance (tests/test_gpu_logprobs.py::tol)"""
    return 1e-4 + 1e-5 * x.abs()


def bound(cond, neg, scale):
    """What an entry of an fp32 guided row may differ from guided_row by: two log-softmax errors scaled, one unscaled, plus three fp32 roundings (the subtract, the
    multiply, the add) -- |s| (e(Lc) + e(Lu)) + e(Lu) + 2^-22 (|s| |Lc - Lu| + |G|).  Derived from the formula, not fitted."""
    G, c, u = guided_row(cond, neg, scale)
    s = abs(float(scale))
    return s * (e(c) + e(u)) + e(u) + 2.0 ** -22 * (s * (c - u).abs() + G.abs())


def rows(g, B, n):
    """The row spreads of tests/test_gpu_logprobs.py::_rows without its -inf entries (raw logits are finite by contract): wide ranges, ties with entry 0, a tie
    at the maximum."""
    x = torch.randn((B, n), generator=g) * torch.tensor([0.5, 2.0, 4.0, 30.0])[torch.arange(B) % 4][:, None]
    x[:, 5::97] = x[:, :1]
    x[:, 11] = x.max(dim=1).values
    x[:, 3] = x[:, 11]
    return x


def op_cases():
    """(n, pairs) of the operator tests, and the rows of one case: 2 * pairs + 1 rows, pair p = (row p, row pairs + p), the last row named by nobody."""
    return [(n, p) for n in (400, 1025, 32064, 128256) for p in (1, 3, 8)]


def op_rows(n, pairs):
    return rows(torch.Generator().manual_seed(n * 31 + pairs), 2 * pairs + 1, n)


def generate(step_cond, step_neg, first_cond, first_neg, scale, max_new, eos, select):
    """The guided generation loop.  first_cond / first_neg: the two prompts' last-row logits; step_cond(tok) / step_neg(tok) feed ONE token to the conditional /
    negative stream and return its logits row -- both streams are fed the SAME token, the one `select(step index, guided row)` picked from the guided row, the first
    token included.  Returns the ids (eos included)."""
    ids = []
    lc, lu = first_cond, first_neg
    while True:
        G = scale * (torch.log_softmax(lc.float(), -1) - torch.log_softmax(lu.float(), -1)) + torch.log_softmax(lu.float(), -1)
        t = int(select(len(ids), G))
        ids.append(t)
        if len(ids) >= max_new or (eos is not None and t == eos):
            return ids
        lc, lu = step_cond(t), step_neg(t)


def greedy(step, G):
    return int(torch.argmax(G))

