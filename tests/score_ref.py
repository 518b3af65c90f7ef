"""float64 restatement of what score_rows_kernel (csrc/gvl_pick.hip) reports for one row of logits and a target id -- the reference of tests/test_gpu_score_rows.py,
itself checked against torch.log_softmax and a sort in tests/test_score_cpu.py.  No torch device work, no library.

  lp    (s_t - m) - log(sum exp(s_i - m)) in float64; -inf for a target at -inf
  rank  how many entries beat the target in the strict order (value descending, lower id first), over ALL entries, -inf included
  top   the best n FINITE entries in that order as (ids, log-probabilities), padded with (-1, -inf)"""
import math

import numpy as np


def logprobs(row):
    """float64 log-softmax of the row (entries at -inf get -inf)"""
    s = np.asarray(row, dtype=np.float64)
    m = s.max()
    with np.errstate(divide="ignore"):
        return (s - m) - math.log(np.exp(s - m).sum())


def rank(row, t):
    s = np.asarray(row, dtype=np.float64)
    return int((s > s[t]).sum() + (s[:t] == s[t]).sum())


def top(row, n, lp=None):
    s = np.asarray(row, dtype=np.float64)
    lp = logprobs(s) if lp is None else lp
    idx = np.nonzero(np.isfinite(s))[0]
    order = idx[np.lexsort((idx, -s[idx]))][:n]                     # value descending, then lower id
    ids = [int(i) for i in order]
    return ids + [-1] * (n - len(ids)), [float(lp[i]) for i in ids] + [-math.inf] * (n - len(ids))


def score_row(row, t, n_top=0):
    """-> (lp, rank, top ids, top log-probabilities) of target t; the lists are empty for n_top = 0"""
    lp = logprobs(row)
    ids, vals = top(row, n_top, lp) if n_top > 0 else ([], [])
    return float(lp[t]), rank(row, t), ids, vals
