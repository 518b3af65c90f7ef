"""fp64 restatement of a sampled token selection (select_rows_kernel, csrc/gvl_pick.hip): the seven stages in HF's order -- scores / T -> top-k -> top-p ->
min_p -> typical_p -> epsilon_cutoff -> eta_cutoff -- each stage's softmax over what the stage before left, and the Gumbel-max draw over the final kept set.
Pinned against the installed transformers' warper classes by test_warpers_cpu.py; the GPU tests compare the kernel with it.  Besides the kept set it reports,
per stage, how far the row's entries are from the stage's cut, so that a test can place its cuts where fp32 rounding cannot move them.
The temperature and top-k stages and the draw's uniforms are gvl_oracle's (sample_keep_mask, sample_uniforms)."""
import math

import numpy as np

import gvl_oracle as O

FIELDS = ("temperature", "top_k", "top_p", "min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")


def _probs(s, keep):
    """softmax of the kept scores in fp64 (0 outside the kept set) and its log."""
    z = np.where(keep, s, -np.inf)
    z = z - z.max()
    with np.errstate(divide="ignore"):
        lse = math.log(np.exp(z).sum())
    logp = z - lse
    return np.exp(logp), logp


def _protect(remove, s, keep, min_keep):
    """the min_keep largest kept scores (ties included) are never removed"""
    z = np.where(keep, s, -np.inf)
    kth = z.max() if min_keep == 1 else np.partition(z, -min(min_keep, s.size))[-min(min_keep, s.size)]
    return remove & (s < kth)


def keep_mask(x, temperature=1.0, top_k=0, top_p=None, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None, min_keep=1, report=None):
    """The final kept set of row x (bool [n]).  None / 0 switch a stage off (top_p / typical_p also at 1).
    top-p keeps an entry iff the mass of STRICTLY larger scores is < top_p (the device's documented tie rule, include/gvl.h; HF splits a tie at the cut by position).
    report (a dict, optional) receives per stage that ran:
      "top_p": min |mass of strictly larger - top_p| over the candidates
      "min_p" / "epsilon_cutoff" / "eta_cutoff": p_i / cut of every candidate (an entry of the current set that the largest-score rule does not protect)
      "typical_p": (mass of d < t, mass of d <= t, next larger distinct d minus t)"""
    x = np.asarray(x)
    full = x.astype(np.float64) / float(temperature)
    keep0 = O.sample_keep_mask(x, temperature, top_k, None) & np.isfinite(full)
    if top_p is not None and 0.0 < top_p < 1.0:
        p, _ = _probs(full, keep0)
        desc = np.sort(p[keep0])[::-1]
        before = np.concatenate([[0.0], np.cumsum(desc)[:-1]])
        greater = before[np.searchsorted(-desc, -p, side="left").clip(max=desc.size - 1)]
        if report is not None:
            report["top_p"] = float(np.min(np.abs(greater[keep0] - top_p)))
        keep0 = keep0 & ((greater < top_p) | ~_protect(np.ones_like(keep0), full, keep0, min_keep))
    idx = np.flatnonzero(keep0)                                     # the later stages see only what is left: work on those entries alone
    s = full[idx]
    keep = np.ones(idx.size, dtype=bool)

    def cut_stage(name, cut_of):
        nonlocal keep
        p, logp = _probs(s, keep)
        cut = cut_of(p, logp)
        remove = _protect(keep & (p < cut), s, keep, min_keep)
        if report is not None:
            report[name] = p[_protect(keep.copy(), s, keep, min_keep)] / cut
        keep = keep & ~remove

    if min_p:
        cut_stage("min_p", lambda p, logp: float(min_p) * p.max())
    if typical_p and typical_p < 1.0:
        p, logp = _probs(s, keep)
        ent = -float(np.sum(p[keep] * logp[keep]))
        d = np.where(keep, np.abs(-logp - ent), np.inf)
        order = np.argsort(d, kind="stable")
        cum = np.cumsum(p[order])
        last = min(int(np.sum(cum < float(typical_p))), s.size - 1)
        t = d[order[last]]
        remove = d > t
        remove[order[:min_keep]] = False
        if report is not None:
            above = d[keep & (d > t)]
            report["typical_p"] = (float(p[d < t].sum()), float(p[d <= t].sum()), float(above.min() - t) if above.size else math.inf)
        keep = keep & ~remove
    if epsilon_cutoff:
        cut_stage("epsilon_cutoff", lambda p, logp: float(epsilon_cutoff))
    if eta_cutoff:
        def eta_cut(p, logp):
            ent = -float(np.sum(p[keep] * logp[keep]))
            return min(float(eta_cutoff), math.sqrt(float(eta_cutoff)) * math.exp(-ent))
        cut_stage("eta_cutoff", eta_cut)
    out = np.zeros(x.size, dtype=bool)
    out[idx[keep]] = True
    return out


def draw(x, keep, temperature, seed, stream, step):
    """-> (token, margin): the Gumbel-max draw over `keep` with the device's counter hash; margin = the winner's perturbed score minus the runner-up's."""
    s = np.asarray(x, dtype=np.float64)
    u = O.sample_uniforms(s.size, seed, stream, step)
    with np.errstate(invalid="ignore"):
        sc = np.where(keep, (s - s[keep].max()) / float(temperature) - np.log(-np.log(u)), -np.inf)
    o = np.argsort(-sc, kind="stable")
    return int(o[0]), float(sc[o[0]] - sc[o[1]]) if keep.sum() > 1 else math.inf


def select(x, setting, step=0):
    """One row's selection by `setting` (a dict as Engine.seq_set_sampling takes it; None or do_sample False = greedy) -> (token, margin, keep)."""
    x = np.asarray(x)
    if not setting or not setting.get("do_sample", True):
        return int(np.argmax(x)), math.inf, np.isfinite(x.astype(np.float64))
    kw = {k: setting.get(k) for k in FIELDS if setting.get(k) is not None}
    kw.setdefault("top_k", 50)
    keep = keep_mask(x, **kw)
    tok, margin = draw(x, keep, kw.get("temperature", 1.0), setting.get("seed", 0), setting.get("stream", 0), step)
    return tok, margin, keep


def log_softmax_kept(x, keep, temperature=1.0):
    """fp64 log-probabilities of the distribution the token was selected from: (s - max) / T over `keep`, -inf elsewhere."""
    s = np.asarray(x, dtype=np.float64) / float(temperature)
    return _probs(s, np.asarray(keep))[1]
