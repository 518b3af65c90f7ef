"""Contrastive search as transformers 4.40.1 computes it (GenerationMixin._contrastive_search and _ranking_fast [ext]), restated in float64 for a batch of one and
unpadded sequences.  transformers 4.40.1 is not installed here and later releases moved the mode out of the library, so THIS file is the authority the tests of
gvl_contrastive_search (csrc/gvl_contrastive.hip) and of generate(penalty_alpha=, top_k=) are built on.

With h_j = outputs.hidden_states[-1] of context row j -- the state AFTER the final RMSNorm (models/modeling_phi3.py:1367-1371; Llama likewise), for every prompt row,
the visual ones included, and every token chosen so far -- one step, the first token included, is:
  1. row = the last logits after the logits processors (HF: logit_for_next_step = logits_processor(input_ids, logits)).  A STATED CHOICE: no warpers.
     generate() passes no warpers in this mode (it builds the warper list for the sampling modes only); this restatement and the library apply none, whatever
     temperature / top_p the call names.
  2. p = softmax(row) over the whole vocabulary; the candidates are the top_k largest p (torch.topk leaves ties unspecified: here ties go to the LOWER token id).
  3. each candidate token is run one step on the current context: its hidden state g_i and its logits.
  4. pen_i = max_j cos(g_i, h_j) over every context row j (the candidates' own rows are not part of the context); score_i = (1 - alpha) p_i - alpha pen_i; the
     arg-max is chosen (torch.max: the first maximum, i.e. ties go to the LOWER candidate rank).
  5. the chosen token is appended, g_i joins the context, its logits are the next step's row.
  6. stop behind eos (it is part of the output) or at max_new_tokens.
Everything below is float64 numpy; nothing here knows the library."""
import numpy as np


def softmax64(row):
    x = np.asarray(row, dtype=np.float64)
    m = x.max()
    e = np.exp(x - m)
    return e / e.sum()


def top_k_candidates(row, k):
    """(ids [k], p [k], p_all): the k largest p = softmax(row), p descending, ties to the lower token id."""
    p = softmax64(row)
    order = np.lexsort((np.arange(p.size), -p))
    ids = order[:k]
    return ids, p[ids], p


def cosine_matrix(cand_h, ctx_h):
    """cos(g_i, h_j) [k, S] in float64 (rows are normalised first, as _ranking_fast does)."""
    g = np.asarray(cand_h, dtype=np.float64)
    h = np.asarray(ctx_h, dtype=np.float64)
    g = g / np.linalg.norm(g, axis=1, keepdims=True)
    h = h / np.linalg.norm(h, axis=1, keepdims=True)
    return g @ h.T


def degeneration_penalty(cand_h, ctx_h):
    """pen [k] = max_j cos(g_i, h_j) and the arg-max rows [k]."""
    c = cosine_matrix(cand_h, ctx_h)
    return c.max(axis=1), c.argmax(axis=1)


def scores(p, pen, alpha):
    return (1.0 - float(alpha)) * np.asarray(p, dtype=np.float64) - float(alpha) * np.asarray(pen, dtype=np.float64)


def select(p, pen, alpha):
    """(selected rank, score [k]): the arg-max of the contrastive score, ties to the lower rank."""
    s = scores(p, pen, alpha)
    return int(np.argmax(s)), s               # np.argmax returns the first maximum


def margin(s):
    """best minus second-best score (inf for one candidate)."""
    t = np.sort(np.asarray(s, dtype=np.float64))[::-1]
    return float(t[0] - t[1]) if t.size > 1 else float("inf")


def contrastive_search(step, first_row, ctx_hidden, k, alpha, max_new, eos=None, process=None):
    """The whole loop over a model given as step(ids_so_far, token) -> (hidden [D], logits [V]) of `token` fed behind the context + ids_so_far.
    first_row: the prompt's last logits; ctx_hidden [S, D]: the prompt's hidden states; process(ids_so_far, row) -> row (the logits processors; None: none).
    Returns (ids, trace) with trace = list of dicts(ids, p, pen, sel) per step."""
    ctx = [np.asarray(h, dtype=np.float64) for h in ctx_hidden]
    row, out, trace = np.asarray(first_row, dtype=np.float64), [], []
    while len(out) < max_new:
        if process is not None:
            row = np.asarray(process(list(out), row), dtype=np.float64)
        ids, p, _ = top_k_candidates(row, k)
        nxt = [step(list(out), int(t)) for t in ids]
        pen, _ = degeneration_penalty(np.stack([h for h, _ in nxt]), np.stack(ctx))
        sel, _ = select(p, pen, alpha)
        trace.append(dict(ids=[int(t) for t in ids], p=p.tolist(), pen=pen.tolist(), sel=sel))
        out.append(int(ids[sel]))
        ctx.append(np.asarray(nxt[sel][0], dtype=np.float64))
        row = np.asarray(nxt[sel][1], dtype=np.float64)
        if eos is not None and out[-1] == eos:
            break
    return out, trace
