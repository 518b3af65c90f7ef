"""-m gpu: the per-row selection kernel (select_rows_kernel, csrc/gvl_pick.hip) through gvl_op_select_rows: every row of a launch has its own setting, some
greedy, the sampled ones running HF's warpers temperature -> top-k -> top-p -> min_p -> typical_p -> epsilon_cutoff -> eta_cutoff.  Against the fp64
restatement tests/warpers_ref.py (pinned to transformers by test_warpers_cpu.py): the kept set exactly, the drawn token, the log-probabilities and top
lists; bit identity with today's kernels for greedy rows and for sampled rows without the new warpers; bad arguments.

Placing the cuts.  A kept set can only be compared exactly where fp32 cannot move a cut across an entry, so every row's parameters start from a nominal
value and are moved (x 1.02 per try; typical_p + 0.0013; top_p / 1.02) until the fp64 reference shows:
  min_p / epsilon / eta   no candidate's p_i within a factor 1.01 of the cut (a 17-level fp32 tree sum plus expf is ~2e-6 relative; the entropy's error of
                          <= ~3e-5 moves eta's cut by as much, relative: the margin is > 300 x the error)
  typical_p               mass below the cut's d <= mass - 1e-5, mass up to and including it >= mass + 1e-5, and the next larger distinct d >= 1e-3 above
                          (the entropy's error is common to every d and moves a pair on opposite sides of the mean by <= ~6e-5)
  top_p                   no candidate's mass of strictly larger scores within 1e-4 of top_p (50 x the fp32 sum's error)
A placement must be found within 50 tries.  At the two vocabulary widths typical_p is only used on rows with scale / T >= 4 (flatter rows there have no
entry-free band of that width), and for the same reason those flatter rows always run with a top-k (5 / 50 / 400) in front of the other cuts.  A GPU
disagreement on a placed row is a kernel bug."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import warpers_ref as WR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from grounded_video_llm_amd import lib as L  # noqa: E402

from test_gpu_logits_processors import _build  # noqa: E402  (a tiny engine: the operator needs a ctx)
from test_gpu_logprobs import _rows, ref_top, tol  # noqa: E402

WIDTHS = (100, 1000, 32064, 128256)
BATCHES = (1, 3, 16)
REPS = (0, 1, 2, 3)
SCALES = (0.5, 2.0, 4.0, 30.0)                                      # of row b % 4 (test_gpu_logprobs._rows)
TOP_N = (8, 0, 8, 3, 1, 2)
_cache = {}


@pytest.fixture(scope="module")
def eng():
    m = _build("phi3.5")
    yield m[0].engine
    m[0].engine.close()


def _margin_ok(name, rep, value):
    if name == "top_p":
        return rep >= 1e-4
    if name == "typical_p":
        below, upto, gap = rep
        return below <= value - 1e-5 and upto >= value + 1e-5 and gap >= 1e-3
    return bool(np.all((rep >= 1.01) | (rep <= 1.0 / 1.01)))


def place(x, st):
    """move the cuts of setting `st` for row x to where fp32 cannot move them (module docstring); -> the placed setting"""
    out = dict(st)
    done = dict(temperature=st["temperature"], top_k=st["top_k"])
    for name in ("top_p", "min_p", "typical_p", "epsilon_cutoff", "eta_cutoff"):
        v = st.get(name)
        if v is None:
            continue
        for _ in range(50):
            rep = {}
            WR.keep_mask(x, **done, **{name: v}, report=rep)
            if _margin_ok(name, rep[name], v):
                break
            v = v / 1.02 if name == "top_p" else v + 0.0013 if name == "typical_p" else v * 1.02
        else:
            raise AssertionError(f"no placement of {name} within 50 tries (nominal {st[name]})")
        out[name] = done[name] = v
    return out


def settings(n, B, rep):
    """row b's nominal setting: greedy for every fourth (b + rep), else sampled with its own T / top-k / top-p / seed / stream and its own subset of the new warpers"""
    rng = np.random.default_rng(n * 31 + B * 7 + rep)
    rows = []
    for b in range(B):
        if (b + rep) % 4 == 3:
            rows.append(None)
            continue
        T = (0.5, 0.7, 1.0, 1.3)[int(rng.integers(4))]
        mask = (b * 7 + rep * 5 + n) % 16                           # which of the four new warpers are on; 0 = none (bit identity with sample_kernel)
        flat = n > 1000 and SCALES[b % 4] / T < 4                   # a flat row over a whole vocabulary: entries lie denser than the 1 % band around any cut -> always top-k there
        st = dict(do_sample=True, temperature=T, top_k=((5, 50, 400, 50) if flat else (0, 5, 50, 400))[int(rng.integers(4))], top_p=(None, 0.9, 0.5, 0.95)[int(rng.integers(4))],
                  seed=int(rng.integers(0, 2 ** 63)), stream=int(rng.integers(0, 2 ** 31)),
                  min_p=float(rng.choice([0.02, 0.1, 0.3])) if mask & 1 else None,
                  typical_p=float(rng.choice([0.2, 0.5, 0.9])) if mask & 2 and (n <= 1000 or SCALES[b % 4] / T >= 4) else None,
                  epsilon_cutoff=float(rng.choice([3e-4, 1e-3, 9e-3])) if mask & 4 else None,
                  eta_cutoff=float(rng.choice([3e-4, 2e-3, 0.02])) if mask & 8 else None)
        rows.append(st)
    return rows


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(a, b) if a.dtype == torch.uint8 else torch.equal(_bits(a), _bits(b))


def run_case(eng, n, B, rep):
    """one launch of B rows; every assertion but the token escape's total; -> (sampled rows, rows that used the escape)"""
    key = (n, B, rep)
    if key in _cache:
        return _cache[key]
    x = _rows(torch.Generator().manual_seed(n + 13 * B + rep), B, n)
    xn = x.numpy()
    rows = [None if st is None else place(xn[b], st) for b, st in enumerate(settings(n, B, rep))]
    steps = [int(v) for v in np.random.default_rng(n + B + rep).integers(0, 4000, B)]
    top_n = [TOP_N[(b + rep) % 6] for b in range(B)]
    xd = x.to(DEV).contiguous()
    toks, lp, ti, tv, kept = [t.cpu() for t in eng.op_select_rows(xd, rows, top_n, steps, kept=True)]
    sampled = escaped = 0
    for b in range(B):
        st, what = rows[b], (n, B, rep, b, rows[b])
        tok, margin, keep = WR.select(xn[b], st, steps[b])
        got_keep = kept[b].numpy()
        assert set(np.unique(got_keep)) <= {0, 1}, what
        assert np.array_equal(got_keep.astype(bool), keep), (what, int(got_keep.sum()), int(keep.sum()))
        t = int(toks[b])
        assert keep[t], what
        if st is not None:
            sampled += 1
            if t != tok:
                assert margin < 1e-3, (what, t, tok, margin)
                escaped += 1
        else:
            assert t == tok, what
        T = 1.0 if st is None else st["temperature"]
        r = torch.as_tensor(WR.log_softmax_kept(xn[b], keep, T))
        assert abs(float(lp[b]) - float(r[t])) <= tol(float(r[t])), (what, float(lp[b]), float(r[t]))
        if top_n[b] > 0:
            ids, vals = ref_top(xn[b], r, top_n[b], keep)
            assert ti[b, :top_n[b]].tolist() == ids, what
            assert ti[b, top_n[b]:].tolist() == [-1] * (8 - top_n[b]), what
            for j in range(8):
                want = vals[j] if j < top_n[b] else -math.inf
                got = float(tv[b, j])
                assert (got == want == -math.inf) or abs(got - want) <= tol(want), (what, j, got, want)
        else:
            assert int(ti[b, 0]) == -2                              # no top list asked for: the fill stays
        # bit identity with today's kernels, the row on its own
        new_off = st is not None and not any(st.get(k) for k in ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff"))
        if st is None or new_off:
            if st is None:
                o = eng.op_select_logprobs(xd[b:b + 1], top_n[b], False)
            else:
                o = eng.op_select_logprobs(xd[b:b + 1], top_n[b], True, st["temperature"], st["top_k"], st["top_p"], st["seed"], [st["stream"]], [steps[b]])
            o = [v.cpu() for v in o]
            assert int(o[0][0]) == t, what
            assert torch.equal(_bits(o[1]), _bits(lp[b:b + 1])), what
            assert torch.equal(o[2], ti[b:b + 1]) and torch.equal(_bits(o[3]), _bits(tv[b:b + 1])), what
    _cache[key] = (sampled, escaped)
    return _cache[key]


@pytest.mark.parametrize("rep", REPS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n", WIDTHS)
def test_select_rows_matches_the_restatement(eng, n, B, rep):
    run_case(eng, n, B, rep)


def test_token_escape_budget(eng):
    """over every case: at least 200 sampled rows, and the near-tie allowance (Gumbel margin < 1e-3, tests/test_gpu_ops.py) covers at most 2 % of them"""
    stats = [run_case(eng, n, B, rep) for n in WIDTHS for B in BATCHES for rep in REPS]
    sampled, escaped = sum(s for s, _ in stats), sum(e for _, e in stats)
    assert sampled >= 200
    assert escaped <= 0.02 * sampled, (escaped, sampled)


def test_rows_do_not_depend_on_their_launch(eng):
    """a row's outputs are a function of its own setting, step and logits: shuffled, or alone, it gives the same bits"""
    n, B = 1000, 16
    x = _rows(torch.Generator().manual_seed(5), B, n)
    rows = [None if st is None else place(x[b].numpy(), st) for b, st in enumerate(settings(n, B, 1))]
    steps = list(range(3, 3 + B))
    xd = x.to(DEV).contiguous()
    a = eng.op_select_rows(xd, rows, 8, steps, kept=True)
    perm = [int(i) for i in np.random.default_rng(1).permutation(B)]
    p = eng.op_select_rows(xd[perm].contiguous(), [rows[i] for i in perm], 8, [steps[i] for i in perm], kept=True)
    for j, i in enumerate(perm):
        one = eng.op_select_rows(xd[i:i + 1], [rows[i]], 8, [steps[i]], kept=True)
        for k in range(5):
            assert _same(a[k][i:i + 1], p[k][j:j + 1]) and _same(a[k][i:i + 1], one[k]), (i, k)
    # another stream or step changes the draws of the sampled rows
    moved = [None if st is None else dict(st, stream=st["stream"] + 1) for st in rows]
    assert not torch.equal(eng.op_select_rows(xd, moved, -1, steps)[0], a[0])
    assert not torch.equal(eng.op_select_rows(xd, rows, -1, [s + 1 for s in steps])[0], a[0])


@pytest.mark.parametrize("bad,msg", [(dict(temperature=0.0), "temperature"), (dict(temperature=float("nan")), "temperature"), (dict(top_k=-1), "top_k"),
                                     (dict(top_p=1.5), "top_p"), (dict(top_p=-0.1), "top_p"), (dict(min_p=1.5), "min_p"), (dict(min_p=-0.1), "min_p"),
                                     (dict(typical_p=-0.5), "typical_p"), (dict(typical_p=1.5), "typical_p"), (dict(epsilon_cutoff=1.0), "epsilon_cutoff"),
                                     (dict(epsilon_cutoff=-1e-3), "epsilon_cutoff"), (dict(eta_cutoff=1.0), "eta_cutoff"), (dict(eta_cutoff=float("nan")), "eta_cutoff")])
def test_bad_arguments(eng, bad, msg):
    x = torch.zeros((2, 64), device=DEV)
    good = dict(do_sample=True, temperature=1.0, top_k=0)
    with pytest.raises(L.GvlError, match=msg):
        eng.op_select_rows(x, [good, dict(good, **bad)], 0, [0, 0])
    with pytest.raises(L.GvlError, match=msg):
        eng.set_sampling(True, **{"min_p": 0.1, **bad})
    toks = eng.op_select_rows(x, [dict(do_sample=False, **bad), None], 0, [0, 0])[0]     # greedy: every other field is ignored
    assert toks.tolist() == [0, 0]
    eng.set_sampling(False)


def test_bad_calls(eng):
    x = torch.zeros((17, 64), device=DEV)
    with pytest.raises(L.GvlError, match="gvl_op_select_rows"):
        eng.op_select_rows(x, [None] * 17, 0)                                                # more than 16 rows
    with pytest.raises(L.GvlError, match="top_n"):
        eng.op_select_rows(x[:1], [None], 9)
    with pytest.raises(L.GvlError, match="gvl_seq_set_sampling"):
        eng.seq_set_sampling(12345, do_sample=False)                                         # unknown sequence
    with pytest.raises(L.GvlError, match="gvl_seq_set_sampling"):
        eng.seq_set_sampling(12345, None)
