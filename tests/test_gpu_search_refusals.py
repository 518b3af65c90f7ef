"""-m gpu: what the three searches inside the library (gvl_beam_search_n, gvl_group_beam_search, gvl_contrastive_search) refuse, through the raw ABI: the status and
the whole message of every refusal -- written out here from the entries as they were before they shared csrc/gvl_search.hip --, and after each one the KV pool and the
caller's sequence where they were: in the end the caller's sequence decodes the greedy ids a fresh sequence decodes.  The mid-search failure of a full context
(a prompt of max_seq - 3 rows, max_new 8) comes after three steps, with every clone given back.  Its text is the first of two checks of the same condition
(position == the clones' capacity == cfg.max_seq) that the step meets: a clone the step needs is refused by gvl_seq_clone ("... max_tokens must exceed them"), and
only a step that needs none reaches the search's own "the context is full".  Contrastive search clones k - 1 sequences at every step, so it always meets the first;
a beam step meets it whenever two beams continue the same parent."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV  # noqa: E402,F401
from grounded_video_llm_amd import lib as L  # noqa: E402
from grounded_video_llm_amd.engine import _ptr  # noqa: E402
from test_gpu_contrastive import _prompt_ids, make_engine  # noqa: E402

K, G, MAX_NEW, S_PROMPT, MAX_SEQ = 4, 2, 8, 70, 256
ENTRIES = ("gvl_beam_search", "gvl_group_beam_search", "gvl_contrastive_search")
NAN = float("nan")
CLONE_FULL = "gvl_seq_clone: the source must hold tokens and max_tokens must exceed them (and fit cfg.max_seq)"


@pytest.fixture(scope="module")
def eng():
    e, geo, _ = make_engine("phi_valu", max_seq=MAX_SEQ, max_prefill=MAX_SEQ, kv_pages=48)
    assert geo.max_seq == MAX_SEQ
    yield e
    e.close()


def call(eng, fn, seq, first, cap=MAX_NEW, max_new=MAX_NEW, k=K, groups=G, lam=1.0, alpha=0.6, num_return=1, length_penalty=1.0, early=0, penalty=1.0, ngram=0, min_new=0,
         rules=-1):
    """one raw call of entry `fn` -> (status, gvl_last_error's text, ids)"""
    room = max(cap, max_new, 1) * max(num_return, 1)
    ids, n, score, ts = (C.c_int32 * room)(), (C.c_int * max(num_return, 1))(), (C.c_double * max(num_return, 1))(), (C.c_float * room)()
    base = L.GvlBeamParams(k, max_new, -1, length_penalty, early, penalty, ngram, min_new, -1, rules)
    if fn == "gvl_beam_search":
        rc = eng.lib.gvl_beam_search_n(eng.ctx, seq, _ptr(first), C.byref(base), num_return, ids, cap, n, score, ts, eng.stream)
    elif fn == "gvl_group_beam_search":
        prm = L.GvlGroupBeamParams(base, groups, lam, -1)
        rc = eng.lib.gvl_group_beam_search(eng.ctx, seq, _ptr(first), C.byref(prm), num_return, ids, cap, n, score, ts, eng.stream)
    else:
        prm = L.GvlContrastiveParams(k, alpha, max_new, -1, penalty, ngram, min_new, -1, rules)
        rc = eng.lib.gvl_contrastive_search(eng.ctx, seq, _ptr(first), C.byref(prm), ids, cap, n, None, None, None, None, None, None, eng.stream)
    msg = eng.lib.gvl_last_error(eng.ctx)
    return rc, (msg.decode() if msg and rc != 0 else ""), [int(ids[i]) for i in range(n[0])] if rc == 0 else None


def greedy(eng, seq, first, n):
    """n greedy ids of `seq` from its prefill logits, by teacher-forced steps (they fill a keep-hidden sequence's bank too), and the last row"""
    out, row = [], first
    for _ in range(n):
        out.append(int(torch.argmax(row)))
        row = eng.decode_step_logits(seq, out[-1])
    return out, row.clone()


def prefilled(eng, emb, cap, keep_hidden):
    seq = eng.seq_alloc(cap)
    if keep_hidden:
        eng.seq_keep_hidden(seq)
    return seq, eng.prefill(seq, emb, want_logits=True).clone()


# the refusals that depend on the arguments' values alone: (overrides, status, text behind "<entry>: ", the entries it is for)
BEAMS = ENTRIES[:2]
VALUE_REFUSALS = [
    (dict(cap=MAX_NEW - 1), L.ERR_ARG, "cap (room of out_ids_host) must be >= max_new_tokens", ENTRIES),
    (dict(penalty=0.0), L.ERR_ARG, "penalty must be > 0, ngram >= 0, min_new >= 0", ENTRIES),
    (dict(penalty=-1.5), L.ERR_ARG, "penalty must be > 0, ngram >= 0, min_new >= 0", ENTRIES),
    (dict(ngram=-1), L.ERR_ARG, "penalty must be > 0, ngram >= 0, min_new >= 0", ENTRIES),
    (dict(rules=999), L.ERR_ARG, "no such rule set", ENTRIES),
    (dict(rules=-2), L.ERR_ARG, "no such rule set", ENTRIES),
    (dict(length_penalty=NAN), L.ERR_ARG, "length_penalty is NaN", BEAMS),
    (dict(early=3), L.ERR_ARG, 'early_stopping must be 0 (False), 1 (True) or 2 ("never")', BEAMS),
    (dict(early=2), L.ERR_ARG, 'early_stopping "never" with length_penalty > 0 needs a maximum length: not supported', BEAMS),
    (dict(k=17), L.ERR_ARG, "num_beams must be 2 .. 16", BEAMS),
    (dict(num_return=K + 1), L.ERR_ARG, "num_return must be 1 .. num_beams", BEAMS),
    (dict(max_new=0), L.ERR_ARG, None, BEAMS),                                           # the text names the engine's limit: checked by its head below
    (dict(k=32, groups=2), L.ERR_ARG, "num_beams must be 2 .. 16", ENTRIES[1:2]),
    (dict(groups=3), L.ERR_ARG, "num_beam_groups must be 2 .. num_beams and divide num_beams", ENTRIES[1:2]),
    (dict(lam=0.0), L.ERR_ARG, "diversity_penalty must be > 0", ENTRIES[1:2]),
    (dict(k=1, num_return=0), L.ERR_ARG, "num_return must be 1 .. num_beams", ENTRIES[:1]),       # two faults: each entry names the one its order meets first
    (dict(k=1, num_return=0), L.ERR_ARG, "num_beams must be 2 .. 16", ENTRIES[1:2]),
    (dict(k=17), L.ERR_ARG, "top_k must be 2 .. 16", ENTRIES[2:]),
    (dict(alpha=1.5), L.ERR_ARG, "penalty_alpha must be in [0, 1]", ENTRIES[2:]),
    (dict(max_new=0), L.ERR_ARG, "max_new_tokens out of range", ENTRIES[2:]),
]


def test_every_refusal_keeps_its_status_and_text_and_leaves_everything_in_place(eng):
    emb = eng.embed_ids(_prompt_ids(S_PROMPT, 71))
    free0 = eng.kv_info()["free_pages"]
    fresh, fresh_first = prefilled(eng, emb, S_PROMPT + 8, False)
    want_ids, want_row = greedy(eng, fresh, fresh_first, 6)
    eng.seq_free(fresh)
    assert eng.kv_info()["free_pages"] == free0
    plain, first = prefilled(eng, emb, S_PROMPT + 8, False)
    kept, kept_first = prefilled(eng, emb, S_PROMPT + 8, True)
    empty, empty_kept = eng.seq_alloc(64), eng.seq_alloc(64)
    eng.seq_keep_hidden(empty_kept)
    assert torch.equal(first, fresh_first) and torch.equal(kept_first, fresh_first)
    held = eng.kv_info()["free_pages"]
    caller = {ENTRIES[0]: (plain, first), ENTRIES[1]: (plain, first), ENTRIES[2]: (kept, kept_first)}
    try:
        good = {fn: call(eng, fn, *caller[fn]) for fn in ENTRIES}
        for fn in ENTRIES:
            assert good[fn][0] == 0 and len(good[fn][2]) == MAX_NEW and eng.kv_info()["free_pages"] == held, (fn, good[fn])

        def refused(fn, status, text, seq, logits, **over):
            rc, msg, _ = call(eng, fn, seq, logits, **over)
            print(f"{fn} {over}: status {rc}, {msg!r}")
            assert rc == status, (fn, over, rc, msg)
            if text is not None:
                assert msg == f"{fn}: {text}", (fn, over, msg)
            assert eng.kv_info()["free_pages"] == held, (fn, over)
            return msg

        n_checked = 0
        for over, status, text, entries in VALUE_REFUSALS:
            for fn in entries:
                msg = refused(fn, status, text, *caller[fn], **over)
                if text is None:
                    assert msg.startswith(f"{fn}: max_new_tokens must be 1 .. ") and msg.rsplit(" ", 1)[1].isdigit(), msg
                n_checked += 1
        assert n_checked == 38
        for fn in ENTRIES:
            seq, logits = caller[fn]
            refused(fn, L.ERR_ARG, "bad seq", 200, logits)
            refused(fn, L.ERR_STATE, "the sequence is not prefilled", empty_kept if fn == ENTRIES[2] else empty, logits)
            refused(fn, L.ERR_ARG, "no such rule set", 200, logits, rules=999)             # two faults: the rule set comes first
            refused(fn, L.ERR_ARG, "penalty must be > 0, ngram >= 0, min_new >= 0", 200, logits, rules=999, penalty=0.0)
        for fn in BEAMS:                                                                  # a keep-hidden sequence handed to the beam entries
            refused(fn, L.ERR_STATE, f"sequence {kept} keeps its hidden states (gvl_seq_keep_hidden); this entry does not fill the bank", kept, kept_first)
        refused(ENTRIES[2], L.ERR_STATE, "the sequence keeps no hidden states (gvl_seq_keep_hidden before its prefill)", plain, first)
        # the searches still give what they gave, and the callers' sequences decode what a fresh one decodes
        for fn in ENTRIES:
            assert call(eng, fn, *caller[fn]) == good[fn], fn
        for seq, logits in (caller[ENTRIES[0]], caller[ENTRIES[2]]):
            ids, row = greedy(eng, seq, logits, 6)
            assert ids == want_ids and torch.equal(row, want_row)
    finally:
        for s in (plain, kept, empty, empty_kept):
            eng.seq_free(s)
    assert eng.kv_info()["free_pages"] == free0


def test_a_full_context_ends_the_search_with_every_clone_given_back(eng):
    S = MAX_SEQ - 3
    emb = eng.embed_ids(_prompt_ids(S, 72))
    free0 = eng.kv_info()["free_pages"]
    fresh, fresh_first = prefilled(eng, emb, MAX_SEQ, False)
    want_ids, want_row = greedy(eng, fresh, fresh_first, 2)
    eng.seq_free(fresh)
    plain, first = prefilled(eng, emb, MAX_SEQ, False)
    kept, kept_first = prefilled(eng, emb, MAX_SEQ, True)
    held = eng.kv_info()["free_pages"]
    try:
        for fn, (seq, logits) in zip(ENTRIES, ((plain, first), (plain, first), (kept, kept_first))):
            rc, msg, _ = call(eng, fn, seq, logits)
            print(f"{fn}: status {rc}, {msg!r}")
            full = f"{fn}: the context is full (cfg.max_seq) before max_new_tokens"
            assert rc == L.ERR_ARG and msg in ((CLONE_FULL,) if fn == ENTRIES[2] else (CLONE_FULL, full)), (fn, rc, msg)
            assert eng.kv_info()["free_pages"] == held, fn
            rc, _, ids = call(eng, fn, seq, logits, cap=3, max_new=3)                     # three steps fit: so the failure above came after some steps
            assert rc == 0 and len(ids) == 3 and eng.kv_info()["free_pages"] == held, fn
        for seq, logits in ((plain, first), (kept, kept_first)):
            ids, row = greedy(eng, seq, logits, 2)
            assert ids == want_ids and torch.equal(row, want_row)
    finally:
        eng.seq_free(plain)
        eng.seq_free(kept)
    assert eng.kv_info()["free_pages"] == free0
