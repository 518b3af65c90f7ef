"""Decoding grammars: HF generate()'s `prefix_allowed_tokens_fn` as a device-resident object.  A Python callback cannot run inside a decode call that
advances several tokens without a host round trip, so the constraint is a small automaton the processor launch evaluates itself (csrc/gvl_grammar.h,
csrc/gvl_logits.hip): a DFA over token CLASSES with one integer register.

  * every id has one class; a class is plain, or ORDINAL -- exactly the contiguous ids base .. base + size - 1, ordinal(t) = t - base;
  * trans[state][class] is FORBIDDEN (0xFFFF) or: bits 0-7 the next state, bit 8 SET (reg = ordinal), bit 9 GE (allowed iff ordinal >= reg; on an
    edge with both flags GE reads the register before SET overwrites it);
  * the walk starts at (start, reg 0) and reads the generated ids in order; it turns OFF for good on an id outside [0, vocab), a forbidden
    transition, a failed GE or a history longer than 8192 ids; a state whose whole row is forbidden is an END state;
  * OFF or END: the logits row is left untouched.  Otherwise allowed ids keep their score (+ 0.0) and every other id gets -inf: HF's
    PrefixConstrainedLogitsProcessor, in HF's place (after the min-length ban, before forced eos).

No state is kept per sequence: the mask is a pure function of the grammar and the generated ids, recomputed at every step.  `Grammar.allowed` is the
host mirror of the device walk; `Grammar.as_prefix_allowed_tokens_fn` hands the same language to HF.  `grounding_grammar` builds the two grammars of
the temporal-grounding answers ("From <s> to <e>." with s <= e)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

MAX_STATES, MAX_CLASSES, MAX_TRANS, MAX_VOCAB, HIST_CAP = 256, 64, 4096, 1 << 23, 8192      # csrc/gvl_grammar.h
FORBIDDEN, NEXT_MASK, SET, GE = 0xFFFF, 0xFF, 0x100, 0x200


def check(n_states: int, n_classes: int, start: int, vocab: int, token_class, class_base, trans) -> str:
    """gvl_grammar::check (csrc/gvl_grammar.h) restated: "" for a valid description, otherwise the library's message."""
    if not 1 <= n_states <= MAX_STATES:
        return f"n_states is {n_states}, must be 1 .. {MAX_STATES}"
    if not 1 <= n_classes <= MAX_CLASSES:
        return f"n_classes is {n_classes}, must be 1 .. {MAX_CLASSES}"
    if n_states * n_classes > MAX_TRANS:
        return f"n_states * n_classes is {n_states * n_classes}, the limit is {MAX_TRANS}"
    if not 1 <= vocab <= MAX_VOCAB:
        return f"vocab is {vocab}, must be 1 .. {MAX_VOCAB}"
    if not 0 <= start < n_states:
        return f"start state {start} out of range"
    tc = np.asarray(token_class).reshape(-1).astype(np.int64)
    cb = np.asarray(class_base).reshape(-1).astype(np.int64)
    tr = np.asarray(trans).reshape(-1).astype(np.int64)
    if len(tc) != vocab or len(cb) != n_classes or len(tr) != n_states * n_classes:
        return "null array"
    bad = np.nonzero(tc >= n_classes)[0]
    if len(bad):
        return f"token {bad[0]} has class {tc[bad[0]]}, n_classes is {n_classes}"
    size = np.bincount(tc, minlength=n_classes)
    for c in range(n_classes):
        b = int(cb[c])
        if b < -1 or b > vocab or (b >= 0 and size[c] > vocab - b):
            return f"class {c}: base {b} out of range"
        if b >= 0 and (tc[b:b + size[c]] != c).any():
            return f"ordinal class {c} is not the contiguous id range {b} .. {b + size[c] - 1}"
    max_set = 0
    for s in range(n_states):
        for c in range(n_classes):
            e = int(tr[s * n_classes + c])
            if e == FORBIDDEN:
                continue
            at = f"edge (state {s}, class {c})"
            if e & ~(NEXT_MASK | SET | GE):
                return f"{at}: reserved bits set"
            if (e & NEXT_MASK) >= n_states:
                return f"{at}: next state {e & NEXT_MASK} out of range"
            if e & (SET | GE) and cb[c] < 0:
                return f"{at}: SET / GE on a class that is not ordinal"
            if e & SET:
                max_set = max(max_set, int(size[c]))
    for s in range(n_states):
        row = tr[s * n_classes:(s + 1) * n_classes]
        if (row == FORBIDDEN).all():
            continue
        if not any(int(e) != FORBIDDEN and size[c] > 0 and (not int(e) & GE or size[c] >= max_set) for c, e in enumerate(row)):
            return (f"state {s} can forbid every token: it needs an edge without GE on a non-empty class, or a GE edge on a class at least as large as every "
                    "class with a SET edge")
    return ""


@dataclass(frozen=True, eq=False)
class Grammar:
    """A checked grammar as the device takes it (Engine.grammar_create): gvl_grammar_desc's fields."""
    n_states: int
    n_classes: int
    start: int
    vocab: int
    token_class: np.ndarray          # [vocab] uint8
    class_base: np.ndarray           # [n_classes] int32, -1 plain
    trans: np.ndarray                # [n_states, n_classes] uint16

    def __post_init__(self):
        msg = check(self.n_states, self.n_classes, self.start, self.vocab, self.token_class, self.class_base, self.trans)
        if msg:
            raise ValueError(f"grammar: {msg}")
        for name, dt, shape in (("token_class", np.uint8, (self.vocab,)), ("class_base", np.int32, (self.n_classes,)), ("trans", np.uint16, (self.n_states, self.n_classes))):
            a = np.array(getattr(self, name), dtype=dt).reshape(shape)
            a.setflags(write=False)
            object.__setattr__(self, name, a)

    def _ordinal(self, t: int, c: int) -> int:
        return t - int(self.class_base[c]) if self.class_base[c] >= 0 else 0

    def walk(self, history: Sequence[int]):
        """(on, state, reg) after the generated ids `history`."""
        state, reg = self.start, 0
        if len(history) > HIST_CAP:
            return False, state, reg
        for t in history:
            t = int(t)
            if not 0 <= t < self.vocab:
                return False, state, reg
            c = int(self.token_class[t])
            e, o = int(self.trans[state, c]), self._ordinal(t, c)
            if e == FORBIDDEN or (e & GE and o < reg):
                return False, state, reg
            if e & SET:
                reg = o
            state = e & NEXT_MASK
        return True, state, reg

    def is_end(self, state: int) -> bool:
        return bool((self.trans[state] == FORBIDDEN).all())

    def allowed(self, history: Sequence[int]) -> Optional[np.ndarray]:
        """The mask of the step after `history`: a bool array [vocab], True = the id keeps its score; None = nothing is masked (the walk is OFF or in
        an END state)."""
        on, state, reg = self.walk(history)
        if not on or self.is_end(state):
            return None
        e = self.trans[state].astype(np.int64)[self.token_class]                 # every id's edge
        base = self.class_base.astype(np.int64)[self.token_class]
        ordinal = np.where(base >= 0, np.arange(self.vocab, dtype=np.int64) - base, 0)
        return (e != FORBIDDEN) & (((e & GE) == 0) | (ordinal >= reg))

    def accepts(self, ids: Sequence[int]) -> bool:
        """`ids` is a whole sentence of the language: every id was allowed where it stands and the walk ends in an END state."""
        on, state, _ = self.walk(ids)
        return on and self.is_end(state)

    def as_prefix_allowed_tokens_fn(self):
        """The same language as HF's generate(prefix_allowed_tokens_fn=...) takes it: fn(batch_id, input_ids) -> the allowed ids (every id where the
        device leaves the row alone).  input_ids are the GENERATED ids: the reference passes inputs_embeds, so HF's input_ids start empty."""
        every = list(range(self.vocab))

        def fn(batch_id, input_ids):
            m = self.allowed([int(t) for t in input_ids])
            return every if m is None else np.nonzero(m)[0].tolist()
        return fn


class GrammarBuilder:
    """Classes, states and edges by name -> a Grammar.  Class 0 is "every id not classified otherwise" (plain)."""

    def __init__(self, vocab: int):
        self.vocab = int(vocab)
        if not 1 <= self.vocab <= MAX_VOCAB:
            raise ValueError(f"grammar: vocab is {self.vocab}, must be 1 .. {MAX_VOCAB}")
        self._class = np.zeros(self.vocab, dtype=np.int64)
        self._base: List[int] = [-1]
        self._edges: List[tuple] = []
        self._states = 0

    def token_class(self, ids: Sequence[int], ordinal: bool = False) -> int:
        """A new class holding `ids` (each may be classified once); ordinal: the ids must be one contiguous range, ordinal(t) = t - min(ids)."""
        ids = [int(t) for t in ids]
        c = len(self._base)
        for t in ids:
            if not 0 <= t < self.vocab:
                raise ValueError(f"grammar: token {t} outside [0, {self.vocab})")
            if self._class[t] != 0:
                raise ValueError(f"grammar: token {t} already has class {self._class[t]}")
        if len(set(ids)) != len(ids):
            raise ValueError("grammar: a token is listed twice")
        self._class[ids] = c
        self._base.append((min(ids) if ids else 0) if ordinal else -1)
        return c

    def state(self) -> int:
        self._states += 1
        return self._states - 1

    def edge(self, s: int, cls: int, s2: int, set_reg: bool = False, ge_reg: bool = False) -> None:
        self._edges.append((int(s), int(cls), int(s2), bool(set_reg), bool(ge_reg)))

    def build(self, start: int) -> Grammar:
        ns, nc = self._states, len(self._base)
        trans = np.full((ns, nc), FORBIDDEN, dtype=np.int64)
        for s, c, s2, st, ge in self._edges:
            if not (0 <= s < ns and 0 <= c < nc):
                raise ValueError(f"grammar: edge (state {s}, class {c}) names no such state or class")
            if not 0 <= s2 <= NEXT_MASK:
                raise ValueError(f"grammar: edge (state {s}, class {c}): next state {s2} out of range")
            trans[s, c] = s2 | (SET if st else 0) | (GE if ge else 0)
        return Grammar(ns, nc, int(start), self.vocab, self._class, np.asarray(self._base), trans)


def _token_ids(tokenizer, text: str) -> List[int]:
    enc = tokenizer(text)
    ids = list(enc.input_ids if hasattr(enc, "input_ids") else enc)
    bos = getattr(tokenizer, "bos_token_id", None)
    return [int(t) for t in (ids[1:] if ids and bos is not None and ids[0] == bos else ids)]


def grounding_grammar(tokenizer, num_temporal_tokens: int, eos_id: int, mode: str = "interval", vocab: Optional[int] = None) -> Grammar:
    """The grammar of the grounding answers over `tokenizer`'s vocabulary (the temporal tokens <0> .. <N> are one ordinal class).
    vocab: how many ids the grammar classifies -- the MODEL's vocabulary (model.geo.vocab: the rows of its embedding and head), which a grammar bound to its
    sequences must match.  It may exceed len(tokenizer): Phi-3.5 has 32 064 embedding rows for about 32 011 tokenizer entries, and both grow by the same added
    tokens.  The rows past the tokenizer name no token; they fall into class 0 like every other id -- forbidden in "interval", an other-token in "ordered".
    None: len(tokenizer).  A vocab below len(tokenizer), or below any id the grammar names, raises ValueError.
    mode "interval": exactly the tokenisation of "From <s> to <e>." followed by eos, with s <= e -- the literal ids come from tokenizer("From <0> to <0>."),
    each in a class of its own, the first timestamp is a SET edge, the second a GE edge; every other id, <timestamp_grounding> included, is forbidden.
    mode "ordered": free text with timestamps in pairs -- state A: another token stays in A, a timestamp (SET) goes to B; state B: another token stays in
    B, a timestamp (GE) goes back to A; eos only in A."""
    if mode not in ("interval", "ordered"):
        raise ValueError(f"grounding_grammar: mode must be 'interval' or 'ordered', not {mode!r}")
    n = int(num_temporal_tokens)
    stamps = []
    for k in range(n + 1):
        ids = _token_ids(tokenizer, f"<{k}>")
        if len(ids) != 1:
            raise ValueError(f"grounding_grammar: <{k}> is not one token of this tokenizer")
        stamps.append(ids[0])
    if stamps != list(range(stamps[0], stamps[0] + n + 1)):
        raise ValueError("grounding_grammar: the temporal tokens are not one contiguous id range")
    eos_id = int(eos_id)
    vocab = len(tokenizer) if vocab is None else int(vocab)
    if vocab < len(tokenizer):
        raise ValueError(f"grounding_grammar: vocab is {vocab}, the tokenizer holds {len(tokenizer)} ids")
    b = GrammarBuilder(vocab)
    ts = b.token_class(stamps, ordinal=True)
    eos = b.token_class([eos_id])
    if mode == "ordered":
        A, B_, end = b.state(), b.state(), b.state()
        b.edge(A, 0, A); b.edge(A, ts, B_, set_reg=True); b.edge(A, eos, end)
        b.edge(B_, 0, B_); b.edge(B_, ts, A, ge_reg=True)
        return b.build(A)
    ids = _token_ids(tokenizer, "From <0> to <0>.")
    if [t for t in ids if t in stamps] != [stamps[0]] * 2:
        raise ValueError("grounding_grammar: 'From <0> to <0>.' does not tokenise to two temporal tokens")
    lit = {}
    for t in ids:
        if t not in stamps and t not in lit:
            if t == eos_id:
                raise ValueError("grounding_grammar: the eos id is part of the answer's literal text")
            lit[t] = b.token_class([t])
    s, seen = b.state(), 0
    for t in ids:
        s2 = b.state()
        if t in lit:
            b.edge(s, lit[t], s2)
        else:
            b.edge(s, ts, s2, set_reg=seen == 0, ge_reg=seen == 1)
            seen += 1
        s = s2
    b.edge(s, eos, b.state())
    return b.build(0)
