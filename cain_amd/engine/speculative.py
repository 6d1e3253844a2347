"""Speculative decoding, self-drafting form: the rule on the host.

Each decode step proposes up to ``K`` tokens per sequence, verifies them in one forward over ``K + 1`` rows per
sequence and keeps the longest correct prefix.  Nothing is approximated: the sampler's random stream is keyed by
``(seed, generated index)`` and its repeat penalty reads the row's history ring, so the row of draft ``j`` draws
exactly the token plain decoding draws at generated index ``n_gen + j`` when drafts ``1 .. j`` are the tokens plain
decoding emitted -- and a draft is accepted only when it *is* that token.  This module states the rule in plain
Python; ``csrc/spec.hip`` implements it on the device, ``ops.spec_draft_ref`` / ``ops.spec_accept_ref`` wrap it for
arrays, and the torch backend decodes with it.

A sequence is a decode row with slot ``s``, input token ``tok`` at position ``pos``, ``ng`` generated tokens and a
record ``seq[0 .. pos]`` (prompt, then generated tokens, by position; ``seq[pos] == tok``).

Draft (n-gram mode)
    For n = 3, 2, 1 (skipping n > pos): the largest ``i`` in ``[n - 1, pos - 1]`` with
    ``seq[i - n + 1 .. i] == seq[pos - n + 1 .. pos]``.  At the first n with a match the drafts are
    ``seq[i + 1 .. min(i + K, pos)]`` (1 .. K tokens).  No match: none.
Draft (given mode)
    ``given[ng .. ng + K - 1]``, ended by a negative id (or one outside the vocabulary).
Clip
    ``d`` drafts at most with ``pos + d <= T_max - 1`` and ``ng + d <= max_new - 1``; a done or masked (slot < 0)
    sequence drafts nothing.
Expand
    Row 0 is the sequence's own row, exactly as plain decode runs it.  Row ``1 <= j <= d``: ``tok = draft[j]``,
    ``pos + j``, the same slot, ``n_gen = ng + j``, not done, no budget of its own; its history ring is the
    sequence's with ``draft[1 .. j]`` at indices ``(ng .. ng + j - 1) & 63``.  Rows ``j > d`` are masked
    (``slot = -1``, ``tok = 0``).
Accept
    ``t_j``: the token sampled for row ``j``.  ``a``: the largest value in ``[0, d]`` with ``t_{j-1} == draft[j]``
    for all ``1 <= j <= a``.  ``t_0 .. t_a`` are committed in order, each as the sampler commits one token
    (generated ids, ring, ``n_gen``, ``tok``, ``pos``, ``done``), stopping at the first that ends the sequence (a
    stop id, ``max_new``, ``T_max``); each is also appended to the record.

K / V of rejected rows stay in the cache at positions above the sequence's: attention masks by position, so nothing
reads them, and later tokens overwrite them.

Draft model (a third source of drafts; verify and accept are given mode's, unchanged)
    A speculative engine may own a second, smaller model: its own weights, plan and KV cache, with the target's
    number of cache slots and ``T_max``; a sequence uses the same slot in both caches.  ``dvalid[slot]`` counts the
    leading positions of the slot's draft cache whose K / V belong to the record ``seq``; after a request's prefill
    (the draft model runs ``prompt[:-1]``, no logits, no sampler) it is ``len(prompt) - 1``.
    One step, with ``d = clip(K, pos, ng, K, T_max, max_new)`` (0 for a done or masked sequence, and on a sequence's
    last token: such a sequence runs no draft row and its ``dvalid`` stays):
    First draft forward, two rows: the catch-up row ``seq[pos - 1]`` at ``pos - 1``, masked unless
    ``dvalid == pos - 1`` (the step before accepted every draft), which only writes K / V; and the sequence's own row
    ``seq[pos]`` at ``pos``, on which the ordinary sampler runs with ``n_gen = ng``, the sequence's ring and the
    request's own options -- stop ids off, no budget.  It draws ``d_1``.
    Draft forwards ``j = 2 .. K``, one row: ``d_{j-1}`` at ``pos + j - 1`` with ``n_gen = ng + j - 1``, the ring
    carrying ``d_1 .. d_{j-1}`` as ``draft_ring`` writes them; masked when ``j > d``.  It draws ``d_j``.
    The sampler's random stream is keyed by (seed, generated index), so the draft row that draws ``d_j`` uses the
    uniform number of the target row that decides whether ``d_j`` is accepted: equal distributions give equal
    tokens.  No rejection-sampling arithmetic: a draft is still kept only when it is the token.
    ``given[ng + j - 1] = d_j`` for ``j <= d``, ``given[ng + d] = -1`` when ``d < K``; then given mode.
    After accept, with ``pos'`` the sequence's new position: ``dvalid = min(pos + d, pos')`` -- for a sequence that
    goes on, ``min(pos + d, pos + a + 1)``: the next step needs one row when ``a < d`` and two when ``a == d``.
    A token id at or above the draft model's vocabulary enters the draft forward as the draft model's ``bos_id``; a
    draft id at or above the target's ends the draft (given mode's ``vocab`` rule).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence

K_MAX = 7       # drafts per step (csrc/spec.h SPEC_K_MAX)
HIST = 64       # the samplers' history ring (csrc/sample.hip HIST)
NO_BUDGET = 0x7FFFFFFF  # max_new of a draft row


def ngram_draft(seq: Sequence[int], pos: int, K: int) -> List[int]:
    """Drafts of the n-gram rule for a record ``seq[0 .. pos]``, before clipping."""
    for n in (3, 2, 1):
        if n > pos:
            continue
        suffix = list(seq[pos - n + 1: pos + 1])
        for i in range(pos - 1, n - 2, -1):  # the most recent match wins
            if list(seq[i - n + 1: i + 1]) == suffix:
                return [int(t) for t in seq[i + 1: min(i + K, pos) + 1]]
    return []


def given_draft(given: Sequence[int], ng: int, K: int, vocab: Optional[int] = None) -> List[int]:
    """Drafts of given mode: ``given[ng .. ng + K - 1]`` up to the first negative (or out-of-vocabulary) id or the
    end of the buffer."""
    out: List[int] = []
    for t in list(given[ng: ng + K]):
        t = int(t)
        if t < 0 or (vocab is not None and t >= vocab):
            break
        out.append(t)
    return out


def clip(n_drafts: int, pos: int, ng: int, K: int, T_max: int, max_new: int) -> int:
    return max(0, min(n_drafts, K, T_max - 1 - pos, max_new - 1 - ng))


def draft(seq: Sequence[int], pos: int, ng: int, K: int, T_max: int, max_new: int, done: bool = False,
          slot: int = 0, given: Optional[Sequence[int]] = None, vocab: Optional[int] = None) -> List[int]:
    """The drafts of one sequence for one step (n-gram mode; given mode when ``given`` is not None)."""
    if done or slot < 0:
        return []
    cap = clip(K, pos, ng, K, T_max, max_new)
    if cap <= 0:
        return []
    d = given_draft(given, ng, K, vocab) if given is not None else ngram_draft(seq, pos, K)
    return d[:cap]


def draft_ring(hist: Sequence[int], ng: int, drafts: Sequence[int], j: int) -> List[int]:
    """History ring of expanded row ``j``: drafts ``1 .. j`` written at indices ``(ng .. ng + j - 1) & 63``."""
    ring = [int(t) for t in hist]
    for jj in range(1, j + 1):
        ring[(ng + jj - 1) & (HIST - 1)] = int(drafts[jj - 1])
    return ring


def accepted_length(drafts: Sequence[int], sampled: Sequence[int]) -> int:
    """``a``: how many leading drafts equal the token sampled by the row before them."""
    a = 0
    while a < len(drafts) and int(sampled[a]) == int(drafts[a]):
        a += 1
    return a


@dataclass
class SeqState:
    """Decode state of one sequence on the host (the device keeps the same fields per row)."""
    tok: int
    pos: int
    max_new: int
    eos_id: int = -1
    stop: Sequence[int] = ()
    slot: int = 0
    n_gen: int = 0
    done: bool = False
    gen: List[int] = field(default_factory=list)
    hist: List[int] = field(default_factory=lambda: [0] * HIST)
    seq: List[int] = field(default_factory=list)  # record by position, seq[pos] == tok
    drafted: int = 0
    accepted: int = 0
    step_tokens: List[int] = field(default_factory=list)

    def commit_token(self, choice: int, T_max: int) -> None:
        """csrc/sample.hip advance_row for one token, plus the record."""
        choice = int(choice)
        self.gen.append(choice)
        self.hist[self.n_gen & (HIST - 1)] = choice
        self.n_gen += 1
        self.tok = choice
        p1 = self.pos + 1
        if p1 < T_max:
            del self.seq[p1:]
            self.seq.append(choice)
        stop = (self.eos_id >= 0 and choice == self.eos_id) or any(s >= 0 and choice == s for s in self.stop)
        if stop or self.n_gen >= self.max_new or p1 >= T_max:
            self.done = True
        else:
            self.pos = p1

    def commit_step(self, drafts: Sequence[int], sampled: Sequence[int], T_max: int) -> int:
        """Accept: ``sampled[j]`` is the token drawn for row ``j`` (``len(drafts) + 1`` of them).  Returns the
        number of tokens committed (0 for a sequence that is done or masked)."""
        if self.done or self.slot < 0:
            return 0
        a = accepted_length(drafts, sampled)
        c = 0
        for j in range(a + 1):
            self.commit_token(sampled[j], T_max)
            c += 1
            if self.done:
                break
        self.drafted += len(drafts)
        self.accepted += c - 1
        self.step_tokens.append(c)
        return c


# ---------------------------------------------------------------------------------------------- draft model
MASKED_ROW = (0, 0, -1, 0, 0, 0)  # (tok, pos, slot, n_gen, max_new, done) of a row no forward acts on


def draft_token(t: int, dvocab: int, dbos: int) -> int:
    """A token id as the draft model's embedding takes it."""
    t = int(t)
    return t if 0 <= t < dvocab else int(dbos)


def draft_model_rows(seq: Sequence[int], pos: int, ng: int, K: int, T_max: int, max_new: int, dvalid: int,
                     dvocab: int, dbos: int, done: bool = False, slot: int = 0):
    """First draft forward of one sequence: ``(d, catch_up, own)``, the rows as ``(tok, pos, slot, n_gen, max_new,
    done)``.  The catch-up row is marked done: its K / V are written, the sampler skips it."""
    d = 0 if done or slot < 0 else clip(K, pos, ng, K, T_max, max_new)
    if d <= 0:
        return 0, MASKED_ROW, MASKED_ROW
    own = (draft_token(seq[pos], dvocab, dbos), pos, slot, ng, NO_BUDGET, 0)
    if pos >= 1 and dvalid == pos - 1:
        return d, (draft_token(seq[pos - 1], dvocab, dbos), pos - 1, slot, ng, NO_BUDGET, 1), own
    return d, MASKED_ROW, own


def draft_model_next(d_j: int, j: int, pos: int, ng: int, d: int, slot: int, dvocab: int, dbos: int):
    """The row of draft forward ``j + 1`` from ``d_j``, the token forward ``j`` drew (``1 <= j <= d``)."""
    if j + 1 > d:
        return MASKED_ROW
    return (draft_token(d_j, dvocab, dbos), pos + j, slot, ng + j, NO_BUDGET, 0)


def draft_model_given(given, ng: int, drafts: Sequence[int], K: int) -> None:
    """``d_1 .. d_d`` into the sequence's given buffer, ended when ``d < K``."""
    d = len(drafts)
    for j in range(1, d + 1):
        given[ng + j - 1] = int(drafts[j - 1])
    if d < K and ng + d < len(given):
        given[ng + d] = -1


def dvalid_after(pos: int, d: int, pos_after: int) -> int:
    """``dvalid`` of a sequence that ran ``d >= 1`` draft forwards from ``pos`` and stands at ``pos_after``."""
    return min(pos + d, pos_after)
