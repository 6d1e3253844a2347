"""Exact host reference of the samplers' further options (csrc/sample.hip SampleExt: ``min_p``, ``presence_penalty``,
``frequency_penalty``), on top of tests/sampler_ref.py, which it imports unchanged.  A plain helper module.

Penalty stage: active when ``repeat_last_n > 0``, at least one token has been generated and ``repeat_penalty != 1`` or
``presence_penalty != 0`` or ``frequency_penalty != 0``.  The window is the repeat penalty's (``sampler_ref.recent_ids``:
the last ``min(repeat_last_n, 64, n_gen)`` ids of the ring; ids outside ``[0, V)`` ignored).  For each distinct id of
the window, ``c`` its number of occurrences there, in float32: first, only if ``repeat_penalty != 1``,
``v = v / rp if v > 0 else v * rp``; then, only if one of the two further penalties is non-zero,
``v = v - fmaf(float(c), frequency_penalty, presence_penalty)``.

``min_p`` (0: off): after top-k, candidate ``i`` (value descending, index ascending) is kept when
``exp((v_i - v_0) / T) >= min_p``, candidate 0 always; the kept set is a prefix, and the final cut is the shorter of
it and the top-p prefix.  Greedy ignores ``min_p``.

What the kernels' fp32 arithmetic may move: the 2-ulp rule of ``sampler_ref.reference_detail`` for adjacent candidates
of which one is penalised stays (the division; the fused multiply-add and the subtraction are exact operations rounded
once, the same on both sides), and a ``min_p`` comparison whose ratio lies within ``DELTA * min_p`` of ``min_p`` admits
both outcomes (the device's ``__expf`` ratio is good to a few 1e-6 relative).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Sequence, Tuple

import numpy as np

import sampler_ref as sr

EXT_KEYS = ("min_p", "presence_penalty", "frequency_penalty")
EXT = [(0.05, 0.0, 0.0), (0.2, 0.0, 0.0), (0.0, 0.5, 0.0), (0.0, 0.0, 0.3), (0.1, 0.6, 0.4), (0.02, 1.5, 0.0),
       (0.5, 0.0, 1.0)]  # (min_p, presence, frequency); 7 is coprime to the 9 KINDS, so the pairs mix


def _f32(o: Dict, k: str) -> np.float32:
    return np.float32(o.get(k, 0.0))


def fmaf32(a: np.float32, b: np.float32, c: np.float32) -> np.float32:
    """fmaf on float32 values: the exact a * b + c rounded once.  The product of two float32 is exact in float64, and
    so is its sum with a float32 of a comparable exponent (counts up to 64, penalties of a few units: far inside
    float64's 53 bits)."""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def penalise_ext(logits_f32: np.ndarray, hist_ring, n_gen: int, opts: Dict) -> Tuple[np.ndarray, List[int], Dict[int, int]]:
    """(the row after the penalty stage, the penalised ids in window order, {id: its count in the window})."""
    v = np.array(logits_f32, dtype=np.float32, copy=True)
    rp = np.float32(opts["repeat_penalty"])
    pp, fp = _f32(opts, "presence_penalty"), _f32(opts, "frequency_penalty")
    ext = pp != np.float32(0.0) or fp != np.float32(0.0)
    pen: List[int] = []
    counts: Dict[int, int] = {}
    if (rp != np.float32(1.0) or ext) and opts["repeat_last_n"] > 0:
        window = sr.recent_ids(hist_ring, n_gen, opts["repeat_last_n"])
        for t in window:
            if 0 <= t < v.shape[0]:
                counts[t] = counts.get(t, 0) + 1
                if t not in pen:
                    pen.append(t)
        for t in pen:
            x = v[t]
            if rp != np.float32(1.0):
                x = np.float32(x / rp) if x > 0 else np.float32(x * rp)
            if ext:
                x = np.float32(x - fmaf32(np.float32(counts[t]), fp, pp))
            v[t] = x
    return v, pen, counts


def draw_ext(ids: List[int], vals: Sequence[float], opts: Dict, u: float, delta: float) -> sr.Draw:
    """``sampler_ref.draw`` with the ``min_p`` prefix: the nominal cut is the shorter of the two prefixes, the picks
    those of every admitted (top-p cut, min_p prefix) pair."""
    inv_t = float(np.float32(1.0) / np.float32(opts["temperature"]))
    v0 = float(vals[0])
    e = [math.exp((float(x) - v0) * inv_t) for x in vals]
    z = math.fsum(e)
    probs = [x / z for x in e]
    cdf, acc = [], 0.0
    for p in probs:
        acc += p
        cdf.append(acc)
    n = len(ids)
    tp = float(np.float32(opts["top_p"]))
    cut, cuts = n, {n}
    if 0.0 < tp < 1.0:
        cut = next((i + 1 for i in range(n) if cdf[i] >= tp), n)
        cuts = {cut} | {i + 1 for i in range(n) if abs(cdf[i] - tp) <= delta}
    mp = float(_f32(opts, "min_p"))
    keep, keeps = n, {n}
    if mp > 0.0:
        keep = next((i for i in range(1, n) if e[i] < mp), n)  # `>=` keeps; candidate 0 always
        lo = next((i for i in range(1, n) if e[i] < mp + delta * mp), n)   # the first that may be dropped
        hi = next((i for i in range(1, n) if e[i] < mp - delta * mp), n)   # the first that must be dropped
        keeps = set(range(lo, hi + 1))
    cut = min(cut, keep)
    cuts = {min(c, k) for c in cuts for k in keeps}

    def pick(c: int, uu: float) -> int:
        zc = cdf[c - 1]
        return ids[next((i for i in range(c) if uu * zc < cdf[i]), c - 1)]

    d = sr.Draw(ids=list(ids), probs=probs, cut=cut, token=pick(cut, u))
    for c in cuts:
        for uu in (u - delta, u, u + delta):
            d.picks.add(pick(c, uu))
    return d


def reference_detail_ext(logits_f32, hist_ring, n_gen: int, opts: Dict, delta: float = sr.DELTA) -> sr.RowRef:
    """``sampler_ref.reference_detail`` under the further options (absent keys are neutral)."""
    v, pen, _ = penalise_ext(logits_f32, hist_ring, n_gen, opts)
    raw = np.asarray(logits_f32, dtype=np.float32)
    V = v.shape[0]
    greedy = opts["temperature"] <= 0
    K = 1 if greedy else sr.top_k_of(opts, V)
    ext = sr.ordered(v, min(K + 1, V))
    orders = [ext[:K]]
    for i in range(min(K, len(ext) - 1)):
        a, b = ext[i], ext[i + 1]
        if abs(sr._ord(v[a]) - sr._ord(v[b])) <= 2 and (a in pen or b in pen):
            if a in pen and b in pen and sr._ord(raw[a]) == sr._ord(raw[b]):
                continue
            sw = list(ext)
            sw[i], sw[i + 1] = b, a
            orders.append(sw[:K])
    support = set().union(*[set(o) for o in orders])
    firsts = {o[0] for o in orders}
    if greedy:
        return sr.RowRef(set(firsts), ext[0], ext[:1], [1.0], 1, pen, v, support, firsts)
    u = sr.u_of(int(opts["seed"]), int(n_gen))
    draws = [draw_ext(o, [v[i] for i in o], opts, u, delta) for o in orders]
    adm = set().union(*[d.picks for d in draws])
    d0 = draws[0]
    return sr.RowRef(adm, d0.token, d0.ids, d0.probs, d0.cut, pen, v, support, firsts)


@dataclass
class CaseExt(sr.Case):
    exts: List[int] = field(default_factory=list)  # index into EXT per row


def exact_case_ext(V: int, launch: int) -> CaseExt:
    """``sampler_ref.exact_case(V, launch)`` whose row g = launch * 64 + i also has ``EXT[g % 7]``, and whose ring
    holds the row's top id at ages 1 and 2 and its second id at age 4 as well (exact_case put them at ages 0 and 3):
    counts of 3 and 2 occur wherever the window is long enough."""
    c = sr.exact_case(V, launch)
    M = len(c.rows)
    top = np.argsort(-c.logits, axis=1, kind="stable")[:, :2]
    rows, exts = [], []
    for i in range(M):
        g = launch * M + i
        x = g % len(EXT)
        exts.append(x)
        rows.append(dict(c.rows[i], **dict(zip(EXT_KEYS, EXT[x]))))
        ng = int(c.state["n_gen"][i])
        for age, t in ((1, top[i, 0]), (2, top[i, 0]), (4, top[i, 1])):
            c.state["hist"][i, (ng - 1 - age) & (sr.HIST - 1)] = t
    return CaseExt(c.logits, rows, c.kinds, c.state, c.T_max, exts)


def case_refs_ext(case: sr.Case, delta: float = sr.DELTA) -> List[sr.RowRef]:
    return [reference_detail_ext(case.logits[m], case.state["hist"][m], int(case.state["n_gen"][m]), case.rows[m],
                                 delta) for m in range(len(case.rows))]
