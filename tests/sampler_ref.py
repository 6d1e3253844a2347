"""Exact host reference of the device samplers (cain_amd/ops/csrc/sample.hip), for the tests.

A plain helper module (numpy and Python ints; no GPU).  The device draw is fully determined by the logits, the
options, the history ring, the seed and the token index, so this module predicts the token itself, not only its
distribution: repeat penalty in float32 (it decides order and ties), everything after it in float64.

``DELTA`` bounds what the kernels' fp32 arithmetic may move on the normalised CDF: at most 256 ``__expf`` terms
accumulated in fp32 (relative error <= 256 * 2^-24 ~ 1.5e-5), the exponent argument rounded in fp32 (|arg| <= ~30 on
the inputs of ``exact_case``: ~2e-6 per term) and a hardware exponential good to a few ulp; 1e-4 is about three times
their sum.  A comparison (top-p cut, pick) that lies further than DELTA from its bound has one possible outcome; the
tokens of every outcome within DELTA form the *admissible set*, and a case is *decided* when that set has one token.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Sequence, Set, Tuple

import numpy as np

MASK64 = (1 << 64) - 1
HIST = 64       # history ring of the last ids (sample.hip HIST)
TOPK_MAX = 256  # top-k clamp of the kernels (sample.hip SS_KMAX); top_k <= 0 or above it means this many
DELTA = 1e-4


def mix64(z: int) -> int:
    """SplitMix64's output function on z + golden gamma (sample.hip mix64)."""
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def u_of(seed: int, ng: int) -> float:
    """The uniform in [0, 1) that decides token index ``ng`` of a request with ``seed`` (24 bits, exact)."""
    r = mix64((seed & MASK64) ^ mix64((ng * 0x632BE59BD9B4E019 + 0x9E3779B97F4A7C15) & MASK64))
    return (r >> 40) / 16777216.0


def recent_ids(hist_ring: Sequence[int], n_gen: int, repeat_last_n: int) -> List[int]:
    """The ids the penalty looks at, newest first: hist[(ng - 1 - j) & 63] for j < min(repeat_last_n, 64, ng)."""
    n = max(0, min(int(repeat_last_n), HIST, int(n_gen)))
    return [int(hist_ring[(n_gen - 1 - j) & (HIST - 1)]) for j in range(n)]


def penalise(logits_f32: np.ndarray, hist_ring, n_gen: int, opts: Dict) -> Tuple[np.ndarray, List[int]]:
    """The row after the repeat penalty (float32: v / rp if v > 0 else v * rp, each distinct valid id once) and the
    penalised ids.  No penalty when repeat_penalty == 1 or repeat_last_n <= 0."""
    v = np.array(logits_f32, dtype=np.float32, copy=True)
    rp = np.float32(opts["repeat_penalty"])
    pen: List[int] = []
    if rp != np.float32(1.0) and opts["repeat_last_n"] > 0:
        for t in recent_ids(hist_ring, n_gen, opts["repeat_last_n"]):
            if 0 <= t < v.shape[0] and t not in pen:
                pen.append(t)
                x = v[t]
                v[t] = np.float32(x / rp) if x > 0 else np.float32(x * rp)
    return v, pen


def _ord(x: np.float32) -> int:
    """float32 -> an integer that grows with the value, consecutive floats one apart."""
    b = int(np.array(x, dtype=np.float32).view(np.uint32))
    return b if b < 0x80000000 else 0x80000000 - b


def top_k_of(opts: Dict, V: int) -> int:
    K = int(opts["top_k"])
    if K <= 0 or K > TOPK_MAX:
        K = TOPK_MAX
    return min(K, V)


def ordered(v: np.ndarray, n: int) -> List[int]:
    """The first n ids by (value descending, index ascending)."""
    idx = np.arange(v.shape[0])
    with np.errstate(invalid="ignore"):
        order = np.lexsort((idx, -v.astype(np.float64)))
    return [int(i) for i in order[:n]]


@dataclass
class Draw:
    ids: List[int]            # candidates in order
    probs: List[float]        # normalised over all candidates (before the top-p cut)
    cut: int                  # nominal number of candidates kept by top-p
    token: int                # nominal pick
    picks: Set[int] = field(default_factory=set)  # picks of every outcome within delta


def draw(ids: List[int], vals: Sequence[float], opts: Dict, u: float, delta: float) -> Draw:
    """Temperature, top-p, renormalisation and pick over candidates in order, in float64."""
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
        cut = next((i + 1 for i in range(n) if cdf[i] >= tp), n)  # `>=` keeps the crossing element
        cuts = {cut} | {i + 1 for i in range(n) if abs(cdf[i] - tp) <= delta}

    def pick(c: int, uu: float) -> int:
        zc = cdf[c - 1]
        return ids[next((i for i in range(c) if uu * zc < cdf[i]), c - 1)]  # else: the cut's last candidate

    d = Draw(ids=list(ids), probs=probs, cut=cut, token=pick(cut, u))
    for c in cuts:
        for uu in (u - delta, u, u + delta):
            d.picks.add(pick(c, uu))
    return d


@dataclass
class RowRef:
    admissible: Set[int]
    token: int
    ids: List[int]        # nominal candidates in order ([argmax] when greedy)
    probs: List[float]
    cut: int
    penalised: List[int]
    values: np.ndarray    # the row after the penalty (float32)
    support: Set[int]     # every id that is a candidate under some admitted order
    firsts: Set[int]      # every id that is the first candidate under some admitted order

    @property
    def decided(self) -> bool:
        return len(self.admissible) == 1


def reference_detail(logits_f32, hist_ring, n_gen: int, opts: Dict, delta: float = DELTA) -> RowRef:
    v, pen = penalise(logits_f32, hist_ring, n_gen, opts)
    raw = np.asarray(logits_f32, dtype=np.float32)
    V = v.shape[0]
    greedy = opts["temperature"] <= 0
    K = 1 if greedy else top_k_of(opts, V)
    ext = ordered(v, min(K + 1, V))
    # adjacent candidates within 2 float32 ulp, one of them penalised: the device's division may round the other
    # way, so both orders are admitted (not when both were penalised from the same raw value: the same operation on
    # the same input rounds the same way, and the index decides)
    orders = [ext[:K]]
    for i in range(min(K, len(ext) - 1)):
        a, b = ext[i], ext[i + 1]
        if abs(_ord(v[a]) - _ord(v[b])) <= 2 and (a in pen or b in pen):
            if a in pen and b in pen and _ord(raw[a]) == _ord(raw[b]):
                continue
            sw = list(ext)
            sw[i], sw[i + 1] = b, a
            orders.append(sw[:K])
    support = set().union(*[set(o) for o in orders])
    firsts = {o[0] for o in orders}
    if greedy:
        return RowRef(set(firsts), ext[0], ext[:1], [1.0], 1, pen, v, support, firsts)
    u = u_of(int(opts["seed"]), int(n_gen))
    draws = [draw(o, [v[i] for i in o], opts, u, delta) for o in orders]
    adm = set().union(*[d.picks for d in draws])
    d0 = draws[0]
    return RowRef(adm, d0.token, d0.ids, d0.probs, d0.cut, pen, v, support, firsts)


def reference_row(logits_f32, hist_ring, n_gen: int, opts: Dict, delta: float = DELTA) -> Tuple[Set[int], int]:
    """(the admissible tokens, the nominal token) of one row."""
    r = reference_detail(logits_f32, hist_ring, n_gen, opts, delta)
    return r.admissible, r.token


STATE_KEYS = ("tok", "pos", "gen", "n_gen", "max_new", "done", "hist", "slot")


def advance_reference(state: Dict[str, np.ndarray], tokens: Sequence[int], rows: Sequence[Dict],
                      T_max: int) -> Dict[str, np.ndarray]:
    """sample.hip advance_row on every live row: gen[m][ng], hist[m][ng & 63], n_gen and tok are written; done is set
    on eos, on a stop id >= 0, on ng + 1 >= max_new or on pos + 1 >= T_max, otherwise pos += 1.  Rows with slot < 0
    or done at entry keep every array.  ``state`` holds int arrays (hist [M][64], gen [M][ldg]); a copy is returned."""
    s = {k: np.array(state[k], copy=True) for k in STATE_KEYS}
    for m, o in enumerate(rows):
        if s["slot"][m] < 0 or s["done"][m]:
            continue
        t, ng = int(tokens[m]), int(s["n_gen"][m])
        s["gen"][m, ng] = t
        s["hist"][m, ng & (HIST - 1)] = t
        s["n_gen"][m] = ng + 1
        s["tok"][m] = t
        stops = [int(o.get("eos_id", -1))] + [int(x) for x in o.get("stop", ())][:3]
        stop = any(x >= 0 and x == t for x in stops)
        if stop or ng + 1 >= int(s["max_new"][m]) or int(s["pos"][m]) + 1 >= T_max:
            s["done"][m] = 1
        else:
            s["pos"][m] += 1
    return s


# ---- the inputs of the exact-token tests (tests/test_sampler_exact_gpu.py 3a; the undecided share of
# tests/test_sampler_ref.py is computed on the same rows)

KINDS = [  # (temperature, top_k, top_p, repeat_penalty)
    (0.8, 40, 0.9, 1.1), (0.8, 40, 0.9, 0.8), (1.0, 256, 1.0, 1.0), (1.2, 10, 0.5, 1.3), (0.7, 100, 0.95, 1.1),
    (1.0, 64, 1.0, 1.1), (0.9, 33, 0.8, 1.0), (1.0, 0, 1.0, 1.1), (0.0, 40, 1.0, 1.1)]
LAST_N = [64, 20, 0]
N_GEN = [0, 1, 5, 63, 64, 65, 100, 200]
EXACT_M, EXACT_LAUNCHES, GEN_W, MAX_NEW, T_MAX, POS0 = 64, 4, 256, 250, 2048, 300


def new_state(M: int, V: int, rng: np.random.Generator, n_gen, pos=POS0, max_new=MAX_NEW) -> Dict[str, np.ndarray]:
    """A decode state whose every array is filled (so an unexpected write shows): random tok / gen / hist."""
    return dict(tok=rng.integers(0, V, M).astype(np.int32),
                pos=np.broadcast_to(np.asarray(pos, dtype=np.int32), (M,)).copy(),
                gen=rng.integers(0, V, (M, GEN_W)).astype(np.int32),
                n_gen=np.broadcast_to(np.asarray(n_gen, dtype=np.int32), (M,)).copy(),
                max_new=np.broadcast_to(np.asarray(max_new, dtype=np.int32), (M,)).copy(),
                done=np.zeros(M, dtype=np.int32),
                hist=rng.integers(0, V, (M, HIST)).astype(np.int32),
                slot=np.arange(M, dtype=np.int32))


@dataclass
class Case:
    logits: np.ndarray            # [M][V] float32
    rows: List[Dict]              # per-row options (ops.sample_params_tensor's dicts)
    kinds: List[int]              # index into KINDS per row
    state: Dict[str, np.ndarray]
    T_max: int = T_MAX


def exact_case(V: int, launch: int) -> Case:
    """Launch ``launch`` (0..3) of the exact-token test at vocabulary V: logits randn * 3 with three entries raised
    by 4 (launch 2: one exact tie among the top; launch 3: the upper half of the row at -inf); options, n_gen and
    repeat_last_n cycle per row so that every (kind, last_n, n_gen) triple occurs; the ring holds the row's top 6
    ids among the most recent ones plus random ids, two of them outside [0, V); seeds up to 2^62."""
    M = EXACT_M
    rng = np.random.default_rng(1000 * V + launch)
    logits = (rng.standard_normal((M, V)) * 3.0).astype(np.float32)
    logits[:, :3] += np.float32(4.0)
    if launch == 2:
        logits[:, 7] = logits[:, 1]
    if launch == 3:
        logits[:, V // 2:] = -np.inf
    rows, kinds, n_gen = [], [], []
    for i in range(M):
        g = launch * M + i
        kind = g % len(KINDS)
        t, k, p, rp = KINDS[kind]
        kinds.append(kind)
        n_gen.append(N_GEN[g % len(N_GEN)])
        rows.append(dict(temperature=t, top_k=k, top_p=p, repeat_penalty=rp,
                         repeat_last_n=LAST_N[(g // len(KINDS)) % len(LAST_N)], eos_id=-1,
                         seed=int(rng.integers(0, 1 << 62))))
    st = new_state(M, V, rng, n_gen)
    top = np.argsort(-logits, axis=1, kind="stable")[:, :6]
    for i in range(M):
        ng = n_gen[i]
        for j in range(6):  # the top ids at ages 0, 3, 6, ..., 15: inside a window of 20 once n_gen >= 16
            st["hist"][i, (ng - 1 - 3 * j) & (HIST - 1)] = top[i, j]
        st["hist"][i, (ng - 3) & (HIST - 1)] = -1
        st["hist"][i, (ng - 6) & (HIST - 1)] = V + 3
    return Case(logits, rows, kinds, st)


def case_refs(case: Case, delta: float = DELTA) -> List[RowRef]:
    return [reference_detail(case.logits[m], case.state["hist"][m], int(case.state["n_gen"][m]), case.rows[m], delta)
            for m in range(len(case.rows))]


def undecided_counts(refs: Sequence[RowRef], kinds: Sequence[int]) -> Tuple[int, Dict[int, List[int]]]:
    """(undecided rows, {kind: [undecided, rows]})."""
    per: Dict[int, List[int]] = {}
    for r, k in zip(refs, kinds):
        c = per.setdefault(k, [0, 0])
        c[0] += 0 if r.decided else 1
        c[1] += 1
    return sum(c[0] for c in per.values()), per
