"""Exact decode-attention cases: one-hot, uniform and power-of-two weights (host side; imports without a GPU).

Why they can be exact (csrc/attention.hip: QK^T and PV on v_mfma_f32_16x16x32_bf16, online softmax on exp2f with
``sl2 = scale * LOG2E`` folded into the scores, (m, l, O) merged over waves in LDS and over splits in global memory,
one ``num * v_rcp_f32(den)`` at the end, rounded to bf16).

QK^T.  q and K hold integers (powers of two times +-1, exact in bf16 and, for K, in e4m3), so every product and every
partial sum of Q K^T is an integer below 2^24 (``Data.check`` asserts A * hd * max |K| < 2^24): the MFMA result is
exact whatever the summation order.  The kernel multiplies by sl2 in fp32, subtracts the running maximum and takes
exp2f.  Two facts carry the cases:

* equal integer scores give bit-equal scaled scores, so every position at the maximum has p = exp2f(0) = 1 exactly;
* a scaled-score gap of 160 or more gives p = 0 exactly (2^-160 < 2^-149, the smallest fp32 denormal, whatever the
  denormal mode) -- and alpha = 0, and a wave / split merge factor f = 0: a wave or split that holds no winning
  position contributes 0 * finite = 0.

PV and the division.  With p in {0, 1} and integer V the accumulators o and l are integers, every LDS and global
merge is exact, and the last operation is num * rcp(den) (v_rcp_f32, 1 ulp) rounded to bf16: where the exact
quotient is a bf16 number, an fp32 error of a few ulp cannot cross a bf16 rounding boundary, so the output equals
the quotient bit for bit.

Key codes.  Position t of a (slot, kv head) holds K[t] = c_t: +1 on every head dim but a set F_t of flipped dims
(-1).  Position perm(0) has F = {} (the origin), perm(1..hd) the single flips {j} (j in a random order, so short
rows do not always use the low dims), the rest distinct double flips {i, j}; perm is a per-(slot, kv head)
permutation of 0..L-1 that puts the origin on the target of one of the group's heads.  A query head that selects t*
is q = A c_t* with A a power of two: score(t) = A (hd - 2 |F_t ^ F_t*|), so the winner leads every neighbour by
exactly 2 A, contributed by ONE head dim -- a dropped or mis-indexed dim, 8-dim lane chunk or 32-dim fragment of the
QK product makes a neighbour tie, den becomes 2 and the output an average.  A = 1024 (2048 where a K scale of 0.5
halves the scores): 2 A sl2 >= 160 at every head dim here (asserted in fp32 by ``Data.check``).

Poison.  In every family the positions t >= L of a row's slot, and every slot no row uses, hold values that wreck
the output if they leak: K[t] = 2 c_t* of the kv group's first head (for kv head 0: the row's first head), which
would win outright, and V[t] = 2^14 (bf16 cache) or 448 (fp8).  Finite on purpose: inside the last partial block the
kernel computes 0 * V[t] (the comment at the top of attention.hip).

Families.
(a) ``select``: every query head has its own target; out[m, h] == V[slot, kh, t*] (times the V scale) bit for bit
    (den = 1, rcp(1) = 1).  V: integers -128..127 (bf16) or arbitrary finite e4m3 codes but -0 (fp8, with K / V scales
    among 0.5, 1, 2).  A row's targets cover 0 and L - 1 and, where L allows, 31, 32, a position of the last full
    block and the origin (all hd single-dim margins at once when L > hd).
(b) ``uniform``: q = 0, so p = 1 on every live position and den = L.  V[t] = c + u[t] - u[(t + 1) mod L] with
    integer c (-64..64; fp8 -4..4) and u (-4..4; fp8 -3..3): the perturbation sums to zero over the L live positions,
    the mean is the integer c for every L, power of two or not: out[m, h] == c.  One dropped, duplicated or leaked
    position misses the integer.
(c) ``graded``: the only family with alpha and merge factors other than 0 and 1.  scale = float32(0.6931472), for
    which scale * LOG2E == 1.0f exactly in fp32 (the neighbouring floats give 1 -+ 2^-23), so the scaled scores are
    the integer scores.  Per (slot, kv head) one code c; a "near" set of positions has K = c with 0..3 dims of a
    6-dim pool zeroed, every other live position K = -8 c.  Head g of the group asks with q = c less the pool dims
    named by the bits of g (amplitude 1; g = 0 is c itself), so the heads of a group weigh the near set differently:
    p = 2^-e with e = |zeroed(t) \\ zeroed(g)| in 0..3, everything else at least 9 (hd - 4) below the maximum, p = 0.
    The near set includes positions 0 and L - 1, three blocks of one wave's list with rising scores and random
    others.  |V| <= 16, so every partial sum is a multiple of 2^-3 below 2^15, exact in any order; den is in
    general no power of two and the expectation is the fp64 quotient rounded to nearest-even in bf16.  An element
    whose quotient lies within a relative 2^-18 of a bf16 rounding midpoint may take either neighbour
    (``Data.alt``; ``Data.near_mid`` counts them, under 1 % of every case).
    This family rests on exp2f(-k) == 2^-k on the device for k = 0..3.  Measured on an MI355X (a one-thread kernel
    built with the library's compile flags, arguments passed at run time): exp2f(0) = 0x3f800000, exp2f(-1) =
    0x3f000000, exp2f(-2) = 0x3e800000, exp2f(-3) = 0x3e000000 -- exact (EXP2F_MEASURED), so the family is held to
    the exact expectation; exp2f(-149) = 0x00000001 and exp2f(-150) = exp2f(-160) = 0.

An idle row (slot < 0) reads nothing and gets a zero output row from the register kernel (its merge finds l = 0)
and from the ring alike; the expectation of such a row is zeros, and the pad columns of ``out`` keep the sentinel.
"""
from __future__ import annotations

import functools
import math
import sys
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

if str(Path(__file__).resolve().parent.parent) not in sys.path:
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from cain_amd import ops  # noqa: E402  (pure-Python layout helpers; the library is loaded on first kernel call)

TWO24 = 1 << 24
LOG2E32 = np.float32(1.4426950408889634)
GRADED_SCALE = float(np.float32(0.6931472))
SENTINEL = -12352.0  # bf16-exact, outside every expectation
V_POISON = {False: 16384.0, True: 448.0}
FAMILIES = ("select", "uniform", "graded")
#: the bits of exp2f(0), exp2f(-1), exp2f(-2), exp2f(-3) as an MI355X returned them (module doc, family (c))
EXP2F_MEASURED = (0x3F800000, 0x3F000000, 0x3E800000, 0x3E000000)

_E4M3 = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
#: every finite e4m3 code but -0 (0 * finite sums give +0)
_E4M3_CODES = np.array([c for c in range(256) if c not in (0x7F, 0xFF, 0x80)], dtype=np.uint8)


# ---------------------------------------------------------------- geometries, lengths, launches
@dataclass(frozen=True)
class Geo:
    """One geometry of tests/test_attn_exact_gpu.py.  ``aw``: waves per workgroup cain_attention_ex picks (8 while
    rows * Hkv <= 64 at hd <= 128, else 4); ``path``: what its nsplit list forces (the merge conditions of
    attn_decode_kernel: vec = hd 256, 1 < nsplit <= 16, 2 AW 64 < G hd <= 8 AW 64; "2 outputs per thread" = nsplit
    <= 16 and G hd <= 2 AW 64; else the LDS-weights merge)."""
    H: int
    Hkv: int
    hd: int
    rows: int
    aw: int
    T_max: int
    nsplits: Tuple[int, ...]
    path: str
    kv8: bool = True
    ring: Optional[bool] = None  # ring cases: whether cain_attention_ex takes the ring at a CU budget of 8
    idle: Tuple[int, ...] = ()   # ring cases: the idle rows

    @property
    def G(self) -> int:
        return self.H // self.Hkv

    @property
    def id(self) -> str:
        return f"H{self.H}-Hkv{self.Hkv}-hd{self.hd}-M{self.rows}-{self.path}"


GEOS: List[Geo] = [
    Geo(8, 2, 128, 6, 8, 1024, (1, 2, 3, 8, 16, 17, 64), "aw8-two_out_merge-ldsw17_64-emptysplits"),
    Geo(16, 1, 64, 4, 8, 1024, (1, 2, 8, 17), "aw8-G16-two_out_merge-ldsw17"),
    Geo(7, 1, 128, 4, 8, 1024, (1, 3, 16, 17), "aw8-G7-two_out_merge-ldsw17"),
    Geo(8, 1, 256, 3, 4, 512, (1, 2, 8, 9, 16, 17), "aw4-hd256-vec16B_merge-ldsw17"),
    Geo(16, 16, 256, 5, 4, 512, (1, 2, 16, 17), "aw4-hd256-G1-two_out_merge-ldsw17"),
    Geo(12, 4, 96, 20, 4, 512, (1, 2, 5), "aw4-80pairs-two_out_merge"),
    Geo(8, 4, 64, 20, 4, 512, (1, 2, 5, 17), "aw4-80pairs-two_out_merge-ldsw17"),
    Geo(8, 4, 128, 20, 4, 512, (1, 2, 5, 17), "aw4-80pairs-two_out_merge-ldsw17"),
]

RING_CU = 8  # ops.set_cu_budget around the ring cases: a persistent grid of 8 workgroups
#: pair p = m Hkv + kh is entry i of compute wave w of workgroup b with p = b + 8 (w + 4 i): the idle rows of the
#: 512-pair cases put entries 0, 7 and 15 of one wave's list idle (pairs 0, 224, 480 and their rows' other kv heads)
RING_GEOS: List[Geo] = [
    Geo(8, 2, 128, 8, 8, 128, (1,), "ring-16pairs-lower_edge", kv8=False, ring=True, idle=(3,)),
    Geo(4, 4, 128, 4, 8, 128, (1,), "ring-16pairs-lower_edge", kv8=False, ring=True, idle=(2,)),
    Geo(8, 2, 128, 256, 4, 64, (1,), "ring-512pairs-upper_edge", kv8=False, ring=True, idle=(0, 112, 240)),
    Geo(4, 4, 128, 128, 4, 64, (1,), "ring-512pairs-upper_edge", kv8=False, ring=True, idle=(0, 56, 120)),
    Geo(6, 3, 128, 5, 8, 128, (1,), "ring-15pairs-falls_back_aw8", kv8=False, ring=False, idle=(1,)),
    Geo(6, 3, 128, 171, 4, 64, (1,), "ring-513pairs-falls_back_aw4", kv8=False, ring=False, idle=(0, 85, 170)),
]


def lengths_for(g: Geo) -> List[int]:
    """The lengths of a geometry: the block edges (multiples of 32 and their neighbours), hd + 1 (all single
    flips present), one, two and three turns of the AW waves, and T_max; what fits under T_max, without repeats."""
    aw = g.aw
    want = [1, 16, 31, 32, 33, 63, 64, 65, g.hd + 1, 32 * aw - 1, 32 * aw, 32 * aw + 1, 3 * 32 * aw + 1,
            g.T_max - 1, g.T_max]
    out: List[int] = []
    for L in want:
        if L <= g.T_max and L not in out:
            out.append(L)
    return out


@dataclass(frozen=True)
class Launch:
    """One launch: per row its length (0: the idle row) and slot (-1: idle) into S = rows + 3 slots."""
    geo: Geo
    idx: int
    lengths: Tuple[int, ...]
    slot: Tuple[int, ...]

    @property
    def S(self) -> int:
        return self.geo.rows + 3

    @property
    def id(self) -> str:
        return f"{self.geo.id}-launch{self.idx}"


@functools.lru_cache(maxsize=None)
def launches(g: Geo) -> Tuple[Launch, ...]:
    """The launches of a geometry: its lengths dealt over ceil(n / live rows) launches (launch i takes lengths
    i, i + n_launch, ...: short and long rows side by side; spare rows repeat the list), one idle row each (a ring
    geometry: ``g.idle``), and ``slot`` a permutation into S slots with slot[m] != m on every row."""
    Ls = lengths_for(g)
    idle = g.idle if g.idle else None
    live = g.rows - (len(idle) if idle else 1)
    n = -(-len(Ls) // live)
    out = []
    for i in range(n):
        rng = np.random.default_rng(1000 * g.rows + 10 * g.hd + i)
        mine = Ls[i::n]
        k = 0
        while len(mine) < live:  # spare rows: the other launches' lengths, then the list again
            mine.append(Ls[(i + 1 + k) % len(Ls)])
            k += 1
        mine = [mine[j] for j in rng.permutation(live)]
        idle_rows = set(idle) if idle else {(i + 1) % g.rows}
        lens, it = [], iter(mine)
        for m in range(g.rows):
            lens.append(0 if m in idle_rows else next(it))
        while True:
            slot = rng.permutation(g.rows + 3)[: g.rows]
            if all(int(slot[m]) != m for m in range(g.rows)):
                break
        slot = [-1 if m in idle_rows else int(slot[m]) for m in range(g.rows)]
        out.append(Launch(g, i, tuple(lens), tuple(slot)))
    return tuple(out)


def all_launches() -> List[Launch]:
    return [l for g in GEOS + RING_GEOS for l in launches(g)]


# ---------------------------------------------------------------- one case's tensors
@dataclass
class Data:
    """One (launch, family, cache type): ``q`` [M, H, hd] int64, ``K`` [S, Hkv, T_max, hd] int8 (the STORED values;
    times ``kscale`` on an fp8 cache), ``V`` [S, Hkv, T_max, hd] fp32 stored values (times ``vscale``), ``want``
    [M, H, hd] fp32 holding bf16 numbers, ``alt`` the other admissible neighbour (graded; == want elsewhere)."""
    launch: Launch
    family: str
    kv8: bool
    q: torch.Tensor
    K: torch.Tensor
    V: torch.Tensor
    want: torch.Tensor
    alt: torch.Tensor
    scale: float
    kscale: float = 1.0
    vscale: float = 1.0
    A: int = 1
    near_mid: int = 0
    info: Dict = field(default_factory=dict)  # select: targets [M, H]; uniform: c; graded: near sets

    @property
    def sl2(self) -> np.float32:
        return np.float32(self.scale) * LOG2E32

    def check(self) -> None:
        """The bounds the module doc rests on (also run by every generator)."""
        g = self.launch.geo
        kmax = float(self.K.abs().max()) * self.kscale
        assert self.A * g.hd * kmax < TWO24, (self.A, g.hd, kmax)
        assert int(self.q.abs().max()) <= self.A
        if self.family == "select":
            assert np.float32(2 * self.A * self.kscale) * self.sl2 >= np.float32(160.0), (self.A, self.sl2)
        if self.family == "graded":
            assert self.sl2 == np.float32(1.0)
        assert bool(torch.isfinite(self.V).all())


def _codes(hd: int, n: int, rng) -> np.ndarray:
    """[n, hd] int64 of +-1: rank 0 the origin, ranks 1..hd single flips (dims in random order), then distinct
    double flips."""
    c = np.ones((n, hd), dtype=np.int64)
    order = rng.permutation(hd)
    ns = min(hd, n - 1)
    c[np.arange(1, 1 + ns), order[:ns]] = -1
    nd = n - 1 - ns
    if nd > 0:
        i, j = np.triu_indices(hd, 1)
        assert nd <= len(i), "more positions than distinct codes"
        pick = rng.permutation(len(i))[:nd]
        r = np.arange(1 + ns, n)
        c[r, i[pick]] = -1
        c[r, j[pick]] = -1
    return c


def _targets(L: int, H: int, m: int, rng) -> np.ndarray:
    """The positions a row's H heads select: 0 and L - 1 first, then 31, 32, a position of the last full block,
    then random ones; dealt to the heads by a random permutation."""
    extra = [t for t in (31, 32) if t < L]
    if L >= 32:
        extra.append(32 * (L // 32 - 1) + 7)
    if extra:
        r = m % len(extra)
        extra = extra[r:] + extra[:r]
    tl: List[int] = []
    for t in [0, L - 1] + extra:
        if t not in tl:
            tl.append(t)
    tl = tl[:H]
    while len(tl) < H:
        tl.append(int(rng.integers(L)))
    out = np.empty(H, dtype=np.int64)
    out[rng.permutation(H)] = tl
    return out


def _v_poisoned(S, Hkv, T_max, hd, kv8):
    return np.full((S, Hkv, T_max, hd), V_POISON[kv8], dtype=np.float32)


def _select_keys(l: Launch, rng, K: np.ndarray) -> np.ndarray:
    """Fills K (poison everywhere first) with the key codes of every live row; returns the targets [M, H] (-1 on
    the idle row)."""
    g = l.geo
    G = g.G
    K[:] = 4 * rng.integers(0, 2, K.shape, dtype=np.int8) - 2  # unused slots: poison-sized random codes
    tg = np.full((g.rows, g.H), -1, dtype=np.int64)
    for m, (L, s) in enumerate(zip(l.lengths, l.slot)):
        if s < 0:
            continue
        tg[m] = _targets(L, g.H, m, rng)
        for kh in range(g.Hkv):
            code = _codes(g.hd, L, rng)
            pos = rng.permutation(L)
            origin = tg[m, kh * G + kh % G]
            w = int(np.nonzero(pos == origin)[0][0])
            pos[0], pos[w] = pos[w], pos[0]
            K[s, kh, pos] = code
            K[s, kh, L:] = 2 * K[s, kh, tg[m, kh * G]]
    return tg


def select_scales(idx: int, kv8: bool) -> Tuple[float, float]:
    return ((1.0, 2.0), (2.0, 1.0), (0.5, 2.0))[idx % 3] if kv8 else (1.0, 1.0)


def _gen_select(l: Launch, kv8: bool) -> Data:
    g = l.geo
    rng = np.random.default_rng(7 + 13 * l.idx + g.hd + 1000 * g.rows + int(kv8))
    ks, vs = select_scales(l.idx, kv8)
    A = 1024 if ks >= 1.0 else 2048
    K = np.empty((l.S, g.Hkv, g.T_max, g.hd), dtype=np.int8)
    tg = _select_keys(l, rng, K)
    V = _v_poisoned(l.S, g.Hkv, g.T_max, g.hd, kv8)
    q = np.zeros((g.rows, g.H, g.hd), dtype=np.int64)
    want = np.zeros((g.rows, g.H, g.hd), dtype=np.float32)
    for m, (L, s) in enumerate(zip(l.lengths, l.slot)):
        if s < 0:
            continue
        if kv8:
            V[s, :, :L] = _E4M3.numpy()[rng.choice(_E4M3_CODES, (g.Hkv, L, g.hd))]
        else:
            V[s, :, :L] = rng.integers(-128, 128, (g.Hkv, L, g.hd))
        for h in range(g.H):
            kh = h // g.G
            q[m, h] = A * K[s, kh, tg[m, h]].astype(np.int64)
            want[m, h] = V[s, kh, tg[m, h]] * vs
    w = torch.from_numpy(want)
    return Data(l, "select", kv8, torch.from_numpy(q), torch.from_numpy(K), torch.from_numpy(V), w, w,
                1.0 / math.sqrt(g.hd), ks, vs, A, 0, {"targets": torch.from_numpy(tg)})


def _gen_uniform(l: Launch, kv8: bool) -> Data:
    g = l.geo
    rng = np.random.default_rng(11 + 13 * l.idx + g.hd + 1000 * g.rows + int(kv8))
    K = np.empty((l.S, g.Hkv, g.T_max, g.hd), dtype=np.int8)
    _select_keys(l, rng, K)  # any finite K: q = 0
    V = _v_poisoned(l.S, g.Hkv, g.T_max, g.hd, kv8)
    camp, uamp = (4, 3) if kv8 else (64, 4)
    cs = np.zeros((g.rows, g.Hkv, g.hd), dtype=np.int64)
    want = np.zeros((g.rows, g.H, g.hd), dtype=np.float32)
    for m, (L, s) in enumerate(zip(l.lengths, l.slot)):
        if s < 0:
            continue
        c = rng.integers(-camp, camp + 1, (g.Hkv, 1, g.hd))
        u = rng.integers(-uamp, uamp + 1, (g.Hkv, L, g.hd))
        V[s, :, :L] = c + u - np.roll(u, -1, axis=1)
        cs[m] = c[:, 0]
        want[m] = np.repeat(c[:, 0], g.G, axis=0)
    w = torch.from_numpy(want)
    return Data(l, "uniform", kv8, torch.zeros((g.rows, g.H, g.hd), dtype=torch.int64), torch.from_numpy(K),
                torch.from_numpy(V), w, w, 1.0 / math.sqrt(g.hd), info={"c": torch.from_numpy(cs)})


def _near_set(L: int, aw: int, rng) -> List[Tuple[int, int]]:
    """(position, zeroed dims k) of a row's near set: 0 and L - 1; blocks 0, AW and 2 AW (one wave's list at one
    split) with k = 3, 1, 0, so that wave's running maximum rises twice; up to 8 random others, so other waves see
    one, none, or a falling sequence.  At least one k = 0."""
    cand = [(0, 2), (L - 1, 1), (5, 3), (32 * aw + 7, 1), (64 * aw + 9, 0)]
    cand += [(int(rng.integers(L)), int(rng.integers(4))) for _ in range(8)]
    seen, out = set(), []
    for t, k in cand:
        if 0 <= t < L and t not in seen:
            seen.add(t)
            out.append((t, k))
    if all(k for _, k in out):
        out[-1] = (out[-1][0], 0)
    return out


def bf16_neighbours(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp64 x -> (nearest-even bf16 as fp32, the other admissible neighbour, near-midpoint mask): an element whose
    value lies within a relative 2^-18 of the midpoint of two neighbouring bf16 numbers may round to either."""
    r = x.float().bfloat16()
    r64 = r.double()
    bits = r.view(torch.int16).to(torch.int32)
    step = torch.where(x.abs() > r64.abs(), 1, -1)  # towards x: magnitude up or down
    nb = (bits + step).to(torch.int16).view(torch.bfloat16)
    nb64 = nb.double()
    mid = (r64 + nb64) / 2
    near = (x != r64) & ((x - mid).abs() <= 2.0 ** -18 * mid.abs())
    return r.float(), torch.where(near, nb.float(), r.float()), near


def _gen_graded(l: Launch, kv8: bool) -> Data:
    g = l.geo
    rng = np.random.default_rng(17 + 13 * l.idx + g.hd + 1000 * g.rows + int(kv8))
    K = np.empty((l.S, g.Hkv, g.T_max, g.hd), dtype=np.int8)
    K[:] = 4 * rng.integers(0, 2, K.shape, dtype=np.int8) - 2
    V = _v_poisoned(l.S, g.Hkv, g.T_max, g.hd, kv8)
    q = np.zeros((g.rows, g.H, g.hd), dtype=np.int64)
    num8 = np.zeros((g.rows, g.H, g.hd), dtype=np.int64)
    den8 = np.ones((g.rows, g.H, 1), dtype=np.int64)
    nears = {}
    for m, (L, s) in enumerate(zip(l.lengths, l.slot)):
        if s < 0:
            continue
        V[s, :, :L] = rng.integers(-16, 17, (g.Hkv, L, g.hd))
        for kh in range(g.Hkv):
            c = 2 * rng.integers(0, 2, g.hd) - 1
            pool = rng.permutation(g.hd)[:6]
            K[s, kh, :L] = -8 * c
            K[s, kh, L:] = 2 * c
            near = _near_set(L, g.aw, rng)
            zero = {}
            for t, k in near:
                zero[t] = set(int(d) for d in rng.choice(pool, k, replace=False))
                K[s, kh, t] = c
                K[s, kh, t, list(zero[t])] = 0
            nears[(m, kh)] = near
            for gi in range(g.G):
                h = kh * g.G + gi
                zg = set(int(pool[b]) for b in range(4) if (gi >> b) & 1)
                q[m, h] = c
                q[m, h, list(zg)] = 0
                e = {t: len(zero[t] - zg) for t, _ in near}
                emin = min(e.values())
                assert emin == 0 and max(e.values()) <= 3
                wts = np.array([8 >> e[t] for t, _ in near], dtype=np.int64)
                vals = V[s, kh, [t for t, _ in near]].astype(np.int64)
                num8[m, h] = (wts[:, None] * vals).sum(0)
                den8[m, h] = wts.sum()
    x = torch.from_numpy(num8).double() / torch.from_numpy(den8).double()
    want, alt, near_mid = bf16_neighbours(x)
    for m, s in enumerate(l.slot):
        if s < 0:
            want[m], alt[m], near_mid[m] = 0.0, 0.0, False
    return Data(l, "graded", kv8, torch.from_numpy(q), torch.from_numpy(K), torch.from_numpy(V), want, alt,
                GRADED_SCALE, near_mid=int(near_mid.sum()),
                info={"near": nears, "num8": torch.from_numpy(num8), "den8": torch.from_numpy(den8)})


_GEN = {"select": _gen_select, "uniform": _gen_uniform, "graded": _gen_graded}


def make(l: Launch, family: str, kv8: bool) -> Data:
    d = _GEN[family](l, kv8)
    d.check()
    return d


def pack(d: Data) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(q bf16 [M, H hd], K cache, V^T cache) in the kernel's layouts (ops.pack_kcache / pack_vcache): bf16, or the
    e4m3 bytes as uint8."""
    g = d.launch.geo
    q = d.q.float().bfloat16().reshape(g.rows, g.H * g.hd)
    if d.kv8:
        k = d.K.float().to(torch.float8_e4m3fn).view(torch.uint8)
        v = d.V.to(torch.float8_e4m3fn).view(torch.uint8)
    else:
        k, v = d.K.float().bfloat16(), d.V.bfloat16()
    return q, ops.pack_kcache(k), ops.pack_vcache(v)


# ---------------------------------------------------------------- comparator
def mismatches(d: Data, got: torch.Tensor) -> Optional[str]:
    """None when ``got`` ([M, H hd] or [M, H, hd]) equals the expectation element by element (graded: either
    admissible neighbour); else the count and the first mismatch as (row, query head, kv head, 16-dim tile, got,
    want), and for ``select`` which position's V row that head's output equals, if any."""
    g = d.launch.geo
    o = got.detach().cpu().float().reshape(g.rows, g.H, g.hd)
    bad = ~((o == d.want) | (o == d.alt))
    n = int(bad.sum())
    if n == 0:
        return None
    m, h, e = (int(v) for v in bad.nonzero()[0])
    kh = h // g.G
    heads = len({(int(a), int(b)) for a, b, _ in bad.nonzero()[:4096]})
    msg = (f"{d.launch.id} {d.family} {'fp8' if d.kv8 else 'bf16'}: {n} of {bad.numel()} elements differ in "
           f"{heads}{'+' if n > 4096 else ''} (row, head) units; first at row {m} (length {d.launch.lengths[m]}, slot "
           f"{d.launch.slot[m]}), query head {h}, kv head {kh}, dim {e}, tile {e // 16}: got {float(o[m, h, e])!r}, "
           f"want {float(d.want[m, h, e])!r}")
    if d.family == "select" and d.launch.slot[m] >= 0:
        rows = d.V[d.launch.slot[m], kh] * d.vscale
        hit = (rows == o[m, h]).all(-1).nonzero().flatten().tolist()
        t = int(d.info["targets"][m, h])
        msg += f"; target position {t}, output equals the V row of position(s) {hit[:8] if hit else 'none'}"
    return msg


def assert_equal(d: Data, got: torch.Tensor, tag: str = "") -> None:
    rep = mismatches(d, got)
    assert rep is None, f"{tag}: {rep}"


# ---------------------------------------------------------------- the kernel's algorithm in plain torch
FAULTS = ("mask_le", "skip_last_block", "drop_wave", "loser_l_unweighted", "skip_kfrag", "swap_v_order",
          "ignore_slot", "alpha_not_on_l")


@functools.lru_cache(maxsize=None)
def _frag_index(T_max: int, hd: int):
    t = torch.arange(T_max)[:, None]
    dd = torch.arange(hd)[None, :]
    return ops.kfrag_off(t, dd, hd), ops.vfrag_off(t, dd, hd)


def _widen(p: torch.Tensor, kv8: bool, sc: float) -> torch.Tensor:
    return (p.view(torch.float8_e4m3fn).float() * sc) if kv8 else p.float()


def emulate(d: Data, kp: torch.Tensor, vp: torch.Tensor, qb: torch.Tensor, nsplit: int,
            fault: Optional[str] = None) -> torch.Tensor:
    """attn_decode_kernel on fp32 CPU tensors: 32-position blocks of a split dealt to AW waves, online softmax with
    bf16 P, the wave merge and the split merge, reading the PACKED caches through ops.kfrag_off / vfrag_off.
    ``fault``: one of FAULTS planted.  Returns [M, H, hd] fp32 holding bf16 numbers (idle rows: zeros)."""
    assert fault is None or fault in FAULTS
    l, g = d.launch, d.launch.geo
    G, hd, aw = g.G, g.hd, g.aw
    kidx, vidx = _frag_index(g.T_max, hd)
    kf = _widen(kp, d.kv8, d.kscale).reshape(l.S, g.Hkv, -1)
    vf = _widen(vp, d.kv8, d.vscale).reshape(l.S, g.Hkv, -1)
    q = qb.float().reshape(g.rows, g.H, hd)
    sl2 = torch.tensor(float(d.sl2), dtype=torch.float32)
    ninf = torch.tensor(float("-inf"))
    out = torch.zeros(g.rows, g.H, hd)

    def merge(parts):
        ms = torch.stack([p[0] for p in parts])  # [n, G]
        Mx = ms.max(0).values
        f = torch.where(ms == ninf, torch.zeros(()), torch.exp2(ms - Mx))
        ls = torch.stack([p[1] for p in parts])
        os_ = torch.stack([p[2] for p in parts])
        return Mx, f, ls, os_

    for m in range(g.rows):
        if l.slot[m] < 0:
            continue
        s = m if fault == "ignore_slot" else l.slot[m]
        L = l.lengths[m]
        nblk = (L + 31) >> 5
        bps = -(-nblk // nsplit)
        for kh in range(g.Hkv):
            Q = q[m, kh * G:(kh + 1) * G]
            kflat, vflat = kf[s, kh], vf[s, kh]
            splits = []
            for sp in range(nsplit):
                b0, b1 = sp * bps, min(nblk, sp * bps + bps)
                waves = []
                for w in range(aw):
                    m_run, l_run, o = torch.full((G,), float("-inf")), torch.zeros(G), torch.zeros(G, hd)
                    for blk in range(b0 + w, b1, aw):
                        if fault == "skip_last_block" and blk == b1 - 1:
                            continue
                        t = torch.arange(32 * blk, 32 * blk + 32)
                        Kb = kflat[kidx[t]]
                        if fault == "skip_kfrag":
                            Kb = Kb.clone()
                            Kb[:, 32:64] = 0
                        sc = Kb @ Q.t()  # [32, G]
                        livemask = (t <= L) if fault == "mask_le" else (t < L)
                        sc = torch.where(livemask[:, None], sc * sl2, ninf)
                        m_new = torch.maximum(m_run, sc.max(0).values)
                        alpha = torch.exp2(m_run - m_new)
                        p = torch.exp2(sc - m_new)
                        order = torch.arange(32)
                        if fault == "swap_v_order":
                            order[0], order[31] = 31, 0
                        Vb = vflat[vidx[t[order]]]
                        l_run = (l_run if fault == "alpha_not_on_l" else l_run * alpha) + p.sum(0)
                        o = o * alpha[:, None] + p.bfloat16().float().t() @ Vb
                        m_run = m_new
                    waves.append((m_run, l_run, o))
                if fault == "drop_wave":
                    waves = waves[1:]
                Mx, f, ls, os_ = merge(waves)
                lsum = ls.sum(0) if fault == "loser_l_unweighted" else (f * ls).sum(0)
                splits.append((Mx, lsum, (f[:, :, None] * os_).sum(0)))
            _, f, ls, os_ = merge(splits)
            den = (f * ls).sum(0)
            num = (f[:, :, None] * os_).sum(0)
            r = torch.where(den > 0, 1.0 / den, torch.zeros(()))
            out[m, kh * G:(kh + 1) * G] = (num * r[:, None]).bfloat16().float()
    return out
