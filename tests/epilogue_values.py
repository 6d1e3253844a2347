"""Per-element epilogue checks through one-hot activation rows (host side; imports without a GPU).

Delivery.  An activation row that holds one value ``a`` at column ``k`` and zeros elsewhere makes every GEMM path
hand ``a W[n, k]`` to its epilogue exactly: every other product is a zero, and a sum of one value and zeros is that
value in any order, tiling or split.  The test therefore chooses, element by element, what the epilogue sees.
``a`` is 1 on the bf16 path, a power of two on the weight-quantised families (whose decoded weights are the
integers of ``exact.GENERATORS``, taken from ``exact.Weights.w / den``, never from a kernel) and 448 2^e on the
activation-quantised pair (the row quantiser's scale is then exactly 2^e and its byte exactly 448, see
``exact.int_x``'s ``plant``).  Formats between accumulator and epilogue, mirrored by ``delivery_exact``:

* fp32 everywhere on the skinny, batched, stream and tile kernels and on the wide kernel's variant 4 slabs: exact;
* wide bf16 kernel, variant 0, ks > 1: fp16 slabs, each lane's four values scaled by 2^-ex,
  ex = max(frexp_exp(max |v|) - 14, 0) (wgemm.hip).  A bf16 value is exact in fp16 while its lowest bit is at least
  2^-24 after the scaling and its magnitude below 2^16 -- so the largest finite bf16 may not share four columns with
  anything small: the value sets of these cases stop below 2^14 (``cap``), where ex = 0;
* wide W8A8 / W4A8 kernels, ks > 1: unscaled fp16 slabs (wgemm8.hip): |v| <= 65504, lowest bit >= 2^-24.

Fused QKV at real angles (``qkv_want`` / ``qkv_check``).  cos / sin are fp32(cos), fp32(sin) of the engine's angles
(``rope_inv_freq``, theta 1e4), given to the kernel and to the reference.  Per rotation pair, from the delivered
values w and the fp32 bias: v = bf16(fp32(w + b)) (one IEEE fp32 addition, one round-to-nearest-even), then
r1 = v1 c - v2 s, r2 = v2 c + v1 s in float64.  An fp32 evaluation -- two products and one sum, each rounded once,
or one product and one fused multiply-add -- differs from r by at most d = 3 2^-24 (|v1 c| + |v2 s|); float64's own
rounding of r (2^-52 of the same sum) is added to d.  The admissible outputs are the bf16 values in
[bf16(r - d), bf16(r + d)]; an element is *decided* when that is one value, and must then match it; an undecided one
must lie in the interval.  K in an fp8 cache: the e4m3 values in [e4m3_sat(lo), e4m3_sat(hi)] (e4m3_sat is monotone
and every e4m3 value is a bf16 value, so these are exactly the images of the admissible bf16 values).  V is not
rotated and is exact: bf16(fp32(w + b)), or e4m3_sat of it.  Equality is by value (+0 = -0: the sign of a zero that
went through a sum of signed zeros depends on the order).  Everything no live row owns keeps the sentinel -7.

Planted faults (``qkv_mirror``, a host statement of the epilogue's arithmetic in fp32); ``qkv_check`` must report
each at every geometry where it can show (``QKV_FAULT_SHOWS``, checked by tests/test_epilogue_values_cpu.py):

    fault                                              bf16 cache          fp8 cache
    nobf16   no bf16 rounding before the rotation      caught              caught
    pos1     cos / sin of position p + 1               caught              caught
    sinflip  sin's sign flipped on the second half     caught              caught
    vnosat   the V line without saturation (NaN code)  cannot show         caught
    trunc    e4m3 by truncation, not RNE               cannot show         caught

at phi3's, the GQA and gemma's head shape alike (none of the five depends on the geometry).

SiLU / GeGLU per element (``act_ref`` / ``act_check``): r = act(g) u in float64, |got - r| <= half a bf16 step of
r + E.  E from the instructions of common.h, with u24 = 2^-24 (half an fp32 ulp: one correctly rounded operation),
v_exp_f32 and v_rcp_f32 at 1 ulp = 2 u24, sig(x) = 1 / (1 + e^-x):

* silu_f(g) = g rcp(1 + exp2(-g log2e)).  The exponent -g log2e carries the rounded constant and one product,
  1.5 u24 relative, i.e. 1.5 |g| u24 relative on e = e^-g; v_exp_f32 adds 2 u24.  In 1 + e that error weighs
  e / (1 + e) = sig(-g); the sum rounds (u24), v_rcp_f32 (2 u24), g times it (u24), times up (u24):
      E_silu = |r| u24 ((1.5 |g| + 2) sig(-g) + 5).
* gelu_tanh_f(g) = 0.5 g (1 + t), t = 1 - 2 rcp(exp(2 y) + 1), y = k0 (g + k1 g^3): y carries two rounded constants
  and four operations, 6 u24; x = 2 y, so e^x carries rho_e = |x| (1.5 + 6) u24 + 2 u24.  q = 2 rcp(e^x + 1) carries
  rho_q = rho_e sig(x) + 3 u24; t = 1 - q and s = 1 + t round absolutely (u24 |t|, u24 |s|), and q's *absolute*
  error q rho_q stays in s however small s = 2 sig(x) becomes -- the cancellation.  0.5 g s rounds, times up rounds:
      E_gelu = 0.5 |g u| (q rho_q + u24 (|t| + |s|)) + 2 u24 |r|,  an absolute term of a few 2^-24 |g u|.
* with the fused RMSNorm both g and u arrive with the factor's relative error rho_n (below); it adds
  rho_n (|g act'(g) u| + |r|).
Where E / |r| exceeds 2^-12 the element is left out (``checked`` is False): GeLU gates below about -2.6, where the
cancellation rules.  Gates with |g| >= 88 are the extremes: e^-g over- or underflows, act(g) is g (then
got = bf16(g u), one exact product) or below 1e-35 in magnitude; both are held to 1e-30, and every output must be
finite.  The dense grids stay inside |g| <= 80, where no intermediate is a denormal; a gate between 80 and 88 (the
quantised families' products and the fused norm's factor put some there) is left out like the cancelling ones:
e^-g nears 2^126 there and v_rcp_f32 flushes a denormal result, which E does not state.

Fused RMSNorm factor (``norm_case`` / ``norm_check``): rows of 1 to 4 non-zero integers, so the sum of squares is an
exact integer on every path; the weight is zero outside the row's one delivering column.  Reference
a W[n, k] / sqrt(ss / K + eps) in float64.  rms_inv = v_rsq_f32(ss v_rcp_f32(K) + eps): the reciprocal (2 u24), the
product and the sum (u24 each) halve under the square root, v_rsq_f32 adds 2 u24, the accumulator times the factor
u24: rho_n = 5 u24; the activation-quantised pair multiplies the factor into the row scale and that into the
accumulator, 2 u24 more.  fp32 outputs: |got - r| <= rho_n |r|; bf16 outputs: the admissible set
[bf16(r (1 - rho_n)), bf16(r (1 + rho_n))] as above.
"""
from __future__ import annotations

import sys
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import exact  # noqa: E402
from cain_amd.models.weights import interleave_tiles, pack_mfma_a  # noqa: E402

U24 = 2.0 ** -24
T_MAX = 64
#: the models' head shapes (exact.QKV_GEOS) with T_max = 64
GEOS: Dict[str, exact.Geo] = {k: (g[0], g[1], g[2], T_MAX) for k, g in exact.QKV_GEOS.items()}
SENT = -7.0
SENT8 = 0xCE  # -7.0 as an e4m3 byte
BF16_MAX = float(torch.finfo(torch.bfloat16).max)
A8 = ("w8a8", "w4a8")
QUANT = ("w8", "w4", "q4_0", "q4_k", "q6", "w8a8", "w4a8")


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(int(seed))


# ---------------------------------------------------------------- bf16 and e4m3, written out
def bf16_rne(v: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest bf16 value (as float64), ties to even, past the largest finite value to infinity;
    written out from the format (8 significant bits, smallest normal 2^-126), one rounding."""
    v = v.double()
    a = v.abs()
    e = (torch.frexp(a)[1] - 1).clamp(min=-126, max=127)
    step = torch.pow(2.0, (e - 7).double())
    r = torch.round(a / step) * step
    r = torch.where(r > BF16_MAX, torch.full_like(r, float("inf")), r)
    r = torch.where(a.isnan(), a, r)
    return torch.copysign(r, v)


def half_step(r: torch.Tensor) -> torch.Tensor:
    """Half a bf16 step at r."""
    e = (torch.frexp(r.double().abs())[1] - 1).clamp(min=-126, max=127)
    return torch.pow(2.0, (e - 8).double())


def is_bf16(v: torch.Tensor) -> torch.Tensor:
    return v.double().bfloat16().double() == v.double()


def bf16_neighbours(a: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The bf16 values just below and above the positive bf16 values ``a``."""
    assert bool(is_bf16(a).all()) and float(a.min()) > 0
    i = exact.bits16(a.bfloat16())
    back = lambda j: j.to(torch.int16).view(torch.bfloat16).double()  # noqa: E731
    return back(i - 1), back(i + 1)


def e4m3_sat(v: torch.Tensor) -> torch.Tensor:
    """exact.e4m3_quant: nearest e4m3 value, ties to even, saturating at +-448; NaN stays NaN."""
    return torch.where(v.isnan(), v.double(), exact.e4m3_quant(torch.nan_to_num(v.double(), nan=0.0)))


def e4m3_trunc(v: torch.Tensor) -> torch.Tensor:
    """The planted wrong conversion: towards zero."""
    a = v.double().abs().clamp(max=exact.E4M3_MAX)
    e = (torch.frexp(a)[1] - 1).clamp(min=-6)
    step = torch.pow(2.0, (e - 3).double())
    return torch.copysign(torch.floor(a / step) * step, v.double())


# ---------------------------------------------------------------- value sets
def e4m3_finite() -> torch.Tensor:
    """The 127 non-negative finite e4m3 values, 0 .. 448."""
    return torch.arange(0, 127, dtype=torch.uint8).view(torch.float8_e4m3fn).double()


def e4m3_ties() -> torch.Tensor:
    """The midpoints of adjacent e4m3 values -- 2^-10 (ties to zero) first -- and 464, the tie above 448."""
    v = e4m3_finite()
    return torch.cat([(v[1:] + v[:-1]) / 2, torch.tensor([464.0], dtype=torch.float64)])


def value_classes(cap: Optional[float] = None) -> Dict[str, torch.Tensor]:
    """Magnitudes of the value set by class, all exact in bf16; ``cap``: only magnitudes below it."""
    ties = e4m3_ties()
    lo, hi = bf16_neighbours(ties)
    out = {"e4m3": e4m3_finite()[1:], "tie": ties, "neighbour": torch.cat([lo, hi]),
           "extreme": torch.tensor([448.0, 480.0, float(torch.tensor(1e4).bfloat16()), BF16_MAX], dtype=torch.float64),
           "zero": torch.zeros(1, dtype=torch.float64)}
    for k, v in out.items():
        assert bool(is_bf16(v).all()), k
        if cap is not None:
            out[k] = v[v < cap]
    return out


def value_set(cap: Optional[float] = None) -> torch.Tensor:
    """Every magnitude of ``value_classes`` with both signs (so +0 and -0), unique."""
    m = torch.unique(torch.cat(list(value_classes(cap).values())))
    return torch.cat([m, -m])


def reach(values: torch.Tensor, cap: Optional[float] = None) -> Dict[str, Tuple[int, int]]:
    """class -> (signed members that occur in ``values``, signed members) -- what a case's epilogue inputs cover."""
    have = set(values.double().flatten().tolist())
    out = {}
    for k, m in value_classes(cap).items():
        signed = torch.cat([m, -m]).tolist() if k != "zero" else [0.0]
        out[k] = (sum(1 for t in signed if t in have), len(signed))
    return out


def rand_bf16(g: torch.Generator, shape) -> torch.Tensor:
    """Random bf16 values (float64), randn over the binades 2^-4 .. 2^6, magnitudes of at least 2^-8 (their lowest
    bit then stays above 2^-24, what an fp16 slab holds)."""
    e = torch.randint(-4, 7, shape, generator=g).double()
    v = (torch.randn(shape, generator=g).double() * torch.pow(2.0, e)).bfloat16().double()
    return torch.copysign(v.abs().clamp(min=2.0 ** -8), v)


# ---------------------------------------------------------------- RoPE tables and rows
def rope_tables(hd: int, T: int = T_MAX):
    """fp32 cos, sin [T, hd / 2] of the engine's angles (models/config.py rope_inv_freq, theta 1e4)."""
    from cain_amd.models.config import ModelConfig, rope_inv_freq
    cfg = ModelConfig(name="t", display_name="t", n_layers=1, d_model=hd, n_heads=1, n_kv_heads=1, head_dim=hd, ffn=16,
                      vocab=16, rope_theta=10000.0)
    ang = torch.arange(T, dtype=torch.float64)[:, None] * torch.tensor(rope_inv_freq(cfg), dtype=torch.float64)
    return torch.cos(ang).float().contiguous(), torch.sin(ang).float().contiguous()


def rows(M: int, seed: int, T: int = T_MAX):
    """(slot, pos, S): ``exact.qkv_rows`` (idle rows, five rows sharing a slot, position T - 1) with one further live
    row moved to position 0; below 8 rows: row m in slot m at positions T - 1, 0, 1, ..."""
    if M < 8:
        return torch.arange(M, dtype=torch.int32), torch.tensor([(T - 1 + m) % T for m in range(M)], dtype=torch.int32), M + 2
    slot, pos, S = exact.qkv_rows(M, T, seed)
    owned = {(int(s), int(p)) for s, p in zip(slot, pos) if s >= 0}
    for m in range(M):
        s, p = int(slot[m]), int(pos[m])
        if s >= 0 and p not in (15, 16, 31, 32, T - 1) and (s, 0) not in owned:
            pos[m] = 0
            break
    else:  # pragma: no cover
        raise AssertionError("no row could move to position 0")
    return slot, pos, S


# ---------------------------------------------------------------- cases: what the kernel is given
@dataclass
class Delivered:
    """One launch's operands and what they deliver: ``packed`` (the kernel's weight operands), x fp64 [M, K] (exact
    in bf16), acc fp64 [M, N] = x @ W^T exactly (kernel row order), w fp64 [N, K] the decoded weights."""
    fam: str
    packed: Dict[str, torch.Tensor]
    x: torch.Tensor
    acc: torch.Tensor
    w: torch.Tensor

    def __post_init__(self):
        assert bool(is_bf16(self.x).all()), "activations must be exact in bf16"
        assert int((self.x != 0).sum(1).max()) <= 4
        assert bool((self.acc.float().double() == self.acc).all()), "a delivered value is no fp32 number"


def _columns(M: int, K: int, g: torch.Generator) -> torch.Tensor:
    """One column per row, distinct, over the whole of K (so over every k slice, wave and split range in turn)."""
    assert M <= K
    return torch.randperm(K, generator=g)[:M]


def one_hot(M: int, K: int, cols: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    x = torch.zeros(M, K, dtype=torch.float64)
    x[torch.arange(M), cols] = a.double()
    return x


def qkv_bias(N: int) -> torch.Tensor:
    """fp32 bias: zero on three columns in four, else one of a few values -- halves, a tie-maker, 1 / 3."""
    b = torch.zeros(N, dtype=torch.float32)
    vals = torch.tensor([0.5, -3.0, 2.0 ** -10, -17.25, 1.0 / 3.0, -2.0 ** -7, 464.0, -0.0625], dtype=torch.float32)
    idx = torch.arange(1, N, 4)
    b[idx] = vals[(idx // 4) % len(vals)]
    return b


def qkv_bf16_case(geo_name: str, M: int, K: int, seed: int, cap: Optional[float] = None):
    """bf16 weights for the fused QKV epilogue.  Row m is one-hot at its own column, and that column of W holds: on
    the V rows the value set, cycling through a shuffle of it; on the q / k rows a quarter value set (without the
    largest bf16), the rest random bf16 -- all value set on a row at position 0, where the rotation is the identity
    and K receives the values themselves.  Where the bias b is non-zero the weight is bf16(t - b), so that many sums
    fp32(w + b) land on the targets t, ties included.  The other columns hold random bf16 values (they meet zeros).
    Returns (Delivered, bias fp32 [N], slot, pos, S)."""
    H, Hkv, hd, T = GEOS[geo_name]
    N = exact.qkv_n(GEOS[geo_name])
    g = _gen(seed)
    slot, pos, S = rows(M, seed, T)
    cols = _columns(M, K, g)
    bias = qkv_bias(N)
    full = value_set(cap)
    rot = full[full.abs() < 2.0 ** 14]
    nrot = (H + Hkv) * hd
    W = rand_bf16(g, (N, K))
    order, ctr = full[torch.randperm(len(full), generator=g)], 0
    for m in range(M):
        t = rand_bf16(g, (N,))
        pick = torch.rand(nrot, generator=g) < (1.0 if int(pos[m]) == 0 and int(slot[m]) >= 0 else 0.25)
        t[:nrot] = torch.where(pick, rot[(torch.randperm(nrot, generator=g) + 131 * m) % len(rot)], t[:nrot])
        tv = full[torch.randint(0, len(full), (N - nrot,), generator=g)]
        if int(slot[m]) >= 0:  # the unbiased V columns of the live rows walk through the whole shuffled set in turn
            free = (bias[nrot:] == 0).nonzero().flatten()
            tv[free] = order[(ctr + torch.arange(len(free))) % len(full)]
            ctr += len(free)
        t[nrot:] = tv
        W[:, cols[m]] = bf16_rne(t - bias.double())
    W = torch.where(W.isinf(), torch.copysign(torch.tensor(BF16_MAX, dtype=torch.float64), W), W)
    x = one_hot(M, K, cols, torch.ones(M))
    d = Delivered("bf16", {"wp": pack_mfma_a(W.bfloat16())}, x, x @ W.t(), W)
    return d, bias, slot, pos, S


#: activation exponents of the quantised families, cycled over the rows: a = 2^e (448 2^e on the a8 pair)
Q_EXPS = {"w8": range(-13, 7), "w4": range(-12, 9), "q4_0": range(-13, 8), "q4_k": range(-16, 5), "q6": range(-18, 4),
          "w8a8": range(-22, 0), "w4a8": range(-21, 1)}


def quant_weights(fam: str, N: int, K: int, seed: int, gateup: bool = False) -> exact.Weights:
    kw = {"amp": 16} if fam in ("w8", "w8a8") else {}
    if gateup:
        kw["gateup"] = True
    return exact.GENERATORS[fam](N, K, seed, **kw)


def quant_case(fam: str, N: int, K: int, M: int, seed: int, gateup: bool = False, exps=None) -> Delivered:
    """A quantised family: the integer weights of ``exact.GENERATORS`` (every code of the format), rows one-hot with
    a = 2^e (448 2^e for the activation-quantised pair), e striding over ``Q_EXPS`` -- so the delivered values are
    (decoded weight) x a, exact: a power of two times an integer below 2^24 (``exact.product`` checks the bounds)."""
    g = _gen(seed)
    ew = quant_weights(fam, N, K, seed + 1, gateup)
    cols = _columns(M, K, g)
    unit = one_hot(M, K, cols, torch.ones(M))
    exact.product((unit * (448 if fam in A8 else 2)).long(), ew)  # the generators' fp32 bounds (2: MXFP4's halves)
    es = list(Q_EXPS[fam] if exps is None else exps)
    import math
    stride = next(st for st in (8, 7, 5, 3, 1) if math.gcd(st, len(es)) == 1)  # few rows still span the whole list
    e = torch.tensor([es[(stride * m + seed) % len(es)] for m in range(M)], dtype=torch.float64)
    a = torch.pow(2.0, e) * (448.0 if fam in A8 else 1.0)
    x = one_hot(M, K, cols, a)
    w = ew.w.double() / ew.den
    return Delivered(fam, ew.packed, x, x @ w.t(), w)


def delivery_exact(d: Delivered, ranges: Optional[List[Tuple[int, int]]] = None, slab: str = "f32") -> Optional[str]:
    """The host mirror of a path's intermediate formats (module doc): None when every k range's partial of every
    element survives its slab format and their fp32 sum is the delivered value; else what breaks.  ``slab``: "f32",
    "f16exp" (wgemm.hip variant 0: per four columns of a row, scaled by a power of two) or "f16" (wgemm8.hip)."""
    M, K = d.x.shape
    total = torch.zeros_like(d.acc, dtype=torch.float32)
    for k0, k1 in (ranges or [(0, K)]):
        p = d.x[:, k0:k1] @ d.w[:, k0:k1].t()
        if bool((p.float().double() != p).any()):
            return f"k range {k0}..{k1}: a partial is no fp32 number"
        if slab != "f32":
            ex = torch.zeros_like(p)
            if slab == "f16exp":
                mx = p.abs().view(M, -1, 4).amax(-1)
                ex = (torch.frexp(mx)[1] - 14).clamp(min=0).double().repeat_interleave(4, 1)
            s = (p * torch.pow(2.0, -ex)).clamp(-65504.0, 65504.0)
            bad = (s.half().double() != s) | (s * torch.pow(2.0, ex) != p)
            if bool(bad.any()):
                r, c = (int(v) for v in bad.nonzero()[0])
                return f"k range {k0}..{k1}: row {r}, column {c}: {float(p[r, c])!r} x 2^-{int(ex[r, c])} is no fp16 number"
            p = s.half().double() * torch.pow(2.0, ex)
        total = total + p.float()
    if bool((total.double() != d.acc).any()):
        return "the fp32 sum of the partials is not the delivered value"
    return None


# ---------------------------------------------------------------- fused QKV: reference, comparator, planted faults
def _natural(t: torch.Tensor, geo: exact.Geo) -> torch.Tensor:
    """Kernel row order -> natural order on the last dim."""
    perm = exact.qkv_perm(*geo[:3])
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel())
    return t[..., inv]


def _split_heads(v: torch.Tensor, geo: exact.Geo):
    H, Hkv, hd, _ = geo
    M = v.shape[0]
    return (v[:, : H * hd].view(M, H, hd), v[:, H * hd:(H + Hkv) * hd].view(M, Hkv, hd), v[:, (H + Hkv) * hd:].view(M, Hkv, hd))


def qkv_want(acc: torch.Tensor, bias: torch.Tensor, slot, pos, cos, sin, geo: exact.Geo, S: int, kv8: bool):
    """What a launch may leave behind (module doc): dict of lo / hi bounds for q [M, H hd] and the natural-order
    K cache [S, Hkv, T, hd], the exact V cache, the float64 r and d of q and K (for the reported error), and owner
    [S, T] (-1: nobody).  Unowned elements and idle rows' q hold the sentinel in lo and hi."""
    H, Hkv, hd, T = geo
    M = acc.shape[0]
    v = _natural((acc.float() + bias.float()[None, :]).bfloat16().double(), geo)
    vq, vk, vv = _split_heads(v, geo)
    c, s = cos[pos.long()].double()[:, None], sin[pos.long()].double()[:, None]
    half = hd // 2

    def rotate(t):
        a, b = t[..., :half], t[..., half:]
        r = torch.cat([a * c - b * s, b * c + a * s], -1)
        mag = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], -1)
        return r, (3 * U24 + 2.0 ** -50) * mag

    rq, dq = rotate(vq)
    rk, dk = rotate(vk)
    live = slot >= 0
    sq = lambda t: torch.where(live[:, None], t.reshape(M, H * hd), torch.full((M, H * hd), SENT, dtype=torch.float64))  # noqa: E731
    want = {"q_lo": sq(bf16_rne(rq - dq)), "q_hi": sq(bf16_rne(rq + dq)), "q_r": rq.reshape(M, H * hd),
            "q_d": dq.reshape(M, H * hd), "live": live}
    full = lambda val: torch.full((S, Hkv, T, hd), val, dtype=torch.float64)  # noqa: E731
    for k in ("k_lo", "k_hi", "v"):
        want[k] = full(SENT)
    want["k_r"], want["k_d"] = full(0.0), full(0.0)
    owner = torch.full((S, T), -1, dtype=torch.long)
    cache = e4m3_sat if kv8 else (lambda t: t)
    for m in range(M):
        sl, ps = int(slot[m]), int(pos[m])
        if sl < 0:
            continue
        assert int(owner[sl, ps]) == -1
        owner[sl, ps] = m
        want["k_lo"][sl, :, ps] = cache(bf16_rne(rk[m] - dk[m]))
        want["k_hi"][sl, :, ps] = cache(bf16_rne(rk[m] + dk[m]))
        want["k_r"][sl, :, ps], want["k_d"][sl, :, ps] = rk[m], dk[m]
        want["v"][sl, :, ps] = cache(vv[m])
    want["owner"], want["kv8"] = owner, kv8
    return want


@dataclass
class Stats:
    decided: int = 0
    undecided: int = 0
    exact: int = 0       # elements compared for equality outright (V; sentinels)
    worst: float = 0.0   # the worst error in units of its bound
    skipped: int = 0

    def line(self, tag: str) -> str:
        return (f"{tag}: decided {self.decided}, undecided {self.undecided}, exact {self.exact}, skipped {self.skipped}, "
                f"worst error {self.worst:.3f} of the bound")


def _interval(name: str, got: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, st: Stats, counted: torch.Tensor,
              out: List[str]) -> None:
    g = got.detach().cpu().double()
    dec = lo == hi
    st.decided += int((dec & counted).sum())
    st.undecided += int((~dec & counted).sum())
    st.exact += int((~counted).sum())
    bad = ~((g >= lo) & (g <= hi))
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        out.append(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside their admissible set "
                   f"({int((bad & dec).sum())} of them decided); first at {i}: got {float(g[i])!r}, "
                   f"admissible [{float(lo[i])!r}, {float(hi[i])!r}]")


def qkv_check(q: torch.Tensor, kn: torch.Tensor, vn: torch.Tensor, want) -> Tuple[Stats, Optional[str]]:
    """q [M, H hd] and the unpacked caches [S, Hkv, T, hd] (as numbers) against ``qkv_want``: (Stats, report or
    None).  ``worst``: max |got - r| / (d + half a bf16 step of r) over q (and K in a bf16 cache)."""
    st, out = Stats(), []
    live = want["live"][:, None].expand_as(want["q_lo"])
    own = (want["owner"] >= 0)[:, None, :, None].expand_as(want["v"])
    _interval("q", q, want["q_lo"], want["q_hi"], st, live, out)
    _interval("K cache", kn, want["k_lo"], want["k_hi"], st, own, out)
    g = vn.detach().cpu().double()
    bad = ~(g == want["v"])
    st.exact += g.numel()
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        out.append(f"V cache: {int(bad.sum())} elements differ; first at (slot, head, position, dim) {i}, "
                   f"{'row ' + str(int(want['owner'][i[0], i[2]])) if want['owner'][i[0], i[2]] >= 0 else 'no row'} writes "
                   f"there: got {float(g[i])!r}, want {float(want['v'][i])!r}")
    pairs = [(q, want["q_r"], want["q_d"], live)] + ([] if want["kv8"] else [(kn, want["k_r"], want["k_d"], own)])
    for got, r, d, mask in pairs:
        e = (got.detach().cpu().double() - r).abs() / (d + half_step(r))
        e = torch.where(mask, torch.nan_to_num(e, nan=float("inf")), torch.zeros_like(e))
        st.worst = max(st.worst, float(e.max()))
    return st, "; ".join(out) if out else None


QKV_FAULTS = ("nobf16", "pos1", "sinflip", "vnosat", "trunc")
#: (fault, fp8 cache?) -> must ``qkv_check`` report it (at every geometry: module doc)
QKV_FAULT_SHOWS = {(f, kv8): (kv8 or f in ("nobf16", "pos1", "sinflip")) for f in QKV_FAULTS for kv8 in (False, True)}


def qkv_mirror(acc, bias, slot, pos, cos, sin, geo: exact.Geo, S: int, kv8: bool, fault: Optional[str] = None):
    """The epilogue's arithmetic on the host in fp32 (separately rounded products and sum), straight into natural
    order: (q [M, H hd], K, V [S, Hkv, T, hd]) as float64 numbers, sentinel where nothing is written.  ``fault``:
    one of QKV_FAULTS planted."""
    assert fault is None or fault in QKV_FAULTS
    H, Hkv, hd, T = geo
    M = acc.shape[0]
    s32 = acc.float() + bias.float()[None, :]
    v = _natural(s32 if fault == "nobf16" else s32.bfloat16().float(), geo)
    vq, vk, vv = _split_heads(v, geo)
    p = (pos.long() + 1) % T if fault == "pos1" else pos.long()
    c, s = cos[p][:, None], sin[p][:, None]
    half = hd // 2

    def rotate(t):
        a, b = t[..., :half], t[..., half:]
        y2 = (b * c - a * s) if fault == "sinflip" else (b * c + a * s)
        return torch.cat([a * c - b * s, y2], -1).bfloat16().double()

    def cache(t):
        t = t.double()
        if not kv8:
            return t
        return e4m3_trunc(t) if fault == "trunc" else e4m3_sat(t)

    def vcache(t):
        t = t.double()
        if kv8 and fault == "vnosat":  # past the tie above 448 the unsaturated conversion gives the NaN code
            return torch.where(t.abs() >= 464.0, torch.full_like(t, float("nan")), e4m3_sat(t))
        return cache(t)

    yq, yk, yv = rotate(vq).reshape(M, H * hd), rotate(vk), vv.bfloat16()
    q = torch.full((M, H * hd), SENT, dtype=torch.float64)
    K = torch.full((S, Hkv, T, hd), SENT, dtype=torch.float64)
    V = K.clone()
    for m in range(M):
        sl, ps = int(slot[m]), int(pos[m])
        if sl < 0:
            continue
        q[m] = yq[m]
        K[sl, :, ps] = cache(yk[m])
        V[sl, :, ps] = vcache(yv[m])
    return q, K, V


# ---------------------------------------------------------------- SiLU / GeGLU
GATE_EXTREMES = (88.0, 89.0, 100.0, 1e4, BF16_MAX)
K0, K1 = 0.7978845608028654, 0.044715


def gate_grid() -> torch.Tensor:
    """bf16 gates over [-80, 80], dense around 0: two linear grids and the powers of two down to 2^-12."""
    p = torch.pow(2.0, torch.arange(-12, 7).double())
    g = torch.cat([torch.linspace(-80, 80, 321, dtype=torch.float64), torch.linspace(-8, 8, 513, dtype=torch.float64),
                   torch.linspace(-1, 1, 257, dtype=torch.float64), p, -p])
    g = torch.unique(g.bfloat16().double())
    return g[g.abs() <= 80]


def split_gateup(acc: torch.Tensor):
    """Interleaved projection [M, 2F] -> (gate, up) [M, F] (8 gate rows, then their 8 up rows, per 16-row tile)."""
    M, n = acc.shape
    hh = acc.view(M, n // 16, 2, 8)
    return hh[:, :, 0].reshape(M, n // 2), hh[:, :, 1].reshape(M, n // 2)


def act_f(g: torch.Tensor, kind: str) -> torch.Tensor:
    if kind == "silu":
        return g * torch.sigmoid(g)
    return g * torch.sigmoid(2.0 * K0 * (g + K1 * g * g * g))  # 0.5 g (1 + tanh y) = g sig(2 y)


def act_ref(g: torch.Tensor, u: torch.Tensor, kind: str, rho_in: float = 0.0):
    """float64 gate and up values as the epilogue receives them (to a relative ``rho_in``) -> dict: r = act(g) u, the
    derived E (module doc), ``checked`` (E / |r| <= 2^-12 and |g| <= 80), ``pos`` / ``neg`` (the extremes)."""
    g, u = g.double(), u.double()
    gg = g.clone().requires_grad_(True)
    a = act_f(gg, kind)
    da, = torch.autograd.grad(a.sum(), gg)
    a, r = a.detach(), a.detach() * u
    if kind == "silu":
        E = r.abs() * U24 * ((1.5 * g.abs() + 2) * torch.sigmoid(-g) + 5)
    else:
        x = 2.0 * K0 * (g + K1 * g * g * g)
        sg = torch.sigmoid(x)
        q, s = 2.0 * torch.sigmoid(-x), 2.0 * sg
        rho_q = (x.abs() * 7.5 * U24 + 2 * U24) * sg + 3 * U24
        E = 0.5 * (g * u).abs() * (q * rho_q + U24 * ((1.0 - q).abs() + s)) + 2 * U24 * r.abs()
    E = E + rho_in * ((g * da * u).abs() + r.abs())
    ext = g.abs() >= 88.0
    tiny = torch.tensor(torch.finfo(torch.float64).tiny, dtype=torch.float64)
    inner = g.abs() <= 80.0  # between 80 and 88 v_rcp_f32's result nears the denormals, which E does not cover
    checked = inner & (E <= 2.0 ** -12 * torch.maximum(r.abs(), tiny)) | (inner & (r == 0) & (E == 0))
    return {"r": r, "E": E, "checked": checked, "pos": ext & (g > 0), "neg": ext & (g < 0), "g": g, "u": u}


def act_check(got: torch.Tensor, ref) -> Tuple[Stats, Optional[str]]:
    """bf16 outputs [M, F] against ``act_ref``: every element finite; checked ones within half a bf16 step of r + E;
    positive extremes equal to bf16(g u) and negative ones within 1e-30 of r (both: |got - r| <= 1e-30 when up is
    +-1)."""
    y = got.detach().cpu().double()
    st, out = Stats(), []
    if not bool(y.isfinite().all()):
        i = tuple(int(v) for v in (~y.isfinite()).nonzero()[0])
        out.append(f"{int((~y.isfinite()).sum())} outputs not finite; first at {i}: gate {float(ref['g'][i])!r}, "
                   f"up {float(ref['u'][i])!r}")
        y = torch.nan_to_num(y, nan=float("inf"))
    bound = half_step(ref["r"]) + ref["E"]
    e = (y - ref["r"]).abs() / bound
    c = ref["checked"]
    st.decided, st.skipped = int(c.sum()), int((~c & ~ref["pos"] & ~ref["neg"]).sum())
    st.exact = int((ref["pos"] | ref["neg"]).sum())
    if st.decided:
        st.worst = float(e[c].max())
    bad = c & ~(e <= 1.0)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        out.append(f"{int(bad.sum())} of {int(c.sum())} elements past their bound; first at (row, column) {i}: gate "
                   f"{float(ref['g'][i])!r}, up {float(ref['u'][i])!r}: got {float(y[i])!r}, want {float(ref['r'][i])!r}, "
                   f"{float(e[i]):.2f} x the bound")
    want_pos = bf16_rne(ref["g"] * ref["u"])
    bad = (ref["pos"] & ~((y - want_pos).abs() <= 1e-30)) | (ref["neg"] & ~((y - ref["r"]).abs() <= 1e-30))
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        out.append(f"{int(bad.sum())} extreme gates wrong; first at (row, column) {i}: gate {float(ref['g'][i])!r}, "
                   f"up {float(ref['u'][i])!r}: got {float(y[i])!r}, want {float(ref['r'][i])!r}")
    return st, "; ".join(out) if out else None


def norm_factor(x: torch.Tensor, eps: float) -> torch.Tensor:
    """float64 1 / sqrt(sum x^2 / K + eps) per row, [M, 1]."""
    return torch.rsqrt(x.double().pow(2).sum(1, keepdim=True) / x.shape[1] + eps)


RHO_NORM = 5 * U24
RHO_NORM_A8 = 7 * U24
EPS = 1e-6


def rho_norm(fam: str) -> float:
    return RHO_NORM_A8 if fam in A8 else RHO_NORM


def act_bf16_case(kind: str, F: int, K: int, M: int, seed: int, norm: bool) -> Delivered:
    """bf16 gate/up weights through ``interleave_tiles(tile=8)``: row m one-hot (a = 1), its column holding the gate
    grid (shuffled, cycling; with ``norm`` divided by the row's RMSNorm factor, so the epilogue sees the grid's range)
    against random bf16 up values in +-[1/4, 4], and in the last 2 x len(GATE_EXTREMES) x 2 places of each row the
    extreme gates, both signs, against up = +1 and -1."""
    g = _gen(seed)
    cols = _columns(M, K, g)
    x = one_hot(M, K, cols, torch.ones(M))
    scale = float(norm_factor(x[:1], EPS)) if norm else 1.0
    grid = gate_grid()
    ext = torch.tensor([s * e for e in GATE_EXTREMES for s in (1.0, -1.0)], dtype=torch.float64).bfloat16().double()
    ext_g, ext_u = ext.repeat_interleave(2), torch.tensor([1.0, -1.0], dtype=torch.float64).repeat(len(ext))
    ne = len(ext_g)
    assert F > 2 * ne
    Wg, Wu = rand_bf16(g, (F, K)), rand_bf16(g, (F, K))
    for m in range(M):
        gs = (grid[(torch.randperm(len(grid), generator=g)[torch.arange(F) % len(grid)] + m) % len(grid)] / scale)
        us = torch.pow(2.0, torch.rand(F, generator=g).double() * 4 - 2) * (torch.randint(0, 2, (F,), generator=g) * 2 - 1)
        gs, us = gs.bfloat16().double(), us.bfloat16().double()
        if not norm:  # with the norm the factor would scale the extremes past the largest bf16: grid only
            gs[F - ne:], us[F - ne:] = ext_g, ext_u
        Wg[:, cols[m]], Wu[:, cols[m]] = gs, us
    W = interleave_tiles(Wg, Wu, tile=8)
    return Delivered("bf16", {"wp": pack_mfma_a(W.bfloat16())}, x, x @ W.t(), W)


def act_case_ref(d: Delivered, kind: str, norm: bool):
    """``act_ref`` of a delivered gate/up case (``norm``: through the fused RMSNorm factor in float64)."""
    f = norm_factor(d.x, EPS) if norm else 1.0
    g, u = split_gateup(d.acc * f)
    return act_ref(g, u, kind, rho_norm(d.fam) if norm else 0.0)


# ---------------------------------------------------------------- fused RMSNorm factor
def norm_case(fam: str, N: int, K: int, M: int, seed: int, ranges: Optional[List[Tuple[int, int]]] = None) -> Delivered:
    """Rows of 1 to 4 non-zero integers (row m: 1 + m % 4 of them), one per k range of ``ranges`` in turn (default:
    quarters of K), the first of them the delivering column: the weight (bf16: random values; quantised: the
    generator's) is zero in every other column a row touches, so acc = a W[:, k] and the sum of squares is an exact
    integer.  On the activation-quantised pair the delivering value is 448 and the others multiples of 64."""
    g = _gen(seed)
    ranges = ranges or [(i * K // 4, (i + 1) * K // 4) for i in range(4)]
    a8 = fam in A8
    if fam == "bf16":
        w = rand_bf16(g, (N, K))
        packed = None
    else:
        ew = quant_weights(fam, N, K, seed + 1)
        w = ew.w.double() / ew.den
        packed = ew.packed
    x = torch.zeros(M, K, dtype=torch.float64)
    dead = []
    # per k range: the first three quarters hold delivering columns (one row each), the last quarter the other
    # non-zeros (shared between rows; the bf16 weight is zero there)
    assert M <= 3 * K // 4 - 4 * len(ranges)
    free = [torch.randperm(k1 - k0 - (k1 - k0) // 4, generator=g).add(k0).tolist() for k0, k1 in ranges]
    for m in range(M):
        for i in range(1 + m % 4):
            ri = (m + i) % len(ranges)
            k0, k1 = ranges[ri]
            val = float(int(torch.randint(1, 5, (1,), generator=g)))
            if i == 0:
                while not free[ri]:
                    ri = (ri + 1) % len(ranges)
                x[m, free[ri].pop()] = 448.0 if a8 else val
            else:
                k = int(torch.randint(k1 - (k1 - k0) // 4, k1, (1,), generator=g))
                x[m, k] += (64.0 if a8 else 1.0) * val * (1 if i % 2 else -1)
                dead.append(k)
    x = torch.where(x == 0, torch.zeros_like(x), x)
    if fam == "bf16":
        w[:, dead] = 0.0
        packed = {"wp": pack_mfma_a(w.bfloat16())}
        return Delivered(fam, packed, x, x @ w.t(), w)
    # a quantised weight cannot be zeroed after packing: the reference keeps every term (all exact integers)
    return Delivered(fam, packed, x, x @ w.t(), w)


def norm_check(got: torch.Tensor, d: Delivered, rho: float) -> Tuple[Stats, Optional[str]]:
    """fp32 outputs: |got - r| <= rho |r|; bf16 outputs: inside [bf16(r (1 - rho)), bf16(r (1 + rho))]."""
    r = d.acc * norm_factor(d.x, EPS)
    st, out = Stats(), []
    y = got.detach().cpu().double()
    if got.dtype == torch.float32:
        inf = torch.full_like(r, float("inf"))
        e = torch.where(r == 0, torch.where(y != 0, inf, torch.zeros_like(r)), (y - r).abs() / (rho * r.abs()).clamp(min=1e-300))
        e = torch.nan_to_num(e, nan=float("inf"))
        st.decided, st.worst = r.numel(), float(e.max())
        if st.worst > 1.0:
            i = tuple(int(v) for v in (e > 1.0).nonzero()[0])
            out.append(f"{int((e > 1.0).sum())} elements past {rho / U24:.0f} x 2^-24; first at {i}: got {float(y[i])!r}, "
                       f"want {float(r[i])!r} ({float(e[i]):.2f} x the bound)")
    else:
        lo, hi = bf16_rne(r - rho * r.abs()), bf16_rne(r + rho * r.abs())
        _interval("bf16 output", got, lo, hi, st, torch.ones_like(r, dtype=torch.bool), out)
        e = (y - r).abs() / (rho * r.abs() + half_step(r))
        st.worst = float(torch.nan_to_num(e, nan=float("inf")).max())
    return st, "; ".join(out) if out else None


# ---------------------------------------------------------------- the GPU file's cases
@dataclass(frozen=True)
class Path_:
    """One kernel path: family, tag, rows, K, and for the wide bf16 kernel the forced (ks, variant)."""
    fam: str
    tag: str
    M: int
    K: int
    plan: Optional[Tuple[int, int]] = None

    @property
    def id(self) -> str:
        p = f"-ks{self.plan[0]}v{self.plan[1]}" if self.plan else ""
        return f"{self.fam}-{self.tag}{p}-M{self.M}-K{self.K}"

    @property
    def cap(self) -> Optional[float]:
        """Value-set cap of a bf16 case: 2^14 where a scaled fp16 slab may carry it (variant 0 or the default plan)."""
        return 2.0 ** 14 if self.tag == "wide" and self.plan[1] != 4 and self.plan[0] != 1 else None


WIDE_PLANS = [(1, 0), (2, 0), (4, 0), (3, 4), (4, 4), (0, -1)]  # tests/test_gemm_exact_gpu.py test_bf16_wide


def _paths() -> List[Path_]:
    ps = [Path_("bf16", "skinny", m, 256) for m in (1, 16)]
    ps += [Path_("bf16", "skinnysplit", m, 4128) for m in (1, 16)]  # 129 k slices: the first K that splits
    # the batched kernel takes 17..32 rows only past K = 4096 (gemm.hip bgemm_eligible): 4352 is its first K there
    ps += [Path_("bf16", "batched", 17, 4352), Path_("bf16", "batched", 64, 256)]
    ps += [Path_("bf16", "wide", m, 256 if ks <= 1 else 1024, (ks, v)) for m in (65, 256) for ks, v in WIDE_PLANS]
    for fam, k in (("w8", 1088), ("w4", 1920), ("q4_0", 3072), ("q4_k", 3072), ("q6", 3072)):
        ps += [Path_(fam, "stream", 9, k), Path_(fam, "tile", 40, k)]
    for fam in A8:
        ps += [Path_(fam, "wide", 129, 640), Path_(fam, "widesplit", 129, 2048)]
    return ps


PATHS = _paths()
QKV_CASES = [(p, geo, kv8) for p in PATHS for geo in GEOS for kv8 in (False, True)]


def qkv_id(c) -> str:
    p, geo, kv8 = c
    return f"{p.id}-{geo}-{'fp8' if kv8 else 'bf16'}cache"


def path_seed(p: Path_, geo: str) -> int:
    return 1000 * list(GEOS).index(geo) + 7 * p.M + p.K + 13 * (PATHS.index(p) + 1)


def qkv_inputs(p: Path_, geo: str):
    """(Delivered, bias, slot, pos, S) of a fused-QKV case; quantised families: ``quant_case`` and the same bias."""
    seed = path_seed(p, geo)
    if p.fam == "bf16":
        return qkv_bf16_case(geo, p.M, p.K, seed, p.cap)
    N = exact.qkv_n(GEOS[geo])
    slot, pos, S = rows(p.M, seed)
    return quant_case(p.fam, N, p.K, p.M, seed), qkv_bias(N), slot, pos, S


def path_ranges(p: Path_, N: int, ks: Optional[int] = None):
    """(k ranges, slab format) of a path for ``delivery_exact``: the wide kernels' split plans; fp32 elsewhere."""
    if p.fam == "bf16" and p.tag == "wide":
        ks = p.plan[0] if ks is None else ks
        if ks > 1:
            return exact.wide_k_ranges(p.K, ks), ("f32" if p.plan[1] == 4 else "f16exp")
    if p.fam in A8 and exact.a8_splits(N, p.K) > 1:
        return exact.wide_k_ranges(p.K, exact.a8_splits(N, p.K), stage=128), "f16"
    return None, "f32"


#: gate/up cases: F output columns (2 F weight rows), bf16 on each path once and the quantised kernels once each
ACT_F = 512
ACT_PATHS = [p for p in PATHS if p.fam == "bf16" and (p.tag != "wide" or p.plan in ((1, 0), (2, 0), (3, 4)))] + \
            [p for p in PATHS if p.fam != "bf16" and p.fam != "q6"]
#: the fused norm's exact paths: not the fp16 slabs, which carry the factor and round to 2^-11 (wgemm.hip, wgemm8.hip)
NORM_PATHS = [p for p in PATHS if p.tag != "widesplit" and (p.fam != "bf16" or p.tag != "wide" or p.plan in ((1, 0), (3, 4)))]
NORM_N = 208
#: (path, fused norm?) of the gate/up cases
ACT_CASES = [(p, n) for p in ACT_PATHS for n in (False, True) if not n or p in NORM_PATHS]


def act_id(v) -> str:
    return v.id if isinstance(v, Path_) else ("norm" if v else "plain")


def act_inputs(p: Path_, kind: str, norm: bool) -> Delivered:
    seed = path_seed(p, "phi3") + (1 if kind == "gelu" else 0) + (2 if norm else 0)
    if p.fam == "bf16":
        return act_bf16_case(kind, ACT_F, p.K, p.M, seed, norm)
    # gates 2^e x integer codes: exponents around 0 so that the gates cover the activations' curved range
    return quant_case(p.fam, 2 * ACT_F, p.K, p.M, seed, gateup=True,
                      exps=range(-19, -8) if p.fam in A8 else range(-10, 1) if p.fam in ("q4_k",) else range(-6, 5))


def norm_k(p: Path_) -> int:
    """K of a path's norm case: its own, or 1024 where the rows would not leave columns for the other non-zeros."""
    return p.K if p.M <= p.K // 2 else 1024


def norm_inputs(p: Path_) -> Delivered:
    ranges = path_ranges(p, NORM_N)[0] if p.tag in ("wide", "widesplit") else None
    return norm_case(p.fam, NORM_N, norm_k(p), p.M, path_seed(p, "gqa"), ranges)
