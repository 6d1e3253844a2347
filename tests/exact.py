"""Exact integer-valued GEMM checks (host side; imports without a GPU).

Why they can be exact.  Every GEMM kernel here accumulates in fp32 (an MFMA's accumulator, the split-K partials,
the cross-wave LDS sums).  With integer operands every product and every partial sum is an integer, and an integer
of magnitude below 2^24 is exact in fp32 -- so the result does not depend on the summation order and equals the
int64 product bit for bit, as long as

    max over (m, n) of  sum_k |x[m, k]| |w[n, k]|  <  2^24                                        (B1)

because any partial sum, over any subset of k in any order, is bounded by the sum of the absolute products.
``Weights.bounds`` lists (B1) and, per format, one matrix per further intermediate a kernel forms:

* Q4_0 / Q4_K (gemm_qstream.hip): the codes enter the MFMA as 128 + q, so per weight row the kernel sums
  ``s_b T_b`` with ``T_b = sum_k x_k (128 + q_k)`` and subtracts ``(128 s_b + o_b) X_b`` with ``X_b = sum_k x_k``
  (s = d, o = 8 d for Q4_0; s = d sc, o = dmin m for Q4_K).  Both sums stay integers below 2^24 when
  ``sum_k |x_k| s (128 + q_k) < 2^24`` and ``sum_k |x_k| (128 s + o) < 2^24``: two more matrices in ``bounds``.
* Q6_K (gemm_qstream.hip): ``s_g T_g`` and ``160 s_g X_g`` with s = d sc (int8): ``|s| (128 + q)`` and ``160 |s|``.
* bf16 wide GEMM, variant 0 (wgemm.hip): each k range's partial is stored as fp16 scaled by 2^-ex with
  ex = max(frexp_exp(max |v|) - 14, 0), i.e. unscaled while |v| < 2^14; fp16 holds integers up to 2^11 exactly, so
  every k range needs ``sum_{k in range} |x w| < 2^11`` (``assert_fp16_slabs``; the ranges are ``wide_k_ranges``, the
  mirror of wg_plan's ``kst``).  With operands in {-1, 0, 1} this is K / ks <= 2048.

Epilogues: bias and residual are integers, added in fp32 (exact below 2^24), then one round-to-nearest-even to
bf16 -- what ``torch.Tensor.bfloat16()`` does to the exact value.  The fused QKV epilogue rounds the projection to
bf16 first (the unfused path stores it before RoPE), then rotates; with (cos, sin) in {(1,0), (0,1), (-1,0), (0,-1)}
the rotation is a signed permutation of those bf16 values, exact.  An fp8 KV cache receives e4m3(bf16 value).

Where exactness is impossible (fused RMSNorm, SiLU / GeLU) ``tile_err`` replaces the whole-matrix norm, against
limits of ``FLOOR_FACTOR`` x the measured floors in ``TILE_FLOORS``.

Fused QKV geometries.  ``QKV_CASES`` run at (H, Hkv, hd, T_max) = 2 / 1 / 32 / 64, where much of the epilogue's index
arithmetic collapses; ``QKV_GEO_CASES`` repeat every family at the models' head shapes (``QKV_GEOS``), with idle rows
(slot -1) and rows that share a slot (``qkv_rows``).  ``epi_mirror`` walks the epilogue's addressing on the host with
one fault planted at a time, and ``qkv_mismatch`` must report it wherever it can show (``QKV_FAULT_SHOWS``, checked by
tests/test_exact_cpu.py):

    fault                                   toy 2/1/32   phi3 4/4/96   gqa 4/2/128   gemma 2/1/256
    hkv   Hkv dropped from the cache base   invisible    caught        caught        invisible (Hkv = 1)
    tph   tiles per head -> power of two    invisible    caught        invisible     invisible (2, 6, 8, 16 tiles)
    idle  an idle row written               no idle row  caught        caught        caught
    d5    d >> 5 dropped from kfrag_off     invisible    caught        caught        caught (hd >> 5 = 1, 3, 4, 8)
    b2    partner bias from b1's rows       caught       caught        caught        caught

Row ops (tests/test_rowops_exact_gpu.py, host twin tests/test_rowops_exact_cpu.py): ``quant_rows_ref`` states
quant_rows byte for byte -- on rows whose amax is 448 2^e the scale and its inverse are powers of two and the e4m3
bytes are exact (``quant_exact_rows``); on random rows every element is held to half an e4m3 step
(``quant_general_mismatch``); the folded RMSNorm factor is checked on sparse integer rows whose sum of squares is
exact (``quant_norm_rows``).  ``embed_ref`` is bit-exact, ``rmsnorm_mismatch`` allows one bf16 step.
"""
from __future__ import annotations

import sys
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import torch

if str(Path(__file__).resolve().parent.parent) not in sys.path:  # run as a script (regenerating TILE_FLOORS)
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from cain_amd.models.q4 import Q6_K, pack_q4, pack_q6, q4_fields, q6_fields
from cain_amd.models.weights import (interleave_tiles, pack_mfma_a, pack_mfma_a_fp8, pack_mfma_a_fp8_k128, pack_mxfp4,
                                     rope_pair_order)

TWO24 = 1 << 24
TWO11 = 1 << 11
E2M1_X2 = (0, 1, 2, 3, 4, 6, 8, 12)  # twice the e2m1 magnitudes by 3-bit code


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(int(seed))


def _randint(g, lo, hi, shape):
    """Integers in lo..hi inclusive, int64."""
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64)


@dataclass
class Weights:
    """One generator's result: ``packed`` (the kernel's operands), the decoded weights ``w`` / ``den`` ([N, K] int64
    numerators over a common denominator: 2 for MXFP4, whose 0.5 and 1.5 need even activations, else 1), the format's
    own bytes ``raw`` (for the project's decoders) and ``bounds``: (what, int64 [N, K]) matrices B whose
    ``|x| @ B^T`` must stay below 2^24 x den (module doc)."""
    packed: Dict[str, torch.Tensor]
    w: torch.Tensor
    den: int = 1
    raw: Dict[str, torch.Tensor] = field(default_factory=dict)
    bounds: List[Tuple[str, torch.Tensor]] = field(default_factory=list)

    def __post_init__(self):
        self.bounds.insert(0, ("sum |x w|", self.w.abs()))


# ---------------------------------------------------------------- activations
def int_x(M: int, K: int, seed: int, amp: int = 2, density: float = 1.0, even: bool = False,
          plant: int = 0) -> torch.Tensor:
    """Integer activations [M, K] int64 in -amp..amp (all exact in bf16 and, up to 16, in e4m3); ``density``: the
    share of non-zeros; ``even``: multiples of 2 (MXFP4's halves then give integers); ``plant``: one element per
    row is +-plant, the row's amax, for the per-row activation quantiser (gemm_w8a8, gemm_w4a8, quant_rows:
    scale = amax / 448, inv = 1 / scale, both correctly rounded fp32 divisions).  With 448 the scale is exactly 1;
    with 7 (14) it is exactly 2^-6 (2^-5), inv 64 (32), and every |x| <= 7 (even |x| <= 14) times inv is a multiple
    of 64 up to 448, which e4m3's 3 mantissa bits hold exactly -- the small amax keeps |k|, |v| inside e4m3 for
    the fp8 KV cases."""
    g = _gen(seed)
    x = _randint(g, -amp, amp, (M, K))
    if even:
        x = x * 2
    if density < 1.0:
        x = x * (torch.rand(M, K, generator=g) < density).long()
    if plant:
        assert int(x.abs().max()) <= plant
        col = _randint(g, 0, K - 1, (M,))
        sign = _randint(g, 0, 1, (M,)) * 2 - 1
        x[torch.arange(M), col] = plant * sign
    return x


# ---------------------------------------------------------------- weight generators
def gen_bf16(N: int, K: int, seed: int, amp: int = 2, gateup: bool = False) -> Weights:
    """bf16 weights in -amp..amp through ``pack_mfma_a`` (``gateup``: N / 2 gate rows and N / 2 up rows through
    ``interleave_tiles(tile=8)``, the activation epilogues' row order; ``w`` is then the interleaved matrix)."""
    w = _randint(_gen(seed), -amp, amp, (N, K))
    if gateup:
        w = interleave_tiles(w[: N // 2], w[N // 2:], tile=8)
    return Weights({"wp": pack_mfma_a(w.to(torch.bfloat16))}, w)


def gen_fp8(N: int, K: int, seed: int, amp: int = 8, k128: bool = False, gateup: bool = False,
            small: bool = False) -> Weights:
    """e4m3 weights in -amp..amp (3 mantissa bits: every integer up to 16 is exact) with row scales of 1, packed by
    ``pack_mfma_a_fp8`` (gemm_w8) or ``pack_mfma_a_fp8_k128`` (gemm_w8a8)."""
    amp = 2 if small else amp  # ``small``: the W8A8 split-K cases (fp16 slabs, ``assert_fp16_slabs``)
    assert amp <= 16
    w = _randint(_gen(seed), -amp, amp, (N, K))
    if gateup:
        w = interleave_tiles(w[: N // 2], w[N // 2:], tile=8)
    q = w.float().to(torch.float8_e4m3fn)
    scale = torch.ones(N, dtype=torch.float32)
    return Weights({"wq": (pack_mfma_a_fp8_k128 if k128 else pack_mfma_a_fp8)(q), "scale": scale}, w,
                   raw={"q": q, "scale": scale})


def gen_mxfp4(N: int, K: int, seed: int, gateup: bool = False) -> Weights:
    """MXFP4 codes over all 16 e2m1 values at scale byte 127 (2^0).  ``w`` holds twice the values (``den`` 2)."""
    codes = _randint(_gen(seed), 0, 15, (N, K))
    if gateup:
        codes = interleave_tiles(codes[: N // 2], codes[N // 2:], tile=8)
    scales = torch.full((N, K // 32), 127, dtype=torch.uint8)
    w2 = torch.tensor(E2M1_X2)[codes & 7] * torch.where((codes & 8) != 0, -1, 1)
    c8 = codes.to(torch.uint8)
    wq, wsc = pack_mxfp4(c8, scales)
    return Weights({"wq": wq, "wsc": wsc}, w2, den=2, raw={"codes": c8, "scales": scales})


def _mixed(g, shape, small: int, full_lo: int, full_hi: int, p_full: float, lo_small: int = 0):
    """Mostly small values, with a share ``p_full`` over the field's full range (keeps the sums below 2^24 while
    every bit of the field is exercised)."""
    v = _randint(g, lo_small, small, shape)
    f = _randint(g, full_lo, full_hi, shape)
    return torch.where(torch.rand(shape, generator=g) < p_full, f, v)


def _fp16_bytes(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float16).contiguous().view(torch.uint8).reshape(*x.shape, 2)


def gen_q4_0(N: int, K: int, seed: int, gateup: bool = False) -> Weights:
    """ggml Q4_0 blocks built field by field: d = 1.0, every code 0..15; w = q - 8."""
    q = _randint(_gen(seed), 0, 15, (N, K))
    if gateup:
        q = interleave_tiles(q[: N // 2], q[N // 2:], tile=8)
    qb = q.to(torch.uint8).reshape(N, K // 32, 32)
    blocks = torch.cat([_fp16_bytes(torch.ones(N, K // 32)), qb[..., :16] | (qb[..., 16:] << 4)], -1).contiguous()
    wq, sb = pack_q4(q4_fields(blocks, 0, N, K), 0)
    one = torch.ones_like(q)
    return Weights({"wq": wq, "sbuf": sb}, q - 8, raw={"blocks": blocks},
                   bounds=[("Q4_0 sum |x| d (128 + q)", 128 + q), ("Q4_0 sum |x| 136 d", 136 * one)])


def gen_q4_k(N: int, K: int, seed: int, small: bool = False, gateup: bool = False) -> Weights:
    """ggml Q4_K blocks built field by field: d = dmin = 1.0, integer 6-bit sub-scales and mins (1 block in 8 over
    the whole 0..63, the rest 0..3; ``small``: 0..1 and 0..2, for the fp8 KV cases), every code; w = sc q - m."""
    g = _gen(seed)
    q = _randint(g, 0, 15, (N, K))
    if gateup:
        q = interleave_tiles(q[: N // 2], q[N // 2:], tile=8)
    shp = (N, K // 256, 8)
    sc = _randint(g, 0, 1, shp) if small else _mixed(g, shp, 3, 0, 63, 0.125)
    mn = _randint(g, 0, 2, shp) if small else _mixed(g, shp, 3, 0, 63, 0.125)
    sci, mi = sc.to(torch.uint8), mn.to(torch.uint8)
    # ggml's 12 bytes of 6-bit pairs (the inverse of get_scale_min_k4)
    scales = torch.cat([sci[..., :4] | ((sci[..., 4:] >> 4) << 6), mi[..., :4] | ((mi[..., 4:] >> 4) << 6),
                        (sci[..., 4:] & 0x0F) | ((mi[..., 4:] & 0x0F) << 4)], -1)
    qp = q.to(torch.uint8).reshape(N, K // 256, 4, 2, 32)  # 4 groups of 64: sub-block 2g low nibbles, 2g + 1 high
    qs = (qp[..., 0, :] | (qp[..., 1, :] << 4)).reshape(N, K // 256, 128)
    one = torch.ones(N, K // 256)
    blocks = torch.cat([_fp16_bytes(one), _fp16_bytes(one), scales, qs], -1).contiguous()
    wq, sb = pack_q4(q4_fields(blocks, 1, N, K), 1)
    s = sc.reshape(N, K // 32).repeat_interleave(32, 1)
    o = mn.reshape(N, K // 32).repeat_interleave(32, 1)
    return Weights({"wq": wq, "sbuf": sb}, s * q - o, raw={"blocks": blocks},
                   bounds=[("Q4_K sum |x| d sc (128 + q)", s * (128 + q)), ("Q4_K sum |x| (128 d sc + dmin m)", 128 * s + o)])


def gen_q6_k(N: int, K: int, seed: int, small: bool = False) -> Weights:
    """ggml Q6_K blocks built field by field: d = 1.0, integer int8 group scales (1 group in 16 over the whole
    -128..127, the rest -3..3; ``small``: -1..1), every code 0..63; w = sc (q - 32)."""
    g = _gen(seed)
    q = _randint(g, 0, 63, (N, K))
    shp = (N, K // 256, 16)
    sc = _randint(g, -1, 1, shp) if small else _mixed(g, shp, 3, -128, 127, 1.0 / 16, lo_small=-3)
    q8 = q.to(torch.uint8).reshape(N, K // 256, 2, 4, 32)  # [half, quarter, l]: element 128 h + 32 j + l
    lo, hi = q8 & 15, q8 >> 4
    ql = torch.cat([lo[..., 0, :] | (lo[..., 2, :] << 4), lo[..., 1, :] | (lo[..., 3, :] << 4)], -1)
    qh = hi[..., 0, :] | (hi[..., 1, :] << 2) | (hi[..., 2, :] << 4) | (hi[..., 3, :] << 6)
    blocks = torch.cat([ql.reshape(N, K // 256, 128), qh.reshape(N, K // 256, 64),
                        sc.to(torch.int8).view(torch.uint8), _fp16_bytes(torch.ones(N, K // 256))], -1).contiguous()
    wq, sb = pack_q6(q6_fields(blocks, N, K))
    s = sc.reshape(N, K // 16).repeat_interleave(16, 1)
    return Weights({"wq": wq, "sbuf": sb}, s * (q - 32), raw={"blocks": blocks},
                   bounds=[("Q6_K sum |x| |d sc| (128 + q)", s.abs() * (128 + q)), ("Q6_K sum |x| 160 |d sc|", 160 * s.abs())])


GENERATORS = {"bf16": gen_bf16, "w8": gen_fp8, "w8a8": lambda *a, **k: gen_fp8(*a, k128=True, **k), "w4": gen_mxfp4,
              "w4a8": gen_mxfp4, "q4_0": gen_q4_0, "q4_k": gen_q4_k, "q6": gen_q6_k}
Q6_FMT = Q6_K


# ---------------------------------------------------------------- the GPU file's cases
@dataclass(frozen=True)
class Case:
    """One exact GEMM case of tests/test_gemm_exact_gpu.py (listed here so that tests/test_exact_cpu.py can check
    the generators and the exactness bounds at every shape the GPU file uses)."""
    fam: str
    N: int
    K: int
    M: int
    tag: str = ""      # the path the GPU test forces / expects
    amp: int = 2       # activations (and bf16 weights) in -amp..amp
    density: float = 1.0
    small: bool = False  # small block scales (fp8 KV: |values| <= 448)
    geo: str = ""      # fused QKV: a key of QKV_GEOS ("": the 2 / 1 / 32 / 64 geometry of QKV_CASES)

    @property
    def id(self) -> str:
        tag = "-".join(t for t in (self.tag, self.geo) if t)
        return f"{self.fam}-{tag + '-' if tag else ''}N{self.N}-K{self.K}-M{self.M}"


def a8_plant(c: Case) -> int:
    """The planted row maximum of an activation-quantised case (``int_x``): 448, or 7 (14 where MXFP4 needs even
    activations) for the fp8 KV cases; 0 for the other families."""
    if c.fam not in ("w8a8", "w4a8"):
        return 0
    return 448 if c.tag != "qkv8" else 14 if c.fam == "w4a8" else 7


def case_inputs(c: Case, seed: int = 0):
    """(x int64 [M, K], Weights, exact product int64 [M, N]) of a case; seeds derive from the shape."""
    sd = seed + c.N + 3 * c.K + 7 * c.M
    even = c.fam in ("w4", "w4a8")
    amp = 8 if a8_plant(c) == 448 else c.amp
    x = int_x(c.M, c.K, sd, amp=max(1, amp // (2 if even else 1)), density=c.density, even=even, plant=a8_plant(c))
    kw = {"amp": c.amp} if c.fam == "bf16" else {"small": True} if c.small else {}
    ew = GENERATORS[c.fam](c.N, c.K, sd + 1, **kw)
    return x, ew, product(x, ew)


#: rows per launch the Q4 / Q6 cases assume at their K (checked against the library on the GPU).  K = 3072 (24 quads,
#: 8 waves) is the K whose launches hold between 2 and 8 rows; K = 2816 is there for the other side of the 4-wave /
#: 8-wave choice (22 quads), where no K has fewer than 9 rows: below 24 quads a launch falls back to the 8-wave
#: kernel's 48 KiB copy once the 4-wave one is full, and that holds 9 rows of 2816.
Q_ROWS = {2816: 9, 3072: 8}


def _cases() -> List[Case]:
    cs: List[Case] = []
    # bf16 skinny kernel, unsplit: fewer tiles than workgroups, 13 tiles, 33 k slices (uneven over the waves)
    cs += [Case("bf16", n, 1056, m, "skinny") for n in (16, 48, 208) for m in (1, 15, 16)]
    # ... its few-row split-K grid: narrow N, K / 32 > 128 slices
    cs += [Case("bf16", 48, 8192, m, "skinnysplit") for m in (1, 16)]
    # batched path (16 < M <= 64): split (narrow N) and unsplit (>= 128 row blocks)
    cs += [Case("bf16", 208, 4352, 17, "batched"), Case("bf16", 208, 512, 33, "batched"),
           Case("bf16", 208, 512, 64, "batched"), Case("bf16", 48, 4352, 64, "batched"),
           Case("bf16", 16400, 256, 33, "batched")]
    # wide path (64 < M <= 256): operands in {-1, 0, 1}, K / ks <= 2048 (fp16 slabs, module doc)
    cs += [Case("bf16", 208, 1024, m, "wide", amp=1) for m in (65, 129, 256)]
    cs += [Case("w8", n, 1088, m) for n in (48, 208) for m in (1, 16, 17, 64)]
    # MXFP4 few-row: 15 quads (uneven over 4 / 8 waves) on every variant; LDS-copy edges; split-K; a wide grid
    cs += [Case("w4", 208, 1920, m, "variants") for m in (1, 5, 40)]
    cs += [Case("w4", n, 1920, m, "lds") for n, m in ((16, 7), (48, 8), (48, 12), (48, 13))]
    cs += [Case("w4", 48, 6144, m, "split") for m in (1, 3)]
    cs += [Case("w4", 12304, 256, 1, "occupancy")]
    for fam in ("q4_0", "q4_k", "q6"):  # M = rows, rows + 1, 2 rows + 1 of the library's rows per launch (Q_ROWS)
        cs += [Case(fam, n, k, m, "rows") for n, k in ((208, 2816), (48, 3072)) for r in (Q_ROWS[k],)
               for m in (r, r + 1, 2 * r + 1)]
    for fam in ("w8a8", "w4a8"):
        cs += [Case(fam, 208, 640, m) for m in (17, 64, 65, 256)]
    # split-K of the activation-quantised kernels: fp16 slabs (wgemm8.hip), so every k range's sum |x w| < 2^11 --
    # W8A8 with weights in -2..2 and sparse activations beside the planted 448; MXFP4's +-6 x 448 cannot fit, so
    # W4A8 split-K is NOT exact: "split16" cases are held to fp16's rounding instead (the GPU test's docstring)
    cs += [Case("w8a8", 48, 2048, m, "split", density=1.0 / 16, small=True) for m in (17, 256)]
    cs += [Case("w4a8", 48, 2048, m, "split16", density=1.0 / 16) for m in (17, 256)]
    return cs


CASES = _cases()

#: fused QKV + RoPE + KV-append geometry of the exact cases: 2 q heads, 1 kv head of 32 dims = 8 tiles
QKV_H, QKV_HKV, QKV_HD, QKV_TMAX = 2, 1, 32, 64
QKV_N = (QKV_H + 2 * QKV_HKV) * QKV_HD
Geo = Tuple[int, int, int, int]  # (H, Hkv, hd, T_max)
QKV_GEO: Geo = (QKV_H, QKV_HKV, QKV_HD, QKV_TMAX)

#: the models' head geometries (module doc, "Fused QKV geometries"); T_max = 96 is no power of two: 6 K blocks of 16
#: positions, 3 V^T blocks of 32
QKV_GEOS: Dict[str, Geo] = {
    "phi3": (4, 4, 96, 96),    # MHA; 6 tiles per head (no power of two)
    "gqa": (4, 2, 128, 96),    # Hkv > 1; hd >> 5 = 4 fragments per K block
    "gemma": (2, 1, 256, 96),  # hd >> 4 = 16 V tiles per block
}


def case_geo(c: "Case") -> Geo:
    return QKV_GEOS[c.geo] if c.geo else QKV_GEO


def qkv_n(geo: Geo) -> int:
    H, Hkv, hd, _ = geo
    return (H + 2 * Hkv) * hd


def qkv_case(fam: str, K: int, M: int, kv8: bool, geo: str = "") -> Case:
    """fp8 KV: sparse activations and small block scales keep |k|, |v| <= 448 (no e4m3 saturation); on the
    activation-quantised families the planted row maximum is 7 / 14 instead of 448 (``int_x``).  ``geo``: a key of
    ``QKV_GEOS`` ("": ``QKV_GEO``)."""
    N = qkv_n(QKV_GEOS[geo] if geo else QKV_GEO)
    if kv8:
        return Case(fam, N, K, M, "qkv8", amp=3 if fam in ("w8a8", "w4a8") else 1, density=8.0 / K,
                    small=fam in ("q4_k", "q6", "w8a8"), geo=geo)
    return Case(fam, N, K, M, "qkv", amp=2 if fam != "bf16" or M <= 64 else 1, geo=geo)


#: (family, K, row counts) of the QKV cases; the Q4 / Q6 row counts straddle their launches (4 rows at K = 3072)
QKV_SHAPES = [("bf16", 1056, (1, 16)), ("bf16", 512, (40,)), ("bf16", 1024, (129,)), ("w8", 1088, (5, 40)),
              ("w4", 1920, (5, 40)), ("q4_0", 3072, (4, 5, 9)), ("q4_k", 3072, (4, 5, 9)), ("q6", 3072, (4, 5, 9)),
              ("w8a8", 640, (40,)), ("w4a8", 640, (40,))]
QKV_ROWS = {3072: 4}
QKV_CASES = [qkv_case(f, k, m, kv8) for f, k, ms in QKV_SHAPES for m in ms for kv8 in (False, True)]

#: one row count per (family, K) of QKV_SHAPES at each geometry of QKV_GEOS, across a row-block or launch boundary
#: where the path has one: the skinny kernel's single 16-row block full; 2.5 row blocks of 16 (batched bf16, fp8 and
#: MXFP4 weights); 129 rows = the wide kernels' 128-row tile + 1 (bf16 and the activation-quantised pair, which then
#: run their 256-row tile); Q4 / Q6: 2 launches of QKV_ROWS rows + 1.  No family is dropped from any geometry.
QKV_GEO_ROWS = {("bf16", 1056): 16, ("bf16", 512): 40, ("bf16", 1024): 129, ("w8", 1088): 40, ("w4", 1920): 40,
                ("q4_0", 3072): 9, ("q4_k", 3072): 9, ("q6", 3072): 9, ("w8a8", 640): 129, ("w4a8", 640): 129}
QKV_GEO_CASES = [qkv_case(f, k, QKV_GEO_ROWS[f, k], kv8, geo) for geo in QKV_GEOS for f, k, _ in QKV_SHAPES
                 for kv8 in (False, True)]


def qkv_rows(M: int, T_max: int, seed: int):
    """(slot int32 [M], pos int32 [M], S) of one fused-QKV launch over S cache slots.

    What a prefill chunk or the K + 1 verify rows of speculative decoding look like, plus masked rows --
    * about a quarter of the rows, always the first and the last, are idle: slot -1 (pos 0: a masked row's position
      is unspecified, the kernel may read its tables);
    * five live rows share one slot at positions 15, 16 (two K blocks), 31, 32 (two V^T blocks) and T_max - 1;
    * the other live rows draw distinct (slot, position) pairs, so every cache element has at most one owner;
    * the live rows stand in random order, so the shared slot's rows fall into different row blocks / launches."""
    g = _gen(seed)
    assert M >= 8 and T_max > 33
    S = max(3, (M + 3) // 4)
    inner = 1 + torch.randperm(M - 2, generator=g)
    idle = torch.cat([torch.tensor([0, M - 1]), inner[: max(2, M // 4) - 2]])
    live = inner[max(2, M // 4) - 2:]  # already in random order
    slot = torch.full((M,), -1, dtype=torch.int32)
    pos = torch.zeros(M, dtype=torch.int32)
    s0 = int(torch.randint(0, S, (1,), generator=g))
    fixed = [15, 16, 31, 32, T_max - 1]
    free = [i for i in torch.randperm(S * T_max, generator=g).tolist() if not (i // T_max == s0 and i % T_max in fixed)]
    pairs = [(s0, p) for p in fixed] + [(i // T_max, i % T_max) for i in free[: len(live) - len(fixed)]]
    for m, (s, p) in zip(live.tolist(), pairs):
        slot[m], pos[m] = s, p
    assert len(idle) + len(pairs) == M
    return slot, pos, S


def plain_extras(c: Case):
    """The integer bias [N] (-300..300, so bf16 outputs pass 256 and round) and residual [M, N] (-128..128, exact
    in bf16) of a case's EPI_BF16 and EPI_RESID runs."""
    g = _gen(c.N + c.M)
    bias = torch.randint(-300, 301, (c.N,), generator=g)
    return bias, torch.randint(-128, 129, (c.M, c.N), generator=g)


# ---------------------------------------------------------------- exact reference and its bounds
def product(x: torch.Tensor, ew: Weights) -> torch.Tensor:
    """The exact x @ W^T as int64 [M, N], with every bound of ``ew`` asserted (module doc)."""
    ax = x.abs()
    for what, b in ew.bounds:
        worst = int((ax @ b.t()).max())
        assert worst < TWO24 * ew.den, f"{what}: {worst} / {ew.den} >= 2^24, fp32 would round"
    y = x @ ew.w.t()
    assert int((y % ew.den).abs().max()) == 0, "halves left over: MXFP4 weights need even activations"
    return y // ew.den


def wide_k_ranges(K: int, ks: int, stage: int = 64) -> List[Tuple[int, int]]:
    """The k ranges of a wide-GEMM launch with ``ks`` splits (wgemm_ring.h wg_split_even, for wgemm.hip wg_plan /
    wgemm8.hip w8_plan: stages of 64 / 128 k, kst = ceil(stages / ks) stages per range)."""
    stages = K // stage
    kst = -(-stages // ks)
    return [(i * kst * stage, min((i + 1) * kst * stage, K)) for i in range(-(-stages // kst))]


def a8_splits(N: int, K: int) -> int:
    """Split count of the W8A8 / W4A8 wide kernels (the mirror of wgemm8.hip w8_plan = wgemm_ring.h wg_split)."""
    nblk = (N // 16 + 7) // 8
    stages = K // 128
    ks = 1 if nblk >= 128 else max(1, min(8, (256 + nblk // 2) // nblk))
    ks = min(ks, max(1, stages // 4))
    kst = -(-stages // ks)
    return -(-stages // kst)


def assert_fp16_slabs(x: torch.Tensor, ew: Weights, ks: int, stage: int = 64) -> None:
    """Every k range's sum |x w| < 2^11: the wide GEMMs' fp16 split-K slabs then hold the partials exactly."""
    if ks <= 1:
        return
    for k0, k1 in wide_k_ranges(x.shape[1], ks, stage):
        worst = int((x[:, k0:k1].abs() @ ew.w[:, k0:k1].abs().t()).max())
        assert worst < TWO11 * ew.den, f"k range {k0}..{k1}: sum |x w| = {worst} >= 2^11, an fp16 slab would round"


def to_bf16(v: torch.Tensor) -> torch.Tensor:
    """Exact integers (|v| < 2^24) -> bf16 by PyTorch's round-to-nearest-even."""
    assert int(v.abs().max()) < TWO24
    return v.float().bfloat16()


def to_fp8_of_bf16(v: torch.Tensor) -> torch.Tensor:
    """What an fp8 KV cache holds: e4m3(bf16(v)) by PyTorch's conversions (|v| <= 448: no saturation), as fp32."""
    assert int(v.abs().max()) <= 448, f"|value| {int(v.abs().max())} > 448 would saturate e4m3"
    return to_bf16(v).float().to(torch.float8_e4m3fn).float()


# ---------------------------------------------------------------- comparator
def mismatches(got: torch.Tensor, want: torch.Tensor) -> Optional[str]:
    """None when ``got`` equals ``want`` element by element (any leading shape, last dim = columns); else a report
    with the count and the first mismatch's (row, column, 16-column tile, got, want)."""
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    g = got.detach().cpu().reshape(-1, got.shape[-1])
    w = want.detach().cpu().reshape(-1, want.shape[-1]).to(g.dtype)
    bad = ~((g == w) | (g.isnan() & w.isnan())) if g.is_floating_point() else g != w
    n = int(bad.sum())
    if n == 0:
        return None
    r, c = (int(v) for v in bad.nonzero()[0])
    tiles = sorted({(int(a), int(b) // 16) for a, b in bad.nonzero()[:4096]})
    return (f"{n} of {bad.numel()} elements differ in {len(tiles)}{'+' if n > 4096 else ''} (row, tile) units; first at "
            f"row {r}, column {c}, tile {c // 16}: got {float(g[r, c])!r}, want {float(w[r, c])!r}")


def assert_equal(got: torch.Tensor, want: torch.Tensor, tag: str = "") -> None:
    rep = mismatches(got, want)
    assert rep is None, f"{tag}: {rep}"


def first_bad_tile(got: torch.Tensor, want: torch.Tensor) -> Optional[Tuple[int, int]]:
    """(row, 16-column tile) of the first mismatch, None if equal (what a failure names)."""
    bad = (got.detach().cpu() != want.detach().cpu().to(got.dtype)).nonzero()
    return None if len(bad) == 0 else (int(bad[0][0]), int(bad[0][1]) // 16)


# ---------------------------------------------------------------- per-tile metric
def tile_errs(y: torch.Tensor, ref64: torch.Tensor) -> torch.Tensor:
    """[M, N / 16]: ||y - ref||_tile / (rms(ref) * 4) per (row, 16-column tile), rms over the whole reference (a tile
    whose values cancel does not blow the figure up); 4 = sqrt(16), so the figure is the tile's rms error in units
    of the reference's rms."""
    ref = ref64.detach().cpu().double()
    d = (y.detach().cpu().double() - ref).reshape(ref.shape[0], -1, 16)
    return d.norm(dim=-1) / (ref.pow(2).mean().sqrt() * 4.0)


def tile_err(y: torch.Tensor, ref64: torch.Tensor) -> float:
    return float(tile_errs(y, ref64).max())


def worst_tile(y: torch.Tensor, ref64: torch.Tensor) -> Tuple[int, int]:
    e = tile_errs(y, ref64)
    i = int(e.argmax())
    return i // e.shape[1], i % e.shape[1]


def f32_bound(x: torch.Tensor, ew: Weights) -> torch.Tensor:
    """Per-element bound of a linear fp32-output GEMM: |y - ref| <= K 2^-24 sum_k |x_k w_k| (fp32 summation of K
    terms in any order: at most K - 1 roundings of relative size 2^-24 each, first order)."""
    return x.shape[1] * 2.0 ** -24 * (x.double().abs() @ ew.w.abs().double().t()) / ew.den


# ---------------------------------------------------------------- the non-exact cases (section 3 of the issue)
def normed(x: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    xd = x.double()
    return xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps)


def gateup_ref(h: torch.Tensor, act: str) -> torch.Tensor:
    """fp64 act(gate) * up of an interleaved projection h [M, 2F] (8 gate rows, then their 8 up rows, per tile)."""
    M, n = h.shape
    hh = h.double().view(M, n // 16, 2, 8)
    g, u = hh[:, :, 0].reshape(M, n // 2), hh[:, :, 1].reshape(M, n // 2)
    a = {"silu": torch.nn.functional.silu, "relu": torch.relu,
         "gelu": lambda t: torch.nn.functional.gelu(t, approximate="tanh")}[act](g)
    return a * u


#: shapes of the per-tile cases: family -> (N, K, M); N covers several tiles, odd tile counts and, above 16 rows,
#: a second row block ("bf16_wide_split": the wide path with a forced 2-way split on fp32 slabs).  The weights are
#: the family's integer generator, with ``gateup`` for the activation epilogues.
SOFT_SHAPES = {"bf16": (224, 512, 5), "bf16_batched": (224, 512, 40), "bf16_wide": (224, 512, 129),
               "bf16_wide_split": (224, 512, 129), "w8": (224, 512, 20), "w4": (224, 512, 20), "q4_0": (224, 512, 5),
               "q4_k": (224, 512, 5), "q6": (224, 512, 5), "w8a8": (224, 512, 40), "w4a8": (224, 512, 40)}
SOFT_SEED = 77


def soft_base(fam: str) -> str:
    return "bf16" if fam.startswith("bf16") else fam


def soft_x(M: int, K: int, seed: int, a8: bool = False) -> torch.Tensor:
    """fp64 activations of the fused-norm cases: even integers -8..8 over 8, sparse (1 in 8); ``a8`` (activation-
    quantised paths): one element per row is +-448 / 8, so amax / 448 = 1 / 8 and the e4m3 step is exact -- there
    too only the RMSNorm arithmetic is inexact."""
    return int_x(M, K, seed, amp=4, density=0.125, even=True, plant=448 if a8 else 0).double() / 8.0


def soft_gate_x(fam: str, w: torch.Tensor) -> torch.Tensor:
    """fp64 activations of the SiLU / GeLU cases: sparse integers -7..7 (each row's maximum a planted 7, see
    ``int_x``: the activation-quantised paths then quantise exactly) times the power of two that puts the rms of
    the gate pre-activations in [1, 2) -- where SiLU, GeLU and ReLU differ most -- whatever the magnitude of the
    family's weights.  Integers times a power of two: x is exact in bf16, and every partial sum of the projection
    is exact in fp32, so only the activation arithmetic and the output rounding are inexact."""
    N, K, M = SOFT_SHAPES[fam]
    xi = int_x(M, K, SOFT_SEED + M, amp=7, density=0.125, plant=7).double()
    h = (xi @ w.t()).view(M, N // 16, 2, 8)[:, :, 0]  # the gate rows (``gateup_ref``)
    rms = float(h.pow(2).mean().sqrt())
    return xi * 2.0 ** -int(torch.floor(torch.log2(torch.tensor(rms))))


def soft_case(fam: str, kind: str):
    """(x fp64 [M, K], Weights, ref fp64) of one per-tile case; ``kind``: "norm" (fused RMSNorm, fp32 output),
    "silu", "gelu" (gate/up epilogues, bf16 output, no norm); "relu" is no epilogue of the kernels: the same case
    with the wrong non-linearity, for tests/test_exact_cpu.py."""
    N, K, M = SOFT_SHAPES[fam]
    base = soft_base(fam)
    if base == "q6" and kind != "norm":
        raise ValueError("gemm_q6 has no gate/up epilogue")
    if kind == "norm":
        ew = GENERATORS[base](N, K, SOFT_SEED)
        x = soft_x(M, K, SOFT_SEED + M, base in ("w8a8", "w4a8"))
        return x, ew, normed(x) @ (ew.w.double() / ew.den).t()
    # Q4_K with small sub-scales and mins: its full-range blocks (1 in 8) would carry the whole rms, and the other
    # blocks' gates would sit near 0, where every activation is linear
    ew = GENERATORS[base](N, K, SOFT_SEED, gateup=True, **({"small": True} if base == "q4_k" else {}))
    w = ew.w.double() / ew.den
    x = soft_gate_x(fam, w)
    return x, ew, gateup_ref(x @ w.t(), kind)


FLOOR_FACTOR = 3.0
#: tile_err of the fp64 reference rounded to the output dtype (fp32 for "norm", bf16 for "silu" / "gelu"): the floor
#: no correct kernel can beat.  Regenerate with ``python tests/exact.py`` (CPU only; prints this dict) after changing
#: SOFT_SHAPES, SOFT_SEED, soft_x or a generator; tests/test_exact_cpu.py checks the stored values are current.
TILE_FLOORS: Dict[str, float] = {
    "bf16/norm": 4.2732e-08,
    "bf16/silu": 3.0987e-03,
    "bf16/gelu": 3.7159e-03,
    "bf16_batched/norm": 6.4085e-08,
    "bf16_batched/silu": 6.1716e-03,
    "bf16_batched/gelu": 4.3012e-03,
    "bf16_wide/norm": 4.7867e-08,
    "bf16_wide/silu": 9.4174e-03,
    "bf16_wide/gelu": 6.3085e-03,
    "bf16_wide_split/norm": 4.7867e-08,
    "bf16_wide_split/silu": 9.4174e-03,
    "bf16_wide_split/gelu": 6.3085e-03,
    "w8/norm": 4.8176e-08,
    "w8/silu": 6.5546e-03,
    "w8/gelu": 5.1664e-03,
    "w4/norm": 4.6240e-08,
    "w4/silu": 5.4972e-03,
    "w4/gelu": 4.2425e-03,
    "q4_0/norm": 4.8195e-08,
    "q4_0/silu": 4.2292e-03,
    "q4_0/gelu": 4.0884e-03,
    "q4_k/norm": 5.4289e-08,
    "q4_k/silu": 3.7993e-03,
    "q4_k/gelu": 3.8787e-03,
    "q6/norm": 5.7781e-08,
    "w8a8/norm": 4.3287e-08,
    "w8a8/silu": 4.8540e-03,
    "w8a8/gelu": 5.9703e-03,
    "w4a8/norm": 5.2359e-08,
    "w4a8/silu": 8.3751e-03,
    "w4a8/gelu": 5.0978e-03,
}


def measure_floor(fam: str, kind: str) -> float:
    _, _, ref = soft_case(fam, kind)
    return tile_err(ref.float() if kind == "norm" else ref.bfloat16(), ref)


def soft_keys():
    for fam in SOFT_SHAPES:
        for kind in ("norm", "silu", "gelu"):
            if not (fam == "q6" and kind != "norm"):
                yield fam, kind


def tile_limit(fam: str, kind: str) -> float:
    return FLOOR_FACTOR * TILE_FLOORS[f"{fam}/{kind}"]


# ---------------------------------------------------------------- RoPE as a signed permutation
def unit_rope_tables(T_max: int, hd: int, seed: int):
    """cos, sin [T_max, hd / 2] fp32 with (cos, sin) in {(1,0), (0,1), (-1,0), (0,-1)}, an independent choice per
    (position, frequency pair)."""
    c = _randint(_gen(seed), 0, 3, (T_max, hd // 2))
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[c]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[c]
    return cos.contiguous(), sin.contiguous()


def rot(v: torch.Tensor, c: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """RoPE of v [..., hd] (pairs j, j + hd / 2) with per-pair c, s [hd / 2]."""
    half = v.shape[-1] // 2
    a, b = v[..., :half], v[..., half:]
    return torch.cat([a * c - b * s, b * c + a * s], -1)


def qkv_perm(H: int, Hkv: int, hd: int) -> torch.Tensor:
    """Kernel row order of a fused QKV projection: q and k heads in ``rope_pair_order``, V rows as they are."""
    per = rope_pair_order(hd)
    return torch.cat([h * hd + per for h in range(H + Hkv)] + [torch.arange((H + Hkv) * hd, (H + 2 * Hkv) * hd)])


def qkv_expected(proj: torch.Tensor, pos: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, H: int, Hkv: int,
                 hd: int):
    """From the exact projection (+ bias) in the KERNEL's row order [M, (H + 2 Hkv) hd] int64: the values the
    epilogue must produce, as fp32 holding bf16-exact numbers -- q [M, H, hd], k [M, Hkv, hd] (natural head-dim
    order, rotated) and v [M, Hkv, hd]."""
    M = proj.shape[0]
    inv = torch.empty_like(qkv_perm(H, Hkv, hd))
    inv[qkv_perm(H, Hkv, hd)] = torch.arange(inv.numel())
    nat = to_bf16(proj).float()[:, inv]  # natural row order: rounded to bf16 BEFORE the rotation (gemm_epi.h)
    c, s = cos[pos.long()][:, None], sin[pos.long()][:, None]  # [M, 1, hd / 2]
    q = rot(nat[:, : H * hd].view(M, H, hd), c, s)
    k = rot(nat[:, H * hd:(H + Hkv) * hd].view(M, Hkv, hd), c, s)
    v = nat[:, (H + Hkv) * hd:].view(M, Hkv, hd)
    return q, k, v


def qkv_launch(c: Case):
    """(bias [N] int64 in the kernel's row order, slot, pos, S, cos, sin) of a fused-QKV case: the rows of
    ``qkv_rows`` at a geometry of QKV_GEOS; for QKV_CASES a permutation of M + 3 slots at any position."""
    T, hd = case_geo(c)[3], case_geo(c)[2]
    g = _gen(c.M + c.K)
    bias = torch.randint(-20, 21, (c.N,), generator=g)
    if c.geo:
        slot, pos, S = qkv_rows(c.M, T, c.M + c.K + c.N)
    else:
        S = c.M + 3
        slot = torch.randperm(S, generator=g)[:c.M].int()
        pos = torch.randint(0, T, (c.M,), generator=g).int()
    cos, sin = unit_rope_tables(T, hd, c.K)
    return bias, slot, pos, S, cos, sin


def qkv_want(proj: torch.Tensor, slot: torch.Tensor, pos: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
             geo: Geo, S: int, kv8: bool, sentinel: float = -7.0, v_only: bool = False):
    """What one launch must leave behind, from the exact projection + bias [M, N] int64 in the kernel's row order:
    (q [M, H hd] with ``sentinel`` on idle rows, K [S, Hkv, T_max, hd], V [S, Hkv, T_max, hd] in natural order, zero
    wherever no row writes, owner [S, T_max]: the row that owns a cache position, -1 for none).  ``v_only``: a launch
    of the V rows alone (q and the K cache untouched)."""
    H, Hkv, hd, T = geo
    M = proj.shape[0]
    wq, wk, wv = qkv_expected(proj, pos, cos, sin, H, Hkv, hd)
    want_q = wq.reshape(M, H * hd).clone()
    want_q[slot < 0] = sentinel
    if v_only:
        want_q[:] = sentinel
    want_k, want_v = torch.zeros(S, Hkv, T, hd), torch.zeros(S, Hkv, T, hd)
    owner = torch.full((S, T), -1, dtype=torch.long)
    for m in range(M):
        sl, ps = int(slot[m]), int(pos[m])
        if sl < 0:
            continue
        assert int(owner[sl, ps]) == -1, f"rows {int(owner[sl, ps])} and {m} both write (slot {sl}, position {ps})"
        owner[sl, ps] = m
        if not v_only:
            want_k[sl, :, ps] = to_fp8_of_bf16(wk[m].long()) if kv8 else wk[m]
        want_v[sl, :, ps] = to_fp8_of_bf16(wv[m].long()) if kv8 else wv[m]
    return want_q, want_k, want_v, owner


def qkv_mismatch(q: torch.Tensor, kn: torch.Tensor, vn: torch.Tensor, want, slot: torch.Tensor, pos: torch.Tensor,
                 geo: Geo) -> Optional[str]:
    """None when q [M, H hd] and the unpacked caches [S, Hkv, T_max, hd] equal ``qkv_want``'s; else a report that
    names, per output, the count and the first mismatch's (row, head, 16-row tile, slot, position)."""
    want_q, want_k, want_v, owner = want
    H, Hkv, hd, _ = geo
    out = []
    qf = q.detach().cpu().float()
    bad = (qf != want_q).nonzero()
    if len(bad):
        m, col = (int(v) for v in bad[0])
        out.append(f"q: {len(bad)} elements differ; first at row {m} (slot {int(slot[m])}, position {int(pos[m])}), "
                   f"head {col // hd}, tile {col // 16}, dim {col % hd}: got {float(qf[m, col])!r}, "
                   f"want {float(want_q[m, col])!r}")
    for name, got, w, t0 in (("K", kn, want_k, H * hd // 16), ("V", vn, want_v, (H + Hkv) * hd // 16)):
        gf = got.detach().cpu().float()
        bad = (gf != w).nonzero()
        if len(bad):
            s, h, t, d = (int(v) for v in bad[0])
            m = int(owner[s, t])
            out.append(f"{name} cache: {len(bad)} elements differ; first at slot {s}, kv head {h}, position {t}, dim {d} "
                       f"(natural-order tile {t0 + (h * hd + d) // 16}; "
                       f"{'row ' + str(m) if m >= 0 else 'no row'} writes there): got {float(gf[s, h, t, d])!r}, "
                       f"want {float(w[s, h, t, d])!r}")
    return "; ".join(out) if out else None


# ---------------------------------------------------------------- the epilogue's addressing, with planted faults
#: the planted faults of ``epi_mirror`` (module doc, "Fused QKV geometries")
QKV_FAULTS = ("hkv", "tph", "idle", "d5", "b2")


def _kfrag(t, d, hd: int, drop_d5: bool = False):
    """common.h kfrag_off on tensors."""
    blk = (t >> 4) * (hd >> 5) + (0 if drop_d5 else (d >> 5))
    return blk * 512 + ((t & 15) + 16 * ((d & 31) >> 3)) * 8 + (d & 7)


def _vfrag(t, d, hd: int):
    """common.h vfrag_off on tensors."""
    return ((t >> 5) * (hd >> 4) + (d >> 4)) * 512 + ((d & 15) + 16 * ((t & 15) >> 2)) * 8 + 4 * ((t >> 4) & 1) + (t & 3)


def epi_mirror(acc: torch.Tensor, bias: torch.Tensor, slot: torch.Tensor, pos: torch.Tensor, cos: torch.Tensor,
               sin: torch.Tensor, geo: Geo, S: int, kv8: bool = False, fault: Optional[str] = None,
               sentinel: float = -7.0):
    """A host mirror of gemm_epi.h's EPI_QKV_ROPE addressing (``epi_load_at`` + ``epi_store``): from the exact
    accumulators acc [M, N] int64 (kernel row order) the q buffer [M, H hd] and the FRAGMENT-MAJOR caches
    kc [S, Hkv, T_max, hd], vtc [S, Hkv, hd, T_max], walked as the kernel walks them -- per 16-row tile gt and lane
    group lane >> 4 (4 accumulator rows nsub.., the RoPE partner rows + 8 from lane + 32).  ``fault``: None, or one of
    QKV_FAULTS planted -- "hkv": Hkv dropped from the cache bases; "tph": tiles per head rounded down to a power of
    two; "idle": the slot >= 0 guards dropped (an idle row writes q and, as slot 0, the caches); "d5": the d >> 5
    term of kfrag_off dropped; "b2": the partner rows' bias taken from b1's rows.  A faulty store that leaves the
    buffer is dropped (the mirror must not fault; the value is then missing where it belongs)."""
    assert fault is None or fault in QKV_FAULTS
    H, Hkv, hd, T = geo
    M, N = acc.shape
    bf = lambda t: t.bfloat16().float()  # noqa: E731
    cache = (lambda t: t.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()) if kv8 else (lambda t: t)
    q = torch.full((M, H * hd), sentinel)
    kc, vt = torch.zeros(S * Hkv * T * hd), torch.zeros(S * Hkv * hd * T)
    tph = hd >> 4
    if fault == "tph":
        tph = 1 << (tph.bit_length() - 1)
    qt, kt, half = H * tph, Hkv * tph, hd >> 1
    hkv_b = 1 if fault == "hkv" else Hkv
    rows = (torch.ones(M, dtype=torch.bool) if fault == "idle" else slot >= 0).nonzero().flatten()
    sl, p = slot[rows].long().clamp(min=0), pos[rows].long()
    f, b, ar4 = acc.float()[rows], bias.float(), torch.arange(4)

    def store(buf, idx, val):
        ok = (idx >= 0) & (idx < buf.numel())
        buf[idx[ok]] = val[ok]

    for gt in range(N // 16):
        for lg in range(4):
            nsub = lg * 4
            n1 = gt * 16 + nsub + ar4
            n2 = gt * 16 + ((nsub + 8) & 15) + ar4
            b1, b2 = b[n1], b[n1 if fault == "b2" else n2]
            if gt < qt + kt:
                if lg >= 2:
                    continue
                head, it = gt // tph, gt % tph
                j = it * 8 + nsub + ar4
                v1, v2 = bf(f[:, n1] + b1), bf(f[:, n1 + 8] + b2)  # lane + 32 holds rows nsub + 8..
                c, s = cos[p][:, j], sin[p][:, j]
                y1, y2 = bf(v1 * c - v2 * s), bf(v2 * c + v1 * s)
                if head < H:
                    q[rows[:, None], head * hd + j] = y1
                    q[rows[:, None], head * hd + j + half] = y2
                else:
                    base = ((sl * hkv_b + (head - H)) * T * hd)[:, None]
                    store(kc, base + _kfrag(p[:, None], j[None, :], hd, fault == "d5"), cache(y1))
                    store(kc, base + _kfrag(p[:, None], (j + half)[None, :], hd, fault == "d5"), cache(y2))
            else:
                vr = (gt - qt - kt) * 16 + nsub
                kh, d = vr // hd, vr % hd
                off = (sl * hkv_b + kh) * hd * T + _vfrag(p, d, hd)
                store(vt, off[:, None] + ar4 * 8, cache(bf(f[:, n1] + b1)))
    return q, kc.view(S, Hkv, T, hd), vt.view(S, Hkv, hd, T)


def unpack_caches(kc: torch.Tensor, vt: torch.Tensor):
    """Fragment-major caches (fp32 values) -> natural K, V [S, Hkv, T_max, hd] on the host."""
    from cain_amd import ops
    return ops.unpack_kcache(kc).cpu(), ops.unpack_vcache(vt).cpu()


#: where each planted fault shows, geometry by geometry ("toy" = QKV_GEO with the rows of QKV_CASES); checked by
#: tests/test_exact_cpu.py, which requires a report where True and silence where False
QKV_FAULT_SHOWS = {
    "toy": {"hkv": False, "tph": False, "idle": False, "d5": False, "b2": True},
    "phi3": {"hkv": True, "tph": True, "idle": True, "d5": True, "b2": True},
    "gqa": {"hkv": True, "tph": False, "idle": True, "d5": True, "b2": True},
    "gemma": {"hkv": False, "tph": False, "idle": True, "d5": True, "b2": True},
}


# ---------------------------------------------------------------- row ops: quant_rows, embed, rmsnorm
QR_CHUNK = 2048            # elements per register chunk of quant_rows_kernel: 256 threads x 8 (wgemm8.hip)
QR_MAXK = 12 * QR_CHUNK    # 24,576
#: one thread; exactly one chunk; one vector into chunk 1; around chunk 7; around the end of the last chunk
QR_KS = (8, 2048, 2056, 14336, 14344, 24568, 24576)
QR_MS = (1, 5)
QR_REFUSED = (24584, 12)   # past QR_MAXK; no whole 8-element vectors
E4M3_MAX = 448.0


def e4m3_quant(y: torch.Tensor, away: bool = False) -> torch.Tensor:
    """fp64 values -> the nearest e4m3 values (fp64), saturating at +-448, written out from the format: 3 mantissa
    bits above 2^-6, a fixed step of 2^-9 below.  Ties go to the even code, or away from zero with ``away`` (the
    planted wrong rounding of tests/test_rowops_exact_cpu.py)."""
    a = y.double().abs().clamp(max=E4M3_MAX)
    e = (torch.frexp(a)[1] - 1).clamp(min=-6)  # floor(log2 a), held at the smallest normal's exponent
    step = torch.pow(2.0, (e - 3).double())
    r = a / step
    return torch.copysign((torch.floor(r + 0.5) if away else torch.round(r)) * step, y.double())


def e4m3_bytes(v: torch.Tensor) -> torch.Tensor:
    """Exactly representable values -> their e4m3 bytes."""
    b = v.float().to(torch.float8_e4m3fn)
    assert torch.equal(b.double(), v.double())
    return b.view(torch.uint8)


def quant_scale(x: torch.Tensor, drop_chunk: Optional[int] = None):
    """(scale, inv) fp32 [M] of quant_rows: scale = fp32(amax / 448), 1 for a zero row; inv = fp32(1 / scale)."""
    xf = x.float().clone()
    if drop_chunk is not None:
        xf[:, drop_chunk * QR_CHUNK:(drop_chunk + 1) * QR_CHUNK] = 0
    amax = xf.abs().amax(1)
    scale = torch.where(amax > 0, amax / torch.tensor(E4M3_MAX), torch.ones_like(amax))
    return scale, 1.0 / scale


def quant_rows_ref(x: torch.Tensor, norm: bool = False, eps: float = 1e-6, away: bool = False,
                   drop_chunk: Optional[int] = None):
    """Reference of ops.quant_rows on bf16 rows x [M, K]: (bytes uint8 [M, K], xs fp64 [M]) --
    bytes = e4m3_rne(clamp(fp32(x) * inv, +-448)) by PyTorch's float8_e4m3fn conversion, xs = scale x
    (rsqrt(mean x^2 + eps) in fp64 if norm else 1), scale and inv as ``quant_scale``.  Planted faults for the CPU
    twin: ``away`` rounds ties away from zero; ``drop_chunk`` leaves one 2048-element chunk out of the row
    statistics (amax and the sum of squares)."""
    assert x.dtype == torch.bfloat16
    scale, inv = quant_scale(x, drop_chunk)
    y = (x.float() * inv[:, None]).clamp(-E4M3_MAX, E4M3_MAX)
    b = e4m3_bytes(e4m3_quant(y, away=True)) if away else y.to(torch.float8_e4m3fn).view(torch.uint8)
    xs = scale.double()
    if norm:
        xd = x.double().clone()
        if drop_chunk is not None:
            xd[:, drop_chunk * QR_CHUNK:(drop_chunk + 1) * QR_CHUNK] = 0
        xs = xs * torch.rsqrt(xd.pow(2).sum(1) / x.shape[1] + eps)
    return b, xs


def _e4m3_specials() -> torch.Tensor:
    """Magnitudes (fp64, <= 448, at most 8 significant bits) that a quantiser gets wrong first: every tie between
    two e4m3 codes of each binade, to the even code below and above (17/16 -> 1, 19/16 -> 5/4, ..., 432 -> 448); the
    subnormal range -- its codes k 2^-9, their ties (2k + 1) 2^-10 (2^-10 itself -> 0), values that vanish or round
    up to 2^-9; the values that round up to 448."""
    v = [(2 * n + 1) / 16.0 * 2.0 ** k for k in range(-6, 9) for n in range(8, 16)]
    v += [(2 * k + 1) * 2.0 ** -10 for k in range(8)] + [k * 2.0 ** -9 for k in range(1, 8)]
    v += [0.75 * 2.0 ** -10, 1.5 * 2.0 ** -10, 2.0 ** -11, 2.0 ** -12, 1.25 * 2.0 ** -9, 1.75 * 2.0 ** -9]
    v += [446.0, 440.0, 434.0, 430.0, 416.0]  # 448 itself is planted: the row maximum, in the last vector only
    return torch.tensor([a for a in v if a < E4M3_MAX], dtype=torch.float64)


def quant_exact_rows(M: int, K: int, seed: int):
    """(x bf16 [M, K], e [M]) of the exact family: row m holds y 2^e[m] with |y| <= 448 of at most 8 significant bits
    and a planted +448 and -448 in the row's last vector (nowhere else), so amax = 448 2^e, scale = 2^e and inv = 2^-e exactly, and the bytes
    are e4m3(y).  y: ``_e4m3_specials`` at the row's first vector, at both sides of every chunk boundary, in the last
    vector and at random places, +-0, and m 2^k (m in 128..255, k in -16..0) elsewhere; random signs.  With five rows,
    row 2 is all zero (+0 and -0): scale 1."""
    g = _gen(seed)
    y = _randint(g, 128, 255, (M, K)).double() * torch.pow(2.0, _randint(g, -16, 0, (M, K)).double())
    y[torch.rand(M, K, generator=g) < 1.0 / 16] = 0.0
    sp = _e4m3_specials()
    edges = [k for c in range(1, -(-K // QR_CHUNK)) for k in (c * QR_CHUNK - 1, c * QR_CHUNK)]
    e = torch.empty(M, dtype=torch.long)
    for m in range(M):
        where = list(range(min(8, K))) + edges + list(range(max(K - 8, 0), K))
        where += torch.randint(0, K, (min(K, 3 * len(sp)),), generator=g).tolist()
        where = torch.tensor(where)
        y[m, where] = sp[(torch.arange(len(where)) + 7 * m + seed) % len(sp)]
    y = y * (_randint(g, 0, 1, (M, K)) * 2 - 1).double()  # signs, of the zeros too
    for m in range(M):
        e[m] = (seed + 3 * m) % 10 - 6  # -6..3
        y[m, K - 1 - (seed + m) % 8] = E4M3_MAX if (seed + m) % 2 else -E4M3_MAX
        y[m, K - 1 - (seed + m + 3) % 8] = -E4M3_MAX if (seed + m) % 2 else E4M3_MAX
    x = y * torch.pow(2.0, e.double())[:, None]
    if M == 5:
        x[2] = torch.where(torch.rand(K, generator=g) < 0.5, 0.0, -0.0).double()
    xb = x.bfloat16()
    assert torch.equal(xb.double(), x), "the exact family must be exact in bf16"
    return xb, e


def quant_general_rows(M: int, K: int, seed: int) -> torch.Tensor:
    """Random bf16 rows, 3 x randn: amax is no power of two, so scale and inv round."""
    return (3.0 * torch.randn(M, K, generator=_gen(seed))).bfloat16()


def quant_norm_rows(M: int, K: int, seed: int) -> torch.Tensor:
    """Sparse integer rows for the folded RMSNorm factor: min(16, K) non-zeros in +-1..+-4 per row, so the sum of
    squares (<= 256) is an exact integer in fp32 in any order.  They sit at the row's first and last element, in
    each of the four waves' ranges of one chunk (elements 512 w.. of it) and on both sides of chunk boundaries --
    the last boundary always, the others in turn over the rows; the rest at random places."""
    g = _gen(seed)
    x = torch.zeros(M, K, dtype=torch.float64)
    nchunk = -(-K // QR_CHUNK)
    for m in range(M):
        where = [0, K - 1]
        c0 = (m + seed) % nchunk
        where += [k for w in range(4) for k in (c0 * QR_CHUNK + 512 * w + int(torch.randint(0, 512, (1,), generator=g)),)
                  if k < K]
        bounds = [nchunk - 1] + [1 + (m + seed + i) % max(1, nchunk - 1) for i in range(nchunk)]
        for c in bounds:
            if 0 < c < nchunk:
                where += [c * QR_CHUNK - 1, c * QR_CHUNK]
        where = list(dict.fromkeys(where))[:16]
        for k in torch.randperm(K, generator=g).tolist():
            if len(where) >= min(16, K):
                break
            if k not in where:
                where.append(k)
        val = _randint(g, 1, 4, (len(where),)) * (_randint(g, 0, 1, (len(where),)) * 2 - 1)
        x[m, torch.tensor(where)] = val.double()
    return x.bfloat16()


def _e4m3_code(b: torch.Tensor) -> torch.Tensor:
    """e4m3 bytes -> signed code numbers (adjacent values differ by 1; +0 and -0 are both 0)."""
    i = b.to(torch.int32)
    return torch.where(i >= 128, -(i & 127), i)


def quant_exact_mismatch(x: torch.Tensor, got8: torch.Tensor, gotxs: torch.Tensor) -> Optional[str]:
    """The exact family's comparator: bytes and (un-normed) scales equal to ``quant_rows_ref`` bit for bit."""
    ref8, refxs = quant_rows_ref(x)
    rep = mismatches(got8.cpu().to(torch.int32), ref8.to(torch.int32))
    if rep is not None:
        c = int((got8.cpu() != ref8).nonzero()[0][1])
        return f"bytes (chunk {c // QR_CHUNK}, thread {c % QR_CHUNK // 8}): {rep}"
    rep = mismatches(gotxs.cpu().double()[:, None], refxs[:, None])
    return None if rep is None else f"scale: {rep}"


def quant_general_mismatch(x: torch.Tensor, got8: torch.Tensor, gotxs: torch.Tensor):
    """The general family's comparator: (number of bytes that differ from the reference's, report or None).  Per
    element |e4m3(x8) scale - x| <= max(2^-4 |y|, 2^-10) scale (1 + 2^-20) with y = x inv -- half an e4m3 step,
    normal or subnormal, with a margin for the two fp32 roundings of scale and inv; the bytes at most one code from
    the reference's; the scale the reference's bit for bit (amax / 448 is one correctly rounded fp32 division)."""
    ref8, refxs = quant_rows_ref(x)
    scale, inv = quant_scale(x)
    g8 = got8.cpu()
    ndiff = int((g8 != ref8).sum())
    rep = mismatches(gotxs.cpu().double()[:, None], refxs[:, None])
    if rep is not None:
        return ndiff, f"scale: {rep}"
    y = x.double() * inv.double()[:, None]
    s = scale.double()[:, None]
    deq = g8.view(torch.float8_e4m3fn).double() * s
    over = (deq - x.double()).abs() - torch.maximum(2.0 ** -4 * y.abs(), torch.tensor(2.0 ** -10, dtype=torch.float64)) \
        * s * (1 + 2.0 ** -20)
    over = torch.where(over.isnan(), torch.tensor(float("inf"), dtype=torch.float64), over)  # an e4m3 NaN byte
    if float(over.max()) > 0:
        r, c = divmod(int(over.argmax()), x.shape[1])
        return ndiff, (f"{int((over > 0).sum())} elements past half an e4m3 step; worst at row {r}, column {c} (chunk "
                       f"{c // QR_CHUNK}): x {float(x[r, c])!r}, byte {int(g8[r, c]):#04x}, reference {int(ref8[r, c]):#04x}")
    far = (_e4m3_code(g8) - _e4m3_code(ref8)).abs() > 1
    if bool(far.any()):
        r, c = (int(v) for v in far.nonzero()[0])
        return ndiff, f"row {r}, column {c}: byte {int(g8[r, c]):#04x} is more than one code from {int(ref8[r, c]):#04x}"
    return ndiff, None


QR_NORM_RTOL = 2.0 ** -21  # 8 fp32 ulp: rms_inv is one v_rcp_f32 and one v_rsq_f32 (~1 ulp each) + 3 roundings


def quant_norm_mismatch(x: torch.Tensor, gotxs: torch.Tensor, eps: float) -> Optional[str]:
    """xs with the RMSNorm factor folded in, against the fp64 reference to a relative 2^-21."""
    _, refxs = quant_rows_ref(x, norm=True, eps=eps)
    rel = (gotxs.cpu().double() - refxs).abs() / refxs
    r = int(rel.argmax())
    if not float(rel[r]) <= QR_NORM_RTOL:
        return f"row {r}: xs {float(gotxs[r])!r}, want {float(refxs[r])!r}: off by {float(rel[r]) * 2 ** 24:.2f} x 2^-24"
    return None


EMBED_DS = (8, 2040, 2048, 2056, 3584)  # one vector; one short of / exactly / one past a full round of 256 threads
EMBED_MS = (1, 300)
NORM_DS = (8, 2048, 8192, 8200, 16384)  # 8200 and 16384 run rmsnorm_kernel<512>; 8200 leaves its second round partial
NORM_REFUSED = (16392, 12)


def embed_scales(d: int):
    """1 (a copy) and sqrt(d) rounded to bf16, as the engine passes for Gemma."""
    return 1.0, float(torch.tensor(float(d)).sqrt().bfloat16())


def embed_case(M: int, d: int, seed: int, rows: int = 37):
    """(table bf16 [rows, d], finite: randn over 14 binades; tok int32 [M]: row 0 first, the last row second when
    M > 1 and last, repeats in between)."""
    g = _gen(seed)
    E = (torch.randn(rows, d, generator=g) * torch.pow(2.0, _randint(g, -10, 3, (rows, d)).float())).bfloat16()
    assert bool(E.float().isfinite().all())
    tok = torch.randint(0, rows, (M,), generator=g).int()
    tok[0] = 0
    if M > 1:
        tok[1] = tok[-1] = rows - 1
        tok[M // 2] = tok[M // 2 - 1]
    return E, tok


def embed_ref(E: torch.Tensor, tok: torch.Tensor, scale: float) -> torch.Tensor:
    """bf16(fp32(E[tok]) x scale): one fp32 product, one round-to-nearest-even."""
    return (E[tok.long()].float() * scale).bfloat16()


def bits16(t: torch.Tensor) -> torch.Tensor:
    """bf16 -> its 16 bits as int32 (so that -0 and +0 differ)."""
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def bf16_ord(t: torch.Tensor) -> torch.Tensor:
    """bf16 -> integers in value order: adjacent bf16 numbers differ by 1 (+0 and -0 are both 0)."""
    i = bits16(t)
    return torch.where(i >= 0x8000, -(i & 0x7FFF), i)


def rmsnorm_case(M: int, d: int, seed: int):
    """(x bf16 [M, d] of integers -16..16: the sum of squares is below 16384 x 256 = 2^22, exact in fp32 in any order;
    gain bf16 [d], randn)."""
    g = _gen(seed)
    return _randint(g, -16, 16, (M, d)).to(torch.bfloat16), torch.randn(d, generator=g).bfloat16()


def rmsnorm_ref(x: torch.Tensor, gain: torch.Tensor, eps: float) -> torch.Tensor:
    """bf16(bf16(x inv) g) with inv = rsqrt(mean x^2 + eps) in fp64."""
    xd = x.double()
    inv = torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps)
    return ((xd * inv).bfloat16().double() * gain.double()).bfloat16()


def rmsnorm_mismatch(got: torch.Tensor, x: torch.Tensor, gain: torch.Tensor, eps: float):
    """(number of elements that differ from ``rmsnorm_ref`` at all, report or None): every output within one bf16
    step of the reference (the kernel's inv, ~8 fp32 ulp from the fp64 one, may flip a rounding)."""
    ref = rmsnorm_ref(x, gain, eps)
    steps = (bf16_ord(got.cpu()) - bf16_ord(ref)).abs()
    steps = torch.where(got.cpu().float().isfinite(), steps, torch.full_like(steps, 1 << 16))
    ndiff = int((steps > 0).sum())
    if int(steps.max()) > 1:
        r, c = (int(v) for v in (steps > 1).nonzero()[0])
        return ndiff, (f"{int((steps > 1).sum())} elements more than one bf16 step off; first at row {r}, column {c} "
                       f"(vector {c // 8}): got {float(got[r, c])!r}, want {float(ref[r, c])!r}")
    return ndiff, None


if __name__ == "__main__":  # regenerate TILE_FLOORS
    print("TILE_FLOORS: Dict[str, float] = {")
    for fam_, kind_ in soft_keys():
        print(f'    "{fam_}/{kind_}": {measure_floor(fam_, kind_):.4e},')
    print("}")
