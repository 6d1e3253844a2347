"""Host-side checks of ``tests/exact.py``: the comparators flag single-tile faults that the whole-matrix relative
error lets through, the integer generators decode to what the project's own decoders return, and every case of
``tests/test_gemm_exact_gpu.py`` stays inside the bounds that make fp32 accumulation exact."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).parent))

import exact  # noqa: E402
from cain_amd.models.q4 import dequantize_q4  # noqa: E402
from cain_amd.models.weights import dequantize_fp8_rows, dequantize_mxfp4  # noqa: E402


def rel_err(a, b):  # the suite's whole-matrix criterion
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


# ---------------------------------------------------------------- the comparators fire
N, K, M = 6144, 4096, 16
ROW, TILE = 5, 37  # where the faults are planted


def _product(n, k, m):
    g = torch.Generator().manual_seed(0)
    W = (torch.randn(n, k, generator=g, dtype=torch.float64) * 0.02).bfloat16().double()
    x = torch.randn(m, k, generator=g, dtype=torch.float64).bfloat16().double()
    r = torch.randn(m, n, generator=g, dtype=torch.float64).bfloat16().double()
    return x, W, r, x @ W.t()


@pytest.fixture(scope="module")
def gemm():
    """The tile faults on the issue's 16-row shape; the wrong row among 256 rows (1 / 16 of the norm)."""
    return {"few": _product(N, K, M), "tall": _product(1024, 256, 256)}


def _faults(products):
    x, W, r, ref = products["few"]
    tall = products["tall"][3]
    cols = slice(16 * TILE, 16 * TILE + 16)
    f1 = ref.clone()  # a tile missing one 128-wide k-quad of its sum
    f1[:, cols] -= x[:, 1024:1152] @ W[cols, 1024:1152].t()
    f2 = tall.clone()  # one row scaled by 1.1
    f2[ROW] *= 1.1
    f3 = ref.clone()  # two 8-column halves of one tile swapped
    f3[ROW, cols] = torch.cat([ref[ROW, 16 * TILE + 8:16 * TILE + 16], ref[ROW, 16 * TILE:16 * TILE + 8]])
    f4 = ref + r      # residual added twice in one tile
    f4[ROW, cols] += r[ROW, cols]
    return {"kquad": (f1, ref), "row": (f2, tall), "halves": (f3, ref), "resid2": (f4, ref + r)}


@pytest.mark.parametrize("fault", ["kquad", "row", "halves", "resid2"])
def test_comparators_flag_single_tile_faults(gemm, fault):
    bad, good = _faults(gemm)[fault]
    floor = exact.tile_err(good.bfloat16(), good)
    # bf16 rounding alone: at most 2^-9 relative per element, so 2^-9 x (the tile's rms / the global rms), and a
    # Gaussian tile of 16 stays below 3 global rms
    assert floor < 3 * 2.0 ** -9
    e = exact.tile_errs(bad.bfloat16(), good)
    print(fault, "tile_err", float(e.max()), "floor", floor, "rel_err", rel_err(bad.bfloat16(), good))
    assert float(e.max()) > exact.FLOOR_FACTOR * floor
    r, t = exact.worst_tile(bad.bfloat16(), good)
    assert t == TILE or fault == "row"
    assert r == ROW or fault == "kquad"
    # the exact comparator names the tile too
    rep = exact.mismatches(bad.bfloat16(), good.bfloat16())
    assert rep is not None and "differ" in rep
    rr, tt = exact.first_bad_tile(bad.bfloat16(), good.bfloat16())
    if fault == "kquad":
        assert (rr, tt) == (0, TILE) and f"tile {TILE}:" in rep
    elif fault == "row":
        assert rr == ROW and f"row {ROW}," in rep
    else:
        assert (rr, tt) == (ROW, TILE) and f"row {ROW}," in rep and f"tile {TILE}:" in rep
    assert exact.mismatches(good.bfloat16(), good.bfloat16()) is None


def test_whole_matrix_error_misses_them(gemm):
    """What the new checks add: faults 1 and 2 pass every ``rel_err < 1e-2`` assertion of the older GPU tests."""
    f = _faults(gemm)
    for name in ("kquad", "row"):
        bad, good = f[name]
        assert rel_err(bad.bfloat16(), good) < 1e-2, name


# ---------------------------------------------------------------- the generators decode correctly
def _decode(fam, ew, n, k):
    if fam in ("w8", "w8a8"):
        return dequantize_fp8_rows(ew.raw["q"], ew.raw["scale"])
    if fam in ("w4", "w4a8"):
        return dequantize_mxfp4(ew.raw["codes"], ew.raw["scales"])
    return dequantize_q4(ew.raw["blocks"], {"q4_0": 0, "q4_k": 1, "q6": exact.Q6_FMT}[fam], n, k)


GEN_OPTIONS = [(f, kw) for f in ("w8", "w8a8", "w4", "w4a8", "q4_0", "q4_k", "q6")
               for kw in ({}, {"small": True}, {"gateup": True})
               if not (("small" in kw and f not in ("q4_k", "q6", "w8", "w8a8")) or ("gateup" in kw and f == "q6"))]


@pytest.mark.parametrize("fam,kw", GEN_OPTIONS, ids=lambda v: str(v))
def test_generators_match_the_project_decoders(fam, kw):
    n, k = 64, 512
    ew = exact.GENERATORS[fam](n, k, 3, **kw)
    dec = _decode(fam, ew, n, k).double()
    assert torch.equal(dec * ew.den, ew.w.double())
    if ew.den == 1:
        assert torch.equal(dec, dec.round())
    if not kw and fam.startswith("q"):  # the whole range of every field is there
        assert int(ew.w.max()) > 60 or fam == "q4_0"
    if fam in ("w4", "w4a8"):
        assert set(ew.raw["codes"].unique().tolist()) == set(range(16))


def test_bf16_generator_packs_what_it_returns():
    from cain_amd.models.weights import unpack_mfma_a
    ew = exact.gen_bf16(64, 512, 3, gateup=True)
    assert torch.equal(unpack_mfma_a(ew.packed["wp"]).long(), ew.w)


@pytest.mark.parametrize("c", exact.CASES + exact.QKV_CASES, ids=lambda c: c.id)
def test_every_gpu_case_is_inside_the_exactness_bounds(c):
    """``exact.product`` asserts each bound; the operands must be exact in their formats too."""
    x, ew, ref = exact.case_inputs(c)
    assert torch.equal(x.to(torch.bfloat16).long(), x)
    if c.fam in ("w8a8", "w4a8"):  # amax = the planted value: scale and 1 / scale powers of two, the bytes exact
        plant = exact.a8_plant(c)
        assert plant in (448, 14, 7) and bool((x.abs().amax(1) == plant).all())
        x8 = x.float() * (448 // plant)
        assert torch.equal(x8.to(torch.float8_e4m3fn).float(), x8)
    if c.fam in ("w4", "w4a8"):
        assert int((x % 2).abs().max()) == 0
    if c.tag == "wide" or (c.tag == "qkv" and c.fam == "bf16" and c.M > 64):  # whatever plan the wide path picks
        for ks in (2, 3, 4, 8):
            exact.assert_fp16_slabs(x, ew, ks)
    if c.fam == "w8a8" and c.tag == "split":
        assert exact.a8_splits(c.N, c.K) > 1
        exact.assert_fp16_slabs(x, ew, exact.a8_splits(c.N, c.K), stage=128)
    if c.tag == "qkv8":
        assert int(ref.abs().max()) + 20 <= 448  # + the integer bias
    elif c.tag != "qkv":  # the bf16 rounding of the output is exercised (bf16 weights: by the bias)
        bias, r0 = exact.plain_extras(c)
        assert int((ref + bias).abs().max()) > 256 and int(r0.abs().max()) <= 128
        if c.fam != "bf16":
            assert int(ref.abs().max()) > 256


@pytest.mark.parametrize("fam", [f for f in exact.SOFT_SHAPES if f != "q6"])
def test_activation_cases_tell_the_activations_apart(fam):
    """The SiLU / GeLU per-tile cases sit where the non-linearity bends: the fp64 result of the WRONG activation
    (the other one, or ReLU) is past the case's limit -- in most (row, tile) units, not only in the worst."""
    refs = {k: exact.soft_case(fam, k)[2] for k in ("silu", "gelu", "relu")}
    for kind in ("silu", "gelu"):
        for wrong in ("silu", "gelu", "relu"):
            if wrong != kind:
                e = exact.tile_errs(refs[wrong], refs[kind])
                assert float(e.median()) > exact.tile_limit(fam, kind), (fam, kind, wrong, float(e.median()))


def test_tile_floors_are_current():
    for fam, kind in exact.soft_keys():
        got = exact.measure_floor(fam, kind)
        assert abs(got - exact.TILE_FLOORS[f"{fam}/{kind}"]) <= 1e-3 * got, (fam, kind, got)


# ---------------------------------------------------------------- fused QKV at the models' geometries
@pytest.mark.parametrize("c", exact.QKV_GEO_CASES, ids=lambda c: c.id)
def test_every_geometry_case_is_inside_the_exactness_bounds(c):
    """As above for ``QKV_GEO_CASES`` (``exact.product`` asserts each bound), and the rows of the launch are what the
    GPU test relies on: idle first and last rows, a shared slot across the block edges, one owner per write."""
    H, Hkv, hd, T = exact.case_geo(c)
    assert c.N == (H + 2 * Hkv) * hd and c.M == exact.QKV_GEO_ROWS[c.fam, c.K]
    x, ew, ref = exact.case_inputs(c)
    assert torch.equal(x.to(torch.bfloat16).long(), x)
    if c.fam in ("w8a8", "w4a8"):
        plant = exact.a8_plant(c)
        assert bool((x.abs().amax(1) == plant).all())
        x8 = x.float() * (448 // plant)
        assert torch.equal(x8.to(torch.float8_e4m3fn).float(), x8)
    if c.fam in ("w4", "w4a8"):
        assert int((x % 2).abs().max()) == 0
    if c.fam == "bf16" and c.M > 64:
        for ks in (2, 3, 4, 8):
            exact.assert_fp16_slabs(x, ew, ks)
    bias, slot, pos, S, cos, sin = exact.qkv_launch(c)
    if c.tag == "qkv8":
        assert int(ref.abs().max()) + 20 <= 448  # |k|, |v| <= 448 with the integer bias: no e4m3 saturation
    idle = slot < 0
    assert bool(idle[0]) and bool(idle[-1]) and c.M // 5 <= int(idle.sum()) <= c.M // 3 and bool((pos[idle] == 0).all())
    assert int(slot.max()) < S and 0 <= int(pos.min()) and int(pos.max()) == T - 1
    pairs = [(int(s), int(p)) for s, p in zip(slot, pos) if s >= 0]
    assert len(set(pairs)) == len(pairs)
    by_slot = {}
    for s, p in pairs:
        by_slot.setdefault(s, set()).add(p)
    assert any({15, 16, 31, 32, T - 1} <= ps for ps in by_slot.values())
    assert T % 32 == 0 and T & (T - 1)  # whole blocks, no power of two


def _mirror_report(c, fault):
    x, ew, ref = exact.case_inputs(c)
    geo = exact.case_geo(c)
    bias, slot, pos, S, cos, sin = exact.qkv_launch(c)
    kv8 = c.tag == "qkv8"
    want = exact.qkv_want(ref + bias, slot, pos, cos, sin, geo, S, kv8)
    q, kc, vt = exact.epi_mirror(ref, bias, slot, pos, cos, sin, geo, S, kv8, fault)
    kn, vn = exact.unpack_caches(kc, vt)
    return exact.qkv_mismatch(q, kn, vn, want, slot, pos, geo)


MIRROR_CASES = {"toy": [exact.qkv_case("w8", 1088, 5, kv8) for kv8 in (False, True)],
                **{geo: [exact.qkv_case("w8", 1088, 40, kv8, geo) for kv8 in (False, True)] for geo in exact.QKV_GEOS}}


@pytest.mark.parametrize("geo", list(MIRROR_CASES))
def test_epilogue_mirror_agrees_and_planted_faults_are_caught(geo):
    """The fault-free mirror of the epilogue's addressing leaves exactly what ``qkv_want`` expects (two independent
    statements of the epilogue: one by addresses, one by values); each planted fault is reported at every geometry
    where it can show and at no other -- ``exact.QKV_FAULT_SHOWS``: at the 2 / 1 / 32 geometry "hkv", "tph", "idle"
    and "d5" are invisible."""
    for c in MIRROR_CASES[geo]:
        assert _mirror_report(c, None) is None
        for fault in exact.QKV_FAULTS:
            rep = _mirror_report(c, fault)
            print(geo, c.tag, fault, rep)
            assert (rep is not None) == exact.QKV_FAULT_SHOWS[geo][fault], (geo, c.tag, fault, rep)
            if rep is not None:
                assert "slot" in rep and "position" in rep and ("row" in rep) and ("head" in rep)


def test_an_idle_row_fault_names_the_row():
    c = MIRROR_CASES["gqa"][0]
    rep = _mirror_report(c, "idle")
    assert rep.startswith("q:") and "first at row 0 (slot -1, position 0)" in rep
