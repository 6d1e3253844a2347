"""Every GEMM family against the exact int64 product of integer operands (``tests/exact.py``): fp32 outputs equal
it bit for bit, bf16 outputs equal its round-to-nearest-even, the fused QKV + RoPE + KV-append epilogue is a signed
permutation of it, on each forced kernel path (confirmed through the library's own query functions), twice per
path (tickets and counters reset).  A failure names the (row, 16-column tile).  Fused RMSNorm and the SiLU / GeLU
epilogues, which cannot be exact, are held to 3 x the per-tile rounding floor of their output type.

The fused QKV epilogue runs at the 2 / 1 / 32 head geometry on every path and row count (``exact.QKV_CASES``), and at
phi3's, a GQA and gemma's head shape with idle rows and shared slots (``exact.QKV_GEO_CASES``): there every family and
both cache types at one row count each, none left out; a failure names (row, head, tile, slot, position)."""
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

sys.path.insert(0, str(Path(__file__).parent))

import exact  # noqa: E402
from exact import Case  # noqa: E402
from cain_amd import ops  # noqa: E402

DEV = torch.device("cuda")
WS_DEV = torch.zeros(1, device=DEV).device  # the workspaces' cache key (the tensors' own device, with its index)
F32, BF16, RESID, QKV = ops.EPI_F32, ops.EPI_BF16, ops.EPI_RESID, ops.EPI_QKV_ROPE
A8 = ("w8a8", "w4a8")


@pytest.fixture(autouse=True)
def _switches():
    """Every switch the tests touch, back at its default afterwards."""
    inline0 = ops.wide_gemm_inline_mode()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:  # a GPU fault: nothing more may run on the device
        pytest.exit(f"GPU error, stopping the session: {exc}", returncode=3)
    ops.set_w4_variant(-1)
    ops.set_w4_split(0)
    ops.set_w4_occupancy(0)
    ops.set_skinny_split(1)
    ops.set_wide_gemm_min_m(64)
    ops.set_wide_gemm_variant(0)
    ops.set_wide_gemm_inline(inline0)
    ops.clear_wide_gemm_plans()


def dev(p):
    return {k: v.to(DEV) for k, v in p.items()}


def run(fam, p, x, n, epi, **kw):
    if fam == "bf16":
        return ops.skinny_gemm(p["wp"], x, n, epi, **kw)
    if fam == "w8":
        return ops.gemm_w8(p["wq"], p["scale"], x, n, epi, **kw)
    if fam == "w8a8":
        return ops.gemm_w8a8(p["wq"], p["scale"], x, n, epi, **kw)
    if fam == "w4":
        return ops.gemm_w4(p["wq"], p["wsc"], x, n, epi, **kw)
    if fam == "w4a8":
        return ops.gemm_w4a8(p["wq"], p["wsc"], x, n, epi, **kw)
    if fam in ("q4_0", "q4_k"):
        return ops.gemm_q4(0 if fam == "q4_0" else 1, p["wq"], p["sbuf"], x, n, epi, **kw)
    return ops.gemm_q6(p["wq"], p["sbuf"], x, n, epi, **kw)


def q_rows(fam, K, epi):
    lib = ops.load()
    return int((lib.cain_gemm_q6_rows if fam == "q6" else lib.cain_gemm_q4_rows)(K, epi))


def check_plain(c: Case, cmax: bool = False, tag: str = ""):
    """EPI_F32 (twice), EPI_BF16 + integer bias, EPI_RESID in place (twice from the same residual): all exact."""
    x, ew, ref = exact.case_inputs(c)
    p, xd = dev(ew.packed), x.to(torch.bfloat16).to(DEV)
    tag = f"{c.id} {tag}"
    for rep in range(2):
        kw = {}
        if cmax:
            kw["cmax"] = torch.full((c.M, c.N // 16), float("nan"), device=DEV)
        y = run(c.fam, p, xd, c.N, F32, **kw)
        assert y.dtype == torch.float32
        exact.assert_equal(y, ref.float(), f"{tag} f32 run {rep}")
        if cmax:  # the sampler's chunk maxima, across the launch boundaries
            exact.assert_equal(kw["cmax"], y.view(c.M, c.N // 16, 16).amax(-1), f"{tag} cmax run {rep}")
    bias, r0 = exact.plain_extras(c)
    y = run(c.fam, p, xd, c.N, BF16, bias=bias.float().to(DEV))
    exact.assert_equal(y, exact.to_bf16(ref + bias), f"{tag} bf16 + bias")
    for rep in range(2):
        r = r0.to(torch.bfloat16).to(DEV)
        run(c.fam, p, xd, c.N, RESID, out=r)
        exact.assert_equal(r, exact.to_bf16(ref + r0), f"{tag} resid run {rep}")  # added exactly once


def by(tag, fam=None):
    return [c for c in exact.CASES if c.tag == tag and (fam is None or c.fam == fam)]


ids = lambda c: c.id  # noqa: E731


# ---------------------------------------------------------------- bf16
@pytest.mark.parametrize("c", by("skinny"), ids=ids)
def test_bf16_skinny_unsplit(c):
    assert ops.gemm_ws_bytes(c.N, c.K, c.M) == 0  # no workspace: the unsplit skinny kernel
    check_plain(c)


@pytest.mark.parametrize("c", by("skinnysplit"), ids=ids)
def test_bf16_skinny_split_k(c):
    ops.set_skinny_split(0)
    assert ops.gemm_ws_bytes(c.N, c.K, c.M) == 0
    check_plain(c, tag="split off")
    ops.set_skinny_split(1)
    assert ops.gemm_ws_bytes(c.N, c.K, c.M) > 0 and c.M <= 16  # the split grid's slabs
    check_plain(c, tag="split on")
    torch.cuda.synchronize()
    assert int(ops._ws_cache[WS_DEV][:16384].count_nonzero()) == 0  # tickets back at zero


@pytest.mark.parametrize("c", by("batched"), ids=ids)
def test_bf16_batched(c):
    assert c.M > 16 and ops.gemm_ws_bytes(c.N, c.K, c.M) > 0 and not ops.wide_gemm_eligible(c.N, c.K, c.M)
    check_plain(c)
    torch.cuda.synchronize()
    assert int(ops._ws_cache[WS_DEV][:16384].count_nonzero()) == 0


@pytest.mark.parametrize("ks,variant", [(1, 0), (2, 0), (4, 0), (3, 4), (4, 4), (0, -1)])
@pytest.mark.parametrize("c", by("wide"), ids=ids)
def test_bf16_wide(c, ks, variant):
    """Unsplit and split plans on fp16 (variant 0) and fp32 (4) slabs; (0, -1): the default rule.  N = 208 is not a
    multiple of the 128-column block."""
    assert ops.wide_gemm_eligible(c.N, c.K, c.M) and c.N % 128
    if ks:
        ops.set_wide_gemm_plan(c.N, c.K, 256 if c.M > 128 else 128, ks, variant)
        assert ops.wide_gemm_plan(c.N, c.K, c.M) == (ks, variant)
    got_ks, got_var = ops.wide_gemm_plan(c.N, c.K, c.M)
    x, ew, _ = exact.case_inputs(c)
    if got_var == 0:
        exact.assert_fp16_slabs(x, ew, got_ks)
    check_plain(c, tag=f"plan ({got_ks}, {got_var})")
    torch.cuda.synchronize()
    # the batched path's tickets [0, 64 KiB) and the wide path's counters [64, 80 KiB) read zero at rest
    assert int(ops._ws_cache[WS_DEV][:80 * 1024 // 4].count_nonzero()) == 0


# ---------------------------------------------------------------- fp8 weights
@pytest.mark.parametrize("c", [c for c in exact.CASES if c.fam == "w8"], ids=ids)
def test_w8(c):
    check_plain(c, cmax=c.M <= 16)


# ---------------------------------------------------------------- MXFP4
def _w4_effective(var, K, M):
    """The W4Var index a forced variant runs as (a stream shape whose LDS copy cannot hold the rows falls back)."""
    if var >= 2 or (M <= 16 and M * K * 2 <= (49152 if var == 0 else 28672)):
        return var
    return None  # the rule's choice


@pytest.mark.parametrize("var", range(6))
@pytest.mark.parametrize("c", by("variants"), ids=ids)
def test_w4_every_variant(c, var):
    rule = ops.w4_variant(c.N, c.K, c.M, F32)
    ops.set_w4_variant(var)
    eff = _w4_effective(var, c.K, c.M)
    assert ops.w4_variant(c.N, c.K, c.M, F32) == (rule if eff is None else eff)
    check_plain(c, tag=f"variant {var}")


@pytest.mark.parametrize("c", by("lds"), ids=ids)
def test_w4_rule_on_both_sides_of_the_lds_copies(c):
    """Rows x K around the 4-wave kernel's 28 KiB and the 8-wave kernel's 48 KiB activation copy."""
    want = {7: 1, 8: 0, 12: 0, 13: 3}[c.M]  # W4S_4_4, W4S_8_4, W4S_8_4, W4T_4_4_1
    assert ops.w4_variant(c.N, c.K, c.M, F32) == want
    check_plain(c, cmax=want <= 1)


@pytest.mark.parametrize("ks", [1, 2, 3, 4])
@pytest.mark.parametrize("c", by("split", "w4"), ids=ids)
def test_w4_split_k(c, ks):
    ops.set_w4_split(ks)
    assert ops.w4_variant(c.N, c.K, c.M, F32) == 0 and ops.w4_split(c.N, c.K, c.M, F32) == ks
    check_plain(c, tag=f"ks {ks}")
    torch.cuda.synchronize()
    assert int(ops._W4_WS[WS_DEV][:16384].count_nonzero()) == 0  # tickets reset


@pytest.mark.parametrize("c", by("occupancy"), ids=ids)
def test_w4_persistent_grid_three_tiles_per_workgroup(c):
    ops.set_w4_occupancy(1)
    n_cu = torch.cuda.get_device_properties(DEV).multi_processor_count
    assert c.N // 16 >= 3 * n_cu and ops.w4_variant(c.N, c.K, c.M, F32) <= 1  # a stream shape, 1 workgroup per CU
    check_plain(c)


# ---------------------------------------------------------------- GGUF Q4_0 / Q4_K / Q6_K
@pytest.mark.parametrize("c", by("rows"), ids=ids)
def test_q4_q6_rows_across_launches(c):
    """M = rows, rows + 1, 2 rows + 1 per launch: the last launch is partial; K / 128 = 22 and 24 on either side
    of the 4-wave / 8-wave choice (at 22 quads the 1-row last launch runs on 4 waves, the full ones on 8)."""
    rows = q_rows(c.fam, c.K, F32)
    assert rows == exact.Q_ROWS[c.K] and c.M in (rows, rows + 1, 2 * rows + 1)
    assert 2 <= exact.Q_ROWS[3072] <= 8  # (at 22 quads no K has fewer than 9 rows: exact.Q_ROWS)
    assert q_rows(c.fam, c.K, BF16) == rows and q_rows(c.fam, c.K, RESID) == rows
    check_plain(c, cmax=True)


@pytest.mark.parametrize("M", [8, 9, 17])
def test_q6_nonzero_tile0(M):
    """The epilogue's tile offset: output columns, bias and residual start at tile 2; columns before it stay."""
    c = Case("q6", 48, 3072, M, "rows")
    x, ew, ref = exact.case_inputs(c)
    p, xd = dev(ew.packed), x.to(torch.bfloat16).to(DEV)
    t0, n_out = 2, 32 + c.N
    g = torch.Generator().manual_seed(M)
    out = torch.full((M, n_out), -7.0, device=DEV)
    ops.gemm_q6(p["wq"], p["sbuf"], xd, c.N, F32, out=out, tile0=t0)
    exact.assert_equal(out[:, 32:], ref.float(), "f32 tile0")
    assert bool((out[:, :32] == -7.0).all())
    bias = torch.randint(-300, 301, (n_out,), generator=g)
    out = torch.full((M, n_out), -7.0, device=DEV).bfloat16()
    ops.gemm_q6(p["wq"], p["sbuf"], xd, c.N, BF16, bias=bias.float().to(DEV), out=out, tile0=t0)
    exact.assert_equal(out[:, 32:], exact.to_bf16(ref + bias[32:]), "bf16 tile0")
    assert bool((out[:, :32] == -7.0).all())
    r0 = torch.randint(-128, 129, (M, n_out), generator=g)
    r = r0.to(torch.bfloat16).to(DEV)
    ops.gemm_q6(p["wq"], p["sbuf"], xd, c.N, RESID, out=r, tile0=t0)
    exact.assert_equal(r[:, 32:], exact.to_bf16(ref + r0[:, 32:]), "resid tile0")
    exact.assert_equal(r[:, :32], r0[:, :32].to(torch.bfloat16), "resid tile0: columns before it")


# ---------------------------------------------------------------- activation-quantised wide kernels
def _a8_quant(c, x):
    """quant_rows on a case's activations: amax = the planted 448 (7, 14): the scale is exactly 1 (2^-6, 2^-5) and
    the e4m3 bytes hold x / scale exactly (exact.int_x)."""
    plant = exact.a8_plant(c)
    x8, xs = ops.quant_rows(x.to(torch.bfloat16).to(DEV))
    exact.assert_equal(xs[:, None], torch.full((c.M, 1), plant / 448.0), f"{c.id} quant_rows scale")
    exact.assert_equal(x8.view(torch.float8_e4m3fn).float(), x.float() * (448 // plant), f"{c.id} quant_rows bytes")


def _a8_front(c):
    assert ops.w8a8_eligible(c.N, c.K, c.M)
    x, ew, ref = exact.case_inputs(c)
    _a8_quant(c, x)
    split = int(ops.load().cain_w8a8_ws_bytes(c.N, c.K, c.M)) > 80 * 1024  # slabs behind the counter regions
    assert split == (c.tag in ("split", "split16")) == (exact.a8_splits(c.N, c.K) > 1)
    return x, ew, ref


@pytest.mark.parametrize("c", [c for c in exact.CASES if c.fam in A8 and c.tag != "split16"], ids=ids)
def test_w8a8_w4a8(c):
    x, ew, _ = _a8_front(c)
    if c.tag == "split":
        exact.assert_fp16_slabs(x, ew, exact.a8_splits(c.N, c.K), stage=128)
    check_plain(c)


@pytest.mark.parametrize("c", by("split16"), ids=ids)
def test_w4a8_split_k_within_fp16_slab_rounding(c):
    """NOT exact: the split-K slabs are fp16, and MXFP4's +-6 times the planted 448 is past 2^11.  Each k range's
    partial rounds once to fp16 (relative 2^-11, |partial| <= the range's sum |x w|) and the fp32 sum of the widened
    partials is exact here, so per element |y - ref| <= 2^-11 sum_k |x_k w_k|; the bf16 outputs are held to 3 x the
    per-tile floor of bf16 rounding at this case (fp16's step is a quarter of bf16's)."""
    x, ew, ref = _a8_front(c)
    p, xd = dev(ew.packed), x.to(torch.bfloat16).to(DEV)
    bound = 2.0 ** -11 * (x.abs() @ ew.w.abs().t()).double() / ew.den
    ys = [run(c.fam, p, xd, c.N, F32) for _ in range(2)]
    assert torch.equal(ys[0], ys[1])
    over = (ys[0].cpu().double() - ref.double()).abs() - bound
    i = int(over.argmax())
    assert float(over.max()) <= 0, f"row {i // c.N}, column {i % c.N}, tile {i % c.N // 16}: over by {float(over.max())}"
    bias, r0 = exact.plain_extras(c)
    yb = run(c.fam, p, xd, c.N, BF16, bias=bias.float().to(DEV))
    r = r0.to(torch.bfloat16).to(DEV)
    run(c.fam, p, xd, c.N, RESID, out=r)
    for what, y, want in (("bf16 + bias", yb, ref + bias), ("resid", r, ref + r0)):
        floor = exact.tile_err(exact.to_bf16(want), want)
        e = exact.tile_err(y, want)
        print(f"{c.id} {what}: tile_err {e:.4e}, floor {floor:.4e}")
        assert e <= exact.FLOOR_FACTOR * floor, f"{what}: {e:.4e} > 3 x {floor:.4e} at (row, tile) {exact.worst_tile(y, want)}"


# ---------------------------------------------------------------- fused QKV + RoPE + KV append
def _qkv(c: Case, kv8: bool, tile0_v: bool = False, geo=None):
    """One fused-QKV case, twice: q, both caches and everything no row owns (idle rows' q, the rest of the caches)
    against ``exact.qkv_want``; a failure names (row, head, tile, slot, position)."""
    geo = exact.case_geo(c) if geo is None else geo
    H, Hkv, hd, T = geo
    assert c.N == exact.qkv_n(geo)
    x, ew, ref = exact.case_inputs(c)  # weight rows in the kernel's order (random rows: any order is a valid case)
    M = c.M
    bias, slot, pos, S, cos, sin = exact.qkv_launch(c)
    want = exact.qkv_want(ref + bias, slot, pos, cos, sin, geo, S, kv8, sentinel=-7.0, v_only=bool(tile0_v))
    p, xd = dev(ew.packed), x.to(torch.bfloat16).to(DEV)
    cdt = torch.uint8 if kv8 else torch.bfloat16
    for rep in range(2):
        kc = torch.zeros(S, Hkv, T, hd, device=DEV, dtype=cdt)
        vt = torch.zeros(S, Hkv, hd, T, device=DEV, dtype=cdt)
        q = torch.full((M, H * hd), -7.0, device=DEV).bfloat16()
        rope = dict(kc=kc, vtc=vt, slot=slot.to(DEV), pos=pos.to(DEV), cos_t=cos.to(DEV), sin_t=sin.to(DEV), H=H,
                    Hkv=Hkv, hd=hd)
        b = bias.float().to(DEV)
        if tile0_v:  # the V rows as a launch of their own behind the q / k rows (gemm_q6's tile offset)
            nv, t0 = Hkv * hd, (H + Hkv) * hd // 16
            ops.gemm_q6(tile0_v["wq"], tile0_v["sbuf"], xd, nv, QKV, bias=b, out=q, rope=rope, tile0=t0)
        elif c.fam == "bf16":
            ops.qkv_rope(p["wp"], xd, c.N, q, kc, vt, rope["slot"], rope["pos"], rope["cos_t"], rope["sin_t"], H, Hkv,
                         hd, bias=b)
        else:
            run(c.fam, p, xd, c.N, QKV, bias=b, out=q, rope=rope)
        kf = kc.view(torch.float8_e4m3fn).float() if kv8 else kc.float()
        vf = vt.view(torch.float8_e4m3fn).float() if kv8 else vt.float()
        kn, vn = exact.unpack_caches(kf, vf)
        report = exact.qkv_mismatch(q, kn, vn, want, slot, pos, geo)
        assert report is None, f"{c.id} run {rep}: {report}"


@pytest.mark.parametrize("c", exact.QKV_CASES, ids=ids)
def test_qkv_rope_is_a_signed_permutation(c):
    if c.fam in ("q4_0", "q4_k", "q6"):
        rows = q_rows(c.fam, c.K, QKV)
        assert rows == exact.QKV_ROWS[c.K] and c.M in (rows, rows + 1, 2 * rows + 1)
    if c.fam == "bf16" and c.M > 64:
        assert ops.wide_gemm_eligible(c.N, c.K, c.M)
        ks, variant = ops.wide_gemm_plan(c.N, c.K, c.M)
        if variant == 0:
            x, ew, _ = exact.case_inputs(c)
            exact.assert_fp16_slabs(x, ew, ks)
    if c.fam in A8:
        assert ops.w8a8_eligible(c.N, c.K, c.M)
        _a8_quant(c, exact.case_inputs(c)[0])
    _qkv(c, c.tag == "qkv8")


@pytest.mark.parametrize("c", exact.QKV_GEO_CASES, ids=ids)
def test_qkv_rope_at_the_models_geometries(c):
    """Every family's epilogue at phi3's, a GQA and gemma's head shape (``exact.QKV_GEOS``: 6 tiles per head, Hkv > 1,
    hd >> 5 up to 8, T_max = 96), with idle rows whose q must keep its sentinel and who add nothing to either cache,
    and rows sharing a slot at positions 15 / 16, 31 / 32 and T_max - 1 (``exact.qkv_rows``).  The bias stays in the
    kernel's row order, so b1 / b2 are checked per head.  One row count per family, across its row-block or launch
    boundary (``exact.QKV_GEO_ROWS``); no family is left out of any geometry."""
    if c.fam in ("q4_0", "q4_k", "q6"):
        rows = q_rows(c.fam, c.K, QKV)
        assert rows == exact.QKV_ROWS[c.K] and c.M == 2 * rows + 1
    if c.fam == "bf16" and c.M > 64:
        assert ops.wide_gemm_eligible(c.N, c.K, c.M)
        ks, variant = ops.wide_gemm_plan(c.N, c.K, c.M)
        if variant == 0:
            x, ew, _ = exact.case_inputs(c)
            exact.assert_fp16_slabs(x, ew, ks)
    elif c.fam == "bf16":
        assert (ops.gemm_ws_bytes(c.N, c.K, c.M) > 0) == (c.M > 16)  # batched above 16 rows, else the skinny kernel
    if c.fam in A8:
        assert ops.w8a8_eligible(c.N, c.K, c.M) and c.M > 128  # the 256-row tile
        _a8_quant(c, exact.case_inputs(c)[0])
    _qkv(c, c.tag == "qkv8")


#: one family per entry file: gemm.hip, gemm_w8.hip, gemm_w4.hip, gemm_qstream.hip, wgemm8.hip
REFUSED = [("bf16", 1056, 16), ("w8", 1088, 5), ("w4", 1920, 5), ("q6", 3072, 4), ("w8a8", 640, 40)]


@pytest.mark.parametrize("hd", [40, 24])
@pytest.mark.parametrize("fam,K,M", REFUSED, ids=lambda v: str(v))
def test_qkv_rope_refuses_head_sizes_it_cannot_tile(fam, K, M, hd):
    """hd = 40 ((hd / 2) % 8 != 0) and hd = 24 (hd % 16 != 0): ``gemm_args`` refuses, the entry returns an error
    before any launch of its own, and nothing is written (W8A8: ``quant_rows`` has run by then, into its own
    buffers)."""
    H, Hkv, T = 2, 2, 64
    N = (H + 2 * Hkv) * hd  # 240, 144: whole 16-row tiles
    ew = exact.GENERATORS[fam](N, K, 1)
    p = dev(ew.packed)
    xd = exact.int_x(M, K, 2, plant=exact.a8_plant(Case(fam, N, K, M))).to(torch.bfloat16).to(DEV)
    kc = torch.zeros(M, Hkv, T, hd, device=DEV, dtype=torch.bfloat16)
    vt = torch.zeros(M, Hkv, hd, T, device=DEV, dtype=torch.bfloat16)
    q = torch.full((M, H * hd), -7.0, device=DEV).bfloat16()
    cos, sin = exact.unit_rope_tables(T, hd, 3)
    rope = dict(kc=kc, vtc=vt, slot=torch.arange(M, dtype=torch.int32, device=DEV),
                pos=torch.zeros(M, dtype=torch.int32, device=DEV), cos_t=cos.to(DEV), sin_t=sin.to(DEV), H=H, Hkv=Hkv,
                hd=hd)
    with pytest.raises(RuntimeError, match=r"failed \(rc="):
        if fam == "bf16":
            ops.qkv_rope(p["wp"], xd, N, q, kc, vt, rope["slot"], rope["pos"], rope["cos_t"], rope["sin_t"], H, Hkv, hd)
        else:
            run(fam, p, xd, N, QKV, out=q, rope=rope)
    assert bool((q == -7.0).all()) and int(kc.count_nonzero()) == 0 and int(vt.count_nonzero()) == 0


@pytest.mark.parametrize("M", [4, 9])
@pytest.mark.parametrize("kv8", [False, True])
def test_q6_v_rows_as_their_own_launch(M, kv8):
    """gemm_q6 with tile0 = (H + Hkv) hd / 16 on the V rows alone: V^T cache written, q and the K cache untouched."""
    c = exact.qkv_case("q6", 3072, M, kv8)
    _, ew, _ = exact.case_inputs(c)
    nq = (exact.QKV_H + exact.QKV_HKV) * exact.QKV_HD
    # the same blocks' V rows, packed as a matrix of their own
    from cain_amd.models.q4 import pack_q6, q6_fields
    vb = ew.raw["blocks"][nq:].contiguous()
    wq, sb = pack_q6(q6_fields(vb, exact.QKV_HKV * exact.QKV_HD, c.K))
    _qkv(c, kv8, tile0_v={"wq": wq.to(DEV), "sbuf": sb.to(DEV)})


# ---------------------------------------------------------------- where exactness is impossible: the per-tile metric
def _soft_run(fam, kind):
    x, ew, ref = exact.soft_case(fam, kind)
    N, K, M = exact.SOFT_SHAPES[fam]
    base = exact.soft_base(fam)
    p, xd = dev(ew.packed), x.to(torch.bfloat16).to(DEV)
    assert torch.equal(xd.cpu().double(), x)  # the activations are exact in bf16
    if fam == "bf16":
        assert ops.gemm_ws_bytes(N, K, M) == 0
    elif fam == "bf16_batched":
        assert ops.gemm_ws_bytes(N, K, M) > 0 and not ops.wide_gemm_eligible(N, K, M)
    elif fam == "bf16_wide":
        # unsplit: the default plan's fp16 split-K slabs round each partial to 2^-11, far above an fp32 output's floor
        ops.set_wide_gemm_plan(N, K, 256 if M > 128 else 128, 1, 0)
        assert ops.wide_gemm_plan(N, K, M) == (1, 0)
    elif fam == "bf16_wide_split":  # the split-K combine (with the fused norm's row sums of squares), fp32 slabs
        ops.set_wide_gemm_plan(N, K, 256 if M > 128 else 128, 2, 4)
        assert ops.wide_gemm_plan(N, K, M) == (2, 4)
    if kind == "norm":
        y = run(base, p, xd, N, F32, norm=True, eps=1e-6)
    else:
        y = run(base, p, xd, N, ops.EPI_SILU if kind == "silu" else ops.EPI_GELU)
    return y, ref


@pytest.mark.parametrize("fam,kind", list(exact.soft_keys()), ids=lambda v: str(v))
def test_norm_and_activation_epilogues_per_tile(fam, kind):
    y, ref = _soft_run(fam, kind)
    assert y.dtype == (torch.float32 if kind == "norm" else torch.bfloat16) and y.shape == ref.shape
    e, lim = exact.tile_err(y, ref), exact.tile_limit(fam, kind)
    r, t = exact.worst_tile(y, ref)
    print(f"{fam}/{kind}: tile_err {e:.4e} at row {r}, tile {t}; floor {exact.TILE_FLOORS[f'{fam}/{kind}']:.4e}, "
          f"limit {lim:.4e}")
    assert e <= lim, f"{fam}/{kind}: tile_err {e:.4e} > {lim:.4e} at row {r}, tile {t}"


@pytest.mark.parametrize("fam", ["bf16", "bf16_batched", "bf16_wide", "w8", "w4", "q4_0", "q4_k", "q6"])
def test_f32_outputs_within_the_summation_bound(fam):
    """Non-integer activations, fp32 output, no non-linearity: |y - ref| <= K 2^-24 sum_k |x_k w_k| per element."""
    N, K, M = exact.SOFT_SHAPES[fam]
    base = exact.soft_base(fam)
    ew = exact.GENERATORS[base](N, K, 5)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(6)).bfloat16()
    if fam == "bf16_wide":
        ops.set_wide_gemm_plan(N, K, 256 if M > 128 else 128, 2, 4)  # split, fp32 slabs
        assert ops.wide_gemm_plan(N, K, M) == (2, 4)
    y = run(base, dev(ew.packed), x.to(DEV), N, F32).cpu().double()
    ref = x.double() @ (ew.w.double() / ew.den).t()
    bound = exact.f32_bound(x.double(), ew)
    if base in ("q4_0", "q4_k", "q6"):  # the 128 + q form: its two sums each round (module doc of exact.py)
        bound = K * 2.0 ** -24 * sum((x.double().abs() @ b.double().t()) for _, b in ew.bounds[1:])
    over = (y - ref).abs() - bound
    i = int(over.argmax())
    assert float(over.max()) <= 0, f"{fam}: row {i // N}, column {i % N}, tile {i % N // 16}: over by {float(over.max())}"
