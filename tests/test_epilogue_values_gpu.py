"""Every GEMM family's epilogue, element by element: one-hot activation rows deliver chosen values to the epilogue
exactly (tests/epilogue_values.py), and every output is compared with a float64 statement of the epilogue -- the fused
QKV + RoPE + KV append at real angles on every path, head shape and cache type (admissible sets; V bit exact, with
e4m3 ties, subnormals and saturation), SiLU / GeGLU against derived per-element bounds with the overflow tails, and
the fused RMSNorm factor through the GEMM prologues and split-K row sums.  Each test prints its counts of decided
and undecided elements and the worst error in units of its bound."""
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

sys.path.insert(0, str(Path(__file__).parent))

import epilogue_values as ev  # noqa: E402
import exact  # noqa: E402
from cain_amd import ops  # noqa: E402

DEV = torch.device("cuda")
QKV = ops.EPI_QKV_ROPE


@pytest.fixture(autouse=True)
def _switches():
    """Every switch the tests touch, back at its default afterwards."""
    inline0 = ops.wide_gemm_inline_mode()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:  # a GPU fault: nothing more may run on the device
        pytest.exit(f"GPU error, stopping the session: {exc}", returncode=3)
    ops.set_skinny_split(1)
    ops.set_q_tile(-1)
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


def force(p: ev.Path_, N: int, K: int = 0):
    """Put the launch on the path the case names and confirm it through the library's own queries; returns the
    (k ranges, slab format) the launch runs with, for ``delivery_exact``."""
    K = K or p.K
    if p.fam == "bf16":
        if p.tag in ("skinny", "skinnysplit"):
            assert p.M <= 16 and (ops.gemm_ws_bytes(N, K, p.M) > 0) == (p.tag == "skinnysplit")
        elif p.tag == "batched":
            assert 16 < p.M <= 64 and ops.gemm_ws_bytes(N, K, p.M) > 0 and not ops.wide_gemm_eligible(N, K, p.M)
        else:
            assert ops.wide_gemm_eligible(N, K, p.M)
            ks, var = p.plan
            if ks:
                ops.set_wide_gemm_plan(N, K, 256 if p.M > 128 else 128, ks, var)
                assert ops.wide_gemm_plan(N, K, p.M) == (ks, var)
            ks, var = ops.wide_gemm_plan(N, K, p.M)
            if ks > 1:
                return exact.wide_k_ranges(K, ks), ("f32" if var == 4 else "f16exp")
        return None, "f32"
    if p.fam in ("q4_0", "q4_k", "q6"):
        ops.set_q_tile(0 if p.tag == "stream" else 1)
    if p.fam in ev.A8:
        assert ops.w8a8_eligible(N, K, p.M)
        split = int(ops.load().cain_w8a8_ws_bytes(N, K, p.M)) > 80 * 1024
        assert split == (p.tag == "widesplit") == (exact.a8_splits(N, K) > 1)
        if split:
            return exact.wide_k_ranges(K, exact.a8_splits(N, K), stage=128), "f16"
    return None, "f32"


@pytest.mark.parametrize("c", ev.QKV_CASES, ids=ev.qkv_id)
def test_qkv_rope_kv_append_per_element(c):
    """Fused QKV at real angles (epilogue_values' module doc): decided elements bit for bit, undecided ones inside
    their admissible set and at most 1 % of the case, V exact, sentinels untouched; twice per case."""
    p, geo_name, kv8 = c
    geo = ev.GEOS[geo_name]
    H, Hkv, hd, T = geo
    N = exact.qkv_n(geo)
    d, bias, slot, pos, S = ev.qkv_inputs(p, geo_name)
    ranges, slab = force(p, N)
    assert ev.delivery_exact(d, ranges, slab) is None
    cos, sin = ev.rope_tables(hd, T)
    want = ev.qkv_want(d.acc, bias, slot, pos, cos, sin, geo, S, kv8)
    pk, xd = dev(d.packed), d.x.to(torch.bfloat16).to(DEV)
    for rep in range(2):
        if kv8:
            kc = torch.full((S, Hkv, T, hd), ev.SENT8, device=DEV, dtype=torch.uint8)
            vt = torch.full((S, Hkv, hd, T), ev.SENT8, device=DEV, dtype=torch.uint8)
        else:
            kc = torch.full((S, Hkv, T, hd), ev.SENT, device=DEV).bfloat16()
            vt = torch.full((S, Hkv, hd, T), ev.SENT, device=DEV).bfloat16()
        q = torch.full((p.M, H * hd), ev.SENT, device=DEV).bfloat16()
        rope = dict(kc=kc, vtc=vt, slot=slot.to(DEV), pos=pos.to(DEV), cos_t=cos.to(DEV), sin_t=sin.to(DEV), H=H,
                    Hkv=Hkv, hd=hd)
        b = bias.to(DEV)
        if p.fam == "bf16":
            ops.qkv_rope(pk["wp"], xd, N, q, kc, vt, rope["slot"], rope["pos"], rope["cos_t"], rope["sin_t"], H, Hkv, hd,
                         bias=b)
        else:
            run(p.fam, pk, xd, N, QKV, bias=b, out=q, rope=rope)
        kf = kc.view(torch.float8_e4m3fn).float() if kv8 else kc.float()
        vf = vt.view(torch.float8_e4m3fn).float() if kv8 else vt.float()
        kn, vn = exact.unpack_caches(kf, vf)
        st, report = ev.qkv_check(q.float().cpu(), kn, vn, want)
        print(st.line(f"{ev.qkv_id(c)} run {rep}"))
        assert report is None, f"{ev.qkv_id(c)} run {rep}: {report}"
        assert st.undecided <= 0.01 * (st.decided + st.undecided)


@pytest.mark.parametrize("kind", ["silu", "gelu"])
@pytest.mark.parametrize("p,norm", ev.ACT_CASES, ids=ev.act_id)
def test_silu_geglu_per_element(p, norm, kind):
    """act(gate) x up per element against the derived bound, gate and up rows interleaved; the overflow tails finite
    and within 1e-30."""
    d = ev.act_inputs(p, kind, norm)
    N = 2 * ev.ACT_F
    ranges, slab = force(p, N)
    assert ev.delivery_exact(d, ranges, slab) is None
    ref = ev.act_case_ref(d, kind, norm)
    kw = {"norm": True, "eps": ev.EPS} if norm else {}
    y = run(p.fam, dev(d.packed), d.x.to(torch.bfloat16).to(DEV), N, ops.EPI_SILU if kind == "silu" else ops.EPI_GELU, **kw)
    assert y.dtype == torch.bfloat16 and y.shape == ref["r"].shape
    st, report = ev.act_check(y.float().cpu(), ref)
    print(st.line(f"{p.id} {kind} {'norm' if norm else 'plain'}"))
    assert report is None, f"{p.id} {kind}: {report}"


@pytest.mark.parametrize("p", ev.NORM_PATHS, ids=lambda p: p.id)
def test_fused_rmsnorm_factor_through_the_gemm(p):
    """a W[n, k] / sqrt(ss / K + eps) on fp32 outputs to 5 x 2^-24 (7 on the activation-quantised pair) and on bf16
    outputs as an admissible set; the sum of squares is an exact integer on every path."""
    d = ev.norm_inputs(p)
    K = ev.norm_k(p)
    force(p, ev.NORM_N, K)
    pk, xd = dev(d.packed), d.x.to(torch.bfloat16).to(DEV)
    for epi in (ops.EPI_F32, ops.EPI_BF16):
        y = run(p.fam, pk, xd, ev.NORM_N, epi, norm=True, eps=ev.EPS)
        st, report = ev.norm_check(y.cpu(), d, ev.rho_norm(p.fam))
        print(st.line(f"{p.id} {'f32' if epi == ops.EPI_F32 else 'bf16'}"))
        assert report is None, f"{p.id}: {report}"
