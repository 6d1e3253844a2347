"""The many-row GGUF tile kernels (``csrc/gemm_qtile.hip``: Q4_0, Q4_K, Q6_K against up to 64 rows per launch, one
pass over the weights): the exact int64 product on the forced tile path
(``tests/exact.py``), the fused paths against the fp32 reference on decoded weights at the tolerances of
tests/test_q4_gpu.py / tests/test_q6_gpu.py, agreement with the stream kernels, and the engine (pass counts, which launch nothing: tests/test_qtile_cpu.py).

The kernel walks K in slabs of ``SLAB`` = 256 (one super-block), two slabs per round of its double buffers: K = 256,
768 and 3072 are 1, 3 and 12 slabs (half a round, one and a half, six), K = 2560 is 10 slabs (five rounds)."""
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
from cain_amd.engine import DecodeEngine  # noqa: E402
from cain_amd.models.q4 import (Q6_K, dequantize_q4, pack_q4, pack_q6, q4_fields, q6_fields,  # noqa: E402
                                quantize_q4, quantize_q4_k, quantize_q6_k)
from cain_amd.models.reference import ReferenceModel  # noqa: E402
from cain_amd.models.weights import interleave_tiles, roundtrip_weights, rope_pair_order  # noqa: E402

DEV = torch.device("cuda")
F32, BF16, RESID, QKV = ops.EPI_F32, ops.EPI_BF16, ops.EPI_RESID, ops.EPI_QKV_ROPE
SLAB = 256  # k per slab of the tile kernels (gemm_qtile.hip QT_SLAB)
FMT = {"q4_0": 0, "q4_k": 1, "q6": 2}


@pytest.fixture(autouse=True)
def _switches():
    """The path switch back at the rule afterwards; a GPU error ends the session."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:  # a GPU fault: nothing more may run on the device
        pytest.exit(f"GPU error, stopping the session: {exc}", returncode=3)
    ops.set_q_tile(-1)
    ops.set_q_tile_nb(0)


def rel_err(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


def dev(p):
    return {k: v.to(DEV) for k, v in p.items()}


def run(fam, p, x, n, epi, **kw):
    if fam in ("q4_0", "q4_k"):
        return ops.gemm_q4(FMT[fam], p["wq"], p["sbuf"], x, n, epi, **kw)
    return ops.gemm_q6(p["wq"], p["sbuf"], x, n, epi, **kw)


def stream_rows(fmt, K, epi):
    lib = ops.load()
    return int((lib.cain_gemm_q6_rows if fmt == 2 else lib.cain_gemm_q4_rows)(K, epi))


# ---------------------------------------------------------------- 1. the entry still refuses (pass counts: test_qtile_cpu.py)
@pytest.mark.parametrize("mode", [-1, 0, 1])
def test_oversized_k_is_still_refused(mode):
    """Q6_K at K = 25600: no stream rows, so the entry fails at any M before a launch, whatever the mode."""
    N, K = 16, 25600
    ops.set_q_tile(mode)
    assert ops.gemm_q_passes(2, K, 64, F32) == -1
    wq = torch.zeros(N // 16, K // 128, 1536, dtype=torch.uint8, device=DEV)
    sb = torch.zeros(N * K // 16 + N * K // 64, dtype=torch.uint8, device=DEV)
    for M in (1, 64):
        out = torch.full((M, N), 7.0, device=DEV)
        with pytest.raises(RuntimeError):
            ops.gemm_q6(wq, sb, torch.ones(M, K, device=DEV).bfloat16(), N, F32, out=out)
        assert bool((out == 7.0).all())


# ---------------------------------------------------------------- 2. exact, per format
def check_plain(c: Case, tag: str = ""):
    """tests/test_gemm_exact_gpu.py check_plain's sequence: EPI_F32 twice with cmax, EPI_BF16 + integer bias,
    EPI_RESID in place twice from the same residual -- all equal to the int64 product."""
    x, ew, ref = exact.case_inputs(c)
    p, xd = dev(ew.packed), x.to(torch.bfloat16).to(DEV)
    tag = f"{c.id} {tag}"
    for rep in range(2):
        cm = torch.full((c.M, c.N // 16), float("nan"), device=DEV)
        y = run(c.fam, p, xd, c.N, F32, cmax=cm)
        assert y.dtype == torch.float32
        exact.assert_equal(y, ref.float(), f"{tag} f32 run {rep}")
        exact.assert_equal(cm, y.view(c.M, c.N // 16, 16).amax(-1), f"{tag} cmax run {rep}")
    bias, r0 = exact.plain_extras(c)
    y = run(c.fam, p, xd, c.N, BF16, bias=bias.float().to(DEV))
    exact.assert_equal(y, exact.to_bf16(ref + bias), f"{tag} bf16 + bias")
    for rep in range(2):
        r = r0.to(torch.bfloat16).to(DEV)
        run(c.fam, p, xd, c.N, RESID, out=r)
        exact.assert_equal(r, exact.to_bf16(ref + r0), f"{tag} resid run {rep}")


@pytest.mark.parametrize("M", [1, 16, 17, 33, 64, 65])
@pytest.mark.parametrize("N,K", [(16, 256), (48, 768), (208, 3072)])
@pytest.mark.parametrize("fam", ["q4_0", "q4_k", "q6"])
def test_tile_path_is_exact(fam, N, K, M):
    ops.set_q_tile(1)
    assert ops.gemm_q_passes(FMT[fam], K, M, F32) == -(-M // 64)
    check_plain(Case(fam, N, K, M, "rows"))


@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("fam", ["q4_0", "q4_k", "q6"])
def test_tile_path_is_exact_over_ring_rounds_and_row_splits(fam, nb):
    """K = 2560: 10 slabs of SLAB = 256, five rounds of the double buffers, at 64 rows (and K = 768, 3 slabs: a round
    and a half, at 40 rows = three row blocks, so one row block or row group idles); with both splits of the row
    blocks over the waves (Q4: 1 or 2 blocks per wave; Q6_K has 1 only and ignores the switch)."""
    assert 2560 // SLAB == 10
    ops.set_q_tile(1)
    ops.set_q_tile_nb(nb)
    check_plain(Case(fam, 48, 2560, 64, "rows"), tag=f"nb {nb}")
    ops.set_q_tile_nb(nb)
    check_plain(Case(fam, 48, 768, 40, "rows"), tag=f"nb {nb}")


@pytest.mark.parametrize("M", [17, 64, 65])
def test_q6_tile_path_nonzero_tile0(M):
    """As test_q6_nonzero_tile0: output columns, bias and residual start at tile 2; columns before it stay."""
    ops.set_q_tile(1)
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


# ---------------------------------------------------------------- 3. fused paths against the fp32 reference
def _normed(x, eps=1e-6):
    xf = x.float()
    return xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)


def _quant(fam, W, gain=None):
    """(wq, sbuf, decoded weights) of a random matrix in one of the three formats."""
    n, k = W.shape
    if fam == "q6":
        b = quantize_q6_k(W)
        wq, sb = pack_q6(q6_fields(b, n, k), gain)
        return wq, sb, dequantize_q4(b, Q6_K, n, k)
    b = quantize_q4(W, FMT[fam])
    wq, sb = pack_q4(q4_fields(b, FMT[fam], n, k), FMT[fam], gain)
    return wq, sb, dequantize_q4(b, FMT[fam], n, k)


@pytest.mark.parametrize("M,nb", [(17, 0), (64, 0), (64, 1), (64, 2)])
@pytest.mark.parametrize("fam", ["q4_0", "q4_k", "q6"])
def test_tile_path_norm_and_separate_gain(fam, M, nb):
    """``nb``: Q4's row blocks per wave forced (0: the rule, which takes 1 at this N; Q6_K has 1 only), so every
    instance runs the norm."""
    ops.set_q_tile(1)
    ops.set_q_tile_nb(nb)
    torch.manual_seed(9 + M)
    N, K = 512, 1024
    W = torch.randn(N, K, device=DEV) * 0.02
    x = (3 * torch.randn(M, K, device=DEV)).bfloat16()
    g = torch.rand(K, device=DEV) + 0.5
    wq, sb, Wd = _quant(fam, W)
    yn = run(fam, {"wq": wq, "sbuf": sb}, x, N, F32, norm=True, eps=1e-6)
    e = rel_err(yn, _normed(x) @ Wd.t())
    print(f"{fam} M={M} nb={nb} norm: rel err {e:.3e}")
    assert e < 1e-3
    wqg, sbg, _ = _quant(fam, W, gain=g)
    yg = run(fam, {"wq": wqg, "sbuf": sbg}, x, N, F32, norm=True, eps=1e-6, gain=True)
    e = rel_err(yg, (_normed(x) * g) @ Wd.t())
    print(f"{fam} M={M} norm + gain: rel err {e:.3e}")
    assert e < 5e-3


@pytest.mark.parametrize("M,nb", [(17, 0), (64, 0), (64, 1), (64, 2)])
@pytest.mark.parametrize("act", ["silu", "gelu"])
@pytest.mark.parametrize("fam", ["q4_0", "q4_k"])
def test_tile_path_gateup_activation(fam, act, M, nb):
    ops.set_q_tile(1)
    ops.set_q_tile_nb(nb)
    torch.manual_seed(11)
    F, K = 256, 1024
    Wg, Wu = torch.randn(F, K, device=DEV) * 0.02, torch.randn(F, K, device=DEV) * 0.02
    x = torch.randn(M, K, device=DEV).bfloat16()
    wq, sb, Wd = _quant(fam, interleave_tiles(Wg, Wu, tile=8))
    y = ops.gemm_q4(FMT[fam], wq, sb, x, 2 * F, ops.EPI_SILU if act == "silu" else ops.EPI_GELU, norm=True)
    hh = (_normed(x) @ Wd.t()).view(M, F // 8, 2, 8)
    a, u = hh[:, :, 0].reshape(M, F), hh[:, :, 1].reshape(M, F)
    a = torch.nn.functional.silu(a) if act == "silu" else torch.nn.functional.gelu(a, approximate="tanh")
    assert rel_err(y, a * u) < 1.5e-2


def _rot(x, c, s_):
    half = x.shape[-1] // 2
    return torch.cat([x[..., :half] * c - x[..., half:] * s_, x[..., half:] * c + x[..., :half] * s_], -1)


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("M,nb", [(17, 0), (64, 0), (64, 1), (64, 2)])
@pytest.mark.parametrize("split", [False, True])
def test_tile_path_qkv_rope_kv_append(split, M, nb, kv8):
    """The fused QKV + RoPE + KV-append epilogue with a distinct (slot, pos) per row, rows in several row blocks:
    one Q4_K launch of all rows, or (``split``, a Q4_K_M layer) the Q4_K q / k rows followed by the Q6_K V rows with
    tile0 = (H + Hkv) hd / 16.  Only the M Hkv cache rows may be written.  ``nb``: row blocks per wave (0: the rule)."""
    ops.set_q_tile(1)
    ops.set_q_tile_nb(nb)
    torch.manual_seed(8)
    H, Hkv, hd = 4, 1, 128
    K, T_max, S = 512, 128, M + 5
    nqk, qkv_dim = (H + Hkv) * hd, (H + 2 * Hkv) * hd
    W = torch.randn(qkv_dim, K, device=DEV) * 0.05
    bias = torch.randn(qkv_dim, device=DEV)
    x = torch.randn(M, K, device=DEV).bfloat16()
    per = rope_pair_order(hd).to(DEV)
    perm = torch.cat([h * hd + per for h in range(H + Hkv)] + [torch.arange(nqk, qkv_dim, device=DEV)])
    cdt = torch.uint8 if kv8 else torch.bfloat16
    kc = torch.zeros(S, Hkv, T_max, hd, device=DEV, dtype=cdt)
    vt = torch.zeros(S, Hkv, hd, T_max, device=DEV, dtype=cdt)
    q = torch.zeros(M, H * hd, device=DEV).bfloat16()
    slot = torch.randperm(S, device=DEV)[:M].int()
    pos = torch.randperm(T_max, device=DEV)[:M].int()
    assert len(set(slot.tolist())) == M and len(set(pos.tolist())) == M
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
    ang = torch.arange(T_max, dtype=torch.float64)[:, None] * inv[None]
    cos_t, sin_t = ang.cos().float().to(DEV), ang.sin().float().to(DEV)
    rope = dict(kc=kc, vtc=vt, slot=slot, pos=pos, cos_t=cos_t, sin_t=sin_t, H=H, Hkv=Hkv, hd=hd)
    if split:
        b4, b6 = quantize_q4_k(W[:nqk]), quantize_q6_k(W[nqk:])
        Wd = torch.cat([dequantize_q4(b4, 1, nqk, K), dequantize_q4(b6, Q6_K, qkv_dim - nqk, K)], 0)
        wq4, sb4 = pack_q4(q4_fields(b4[perm[:nqk]].contiguous(), 1, nqk, K), 1)
        wq6, sb6 = pack_q6(q6_fields(b6, qkv_dim - nqk, K))
        ops.gemm_q4(1, wq4, sb4, x, nqk, QKV, bias=bias[perm], out=q, norm=True, rope=rope)
        ops.gemm_q6(wq6, sb6, x, qkv_dim - nqk, QKV, bias=bias[perm], out=q, norm=True, rope=rope, tile0=nqk // 16)
    else:
        b4 = quantize_q4_k(W)
        Wd = dequantize_q4(b4, 1, qkv_dim, K)
        wq4, sb4 = pack_q4(q4_fields(b4[perm].contiguous(), 1, qkv_dim, K), 1)
        ops.gemm_q4(1, wq4, sb4, x, qkv_dim, QKV, bias=bias[perm], out=q, norm=True, rope=rope)
    ref = (_normed(x) @ Wd.t() + bias).bfloat16().float()
    if kv8:
        kc, vt = kc.view(torch.float8_e4m3fn).float(), vt.view(torch.float8_e4m3fn).float()
    kn, vn = ops.unpack_kcache(kc), ops.unpack_vcache(vt)
    tol = 8e-2 if kv8 else 1e-2
    for m in range(M):
        p, sl = int(pos[m]), int(slot[m])
        cc, ss = cos_t[p], sin_t[p]
        assert rel_err(q[m].view(H, hd), _rot(ref[m, : H * hd].view(H, hd), cc, ss)) < 1e-2, m
        assert rel_err(kn[sl, :, p], _rot(ref[m, H * hd:nqk].view(Hkv, hd), cc, ss)) < tol, m
        assert rel_err(vn[sl, :, p], ref[m, nqk:].view(Hkv, hd)) < tol, m
    assert int((kn != 0).any(-1).sum()) == M * Hkv and int((vn != 0).any(-1).sum()) == M * Hkv


# ---------------------------------------------------------------- 4. path agreement
@pytest.mark.parametrize("fam", ["q4_k", "q6"])
def test_tile_path_error_against_the_stream_path(fam):
    """Random bf16 activations, (N, K) = (1024, 4096), M = 20, F32: each path's error against the fp64 product of the
    decoded weights; the tile path's is at most twice the stream path's, both under the existing 1e-3."""
    torch.manual_seed(20)
    N, K, M = 1024, 4096, 20
    W = torch.randn(N, K, device=DEV) * 0.02
    x = torch.randn(M, K, device=DEV).bfloat16()
    wq, sb, Wd = _quant(fam, W)
    ref = x.double() @ Wd.double().t()
    errs = {}
    for mode in (0, 1):
        ops.set_q_tile(mode)
        assert ops.gemm_q_passes(FMT[fam], K, M, F32) == (1 if mode else -(-M // stream_rows(FMT[fam], K, F32)))
        y = run(fam, {"wq": wq, "sbuf": sb}, x, N, F32)
        errs[mode] = float((y.double() - ref).norm() / ref.norm())
    print(f"{fam}: stream path {errs[0]:.3e}, tile path {errs[1]:.3e}")
    assert errs[0] < 1e-3 and errs[1] < 1e-3
    assert errs[1] <= 2 * errs[0]


# ---------------------------------------------------------------- 5. engine
def _cos(a, b):
    return float(torch.nn.functional.cosine_similarity(a.float(), b.float(), dim=0))


@pytest.mark.parametrize("wd", ["q4_k_m", "q4_0"])
def test_engine_logits_under_both_paths(wd):
    eng = DecodeEngine("tiny-llama3.1:8b", device="cuda", max_batch=32, max_context=512, keep_natural=True, seed=3,
                       weight_dtype=wd)
    prompts = ["In 500 words, please give me information about Elizabeth II " * 6, "hi", "abc def ghi"]
    assert len(eng.encode(prompts[0])) > eng.prefill_chunk
    got = {}
    for mode in (0, -1):
        ops.set_q_tile(mode)
        got[mode] = [t.clone() for t in eng.last_logits(prompts)]
    ref = ReferenceModel(roundtrip_weights(eng.weights, wd))
    for i, p in enumerate(prompts):
        want = ref.forward(torch.tensor([eng.encode(p)], device="cuda"))[0, -1]
        for mode in (0, -1):
            assert _cos(got[mode][i], want) > 0.995, (wd, mode, i)
        assert _cos(got[0][i], got[-1][i]) > 0.9999, (wd, i)
    eng.close()


@pytest.mark.parametrize("wd", ["q4_k_m", "q4_0"])
def test_engine_generate_20_rows_graph_equals_eager(wd):
    """20 concurrent requests: decode forwards of 20 rows, the tile kernels under mode 1 (and under the rule)."""
    eng = DecodeEngine("tiny-llama3.1:8b", device="cuda", max_batch=32, max_context=256, seed=5, steps_per_graph=4,
                       weight_dtype=wd)
    ops.set_q_tile(1)
    opts = [dict(temperature=0.8, seed=11 + i, eos_id=-1) for i in range(20)]
    prompts = [f"prompt number {i} about India" for i in range(20)]
    a = eng.generate(prompts, 8, opts, use_graph=True)
    b = eng.generate(prompts, 8, opts, use_graph=False)
    assert len(a) == 20 and [r.tokens for r in a] == [r.tokens for r in b]
    eng.close()
