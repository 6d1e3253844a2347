"""The GGUF Q6_K weight kernel of ``csrc/gemm_qstream.hip`` against a plain PyTorch fp32 reference on the blocks' values
as ``gguf.py``'s ``_q6_k`` decodes them, its epilogues and the fused RMSNorm with and without a separate gain, the V
rows of a QKV projection as a launch of their own behind a Q4_K launch of the q / k rows, and the engine on the
Q4_K_M mix: ``weight_dtype="q4_k_m"`` against the torch oracle on per-matrix round trips, and a Q4_K_M GGUF file
run as stored.  The reference is never the code under test."""
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

sys.path.insert(0, str(Path(__file__).parent))

from cain_amd import ops  # noqa: E402
from cain_amd.engine import DecodeEngine  # noqa: E402
from cain_amd.models import TINY  # noqa: E402
from cain_amd.models.q4 import (Q6_K, dequantize_q4, pack_q4, pack_q6, q4_fields, q6_fields,  # noqa: E402
                                quantize_q4_k, quantize_q6_k)
from cain_amd.models.reference import ReferenceModel  # noqa: E402
from cain_amd.models.weights import roundtrip_weights, rope_pair_order  # noqa: E402

DEV = torch.device("cuda")


def rel_err(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


def q6(w, gain=None):
    n, k = w.shape
    b = quantize_q6_k(w)
    wq, sb = pack_q6(q6_fields(b, n, k), gain)
    return wq, sb, dequantize_q4(b, Q6_K, n, k)


def _normed(x, eps=1e-6):
    xf = x.float()
    return xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)


def test_code_and_scale_semantics():
    """Unit activation rows pick single weights out of random-byte blocks (every code, negative scales, -128 / 127;
    |d| <= 1e-2): two tiles, two super-blocks.

    Bound.  For a unit row at k the kernel computes fl(s (128 + q)) - 160 s with s = d sc of k's group: s is exact in
    fp32 (11 x 8 significant bits), 128 + q comes exact out of the MFMA, 160 s is exact (3 more bits) and the
    difference of the two, smaller than either and on their grid, is exact -- so the one rounding is that of the
    product s (128 + q), |s| (128 + q) <= 191 |s|, at most 2^-24 * 191 |s| (half an ulp).  The weight itself is
    s (q - 32), up to 6 times smaller than that product (0 at q = 32), so the Q4 test's allclose(rtol=1e-5,
    atol=1e-6) cannot hold here (|s| reaches 1.28: 1.5e-5); the cancellation term is added to it."""
    from test_q6_pack import random_q6_blocks

    N, K = 32, 512
    b = random_q6_blocks(N, K, 5, d_max=1e-2).to(DEV)
    f = q6_fields(b, N, K)
    wq, sb = pack_q6(f)
    Wd = dequantize_q4(b, Q6_K, N, K)
    s = (f["d"].float().repeat_interleave(16, 1) * f["sc"].float()).repeat_interleave(16, 1)  # [N, K]
    y = ops.gemm_q6(wq, sb, torch.eye(K, device=DEV).bfloat16(), N, ops.EPI_F32)              # [K, N]
    err = (y - Wd.t()).abs()
    bound = 1e-6 + 1e-5 * Wd.t().abs() + 2.0 ** -24 * 191 * s.t().abs()
    print("unit activations: max err", float(err.max()), "max err / bound", float((err / bound).max()))
    assert bool((err <= bound).all())


F32_REF = {}


def _f32_case(N, K):
    """One weight matrix per shape, shared by the row counts (quantised and decoded once, left unchanged)."""
    if (N, K) not in F32_REF:
        g = torch.Generator(device=DEV).manual_seed(N + K)
        W = torch.randn(N, K, device=DEV, generator=g) * 0.02
        F32_REF[(N, K)] = (W, *q6(W))
    return F32_REF[(N, K)]


@pytest.mark.parametrize("M", [1, 3, 16, 20])
@pytest.mark.parametrize("N,K", [(512, 256), (1024, 4096), (256, 14336), (256, 24576)])
def test_q6_f32_matches_reference(M, N, K):
    """(256, 14336) and (256, 24576) hold one activation row per launch (M K 2.25 bytes of LDS)."""
    W, wq, sb, Wd = _f32_case(N, K)
    torch.manual_seed(M + K)
    x = torch.randn(M, K, device=DEV).bfloat16()
    y = ops.gemm_q6(wq, sb, x, N, ops.EPI_F32)
    e = rel_err(y, x.float() @ Wd.t())
    print(f"M={M} N={N} K={K} rel err {e:.3e}")
    assert e < 1e-3
    assert rel_err(y, x.float() @ W.t()) < 0.05  # and the 6-bit fit stays near the original weights


def test_q6_rows_per_launch():
    lib = ops.load()
    assert lib.cain_gemm_q6_rows(256, ops.EPI_F32) == 16 and lib.cain_gemm_q6_rows(4096, ops.EPI_F32) == 6
    assert lib.cain_gemm_q6_rows(14336, ops.EPI_F32) == 1 and lib.cain_gemm_q6_rows(24576, ops.EPI_F32) == 1
    assert lib.cain_gemm_q6_rows(4096, ops.EPI_QKV_ROPE) == 3  # the 4-wave kernel's 28 KiB copy only


@pytest.mark.parametrize("M", [1, 3, 20])
def test_q6_chunk_maxima(M):
    _, wq, sb, Wd = _f32_case(1024, 4096)
    N = 1024
    torch.manual_seed(M)
    x = torch.randn(M, 4096, device=DEV).bfloat16()
    cm = torch.full((M, N // 16), float("nan"), device=DEV)
    y = ops.gemm_q6(wq, sb, x, N, ops.EPI_F32, cmax=cm)
    assert torch.equal(cm, y.view(M, N // 16, 16).amax(-1))


@pytest.mark.parametrize("M", [1, 5])
def test_q6_bias_residual_norm_and_gain(M):
    torch.manual_seed(9 + M)
    N, K = 1024, 1024
    W = torch.randn(N, K, device=DEV) * 0.02
    x = (3 * torch.randn(M, K, device=DEV)).bfloat16()
    g = torch.rand(K, device=DEV) + 0.5
    wq, sb, Wd = q6(W)
    bias = torch.randn(N, device=DEV)
    yb = ops.gemm_q6(wq, sb, x, N, ops.EPI_BF16, bias=bias)
    assert rel_err(yb, x.float() @ Wd.t() + bias) < 1e-2
    r = torch.randn(M, N, device=DEV).bfloat16()
    ref = x.float() @ Wd.t() + r.float()
    ops.gemm_q6(wq, sb, x, N, ops.EPI_RESID, out=r)
    assert rel_err(r, ref) < 1e-2
    yn = ops.gemm_q6(wq, sb, x, N, ops.EPI_F32, norm=True, eps=1e-6)
    assert rel_err(yn, _normed(x) @ Wd.t()) < 1e-3
    # a GGUF file's gain kept separate from its blocks: applied to the activations while staging
    wqg, sbg, _ = q6(W, gain=g)
    yg = ops.gemm_q6(wqg, sbg, x, N, ops.EPI_F32, norm=True, eps=1e-6, gain=True)
    assert rel_err(yg, (_normed(x) * g) @ Wd.t()) < 5e-3


def _rot(x, c, s_):
    half = x.shape[-1] // 2
    return torch.cat([x[..., :half] * c - x[..., half:] * s_, x[..., half:] * c + x[..., :half] * s_], -1)


@pytest.mark.parametrize("H,Hkv,hd,M,kv8", [(4, 1, 128, 1, False), (4, 1, 128, 4, False), (2, 1, 256, 1, False),
                                            (2, 1, 256, 4, False), (4, 1, 128, 4, True)])
def test_split_qkv_q4_then_q6(H, Hkv, hd, M, kv8):
    """A Q4_K_M layer's QKV projection: the q and k rows through gemm_q4 with N = (H + Hkv) hd, the V rows through
    gemm_q6 with the tile offset, both normalising the activations and adding the whole projection's bias.  An fp8
    (e4m3) cache rounds K and V to 3 mantissa bits (2^-4 relative at most, ~3.6 % rms): the project's 8e-2 for it."""
    torch.manual_seed(8)
    K, T_max, S = 512, 256, 16
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
    pos = torch.randint(0, T_max, (M,), device=DEV).int()
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
    ang = torch.arange(T_max, dtype=torch.float64)[:, None] * inv[None]
    cos_t, sin_t = ang.cos().float().to(DEV), ang.sin().float().to(DEV)
    b4 = quantize_q4_k(W[:nqk])
    b6 = quantize_q6_k(W[nqk:])
    Wd = torch.cat([dequantize_q4(b4, 1, nqk, K), dequantize_q4(b6, Q6_K, qkv_dim - nqk, K)], 0)
    wq4, sb4 = pack_q4(q4_fields(b4[perm[:nqk]].contiguous(), 1, nqk, K), 1)  # blocks along K: rows permute freely
    wq6, sb6 = pack_q6(q6_fields(b6, qkv_dim - nqk, K))
    rope = dict(kc=kc, vtc=vt, slot=slot, pos=pos, cos_t=cos_t, sin_t=sin_t, H=H, Hkv=Hkv, hd=hd)
    ops.gemm_q4(1, wq4, sb4, x, nqk, ops.EPI_QKV_ROPE, bias=bias[perm], out=q, norm=True, rope=rope)
    ops.gemm_q6(wq6, sb6, x, qkv_dim - nqk, ops.EPI_QKV_ROPE, bias=bias[perm], out=q, norm=True, rope=rope,
                tile0=nqk // 16)
    ref = (_normed(x) @ Wd.t() + bias).bfloat16().float()
    if kv8:
        kc, vt = kc.view(torch.float8_e4m3fn).float(), vt.view(torch.float8_e4m3fn).float()
    kn, vn = ops.unpack_kcache(kc), ops.unpack_vcache(vt)
    tol = 8e-2 if kv8 else 1e-2
    for m in range(M):
        p, sl = int(pos[m]), int(slot[m])
        cc, ss = cos_t[p], sin_t[p]
        assert rel_err(q[m].view(H, hd), _rot(ref[m, : H * hd].view(H, hd), cc, ss)) < 1e-2
        assert rel_err(kn[sl, :, p], _rot(ref[m, H * hd:nqk].view(Hkv, hd), cc, ss)) < tol
        assert rel_err(vn[sl, :, p], ref[m, nqk:].view(Hkv, hd)) < tol
    assert int((kn != 0).any(-1).sum()) == M * Hkv and int((vn != 0).any(-1).sum()) == M * Hkv


Q4_TINY = sorted(n for n, c in TINY.items() if not (c.d_model % 256 or c.q_dim % 256 or c.ffn % 256))


@pytest.mark.parametrize("name", Q4_TINY)
def test_q4_k_m_engine_logits_match_oracle(name):
    """Prompts longer than one prefill chunk; oracle = the same model on per-matrix round trips of the mix."""
    eng = DecodeEngine(name, device="cuda", max_batch=4, max_context=512, keep_natural=True, seed=3,
                       weight_dtype="q4_k_m")
    lay = eng._packed["layers"]
    assert "wv" not in lay[0] and lay[1]["fv"] == Q6_K and lay[1]["fdown"] == Q6_K and eng._packed["flm_head"] == Q6_K
    prompts = ["In 500 words, please give me information about Elizabeth II " * 6, "hi", "abc def ghi"]
    assert len(eng.encode(prompts[0])) > eng.prefill_chunk
    got = eng.last_logits(prompts)
    ref = ReferenceModel(roundtrip_weights(eng.weights, "q4_k_m"))
    for i, p in enumerate(prompts):
        want = ref.forward(torch.tensor([eng.encode(p)], device="cuda"))[0, -1]
        cos = torch.nn.functional.cosine_similarity(got[i].float(), want.float(), dim=0)
        assert cos > 0.995, (name, i, float(cos))
    eng.close()


def test_q4_k_m_engine_generate_graph_equals_eager():
    eng = DecodeEngine("tiny-llama3.1:8b", device="cuda", max_batch=4, max_context=256, seed=5, steps_per_graph=4,
                       weight_dtype="q4_k_m")
    opts = [dict(temperature=0.8, seed=11 + i, eos_id=-1) for i in range(3)]
    prompts = ["In 100 words, please give me information about India", "hi", "abc"]
    a = eng.generate(prompts, 10, opts, use_graph=True)
    b = eng.generate(prompts, 10, opts, use_graph=False)
    assert [r.tokens for r in a] == [r.tokens for r in b]
    eng.close()


@pytest.mark.parametrize("family", ["llama", "gemma"])
def test_mixed_gguf_file_runs_its_blocks_as_stored(family, tmp_path):
    """A Q4_K_M file (layer 1's attn_v and ffn_down and the head Q6_K, the rest Q4_K) on weight_dtype q4_k: nothing
    is re-quantised, the gains stay separate, and the logits match the fp32 oracle of the file's decoded weights."""
    from hf_fixtures import make_checkpoint

    from cain_amd.models.gguf import export_gguf, load_gguf
    from cain_amd.models.hf import load_pretrained

    make_checkpoint(family, tmp_path / "hf", scale=4.0)
    _, mw, _ = load_pretrained(tmp_path / "hf", dtype=torch.float32)
    for lw in mw.layers:  # non-unit gains: the separate-gain path must apply them, in both QKV launches
        lw.attn_norm = lw.attn_norm + 0.3 * torch.rand_like(lw.attn_norm)
        lw.mlp_norm = lw.mlp_norm + 0.3 * torch.rand_like(lw.mlp_norm)
    export_gguf(mw, tmp_path / "m.gguf", family, tensor_type="Q4_K_M")
    eng = DecodeEngine.from_pretrained(str(tmp_path / "m.gguf"), device="cuda", max_batch=2, max_context=256,
                                       weight_dtype="q4_k")
    assert eng._packed.get("q4_gain") and eng.weights.native["requantized"] == []
    assert eng._packed["layers"][1]["fv"] == Q6_K and eng._packed["flm_head"] == Q6_K
    _, mg, _ = load_gguf(tmp_path / "m.gguf", dtype=torch.float32)
    ref = ReferenceModel(mg)
    ids = [[1, 5, 9, 33, 100, 7, 64], [1, 200, 3]]
    got = eng.last_logits(ids)
    for i, p in enumerate(ids):
        want = ref.forward(torch.tensor([p]))[0, -1]
        cos = torch.nn.functional.cosine_similarity(got[i].float().cpu(), want.float(), dim=0)
        assert cos > 0.999, (family, i, float(cos))
    eng.close()


def test_oversized_k_is_refused_without_a_launch():
    """K = 25600: one row needs 57,600 bytes of LDS, over the 56 KiB copy.  The entry returns an error before any
    launch (its output stays untouched), and a model with such a Q6_K matrix is refused at construction."""
    import dataclasses

    K, N = 25600, 16
    lib = ops.load()
    assert lib.cain_gemm_q6_rows(K, ops.EPI_F32) == 0 and lib.cain_gemm_q6_rows(K, ops.EPI_RESID) == 0
    assert lib.cain_gemm_q4_rows(K, ops.EPI_RESID) == 1  # (Q4's 2.125 bytes per element still fit)
    wq = torch.zeros(N // 16, K // 128, 1536, device=DEV, dtype=torch.uint8)
    sb = torch.zeros(N * K // 16 + N * K // 64, device=DEV, dtype=torch.uint8)
    x = torch.ones(20, K, device=DEV).bfloat16()
    out = torch.full((20, N), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match="gemm_q6 failed"):
        ops.gemm_q6(wq, sb, x, N, ops.EPI_F32, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    cfg = dataclasses.replace(TINY["tiny-llama3.1:8b"], name="tiny-wide-ffn", ffn=K)  # layer 1's w_down is Q6_K
    with pytest.raises(ValueError, match="does not fit"):
        DecodeEngine(cfg, device="cuda", max_batch=1, max_context=64, weight_dtype="q4_k_m")
