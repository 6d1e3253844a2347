"""GGUF Q6_K blocks for the native Q6_K kernel (models/q4.py, ops/csrc/gemm_qstream.hip) and the Q4_K_M mix, CPU checks:
the field extraction is bit-exact against gguf.py's ``_q6_k`` decoder on random block bytes, an emulation of the
kernel's arithmetic on the PACKED bytes -- its lane layout, nibble / bit-pair order and scale indexing, T_g = sum x
(128 + q) and the 160 s_g X_g correction -- reproduces the fp32 product with the decoded weights, a Q4_K_M file goes
through the loader with nothing re-quantised, and ``weight_dtype="q4_k_m"`` runs on the torch backend.  The reference
of every numeric check is gguf.py's fp32 decoders, never the code under test."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).parent))

from cain_amd.models.gguf import GGML_TYPES, TYPE_ID, dequantize  # noqa: E402
from cain_amd.models.q4 import (Q6_K, dequantize_q4, pack_native, pack_q6, q6_fields, quant_pack_q4,  # noqa: E402
                                quantize_q4_k, quantize_q6_k)


def random_q6_blocks(n, k, seed, d_max=None):
    """Q6_K block bytes with ql, qh and the scales uniform over all byte values (negative scales, -128 / 127, q = 0 /
    63) and d a finite fp16 (|d| <= d_max when given)."""
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(0, 256, (n, k // 256, 210), generator=g, dtype=torch.int64).to(torch.uint8)
    if d_max is None:
        d = torch.randint(0, 0x7C00, (n, k // 256), generator=g).to(torch.int16)      # any finite positive fp16 ...
        d = d | (torch.randint(0, 2, d.shape, generator=g).to(torch.int16) << 15)     # ... of either sign
        d = d.view(torch.float16)
    else:
        d = ((torch.rand(n, k // 256, generator=g) * 2 - 1) * d_max).to(torch.float16)
    b[..., 208:210] = d.contiguous().view(torch.uint8).reshape(n, k // 256, 2)
    return b


def test_fields_are_exact_on_random_block_bytes():
    n, k = 16, 1024
    b = random_q6_blocks(n, k, 0)
    f = q6_fields(b, n, k)
    assert f["codes"].dtype == torch.uint8 and f["sc"].dtype == torch.int8 and f["d"].dtype == torch.float16
    assert int(f["codes"].min()) == 0 and int(f["codes"].max()) == 63
    assert int(f["sc"].min()) == -128 and int(f["sc"].max()) == 127
    # the decoder's own expression order: (d * sc) * (q - 32)
    d = f["d"].float().repeat_interleave(16, 1)
    w = (d * f["sc"].float()).repeat_interleave(16, 1) * (f["codes"].float() - 32)
    ref = dequantize(b.reshape(-1), TYPE_ID["Q6_K"], n * k).reshape(n, k)
    assert torch.isfinite(ref).all()
    assert torch.equal(w, ref)
    assert torch.equal(ref, dequantize_q4(b, Q6_K, n, k))


def emulate(wq, sbuf, x, n, k, dt=torch.float32):
    """gemm_qstream.hip's step on the packed bytes: per (tile t, quad p) the lane 16 g + r reads 16 bytes of low nibbles
    at 16 lane and 8 bytes of high bit pairs at 1024 + 8 lane; MFMA s takes k = 128 p + 16 s + 4 g + j from byte j of
    low dword s >> 1 (nibble s & 1) and of high dword s >> 2 (bits 2 (s & 3)); T = sum x (128 + q); out = sum_g s_g
    T_g - 160 s_g X_g with s_g = d sc_g read at the kernel's offsets."""
    nt, kq = n // 16, k // 128
    m = x.shape[0]
    lo = wq[..., :1024].reshape(nt, kq, 4, 16, 4, 4).long()    # [t, p, g, r, dword, byte j]
    hi = wq[..., 1024:].reshape(nt, kq, 4, 16, 2, 4).long()
    codes = torch.empty(nt, 16, kq, 8, 4, 4, dtype=torch.long)  # [t, r, p, s, g, j]
    for s in range(8):
        c = ((lo[..., s >> 1, :] >> (4 * (s & 1))) & 15) | (((hi[..., s >> 2, :] >> (2 * (s & 3))) & 3) << 4)
        codes[:, :, :, s] = c.permute(0, 3, 1, 2, 4)           # [t, p, g, r, j] -> [t, r, p, g, j]
    codes = codes.reshape(n, k)
    sc = sbuf[: n * k // 16].view(torch.int8).reshape(nt, kq, 16, 8).permute(0, 2, 1, 3).reshape(n, k // 16).to(dt)
    d = sbuf[n * k // 16: n * k // 16 + n * k // 64].view(torch.float32).reshape(nt, k // 256, 16)
    d = d.permute(0, 2, 1).reshape(n, k // 256)
    sg = d.to(dt).repeat_interleave(16, 1) * sc                         # [n, groups]
    xg = x.to(dt).reshape(m, k // 16, 16)
    T = torch.einsum("mgj,ngj->mng", xg, (128 + codes).to(dt).reshape(n, k // 16, 16))
    X = xg.sum(-1)
    return (T * sg[None]).sum(-1) - torch.einsum("ng,mg->mn", 160 * sg, X)


def test_packed_layout_and_kernel_arithmetic():
    torch.manual_seed(7)
    n, k, m = 64, 1024, 3
    b = quantize_q6_k(torch.randn(n, k) * 0.02)
    x = torch.randn(m, k).bfloat16()
    wq, sbuf = pack_q6(q6_fields(b, n, k))
    got = emulate(wq, sbuf, x, n, k)
    ref = x.float() @ dequantize_q4(b, Q6_K, n, k).t()
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-5


def test_packed_layout_on_random_block_bytes():
    """The layout alone, on blocks no quantiser would write (every code, scale sign and extreme): the same
    arithmetic in fp64, where nothing rounds at this size."""
    n, k = 32, 512
    b = random_q6_blocks(n, k, 3, d_max=1e-2)
    wq, sbuf = pack_q6(q6_fields(b, n, k))
    x = torch.randint(-3, 4, (5, k)).bfloat16()
    got = emulate(wq, sbuf, x, n, k, dt=torch.float64)
    ref = x.double() @ dequantize_q4(b, Q6_K, n, k).double().t()
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-9


def test_packed_sizes_and_gain_last():
    n, k = 32, 512
    w = torch.randn(n, k) * 0.02
    g = torch.rand(k) + 0.5
    wq, s0 = quant_pack_q4(w, Q6_K)
    _, s1 = quant_pack_q4(w, Q6_K, gain=g)
    assert wq.shape == (n // 16, k // 128, 1536) and wq.dtype == torch.uint8
    assert s0.numel() == n * k // 16 + n * k // 64
    assert (wq.numel() + s0.numel()) * 8 == n * k * 6.625           # the file's blocks: 6.5625 bits per weight
    assert GGML_TYPES[TYPE_ID["Q6_K"]][2] * 8 / 256 == 6.5625
    assert torch.equal(s1[: s0.numel()], s0)
    assert torch.equal(s1[s0.numel():].view(torch.float32), g)
    # pack_native dispatches on the format id
    b = quantize_q6_k(w)
    wq2, s2 = pack_native(b, Q6_K, g)
    assert torch.equal(wq2, wq) and torch.equal(s2, s1)


def test_quantiser_round_trips_below_q4_k_and_writes_negative_scales():
    torch.manual_seed(1)
    n, k = 48, 1024
    w = torch.randn(n, k) * 0.02
    b6 = quantize_q6_k(w)
    assert b6.shape == (n, k // 256, 210) and b6.dtype == torch.uint8
    e6 = float((dequantize_q4(b6, Q6_K, n, k) - w).norm() / w.norm())
    e4 = float((dequantize_q4(quantize_q4_k(w), 1, n, k) - w).norm() / w.norm())
    assert e6 < e4, (e6, e4)
    sc = q6_fields(b6, n, k)["sc"]
    assert int((sc < 0).sum()) > 0 and int((sc > 0).sum()) > 0


def test_q4_k_m_rule_on_two_and_32_layers():
    from cain_amd.models.gguf import q4_k_m_type

    assert q4_k_m_type("output.weight", 2) == "Q6_K"
    assert q4_k_m_type("token_embd.weight", 2) == "Q4_K" and q4_k_m_type("token_embd.weight", 2, tied=True) == "Q6_K"
    for name in ("attn_v", "ffn_down"):
        assert q4_k_m_type(f"blk.0.{name}.weight", 2) == "Q4_K"
        assert q4_k_m_type(f"blk.1.{name}.weight", 2) == "Q6_K"
        got = [i for i in range(32) if q4_k_m_type(f"blk.{i}.{name}.weight", 32) == "Q6_K"]
        assert got == [0, 1, 2, 3, 6, 9, 12, 15, 18, 21, 24, 27, 28, 29, 30, 31]
    assert q4_k_m_type("blk.1.attn_q.weight", 2) == "Q4_K" and q4_k_m_type("blk.1.ffn_up.weight", 2) == "Q4_K"


@pytest.fixture(scope="module")
def mixed_files(tmp_path_factory):
    """Q4_K_M files of the llama and gemma fixtures (layer 0 all Q4_K, layer 1 mixed, the head Q6_K), written once."""
    from hf_fixtures import make_checkpoint

    from cain_amd.models.gguf import export_gguf
    from cain_amd.models.hf import load_pretrained

    out = {}
    for family in ("llama", "gemma"):
        d = tmp_path_factory.mktemp(family)
        make_checkpoint(family, d / "hf", scale=4.0)
        _, mw, _ = load_pretrained(d / "hf", dtype=torch.float32)
        export_gguf(mw, d / "m.gguf", family, tensor_type="Q4_K_M")
        out[family] = d / "m.gguf"
    return out


@pytest.mark.parametrize("family", ["llama", "gemma"])
def test_mixed_file_keeps_its_blocks_as_stored(family, mixed_files):
    from cain_amd.models.gguf import GGUFFile, load_gguf
    from cain_amd.models.q4 import gguf_q4_native

    path = mixed_files[family]
    g = GGUFFile(path)
    assert g.tensors["blk.1.attn_v.weight"].type_name == "Q6_K" and g.tensors["blk.0.attn_v.weight"].type_name == "Q4_K"
    cfg, mg, _ = load_gguf(path, dtype=torch.float32)
    nat = gguf_q4_native(g, cfg, 1)
    assert nat["requantized"] == []
    l0, l1 = nat["layers"]
    assert "wv" not in l0 and set(l0["fmts"].values()) == {1}
    assert l1["fmts"] == {"wqkv": 1, "wv": Q6_K, "wo": 1, "wgu": 1, "w_down": Q6_K}
    assert nat["lm_head_fmt"] == Q6_K

    def dq(b, f):
        return dequantize_q4(b, f, b.shape[0], b.shape[1] * 256)

    nqk = cfg.q_dim + cfg.kv_dim
    for lw, nl in zip(mg.layers, nat["layers"]):
        fm = nl["fmts"]
        if "wv" in nl:
            assert torch.equal(dq(nl["wqkv"], fm["wqkv"]), lw.wqkv[:nqk])
            assert torch.equal(dq(nl["wv"], fm["wv"]), lw.wqkv[nqk:])
        else:
            assert torch.equal(dq(nl["wqkv"], fm["wqkv"]), lw.wqkv)
        for name, key in (("wo", "wo"), ("w_gate", "wgu"), ("w_up", "wgu"), ("w_down", "w_down")):
            assert torch.equal(dq(nl[name], fm[key]), getattr(lw, name)), name
    assert torch.equal(dq(nat["lm_head"], Q6_K), mg.lm_head)


def test_mixed_file_packs_a_split_v(mixed_files):
    """pack_for_engine on the file's blocks: layer 1 gets its V rows on their own (unpermuted, Q6_K), formats
    recorded per matrix, sizes those of each format."""
    from cain_amd.models.gguf import GGUFFile, load_gguf
    from cain_amd.models.q4 import gguf_q4_native
    from cain_amd.models.weights import pack_for_engine

    cfg, mg, _ = load_gguf(mixed_files["llama"], dtype=torch.float32)
    mg.native = gguf_q4_native(GGUFFile(mixed_files["llama"]), cfg, 1)
    p = pack_for_engine(mg, weight_dtype="q4_k")
    l0, l1 = p["layers"]
    nqk, d = cfg.q_dim + cfg.kv_dim, cfg.d_model
    assert "wv" not in l0 and l0["wqkv"].shape[0] * 16 == cfg.qkv_dim
    assert l1["wqkv"].shape[0] * 16 == nqk and l1["wv"].shape == (cfg.kv_dim // 16, d // 128, 1536)
    assert (l1["fqkv"], l1["fv"], l1["fo"], l1["fgu"], l1["fdown"]) == (1, Q6_K, 1, 1, Q6_K) and p["flm_head"] == Q6_K
    want_v, want_sv = pack_native(mg.native["layers"][1]["wv"], Q6_K, mg.layers[1].attn_norm.float())
    assert torch.equal(l1["wv"], want_v) and torch.equal(l1["sv"], want_sv)


def test_cpu_engine_runs_the_q4_k_m_oracle():
    """weight_dtype q4_k_m on the torch backend: every matrix of the oracle is the round trip through its own format
    of the Q4_K_M mix (layer 0 all Q4_K; layer 1's V rows and w_down, and the head, Q6_K), and generation runs."""
    from cain_amd.engine import DecodeEngine
    from cain_amd.models.q4 import q4_roundtrip
    from cain_amd.models.weights import WEIGHT_DTYPES

    assert "q4_k_m" in WEIGHT_DTYPES
    eng = DecodeEngine("tiny-llama3.1:8b", device="cpu", max_batch=2, max_context=64, weight_dtype="q4_k_m", seed=1)
    r = eng.generate(["hello there"], 4, [dict(temperature=0.0, eos_id=-1)])[0]
    assert r.eval_count == 4
    cfg, w, o = eng.cfg, eng.weights, eng.ref.mw
    nqk = cfg.q_dim + cfg.kv_dim
    for i, (fv, fdown) in enumerate([(1, 1), (Q6_K, Q6_K)]):
        lw, lo = w.layers[i], o.layers[i]          # unit gains at random init: the gain fold changes nothing
        assert torch.equal(lo.wqkv[:nqk], q4_roundtrip(lw.wqkv[:nqk], 1))
        assert torch.equal(lo.wqkv[nqk:], q4_roundtrip(lw.wqkv[nqk:], fv))
        assert torch.equal(lo.wo, q4_roundtrip(lw.wo, 1)) and torch.equal(lo.w_up, q4_roundtrip(lw.w_up, 1))
        assert torch.equal(lo.w_down, q4_roundtrip(lw.w_down, fdown))
    assert torch.equal(o.lm_head, q4_roundtrip(w.lm_head, Q6_K))
    assert not torch.equal(o.lm_head, q4_roundtrip(w.lm_head, 1))
