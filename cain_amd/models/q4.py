"""GGUF 4-bit weights (llama.cpp's Q4_0 and Q4_K) for the native Q4 kernel (``ops/csrc/gemm_qstream.hip``).

The reference's models are Ollama pulls whose default builds are Q4_0 / Q4_K_M GGUF files
(/root/reference/README.md:29-30; tags at /root/reference/experiment/RunnerConfig.py:80).  Round 5 dequantised such
files and re-quantised them to MXFP4, a different 4-bit grid.  Here the block VALUES stay exactly as the file stores
them and only their layout changes:

* ``q4_fields``: ggml block bytes -> codes (uint8 0..15 per weight) plus the block scales -- Q4_0: fp16 ``d`` per 32;
  Q4_K: 6-bit ``sc`` / ``m`` per 32 and fp16 ``d`` / ``dmin`` per 256 (decoded as ggml's ``get_scale_min_k4``,
  ``gguf._k_scale_min``);
* ``pack_q4``: the fields -> the kernel's tile layout (gemm_qstream.hip header), one byte buffer of scales
  ``[sc: N K / 16][Q4_K (d, dmin): N K / 64][optional fp32 gain: K]``;
* ``quantize_q4_0`` / ``quantize_q4_k``: weights -> ggml block bytes (random-init models in a GGUF format: the
  bench's ``--weights q4_0 / q4_k`` rows), ``dequantize_q4``: bytes -> fp32 (gguf.py's decoders, the oracle).

Q4_K's quantiser is a plain min/max fit (per 32: scale (max - min) / 15, min -min; per 256: d, dmin = the largest
/ 63), not llama.cpp's iterative ``make_qkx2_quants`` search: the kernel runs whatever valid blocks a file holds,
and random weights only need valid blocks of the right layout.

Q6_K (format id ``Q6_K`` = 2; ``ops/csrc/gemm_qstream.hip``) is the type a Q4_K_M file keeps its output head and part of
its ``attn_v`` / ``ffn_down`` tensors in: ``q6_fields`` / ``pack_q6`` / ``quantize_q6_k`` are its members of the same
three steps, ``gguf_q4_native`` keeps such tensors as stored beside the plan's 4-bit format, and ``q4_k_m_formats``
is the per-matrix mix ``weight_dtype="q4_k_m"`` lays random or Hugging Face weights out in.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from .gguf import _k_scale_min, dequantize

Q4_FORMATS = {"q4_0": 0, "q4_k": 1}  # csrc/gemm_q.h Q4F_*
Q6_K = 2                              # csrc/gemm_q.h Q6F_K
_BLOCK_BYTES = {0: 18, 1: 144, 2: 210}
_BLOCK_ELEMS = {0: 32, 1: 256, 2: 256}
GGML_TYPE = {0: 2, 1: 12, 2: 14}  # ggml type ids of Q4_0 / Q4_K / Q6_K


def _fp16_bytes(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float16).contiguous().view(torch.uint8).reshape(*x.shape, 2)


def quantize_q4_0(w: torch.Tensor) -> torch.Tensor:
    """ggml Q4_0 blocks of ``w`` [N, K] (K % 32 == 0) as uint8 [N, K / 32, 18] (ggml's quantize_row_q4_0_ref: d =
    the signed value of largest magnitude / -8, q = clamp(floor(x / d + 8.5), 0, 15), low nibbles the first 16)."""
    n, k = w.shape
    x = w.float().reshape(n, k // 32, 32)
    idx = x.abs().argmax(-1, keepdim=True)
    d = torch.gather(x, -1, idx) / -8.0  # ggml takes the codes with the fp32 d, then stores d as fp16
    inv = torch.where(d != 0, 1.0 / torch.where(d != 0, d, torch.ones_like(d)), torch.zeros_like(d))
    q = torch.clamp(torch.floor(x * inv + 8.5), 0, 15).to(torch.uint8)
    qs = q[..., :16] | (q[..., 16:] << 4)
    return torch.cat([_fp16_bytes(d[..., 0]), qs], -1).contiguous()


def quantize_q4_k(w: torch.Tensor) -> torch.Tensor:
    """Q4_K blocks of ``w`` [N, K] (K % 256 == 0) as uint8 [N, K / 256, 144]: [d fp16][dmin fp16][12 bytes of 6-bit
    (sc, m) pairs][128 bytes of codes], w = d sc q - dmin m (see the module doc for the fit)."""
    n, k = w.shape
    x = w.float().reshape(n, k // 256, 8, 32)
    mn = torch.clamp(x.amin(-1), max=0.0)                    # [n, sb, 8]
    mx = x.amax(-1)
    scale = torch.clamp(mx - mn, min=0.0) / 15.0
    mins = -mn
    d = scale.amax(-1) / 63.0                                 # [n, sb]
    dmin = mins.amax(-1) / 63.0
    d16, dmin16 = d.to(torch.float16).float(), dmin.to(torch.float16).float()
    safe = lambda v: torch.where(v > 0, v, torch.ones_like(v))  # noqa: E731
    sc = torch.where(d16[..., None] > 0, torch.round(scale / safe(d16)[..., None]), torch.zeros_like(scale))
    m = torch.where(dmin16[..., None] > 0, torch.round(mins / safe(dmin16)[..., None]), torch.zeros_like(mins))
    sc, m = sc.clamp(0, 63), m.clamp(0, 63)
    s = d16[..., None] * sc                                   # effective per-32 scale and offset
    o = dmin16[..., None] * m
    q = torch.where(s[..., None] > 0, torch.round((x + o[..., None]) / safe(s)[..., None]), torch.zeros_like(x))
    q = q.clamp(0, 15).to(torch.uint8)                        # [n, sb, 8, 32]
    sci, mi = sc.to(torch.uint8), m.to(torch.uint8)
    scales = torch.cat([sci[..., :4] | ((sci[..., 4:] >> 4) << 6), mi[..., :4] | ((mi[..., 4:] >> 4) << 6),
                        (sci[..., 4:] & 0x0F) | ((mi[..., 4:] & 0x0F) << 4)], -1)  # inverse of _k_scale_min
    qp = q.reshape(n, k // 256, 4, 2, 32)                     # 4 groups of 64: sub-block 2g low, 2g + 1 high
    qs = (qp[..., 0, :] | (qp[..., 1, :] << 4)).reshape(n, k // 256, 128)
    return torch.cat([_fp16_bytes(d), _fp16_bytes(dmin), scales, qs], -1).contiguous()


def quantize_q6_k(w: torch.Tensor) -> torch.Tensor:
    """Q6_K blocks of ``w`` [N, K] (K % 256 == 0) as uint8 [N, K / 256, 210]: [ql 128: low nibbles][qh 64: high bit
    pairs][16 int8 group scales][d fp16], w = d sc (q - 32), q in 0..63, one sc per 16 elements.  A plain fit, not
    llama.cpp's ``make_qx_quants`` error search: per group the scale is (the signed value of largest magnitude) /
    -32, the sign ggml picks so that this value lands on the code 0 exactly (so about half the scales are
    negative); per super-block d = the largest |scale| / 127 and sc = round(scale / d); the codes are then taken
    with the scale the block really stores, d sc."""
    n, k = w.shape
    x = w.float().reshape(n, k // 256, 16, 16)
    idx = x.abs().argmax(-1, keepdim=True)
    scale = torch.gather(x, -1, idx)[..., 0] / -32.0              # [n, sb, 16]
    d = scale.abs().amax(-1) / 127.0                              # [n, sb]
    d16 = d.to(torch.float16).float()
    safe = lambda v: torch.where(v != 0, v, torch.ones_like(v))  # noqa: E731
    sc = torch.where(d16[..., None] > 0, torch.round(scale / safe(d16)[..., None]), torch.zeros_like(scale))
    sc = sc.clamp(-128, 127)
    s = d16[..., None] * sc                                       # the scale the decoder applies
    q = torch.where(s[..., None] != 0, torch.round(x / safe(s)[..., None]), torch.zeros_like(x))
    q = (q.clamp(-32, 31) + 32).to(torch.uint8).reshape(n, k // 256, 2, 4, 32)  # [half, quarter, l]: 128 h + 32 j + l
    lo, hi = q & 15, q >> 4
    ql = torch.cat([lo[..., 0, :] | (lo[..., 2, :] << 4), lo[..., 1, :] | (lo[..., 3, :] << 4)], -1)  # [n, sb, 2, 64]
    qh = hi[..., 0, :] | (hi[..., 1, :] << 2) | (hi[..., 2, :] << 4) | (hi[..., 3, :] << 6)            # [n, sb, 2, 32]
    return torch.cat([ql.reshape(n, k // 256, 128), qh.reshape(n, k // 256, 64),
                      sc.to(torch.int8).view(torch.uint8), _fp16_bytes(d)], -1).contiguous()


def quantize_q4(w: torch.Tensor, fmt: int) -> torch.Tensor:
    """``w`` [N, K] as ggml blocks of format id ``fmt`` (0 Q4_0, 1 Q4_K, 2 Q6_K)."""
    return quantize_q4_0(w) if fmt == 0 else quantize_q4_k(w) if fmt == 1 else quantize_q6_k(w)


def dequantize_q4(blocks: torch.Tensor, fmt: int, n: int, k: int) -> torch.Tensor:
    """fp32 [N, K] values of ggml block bytes (the decoders of ``gguf.py``: the kernel's oracle)."""
    return dequantize(blocks.reshape(-1), GGML_TYPE[fmt], n * k).reshape(n, k)


def q4_fields(blocks: torch.Tensor, fmt: int, n: int, k: int) -> Dict[str, torch.Tensor]:
    """ggml block bytes (any shape holding N K / elems blocks, rows in order) -> codes uint8 [N, K] in 0..15 and the
    scale fields: Q4_0 ``d`` fp16 [N, K / 32]; Q4_K ``sc`` / ``m`` uint8 [N, K / 32], ``d`` / ``dmin`` fp16
    [N, K / 256].  Bit-exact: no value is recomputed."""
    bb, be = _BLOCK_BYTES[fmt], _BLOCK_ELEMS[fmt]
    b = blocks.reshape(n, k // be, bb)
    if fmt == 0:
        qs = b[..., 2:18]
        codes = torch.cat([qs & 15, qs >> 4], -1).reshape(n, k)
        return {"codes": codes.contiguous(), "d": b[..., 0:2].contiguous().view(torch.float16)[..., 0]}
    sc, mn = _k_scale_min(b[..., 4:16].reshape(-1, 12))
    qs = b[..., 16:144].reshape(n, k // 256, 4, 32)
    codes = torch.stack([qs & 15, qs >> 4], 3).reshape(n, k)  # [sb, group, low / high, 32] = element order
    return {"codes": codes.contiguous(), "sc": sc.to(torch.uint8).reshape(n, k // 32),
            "m": mn.to(torch.uint8).reshape(n, k // 32),
            "d": b[..., 0:2].contiguous().view(torch.float16)[..., 0],
            "dmin": b[..., 2:4].contiguous().view(torch.float16)[..., 0]}


def q6_fields(blocks: torch.Tensor, n: int, k: int) -> Dict[str, torch.Tensor]:
    """ggml Q6_K block bytes (any shape holding N K / 256 blocks, rows in order) -> ``codes`` uint8 [N, K] in 0..63,
    ``sc`` int8 [N, K / 16] and ``d`` fp16 [N, K / 256].  Bit-exact: no value is recomputed."""
    b = blocks.reshape(n, k // 256, 210)
    ql = b[..., 0:128].reshape(n, k // 256, 2, 64)
    qh = b[..., 128:192].reshape(n, k // 256, 2, 32)
    q = torch.stack([(ql[..., :32] & 15) | ((qh & 3) << 4), (ql[..., 32:] & 15) | (((qh >> 2) & 3) << 4),
                     (ql[..., :32] >> 4) | (((qh >> 4) & 3) << 4), (ql[..., 32:] >> 4) | ((qh >> 6) << 4)], 3)
    return {"codes": q.reshape(n, k).contiguous(),       # [sb, half, quarter, 32] = element order
            "sc": b[..., 192:208].contiguous().view(torch.int8).reshape(n, k // 16),
            "d": b[..., 208:210].contiguous().view(torch.float16)[..., 0]}


def pack_q6(fields: Dict[str, torch.Tensor], gain: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``q6_fields`` -> (codes uint8 [N / 16, K / 128, 1536], scale buffer uint8) in gemm_qstream.hip's layout: per (tile,
    128-k quad) [64 lanes x 16 bytes of low nibbles][64 lanes x 8 bytes of high bit pairs], lane l = 16 g + r holding
    row 16 t + r; group s of the quad (k = 128 p + 16 s + 4 g + j) sits in byte j of low dword s >> 1 (nibble s & 1)
    and of high dword s >> 2 (bits 2 (s & 3)).  The scale buffer is [per (t, p, r): 8 int8 group scales][per (t,
    super-block, r): d as fp32][gain]: 6 + 0.5 + 0.125 bits per weight."""
    codes = fields["codes"]
    n, k = codes.shape
    if n % 16 or k % 256:
        raise ValueError(f"pack_q6 needs N % 16 == 0 and K % 256 == 0, got {tuple(codes.shape)}")
    nt, kq = n // 16, k // 128
    lo = (codes & 15).reshape(nt, 16, kq, 4, 2, 4, 4)           # [t, r, p, dword, nibble, g, j]
    lo = lo.permute(0, 2, 5, 1, 3, 6, 4)                        # [t, p, g, r, dword, j, nibble]
    lo = (lo[..., 0] | (lo[..., 1] << 4)).reshape(nt, kq, 1024)
    hi = (codes >> 4).reshape(nt, 16, kq, 2, 4, 4, 4)           # [t, r, p, dword, pair, g, j]
    hi = hi.permute(0, 2, 5, 1, 3, 6, 4)                        # [t, p, g, r, dword, j, pair]
    hi = (hi[..., 0] | (hi[..., 1] << 2) | (hi[..., 2] << 4) | (hi[..., 3] << 6)).reshape(nt, kq, 512)
    wq = torch.cat([lo, hi], -1).contiguous()
    sc = fields["sc"].reshape(nt, 16, kq, 8).permute(0, 2, 1, 3).contiguous().view(torch.uint8).reshape(-1)
    d = fields["d"].float().reshape(nt, 16, k // 256).permute(0, 2, 1).contiguous().view(torch.uint8).reshape(-1)
    parts = [sc, d]
    if gain is not None:
        parts.append(gain.float().contiguous().view(torch.uint8).reshape(-1))
    return wq, torch.cat(parts).contiguous()


def pack_q4(fields: Dict[str, torch.Tensor], fmt: int, gain: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor,
                                                                                                      torch.Tensor]:
    """``q4_fields`` -> (codes uint8 [N / 16, K / 128, 64, 16], scale buffer uint8) in gemm_qstream.hip's layout: lane
    l = 16 g + r of quad p holds row 16 t + r, k = 128 p + 32 s + 8 g + j at dword s, byte j & 3, nibble j >> 2; the
    scale buffer is [per (t, p, r): 4 x 2 bytes of block scales][Q4_K: per (t, super-block, r) (d, dmin)][gain]."""
    codes = fields["codes"]
    n, k = codes.shape
    if n % 16 or k % 256:
        raise ValueError(f"pack_q4 needs N % 16 == 0 and K % 256 == 0, got {tuple(codes.shape)}")
    nt, kq = n // 16, k // 128
    t = codes.reshape(nt, 16, kq, 4, 4, 2, 4)              # [t, r, p, s, g, h, b]
    t = t.permute(0, 2, 4, 1, 3, 6, 5)                     # [t, p, g, r, s, b, h]
    wq = (t[..., 0] | (t[..., 1] << 4)).contiguous().reshape(nt, kq, 64, 16)

    def tiles(x16: torch.Tensor) -> torch.Tensor:          # [N, K / 32] 16-bit -> [t, p, r, 4 blocks] bytes
        return x16.reshape(nt, 16, kq, 4).permute(0, 2, 1, 3).contiguous().view(torch.uint8).reshape(-1)

    if fmt == 0:
        parts = [tiles(fields["d"].contiguous().view(torch.int16))]
    else:
        scm = fields["sc"].to(torch.int16) | (fields["m"].to(torch.int16) << 8)
        dd = torch.stack([fields["d"], fields["dmin"]], -1).contiguous().view(torch.int32)[..., 0]  # [N, K / 256]
        parts = [tiles(scm), dd.reshape(nt, 16, k // 256).permute(0, 2, 1).contiguous().view(torch.uint8).reshape(-1)]
    if gain is not None:
        parts.append(gain.float().contiguous().view(torch.uint8).reshape(-1))
    return wq, torch.cat(parts).contiguous()


def quant_pack_q4(w: torch.Tensor, fmt: int, gain: Optional[torch.Tensor] = None):
    """Quantise ``w`` [N, K] to ggml blocks and pack them: (codes, scale buffer)."""
    return pack_native(quantize_q4(w, fmt), fmt, gain)


def q4_roundtrip(w: torch.Tensor, fmt: int) -> torch.Tensor:
    """The values a Q4 engine multiplies by: dequant(quant(w)), in w's dtype (the torch oracle)."""
    n, k = w.shape
    return dequantize_q4(quantize_q4(w, fmt), fmt, n, k).to(w.dtype)




def q4_k_m_formats(cfg) -> Dict[str, object]:
    """The per-matrix format ids of ``weight_dtype="q4_k_m"``: llama.cpp's Q4_K_M mix (``gguf.q4_k_m_type``) over
    this engine's matrices -- {"layers": [{wqkv, wv, wo, wgu, w_down}], "lm_head"}; ``wv`` differs from ``wqkv`` in
    the layers whose V rows are Q6_K (a launch of their own, runtime.hip)."""
    from .gguf import q4_k_m_type

    ids = {"Q4_K": 1, "Q6_K": Q6_K}
    layers = []
    for i in range(cfg.n_layers):
        t = lambda x: ids[q4_k_m_type(f"blk.{i}.{x}.weight", cfg.n_layers)]  # noqa: E731
        layers.append({"wqkv": t("attn_q"), "wv": t("attn_v"), "wo": t("attn_output"), "wgu": t("ffn_gate"),
                       "w_down": t("ffn_down")})
    return {"layers": layers, "lm_head": ids[q4_k_m_type("output.weight", cfg.n_layers)]}


def gguf_q4_native(g, cfg, fmt: int, device="cpu") -> Dict[str, object]:
    """A GGUF file's GEMM weights as ggml blocks (uint8 [N, K / elems, bytes]) in the engine's natural row order --
    the same row operations as ``gguf.load_gguf_weights`` (Llama q / k un-permuted, q / k / v concatenated, Phi-3's
    fused gate/up split), applied to whole rows of blocks, so no value changes.  A tensor stored as ``fmt`` (the
    plan's 4-bit format) or as Q6_K (a Q4_K_M file's output head and part of its attn_v / ffn_down) stays as stored;
    each matrix's format id is recorded under ``fmts``.  The fused QKV takes one format: where V's differs from q /
    k's (Q4_K_M), V is returned on its own under ``wv`` and ``wqkv`` holds the q and k rows only.  What is
    quantised to ``fmt`` from its decoded values instead, and listed under ``requantized``: tensors of any other
    type (Q5_K, Q8_0, F16 ...), q and k when their types differ from each other, and a Q6_K gate / up (gemm_qstream.hip
    has no gate/up activation epilogue).  Result: {"fmt", "layers": [{wqkv, [wv,] wo, w_gate, w_up, w_down, fmts}],
    "lm_head", "lm_head_fmt", "requantized"}, attached to ``ModelWeights.native`` for ``pack_for_engine``."""
    import numpy as np

    from .gguf import unpermute_qk

    arch = g.metadata["general.architecture"]
    requant = []

    def stored(name: str) -> Optional[int]:  # the format id the tensor can run as stored in
        return next((f for f in (fmt, Q6_K) if g.tensors[name].type == GGML_TYPE[f]), None)

    def blocks(name: str, q6: bool = True) -> Tuple[torch.Tensor, int]:
        t = g.tensors[name]
        n, k = t.shape
        f = stored(name)
        if f is not None and (q6 or f == fmt):
            return torch.from_numpy(np.array(g.raw(name))).to(device).reshape(n, k // _BLOCK_ELEMS[f],
                                                                              _BLOCK_BYTES[f]), f
        requant.append(f"{name} ({t.type_name})")
        return quantize_q4(g.tensor(name, device=device, dtype=torch.float32), fmt), fmt

    f = cfg.ffn
    layers = []
    for i in range(cfg.n_layers):
        p = f"blk.{i}."
        lw: Dict[str, object] = {}
        fm: Dict[str, int] = {}
        if g.has(p + "attn_qkv.weight"):
            qkv, fm["wqkv"] = blocks(p + "attn_qkv.weight")
        else:
            v, fv = blocks(p + "attn_v.weight")
            # q / k stay Q6_K only beside a Q6_K V: a separate V launch is always gemm_q6's (it takes the tile offset)
            same = stored(p + "attn_q.weight") == stored(p + "attn_k.weight") and fv == Q6_K
            (q, fq), (kk, _) = blocks(p + "attn_q.weight", same), blocks(p + "attn_k.weight", same)
            if arch == "llama":
                q, kk = unpermute_qk(q, cfg.n_heads), unpermute_qk(kk, cfg.n_kv_heads)
            fm["wqkv"] = fq
            if fv == fq:
                qkv = torch.cat([q, kk, v], 0)
            else:
                qkv, lw["wv"], fm["wv"] = torch.cat([q, kk], 0), v.contiguous(), fv
        if g.has(p + "ffn_gate.weight"):
            (gate, _), (up, _) = blocks(p + "ffn_gate.weight", False), blocks(p + "ffn_up.weight", False)
        else:  # phi3: ffn_up = [gate; up]
            gu, _ = blocks(p + "ffn_up.weight", False)
            gate, up = gu[:f].contiguous(), gu[f:].contiguous()
        fm["wgu"] = fmt
        lw["wo"], fm["wo"] = blocks(p + "attn_output.weight")
        lw["w_down"], fm["w_down"] = blocks(p + "ffn_down.weight")
        lw.update({"wqkv": qkv.contiguous(), "w_gate": gate, "w_up": up, "fmts": fm})
        layers.append(lw)
    lm, flm = blocks("output.weight") if g.has("output.weight") else blocks("token_embd.weight")
    return {"fmt": fmt, "layers": layers, "lm_head": lm, "lm_head_fmt": flm, "requantized": requant}


def pack_native(blocks: torch.Tensor, fmt: int, gain: Optional[torch.Tensor] = None,
                rows: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Pack ggml blocks [N, K / elems, bytes] of format id ``fmt`` (rows reordered by ``rows`` first) for their
    kernel (``pack_q4`` / ``pack_q6``), the RMSNorm gain appended unfolded (a file's values stay exact)."""
    n = blocks.shape[0]
    k = blocks.shape[1] * _BLOCK_ELEMS[fmt]
    b = (blocks if rows is None else blocks[rows]).contiguous()
    if fmt == Q6_K:
        return pack_q6(q6_fields(b, n, k), gain)
    return pack_q4(q4_fields(b, fmt, n, k), fmt, gain)
