#!/usr/bin/env python3
"""Bit-for-bit A/B of the wide GEMMs (csrc/wgemm.hip, wgemm8.hip) between two builds of the kernel library.

    CAIN_KERNELS_LIB=<other build> python tools/wide_ab.py dump a.pt
    python tools/wide_ab.py dump b.pt
    python tools/wide_ab.py compare a.pt b.pt

``dump`` runs every case with fixed seeds on the loaded library and saves each output tensor (the K / V^T caches
of the QKV epilogue and the bf16 chunk maxima included); ``compare`` counts the tensors that are not
``torch.equal``.  The shapes are the small ones at which each shared piece of the two kernels can go wrong: partial
column blocks (N 48, 208), eight column blocks with split-K (N 1024: the XCD-local placement), K giving 1, 4 and 8
splits, rows on both sides of the 128-row tile, every epilogue (QKV with head size 32 and one inactive row), and
for bf16 the norm, both slab formats, per-shape split counts (9 splits at K 4608: the runtime-count combine) and
the in-launch combine modes.
"""
from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cain_amd import ops  # noqa: E402
from cain_amd.models.weights import (pack_mfma_a, pack_mfma_a_fp8_k128, pack_mxfp4, quantize_fp8_rows,  # noqa: E402
                                     quantize_mxfp4)

PLAIN = [ops.EPI_BF16, ops.EPI_RESID, ops.EPI_F32, ops.EPI_SILU, ops.EPI_GELU]
HD, T_MAX, SLOTS = 32, 64, 256
QKV_HEADS = {96: (1, 1), 224: (5, 1), 1024: (24, 4)}  # N -> (H, Hkv) at head size 32


class Runner:
    def __init__(self, dev):
        self.dev, self.out, self.cases = dev, {}, 0
        self._w, self._x = {}, {}

    def gen(self, seed):
        return torch.Generator(device=self.dev).manual_seed(seed)

    def weights(self, fmt, N, K):
        if (fmt, N, K) not in self._w:
            W = (torch.randn(N, K, device=self.dev, generator=self.gen(N * 7 + K)) * 0.05).bfloat16()
            if fmt == "bf16":
                p = (pack_mfma_a(W),)
            elif fmt == "fp8":
                q, s = quantize_fp8_rows(W)
                p = (pack_mfma_a_fp8_k128(q), s.contiguous())
            else:
                p = pack_mxfp4(*quantize_mxfp4(W))
            self._w[(fmt, N, K)] = p
        return self._w[(fmt, N, K)]

    def x(self, M, K):
        if (M, K) not in self._x:
            x = torch.randn(M, K, device=self.dev, generator=self.gen(M * 3 + K)).bfloat16()
            x[M // 2] *= 64  # a row of outliers (the scaled fp16 slabs)
            self._x[(M, K)] = x
        return self._x[(M, K)]

    def run(self, tag, fmt, N, K, M, epi, norm):
        dev, g = self.dev, self.gen(N + K + M + epi)
        w, x = self.weights(fmt, N, K), self.x(M, K)
        kw, keep = dict(norm=bool(norm), eps=1e-6), {}
        n_out = N // 2 if epi in (ops.EPI_SILU, ops.EPI_GELU) else N
        if epi == ops.EPI_BF16:
            kw["bias"] = torch.randn(N, device=dev, generator=g)
        if epi == ops.EPI_RESID:
            kw["out"] = torch.randn(M, N, device=dev, generator=g).bfloat16()
        if epi == ops.EPI_QKV_ROPE:
            H, Hkv = QKV_HEADS[N]
            kc = torch.zeros(SLOTS, Hkv, T_MAX, HD, device=dev, dtype=torch.bfloat16)
            vt = torch.zeros(SLOTS, Hkv, HD, T_MAX, device=dev, dtype=torch.bfloat16)
            slot = torch.randperm(SLOTS, device=dev, generator=g)[:M].int()
            slot[M // 3] = -1  # one inactive row
            pos = torch.randint(0, T_MAX, (M,), device=dev, generator=g).int()
            ang = torch.rand(T_MAX, HD // 2, device=dev, generator=g) * 6.28
            rope = dict(kc=kc, vtc=vt, slot=slot, pos=pos, cos_t=ang.cos(), sin_t=ang.sin(), H=H, Hkv=Hkv, hd=HD)
            kw["bias"] = torch.randn(N, device=dev, generator=g)
            q = torch.zeros(M, H * HD, device=dev, dtype=torch.bfloat16)
            keep.update(kc=kc, vt=vt)
            if fmt == "bf16":
                ops.qkv_rope(w[0], x, N, q, kc, vt, slot, pos, rope["cos_t"], rope["sin_t"], H, Hkv, HD, bias=kw["bias"],
                             norm=bool(norm), eps=1e-6)
            else:
                (ops.gemm_w8a8 if fmt == "fp8" else ops.gemm_w4a8)(*w, x, N, epi, out=q, rope=rope, **kw)
            keep["y"] = q
        elif fmt == "bf16":
            if epi == ops.EPI_F32:  # the chunk maxima, where this path writes them
                cm = torch.full((M, N // 16), -1.0, device=dev)
                ops.load().cain_gemm_set_cmax(ops._p(cm))
                keep["cmax"] = cm
            keep["y"] = ops.skinny_gemm(w[0], x, N, epi, **kw)
            if epi == ops.EPI_F32:
                ops.load().cain_gemm_cmax_take()
        else:
            keep["y"] = (ops.gemm_w8a8 if fmt == "fp8" else ops.gemm_w4a8)(*w, x, N, epi, **kw)
        assert keep["y"].shape[1] == (QKV_HEADS[N][0] * HD if epi == ops.EPI_QKV_ROPE else n_out)
        torch.cuda.synchronize()
        for k, v in keep.items():
            self.out[f"{tag} {fmt} N{N} K{K} M{M} epi{epi} norm{norm} {k}"] = v.cpu()
        self.cases += 1


def dump(path):
    dev = torch.device("cuda")
    ops.load()
    r = Runner(dev)
    epis = lambda N: PLAIN if N in (48, 208) else PLAIN + [ops.EPI_QKV_ROPE]  # noqa: E731
    ns = (48, 96, 208, 224, 1024)
    for variant in (0, 4):
        ops.set_wide_gemm_variant(variant)
        for N in ns:
            for K in (256, 512, 2048, 4096):
                for M in (65, 129, 256):
                    for norm in (0, 1):
                        for epi in ([ops.EPI_QKV_ROPE] if N in (96, 224) else epis(N)):
                            r.run(f"v{variant}", "bf16", N, K, M, epi, norm)
        for ks in (2, 3, 9):
            for N in (208, 1024):
                for K in (4096, 4608):
                    for M in (129, 256):
                        ops.set_wide_gemm_plan(N, K, 128 if M <= 128 else 256, ks)
                        for norm in (0, 1):
                            for epi in (ops.EPI_F32, ops.EPI_RESID):
                                r.run(f"v{variant} ks{ks}", "bf16", N, K, M, epi, norm)
            ops.clear_wide_gemm_plans()
        for mode in (1, 2):
            ops.set_wide_gemm_inline(mode)
            for N in (208, 1024):
                for K in (2048, 4096):
                    for M in (129, 256):
                        for norm in (0, 1):
                            for epi in (ops.EPI_F32, ops.EPI_RESID, ops.EPI_BF16):
                                r.run(f"v{variant} inline{mode}", "bf16", N, K, M, epi, norm)
        ops.set_wide_gemm_inline(0)
    ops.set_wide_gemm_variant(0)
    for fmt in ("fp8", "fp4"):
        for N in ns:
            for K in (512, 2048, 4096):
                for M in (17, 128, 129, 256):
                    for norm in (0, 1):
                        for epi in ([ops.EPI_QKV_ROPE] if N in (96, 224) else epis(N)):
                            r.run("a8", fmt, N, K, M, epi, norm)
    torch.save(r.out, path)
    print(f"{os.environ.get('CAIN_KERNELS_LIB', 'default library')}: {r.cases} cases, {len(r.out)} tensors -> {path}")


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    assert a.keys() == b.keys(), "the two dumps ran different cases"
    bits = lambda t: t.contiguous().view(torch.uint8)  # noqa: E731
    bad = [k for k in a if not (a[k].dtype == b[k].dtype and torch.equal(bits(a[k]), bits(b[k])))]
    cases = len({k.rsplit(" ", 1)[0] for k in a})
    for k in bad[:40]:
        print("DIFFERS", k)
    print(f"{cases} cases, {len(a)} tensors, {len(bad)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
