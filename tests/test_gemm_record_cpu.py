"""The GEMM entries refuse a bad call record before any HIP call (CPU-only: host pointers, the null stream).

A refusal is -1; a launch attempted without a GPU would return a HIP error code instead, so the value is asserted,
not merely that it is non-zero.
"""
import ctypes

import pytest

from cain_amd import ops

Q4_0, Q4_K, Q6_K = 0, 1, 2
_buf = (ctypes.c_char * 64)()  # stands for every buffer: no entry may read or launch on it


def _record(**fields):
    """A well-formed 16 x 256 GEMM of 4 rows on host pointers, with ``fields`` replaced."""
    p = ctypes.addressof(_buf)
    g = ops.CainGemm(W=p, sc=p, dd=p, X=p, Y=p, ldx=256, K=256, N=16, M=4, ldy=16, epi=ops.EPI_BF16)
    for k, v in fields.items():
        setattr(g, k, v)
    return g


@pytest.mark.parametrize("fields", [dict(fmt=Q4_K, tile0=1), dict(fmt=Q4_0, tile0=1), dict(fmt=Q6_K, K=128),
                                    dict(fmt=Q4_K, K=128, ldx=128), dict(fmt=3), dict(fmt=-1)])
def test_gguf_entry_refuses(fields):
    assert ops.load().cain_gemm_gguf(_record(**fields), None) == -1


@pytest.mark.parametrize("entry,kstep", [("cain_gemm_fp8", 64), ("cain_gemm_mxfp4", 128)])
def test_few_row_entries_refuse(entry, kstep):
    fn = getattr(ops.load(), entry)
    assert fn(_record(M=65), None) == -1
    assert fn(_record(M=0), None) == -1
    assert fn(_record(K=256 + kstep // 2), None) == -1


def test_head_size_refused_by_every_entry():
    """The fused QKV epilogue takes head sizes of whole 16-row tiles whose halves are whole groups of 8 pairs."""
    lib = ops.load()
    for entry in ("cain_gemm_bf16", "cain_gemm_fp8", "cain_gemm_mxfp4", "cain_gemm_gguf"):
        for hd in (24, 40):
            assert getattr(lib, entry)(_record(epi=ops.EPI_QKV_ROPE, H=1, Hkv=1, hd=hd, T_max=16), None) == -1, entry
