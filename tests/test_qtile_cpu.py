"""How often the GGUF GEMM entries stream their weights (``ops.gemm_q_passes``, ``csrc/gemm_qtile.hip``) under every
``ops.set_q_tile`` mode: host arithmetic only, no kernel launch, no GPU."""
import pytest

from cain_amd import ops

F32, BF16, RESID, QKV = ops.EPI_F32, ops.EPI_BF16, ops.EPI_RESID, ops.EPI_QKV_ROPE
Q4_0, Q4_K, Q6_K = 0, 1, 2
PASS_CASES = [(Q4_K, 14336, 64, RESID), (Q6_K, 4096, 20, F32), (Q4_K, 4096, 65, BF16)]


@pytest.fixture(autouse=True)
def _rule_afterwards():
    yield
    ops.set_q_tile(-1)


def stream_rows(fmt, K, epi):
    lib = ops.load()
    return int((lib.cain_gemm_q6_rows if fmt == Q6_K else lib.cain_gemm_q4_rows)(K, epi))


def test_pass_counts_under_every_mode():
    ops.set_q_tile(-1)
    assert ops.gemm_q_passes(Q4_K, 14336, 64, RESID) == 1
    assert ops.gemm_q_passes(Q6_K, 4096, 20, F32) == 1
    assert ops.gemm_q_passes(Q4_K, 4096, 65, BF16) == 2
    ops.set_q_tile(0)
    for fmt, K, M, epi in PASS_CASES:
        assert ops.gemm_q_passes(fmt, K, M, epi) == -(-M // stream_rows(fmt, K, epi))
    assert ops.gemm_q_passes(Q4_K, 14336, 64, RESID) == 64
    ops.set_q_tile(1)
    for fmt, K, M, epi in PASS_CASES:
        assert ops.gemm_q_passes(fmt, K, M, epi) == -(-M // 64)
    assert ops.gemm_q_passes(Q4_K, 4096, 1, BF16) == 1


def test_rule_keeps_few_rows_on_the_stream_kernels():
    """The measured crossovers (profiles/r8/q_tile/README.md): one stream pass stays; below 8 rows stays; 8-16 rows
    move at 4 or more stream passes; from 17 rows every shape moves."""
    ops.set_q_tile(-1)
    for fmt in (Q4_0, Q4_K, Q6_K):
        for K in (1536, 4096, 14336):
            rows = stream_rows(fmt, K, RESID)
            for M in (1, 2, 4, 7):
                assert ops.gemm_q_passes(fmt, K, M, RESID) == -(-M // rows)  # the stream kernels
            for M in (8, 16):
                assert ops.gemm_q_passes(fmt, K, M, RESID) == (1 if -(-M // rows) >= 4 else -(-M // rows))
            for M in (17, 32, 64):
                assert ops.gemm_q_passes(fmt, K, M, RESID) == 1


@pytest.mark.parametrize("mode", [-1, 0, 1])
def test_oversized_k_has_no_pass_count(mode):
    ops.set_q_tile(mode)
    assert stream_rows(Q6_K, 25600, F32) == 0
    assert ops.gemm_q_passes(Q6_K, 25600, 64, F32) == -1 and ops.gemm_q_passes(Q6_K, 25600, 1, F32) == -1


def test_every_model_gemm_is_one_pass_at_64_rows():
    """Under the rule, every GEMM of the seven models at M = 64 streams its weights once, in each format q4_k_m
    gives it."""
    from cain_amd.models import MODELS

    ops.set_q_tile(-1)
    assert len(MODELS) == 7
    for name, c in MODELS.items():
        act = ops.EPI_GELU if "gemma" in name else ops.EPI_SILU
        roles = [(c.d_model, QKV, (Q4_K, Q6_K)), (c.q_dim, RESID, (Q4_K,)), (c.d_model, act, (Q4_K,)),
                 (c.ffn, RESID, (Q4_K, Q6_K)), (c.d_model, F32, (Q4_K, Q6_K))]
        for K, epi, fmts in roles:
            for fmt in fmts:
                assert ops.gemm_q_passes(fmt, K, 64, epi) == 1, (name, K, epi, fmt)
