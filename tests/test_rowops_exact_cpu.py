"""Host-side checks of the row-op references in ``tests/exact.py`` (quant_rows, embed, rmsnorm): the inputs of
``tests/test_rowops_exact_gpu.py`` land where they are meant to (e4m3 ties, subnormals, saturation), the comparators
accept the reference itself and reject a reference with a planted fault."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).parent))

import exact  # noqa: E402

SHAPES = [(M, K) for K in exact.QR_KS for M in exact.QR_MS]
ids = lambda v: f"M{v[0]}-K{v[1]}"  # noqa: E731


def test_e4m3_quantiser_written_from_the_format_is_pytorchs():
    """Every e4m3 value, every midpoint between neighbours and a point on either side of each midpoint: the
    round-to-nearest-even quantiser written out in ``exact.e4m3_quant`` agrees with PyTorch's conversion, and the
    round-half-away one differs from it on exactly the ties whose even neighbour is the lower one."""
    codes = torch.arange(0, 0x7F, dtype=torch.uint8).view(torch.float8_e4m3fn).double()  # 0 .. 448, ascending
    assert float(codes[-1]) == 448.0 and float(codes[1]) == 2.0 ** -9 and float(codes[8]) == 2.0 ** -6
    mid = (codes[1:] + codes[:-1]) / 2
    pts = torch.cat([codes, mid, mid * (1 + 2.0 ** -20), mid * (1 - 2.0 ** -20)])
    pts = torch.cat([pts, -pts])
    torch_q = pts.float().to(torch.float8_e4m3fn).double()
    assert torch.equal(exact.e4m3_quant(pts), torch_q)
    away = exact.e4m3_quant(pts, away=True)
    differ = away != torch_q
    is_mid = torch.cat([torch.zeros(len(codes), dtype=torch.bool), torch.ones(len(mid), dtype=torch.bool),
                        torch.zeros(2 * len(mid), dtype=torch.bool)]).repeat(2)
    assert bool((differ <= is_mid).all()) and int(differ.sum()) == 2 * ((len(mid) + 1) // 2)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_exact_family_lands_on_ties_subnormals_and_saturation(shape):
    M, K = shape
    x, e = exact.quant_exact_rows(M, K, K + M)
    scale, inv = exact.quant_scale(x)
    live = torch.ones(M, dtype=torch.bool)
    if M == 5:
        live[2] = False
        assert float(scale[2]) == 1.0 and bool((x[2] == 0).all())
        assert {0x00, 0x80} == set(exact.quant_rows_ref(x)[0][2].tolist())  # +0 and -0 keep their sign
    assert torch.equal(scale[live].double(), torch.pow(2.0, e[live].double()))  # exact powers of two, and so is inv
    assert torch.equal((scale * inv)[live], torch.ones(int(live.sum())))
    assert -6 <= int(e.min()) and int(e.max()) <= 3
    # amax sits in the row's last vector
    assert bool((x[live].float().abs().argmax(1) >= K - 8).all())
    y = x.double() * inv.double()[:, None]
    assert float(y.abs().max()) == 448.0 and bool(((y == 448).sum(1) == live).all()) and bool(((y == -448).sum(1) == live).all())
    b, xs = exact.quant_rows_ref(x)
    assert torch.equal(xs, scale.double())
    q = b.view(torch.float8_e4m3fn).double()
    assert torch.equal(q, exact.e4m3_quant(y))  # PyTorch's conversion = the format's RNE on these inputs
    step = torch.pow(2.0, (torch.frexp(y.abs())[1] - 1).clamp(min=-6).double() - 3)
    tie = ((y.abs() / step) % 1.0) == 0.5
    up, down = tie & (q.abs() > y.abs()), tie & (q.abs() < y.abs())
    sub = (y.abs() < 2.0 ** -6) & (y != 0)
    for m in live.nonzero().flatten().tolist():
        few = 3 if K > 8 else 1  # K = 8: six values beside the planted +-448
        assert int(up[m].sum()) >= few and int(down[m].sum()) >= few, (m, int(up[m].sum()), int(down[m].sum()))
        if K > 8:
            assert int((sub[m] & tie[m]).sum()) >= 2 and int((sub[m] & (q[m] == 0)).sum()) >= 1
            assert int((sub[m] & (q[m] != y[m]) & (q[m] != 0)).sum()) >= 1  # rounded onto the 2^-9 grid
            assert int(((y[m].abs() < 448) & (q[m].abs() == 448)).sum()) >= 1  # rounds up to the maximum
            assert int((b[m] == 0x80).sum()) >= 1 and int((b[m] == 0x00).sum()) >= 1
    # the comparator accepts the reference and names a single wrong byte
    assert exact.quant_exact_mismatch(x, b, xs.float()) is None
    bad = b.clone()
    bad[M - 1, K - 3] ^= 1
    rep = exact.quant_exact_mismatch(x, bad, xs.float())
    assert rep is not None and f"row {M - 1}, column {K - 3}" in rep and f"chunk {(K - 3) // 2048}" in rep


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_round_half_away_is_rejected(shape):
    M, K = shape
    x, _ = exact.quant_exact_rows(M, K, K + M)
    b, xs = exact.quant_rows_ref(x, away=True)
    rep = exact.quant_exact_mismatch(x, b, xs.float())
    assert rep is not None and rep.startswith("bytes")


@pytest.mark.parametrize("chunk", range(12))
def test_a_chunk_dropped_from_the_statistics_is_rejected(chunk):
    """K = 24,576: the exact family's comparator rejects a dropped last chunk (amax lives there), the norm-factor
    comparator a dropped chunk wherever it is (among five rows every chunk holds a non-zero)."""
    K, eps = exact.QR_MAXK, 1e-6
    x = exact.quant_norm_rows(5, K, K + 5)
    _, xs = exact.quant_rows_ref(x, norm=True, eps=eps, drop_chunk=chunk)
    rep = exact.quant_norm_mismatch(x, xs.float(), eps)
    assert rep is not None and "row" in rep
    for M in exact.QR_MS:
        xe, _ = exact.quant_exact_rows(M, K, K + M)
        b, s = exact.quant_rows_ref(xe, drop_chunk=chunk)
        assert (exact.quant_exact_mismatch(xe, b, s.float()) is not None) == (chunk == 11)
        xg = exact.quant_general_rows(M, K, K + M)
        amax_chunk = (xg.float().abs().argmax(1) // exact.QR_CHUNK).tolist()
        b, s = exact.quant_rows_ref(xg, drop_chunk=chunk)
        assert (exact.quant_general_mismatch(xg, b, s.float())[1] is not None) == (chunk in amax_chunk)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_general_family_bound_holds_for_the_reference(shape):
    M, K = shape
    x = exact.quant_general_rows(M, K, K + M)
    scale, _ = exact.quant_scale(x)
    assert all(torch.frexp(s)[0] != 0.5 for s in scale)  # no power of two: scale and inv round
    b, xs = exact.quant_rows_ref(x)
    ndiff, rep = exact.quant_general_mismatch(x, b, xs.float())
    assert (ndiff, rep) == (0, None)
    # two codes off, and half a step past the bound, are both reported
    bad = b.clone()
    bad[0, K // 2] = (int(bad[0, K // 2]) & 0x80) | ((int(bad[0, K // 2]) & 0x7F) + 2) % 0x7F
    ndiff, rep = exact.quant_general_mismatch(x, bad, xs.float())
    assert ndiff == 1 and rep is not None and f"column {K // 2}" in rep
    ndiff, rep = exact.quant_general_mismatch(x, b, xs.float() * (1 + 2.0 ** -22))
    assert rep is not None and rep.startswith("scale")


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_norm_rows_are_exact_and_every_non_zero_counts(shape):
    M, K = shape
    x = exact.quant_norm_rows(M, K, K + M).double()
    nz = (x != 0).sum(1)
    assert bool((nz == min(16, K)).all()) and float(x.abs().max()) <= 4 and torch.equal(x, x.round())
    assert bool((x[:, 0] != 0).all()) and bool((x[:, -1] != 0).all())
    if K > exact.QR_CHUNK:  # both sides of the last chunk boundary, and all four waves' ranges of one chunk
        last = (K - 1) // exact.QR_CHUNK * exact.QR_CHUNK
        assert bool((x[:, last - 1] != 0).all()) and bool((x[:, last] != 0).all())
    if K >= exact.QR_CHUNK:
        waves = (x != 0).nonzero()[:, 1] % exact.QR_CHUNK // 512
        assert set(waves.tolist()) == {0, 1, 2, 3}
    eps = 1e-6
    xb = x.bfloat16()
    _, xs = exact.quant_rows_ref(xb, norm=True, eps=eps)
    assert exact.quant_norm_mismatch(xb, xs.float(), eps) is None
    # dropping the smallest non-zero of a row moves xs by far more than the tolerance
    ss = x.pow(2).sum(1)
    assert float(ss.max()) <= 256
    m = M - 1
    k = int((x[m].abs() + (x[m] == 0) * 9).argmin())
    y = xb.clone()
    y[m, k] = 0
    if float(y[m].float().abs().max()) == float(xb[m].float().abs().max()):  # same amax: only the sum changed
        _, xs_bad = exact.quant_rows_ref(y, norm=True, eps=eps)
        assert abs(float(xs_bad[m] / xs[m]) - 1) > 1.0 / 600 > 1000 * exact.QR_NORM_RTOL
        assert exact.quant_norm_mismatch(xb, xs_bad.float(), eps) is not None


@pytest.mark.parametrize("d", exact.EMBED_DS)
def test_embed_reference_and_its_tokens(d):
    for M in exact.EMBED_MS:
        E, tok = exact.embed_case(M, d, d + M)
        assert int(tok[0]) == 0 and (M == 1 or (int(tok[1]) == int(tok[-1]) == E.shape[0] - 1))
        assert M == 1 or len(set(tok.tolist())) < M
        one, gemma = exact.embed_scales(d)
        assert one == 1.0 and gemma == float(torch.tensor(gemma).bfloat16()) and abs(gemma / d ** 0.5 - 1) < 2.0 ** -8
        assert torch.equal(exact.bits16(exact.embed_ref(E, tok, one)), exact.bits16(E[tok.long()]))
        ref = exact.embed_ref(E, tok, gemma)
        assert bool(ref.float().isfinite().all())
        # the product really rounds: a truncating kernel would differ
        trunc = ((E[tok.long()].float() * gemma).view(torch.int32) & ~0xFFFF).view(torch.float32).bfloat16()
        assert int((exact.bits16(trunc) != exact.bits16(ref)).sum()) > ref.numel() // 4


@pytest.mark.parametrize("d", exact.NORM_DS)
def test_rmsnorm_reference_accepts_itself_and_rejects_two_steps(d):
    x, g = exact.rmsnorm_case(3, d, d)
    assert float(x.double().pow(2).sum(1).max()) < 2 ** 24
    ref = exact.rmsnorm_ref(x, g, 1e-6)
    assert exact.rmsnorm_mismatch(ref, x, g, 1e-6) == (0, None)
    one = (ref.view(torch.int16) + 1).view(torch.bfloat16)  # one step away from zero everywhere
    ndiff, rep = exact.rmsnorm_mismatch(one, x, g, 1e-6)
    assert rep is None and ndiff == ref.numel()
    two = ref.clone()
    two[2, d - 1] = (ref[2, d - 1:].view(torch.int16) + 2).view(torch.bfloat16)
    ndiff, rep = exact.rmsnorm_mismatch(two, x, g, 1e-6)
    assert ndiff == 1 and rep is not None and f"row 2, column {d - 1}" in rep
    # a sum of squares that misses the last vector is past one step somewhere
    xd = x.double()
    inv_bad = torch.rsqrt(xd[:, : d - 8].pow(2).sum(-1, keepdim=True) / d + 1e-6)
    bad = ((xd * inv_bad).bfloat16().double() * g.double()).bfloat16()
    if d <= 2048:  # 8 of 2048 elements: 0.2 % of inv, half a bf16 step
        assert exact.rmsnorm_mismatch(bad, x, g, 1e-6)[1] is not None
