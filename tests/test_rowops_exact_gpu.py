"""The row ops that run on every forward -- quant_rows (wgemm8.hip), embed and rmsnorm (norm.hip) -- against the
references of ``tests/exact.py``: quant_rows byte for byte on rows whose scale is a power of two, per element to half
an e4m3 step on random rows, its folded RMSNorm factor to 2^-21; embed bit for bit; rmsnorm to one bf16 step.  Inputs
and outputs are views into wider buffers whose padding must keep its sentinel; sizes the kernels cannot take are
refused with an error.  ``tests/test_rowops_exact_cpu.py`` checks the references and comparators on the host."""
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

sys.path.insert(0, str(Path(__file__).parent))

import exact  # noqa: E402
from cain_amd import ops  # noqa: E402

DEV = torch.device("cuda")
EPS = 1e-6
SENT8, SENT16 = 0xA5, -7.0


@pytest.fixture(autouse=True)
def _sync():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:  # a GPU fault: nothing more may run on the device
        pytest.exit(f"GPU error, stopping the session: {exc}", returncode=3)


def wide_view(x: torch.Tensor, pad: int, fill: float):
    """x [M, n] on the device as a view at column pad / 2 of a [M, n + pad] buffer filled with ``fill``."""
    M, n = x.shape
    buf = torch.full((M, n + pad), fill, dtype=x.dtype, device=DEV)
    view = buf[:, pad // 2: pad // 2 + n]
    view.copy_(x)
    return buf, view


def pad_intact(buf: torch.Tensor, n: int, pad: int, fill) -> bool:
    return bool((buf[:, : pad // 2] == fill).all()) and bool((buf[:, pad // 2 + n:] == fill).all())


def quant(x: torch.Tensor, norm: bool = False):
    """ops.quant_rows with ldx = K + 64 and an output pitch of K + 128 bytes between sentinel bytes."""
    M, K = x.shape
    _, xv = wide_view(x, 64, SENT16)
    out = torch.full((M, K + 128), SENT8, dtype=torch.uint8, device=DEV)
    o8 = out[:, 64: 64 + K]
    assert xv.stride(0) == K + 64 and o8.stride(0) == K + 128
    x8, xs = ops.quant_rows(xv, norm, EPS, x8=o8)
    assert x8.data_ptr() == o8.data_ptr()
    assert pad_intact(out, K, 128, SENT8), "quant_rows wrote outside its K bytes of a row"
    return x8.cpu(), xs.cpu()


QR_SHAPES = [(M, K) for K in exact.QR_KS for M in exact.QR_MS]
qr_ids = lambda v: f"M{v[0]}-K{v[1]}"  # noqa: E731


@pytest.mark.parametrize("shape", QR_SHAPES, ids=qr_ids)
def test_quant_rows_bytes_and_scales_are_exact(shape):
    """Rows of y 2^e with amax = 448 2^e in the last vector: e4m3 ties both ways, the subnormal step 2^-9, +-0,
    saturation at +-448, an all-zero row (``exact.quant_exact_rows``).  Bytes and scales equal the reference's."""
    M, K = shape
    x, _ = exact.quant_exact_rows(M, K, K + M)
    x8, xs = quant(x)
    rep = exact.quant_exact_mismatch(x, x8, xs)
    assert rep is None, f"M {M}, K {K}: {rep}"


@pytest.mark.parametrize("shape", QR_SHAPES, ids=qr_ids)
def test_quant_rows_every_element_within_half_a_step(shape):
    """Random rows (3 x randn): per element within half an e4m3 step of x, at most one code from the reference's
    byte, the scale the reference's (``exact.quant_general_mismatch``).  Prints the number of differing bytes."""
    M, K = shape
    x = exact.quant_general_rows(M, K, K + M)
    x8, xs = quant(x)
    ndiff, rep = exact.quant_general_mismatch(x, x8, xs)
    print(f"quant_rows M {M} K {K}: {ndiff} of {M * K} bytes differ from the reference")
    assert rep is None, f"M {M}, K {K}: {rep}"


@pytest.mark.parametrize("shape", QR_SHAPES, ids=qr_ids)
def test_quant_rows_norm_factor(shape):
    """xs with the RMSNorm folded in, on sparse integer rows whose sum of squares is exact in fp32 in any order
    (``exact.quant_norm_rows``: non-zeros at the row's ends, on both sides of chunk boundaries, in every wave's
    range), to a relative 2^-21; losing one non-zero moves xs by 0.2 % or more.  The bytes stay exact."""
    M, K = shape
    x = exact.quant_norm_rows(M, K, K + M)
    x8, xs = quant(x, norm=True)
    rep = exact.quant_norm_mismatch(x, xs, EPS)
    assert rep is None, f"M {M}, K {K}: {rep}"
    ndiff, rep = exact.quant_general_mismatch(x, x8, exact.quant_rows_ref(x)[1].float())
    assert (ndiff, rep) == (0, None), f"M {M}, K {K}: {ndiff} bytes differ: {rep}"


@pytest.mark.parametrize("K", exact.QR_REFUSED)
def test_quant_rows_refuses(K):
    """K past the 12 register chunks (24,584) or no whole vectors (12): an error, nothing launched or written."""
    pitch = (K + 15) // 8 * 8  # both pitches whole vectors: K alone is what is refused
    x = torch.ones(2, pitch, dtype=torch.bfloat16, device=DEV)[:, :K]
    out = torch.full((2, pitch), SENT8, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match=r"quant_rows failed \(rc="):
        ops.quant_rows(x, x8=out[:, :K])
    assert bool((out == SENT8).all())


# ---------------------------------------------------------------- embed
@pytest.mark.parametrize("M", exact.EMBED_MS)
@pytest.mark.parametrize("d", exact.EMBED_DS)
def test_embed_is_bit_exact(d, M):
    """out = bf16(fp32(E[tok]) x scale) bit for bit, for scale 1 and Gemma's bf16(sqrt(d)); tokens with row 0, the
    last row and repeats; ``out`` a view with ldo = d + 64 whose padding keeps its sentinel."""
    E, tok = exact.embed_case(M, d, d + M)
    Ed, tokd = E.to(DEV), tok.to(DEV)
    for scale in exact.embed_scales(d):
        buf = torch.full((M, d + 64), SENT16, dtype=torch.bfloat16, device=DEV)
        out = buf[:, 32: 32 + d]
        assert out.stride(0) == d + 64
        ops.embed(tokd, Ed, scale, out=out)
        rep = exact.mismatches(exact.bits16(out.cpu()), exact.bits16(exact.embed_ref(E, tok, scale)))
        assert rep is None, f"embed d {d}, M {M}, scale {scale} (16-bit patterns; row = token index): {rep}"
        assert pad_intact(buf, d, 64, SENT16), "embed wrote outside its d columns of a row"


# ---------------------------------------------------------------- rmsnorm
@pytest.mark.parametrize("d", exact.NORM_DS)
def test_rmsnorm_within_one_bf16_step(d):
    """Integer rows (the sum of squares is exact) against bf16(bf16(x inv) g) in fp64: every output within one
    bf16 step; d = 8200 and 16384 run the 512-thread kernel; ldx and ldy wider than d, padding intact.  Prints the
    number of elements that differ at all."""
    M = 3
    x, g = exact.rmsnorm_case(M, d, d)
    xbuf, xv = wide_view(x, 64, SENT16)
    ybuf = torch.full((M, d + 128), SENT16, dtype=torch.bfloat16, device=DEV)
    y = ybuf[:, 64: 64 + d]
    assert xv.stride(0) == d + 64 and y.stride(0) == d + 128
    ops.rmsnorm(xv, g.to(DEV), EPS, out=y)
    ndiff, rep = exact.rmsnorm_mismatch(y.cpu(), x, g, EPS)
    print(f"rmsnorm d {d}: {ndiff} of {M * d} elements differ from the reference")
    assert rep is None, f"rmsnorm d {d}: {rep}"
    assert pad_intact(ybuf, d, 128, SENT16) and pad_intact(xbuf, d, 64, SENT16)
    assert torch.equal(xv.cpu(), x)  # the input is only read


@pytest.mark.parametrize("d", exact.NORM_REFUSED)
def test_rmsnorm_refuses(d):
    """d past 4 vectors x 512 threads (16,392) or no whole vectors (12): an error, nothing launched or written."""
    x = torch.ones(2, d, dtype=torch.bfloat16, device=DEV)
    y = torch.full((2, d), SENT16, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match=r"rmsnorm failed \(rc="):
        ops.rmsnorm(x, torch.ones(d, dtype=torch.bfloat16, device=DEV), EPS, out=y)
    assert bool((y == SENT16).all())
