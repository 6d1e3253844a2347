"""The embedding pooling kernels alone (csrc/pool.hip: ``cain_pool_rows``, ``cain_pool_finish``) against float64 numpy.

Exact cases take the norm's effect out: rows of +-2^k entries with one sum of squares per row (every row of a call must
get the identical ``rinv``), small-integer rows with power-of-two gains (the ``mean`` sums are then exact up to the one
common factor ``rinv``, removed by dividing by ``acc[0][0]``), ``last`` against ``mean`` on a one-row sequence, and a
sequence fed in two calls cut at every row against the single call, all bit for bit.  The general case holds random
rows to a bound counted from the kernel's own arithmetic (``C_TERM`` / ``finish_path`` below).  Rows that no run names
keep a poison pattern bit for bit, and the sizes the entry cannot take are refused with nothing launched."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from cain_amd import ops  # noqa: E402

DEV = torch.device("cuda")
EPS = 1e-6
U = 2.0 ** -24          # unit roundoff of fp32
POISON_F = -7.25e11     # a finite fp32 pattern no result comes near
POISON_I = -123456789
POISON_BITS = int(np.float32(POISON_F).view(np.int32))
DIMS = (8, 2056, 4096, 16384)  # 2056: not a multiple of 8 x 256, the last workgroup column is part empty
ROWS = (1, 2, 128)
MEAN, LAST = ops.POOL_MEAN, ops.POOL_LAST

# Roundings of one term of pool_acc_kernel, relative to the term, first order:
#   rinv = rsq(ss * rcp(d) + eps).  ss: each thread adds up to 4 x 8 squares (a product and an add each: 64 roundings),
#   then 6 wave-shuffle adds and up to 8 adds over the waves' partials: 78 roundings on the longest path, all terms
#   positive, so ss is off by at most 78 u relatively.  rcp and rsq are the hardware's 1-ulp instructions (2 u each),
#   the product with rcp(d) and the add of eps one rounding each.  Through the square root the error of the argument
#   halves: (78 + 2 + 1 + 1) / 2 + 2 = 43 u on rinv.
#   term = fl(fl(x * rinv) * gain): 2 more roundings, x and gain exact inputs: 45 u.
# Each accumulation adds one rounding of the running sum, at most u * sum|term| each, `rows` of them.  In all
#   |acc - exact| <= (45 + rows) u sum|term| <= rows * C_TERM * u * sum|term|   with C_TERM = 46,
# u taken as u / (1 - 46 u) to cover the higher-order terms.
C_TERM = 46


@pytest.fixture(autouse=True)
def _sync():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:  # a GPU fault: nothing more may run on the device
        pytest.exit(f"GPU error, stopping the session: {exc}", returncode=3)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def layout(M: int):
    """(run lengths, their rows of acc, rows of acc in all) for a call of M rows: one run of one row; two runs around
    an empty one; runs of 1, 5 and M - 6 rows and an empty one, their rows of acc permuted.  Two further rows of acc
    belong to no run."""
    if M == 1:
        return [1], [1], 3
    if M == 2:
        return [1, 0, 1], [2, 1, 0], 5
    return [1, 5, 0, M - 6], [3, 0, 4, 1], 6


def run_pool(x, gain, lens, dst, B, mode, eps=EPS, acc=None, cnt=None, pad=8):
    """One cain_pool_rows call over the rows of ``x`` (float tensor [M, d], rounded to bf16 here), handed over as a
    view of pitch d + pad; returns (acc, cnt, rinv) on the device.  ``acc`` / ``cnt``: continue these."""
    M, d = x.shape
    buf = torch.full((M, d + pad), 3.0, dtype=torch.bfloat16, device=DEV)
    xv = buf[:, :d]
    xv.copy_(x.to(torch.bfloat16))
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=DEV)
    sd = torch.tensor(dst, dtype=torch.int32, device=DEV)
    if acc is None:
        acc = torch.full((B, d), POISON_F, dtype=torch.float32, device=DEV)
        cnt = torch.full((B,), POISON_I, dtype=torch.int32, device=DEV)
        for s, q in zip(lens, dst):  # the rows a run names start at zero, as the engine's do
            if s:
                acc[q] = 0
                cnt[q] = 0
    rinv = torch.full((M,), POISON_F, dtype=torch.float32, device=DEV)
    rc = ops.pool_rows(xv, gain, eps, off, sd, mode, acc, cnt, rinv, d=d)
    assert rc == 0
    assert bool((buf[:, d:] == 3.0).all())
    return acc, cnt, rinv


def reference(x, gain, lens, dst, B, mode, eps=EPS):
    """float64: (acc [B, d], sum|term| [B, d], rows added [B]) of the bf16 rows."""
    xb = x.to(torch.bfloat16).double().cpu().numpy()
    g = gain.double().cpu().numpy()
    inv = 1.0 / np.sqrt((xb * xb).sum(1, keepdims=True) / xb.shape[1] + eps)
    term = xb * inv * g
    acc, mag, n = np.zeros((B, xb.shape[1])), np.zeros((B, xb.shape[1])), np.zeros(B, dtype=np.int64)
    r = 0
    for s, q in zip(lens, dst):
        if s:
            sl = slice(r + s - 1, r + s) if mode == LAST else slice(r, r + s)
            acc[q], mag[q], n[q] = term[sl].sum(0), np.abs(term[sl]).sum(0), sl.stop - sl.start
        r += s
    return acc, mag, n


def random_rows(M, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, d, generator=g) * torch.exp(torch.randn(M, 1, generator=g))
    gain = (1.0 + 0.25 * torch.randn(d, generator=g)).float().to(DEV)
    return x, gain


@pytest.mark.parametrize("mode", [MEAN, LAST], ids=["mean", "last"])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("d", DIMS)
def test_random_rows_within_the_counted_bound(d, M, mode):
    x, gain = random_rows(M, d, 1000 * d + M)
    lens, dst, B = layout(M)
    acc, cnt, _ = run_pool(x, gain, lens, dst, B, mode)
    want, mag, n = reference(x, gain, lens, dst, B, mode)
    got = acc.cpu().double().numpy()
    named = sorted(q for s, q in zip(lens, dst) if s)
    u = U / (1 - C_TERM * U)
    for q in named:
        bound = n[q] * C_TERM * u * mag[q]
        err = np.abs(got[q] - want[q])
        print(f"d={d} M={M} mode={mode} row {q}: worst err / bound = {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (q, float((err / bound).max()))
        assert int(cnt[q]) == (1 if mode == LAST else n[q])
    # rows of acc / cnt that no run names (an empty run's included) keep the poison, bit for bit
    others = [q for q in range(B) if q not in named]
    assert bool((bits(acc[others]) == POISON_BITS).all())
    assert bool((cnt[others] == POISON_I).all())


@pytest.mark.parametrize("M", (2, 128))
@pytest.mark.parametrize("d", DIMS)
def test_two_calls_cut_anywhere_equal_one_call_bitwise(d, M):
    x, gain = random_rows(M, d, 77 * d + M)
    one, cnt1, _ = run_pool(x, gain, [M], [1], 2, MEAN)
    for cut in range(1, M):
        acc, cnt, _ = run_pool(x[:cut], gain, [cut], [1], 2, MEAN)
        acc, cnt, _ = run_pool(x[cut:], gain, [M - cut], [1], 2, MEAN, acc=acc, cnt=cnt)
        assert torch.equal(bits(acc), bits(one)), f"cut at row {cut}"
        assert torch.equal(cnt, cnt1)
    again, _, _ = run_pool(x, gain, [M], [1], 2, MEAN)
    assert torch.equal(bits(again), bits(one))  # the same inputs give the same bits


@pytest.mark.parametrize("d", DIMS)
def test_last_equals_mean_on_one_row_bitwise(d):
    x, gain = random_rows(1, d, 5 * d)
    a, ca, _ = run_pool(x, gain, [1], [0], 1, MEAN)
    b, cb, _ = run_pool(x, gain, [1], [0], 1, LAST)
    assert torch.equal(bits(a), bits(b)) and int(ca[0]) == int(cb[0]) == 1


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("d", DIMS)
def test_power_of_two_rows_get_one_rinv(d, M):
    """Entries +-2^k, k in -2 .. 2, the same multiset in every row (each row its own order and signs): the squares are
    multiples of 1 / 16 whose sums stay below 2^18, exact in fp32 in any order, so every row's sum of squares -- and
    with it rinv -- is the same number whatever the reduction tree."""
    rng = np.random.default_rng(d + M)
    base = 2.0 ** rng.integers(-2, 3, size=d)
    x = np.stack([rng.permutation(base) * rng.choice([-1.0, 1.0], size=d) for _ in range(M)])
    gain = torch.ones(d, device=DEV)
    _, _, rinv = run_pool(torch.tensor(x, dtype=torch.float32), gain, [M], [0], 1, MEAN)
    assert bool((bits(rinv) == bits(rinv[0])).all())
    want = 1.0 / math.sqrt(float((base * base).sum()) / d + EPS)
    assert abs(float(rinv[0]) - want) <= 6 * U * want  # rcp, product, add, rsq: 2 + 1 + 1 + 2 u


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("d", (8, 4096, 16384))
def test_small_integer_rows_sum_exactly_up_to_rinv(d, M):
    """Rows of the integers (3, 3, 3, 1, 1, 1, 1, 1) in every 8 columns, each row in its own order and signs: a sum of
    squares of 4 d, with eps = 0 and d a power of two a mean square of exactly 4, so one rinv for every row (a power of
    two where the hardware's rsq is exact there; whatever it is, it is the one common factor).  With power-of-two
    gains every term is rinv x a small dyadic number and so is every partial sum: acc = rinv x the exact sum, and
    acc / acc[0][0] equals the reference's ratio bit for bit."""
    rng = np.random.default_rng(3 * d + M)
    base = np.tile([3.0, 3.0, 3.0, 1.0, 1.0, 1.0, 1.0, 1.0], d // 8)
    x = np.stack([rng.permutation(base) * rng.choice([-1.0, 1.0], size=d) for _ in range(M)])
    x[:, 0] = np.abs(x[:, 0])  # acc[0][0] is a sum of positive terms
    g = 2.0 ** rng.integers(-3, 4, size=d)
    lens, dst, B = ([M], [0], 1) if M < 7 else ([7, M - 7], [0, 1], 2)
    acc, _, rinv = run_pool(torch.tensor(x, dtype=torch.float32), torch.tensor(g, dtype=torch.float32, device=DEV),
                            lens, dst, B, MEAN, eps=0.0)
    assert bool((bits(rinv) == bits(rinv[0])).all())
    want = np.zeros((B, d), dtype=np.float32)
    r = 0
    for s, q in zip(lens, dst):
        want[q] = (x[r:r + s] * g).sum(0)  # exact: small dyadic numbers
        r += s
    got = acc.cpu().numpy()
    assert np.array_equal((got / got[0, 0]).view(np.int32), (want / want[0, 0]).view(np.int32))


def finish_path(d: int) -> int:
    """Roundings on the longest path of pool_finish_kernel's sum of squares: thread 0's FMAs (one per element it
    owns), then the wave-shuffle levels and the adds over the waves' partials that join two non-zero numbers (an add of
    a zero partial is exact)."""
    per_thread = -(-d // 256)
    lanes = min(d, 64)
    waves = min(-(-d // 64), 4)
    return per_thread + math.ceil(math.log2(lanes)) + (waves - 1)


@pytest.mark.parametrize("d", DIMS)
def test_finish(d):
    assert finish_path(d) <= d  # never more roundings than a serial sum of d terms
    g = torch.Generator().manual_seed(d)
    B = 6
    acc = (torch.randn(B, d, generator=g) * 3).to(DEV)
    acc[4] = 0  # a zero vector stays zero
    cnt = torch.tensor([1, 7, 0, 128, 3, 0], dtype=torch.int32, device=DEV)
    a64, n64 = acc.cpu().double().numpy(), cnt.cpu().numpy()
    for normalize in (True, False):
        out = torch.full((B, d), POISON_F, dtype=torch.float32, device=DEV)
        assert ops.pool_finish(acc, cnt, out, normalize) == 0
        got = out.cpu().numpy()
        for b in range(B):
            if n64[b] == 0:  # untouched, bit for bit
                assert (got[b].view(np.int32) == np.float32(POISON_F).view(np.int32)).all()
                continue
            v32 = acc[b].cpu().numpy() / np.float32(n64[b])
            if not normalize or b == 4:
                assert np.array_equal(got[b].view(np.int32), v32.view(np.int32))
                continue
            v = a64[b] / n64[b]
            want = v / np.sqrt((v * v).sum())
            # v = fl(acc / n): u.  ss: v^2 carries 2 u, the sum finish_path(d) roundings; the root halves that and
            # rounds once; the quotient rounds once: u + (2 + P) / 2 u + u + u = (4 + P / 2) u per element.
            c = 4 + finish_path(d) / 2
            err = np.abs(got[b].astype(np.float64) - want)
            bound = c * U / (1 - c * U) * np.abs(want)
            print(f"d={d} row {b}: worst err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
            assert (err <= bound).all()
            assert np.isfinite(got[b]).all()


@pytest.mark.parametrize("what", ["d = 12", "d = 16392", "null gain"])
def test_refused_with_nothing_launched(what):
    d = {"d = 12": 12, "d = 16392": 16392}.get(what, 64)
    x = torch.ones(2, d, dtype=torch.bfloat16, device=DEV)
    gain = None if what == "null gain" else torch.ones(d, device=DEV)
    acc = torch.full((1, d), POISON_F, dtype=torch.float32, device=DEV)
    cnt = torch.full((1,), POISON_I, dtype=torch.int32, device=DEV)
    rinv = torch.full((2,), POISON_F, dtype=torch.float32, device=DEV)
    off = torch.tensor([0, 2], dtype=torch.int32, device=DEV)
    dst = torch.zeros(1, dtype=torch.int32, device=DEV)
    for mode in (MEAN, LAST):
        assert ops.pool_rows(x, gain, EPS, off, dst, mode, acc, cnt, rinv) == -1
    torch.cuda.synchronize()
    assert bool((bits(acc) == POISON_BITS).all()) and int(cnt[0]) == POISON_I
    assert bool((bits(rinv) == POISON_BITS).all())
