"""The device samplers under ``min_p``, ``presence_penalty`` and ``frequency_penalty`` (csrc/sample.hip SampleExt)
against the exact host reference of tests/sampler_ref_ext.py, in the manner of tests/test_sampler_exact_gpu.py: the
token itself on every row the reference decides, an admissible token on the others, the whole decode state, and the
logits (changed by the in-place kernels at the penalised ids only, to the reference's float32 value).

Vocabularies 64 and 4096 for every kernel, 32064 for the one-workgroup and the lean kernel: the smallest that reach
the register-slice, chunk-maximum and tail paths.  Four launches of 64 rows each.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import sampler_ref as sr  # noqa: E402
import sampler_ref_ext as sx  # noqa: E402
from cain_amd import ops  # noqa: E402

DEV = torch.device("cuda")
KERNELS = ["one", "split", "lean"] + (["cm"] if hasattr(ops.load(), "cain_sample_cm") else [])
IN_PLACE = ("one", "cm")
NO_EXT = object()  # _launch: no record at all (ext=None), as opposed to one packed from the rows


def _launch(kernel, logits, rows, state, T_max, ext_rows=None):
    """One sampler launch (tests/test_sampler_exact_gpu.py _launch) with the rows' SampleExt records: packed from
    ``ext_rows`` (default: ``rows``), or none at all for ``NO_EXT``."""
    M, V = logits.shape
    st = {k: torch.from_numpy(np.ascontiguousarray(state[k])).to(DEV) for k in sr.STATE_KEYS}
    hist = torch.zeros((M + 4) * sr.HIST, device=DEV, dtype=torch.int32)
    hist[:M * sr.HIST] = st["hist"].view(-1)
    cmax = logits.reshape(M, V // 16, 16).amax(-1).contiguous() if kernel in ("cm", "lean") else None
    ext = None if ext_rows is NO_EXT else ops.sample_ext_tensor(rows if ext_rows is None else ext_rows, DEV)
    ops.sample(logits, st["tok"], st["pos"], st["gen"], st["n_gen"], st["max_new"], st["done"], hist, st["slot"],
               ops.sample_params_tensor(rows, DEV), T_max, split=(kernel == "split"), cmax=cmax,
               lean=(kernel == "lean"), ext=ext)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in st.items()}
    out["hist"] = hist[:M * sr.HIST].view(M, sr.HIST).cpu().numpy()
    assert not hist[M * sr.HIST:].any()
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _check_state(out, state, toks, rows, T_max, what):
    want = sr.advance_reference(state, toks, rows, T_max)
    for k in sr.STATE_KEYS:
        bad = np.argwhere(out[k] != want[k])
        assert bad.size == 0, (what, k, bad[:8].tolist())


def _check_logits(kernel, after, before, refs, what):
    """Untouched by split / lean; one / cm change the penalised ids only, to the reference's float32 value within
    2.4e-7 relative (two float32 ulp: the division)."""
    same = _bits(after) == _bits(before)
    for m, r in enumerate(refs):
        pen = r.penalised if kernel in IN_PLACE else []
        mask = np.ones(after.shape[1], dtype=bool)
        mask[pen] = False
        assert same[m][mask].all(), (what, m, np.flatnonzero(~same[m] & mask)[:8].tolist())
        for t in pen:
            a, b = float(after[m, t]), float(r.values[t])
            assert a == b or abs(a - b) <= 2.4e-7 * abs(b), (what, m, t, a, b)


def _wrong_tokens(toks, refs):
    wrong = []
    for m, r in enumerate(refs):
        t = int(toks[m])
        if (r.decided and t != r.token) or t not in r.admissible:
            wrong.append((m, t, r.token, sorted(r.admissible)))
    return wrong


@functools.lru_cache(maxsize=None)
def _exact(V):
    """The ext cases of vocabulary V with their references (computed once, shared by the kernels, never modified)."""
    out = []
    for launch in range(sr.EXACT_LAUNCHES):
        case = sx.exact_case_ext(V, launch)
        out.append((case, sx.case_refs_ext(case)))
    return out


EXACT = [(k, V) for V in (64, 4096) for k in KERNELS] + [("one", 32064), ("lean", 32064)]


@pytest.mark.parametrize("kernel,V", EXACT)
def test_exact_token_ext(kernel, V):
    cases = _exact(V)
    und = sum(sr.undecided_counts(refs, case.kinds)[0] for case, refs in cases)
    rows = sum(len(refs) for _, refs in cases)
    print(f"V {V}: {und} of {rows} rows undecided")
    assert und <= 0.04 * rows, (und, rows)  # (per kind and per EXT entry: tests/test_sampler_ext_ref.py)
    for launch, (case, refs) in enumerate(cases):
        what = (kernel, V, launch)
        lg = torch.from_numpy(case.logits).to(DEV)
        out = _launch(kernel, lg, case.rows, case.state, case.T_max)
        ng = case.state["n_gen"]
        toks = out["gen"][np.arange(len(refs)), ng]
        assert ((toks >= 0) & (toks < V)).all(), (what, toks)
        wrong = _wrong_tokens(toks, refs)
        assert not wrong, (what, len(wrong), "n_gen", sorted({int(ng[w[0]]) for w in wrong}),
                           "ext", sorted({case.exts[w[0]] for w in wrong}), wrong[:6])
        _check_state(out, case.state, toks, case.rows, case.T_max, what)
        _check_logits(kernel, lg.cpu().numpy(), case.logits, refs, what)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_record_equals_a_zero_record(kernel):
    """``ext=None`` and an all-zero record: bitwise the same decode state and logits, and the plain reference's
    tokens (the rows keep exact_case's options: repeat penalties, top-p)."""
    case = sr.exact_case(4096, 0)
    refs = sr.case_refs(case)
    got = []
    for ext_rows in (NO_EXT, [{}] * len(case.rows)):
        lg = torch.from_numpy(case.logits).to(DEV)
        out = _launch(kernel, lg, case.rows, case.state, case.T_max, ext_rows=ext_rows)
        got.append((out, lg.cpu().numpy()))
    (a, la), (b, lb) = got
    for k in sr.STATE_KEYS:
        assert np.array_equal(a[k], b[k]), (kernel, k)
    assert np.array_equal(_bits(la), _bits(lb))
    assert not _wrong_tokens(a["tok"], refs)


@pytest.mark.parametrize("kernel", KERNELS)
def test_min_p_one_draws_the_greedy_token(kernel):
    """min_p 1.0 at a sampling temperature keeps the candidates whose ratio to the first is >= 1: on a row whose
    maximum after the penalty is no exact tie (and lies further than the reference's margin from the next value:
    sampler_ref_ext's admission rule, which decides all but a handful of rows) the token is the row's greedy token."""
    case = sx.exact_case_ext(4096, 1)
    rows = [dict(o, min_p=1.0) for o in case.rows]
    hist, ngs = case.state["hist"], case.state["n_gen"]
    refs = [sx.reference_detail_ext(case.logits[m], hist[m], int(ngs[m]), rows[m]) for m in range(len(rows))]
    greedy = [sx.reference_detail_ext(case.logits[m], hist[m], int(ngs[m]), dict(rows[m], temperature=0.0))
              for m in range(len(rows))]
    out = _launch(kernel, torch.from_numpy(case.logits).to(DEV), rows, case.state, case.T_max)
    checked = 0
    for m, (r, g) in enumerate(zip(refs, greedy)):
        t = int(out["tok"][m])
        assert t in r.admissible, (kernel, m, t, sorted(r.admissible))
        tie = len(r.ids) > 1 and r.values[r.ids[0]] == r.values[r.ids[1]]
        if r.decided and not tie and len(g.firsts) == 1:
            assert t == g.token, (kernel, m, rows[m], t, g.token)
            checked += 1
    assert checked >= 0.9 * len(rows), checked
    _check_state(out, case.state, out["tok"], rows, case.T_max, kernel)


@pytest.mark.parametrize("kernel", KERNELS)
def test_ring_wrap_and_counts(kernel):
    """Greedy, frequency penalty 0.5, no other penalty.  Id A (logit 10) fills 10 slots of the window on the even
    rows and 3 on the odd ones, id B holds 7, everything else is below 0: A falls by exactly 5.0 to 5.0 and B wins,
    or by 1.5 and A stays.  n_gen 63 (slot 63 holds A too, but was never written: outside the window), 64, 65 and 200
    (the ring wrapped)."""
    V, A, B = 4096, 1234, 77
    ngs = [63, 63, 64, 64, 65, 65, 200, 200]
    M = len(ngs)
    rng = np.random.default_rng(9)
    logits = (-1.0 - rng.random((M, V))).astype(np.float32)
    logits[:, A], logits[:, B] = 10.0, 7.0
    rows = [dict(temperature=0.0, top_k=40, top_p=1.0, repeat_penalty=1.0, repeat_last_n=64, eos_id=-1, seed=1,
                 frequency_penalty=0.5) for _ in range(M)]
    state = sr.new_state(M, V, rng, n_gen=ngs)
    state["hist"][state["hist"] == A] = A + 1
    state["hist"][state["hist"] == B] = B + 1
    fills = []
    for m, ng in enumerate(ngs):
        n = 10 if m % 2 == 0 else 3
        fills.append(n)
        for j in range(n):
            state["hist"][m, (ng - 1 - 6 * j) & (sr.HIST - 1)] = A  # ages 0, 6, ..., 54: inside every window here
        if ng == 63:
            state["hist"][m, 63] = A
    refs = [sx.reference_detail_ext(logits[m], state["hist"][m], ngs[m], rows[m]) for m in range(M)]
    want = [B if n == 10 else A for n in fills]
    assert [r.token for r in refs] == want and all(r.decided for r in refs)
    lg = torch.from_numpy(logits).to(DEV)
    out = _launch(kernel, lg, rows, state, sr.T_MAX)
    assert out["tok"].tolist() == want, (kernel, out["tok"].tolist())
    _check_state(out, state, want, rows, sr.T_MAX, kernel)
    after = lg.cpu().numpy()
    if kernel == "one":
        assert after[:, A].tolist() == [10.0 - 0.5 * n for n in fills]  # exact: 10 - fmaf(n, 0.5, 0)
    _check_logits(kernel, after, logits, refs, kernel)
