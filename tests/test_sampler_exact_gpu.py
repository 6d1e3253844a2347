"""The device samplers (csrc/sample.hip: one workgroup per row, two-stage split, chunk-maximum, lean chunk-maximum)
against the exact host reference of tests/sampler_ref.py -- not against each other: the kernels share their draw and
their decode-state update, so a mistake there leaves them in agreement.

The reference predicts the token itself (penalty in float32, temperature / top-p / renormalisation / pick in float64,
the kernels' own hash of seed and token index).  Where a comparison lies within sampler_ref.DELTA of its bound the
reference admits every outcome; on all other rows (the share is capped before anything is launched) the kernel's
token must be the reference's.  The decode state after the launch must equal sampler_ref.advance_reference, array for
array, including history-ring wrap, context end, budget end, finished and idle rows, and rows of padded logits.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import sampler_ref as sr  # noqa: E402
from cain_amd import ops  # noqa: E402

DEV = torch.device("cuda")
# the chunk-maximum kernel only while the library still exports it
KERNELS = ["one", "split", "lean"] + (["cm"] if hasattr(ops.load(), "cain_sample_cm") else [])
IN_PLACE = ("one", "cm")  # these apply the penalty to the logits themselves; the others leave them alone


def _launch(kernel, logits, rows, state, T_max):
    """One sampler launch on ``logits`` (a device tensor, possibly a view of padded rows; modified by the in-place
    kernels) from the numpy decode state ``state``; returns the state afterwards as numpy arrays."""
    M, V = logits.shape
    st = {k: torch.from_numpy(np.ascontiguousarray(state[k])).to(DEV) for k in sr.STATE_KEYS}
    hist = torch.zeros((M + 4) * sr.HIST, device=DEV, dtype=torch.int32)  # spare rows behind the ring
    hist[:M * sr.HIST] = st["hist"].view(-1)
    cmax = logits.reshape(M, V // 16, 16).amax(-1).contiguous() if kernel in ("cm", "lean") else None
    ops.sample(logits, st["tok"], st["pos"], st["gen"], st["n_gen"], st["max_new"], st["done"], hist, st["slot"],
               ops.sample_params_tensor(rows, DEV), T_max, split=(kernel == "split"), cmax=cmax,
               lean=(kernel == "lean"))
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
    """Untouched by split / lean; one / cm change the penalised ids only, to the reference's float32 value (2 ulp)."""
    same = _bits(after) == _bits(before)
    for m, r in enumerate(refs):
        pen = r.penalised if kernel in IN_PLACE else []
        mask = np.ones(after.shape[1], dtype=bool)
        mask[pen] = False
        assert same[m][mask].all(), (what, m, np.flatnonzero(~same[m] & mask)[:8].tolist())
        for t in pen:
            a, b = float(after[m, t]), float(r.values[t])
            assert a == b or abs(a - b) <= 2.4e-7 * abs(b), (what, m, t, a, b)


@functools.lru_cache(maxsize=None)
def _exact(V):
    """The cases of vocabulary V with their references (computed once, shared by the kernels, never modified)."""
    out = []
    for launch in range(sr.EXACT_LAUNCHES):
        case = sr.exact_case(V, launch)
        out.append((case, sr.case_refs(case)))
    return out


@functools.lru_cache(maxsize=None)
def _undecided_by_kind():
    pooled = {}
    for V in (64, 4096, 32064):
        for case, refs in _exact(V):
            for k, (a, b) in sr.undecided_counts(refs, case.kinds)[1].items():
                c = pooled.setdefault(k, [0, 0])
                c[0] += a
                c[1] += b
    return pooled


def _wrong_tokens(toks, refs):
    """Rows whose token is not the reference's (decided rows) or not admissible: (row, token, reference, admissible)."""
    wrong = []
    for m, r in enumerate(refs):
        t = int(toks[m])
        if (r.decided and t != r.token) or t not in r.admissible:
            wrong.append((m, t, r.token, sorted(r.admissible)))
    return wrong


EXACT = [(k, V) for V in (64, 4096) for k in KERNELS] + [("one", 32064), ("lean", 32064)]


@pytest.mark.parametrize("kernel,V", EXACT)
def test_exact_token(kernel, V):
    cases = _exact(V)
    und = sum(sr.undecided_counts(refs, case.kinds)[0] for case, refs in cases)
    rows = sum(len(refs) for _, refs in cases)
    print(f"V {V}: {und} of {rows} rows undecided")
    assert und <= 0.04 * rows, (und, rows)
    for k, (a, b) in _undecided_by_kind().items():
        assert a <= 0.08 * b, (sr.KINDS[k], a, b)
    for launch, (case, refs) in enumerate(cases):
        what = (kernel, V, launch)
        lg = torch.from_numpy(case.logits).to(DEV)
        out = _launch(kernel, lg, case.rows, case.state, case.T_max)
        ng = case.state["n_gen"]
        toks = out["gen"][np.arange(len(refs)), ng]  # (tok as well: the state check below compares every array)
        assert ((toks >= 0) & (toks < V)).all(), (what, toks)
        wrong = _wrong_tokens(toks, refs)
        # (reported with the rows' n_gen: a wrong ring read shows on the wrapped rows, 65 and up)
        assert not wrong, (what, len(wrong), "n_gen", sorted({int(ng[w[0]]) for w in wrong}), wrong[:6])
        _check_state(out, case.state, toks, case.rows, case.T_max, what)
        _check_logits(kernel, lg.cpu().numpy(), case.logits, refs, what)


@pytest.mark.parametrize("kernel", KERNELS)
def test_top_p_cut_at_the_exact_boundary(kernel):
    """Four equal candidates and top_p 0.5: every device value is a power of two (exp(0) = 1, 1 / 4, the sums), so
    nothing rounds, the cumulative probability reaches top_p exactly at the second candidate and `>=` keeps two:
    the token is the first candidate for u < 0.5 and the second otherwise, never the third.  (The other logits are
    distinct: thousands of exact ties at the top-k threshold are a case of their own, which the one-workgroup and the
    chunk-maximum kernel resolve by arrival order -- test_sample_lean_gpu.py test_lean_sampler_ties_everywhere.)"""
    V, M = 4096, 64
    rng = np.random.default_rng(3)
    logits = (-50.0 - rng.permutation(M * V).reshape(M, V) / float(M * V)).astype(np.float32)
    ids = np.sort(np.stack([rng.choice(V, 4, replace=False) for _ in range(M)]), axis=1)
    np.put_along_axis(logits, ids, np.float32(1.0), axis=1)
    rows = [dict(temperature=1.0, top_k=4, top_p=0.5, repeat_penalty=1.0, repeat_last_n=64, eos_id=-1,
                 seed=int(rng.integers(0, 1 << 62))) for _ in range(M)]
    state = sr.new_state(M, V, rng, n_gen=np.arange(M) % 7)
    refs = [sr.reference_detail(logits[m], state["hist"][m], int(state["n_gen"][m]), rows[m], delta=0.0)
            for m in range(M)]
    want = [int(ids[m, 0 if sr.u_of(rows[m]["seed"], int(state["n_gen"][m])) < 0.5 else 1]) for m in range(M)]
    assert [r.token for r in refs] == want and all(r.cut == 2 for r in refs)
    assert len({w == ids[m, 0] for m, w in enumerate(want)}) == 2  # both candidates occur
    out = _launch(kernel, torch.from_numpy(logits).to(DEV), rows, state, sr.T_MAX)
    assert out["tok"].tolist() == want
    _check_state(out, state, want, rows, sr.T_MAX, kernel)


@pytest.mark.parametrize("kernel", KERNELS)
def test_extremes(kernel):
    """Temperatures 0.01 and 100, top_p 1e-6 / 0 (off) / 1 (off), one row of logits scaled by 30.  The fp32 error
    bound behind DELTA does not hold here (exponent arguments in the thousands), so: the token is a top-K candidate
    after the penalty, the first candidate where nothing else has any weight, and never a garbage id."""
    V, M = 4096, 64
    rng = np.random.default_rng(11)
    logits = (rng.standard_normal((M, V)) * 3.0).astype(np.float32)
    logits[:, :3] += np.float32(4.0)
    logits[8] *= np.float32(30.0)  # (a row of temperature 0.01: exponent arguments down to about -1e5)
    extremes = [(t, p) for t in (0.01, 100.0) for p in (1e-6, 0.0, 1.0)]
    rows = []
    for i in range(M):
        t, p = extremes[i % 6]
        rows.append(dict(temperature=t, top_p=p, top_k=[40, 256, 10, 0][i % 4], repeat_penalty=[1.1, 1.0, 0.8][(i // 6) % 3],
                         repeat_last_n=64, eos_id=-1, seed=int(rng.integers(0, 1 << 62))))
    state = sr.new_state(M, V, rng, n_gen=30)
    state["hist"][:, 3:9] = np.argsort(-logits, axis=1, kind="stable")[:, :6]
    refs = [sr.reference_detail(logits[m], state["hist"][m], 30, rows[m]) for m in range(M)]
    out = _launch(kernel, torch.from_numpy(logits).to(DEV), rows, state, sr.T_MAX)
    toks = out["tok"]
    assert ((toks >= 0) & (toks < V)).all(), toks
    n_first = 0
    for m, r in enumerate(refs):
        t = int(toks[m])
        assert t in r.support, (m, rows[m], t)
        gap = float(r.values[r.ids[0]]) - float(r.values[r.ids[1]])
        if rows[m]["top_p"] == 1e-6 or (rows[m]["temperature"] == 0.01 and gap >= 1.0):
            assert t in r.firsts, (m, rows[m], t, r.ids[:3])
            n_first += 1
    assert n_first > M // 3
    _check_state(out, state, toks, rows, sr.T_MAX, kernel)


@pytest.mark.parametrize("kernel", KERNELS)
def test_decode_state_edges(kernel):
    V, M, T_max = 4096, 8, 2048
    rng = np.random.default_rng(5)
    logits = rng.standard_normal((M, V)).astype(np.float32)
    win = [101, 202, 303, 404, 505, 0, 707, 808]
    for m, w in enumerate(win):
        logits[m, w] = 50.0
    greedy = dict(temperature=0.0, top_p=1.0, repeat_penalty=1.0, top_k=40, repeat_last_n=0, eos_id=-1, seed=1)
    rows = [dict(greedy) for _ in range(M)]
    state = sr.new_state(M, V, rng, n_gen=3, pos=50)
    state["pos"][0] = T_max - 1             # context end: done, pos kept
    state["pos"][1] = T_max - 2             # one before it: goes on
    state["n_gen"][2] = sr.MAX_NEW - 1      # budget end
    rows[3]["eos_id"] = win[3]              # eos
    rows[4]["stop"] = [5, 6, win[4]]        # the last stop id
    rows[5].update(eos_id=-1, stop=[-1])    # unused ids (-1) never stop, also when the winner is id 0
    state["done"][6] = 1                    # finished at entry: untouched
    state["slot"][7] = -1                   # idle: untouched
    out = _launch(kernel, torch.from_numpy(logits).to(DEV), rows, state, T_max)
    assert out["done"].tolist() == [1, 0, 1, 1, 1, 0, 1, 0]
    assert out["pos"].tolist() == [T_max - 1, T_max - 1, 50, 50, 50, 51, 50, 50]
    assert out["n_gen"].tolist() == [4, 4, sr.MAX_NEW, 4, 4, 4, 3, 3]
    assert out["tok"][:6].tolist() == win[:6]
    _check_state(out, state, win, rows, T_max, kernel)  # every array; rows 6 and 7 keep tok, gen and hist too


PADDED = [(k, 4096) for k in KERNELS] + [("one", 260), ("split", 260)]  # cm / lean need V % 64 == 0


@pytest.mark.parametrize("kernel,V", PADDED)
def test_padded_rows(kernel, V):
    """Logits as a [:, :V] view of [M][V + 64] rows whose padding holds +1e30: the samplers take the row stride, draw
    the tokens of the contiguous run, never choose a padding column and never write one."""
    case = _exact(V)[0][0] if V == 4096 else sr.exact_case(V, 0)
    refs = _exact(V)[0][1] if V == 4096 else sr.case_refs(case)
    M = len(case.rows)
    flat = _launch(kernel, torch.from_numpy(case.logits).to(DEV), case.rows, case.state, case.T_max)
    buf = torch.full((M, V + 64), 1e30, device=DEV)
    buf[:, :V] = torch.from_numpy(case.logits).to(DEV)
    view = buf[:, :V]
    assert view.stride(0) == V + 64
    out = _launch(kernel, view, case.rows, case.state, case.T_max)
    assert ((out["tok"] >= 0) & (out["tok"] < V)).all(), out["tok"]
    for k in sr.STATE_KEYS:
        assert np.array_equal(out[k], flat[k]), (k, np.argwhere(out[k] != flat[k])[:8].tolist())
    after = buf.cpu().numpy()
    assert (_bits(after[:, V:]) == _bits(np.float32(1e30))).all()
    wrong = _wrong_tokens(out["tok"], refs)
    assert not wrong, (kernel, V, "padded", len(wrong), wrong[:6])
    _check_logits(kernel, after[:, :V], case.logits, refs, (kernel, V, "padded"))
