"""Token log-probabilities on the GPU: the kernels of csrc/logprob.hip through their ``ops`` wrappers, then the engine.

Kernel reference: float64 log-softmax of the same fp32 logits on the host, top-n by (logit descending, index
ascending).  Logprob tolerance, absolute: ``2e-5 * max(1, |ref| / 32)`` -- one fp32 rounding of ``x - max`` at
magnitude <= 32 (1.9e-6), the rounding of the exp argument (3e-6 relative on every term, so on the sum), 2-ulp exp /
log and a tree sum of <= 20 levels (1.5e-6): about 8e-6, doubled.  Top-n ids must equal the host order exactly.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from cain_amd import ops  # noqa: E402

DEV = torch.device("cuda")
TOP = ops.LOGPROB_TOP_MAX
PAD = 1e30  # behind each row of a padded buffer: a read past V shows up in the sum and in the top-n
POISON_F, POISON_I = -12345.5, -77


def tol(ref):
    return 2e-5 * np.maximum(1.0, np.abs(ref) / 32.0)


def host_ref(lg: np.ndarray):
    """(lse [M] float64, top ids [M, min(20, V)], their logprobs) of fp32 logits [M, V]."""
    x = lg.astype(np.float64)
    mx = x.max(1, keepdims=True)
    lse = (mx + np.log(np.exp(x - mx).sum(1, keepdims=True)))[:, 0]
    M, V = lg.shape
    k = min(TOP, V)
    ids = np.empty((M, k), dtype=np.int64)
    for m in range(M):
        kth = np.partition(lg[m], V - k)[V - k]
        cand = np.flatnonzero(lg[m] >= kth)
        ids[m] = cand[np.lexsort((cand, -x[m, cand]))][:k]
    return lse, ids, np.take_along_axis(x, ids, 1) - lse[:, None]


def device_rows(lg: np.ndarray, pad: int):
    """The logits on the device as a [M, V] view of [M, V + pad] rows whose pad holds PAD."""
    M, V = lg.shape
    buf = torch.full((M, V + pad), PAD, device=DEV, dtype=torch.float32)
    buf[:, :V] = torch.from_numpy(lg).to(DEV)
    return buf


def outputs(M):
    return dict(lse=torch.full((M,), POISON_F, device=DEV), lp=torch.full((M,), POISON_F, device=DEV),
                top_id=torch.full((M, TOP), POISON_I, device=DEV, dtype=torch.int32),
                top_lp=torch.full((M, TOP), POISON_F, device=DEV))


def run_rows(buf, V, n, target, slot=None, done=None):
    """One launch with per-row ``n`` (an int for all rows or a list); returns the outputs as numpy arrays."""
    M = buf.shape[0]
    topn = torch.tensor([n] * M if isinstance(n, int) else n, device=DEV, dtype=torch.int32)
    o = outputs(M)
    rc = ops.logprob_rows(buf, V, topn, slot=slot, done=done,
                          target=torch.from_numpy(target.astype(np.int32)).to(DEV), **o)
    torch.cuda.synchronize()
    assert rc == 0
    return {k: v.cpu().numpy() for k, v in o.items()}


def check(out, lg, ref, n, target, what, worst=None):
    lse, ids, lps = ref
    M = lg.shape[0]
    k = min(n, ids.shape[1])
    err = np.abs(out["lse"] - lse)
    assert (err <= tol(lse)).all(), (what, "lse", float(err.max()))
    want = lg[np.arange(M), target].astype(np.float64) - lse
    e2 = np.abs(out["lp"] - want)
    assert (e2 <= tol(want)).all(), (what, "target", float(e2.max()))
    assert (out["top_id"][:, :k] == ids[:, :k]).all(), (what, "ids", out["top_id"][0, :k], ids[0, :k])
    e3 = np.abs(out["top_lp"][:, :k] - lps[:, :k])
    assert (e3 <= tol(lps[:, :k])).all(), (what, "top", float(e3.max()) if k else 0.0)
    assert (out["top_id"][:, k:] == POISON_I).all() and (out["top_lp"][:, k:] == np.float32(POISON_F)).all(), what
    if worst is not None:
        worst.append(max(float(err.max()), float(e2.max()), float(e3.max()) if k else 0.0))


@functools.lru_cache(maxsize=None)
def random_case(M, V):
    """Random logits in [-16, 16] with their reference and targets (computed once per shape, never modified)."""
    rng = np.random.default_rng(1000 * M + V)
    lg = rng.uniform(-16, 16, size=(M, V)).astype(np.float32)
    return lg, host_ref(lg), rng.integers(0, V, size=M)


@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("V", [1024, 32064, 256000])
@pytest.mark.parametrize("M", [1, 3, 64])
def test_rows_random(M, V, pad):
    lg, ref, target = random_case(M, V)
    buf = device_rows(lg, pad)
    worst = []
    for n in (0, 1, 5, 20):
        check(run_rows(buf[:, :V], V, n, target), lg, ref, n, target, (M, V, pad, n), worst)
    print(f"logprob kernel M={M} V={V} pad={pad}: worst |error| {max(worst):.3e} "
          f"(bound {float(tol(np.float64(ref[0].max()))):.1e})")


def test_rows_mixed_topn():
    """Rows of one launch ask for different n."""
    lg, ref, target = random_case(3, 32064)
    out = run_rows(device_rows(lg, 64)[:, :32064], 32064, [20, 0, 5], target)
    for m, n in enumerate((20, 0, 5)):
        assert (out["top_id"][m, :n] == ref[1][m, :n]).all()
        assert (out["top_id"][m, n:] == POISON_I).all()


@pytest.mark.parametrize("V,levels,run", [(1024, 7, 1), (32064, 40, 1), (32064, 3, 1), (32064, 40, 2000)])
def test_ties(V, levels, run):
    """Rows of a few distinct values: ties straddle every n-th place (the order among equals is the index).  With
    ``run`` elements sharing the maximum there are more ties above the threshold than the gather pass holds, which
    takes the selection passes."""
    rng = np.random.default_rng(V + levels)
    lg = rng.integers(0, levels, size=(3, V)).astype(np.float32) * 0.5 - 3.0
    if run > 1:
        for m in range(3):
            lg[m, rng.choice(V, size=run, replace=False)] = 9.0
    ref = host_ref(lg)
    target = rng.integers(0, V, size=3)
    buf = device_rows(lg, 64)
    for n in (1, 5, 20):
        check(run_rows(buf[:, :V], V, n, target), lg, ref, n, target, (V, levels, run, n))


def test_uniform_row():
    V = 1024
    lg = np.full((2, V), 3.25, dtype=np.float32)
    target = np.array([0, V - 1])
    out = run_rows(device_rows(lg, 64)[:, :V], V, 20, target)
    want = -10 * np.log(2.0)
    assert np.abs(out["lp"] - want).max() < 1e-6
    assert np.abs(out["top_lp"] - want).max() < 1e-6
    assert (out["top_id"] == np.arange(20)).all()
    assert np.abs(out["lse"] - (3.25 + 10 * np.log(2.0))).max() < 1e-5


def test_one_hot_row():
    V = 32064
    lg = np.full((2, V), -80.0, dtype=np.float32)
    hot = [7, V - 1]
    for m, h in enumerate(hot):
        lg[m, h] = 80.0
    out = run_rows(device_rows(lg, 64)[:, :V], V, 5, np.array(hot))
    assert np.abs(out["lp"]).max() < 1e-6
    assert (out["top_id"][:, 0] == hot).all() and np.abs(out["top_lp"][:, 0]).max() < 1e-6
    rest = out["top_lp"][:, 1:5]
    assert np.isfinite(rest).all() and np.abs(rest + 160.0).max() < 1e-3
    assert (out["top_id"][0, 1:5] == [0, 1, 2, 3]).all() and (out["top_id"][1, 1:5] == [0, 1, 2, 3]).all()


def test_skipped_rows_untouched():
    """slot -1, done 1 and topn -1 leave their rows of every output as they were, bit for bit."""
    lg, ref, target = random_case(3, 1024)
    lg4 = np.concatenate([lg, lg[:1]])
    t4 = np.concatenate([target, target[:1]])
    slot = torch.tensor([-1, 0, 1, 2], device=DEV, dtype=torch.int32)
    done = torch.tensor([0, 1, 0, 0], device=DEV, dtype=torch.int32)
    out = run_rows(device_rows(lg4, 0), 1024, [5, 5, -1, 5], t4, slot=slot, done=done)
    for k, poison in (("lse", POISON_F), ("lp", POISON_F), ("top_lp", POISON_F), ("top_id", POISON_I)):
        assert (out[k][:3] == np.asarray(poison, dtype=out[k].dtype)).all(), k
    assert (out["top_id"][3, :5] == ref[1][0, :5]).all() and abs(out["lse"][3] - ref[0][0]) <= tol(ref[0][0])


def test_refusals():
    """V % 4, ldl < V and n > 20 return an error and launch nothing."""
    lg, _, target = random_case(3, 1024)
    buf = device_rows(lg, 64)
    tgt = torch.from_numpy(target.astype(np.int32)).to(DEV)
    n5 = torch.full((3,), 5, device=DEV, dtype=torch.int32)
    o = outputs(3)
    assert ops.logprob_rows(buf[:, :1022], 1022, n5, target=tgt, **o) != 0
    assert ops.logprob_rows(buf[:, :1024], 2048, n5, target=tgt, **o) != 0          # ldl = 1088 < V
    assert ops.logprob_rows(buf[:, :1024], 1024, n5, target=tgt, nmax=21, **o) != 0
    n21 = torch.full((3,), 21, device=DEV, dtype=torch.int32)
    assert ops.logprob_rows(buf[:, :1024], 1024, n21, target=tgt, **o) != 0
    keep = ops.logprob_keep(3, DEV)
    gen = torch.zeros(3, 32, device=DEV, dtype=torch.int32)
    ring_id = torch.full((3, 32, TOP), POISON_I, device=DEV, dtype=torch.int32)
    ring_lp = torch.full((3, 32, TOP), POISON_F, device=DEV)
    zeros = torch.zeros(3, device=DEV, dtype=torch.int32)
    hist = torch.zeros(3 * 64, device=DEV, dtype=torch.int32)
    assert ops.logprob_pre(buf[:, :1022], 1022, n5, zeros, hist, gen, ring_id, ring_lp, keep) != 0
    assert ops.logprob_pre(buf[:, :1024], 1024, n5, zeros, hist, gen, ring_id, ring_lp, keep, nmax=21) != 0
    torch.cuda.synchronize()
    for k, poison in (("lse", POISON_F), ("lp", POISON_F), ("top_lp", POISON_F), ("top_id", POISON_I)):
        assert (o[k] == poison).all(), k
    assert (ring_id == POISON_I).all() and (ring_lp == POISON_F).all() and not keep.any()


# ------------------------------------------------------------------------------------------- the penalty hazard
@pytest.mark.parametrize("split", [False, True])
def test_chosen_logprob_uses_raw_logit(split):
    """sample_kernel applies the repeat penalty in place on the logits; the chosen token's logprob must still be the
    log-softmax of the model's logits.  Row 0: the argmax (+20, margin 40) is in the history, repeat_penalty 1.5,
    greedy.  Row 1: the same logits, the argmax not in the history (read from the buffer).  Row 2: finished before
    the step (nothing written).  Negative control: the value a kernel would produce by reading the buffer after the
    sampler (the penalised logit minus the row's log-sum-exp) is off by more than 100 tolerances -- where the
    sampler under test does write the buffer (the one-workgroup kernel; the two-stage kernel leaves it alone)."""
    V, T, M = 1024, 96, 3
    rng = np.random.default_rng(5)
    row = rng.uniform(-30, -20, size=V).astype(np.float32)
    a = 321
    row[a] = 20.0
    lg = np.stack([row] * M)
    lse, _, _ = host_ref(lg)
    want = np.float64(row[a]) - lse[0]
    ng = np.array([70, 70, 5], dtype=np.int32)  # past one turn of the 64-entry history ring
    hist = rng.integers(0, V, size=(M, 64)).astype(np.int32)
    hist[hist == a] = a + 1
    hist[0, (ng[0] - 3) & 63] = a
    buf = device_rows(lg, 64)
    logits = buf[:, :V]
    st = dict(tok=torch.zeros(M, dtype=torch.int32), pos=torch.full((M,), 80, dtype=torch.int32),
              n_gen=torch.from_numpy(ng.copy()), max_new=torch.full((M,), 90, dtype=torch.int32),
              done=torch.tensor([0, 0, 1], dtype=torch.int32), slot=torch.arange(M, dtype=torch.int32))
    st = {k: v.to(DEV) for k, v in st.items()}
    hist_d = torch.from_numpy(hist).to(DEV).view(-1).contiguous()
    gen = torch.full((M, T), -1, device=DEV, dtype=torch.int32)
    lp = torch.full((M, T), POISON_F, device=DEV)
    ring_id = torch.full((M, T, TOP), POISON_I, device=DEV, dtype=torch.int32)
    ring_lp = torch.full((M, T, TOP), POISON_F, device=DEV)
    keep = ops.logprob_keep(M, DEV)
    topn = torch.full((M,), 3, device=DEV, dtype=torch.int32)
    params = ops.sample_params_tensor(
        [dict(temperature=0.0, top_p=1.0, repeat_penalty=1.5, top_k=1, repeat_last_n=64, eos_id=-1, seed=0)] * M, DEV)
    assert ops.logprob_pre(logits, V, topn, st["n_gen"], hist_d, gen, ring_id, ring_lp, keep, slot=st["slot"],
                           done=st["done"], nmax=3) == 0
    ops.sample(logits, st["tok"], st["pos"], gen, st["n_gen"], st["max_new"], st["done"], hist_d, st["slot"], params,
               T, split=split)
    assert ops.logprob_chosen(logits, V, gen, keep, lp) == 0
    torch.cuda.synchronize()
    gen_h, lp_h, after = gen.cpu().numpy(), lp.cpu().numpy(), logits.cpu().numpy()
    assert gen_h[0, 70] == a and gen_h[1, 70] == a and (gen_h[2] == -1).all()
    for m in (0, 1):
        assert abs(lp_h[m, 70] - want) <= tol(want), (m, lp_h[m, 70], want)
        assert ring_id[m, 70, 0].item() == a and abs(ring_lp[m, 70, 0].item() - want) <= tol(want)
        assert (np.delete(lp_h[m], 70) == np.float32(POISON_F)).all()
    assert (lp_h[2] == np.float32(POISON_F)).all() and (ring_id[2] == POISON_I).all()
    assert after[1, a] == np.float32(20.0)  # not a history id of row 1: never penalised
    if not split:
        assert after[0, a] == np.float32(20.0) / np.float32(1.5)
        from_buffer = np.float64(after[0, a]) - lse[0]
        assert abs(from_buffer - want) > 100 * tol(want), (from_buffer, want)
    else:
        assert after[0, a] == np.float32(20.0)


# =========================================================================================================== engine
from cain_amd.engine import DecodeEngine, logprob_host  # noqa: E402
from cain_amd.models.reference import ReferenceModel  # noqa: E402
from cain_amd.models.weights import roundtrip_weights  # noqa: E402

ENGINES = [("tiny-llama3.1:8b", "bf16"), ("tiny-gemma:2b", "bf16"), ("tiny-mistral:7b", "q4_k_m")]
# max |logprob(engine) - logprob(fp32 oracle on the same dequantised weights)| allowed on the prompts of
# test_score_multi_chunk_vs_oracle, and between decode and score in test_decode_logprobs_match_score: twice what
# score measured against the oracle on those prompts (profiles/r12/logprobs/README.md; the kernels are deterministic,
# the margin only covers a later change of prompt or seed).
ORACLE_BOUND = {
    ("tiny-llama3.1:8b", "bf16"): 2 * 3.7483e-3,    # measured 3.7483e-03 (decode vs score: 5.6e-04)
    ("tiny-gemma:2b", "bf16"): 2 * 2.7644e-3,       # measured 2.7644e-03 (decode vs score: 3.5e-04)
    ("tiny-mistral:7b", "q4_k_m"): 2 * 4.9059e-3,   # measured 4.9059e-03 (decode vs score: 2.7e-03)
}


def _engine(name, wd, **kw):
    return DecodeEngine(name, device="cuda", max_batch=4, max_context=256, seed=3, steps_per_graph=4,
                        weight_dtype=wd, keep_natural=True, **kw)


def _prompt(n, seed):
    return np.random.default_rng(seed).integers(3, 1000, size=n).tolist()


def _oracle_logprobs(eng, wd, p):
    """float64 log-softmax rows [n - 1, V] of the fp32 oracle on the weights the kernels multiply by."""
    ref = ReferenceModel(roundtrip_weights(eng.weights, wd))
    lg = ref.forward(torch.tensor([p], device="cuda"))[0].float().cpu()
    return np.stack([logprob_host(lg[j], 0)[0] for j in range(len(p) - 1)])


@pytest.mark.parametrize("name,wd", ENGINES)
def test_tokens_unchanged_and_graph_equals_eager(name, wd):
    """Seeded sampling with the repeat penalty: the tokens with logprobs on are bitwise those with logprobs off, and
    graph replay and eager single steps give bitwise the same logprobs."""
    eng = _engine(name, wd)
    prompts = [_prompt(5 + 3 * i, 40 + i) for i in range(4)]
    opts = [dict(temperature=0.8, repeat_penalty=1.1, seed=100 + i, eos_id=-1) for i in range(4)]
    off = eng.generate(prompts, 40, opts)
    on = eng.generate(prompts, 40, opts, logprobs=True, top_logprobs=5)
    eager = eng.generate(prompts, 40, opts, use_graph=False, logprobs=True, top_logprobs=5)
    assert (4, 4) in eng._graphs and (4, 4, "lp") in eng._graphs
    eng.close()
    assert [r.tokens for r in on] == [r.tokens for r in off] == [r.tokens for r in eager]
    assert all(r.logprobs is None and r.top_logprobs is None for r in off)
    for a, b in zip(on, eager):
        assert len(a.logprobs) == 40 and all(len(t) == 5 for t in a.top_logprobs)
        assert np.array_equal(np.float32(a.logprobs).view(np.int32), np.float32(b.logprobs).view(np.int32))
        assert a.top_logprobs == b.top_logprobs
        assert all(lp <= 0 for lp in a.logprobs)
        for t in a.top_logprobs:
            assert [v for _, v in t] == sorted((v for _, v in t), reverse=True)


@pytest.mark.parametrize("name,wd", ENGINES)
def test_score_single_chunk_vs_own_logits(name, wd):
    """A 24-token prompt is one chunk: its logprobs against float64 log-softmax of the logits buffer the call left
    behind, at the kernel tolerance -- row j - 1 scores token j."""
    eng = _engine(name, wd)
    p = _prompt(24, 7)
    res = eng.score([p], top_logprobs=3)[0]
    lg = eng.buf["logits"][:23].cpu()
    eng.close()
    assert res.tokens == p and len(res.logprobs) == 23
    for j in range(1, 24):
        ls, top = logprob_host(lg[j - 1], 3)
        assert abs(res.logprobs[j - 1] - ls[p[j]]) <= tol(ls[p[j]]), j
        assert [i for i, _ in res.top_logprobs[j - 1]] == [i for i, _ in top], j
        assert all(abs(a - b) <= tol(b) for (_, a), (_, b) in zip(res.top_logprobs[j - 1], top))


@pytest.mark.parametrize("name,wd", ENGINES)
def test_score_multi_chunk_vs_oracle(name, wd):
    """A 200-token and a 70-token prompt in one call (268 rows: over a 128-row chunk boundary, three of the 64-row
    format's) against the fp32 oracle; targets shifted by one are off by more than 10 bounds."""
    eng = _engine(name, wd)
    ps = [_prompt(200, 11), _prompt(70, 12)]
    res = eng.score(ps)
    bound = ORACLE_BOUND[(name, wd)]
    worst, worst_shift = 0.0, 0.0
    for p, r in zip(ps, res):
        ls = _oracle_logprobs(eng, wd, p)
        got = np.array(r.logprobs)
        assert got.shape == (len(p) - 1,)
        worst = max(worst, float(np.abs(got - ls[np.arange(len(p) - 1), p[1:]]).max()))
        worst_shift = max(worst_shift, float(np.abs(got[:-1] - ls[np.arange(len(p) - 2), p[2:]]).max()))
    eng.close()
    print(f"score vs oracle {name} {wd}: max |dlogprob| {worst:.4e} (bound {bound:.3e}); shifted targets {worst_shift:.3f}")
    assert worst <= bound
    assert worst_shift > 10 * bound


@pytest.mark.parametrize("name,wd", ENGINES)
def test_decode_logprobs_match_score(name, wd):
    """Greedy generation with logprobs, then score(prompt + generated): the generated tokens' logprobs agree within
    the measured bound, and each step's first alternative is the generated token."""
    eng = _engine(name, wd)
    p = _prompt(9, 21)
    r = eng.generate([p], 32, [dict(temperature=0.0, eos_id=-1)], logprobs=True, top_logprobs=2)[0]
    s = eng.score([p + r.tokens])[0]
    eng.close()
    assert len(r.tokens) == 32 and len(r.logprobs) == 32
    d = float(np.abs(np.array(r.logprobs) - np.array(s.logprobs[len(p) - 1:])).max())
    print(f"decode vs score {name} {wd}: max |dlogprob| {d:.4e}")
    assert d <= ORACLE_BOUND[(name, wd)]
    assert [t[0][0] for t in r.top_logprobs] == r.tokens
    assert all(t[0][1] == lp for t, lp in zip(r.top_logprobs, r.logprobs))


def test_continuous_batch_mixes_requests():
    """A request with top_logprobs = 3 joins one without: the first gets 3 alternatives per token, the second none,
    and the second's tokens are those of a run on its own."""
    eng = _engine("tiny-llama3.1:8b", "bf16")
    opts = dict(temperature=0.8, repeat_penalty=1.1, seed=9, eos_id=-1)
    alone = eng.generate(["plain request"], 20, [opts])[0].tokens
    with_lp = eng.generate(["wants logprobs"], 12, [opts], logprobs=True, top_logprobs=3)[0]
    cb = eng.continuous()
    assert cb.admit(["plain request"], [20], [opts]) == [0]
    cb.step()
    assert cb.admit(["wants logprobs"], [12], [opts], logprobs=True, top_logprobs=3) == [1]
    for _ in range(8):
        cb.step()
        _, fin = cb.poll()
        if all(fin):
            break
    assert all(fin)
    assert cb.tokens(0) == alone and cb.tokens(1) == with_lp.tokens
    assert cb.logprobs(0) is None
    lps, tops = cb.logprobs(1)
    eng.close()
    assert len(lps) == 12 and all(len(t) == 3 for t in tops)
    assert np.array_equal(np.float32(lps).view(np.int32), np.float32(with_lp.logprobs).view(np.int32))
    assert tops == with_lp.top_logprobs
