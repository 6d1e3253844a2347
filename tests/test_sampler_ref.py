"""The host reference of the samplers (tests/sampler_ref.py) itself: the RNG against SplitMix64's published first
output and for uniformity, the pipeline on rows small enough to compute by hand, the share of test rows on which the
reference cannot decide the token, and engine.sample_host against it.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import sampler_ref as sr
from cain_amd.engine.engine import SAMPLE_TOPK_MAX, sample_host, sample_host_candidates


def _opts(**kw):
    o = dict(temperature=1.0, top_k=40, top_p=1.0, repeat_penalty=1.0, repeat_last_n=64, eos_id=-1, seed=1)
    o.update(kw)
    return o


NO_HIST = [0] * 64


def test_mix64_is_splitmix64():
    assert sr.mix64(0) == 0xE220A8397B1DCDAF  # first output of SplitMix64 seeded with 0
    assert 0.0 <= sr.u_of(0, 0) < 1.0
    assert sr.u_of(5, 7) == sr.u_of(5 + (1 << 64), 7)  # 64-bit seeds
    assert sr.u_of(1 << 61, 3) != sr.u_of(0, 3)  # the high seed bits count


def test_rng_uniform_and_uncorrelated():
    u = np.array([[sr.u_of(s, n) for n in range(257)] for s in range(257)])
    grid = u[:256, :256]
    counts = np.bincount((grid.ravel() * 64).astype(int), minlength=64)
    expect = grid.size / 64
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print("chi-square over 64 bins:", chi2)
    assert chi2 < 103.4  # the 99.9 % quantile of chi-square with 63 degrees of freedom
    c_tok = float(np.corrcoef(grid.ravel(), u[:256, 1:257].ravel())[0, 1])
    c_seed = float(np.corrcoef(grid.ravel(), u[1:257, :256].ravel())[0, 1])
    print("corr over token index, over seed:", c_tok, c_seed)
    assert abs(c_tok) < 0.02 and abs(c_seed) < 0.02  # 5 sigma for 65,536 pairs


# ---- rows computed by hand

def _four_equal(V=16):
    lg = np.full(V, -50.0, dtype=np.float32)
    lg[[2, 5, 9, 11]] = 1.0  # four candidates of probability 1/4 each (exact in binary)
    return lg


def test_top_p_cut_keeps_the_crossing_element():
    lg = _four_equal()
    for top_p, cut in ((0.5, 2), (0.75, 3), (0.25, 1), (0.26, 2), (0.74, 3), (0.76, 4)):
        r = sr.reference_detail(lg, NO_HIST, 0, _opts(top_k=4, top_p=top_p), delta=0.0)
        assert r.ids == [2, 5, 9, 11] and r.probs == [0.25] * 4
        assert r.cut == cut, (top_p, r.cut)


def test_tiny_top_p_keeps_one():
    lg = _four_equal()
    for seed in range(20):
        r = sr.reference_detail(lg, NO_HIST, 3, _opts(top_k=4, top_p=1e-6, seed=seed))
        assert r.cut == 1 and r.token == 2 and r.admissible == {2}


def test_pick_renormalises_over_the_cut():
    lg = _four_equal()
    seen = set()
    for seed in range(200):
        u = sr.u_of(seed, 4)
        r = sr.reference_detail(lg, NO_HIST, 4, _opts(top_k=4, top_p=0.75, seed=seed), delta=0.0)
        want = [2, 5, 9][min(int(u * 3), 2)]  # thirds of the unit interval after the cut of 3
        assert abs(u * 3 - round(u * 3)) > 1e-9
        assert r.token == want and r.admissible == {want}
        seen.add(want)
    assert seen == {2, 5, 9}


def test_admissible_set_opens_near_a_boundary():
    """A draw within delta of a CDF boundary, or a cut within delta of top_p, admits both neighbours."""
    lg = _four_equal()
    seed = next(s for s in range(100000) if 0.5 - 5e-5 < sr.u_of(s, 0) < 0.5)
    r = sr.reference_detail(lg, NO_HIST, 0, _opts(top_k=4, seed=seed))
    assert r.token == 5 and r.admissible == {5, 9} and not r.decided
    assert sr.reference_detail(lg, NO_HIST, 0, _opts(top_k=4, seed=seed), delta=0.0).admissible == {5}
    seed = next(s for s in range(1000) if 0.8 < sr.u_of(s, 0) < 0.9)
    r = sr.reference_detail(lg, NO_HIST, 0, _opts(top_k=4, top_p=0.50001, seed=seed))
    assert r.cut == 3 and r.token == 9 and r.admissible == {5, 9}  # a cut of 2 is within delta


def test_penalty_rules():
    lg = np.array([0.0, -2.0, 3.0, 4.0, 1.0, 0.5], dtype=np.float32)
    ring = [0] * 64
    ring[0:5] = [1, 3, 3, 0, 3]  # ids 1, 3 (three times), 0
    ring[5:8] = [-1, 9, 6]       # outside [0, V): ignored
    v, pen = sr.penalise(lg, ring, 8, _opts(repeat_penalty=2.0))
    assert sorted(pen) == [0, 1, 3]
    assert v.tolist() == [0.0, -4.0, 3.0, 2.0, 1.0, 0.5]  # 0 stays, a negative multiplies, a duplicate id once
    # a penalty below 1 raises: the order changes accordingly
    r = sr.reference_detail(lg, ring, 8, _opts(repeat_penalty=0.5, temperature=0.0))
    assert r.token == 3 and r.values.tolist() == [0.0, -1.0, 3.0, 8.0, 1.0, 0.5]
    # off: penalty 1, a window of 0, nothing generated yet
    for o, ng in ((_opts(repeat_penalty=1.0), 8), (_opts(repeat_penalty=2.0, repeat_last_n=0), 8),
                  (_opts(repeat_penalty=2.0), 0)):
        v, pen = sr.penalise(lg, ring, ng, o)
        assert pen == [] and v.tolist() == lg.tolist()
    # the window: the last 2 of 8 are slots 7 and 6 (ids 6 and 9: outside), so nothing changes
    assert sr.penalise(lg, ring, 8, _opts(repeat_penalty=2.0, repeat_last_n=2))[1] == []
    assert sr.penalise(lg, ring, 5, _opts(repeat_penalty=2.0, repeat_last_n=2))[1] == [3, 0]
    # the float32 penalty decides ties: 3 / 1.5 == 2 exactly, the lower index wins
    lg2 = np.array([1.0, 3.0, 2.0], dtype=np.float32)
    r = sr.reference_detail(lg2, [1] * 64, 1, _opts(repeat_penalty=1.5, temperature=0.0))
    assert r.token == 1 and r.values.tolist() == [1.0, 2.0, 2.0]


def test_ring_across_a_wrap():
    ring = list(range(100, 164))  # slot s holds id 100 + s
    got = sr.recent_ids(ring, 70, 20)  # the 70 ids written so far: 64..69 sit in slots 0..5
    assert got == [105, 104, 103, 102, 101, 100] + list(range(163, 149, -1))
    assert sr.recent_ids(ring, 70, 200) == [100 + ((69 - j) & 63) for j in range(64)]
    assert sr.recent_ids(ring, 64, 3) == [163, 162, 161] and sr.recent_ids(ring, 65, 3) == [100, 163, 162]
    lg = np.zeros(200, dtype=np.float32) + 1.0
    v, pen = sr.penalise(lg, ring, 70, _opts(repeat_penalty=2.0, repeat_last_n=20))
    assert sorted(pen) == list(range(100, 106)) + list(range(150, 164))
    assert set(np.flatnonzero(v == 0.5).tolist()) == set(pen) and np.count_nonzero(v == 1.0) == 200 - 20


def test_top_k_clamp_and_order():
    lg = np.arange(600, dtype=np.float32)
    lg[10] = lg[599]  # a tie for the top: the lower index first
    for top_k, n in ((0, 256), (-5, 256), (257, 256), (256, 256), (255, 255), (1, 1), (1000, 256)):
        r = sr.reference_detail(lg, NO_HIST, 0, _opts(top_k=top_k))
        assert len(r.ids) == n and r.ids[:3] == [10, 599, 598][:n]
    assert len(sr.reference_detail(lg[:50], NO_HIST, 0, _opts(top_k=0)).ids) == 50
    assert sr.TOPK_MAX == SAMPLE_TOPK_MAX == 256


def test_near_tie_after_a_penalty_admits_both_orders():
    x = np.float32(3.3)
    lg = np.array([np.float32(x / np.float32(1.1)), x, -9.0], dtype=np.float32)  # id 1 is penalised onto id 0's value
    r = sr.reference_detail(lg, [1] * 64, 1, _opts(repeat_penalty=1.1, temperature=0.0))
    assert r.token == 0 and r.admissible == {0, 1}
    # two ids penalised from the same value round the same way: the index decides
    lg = np.array([x, x, -9.0], dtype=np.float32)
    r = sr.reference_detail(lg, [0, 1] * 32, 2, _opts(repeat_penalty=1.1, temperature=0.0))
    assert r.admissible == {0}


def test_advance_reference():
    rng = np.random.default_rng(0)
    st = sr.new_state(6, 100, rng, n_gen=[3, 64, 249, 3, 3, 3], pos=[10, 10, 10, 2047, 10, 10])
    st["done"][4] = 1
    st["slot"][5] = -1
    rows = [_opts(eos_id=7), _opts(stop=[1, 2, 9]), _opts(), _opts(), _opts(), _opts()]
    out = sr.advance_reference(st, [5, 9, 8, 8, 8, 8], rows, 2048)
    assert out["done"].tolist() == [0, 1, 1, 1, 1, 0] and out["pos"].tolist() == [11, 10, 10, 2047, 10, 10]
    assert out["n_gen"].tolist() == [4, 65, 250, 4, 3, 3] and out["tok"][:4].tolist() == [5, 9, 8, 8]
    assert out["gen"][0, 3] == 5 and out["hist"][0, 3] == 5 and out["gen"][1, 64] == 9 and out["hist"][1, 0] == 9
    for k in sr.STATE_KEYS:
        assert np.array_equal(out[k][4:], st[k][4:]), k  # done / idle rows keep everything
    changed = {k: int((out[k] != st[k]).sum()) for k in ("gen", "hist")}
    assert changed["gen"] <= 4 and changed["hist"] <= 4


# ---- the share of the exact-token test's rows on which the reference cannot decide

@functools.lru_cache(maxsize=None)
def _refs(V):
    cases = [sr.exact_case(V, launch) for launch in range(sr.EXACT_LAUNCHES)]
    return [(c, sr.case_refs(c)) for c in cases]


def test_share_of_undecided_cases():
    pooled = {}
    for V in (64, 4096, 32064):
        und = rows = 0
        for case, refs in _refs(V):
            n, per = sr.undecided_counts(refs, case.kinds)
            und += n
            rows += len(refs)
            for k, (a, b) in per.items():
                c = pooled.setdefault(k, [0, 0])
                c[0] += a
                c[1] += b
        print(f"V {V}: {und} of {rows} rows undecided ({100.0 * und / rows:.2f} %)")
        assert und <= 0.04 * rows, (V, und, rows)
    for k, (a, b) in sorted(pooled.items()):
        print(f"kind {sr.KINDS[k]}: {a} of {b} undecided ({100.0 * a / b:.2f} %)")
        assert a <= 0.08 * b, (sr.KINDS[k], a, b)


def test_exact_cases_cover_every_combination():
    seen = set()
    for case, _ in _refs(64):
        for m, o in enumerate(case.rows):
            seen.add((case.kinds[m], o["repeat_last_n"], int(case.state["n_gen"][m])))
            ring = case.state["hist"][m].tolist()
            if case.state["n_gen"][m] >= 17:
                assert -1 in ring and 64 + 3 in ring
        assert max(o["seed"] for o in case.rows) > 1 << 58
    assert len(seen) == len(sr.KINDS) * len(sr.LAST_N) * len(sr.N_GEN)


# ---- engine.sample_host

def test_sample_host_agrees_with_the_reference():
    rng = np.random.default_rng(7)
    kinds = sr.KINDS + [(1.0, 1, 1.0, 1.0), (0.5, 1000, 0.3, 1.2), (0.0, 40, 0.9, 0.8)]
    for i in range(200):
        V = [64, 500, 4096][i % 3]
        lg = (rng.standard_normal(V) * 3.0).astype(np.float32)
        lg[:3] += np.float32(4.0)
        if i % 4 == 1:
            lg[7] = lg[1]
            lg[20:30] = np.round(lg[20:30])
        if i % 4 == 2:
            lg[V // 2:] = -np.inf
        t, k, p, rp = kinds[i % len(kinds)]
        o = _opts(temperature=t, top_k=k, top_p=p, repeat_penalty=rp, repeat_last_n=[64, 20, 0, 200][(i // 7) % 4],
                  seed=i)
        ng = [0, 1, 5, 63, 64, 65, 100, 200][i % 8]
        history = rng.integers(0, V, ng).tolist()
        top = np.argsort(-lg, kind="stable")[:6].tolist()
        for j, t_id in enumerate(top + [-1, V + 3]):
            if 2 * j < ng:
                history[ng - 1 - 2 * j] = int(t_id)
        ring = [0] * 64
        for n, t_id in enumerate(history):
            ring[n & 63] = t_id
        r = sr.reference_detail(lg, ring, ng, o)
        ids, probs, cut = sample_host_candidates(torch.from_numpy(lg), history, o)
        assert list(ids) == r.ids, (i, o)
        assert cut == r.cut, (i, o, cut, r.cut)
        assert np.abs(np.asarray(probs) - np.asarray(r.probs)).max() <= 1e-12
        tok = sample_host(torch.from_numpy(lg), history, o, np.random.default_rng(i))
        assert tok in r.ids[:r.cut]
        if t <= 0:
            assert tok == r.token


def test_sample_host_draws_from_the_cut():
    lg = torch.from_numpy(_four_equal())
    o = _opts(top_k=4, top_p=0.75)
    rng = np.random.default_rng(0)
    counts = np.bincount([sample_host(lg, [], o, rng) for _ in range(3000)], minlength=16)
    assert counts[11] == 0 and counts[[2, 5, 9]].sum() == 3000
    assert np.abs(counts[[2, 5, 9]] / 3000 - 1 / 3).max() < 0.05  # 5.8 sigma of a third over 3,000 draws
