"""The host reference of the samplers' further options (tests/sampler_ref_ext.py) itself: the presence / frequency
penalty arithmetic and the ``min_p`` prefix on rows small enough to compute by hand, its equality with
tests/sampler_ref.py at neutral values, engine.sample_host_candidates against it, and the share of the exact-token
test's rows on which it cannot decide the token.  No GPU."""
import functools

import numpy as np
import torch

import sampler_ref as sr
import sampler_ref_ext as sx
from cain_amd.engine.engine import sample_host, sample_host_candidates


def _opts(**kw):
    o = dict(temperature=1.0, top_k=40, top_p=1.0, repeat_penalty=1.0, repeat_last_n=64, eos_id=-1, seed=1)
    o.update(kw)
    return o


NO_HIST = [0] * 64
LG = np.array([0.0, -2.0, 3.0, 4.0, 1.0, 0.5], dtype=np.float32)
RING = [1, 3, 3, 0, 3, -1, 9, 6] + [0] * 56  # ids 1, 3 (three times), 0; then three outside [0, 6)


def test_penalty_hand_case():
    o = _opts(repeat_penalty=2.0, presence_penalty=0.5, frequency_penalty=0.25)
    v, pen, counts = sx.penalise_ext(LG, RING, 8, o)
    assert sorted(pen) == [0, 1, 3] and counts == {1: 1, 3: 3, 0: 1}
    # id 0: 0 * 2 - (0.25 + 0.5); id 1: -2 * 2 - 0.75; id 3: 4 / 2 - (3 * 0.25 + 0.5)
    assert v.tolist() == [-0.75, -4.75, 3.0, 0.75, 1.0, 0.5]
    r = sx.reference_detail_ext(LG, RING, 8, dict(o, temperature=0.0))
    assert r.token == 2 and r.values.tolist() == v.tolist()  # the penalties apply before the argmax


def test_penalty_window():
    o = _opts(presence_penalty=0.0, frequency_penalty=0.25)
    for oo, ng in ((dict(o, repeat_last_n=0), 8), (o, 0)):  # a window of 0, nothing generated yet
        v, pen, _ = sx.penalise_ext(LG, RING, ng, oo)
        assert pen == [] and v.tolist() == LG.tolist()
    # the last 2 of 5 are slots 4 and 3 (ids 3 and 0): id 3 counts once, not three times
    v, pen, counts = sx.penalise_ext(LG, RING, 5, dict(o, repeat_last_n=2))
    assert pen == [3, 0] and counts == {3: 1, 0: 1}
    assert v.tolist() == [-0.25, -2.0, 3.0, 3.75, 1.0, 0.5]
    # the last 2 of 8 are ids outside the vocabulary: nothing changes
    assert sx.penalise_ext(LG, RING, 8, dict(o, repeat_last_n=2))[1] == []
    # the whole window of 5: id 3 three times
    assert sx.penalise_ext(LG, RING, 5, o)[0].tolist() == [-0.25, -2.25, 3.0, 3.25, 1.0, 0.5]


def test_presence_alone_activates_the_stage():
    v, pen, _ = sx.penalise_ext(LG, RING, 8, _opts(repeat_penalty=1.0, presence_penalty=0.5))
    assert sorted(pen) == [0, 1, 3] and v.tolist() == [-0.5, -2.5, 3.0, 3.5, 1.0, 0.5]
    v, pen, _ = sx.penalise_ext(LG, RING, 8, _opts(repeat_penalty=1.0))
    assert pen == [] and v.tolist() == LG.tolist()


def _four_equal(V=16):
    lg = np.full(V, -50.0, dtype=np.float32)
    lg[[2, 5, 9, 11]] = 1.0
    return lg


def test_min_p_keeps_equal_ratios():
    """Four equal candidates: every ratio is exp(0) = 1, and `>=` keeps all four at min_p 1.0."""
    r = sx.reference_detail_ext(_four_equal(), NO_HIST, 0, _opts(top_k=4, min_p=1.0), delta=0.0)
    assert r.ids == [2, 5, 9, 11] and r.cut == 4
    r = sx.reference_detail_ext(_four_equal(), NO_HIST, 0, _opts(top_k=8, min_p=1.0), delta=0.0)
    assert len(r.ids) == 8 and r.cut == 4  # the -50s have ratio exp(-51)


def _two_level(V=16):
    lg = np.full(V, -50.0, dtype=np.float32)
    lg[0], lg[1] = 1.0, 0.0  # ratios 1, exp(-1) = 0.3679, exp(-51)
    return lg


def test_min_p_prefix():
    for mp, cut in ((0.5, 1), (0.3, 2), (0.37, 1), (0.36, 2), (1e-30, 16), (0.0, 16)):
        r = sx.reference_detail_ext(_two_level(), NO_HIST, 0, _opts(top_k=0, min_p=mp), delta=0.0)
        assert r.ids[:2] == [0, 1] and r.cut == cut, (mp, r.cut)
    # the temperature scales the ratio: at T = 2 it is exp(-0.5) = 0.6065
    assert sx.reference_detail_ext(_two_level(), NO_HIST, 0, _opts(min_p=0.5, temperature=2.0), delta=0.0).cut == 2


def test_min_p_and_top_p_take_the_shorter_prefix():
    r = sx.reference_detail_ext(_four_equal(), NO_HIST, 0, _opts(top_k=4, top_p=0.5, min_p=1.0), delta=0.0)
    assert r.cut == 2  # top-p is the shorter
    r = sx.reference_detail_ext(_two_level(), NO_HIST, 0, _opts(top_p=0.9, min_p=0.5), delta=0.0)
    assert r.cut == 1 and r.admissible == {0}  # min_p is the shorter (top-p alone keeps two: 0.731 < 0.9)
    assert sx.reference_detail_ext(_two_level(), NO_HIST, 0, _opts(top_p=0.9), delta=0.0).cut == 2
    # the pick renormalises over the cut: with three of four kept by top-p and all by min_p, thirds
    for seed in range(50):
        u = sr.u_of(seed, 4)
        r = sx.reference_detail_ext(_four_equal(), NO_HIST, 4, _opts(top_k=4, top_p=0.75, min_p=0.9, seed=seed),
                                    delta=0.0)
        assert r.cut == 3 and r.token == [2, 5, 9][min(int(u * 3), 2)]


def test_min_p_is_ignored_when_greedy():
    r = sx.reference_detail_ext(_two_level(), NO_HIST, 0, _opts(temperature=0.0, min_p=1.0))
    assert r.token == 0 and r.ids == [0] and r.cut == 1
    assert sample_host(torch.from_numpy(_two_level()), [], _opts(temperature=0.0, min_p=1.0), None) == 0


def test_min_p_comparison_near_its_bound_admits_both():
    lg = _two_level()
    mp = float(np.exp(-1.0))
    seed = next(s for s in range(1000) if 0.9 < sr.u_of(s, 0))  # a draw that lands on candidate 1 when it is kept
    r = sx.reference_detail_ext(lg, NO_HIST, 0, _opts(min_p=mp * (1 + 5e-5), seed=seed))
    assert r.cut == 1 and r.token == 0 and r.admissible == {0, 1} and not r.decided
    r = sx.reference_detail_ext(lg, NO_HIST, 0, _opts(min_p=mp * (1 + 5e-4), seed=seed))
    assert r.cut == 1 and r.admissible == {0}
    r = sx.reference_detail_ext(lg, NO_HIST, 0, _opts(min_p=mp * (1 - 5e-4), seed=seed))
    assert r.cut == 2 and r.admissible == {1}


def test_neutral_values_equal_the_plain_reference():
    for launch in range(sr.EXACT_LAUNCHES):
        case = sr.exact_case(64, launch)
        for m, o in enumerate(case.rows):
            args = (case.logits[m], case.state["hist"][m], int(case.state["n_gen"][m]))
            a = sr.reference_detail(*args, o)
            for oo in (o, dict(o, min_p=0.0, presence_penalty=0.0, frequency_penalty=0.0)):
                b = sx.reference_detail_ext(*args, oo)
                assert (a.admissible, a.token, a.ids, a.probs, a.cut, a.penalised, a.support, a.firsts) == \
                    (b.admissible, b.token, b.ids, b.probs, b.cut, b.penalised, b.support, b.firsts), (launch, m)
                assert np.array_equal(a.values.view(np.int32), b.values.view(np.int32))


# ---- the exact-token test's rows (tests/test_sampler_ext_gpu.py)

@functools.lru_cache(maxsize=None)
def _refs(V):
    cases = [sx.exact_case_ext(V, launch) for launch in range(sr.EXACT_LAUNCHES)]
    return [(c, sx.case_refs_ext(c)) for c in cases]


def test_ext_cases_mix_and_count():
    seen, counts = set(), set()
    for case, refs in _refs(64):
        for m, o in enumerate(case.rows):
            assert tuple(o[k] for k in sx.EXT_KEYS) == sx.EXT[case.exts[m]]
            seen.add((case.kinds[m], case.exts[m]))
            counts |= set(sx.penalise_ext(case.logits[m], case.state["hist"][m], int(case.state["n_gen"][m]), o)[2]
                          .values())
    assert len(seen) == len(sr.KINDS) * len(sx.EXT)  # 7 and 9 are coprime: every pair within 63 rows
    assert {1, 2, 3} <= counts


def test_sample_host_candidates_agree_with_the_reference():
    for V in (64, 4096):
        for case, refs in _refs(V):
            for m, (o, r) in enumerate(zip(case.rows, refs)):
                ng = int(case.state["n_gen"][m])
                ring = case.state["hist"][m]
                history = [0] * ng
                for j in range(min(ng, sr.HIST)):
                    history[ng - 1 - j] = int(ring[(ng - 1 - j) & (sr.HIST - 1)])
                ids, probs, cut = sample_host_candidates(torch.from_numpy(case.logits[m]), history, o)
                assert list(ids) == r.ids and cut == r.cut, (V, m, o, cut, r.cut)
                assert np.abs(np.asarray(probs) - np.asarray(r.probs)).max() <= 1e-12
                tok = sample_host(torch.from_numpy(case.logits[m]), history, o, np.random.default_rng(m))
                assert tok in r.ids[:r.cut]


def test_share_of_undecided_cases():
    by_kind, by_ext = {}, {}
    for V in (64, 4096, 32064):
        und = rows = 0
        for case, refs in _refs(V):
            und += sr.undecided_counts(refs, case.kinds)[0]
            rows += len(refs)
            for pooled, keys in ((by_kind, case.kinds), (by_ext, case.exts)):
                for k, (a, b) in sr.undecided_counts(refs, keys)[1].items():
                    c = pooled.setdefault(k, [0, 0])
                    c[0] += a
                    c[1] += b
        print(f"V {V}: {und} of {rows} rows undecided ({100.0 * und / rows:.2f} %)")
        assert und <= 0.04 * rows, (V, und, rows)
    for name, pooled, table in (("kind", by_kind, sr.KINDS), ("ext", by_ext, sx.EXT)):
        for k, (a, b) in sorted(pooled.items()):
            print(f"{name} {table[k]}: {a} of {b} undecided ({100.0 * a / b:.2f} %)")
            assert a <= 0.08 * b, (name, table[k], a, b)
