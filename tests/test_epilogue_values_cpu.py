"""Host checks of tests/epilogue_values.py: the one-hot cases deliver their values exactly through every path's
intermediate formats, the value sets reach what they claim (and what the quantised formats cannot express is printed),
few elements are undecided, every planted fault is reported, and the derived activation bounds stay below 2^-12."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).parent))

import epilogue_values as ev  # noqa: E402
import exact  # noqa: E402

ids = lambda p: p.id  # noqa: E731
BF16_PATHS = [p for p in ev.PATHS if p.fam == "bf16"]
QUANT_PATHS = [p for p in ev.PATHS if p.fam != "bf16"]


def test_number_formats_written_out():
    v = torch.randn(4096, generator=torch.Generator().manual_seed(1)).double() * 1e3
    assert torch.equal(ev.bf16_rne(v.float().double()), v.float().bfloat16().double())  # one rounding from fp32
    t64 = lambda a: torch.tensor([a], dtype=torch.float64)  # noqa: E731
    assert float(ev.bf16_rne(t64(1.0 + 2.0 ** -8))) == 1.0  # a tie, to even
    assert float(ev.bf16_rne(t64(1.0 + 2.0 ** -8 + 2.0 ** -40))) == 1.0 + 2.0 ** -7  # just past it (fp32 would not see it)
    assert float(ev.bf16_rne(t64(3.4e38))) == float("inf")
    fin, ties = ev.e4m3_finite(), ev.e4m3_ties()
    assert len(fin) == 127 and float(fin[-1]) == 448.0 and float(ties[0]) == 2.0 ** -10 and float(ties[-1]) == 464.0
    assert torch.equal(ev.e4m3_sat(fin), fin) and torch.equal(ev.e4m3_sat(-fin), -fin)
    q = ev.e4m3_sat(ties)  # every tie goes to the even code: 2^-10 to zero, 464 saturates
    assert float(q[0]) == 0.0 and float(q[-1]) == 448.0
    assert bool(((q[:-1] == fin[:-1]) | (q[:-1] == fin[1:])).all())
    lo, hi = ev.bf16_neighbours(ties)
    assert torch.equal(ev.e4m3_sat(lo[:-1]), fin[:-1]) and torch.equal(ev.e4m3_sat(hi[:-1]), fin[1:])
    assert ev.SENT8 == int(torch.tensor([ev.SENT]).to(torch.float8_e4m3fn).view(torch.uint8))


@pytest.mark.parametrize("geo", list(ev.GEOS))
@pytest.mark.parametrize("p", BF16_PATHS, ids=ids)
def test_bf16_qkv_cases_deliver_and_reach(p, geo):
    d, bias, slot, pos, S = ev.qkv_inputs(p, geo)
    N = exact.qkv_n(ev.GEOS[geo])
    assert d.acc.shape == (p.M, N) and bool((d.x.sum(1) == 1).all()) and bool(d.w.isfinite().all())
    for ks in ((1, 2, 4) if p.plan == (0, -1) else (None,)):  # the default wide plan: whatever the rule picks
        ranges, slab = ev.path_ranges(p, N, ks)
        assert ev.delivery_exact(d, ranges, slab) is None, p.id
    if p.M >= 8:
        assert int((slot < 0).sum()) >= 1 and 0 in pos[slot >= 0].tolist() and ev.T_MAX - 1 in pos[slot >= 0].tolist()
        live = [(int(s), int(t)) for s, t in zip(slot, pos) if s >= 0]
        assert len(set(live)) == len(live) and max(sum(1 for s, _ in live if s == s0) for s0, _ in live) >= 5
    s = (d.acc.float() + bias[None, :]).bfloat16().double()[slot >= 0]  # what the epilogue rounds and converts
    got = ev.reach(s, p.cap)
    print(p.id, geo, {k: f"{a}/{b}" for k, (a, b) in got.items()})
    if p.M >= 16:  # every member of every class, both signs
        assert all(a == b for a, b in got.values()), got
    v_sums = s[:, -ev.GEOS[geo][1] * ev.GEOS[geo][2]:]
    on_tie = torch.isin(v_sums.abs(), ev.e4m3_ties())
    assert int((on_tie & (bias[-v_sums.shape[1]:] != 0)[None, :]).sum()) > 0  # a biased sum lands on a tie


def test_scaled_fp16_slabs_need_the_cap():
    """The mirror bites: with the largest bf16 in the value set a scaled fp16 slab loses the small values beside it."""
    p = next(p for p in BF16_PATHS if p.plan == (2, 0) and p.M == 65)
    d = ev.qkv_bf16_case("gqa", p.M, p.K, 5, cap=None)[0]
    rep = ev.delivery_exact(d, exact.wide_k_ranges(p.K, 2), "f16exp")
    assert rep is not None and "no fp16 number" in rep
    assert ev.delivery_exact(d, exact.wide_k_ranges(p.K, 2), "f32") is None


@pytest.mark.parametrize("p", QUANT_PATHS, ids=ids)
def test_quantised_cases_deliver_and_reach(p):
    geo = "gqa"
    d, bias, slot, pos, S = ev.qkv_inputs(p, geo)
    N = exact.qkv_n(ev.GEOS[geo])
    ranges, slab = ev.path_ranges(p, N)
    assert (slab == "f16") == (p.tag == "widesplit")
    assert ev.delivery_exact(d, ranges, slab) is None, p.id
    a = d.x.abs().amax(1)
    unit = 448.0 if p.fam in ev.A8 else 1.0
    assert bool((torch.log2(a / unit) % 1 == 0).all())  # powers of two (x 448): the row quantiser is exact
    s = (d.acc.float() + bias[None, :]).bfloat16().double()[slot >= 0]
    got = ev.reach(s)
    missing = {k: b - a_ for k, (a_, b) in got.items()}
    print(f"{p.id}: cannot reach (of the signed members) " + ", ".join(f"{k} {missing[k]}/{got[k][1]}" for k in got))
    assert float(s.abs().max()) > 464.0 and float(s[s != 0].abs().min()) < 2.0 ** -9  # saturation and the subnormals
    assert got["e4m3"][0] > 0 and got["zero"][0] == 1


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("geo", list(ev.GEOS))
@pytest.mark.parametrize("p", [p for p in ev.PATHS if p.M in (16, 40, 65)], ids=ids)
def test_undecided_cap_and_planted_faults(p, geo, kv8):
    """The mirror without a fault passes, with at most 1 % of the elements undecided; each planted fault is reported
    where ``QKV_FAULT_SHOWS`` says it shows and not where it cannot."""
    d, bias, slot, pos, S = ev.qkv_inputs(p, geo)
    g = ev.GEOS[geo]
    cos, sin = ev.rope_tables(g[2])
    want = ev.qkv_want(d.acc, bias, slot, pos, cos, sin, g, S, kv8)
    st, rep = ev.qkv_check(*ev.qkv_mirror(d.acc, bias, slot, pos, cos, sin, g, S, kv8), want)
    print(st.line(f"{p.id} {geo} kv8={kv8}"))
    assert rep is None, rep
    assert st.undecided <= 0.01 * (st.decided + st.undecided) and st.worst <= 1.0
    if p.fam not in ("bf16", "q4_k"):  # one quantised family is enough for the fault table
        return
    for fault in ev.QKV_FAULTS:
        _, rep = ev.qkv_check(*ev.qkv_mirror(d.acc, bias, slot, pos, cos, sin, g, S, kv8, fault=fault), want)
        assert (rep is not None) == ev.QKV_FAULT_SHOWS[fault, kv8], (fault, rep)


def test_sentinels_and_idle_rows_are_checked():
    p = next(p for p in BF16_PATHS if p.tag == "batched" and p.M == 17)
    d, bias, slot, pos, S = ev.qkv_inputs(p, "phi3")
    g = ev.GEOS["phi3"]
    cos, sin = ev.rope_tables(g[2])
    want = ev.qkv_want(d.acc, bias, slot, pos, cos, sin, g, S, False)
    q, K, V = ev.qkv_mirror(d.acc, bias, slot, pos, cos, sin, g, S, False)
    free = (want["owner"] < 0).nonzero()[0]
    for t in (K, V):
        t2 = t.clone()
        t2[int(free[0]), 0, int(free[1]), 3] = 0.0
        _, rep = ev.qkv_check(q, t2 if t is K else K, t2 if t is V else V, want)
        assert rep is not None
    q2 = q.clone()
    q2[int((slot < 0).nonzero()[0]), 5] = 1.0
    assert ev.qkv_check(q2, K, V, want)[1] is not None


@pytest.mark.parametrize("kind", ["silu", "gelu"])
@pytest.mark.parametrize("p,norm", ev.ACT_CASES, ids=ev.act_id)
def test_activation_cases(p, norm, kind):
    d = ev.act_inputs(p, kind, norm)
    ranges, slab = ev.path_ranges(p, 2 * ev.ACT_F, 1 if p.plan == (0, -1) else None)
    assert ev.delivery_exact(d, ranges, slab) is None
    ref = ev.act_case_ref(d, kind, norm)
    c = ref["checked"]
    rel = (ref["E"][c] / ref["r"][c].abs().clamp(min=1e-300))
    assert float(rel[ref["r"][c] != 0].max()) <= 2.0 ** -12  # the derived bound, never wider
    # the fp64 reference rounded to bf16 passes its own check; one bf16 step off does not
    y = ev.bf16_rne(ref["r"])
    st, rep = ev.act_check(y, ref)
    print(st.line(f"{p.id} {kind} norm={norm}"))
    assert rep is None and st.worst <= 1.0, rep
    i = tuple(int(v) for v in (c & (ref["r"].abs() > 1e-3)).nonzero()[0])
    y2 = y.clone()
    y2[i] = y2[i] + 2 * ev.half_step(y[i])
    assert ev.act_check(y2, ref)[1] is not None
    if p.fam == "bf16":
        g = ref["g"]
        skipped = ~c & ~ref["pos"] & ~ref["neg"]
        if kind == "silu":  # nothing inside the grid is left out (the norm's factor may push its ends just past 80)
            assert not bool((skipped & (g.abs() <= 80)).any()) and int(skipped.sum()) <= 0.01 * g.numel()
        else:  # GeLU's cancellation: only gates well below zero are left out
            assert float(g[skipped & (g.abs() <= 80)].max()) < -2.0 and float(g[c].min()) < -2.0
        if not norm:
            assert st.exact == p.M * 4 * len(ev.GATE_EXTREMES)
            assert float(g[c].min()) <= -79 and float(g[c].max()) >= 79 if kind == "silu" else float(g[c].max()) >= 79
        # a gate row paired with the up row of the next column: reported
        up1 = torch.roll(ref["u"], 1, 1)
        assert ev.act_check(ev.bf16_rne(ev.act_f(g, kind) * up1), ref)[1] is not None


@pytest.mark.parametrize("p", ev.NORM_PATHS, ids=ids)
def test_norm_cases(p):
    d = ev.norm_inputs(p)
    ss = d.x.pow(2).sum(1)
    assert bool((ss == ss.round()).all()) and sorted(set((d.x != 0).sum(1).tolist())) == [1, 2, 3, 4][: min(4, p.M)]
    assert ev.delivery_exact(d, None, "f32") is None
    if p.fam == "bf16":  # only the delivering column meets a weight
        assert bool((((d.x != 0) & (d.w != 0).any(0)[None, :]).sum(1) == 1).all())
    r = d.acc * ev.norm_factor(d.x, ev.EPS)
    for y in (r.float(), ev.bf16_rne(r).bfloat16()):
        st, rep = ev.norm_check(y, d, ev.rho_norm(p.fam))
        assert rep is None and st.worst <= 1.0, rep
    bad = (r * (1 + 12 * ev.U24)).float()  # a factor off by 12 x 2^-24
    assert ev.norm_check(bad, d, ev.rho_norm(p.fam))[1] is not None
