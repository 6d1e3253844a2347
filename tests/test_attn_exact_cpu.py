"""Host-side checks of ``tests/attn_exact.py``: the generators keep the properties that make the attention cases exact
at every (geometry, length) of ``tests/test_attn_exact_gpu.py``, and a plain torch emulation of the kernel's
algorithm over the packed caches reproduces every family exactly -- and stops doing so under each planted fault."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).parent))

import attn_exact as ax  # noqa: E402

ALL = ax.all_launches()
PARAMS = [(l, kv8) for l in ALL for kv8 in (False, True) if l.geo.kv8 or not kv8]  # the ring reads bf16 caches only
PARAM_IDS = [f"{l.id}-{'fp8' if k else 'bf16'}" for l, k in PARAMS]


def test_graded_scale_is_ln2_in_fp32():
    s = np.float32(ax.GRADED_SCALE)
    assert s * ax.LOG2E32 == np.float32(1.0)
    up, dn = np.nextafter(s, np.float32(1)), np.nextafter(s, np.float32(0))
    assert up * ax.LOG2E32 == np.float32(1.0) + np.float32(2.0 ** -23)
    assert dn * ax.LOG2E32 == np.float32(1.0) - np.float32(2.0 ** -23)


def test_case_list_covers_the_lengths():
    for g in ax.GEOS:
        Ls = ax.lengths_for(g)
        used = {L for l in ax.launches(g) for L in l.lengths if L}
        assert used == set(Ls), g.id
        for L in (1, 31, 32, 33, g.hd + 1, 32 * g.aw - 1, 32 * g.aw, 32 * g.aw + 1, 3 * 32 * g.aw + 1, g.T_max - 1,
                  g.T_max):
            assert L in Ls, (g.id, L)
        assert g.aw == (4 if g.hd == 256 or g.rows * g.Hkv > 64 else 8), g.id
        # the smallest T_max at which one split of two still holds more than 2 AW blocks
        assert g.T_max // 32 // 2 >= 2 * g.aw
        for l in ax.launches(g):
            assert sum(s < 0 for s in l.slot) == 1
            live = [s for s in l.slot if s >= 0]
            assert len(set(live)) == len(live) and all(s != m for m, s in enumerate(l.slot))
    for g in ax.RING_GEOS:
        pairs = g.rows * g.Hkv
        assert g.ring == (2 * ax.RING_CU <= pairs <= 64 * ax.RING_CU), g.id
        assert g.hd == 128 and not g.kv8 and g.nsplits == (1,)
    # several idle rows on one compute wave's list (workgroup 0, wave 0: pairs 32 i), first and last entry included
    g = ax.RING_GEOS[2]
    entries = sorted(m * g.Hkv // 32 for m in g.idle if (m * g.Hkv) % 32 == 0)
    assert entries[0] == 0 and entries[-1] == 15 and len(entries) >= 3


def _roundtrip(d: ax.Data):
    if d.kv8:
        assert torch.equal(d.K.float().to(torch.float8_e4m3fn).float(), d.K.float())
        assert torch.equal(d.V.to(torch.float8_e4m3fn).float(), d.V)
    else:
        assert torch.equal(d.K.float().bfloat16().float(), d.K.float())
        assert torch.equal(d.V.bfloat16().float(), d.V)
    assert torch.equal(d.q.float().bfloat16().float(), d.q.float())
    assert torch.equal(d.want.bfloat16().float(), d.want) and torch.equal(d.alt.bfloat16().float(), d.alt)


def _scores2(d: ax.Data, m: int, kh: int):
    """Twice the exact scores [G, T_max] int64 of row m against kv head kh of its slot (the K scale is 0.5, 1 or 2)."""
    g = d.launch.geo
    k2 = d.K[d.launch.slot[m], kh].long() * int(2 * d.kscale)
    return d.q[m, kh * g.G:(kh + 1) * g.G] @ k2.t()


@pytest.mark.parametrize("l,kv8", PARAMS, ids=PARAM_IDS)
def test_select_properties(l, kv8):
    g = l.geo
    d = ax.make(l, "select", kv8)
    _roundtrip(d)
    gap2 = 2 * int(2 * d.A * d.kscale)
    assert np.float32(gap2 / 2) * d.sl2 >= np.float32(160.0)
    tg = d.info["targets"]
    for m, (L, s) in enumerate(zip(l.lengths, l.slot)):
        if s < 0:
            assert int(d.want[m].abs().max()) == 0
            continue
        assert {0, L - 1} <= set(tg[m].tolist())
        for t in (31, 32, 32 * (L // 32 - 1) + 7):
            if 0 <= t < L and g.H >= 5:
                assert t in tg[m].tolist(), (m, L, t)
        assert bool((d.V[s, :, L:] == ax.V_POISON[kv8]).all())
        for kh in range(g.Hkv):
            sc = _scores2(d, m, kh)
            assert int(sc.abs().max()) < 2 * ax.TWO24
            for gi in range(g.G):
                h = kh * g.G + gi
                t = int(tg[m, h])
                live = sc[gi, :L]
                assert int(live.argmax()) == t and int((live == live[t]).sum()) == 1
                if L > 1:
                    rest = torch.cat([live[:t], live[t + 1:]])
                    assert int(live[t] - rest.max()) == gap2  # one head dim
                assert torch.equal(d.want[m, h], d.V[s, kh, t] * d.vscale)
                if L < g.T_max:  # the poison would win outright
                    assert int(sc[gi, L:].min()) > int(live[t])
            # the origin is a target: every single flip present is a neighbour at exactly one head dim
            h0 = kh * g.G + kh % g.G
            live = sc[kh % g.G, :L]
            assert int((live == live[int(tg[m, h0])] - gap2).sum()) == min(g.hd, L - 1)
            first = d.K[s, kh, int(tg[m, kh * g.G])].long()
            if L < g.T_max:
                assert bool((d.K[s, kh, L:].long() == 2 * first).all())
    used = {s for s in l.slot if s >= 0}
    for s in range(l.S):
        if s not in used:
            assert bool((d.V[s] == ax.V_POISON[kv8]).all()) and bool((d.K[s].abs() == 2).all())


@pytest.mark.parametrize("l,kv8", PARAMS, ids=PARAM_IDS)
def test_uniform_properties(l, kv8):
    g = l.geo
    d = ax.make(l, "uniform", kv8)
    _roundtrip(d)
    assert int(d.q.abs().max()) == 0
    for m, (L, s) in enumerate(zip(l.lengths, l.slot)):
        if s < 0:
            continue
        v = d.V[s, :, :L].double()
        assert float(v.abs().max()) <= (10 if kv8 else 72)
        assert torch.equal(v, v.round())
        c = d.info["c"][m]
        assert torch.equal(v.sum(1).long(), L * c)  # zero-sum perturbation: the mean is the integer c
        assert int(c.abs().max()) <= (4 if kv8 else 64)
        assert torch.equal(d.want[m], c.float().repeat_interleave(g.G, 0))
        assert bool((d.V[s, :, L:] == ax.V_POISON[kv8]).all())
        if L > 1:
            assert bool((v != c[:, None].double()).any())  # the perturbation is there


@pytest.mark.parametrize("l,kv8", PARAMS, ids=PARAM_IDS)
def test_graded_properties(l, kv8):
    g = l.geo
    d = ax.make(l, "graded", kv8)
    _roundtrip(d)
    assert d.sl2 == np.float32(1.0)
    assert float(d.V[[s for s in l.slot if s >= 0]].abs().max()) == ax.V_POISON[kv8]
    n_live = 0
    for m, (L, s) in enumerate(zip(l.lengths, l.slot)):
        if s < 0:
            continue
        n_live += 1
        assert float(d.V[s, :, :L].abs().max()) <= 16
        for kh in range(g.Hkv):
            sc = _scores2(d, m, kh) // 2  # [G, T_max] integer scores = scaled scores
            near = [t for t, _ in d.info["near"][(m, kh)]]
            assert 0 in near and L - 1 in near
            far = torch.ones(L, dtype=torch.bool)
            far[near] = False
            for gi in range(g.G):
                live = sc[gi, :L]
                top = int(live.max())
                e = top - live[near]
                assert int(e.min()) == 0 and int(e.max()) <= 3  # p = 2^-e: multiples of 2^-3
                if bool(far.any()):
                    assert top - int(live[far].max()) >= 160  # p = 0 exactly
                if L < g.T_max:
                    assert int(sc[gi, L:].min()) > top
                # the expectation, recomputed from the scores alone
                w = (8 >> e).long()
                num8 = (w[:, None] * d.V[s, kh, near].long()).sum(0)
                assert int(num8.abs().max()) < 8 * (1 << 15)
                h = kh * g.G + gi
                assert torch.equal(num8, d.info["num8"][m, h]) and int(w.sum()) == int(d.info["den8"][m, h])
    if g.G > 1 and max(l.lengths) > 64:  # the heads of a group weigh the near set differently
        assert len({tuple(d.want[m, h].tolist()) for m in range(g.rows) for h in range(g.H)}) > n_live * g.Hkv
    assert d.near_mid < 0.01 * d.want.numel(), (d.near_mid, d.want.numel())
    x = d.info["num8"].double() / d.info["den8"].double()
    ok = (x - d.want.double()).abs() <= x.abs() * 2.0 ** -8
    assert bool(ok.all())


def test_bf16_neighbours():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 2.0 ** -9, -3.0 - 2.0 ** -7, 5.3],
                     dtype=torch.float64)
    r, alt, near = ax.bf16_neighbours(x)
    assert near.tolist() == [False, True, True, False, True, False]
    assert r.tolist()[:2] == [1.0, 1.0] and float(r[3]) == 1.0  # an exact tie goes to even
    assert alt.tolist()[:2] == [1.0, 1.0078125] and float(alt[3]) == 1.0
    assert sorted([float(r[2]), float(alt[2])]) == [1.0, 1.0078125]  # 2^-30 past the midpoint: either neighbour
    assert sorted([float(r[4]), float(alt[4])]) == [-3.015625, -3.0]
    assert float(alt[5]) == float(r[5])


# ---------------------------------------------------------------- the emulation and the planted faults
EMU_GEOS = [ax.GEOS[0], ax.GEOS[1], ax.GEOS[3]]  # 8 waves with GQA 4; G = 16 at hd 64; 4 waves at hd 256
EMU = [(l, kv8) for g in EMU_GEOS for l in ax.launches(g) for kv8 in (False, True)]


@pytest.mark.parametrize("l,kv8", EMU, ids=[f"{l.id}-{'fp8' if k else 'bf16'}" for l, k in EMU])
def test_emulation_reproduces_every_family(l, kv8):
    for fam in ax.FAMILIES:
        d = ax.make(l, fam, kv8)
        q, kp, vp = ax.pack(d)
        for nsplit in (1, 3):
            ax.assert_equal(d, ax.emulate(d, kp, vp, q, nsplit), f"nsplit {nsplit}")


#: fault -> (families that must flag it at some listed length, families that cannot).  Why:
#:   mask_le             position L leaks: the poison K wins (select, graded) or its V joins the sum (uniform)
#:   skip_last_block     position L - 1 is a select target and a graded near position; uniform loses terms
#:   drop_wave           wave 0 holds block 0: position 0 is a select target and a graded near position
#:   loser_l_unweighted  select: den > 1; graded: a wave of far positions adds its count; uniform: every f is 1
#:   skip_kfrag          select: the origin's neighbours that flip dims 32..63 tie; uniform: q = 0
#:   swap_v_order        select: the head that targets 0 reads position 31
#:   ignore_slot         every row's slot differs from its index
#:   alpha_not_on_l      select: a wave that met a loser first keeps its l; graded: a rising maximum; uniform: alpha 1
FAULT_FAMILIES = {
    "mask_le": ({"select", "uniform", "graded"}, set()),
    "skip_last_block": ({"select", "uniform", "graded"}, set()),
    "drop_wave": ({"select", "uniform", "graded"}, set()),
    "loser_l_unweighted": ({"select", "graded"}, {"uniform"}),
    "skip_kfrag": ({"select"}, {"uniform"}),
    "swap_v_order": ({"select"}, set()),
    "ignore_slot": ({"select", "uniform", "graded"}, set()),
    "alpha_not_on_l": ({"select", "graded"}, {"uniform"}),
}


@pytest.fixture(scope="module")
def fault_cases():
    """The three families of the first geometry (8 waves, 3 splits), bf16, every launch: between them every listed
    length."""
    out = []
    for l in ax.launches(ax.GEOS[0]):
        for fam in ax.FAMILIES:
            d = ax.make(l, fam, False)
            out.append((d, ax.pack(d)))
    return out


@pytest.mark.parametrize("fault", ax.FAULTS)
def test_planted_fault_is_flagged(fault_cases, fault):
    must, never = FAULT_FAMILIES[fault]
    flagged = {}
    for d, (q, kp, vp) in fault_cases:
        rep = ax.mismatches(d, ax.emulate(d, kp, vp, q, 3, fault=fault))
        if rep is not None:
            flagged.setdefault(d.family, rep)
    assert must <= set(flagged), (fault, sorted(flagged))
    assert not (never & set(flagged)), (fault, {f: flagged[f] for f in never & set(flagged)})
    for rep in flagged.values():  # the report names row, heads and tile
        assert "query head" in rep and "kv head" in rep and "tile" in rep


def test_select_report_names_the_position_read():
    l = ax.launches(ax.GEOS[0])[0]
    d = ax.make(l, "select", False)
    q, kp, vp = ax.pack(d)
    rep = ax.mismatches(d, ax.emulate(d, kp, vp, q, 1, fault="swap_v_order"))
    assert rep is not None and "output equals the V row of position(s) [" in rep, rep
