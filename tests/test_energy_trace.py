"""The GPU energy path against the exact integral: a scripted amd-smi stand-in (tests/csrc/fake_amdsmi.cpp) makes the
energy accumulator a pure function of CLOCK_MONOTONIC, a child process runs the real sampler and meter on it, and
every window is compared with the closed-form integral of the power schedule, held here in integer nanojoules.

The stand-in updates every CAD = 16 ms: acc = floor(E(tq) / res) with res = float32(15.259) uJ, timestamp = tq - offset.
A trace point k is therefore (tq_k, E(tq_k) - E(tq_0) + q_k) with |q_k| < 1 count, and the sampler places it at
tq_k + delta, where delta = min over all polls of (poll time - tq) is the bias of its offset estimate (measured from
the returned trace, printed).  Bounds used below, derived rather than fitted:

  QUANT(E) = 4 * res + 1e-9 * E   two window edges, each interpolated between two points that are < 1 count off; the
                                  relative term is double rounding of the running sum
  shift    = |P(b) - P(a)| * delta  a uniform delay of the time axis moves both edges; at equal power it cancels
  kink     = dP * CAD / 4         an edge inside an update interval with a power step: the chord of a two-slope line over
                                  CAD with the kink at fraction s is off by s * (1 - s) * dP * CAD <= dP * CAD / 4
  P * d    without device timestamps a point sits at its observation time tq_k + d_k, so the interpolant lies between
           E(t - d) and E(t); d = the largest delay of the points that bracket the window's edges

All scenarios start together in children of their own (the sampler opens amd-smi once per process); nothing here
needs a GPU.
"""
import json
import math
import os
import shutil
import struct
import subprocess
import sys
import time
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
FAKE_SRC = ROOT / "tests" / "csrc" / "fake_amdsmi.cpp"
CHILD = ROOT / "tests" / "energy_trace_child.py"

MS = 1_000_000
CAD = 16 * MS
RES_UJ = struct.unpack("f", struct.pack("f", 15.259))[0]  # the float the stand-in reports
RES_J = RES_UJ * 1e-6
TS_OFFSET = 123_456_789_012
U32_MAX = 4294967295
T1, T2 = 20 * CAD + 5 * MS, 40 * CAD + 11 * MS  # power steps of the step schedule, inside update intervals 20 and 40
STEP = [(0, 300), (T1, 1000), (T2, 300)]
LATE_T = 31 * CAD  # the read that first sees the update at 31 CAD blocks for 80 ms
BACK_T, BACK_COUNTS = 30 * CAD, 5_000_000  # 76 J down; one interval at 600 W is 9.6 J


def sched_str(s):
    return ",".join([str(s[0][1])] + [f"{t}:{w}" for t, w in s[1:]])


def energy_nj(sched, rel):
    """Exact integral of a [(start, watts), ...] schedule from the origin to `rel` ns, in nanojoules (W * ns)."""
    e = 0
    for i, (t, w) in enumerate(sched):
        if t >= rel:
            break
        end = min(sched[i + 1][0], rel) if i + 1 < len(sched) else rel
        e += w * (end - t)
    return e


def truth_j(sched, a_rel, b_rel):
    return (energy_nj(sched, b_rel) - energy_nj(sched, a_rel)) * 1e-9


def power_at(sched, rel):
    return [w for t, w in sched if t <= rel][-1]


def quant(e):
    return 4 * RES_J + 1e-9 * abs(e)


def num(x):
    return float(x) if isinstance(x, str) else x


SCENARIOS = {
    # name: (environment of the stand-in, config of the child); times relative to the origin, filled in by `runs`
    "base": ({"NGPU": 2, "POWER_0": "650", "POWER_1": sched_str(STEP)}, {"smi": [0, 1], "run_ms": 1000}),
    "ts_zero": ({"POWER_0": "800", "TS_MODE": "zero"}, {"smi": [0], "run_ms": 1000}),
    "ts_ticks": ({"POWER_0": "800", "TS_MODE": "ticks10"}, {"smi": [0], "run_ms": 1000}),
    "late": ({"POWER_0": "700", "BLOCK": f"{LATE_T}:{80 * MS}:after"}, {"smi": [0], "run_ms": 1000}),
    "late_before": ({"POWER_0": "700", "BLOCK": f"{LATE_T}:{80 * MS}:before"}, {"smi": [0], "run_ms": 1000}),
    "fail": ({"NGPU": 2, "POWER_0": "500", "POWER_1": "500", "FAIL_0": f"{300 * MS}:{400 * MS}", "FAIL_1": "always"},
             {"smi": [0, 1], "run_ms": 800}),
    "back": ({"POWER_0": "600", "BACK_0": f"{BACK_T}:{BACK_COUNTS}"}, {"smi": [0], "run_ms": 1000}),
    "slots_10": ({"NGPU": 2, "CPU_BETWEEN": 1, "POWER_0": "300", "POWER_1": "900"}, {"smi": [1, 0], "run_ms": 600}),
    "slots_01": ({"NGPU": 2, "CPU_BETWEEN": 1, "POWER_0": "300", "POWER_1": f"300,{40 * CAD}:900"},
                 {"smi": [0, 1], "run_ms": 600, "idle_s": 0.4}),
    "slow": ({"NGPU": 3, "POWER_0": "300", "POWER_1": "300", "POWER_2": "300", "CURPOWER_0": 432, "GFX_0": 40,
              "VRAM_0": "1000:4000", "CURPOWER_1": U32_MAX, "SOCKPOWER_1": 555, "GFX_1": U32_MAX, "UMC_1": U32_MAX,
              "VRAM_1": "10:0", "CURPOWER_2": 0, "SOCKPOWER_2": 444, "GFX_2": 60, "VRAM_2": "3000:4000"},
             {"smi": [0, 1, 2], "run_ms": 300, "period_ms": 20.0}),
    "trim": ({"POWER_0": "400"}, {"smi": [0], "run_ms": 4000}),
}


def rel_windows(*pairs):
    return [[0, ["abs", a], ["abs", b]] for a, b in pairs]


def queries_for(name):
    """Window lists per scenario ("abs" times still relative to the origin here)."""
    first, last = lambda d=0: ["first", d], lambda d=0: ["last", d]  # noqa: E731
    A = lambda t: ["abs", t]  # noqa: E731
    if name == "base":
        const = [(10 * CAD, 10 * CAD + 2 * MS), (12 * CAD + 3 * MS, 12 * CAD + 5 * MS),  # 2 ms: grid / mid-interval
                 (15 * CAD + 14 * MS, 16 * CAD + 3 * MS), (18 * CAD, 18 * CAD + 5 * MS),  # 5 ms, one across an update
                 (20 * CAD, 20 * CAD + 50 * MS), (22 * CAD + 7 * MS, 22 * CAD + 57 * MS)]  # 50 ms
        q = [[0, A(a), A(b)] for a, b in const]
        q += [[0, first(), last()],                                     # 6: the whole run
              [0, A(-100 * MS), A(-50 * MS)],                           # 7: before the first point
              [0, A(-50 * MS), A(10 * CAD)], [0, first(), A(10 * CAD)],  # 8, 9: from before it / from it
              [0, last(), last(CAD // 2)], [0, last(), last(CAD)], [0, last(), last(5 * CAD)],  # 10-12: past the end
              [0, A(50 * CAD), last(5 * CAD)]]                          # 13: into the flat part
        step = [(5 * CAD + 3 * MS, 15 * CAD + 9 * MS), (25 * CAD + MS, 35 * CAD + 2 * MS), (10 * CAD, 50 * CAD),
                (10 * CAD + MS, 30 * CAD + 5 * MS), (30 * CAD, 55 * CAD + 3 * MS),   # edges at 300 / 1000 W
                (20 * CAD + 2 * MS, 30 * CAD), (20 * CAD + 8 * MS, 23 * CAD + 2 * MS), (10 * CAD, 40 * CAD + 12 * MS),
                (20 * CAD + 4 * MS, 40 * CAD + 8 * MS)]                              # edges in the stepped intervals
        return q + [[1, A(a), A(b)] for a, b in step]
    if name in ("ts_zero", "ts_ticks"):
        return rel_windows((100 * MS, 878 * MS), (300 * MS, 350 * MS), (403 * MS, 408 * MS)) + \
            [[0, first(5 * MS), first(45 * MS)], [0, first(20 * MS), A(500 * MS)]]  # the first 50 ms of the trace
    if name in ("late", "late_before"):
        ts = [400 * MS + i * 1_500_000 + (i * 7919) % 1000 for i in range(201)]  # 400 .. 700 ms, off the grid
        return [[0, A(ts[0]), A(t)] for t in ts] + \
               [[0, A(ts[i]), A(ts[j])] for i in range(0, 200, 8) for j in (i + 3, min(200, i + 40))]
    if name == "fail":
        return rel_windows((250 * MS, 450 * MS), (310 * MS, 390 * MS), (100 * MS, 700 * MS)) + [[1, A(100 * MS), A(700 * MS)]]
    if name == "back":
        return rel_windows((25 * CAD + 3 * MS, 35 * CAD + 5 * MS), (29 * CAD + 2 * MS, 29 * CAD + 10 * MS),
                           (5 * CAD, 28 * CAD + 9 * MS), (31 * CAD + MS, 55 * CAD), (5 * CAD, 55 * CAD))
    if name in ("slots_10", "slots_01"):
        w = (45 * CAD + 3 * MS, 57 * CAD + 9 * MS) if name == "slots_01" else (10 * CAD + 3 * MS, 30 * CAD + 9 * MS)
        return [[0, A(w[0]), A(w[1])], [1, A(w[0]), A(w[1])]]
    if name == "trim":
        return rel_windows((3000 * MS, 3500 * MS), (3000 * MS + 3 * MS, 3900 * MS), (3000 * MS, 3000 * MS + 2 * MS))
    return []


def readings_for(name):
    return {"fail": [(200 * MS, 600 * MS)], "slots_01": [(45 * CAD + 3 * MS, 57 * CAD + 9 * MS)],
            "slow": [(0, 300 * MS)]}.get(name, [])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    from cain_amd.energy import native
    native.load()  # build the sampler once, before the children race for it
    libdir = tmp_path_factory.mktemp("fake_amdsmi")
    b = subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-I/opt/rocm/include", str(FAKE_SRC), "-o",
                        str(libdir / "libamd_smi.so")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    origin = time.clock_gettime_ns(time.CLOCK_MONOTONIC) + 1500 * MS
    procs = {}
    for name, (fenv, cfg) in SCENARIOS.items():
        env = dict(os.environ)
        env["LD_LIBRARY_PATH"] = str(libdir) + os.pathsep + env.get("LD_LIBRARY_PATH", "")
        env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
        env["FAKE_SMI_ORIGIN_NS"] = str(origin)
        env.update({f"FAKE_SMI_{k}": str(v) for k, v in fenv.items()})
        cfg = dict(cfg, start_ns=origin + 5 * MS)

        def absolute(spec):
            return ["abs", origin + spec[1]] if spec[0] == "abs" else spec

        cfg["queries"] = [[s, absolute(a), absolute(b)] for s, a, b in queries_for(name)]
        cfg["readings"] = [[["abs", origin + a], ["abs", origin + b]] for a, b in readings_for(name)]
        if name == "trim":
            cfg["trim"] = [origin + 1000 * MS, origin + 3000 * MS]  # t0 - 2 s as the meter does, then t0 itself
        procs[name] = subprocess.Popen(["timeout", "-k", "5", "30", sys.executable, str(CHILD), json.dumps(cfg)],
                                       env=env, cwd=str(ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out = {"origin": origin}
    for name, p in procs.items():
        so, se = p.communicate(timeout=60)
        assert p.returncode == 0, f"{name}: exit {p.returncode}\n{se[-3000:]}"
        out[name] = json.loads(so.strip().splitlines()[-1])
        assert out[name]["created_ns"] < origin + 60 * MS, f"{name}: child started late"
    return out


# ------------------------------------------------------------------ helpers on a returned trace
def rel_trace(run, origin, slot=0):
    """[(host, dev, used, joules)] with host and used relative to the origin (ns)."""
    return [(h - origin, d, u - origin, num(j)) for h, d, u, j in run["traces"][slot]]


def mapped_delta(tr, origin):
    """delta of a fully mapped trace: used - tq, the same for every point (tq from the device timestamp)."""
    ds = [u - (d + TS_OFFSET - origin) for _, d, u, _ in tr]
    assert max(ds) - min(ds) <= 1, ("points are not all at their mapped time", min(ds), max(ds))
    assert 0 <= ds[0] < 2 * MS, ds[0]
    return ds[0]


def got(run, i, origin):
    slot, a, b, e = run["queries"][i]
    return slot, a - origin, b - origin, num(e)


def bracket_delay(tr, tq, t):
    """Largest observation delay (used - tq) of the two trace points around time t."""
    us = [p[2] for p in tr]
    hi = next((k for k, u in enumerate(us) if u > t), len(us) - 1)
    lo = max(0, hi - 1)
    return max(us[lo] - tq[lo], us[hi] - tq[hi])


def grid_times(tr, watts):
    """Update time tq of every point of a constant-power trace: the first from its observation time, the others
    from their exact energy (robust against an update landing between the read and its stamp)."""
    n0 = tr[0][0] // CAD
    return [(n0 + round(j / (watts * CAD * 1e-9))) * CAD for _, _, _, j in tr]


# ------------------------------------------------------------------ constant power, device timestamps on
def test_constant_power_windows_are_exact(runs):
    o, run = runs["origin"], runs["base"]
    tr = rel_trace(run, o)
    delta = mapped_delta(tr, o)
    print(f"constant 650 W: {len(tr)} points, mapping bias delta = {delta} ns")
    assert tr[0][2] < 40 * MS and tr[-1][2] > 900 * MS and len(tr) > 50
    for i in range(6):
        _, a, b, e = got(run, i, o)
        want = truth_j([(0, 650)], a, b)
        print(f"  [{a / MS:.3f}, {b / MS:.3f}] ms: got {e:.9f} J, exact {want:.9f} J, err {e - want:+.3e}")
        assert abs(e - want) <= quant(want), (a, b, e, want)
    _, a, b, e = got(run, 6, o)  # whole run: first to last point, both on the (shifted) grid
    want = truth_j([(0, 650)], a, b)
    print(f"  whole run {(b - a) / MS:.1f} ms: got {e:.6f} J, exact {want:.6f} J, err {e - want:+.3e}")
    assert abs(e - want) <= quant(want)


def test_before_the_first_point_reads_zero(runs):
    o, run = runs["origin"], runs["base"]
    assert got(run, 7, o)[3] == 0.0
    assert got(run, 8, o)[3] == got(run, 9, o)[3] > 0


def test_extrapolation_is_exact_for_one_interval_then_flat(runs):
    o, run = runs["origin"], runs["base"]
    tr = rel_trace(run, o)
    span = tr[-1][2] - tr[-2][2]  # the last segment: one cadence unless an update was missed
    assert span % CAD == 0 and span <= 2 * CAD
    half, one, five = (got(run, i, o)[3] for i in (10, 11, 12))
    print(f"past the end: +CAD/2 {half:.6f} J, +CAD {one:.6f} J, +5 CAD {five:.6f} J, last segment {span / MS} ms")
    assert abs(half - 650 * (CAD // 2) * 1e-9) <= quant(half)
    assert abs(one - 650 * CAD * 1e-9) <= quant(one)
    assert abs(five - 650 * span * 1e-9) <= quant(five)  # flat after one segment's length, not 5 x
    _, a, b, e = got(run, 13, o)
    assert abs(e - (truth_j([(0, 650)], a, tr[-1][2]) + 650 * span * 1e-9)) <= quant(e)


# ------------------------------------------------------------------ step power
def test_step_power_windows(runs):
    o, run = runs["origin"], runs["base"]
    tr = rel_trace(run, o, 1)
    delta = mapped_delta(tr, o)
    assert delta < MS
    dp = 700
    print(f"step 300/1000/300 W: mapping bias delta = {delta} ns -> shift term {dp * delta * 1e-9:.3e} J")
    stepped = (T1 // CAD, T2 // CAD)
    for i in range(14, 23):
        _, a, b, e = got(run, i, o)
        want = truth_j(STEP, a, b)
        # the sampler's axis runs delta late: an edge t sits in update interval floor((t - delta) / CAD)
        in_step = [((t - delta) // CAD) in stepped for t in (a, b)]
        bound = quant(want) + abs(power_at(STEP, b) - power_at(STEP, a)) * delta * 1e-9
        bound += sum(in_step) * (dp * CAD * 1e-9 / 4 + dp * delta * 1e-9)
        print(f"  [{a / MS:.1f}, {b / MS:.1f}] ms edges in a stepped interval {in_step}: got {e:.6f} J, exact {want:.6f} J, "
              f"err {e - want:+.3e}, bound {bound:.3e}")
        assert in_step == ([False, False] if i < 19 else [i != 21, i != 19 and i != 20]), (i, in_step)
        assert abs(e - want) <= bound, (a, b, e, want, bound)


# ------------------------------------------------------------------ no usable device timestamps
def _observation_time_windows(run, o, label):
    tr = rel_trace(run, o)
    assert all(abs(u - h) <= 0.5 for h, _, u, _ in tr), "points must sit at their observation times"
    tq = grid_times(tr, 800)
    delays = [h - t for (h, _, _, _), t in zip(tr, tq)]
    assert min(delays) >= 0
    print(f"{label}: observation delay of {len(tr)} points: min {min(delays) / 1e3:.1f} us, "
          f"median {sorted(delays)[len(delays) // 2] / 1e3:.1f} us, max {max(delays) / 1e3:.1f} us")
    errs = []
    for i in range(len(run["queries"])):
        _, a, b, e = got(run, i, o)
        want = truth_j([(0, 800)], a, b)
        d = max(bracket_delay(tr, tq, a), bracket_delay(tr, tq, b))
        bound = 800 * d * 1e-9 + quant(want)
        print(f"  [{a / MS:.1f}, {b / MS:.1f}] ms: err {e - want:+.4f} J, d = {d / 1e3:.1f} us, bound {bound:.4f} J")
        assert abs(e - want) <= bound, (a, b, e, want, bound)
        errs.append(abs(e - want))
    return errs


def test_without_device_timestamps_error_is_the_poll_delay(runs):
    _observation_time_windows(runs["ts_zero"], runs["origin"], "ts = 0")


def test_timestamp_in_another_unit_is_no_worse_than_none(runs):
    _observation_time_windows(runs["ts_ticks"], runs["origin"], "ts in 10 ns ticks")


# ------------------------------------------------------------------ late observation
def _late_checks(run, o, expect_late):
    tr = rel_trace(run, o)
    late = [(k, h - u) for k, (h, _, u, _) in enumerate(tr) if h - u >= 50 * MS]
    gaps = [tr[k + 1][2] - tr[k][2] for k in range(len(tr) - 1)]
    print(f"points observed >= 50 ms after the time they are used at: {late}; largest gap {max(gaps) / MS:.1f} ms")
    assert max(gaps) >= 80 * MS  # the blocked call did happen
    if expect_late:
        assert len(late) == 1 and abs(tr[late[0][0]][2] - LATE_T) < 2 * MS
    us = [p[2] for p in tr]
    assert us == sorted(us)
    q = [got(run, i, o) for i in range(len(run["queries"]))]
    cum = [e for _, _, _, e in q[:201]]
    assert all(y >= x for x, y in zip(cum, cum[1:])), "cumulative energy must not decrease"
    table = {(a, b): e for _, a, b, e in q}
    a0 = q[0][1]
    worst = 0.0
    for _, a, b, e in q[201:]:
        add = table[(a0, b)] - table[(a0, a)]
        worst = max(worst, abs(add - e))
        assert abs(add - e) <= 1e-9 * max(1.0, table[(a0, b)]), (a, b, e, add)
    hole = (tr[[g >= 80 * MS for g in gaps].index(True)][2], tr[[g >= 80 * MS for g in gaps].index(True) + 1][2])
    worst_err = 0.0
    for _, a, b, e in q:
        want = truth_j([(0, 700)], a, b)
        touches = a <= hole[1] and b >= hole[0]
        worst_err = max(worst_err, abs(e - want))
        assert abs(e - want) <= quant(want) + (700 * CAD * 1e-9 if touches else 0.0), (a, b, e, want)
    print(f"additivity worst {worst:.2e} J; worst window error {worst_err:.3e} J over {len(q)} windows")


def test_a_point_observed_late_keeps_windows_monotone_and_additive(runs):
    _late_checks(runs["late"], runs["origin"], True)


def test_a_read_that_blocks_before_reading_does_not_spoil_the_mapping(runs):
    o, run = runs["origin"], runs["late_before"]
    mapped_delta(rel_trace(run, o), o)  # every point still at its mapped time
    _late_checks(run, o, False)


# ------------------------------------------------------------------ read failures
def test_reads_that_fail_for_a_while_lose_nothing(runs):
    o, run = runs["origin"], runs["fail"]
    tr = rel_trace(run, o)
    assert max(tr[k + 1][2] - tr[k][2] for k in range(len(tr) - 1)) >= 100 * MS
    for i in range(3):
        _, a, b, e = got(run, i, o)
        want = truth_j([(0, 500)], a, b)
        print(f"  [{a / MS:.0f}, {b / MS:.0f}] ms across failed reads: err {e - want:+.3e} J")
        assert abs(e - want) <= quant(want)


def test_a_gpu_that_never_reads_makes_the_sum_nan(runs):
    run = runs["fail"]
    assert run["tracked"] == 2 and run["traces"][1] == []
    assert math.isnan(got(run, 3, runs["origin"])[3])
    r = run["readings"][0]
    assert abs(r["per_gpu_energy_j"][0] - 500 * 0.4) <= quant(200)
    assert math.isnan(num(r["per_gpu_energy_j"][1]))
    for key in ("gpu_energy_j", "total_energy_j", "gpu_power_w"):
        assert math.isnan(num(r[key])), (key, r[key])
    none = run["readings_none"]
    assert none["gpu_energy_j"] == 0.0 and none["per_gpu_energy_j"] == [] and none["total_energy_j"] == 0.0


# ------------------------------------------------------------------ backwards accumulator step
def test_backwards_step_loses_at_most_its_own_interval(runs):
    o, run = runs["origin"], runs["back"]
    one = 600 * CAD * 1e-9
    for i, crosses in enumerate([True, True, False, False, True]):
        _, a, b, e = got(run, i, o)
        want = truth_j([(0, 600)], a, b)
        print(f"  [{a / MS:.0f}, {b / MS:.0f}] ms crosses the step: {crosses}; got {e:.6f} J, exact {want:.6f} J, lost {want - e:.6f}")
        assert e >= 0
        assert e <= want + quant(want)
        assert want - e <= (one if crosses else 0.0) + quant(want)
    assert abs((truth_j([(0, 600)], 5 * CAD, 55 * CAD) - got(run, 4, o)[3]) - one) <= quant(one)  # exactly one interval


# ------------------------------------------------------------------ slots and enumeration
def test_slots_follow_smi_indices(runs):
    o = runs["origin"]
    for name, order in (("slots_10", [1, 0]), ("slots_01", [0, 1])):
        run = runs[name]
        assert run["es_gpu_count"] == 2 and run["gpu_count"] == 2 and run["tracked"] == 2
        assert run["bdfs"] == ["0000:10:00.0", "0000:11:00.0"]
        for slot, g in enumerate(order):
            _, a, b, e = got(run, slot, o)
            want = (b - a) * 1e-9 * (300 if g == 0 else 900)
            print(f"  {name} slot {slot} = GPU {g}: got {e:.6f} J, exact {want:.6f} J")
            assert abs(e - want) <= quant(want), (name, slot, e, want)


def test_meter_sums_slots_and_subtracts_idle(runs):
    run = runs["slots_01"]
    r = run["readings"][0]
    dur = r["duration_s"]
    idle = run["idle_w"]
    tol_w = 2 * 2 * 4 * RES_J / 0.4 + 1e-9 * 600  # two GPUs, two edges each, over >= 0.4 s
    print(f"idle {idle:.6f} W (300 + 300), window {dur * 1e3:.1f} ms: {r['gpu_energy_j']:.6f} J, {r['gpu_power_w']:.6f} W, "
          f"idle-subtracted {r['idle_subtracted_j']:.6f} J")
    assert abs(idle - 600) <= tol_w
    assert r["per_gpu_energy_j"][0] == pytest.approx(300 * dur, abs=quant(300 * dur))
    assert r["per_gpu_energy_j"][1] == pytest.approx(900 * dur, abs=quant(900 * dur))
    assert r["gpu_energy_j"] == sum(r["per_gpu_energy_j"]) == r["total_energy_j"]
    assert r["gpu_power_w"] == pytest.approx(1200, abs=2 * quant(1200 * dur) / dur)
    assert r["idle_power_w"] == idle
    assert r["idle_subtracted_j"] == pytest.approx(r["gpu_energy_j"] - idle * dur, abs=1e-9)
    assert r["idle_subtracted_j"] == pytest.approx(600 * dur, abs=2 * quant(1200 * dur) + tol_w * dur)


# ------------------------------------------------------------------ slow samples
def test_slow_sample_fallbacks(runs):
    r = runs["slow"]["readings"][0]
    by_gpu = {g: [s for s in r["samples"] if s["gpu"] == g] for g in range(3)}
    assert all(len(v) >= 5 for v in by_gpu.values())
    assert {s["power_w"] for s in by_gpu[0]} == {432.0}  # current_socket_power valid
    assert {s["power_w"] for s in by_gpu[1]} == {555.0}  # UINT32_MAX -> socket_power
    assert {s["power_w"] for s in by_gpu[2]} == {444.0}  # 0 -> socket_power
    assert {s["gfx_pct"] for s in by_gpu[0]} == {40.0} and {s["gfx_pct"] for s in by_gpu[2]} == {60.0}
    assert all(math.isnan(num(s["gfx_pct"])) and math.isnan(num(s["umc_pct"])) for s in by_gpu[1])
    assert {s["vram_pct"] for s in by_gpu[0]} == {25.0} and {s["vram_pct"] for s in by_gpu[2]} == {75.0}
    assert all(math.isnan(num(s["vram_pct"])) for s in by_gpu[1])  # total = 0
    n0, n2 = len(by_gpu[0]), len(by_gpu[2])
    assert r["gpu_usage"] == pytest.approx((40 * n0 + 60 * n2) / (n0 + n2))  # the NaN rows are left out
    assert r["vram_usage"] == pytest.approx((25 * n0 + 75 * n2) / (n0 + n2))


# ------------------------------------------------------------------ trim
def test_trim_keeps_later_windows_bit_for_bit(runs):
    o, run = runs["origin"], runs["trim"]
    n0 = len(run["traces"][0])
    window = run["stopped_ns"] - (o + 3000 * MS)
    for kept, after in zip((2000 * MS, 0), run["after_trim"]):  # trim(t0 - 2 s), then trim(t0): one point before t stays
        for (_, a, b, e0), (_, _, _, e1) in zip(run["queries"], after["queries"]):
            want = truth_j([(0, 400)], a - o, b - o)
            assert struct.pack("d", num(e0)) == struct.pack("d", num(e1)), (kept, e0, e1)
            assert abs(num(e0) - want) <= quant(want)
        n1 = after["points"][0]
        print(f"trim(t0 - {kept / MS:.0f} ms): {n0} -> {n1} points, window {window / MS:.0f} ms")
        assert n1 <= (kept + window) / CAD + 2
        assert n1 >= window / CAD - 2
