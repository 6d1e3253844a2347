"""Child process of tests/test_energy_trace.py: runs one EnergyMeter against the scripted amd-smi stand-in
(tests/csrc/fake_amdsmi.cpp, found through LD_LIBRARY_PATH) and prints what it saw as one JSON line.

argv[1] is a JSON config:
  smi          amd-smi indices to track, in slot order
  start_ns     absolute CLOCK_MONOTONIC time to create the meter at
  run_ms       how long the sampler runs
  period_ms    slow-sample period
  idle_s       > 0: measure_idle(idle_s) first
  queries      [[slot, A, B], ...]; A and B are ["abs", ns], or ["first", d] / ["last", d]: d ns after the time the
               slot's first / last trace point is used at
  readings     [[A, B], ...] for reading_between (slot 0's trace resolves "first" / "last")
  trim         list of absolute ns: after the queries, trim(before) for each in turn and evaluate them again
"""
import json
import math
import sys
import time

from cain_amd.energy import EnergyMeter, native


def _clean(x):
    if isinstance(x, float) and not math.isfinite(x):
        return "nan" if math.isnan(x) else ("inf" if x > 0 else "-inf")
    if isinstance(x, dict):
        return {k: _clean(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_clean(v) for v in x]
    return x


def main():
    cfg = json.loads(sys.argv[1])
    lib = native.load()
    n_gpus = native.init()
    while native.now_ns() < cfg["start_ns"]:
        time.sleep(0.001)
    m = EnergyMeter(smi_indices=cfg["smi"], period_ms=cfg.get("period_ms", 100.0), fast_period_ms=1.0,
                    sources=("gpu",), cpu_tdp_w=100.0)
    none = EnergyMeter(smi_indices=[], period_ms=100.0, sources=("gpu",), cpu_tdp_w=100.0)
    out = {"gpu_count": n_gpus, "es_gpu_count": int(lib.es_gpu_count()), "tracked": m.n_gpus, "bdfs": native.gpu_bdfs(),
           "created_ns": native.now_ns()}
    if cfg.get("idle_s", 0) > 0:
        out["idle_w"] = m.measure_idle(cfg["idle_s"])
    time.sleep(cfg["run_ms"] / 1000.0)
    m.sampler.stop()
    none.sampler.stop()
    out["stopped_ns"] = native.now_ns()
    traces = [m.sampler.trace_ex(i) for i in range(m.n_gpus)]
    out["traces"] = traces

    def at(slot, spec):
        kind, v = spec
        if kind == "abs":
            return int(v)
        tr = traces[slot]
        return int(round(tr[0][2] if kind == "first" else tr[-1][2])) + int(v)

    def run_queries():
        res = []
        for slot, a, b in cfg.get("queries", []):
            ta, tb = at(slot, a), at(slot, b)
            res.append([slot, ta, tb, m.sampler.energy_between(slot, ta, tb)])
        return res

    out["queries"] = run_queries()
    out["readings"] = []
    for a, b in cfg.get("readings", []):
        ta, tb = at(0, a), at(0, b)
        out["readings"].append(m.reading_between(ta, tb).as_dict(with_samples=True))
        out["readings_none"] = none.reading_between(ta, tb).as_dict()
    out["after_trim"] = []
    for before in cfg.get("trim", []):
        m.sampler.trim(int(before))
        out["after_trim"].append({"queries": run_queries(), "points": [m.sampler.trace_points(i) for i in range(m.n_gpus)]})
    m.close()
    none.close()
    print(json.dumps(_clean(out)))


if __name__ == "__main__":
    main()
