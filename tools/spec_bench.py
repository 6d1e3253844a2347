#!/usr/bin/env python
"""Cost and payoff of speculative decoding at batch 1, graph-replayed (profiles/r13/speculative/README.md).

Per model and weight format, on one GPU:

1. ``step``: us per decode step of the plain graph (K = 0) and of the speculative graph at K = 1, 3, 7 with drafts
   that are never accepted (every step verifies K + 1 rows and commits one token).  The ratio to K = 0 is the number of
   tokens a step has to commit to break even.
2. ``rate``: tok/s and board J/token in given mode at controlled acceptance rates: the tokens the speculative engine
   itself emits as drafts, corrupted at a fixed stride.  Plain decode is measured interleaved with every
   configuration; medians.  ``plain_prefix``: how many leading tokens equal the plain engine's (a K + 1-row forward
   rounds differently from a 1-row one; a deep random-init stack parts at the first near-tie).
3. ``ngram``: the n-gram mode's acceptance on the model's own greedy decode (random-init weights: not natural text).
4. ``draft`` (``--draft-model TAG``, instead of 1 - 3; profiles/r16/draft_model/README.md): ms per plain, n-gram and
   draft-model step at K = ``--rate-k``, the break-even tokens per step and the measured ones.

One JSON line per measurement on stdout (and in ``--out``).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

PROMPT = "In 500 words, please give me information about Elizabeth II, Queen of the United Kingdom"
GREEDY = dict(temperature=0.0, repeat_penalty=1.0, eos_id=-1)
RATES = {0: (), 25: (0,), 50: (0, 2), 75: (0, 1, 2), 100: (0, 1, 2, 3)}  # of 4 consecutive indices: the right drafts


def drafts_at(tokens, rate: int, vocab: int):
    keep = RATES[rate]
    return [t if i % 4 in keep else (t + 1) % vocab for i, t in enumerate(tokens)]


def common(a, b) -> int:
    """Length of the common prefix of two token lists."""
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


def draft_model_bench(model, draft, wd, k, n, repeats, run, emit) -> None:
    """``kind="draft"``: ms per plain step, per n-gram speculative step and per draft-model step (interleaved,
    medians), the tokens a draft-model step has to commit to break even with plain decoding, and the tokens it did
    commit on the model's own greedy decode (random-init weights: not natural text)."""
    import torch

    from cain_amd.engine import DecodeEngine
    from cain_amd.models import get_config, random_weights

    w = random_weights(get_config(model), device=torch.device("cuda"), seed=0)
    kw = dict(device="cuda", max_batch=1, max_context=1024, weights=w, weight_dtype=wd, keep_natural=True,
              steps_per_graph=8)
    engines = dict(plain=DecodeEngine(model, **kw), ngram=DecodeEngine(model, speculative=k, **kw),
                   draft=DecodeEngine(model, speculative=k, draft_model=w if draft == "self" else draft, **kw))
    for e in engines.values():  # warm: graphs captured
        run(e, n)
    ms = {name: [] for name in engines}
    last = {}
    for _ in range(repeats):
        for name, e in engines.items():
            r, t, _ = run(e, n)
            ms[name].append(t * 1e3 / (r.decode_steps or n))
            last[name] = r
    med = {name: statistics.median(v) for name, v in ms.items()}
    r = last["draft"]
    emit(kind="draft", model=model, draft=draft, weights=wd, K=k, plain_ms_per_step=round(med["plain"], 4),
         ngram_ms_per_step=round(med["ngram"], 4), draft_ms_per_step=round(med["draft"], 4),
         break_even_tokens_per_step=round(med["draft"] / med["plain"], 3),
         tokens_per_step=round(r.eval_count / max(1, r.decode_steps), 3),
         ngram_tokens_per_step=round(last["ngram"].eval_count / max(1, last["ngram"].decode_steps), 3),
         drafted=r.draft_count, accepted=r.draft_accepted,
         same_tokens_as_ngram_engine=r.tokens == last["ngram"].tokens,
         note="random-init weights: acceptance is not representative of natural text")
    for e in engines.values():
        e.close()
    del engines, w
    torch.cuda.empty_cache()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="llama3.1:8b,qwen2:1.5b")
    ap.add_argument("--weights", default="fp4,q4_k_m")
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ks", default="1,3,7")
    ap.add_argument("--rate-k", type=int, default=3, help="K of the acceptance-rate sweep")
    ap.add_argument("--draft-model", default=None, metavar="TAG",
                    help="measure draft-model mode instead (K = --rate-k): TAG drafts for each of --models; 'self': "
                         "the target's own weights, which accepts everything up to rounding (the upper bound)")
    ap.add_argument("--no-energy", action="store_true")
    ap.add_argument("--out", default=None)
    ns = ap.parse_args(argv)

    import torch

    from cain_amd.engine import DecodeEngine
    from cain_amd.models import get_config, random_weights

    meter = None
    if not ns.no_energy:
        try:
            from cain_amd.energy import EnergyMeter

            meter = EnergyMeter(devices=[0], period_ms=50.0, keep_samples=False, sources=("gpu",))
        except Exception as exc:  # noqa: BLE001 - energy is auxiliary
            print(f"[spec_bench] energy meter unavailable: {exc}", file=sys.stderr)
    sink = open(ns.out, "a") if ns.out else None

    def emit(**kw) -> None:
        line = json.dumps(kw)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def run(eng, n, drafts=None):
        """(result, decode seconds, board joules or None) of one generation."""
        if meter:
            meter.start()
        r = eng.generate([PROMPT], n, [GREEDY], drafts=drafts)[0]
        rd = meter.stop() if meter else None
        return r, eng.last_decode_ns * 1e-9, (rd.gpu_energy_j if rd is not None else None)

    n, ks = ns.tokens, [int(k) for k in ns.ks.split(",")]
    if ns.draft_model:
        for model in ns.models.split(","):
            for wd in ns.weights.split(","):
                draft_model_bench(model, ns.draft_model, wd, ns.rate_k, n, ns.repeats, run, emit)
        return 0
    for model in ns.models.split(","):
        for wd in ns.weights.split(","):
            cfg = get_config(model)
            w = random_weights(cfg, device=torch.device("cuda"), seed=0)
            kw = dict(device="cuda", max_batch=1, max_context=1024, weights=w, weight_dtype=wd, keep_natural=True,
                      steps_per_graph=8)
            plain = DecodeEngine(model, **kw)
            base = run(plain, n)[0]
            run(plain, n)  # warm: graphs captured
            # A K + 1-row forward rounds differently from a 1-row one, and a deep random-init stack turns that into
            # other greedy tokens at near-ties: each K's drafts come from its own engine's trajectory (the forward
            # always has K + 1 rows, so the trajectory does not depend on the drafts), not from the plain run's.
            specs, own = {}, {}
            for k in sorted(set(ks + [ns.rate_k])):
                specs[k] = DecodeEngine(model, speculative=k, **kw)
                own[k] = run(specs[k], n, [None])[0].tokens
                run(specs[k], n, [drafts_at(own[k], 0, cfg.vocab)])
            # 1. step cost, no draft accepted; plain interleaved
            t_plain, t_spec = [], {k: [] for k in ks}
            for _ in range(ns.repeats):
                t_plain.append(run(plain, n)[1] / n)
                for k in ks:
                    r, t, _ = run(specs[k], n, [drafts_at(own[k], 0, cfg.vocab)])
                    t_spec[k].append(t / r.decode_steps)
            us0 = statistics.median(t_plain) * 1e6
            emit(kind="step", model=model, weights=wd, K=0, us_per_step=round(us0, 1), break_even=1.0)
            for k in ks:
                us = statistics.median(t_spec[k]) * 1e6
                emit(kind="step", model=model, weights=wd, K=k, us_per_step=round(us, 1), break_even=round(us / us0, 3))
            # 2. acceptance-rate sweep in given mode
            k = ns.rate_k
            for rate in sorted(RATES):
                tp, ts, jp, js, steps, same = [], [], [], [], 0, True
                for _ in range(ns.repeats):
                    r0, t0, e0 = run(plain, n)
                    r1, t1, e1 = run(specs[k], n, [drafts_at(own[k], rate, cfg.vocab)])
                    tp.append(n / t0), ts.append(r1.eval_count / t1)
                    if e0 is not None and e1 is not None:
                        jp.append(e0 / n), js.append(e1 / r1.eval_count)
                    steps, same = r1.decode_steps, same and r1.tokens == own[k]
                emit(kind="rate", model=model, weights=wd, K=k, drafts_right_pct=rate,
                     tokens_per_step=round(n / max(1, steps), 3), same_tokens_as_undrafted=same,
                     plain_prefix=common(own[k], base.tokens),
                     plain_tok_s=round(statistics.median(tp), 1), spec_tok_s=round(statistics.median(ts), 1),
                     speedup=round(statistics.median(ts) / statistics.median(tp), 3),
                     plain_j_per_token=round(statistics.median(jp), 4) if jp else None,
                     spec_j_per_token=round(statistics.median(js), 4) if js else None)
            # 3. n-gram mode on the model's own greedy decode
            for k in ks:
                r, t, _ = run(specs[k], n)
                emit(kind="ngram", model=model, weights=wd, K=k, drafted=r.draft_count, accepted=r.draft_accepted,
                     steps=r.decode_steps, tokens=r.eval_count, tok_s=round(r.eval_count / t, 1),
                     same_tokens_as_undrafted=r.tokens == own[k], plain_prefix=common(r.tokens, base.tokens),
                     note="random-init weights: not representative of natural text")
            plain.close()
            for e in specs.values():
                e.close()
            del plain, specs, w
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
