#!/usr/bin/env python3
"""JSON mode's cost: decode tok/s of the same seeded requests with ``format`` off and ``"json"``, interleaved, per model
and batch on MXFP4 weights.  One JSON line per cell (profiles/r15/json_mode/README.md).

    python tools/json_bench.py [--reps 3] [--tokens 256] [--modes off,json] [--models a,b] [--batches 1,16]

The vocabulary has no piece with a closing brace, so a JSON row's top-level object never closes and every row runs
its whole budget: both modes time the same number of decode steps.  CAIN_KERNELS_LIB=ab/... runs another build of
the kernel library (tools/ab_lib.py) for the format-off comparison with the parent commit."""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from cain_amd.engine.engine import DecodeEngine  # noqa: E402


def vocab(V):
    # single bytes without '}' (the top-level object can then never close: every row runs its whole budget),
    # then fragments; passes the vocabulary check (liveness, not closability)
    rng = np.random.default_rng(0)
    frag = [b'{"', b'":', b'", "', b'":"', b'": ', b'","', b'[]', b'true', b'false', b'null', b' 12', b'\n  ', b', ',
            b'\\n', b'\\u00', b'name', b'"id":', b'\xc3\xa9', b'\xe2\x82', b'\xac', b'0.5', b'e+', b'[1,2]']
    out = [b""] * 16 + [bytes([b]) for b in range(256) if b != ord("}")]
    words = "abcdefghijklmnopqrstuvwxyz"
    while len(out) < V:
        if len(out) - 271 < len(frag):
            out.append(frag[len(out) - 271])
            continue
        n = int(rng.integers(2, 7))
        w = "".join(words[i] for i in rng.integers(0, 26, n)).encode()
        out.append([b" " + w, w, b'"' + w, w + b'"', w + b'":', str(int(rng.integers(10, 99999))).encode()][int(rng.integers(0, 6))])
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--models", default="llama3.1:8b,gemma:2b")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--modes", default="off,json")
    ns = ap.parse_args()
    for name in ns.models.split(","):
        for B in [int(x) for x in ns.batches.split(",")]:
            eng = DecodeEngine(name, device="cuda", max_batch=B, max_context=512, seed=1, weight_dtype="fp4")
            eng.set_json_vocab(vocab(eng.cfg.vocab))
            prompts = [np.random.default_rng(i).integers(16, 1000, size=12).tolist() for i in range(B)]
            opts = [dict(seed=100 + i, eos_id=-1) for i in range(B)]
            res = {m: [] for m in ns.modes.split(",")}
            ngen = {}
            for rep in range(ns.reps + 1):
                for m in res:  # interleaved
                    r = eng.generate(prompts, ns.tokens, opts, format="json" if m == "json" else None)
                    ngen[m] = sum(len(x.tokens) for x in r)
                    if rep:
                        res[m].append(ngen[m] / (eng.last_decode_ns * 1e-9))
            print(json.dumps(dict(model=name, batch=B, lib=os.path.basename(os.environ.get("CAIN_KERNELS_LIB", "this")), tokens=ngen,
                                  tok_per_s={m: [round(v, 1) for v in vs] for m, vs in res.items()},
                                  median={m: round(statistics.median(vs), 1) for m, vs in res.items()})), flush=True)
            eng.close()
            del eng
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
