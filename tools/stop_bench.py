#!/usr/bin/env python3
"""Stop sequences' cost: decode tok/s of the same seeded requests without ``stop`` and with eight stop strings that
never occur, interleaved, per batch on MXFP4 weights.  One JSON line per cell
(profiles/r17/stop_sequences/README.md).

    python tools/stop_bench.py [--reps 3] [--tokens 256] [--modes off,stop] [--models a,b] [--batches 1,256]

The strings hold bytes the synthetic tokenizer's pieces never spell, so every row runs its whole budget: both modes
time the same number of decode steps.  CAIN_KERNELS_LIB=... runs another build of the kernel library
(tools/ab_lib.py) for the comparison with the parent commit (``--modes off``: the parent has no stop entry)."""
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

# what chat front ends send, plus strings whose last bytes the synthetic pieces do spell (the compare runs from the
# newest byte back, so these cost more than a first-byte mismatch), one of them 32 bytes long
STOPS = ["\n\n", "###", "User:", "</s>", "Observation:", "Qu" + "zu" * 15, "Xtuzu", "X vizudo"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--models", default="llama3.1:8b")
    ap.add_argument("--batches", default="1,256")
    ap.add_argument("--modes", default="off,stop")
    ns = ap.parse_args()
    for name in ns.models.split(","):
        for B in [int(x) for x in ns.batches.split(",")]:
            eng = DecodeEngine(name, device="cuda", max_batch=B, max_context=512, seed=1, weight_dtype="fp4")
            prompts = [np.random.default_rng(i).integers(16, 1000, size=12).tolist() for i in range(B)]
            res = {m: [] for m in ns.modes.split(",")}
            ngen = {}
            for rep in range(ns.reps + 1):
                for m in res:  # interleaved
                    opts = [dict(seed=100 + i, eos_id=-1, **({"stop": STOPS} if m == "stop" else {})) for i in range(B)]
                    r = eng.generate(prompts, ns.tokens, opts)
                    ngen[m] = sum(len(x.tokens) for x in r)
                    assert all(x.done_reason == "length" for x in r)
                    if rep:
                        res[m].append(ngen[m] / (eng.last_decode_ns * 1e-9))
            print(json.dumps(dict(model=name, batch=B, lib=os.path.basename(os.environ.get("CAIN_KERNELS_LIB", "this")),
                                  tokens=ngen, tok_per_s={m: [round(v, 1) for v in vs] for m, vs in res.items()},
                                  median={m: round(statistics.median(vs), 1) for m, vs in res.items()})), flush=True)
            eng.close()
            del eng
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
