"""``python -m cain_amd perplexity``: the perplexity of a text under a model, on any weight / KV format.

The text is tokenised and cut into non-overlapping windows of ``ctx`` tokens (a last window of at least two tokens is
kept); every token after the first of each window is scored by ``DecodeEngine.score`` (teacher forcing: the natural-log
softmax of the model's own logits at the position before it).  Prints one JSON line:
``model, weights, kv, ctx, windows, tokens_scored, nll_mean, ppl, tok_per_s``.
"""
from __future__ import annotations

import argparse
import json
import math
import time
from typing import List, Optional, Sequence


def windows(ids: Sequence[int], ctx: int) -> List[List[int]]:
    """Non-overlapping windows of ``ctx`` tokens; a remainder of fewer than two tokens scores nothing and is dropped."""
    out = [list(ids[i:i + ctx]) for i in range(0, len(ids), ctx)]
    return [w for w in out if len(w) >= 2]


def perplexity(eng, ids: Sequence[int], ctx: Optional[int] = None, batch: Optional[int] = None) -> dict:
    """Mean negative log-likelihood and perplexity of ``ids`` under ``eng``, ``batch`` windows per ``score`` call."""
    ctx = int(ctx or min(512, eng.T_max))
    if not 2 <= ctx <= eng.T_max:
        raise ValueError(f"ctx must be in 2..{eng.T_max}, got {ctx}")
    wins = windows(ids, ctx)
    if not wins:
        raise ValueError("the text has fewer than two tokens: nothing to score")
    batch = max(1, int(batch or eng.max_batch))
    nll, n = 0.0, 0
    t0 = time.perf_counter()
    for i in range(0, len(wins), batch):
        for r in eng.score(wins[i:i + batch]):
            nll -= math.fsum(r.logprobs)
            n += len(r.logprobs)
    dt = time.perf_counter() - t0
    mean = nll / n
    return {"ctx": ctx, "windows": len(wins), "tokens_scored": n, "nll_mean": mean, "ppl": math.exp(mean),
            "tok_per_s": n / dt if dt > 0 else 0.0}


def main(argv: Optional[List[str]] = None) -> None:
    from ..models.weights import WEIGHT_DTYPES
    from ..serve.server import register_checkpoints
    from .engine import DecodeEngine

    ap = argparse.ArgumentParser(prog="python -m cain_amd perplexity")
    ap.add_argument("--model", required=True, metavar="TAG")
    ap.add_argument("--checkpoint", metavar="PATH", help="a Hugging Face checkpoint directory or GGUF file, as --model")
    ap.add_argument("--weights", choices=list(WEIGHT_DTYPES), default="bf16")
    ap.add_argument("--kv", choices=["bf16", "fp8"], default="bf16")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--file", metavar="PATH", help="UTF-8 text to score")
    src.add_argument("--prompt", metavar="TEXT")
    ap.add_argument("--ctx", type=int, default=None, help="window length in tokens (default min(512, context))")
    ap.add_argument("--batch", type=int, default=8, help="windows scored per call")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--backend", choices=["hip", "torch"], default=None)
    ap.add_argument("--max-context", type=int, default=2048)
    ns = ap.parse_args(argv)
    if ns.checkpoint:
        register_checkpoints([f"{ns.model}={ns.checkpoint}"])
    if ns.file:
        with open(ns.file, encoding="utf-8") as f:
            text = f.read()
    else:
        text = ns.prompt
    eng = DecodeEngine(ns.model, device=ns.device, max_batch=ns.batch, max_context=ns.max_context,
                       weight_dtype=ns.weights, kv_dtype=ns.kv, backend=ns.backend)
    try:
        res = perplexity(eng, eng.encode(text), ns.ctx, ns.batch)
    finally:
        eng.close()
    print(json.dumps({"model": ns.model, "weights": ns.weights, "kv": ns.kv, **res}))
