"""Autoregressive decode engine (the on-device arm's LLM; replaces Ollama/llama.cpp).

Reference: the reference never runs a model itself — it POSTs to an external
Ollama server (experiment/RunnerConfig.py:122-131).  SURVEY §2.3 row 1 and
§3.4 specify what replaces it: tokenize, prefill, autoregressive decode with a
KV cache and Ollama's sampling, returning Ollama's statistics
(``prompt_eval_count``, ``eval_count``, ``*_duration`` in ns).

Backends
--------
``hip``    the MI355X path: packed bf16 weights resident in HBM, the hand-written
           gfx950 kernels of ``cain_amd.ops`` sequenced by the native runtime
           (``csrc/runtime.hip``) and replayed from hipGraphs — ``steps_per_graph``
           decode steps per graph launch, the sampler advancing tok/pos on the
           device, one host sync per generation.
``torch``  torch-eager oracle (``models/reference.py``): CPU tests / debugging.

Batching: up to ``max_batch`` (≤ 256) sequences decode together ("trial
batching") — each row has its own cache slot, position, budget
and sampling options; rows that finish early idle until the batch ends.
(An idle row keeps its last position and token, so each later step rewrites that one KV position with the last
generated token's K / V: harmless, nothing reads it again; tests/engine_state.py expected_inputs encodes it.)
Prefill: every prompt token but the last goes through the same forward as
≤128-row chunks (rows carry their own slot/position, so the decode attention
kernel doubles as causal prefill attention); the last prompt token is the
first decode step's input, so no separate prefill LM-head path exists.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
import threading
import time
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from ..models.config import ModelConfig, get_config, rope_inv_freq
from ..models.hf import checkpoint_for, load_hf_weights, load_pretrained, load_tokenizer
from ..models.tokenizer import get_tokenizer
from .. import ops
from . import jsonmode, stopseq
from .speculative import K_MAX, SeqState, draft_model_given, draft_model_rows, draft_token, dvalid_after
from .speculative import draft as spec_draft_host
from ..models.weights import WEIGHT_DTYPES, ModelWeights, pack_for_engine, random_weights, roundtrip_weights

#: Ollama's default sampling options (SURVEY §2.4 "Sampling" row)
OLLAMA_DEFAULTS = dict(temperature=0.8, top_k=40, top_p=0.9, repeat_penalty=1.1, repeat_last_n=64, seed=None)

MAX_ROWS = 256  # rows per forward: decode batch (runtime.hip CAIN_MAX_ROWS)
PREFILL_ROWS = 128  # prompt tokens per prefill forward
W8_MAX_ROWS = 64  # few-row fp8 / MXFP4 weight kernels (gemm_w8.hip / gemm_w4.hip): rows per forward without W8A8
W8A8_MIN_ROWS = 16  # fp8 engines run forwards of more rows on the W8A8 wide kernel (csrc/wgemm8.hip)
# Prefix reuse (``prefix_cache=True``): a request copies a prefix from another slot (csrc/kv_prefix.hip) instead of
# reusing a free slot in place only when that saves at least this many prompt tokens of prefill.  Measured on the
# graph-free admit path (profiles/r11/prefix_cache/README.md; llama3.1:8b and qwen2:1.5b, bf16, one box, interleaved):
# one copy launch costs 36 - 117 us of wall time (64 .. 2,016 positions), a prefill forward 1.1 / 2.8 ms for its first
# token and 6.6 / 9.1 us for each further one, so a copy pays for itself from 13 tokens at the longest prefix on the
# dearer model; 16 covers every row of the table.
PREFIX_COPY_MIN = 16


@dataclass
class GenResult:
    model: str
    prompt_tokens: List[int]
    tokens: List[int]
    text: str
    done_reason: str
    load_duration_ns: int = 0
    prompt_eval_duration_ns: int = 0
    eval_duration_ns: int = 0
    total_duration_ns: int = 0
    prompt_cached: int = 0  # leading prompt tokens whose KV a cache slot already held (prefix reuse)
    # per generated token (None: not asked for): its natural-log softmax under the model's own logits (temperature 1,
    # before the repeat penalty and top-k / top-p), and the ``top_logprobs`` most likely (id, logprob) pairs of that
    # distribution, logit descending, index ascending on ties
    logprobs: Optional[List[float]] = None
    top_logprobs: Optional[List[List[tuple]]] = None
    # speculative decoding (None: the mode is off): drafts proposed, generated tokens that were accepted drafts, the
    # decode steps the row was live for, and the tokens each of those steps committed
    draft_count: Optional[int] = None
    draft_accepted: Optional[int] = None
    decode_steps: Optional[int] = None
    step_tokens: Optional[List[int]] = None
    # JSON mode (None: the row was not in it): "done" -- the top-level object closed, on the row's last token;
    # "open" -- the budget ran out inside the document (the text is a viable prefix); "fail" -- the sampler drew a
    # masked token (a rounding of its last prefix sum), which was taken back
    json_state: Optional[str] = None
    # stop sequences (options.stop): the string that ended the row (None: the row had none, or hit none); the text
    # is then cut where that occurrence starts, ``tokens`` keeps every generated token
    stop_hit: Optional[str] = None

    @property
    def prompt_eval_count(self) -> int:
        return len(self.prompt_tokens)

    @property
    def eval_count(self) -> int:
        return len(self.tokens)

    def ollama_json(self, created_at: Optional[str] = None, context: bool = False) -> Dict:
        """``context``: fill Ollama's ``context`` (the prompt's token ids, then the generated ones: what a client
        sends back to continue); otherwise it stays empty and the response small."""
        import datetime

        d = {
            "model": self.model,
            "created_at": created_at or datetime.datetime.utcnow().isoformat() + "Z",
            "response": self.text,
            "done": True,
            "done_reason": self.done_reason,
            "context": list(self.prompt_tokens) + list(self.tokens) if context else [],
            "total_duration": self.total_duration_ns,
            "load_duration": self.load_duration_ns,
            "prompt_eval_count": self.prompt_eval_count,
            "prompt_eval_duration": self.prompt_eval_duration_ns,
            "eval_count": self.eval_count,
            "eval_duration": self.eval_duration_ns,
        }
        if self.prompt_cached > 0:
            d["prompt_cached_count"] = int(self.prompt_cached)
        if self.draft_count is not None:
            d["draft_count"] = int(self.draft_count)
            d["draft_accepted_count"] = int(self.draft_accepted or 0)
        return d


#: the further sampling options (csrc/sample.hip SampleExt), each neutral at 0: ``min_p`` in [0, 1]; the presence and
#: frequency penalties >= 0 (the few-row samplers' thresholds rest on penalties that only lower a logit)
SAMPLE_EXT_DEFAULTS = dict(min_p=0.0, presence_penalty=0.0, frequency_penalty=0.0)
SPEC_EXT_REFUSAL = ("min_p, presence_penalty and frequency_penalty cannot be combined with speculative decoding (the "
                    "K + 1 expanded rows would each need their own record)")


def ext_options(opts: Optional[Dict]) -> Dict:
    """``min_p`` / ``presence_penalty`` / ``frequency_penalty`` of a request's options (None or absent: 0), as
    floats; ValueError on a non-number, a non-finite value, ``min_p`` outside [0, 1] or a negative penalty."""
    out = {}
    for k, d in SAMPLE_EXT_DEFAULTS.items():
        v = opts.get(k) if opts else None
        if v is None:
            v = d
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{k} must be a number, got {v!r}")
        v = float(v)
        if not math.isfinite(v):
            raise ValueError(f"{k} must be finite, got {v!r}")
        if k == "min_p" and not 0.0 <= v <= 1.0:
            raise ValueError(f"min_p must be in [0, 1], got {v!r}")
        if k != "min_p" and v < 0.0:
            raise ValueError(f"{k} must be >= 0, got {v!r}")
        out[k] = v
    return out


def ext_active(o: Dict) -> bool:
    return any(o.get(k, 0.0) != 0.0 for k in SAMPLE_EXT_DEFAULTS)


def _row_options(opts: Optional[Dict], cfg: ModelConfig, index: int, base_seed: int) -> Dict:
    o = dict(OLLAMA_DEFAULTS)
    if opts:
        o.update({k: v for k, v in opts.items() if v is not None and k in OLLAMA_DEFAULTS})
    ext = ext_options(opts)
    seed = o.get("seed")
    if seed is None:
        seed = (base_seed * 1000003 + index * 7919 + time.monotonic_ns()) & 0xFFFFFFFFFFFF
    return dict(temperature=float(o["temperature"]), top_p=float(o["top_p"]),
                repeat_penalty=float(o["repeat_penalty"]), top_k=int(o["top_k"]),
                repeat_last_n=int(o["repeat_last_n"]),
                eos_id=int(opts.get("eos_id", cfg.eos_id)) if opts and "eos_id" in opts else int(cfg.eos_id),
                # further stop ids: the caller's, else the model's unless the caller set eos_id (forced lengths:
                # eos_id -1 disables every stop)
                stop=tuple(int(x) for x in (opts["stop_ids"] if opts and "stop_ids" in opts else
                                            () if opts and "eos_id" in opts else cfg.stop_ids))[:3],
                # stop strings (options.stop, engine/stopseq.py) under a name of their own: ``stop`` above is the ids
                stop_strs=stopseq.parse_stop(opts.get("stop")) if opts else (),
                seed=int(seed) & 0xFFFFFFFFFFFFFFFF, **ext)


def _stopped(toks: List[int], o: Dict) -> bool:
    """A generation that ended on one of its row's stop ids (done_reason "stop")."""
    return bool(toks) and ((o["eos_id"] >= 0 and toks[-1] == o["eos_id"]) or toks[-1] in o.get("stop", ()))


# ============================================================== the plan's formats (records: ops CainPlanDesc ...)
WFMT = {"bf16": 0, "fp8": 1, "fp4": 2, "q4_0": 3, "q4_k": 4, "q4_k_m": 4}  # runtime.hip WFMT_* (q4_k_m: Q4_K + MFMT)
MFMT = {0: 3, 1: 4, 2: 5}  # models/q4.py format id -> runtime.hip WFMT_Q4_0 / WFMT_Q4_K / MFMT_Q6_K
Q4_DTYPES = ("q4_0", "q4_k", "q4_k_m")


def _want_format(format, opts: Sequence[Optional[Dict]], B: int) -> List[bool]:
    """Per row: JSON mode or not, from ``format`` (None / "" off, "json" on; one value or one per row) or, where
    that leaves a row off, the row's option key ``"format"``."""
    fs = list(format) if isinstance(format, (list, tuple)) else [format] * B
    if len(fs) != B:
        raise ValueError(f"format for {len(fs)} rows, {B} prompts")
    out = []
    for i, f in enumerate(fs):
        f = f or (opts[i].get("format") if i < len(opts) and opts[i] else None)
        if f not in (None, "", "json"):
            raise ValueError(f'format must be "json" or absent, got {f!r}')
        out.append(f == "json")
    return out


TOP_LOGPROBS_MAX = 20  # Ollama's limit; the entries per token of the device buffers (csrc/logprob.hip LP_TOP)


@dataclass
class ScoreResult:
    """``DecodeEngine.score`` of one prompt: ``logprobs[j]`` is the logprob of ``tokens[j + 1]`` given
    ``tokens[:j + 1]`` (n - 1 values for n tokens), ``top_logprobs[j]`` the alternatives at that position."""
    tokens: List[int]
    logprobs: List[float]
    top_logprobs: List[List[tuple]]

    @property
    def nll(self) -> float:
        return -float(sum(self.logprobs))


POOLINGS = ("last", "mean")


@dataclass
class EmbedResult:
    """One prompt's embedding (``DecodeEngine.embed``): ``embedding`` d floats, ``prompt_eval_count`` the tokens that
    went through the model, ``truncated`` whether the prompt was cut to the context."""
    embedding: List[float]
    prompt_eval_count: int
    truncated: bool = False


def logprob_host(logits: torch.Tensor, n: int = 0):
    """The definition on the host: float64 log-softmax of one row of fp32 logits; returns it ([V] float64 numpy) with
    the ``n`` most likely ``(id, logprob)`` pairs, logit descending and index ascending on ties (the samplers'
    order).  The torch backend's logprobs, and the reference of the device kernels' tests."""
    lg = logits.detach().to(torch.float32).cpu().numpy()
    x = lg.astype(np.float64)
    mx = x.max()
    ls = x - (mx + np.log(np.exp(x - mx).sum()))
    V = lg.shape[0]
    k = min(int(n), V)
    if k <= 0:
        return ls, []
    cand = np.flatnonzero(lg >= np.partition(lg, V - k)[V - k])  # ties with the k-th largest included
    ids = cand[np.lexsort((cand, -x[cand]))][:k]
    return ls, [(int(i), float(ls[i])) for i in ids]


def _want_logprobs(logprobs, top_logprobs, B: int) -> List[int]:
    """Per row: -1 (no logprobs) or the number of alternatives, from scalars or per-row sequences."""
    lps = list(logprobs) if isinstance(logprobs, (list, tuple)) else [logprobs] * B
    tops = list(top_logprobs) if isinstance(top_logprobs, (list, tuple)) else [top_logprobs] * B
    if len(lps) != B or len(tops) != B:
        raise ValueError(f"logprobs / top_logprobs for {len(lps)} / {len(tops)} rows, {B} prompts")
    out = []
    for want, n in zip(lps, tops):
        n = int(n or 0)
        if not 0 <= n <= TOP_LOGPROBS_MAX:
            raise ValueError(f"top_logprobs must be in 0..{TOP_LOGPROBS_MAX}, got {n}")
        if n and not want:
            raise ValueError("top_logprobs needs logprobs")
        out.append(n if want else -1)
    return out


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def attention_splits(M: int, Hkv: int, T_max: int) -> int:
    """Position splits per (row, kv head): ~256 workgroups in flight, >= 4 blocks of 32 per split at
    full context, <= 64 splits (measured: 1024-WG targets lose more to the split combine than they
    gain in parallelism, profiles/kernels.md).  (Round 1-3's per-split block cap and forced split count were tuning
    switches; their measurements are in profiles/r2/attn_occupancy.md.)"""
    if M * Hkv <= 64:
        # few (row, kv head) pairs run 8-wave workgroups (attention.hip): position splits up to ~64 workgroups
        # (<= 8 splits, >= 4 blocks of 32 positions per split at full context), and at most 64 blocks per split.
        # Measured in the graph-replayed batch-1 decode (rocprof, profiles/r2/attn_occupancy.md): llama3.1:8b
        # 10.9 -> 7.7 us per call at 8 splits (4: 9.1, 16: 8.5), qwen2:1.5b 11.2 -> 8.2, gemma:2b 18.9 -> 13.2,
        # phi3 (32 pairs, 2 splits) 9.7 -> 9.2, llama at 2 rows (4 splits) 11.2 -> 9.4 -- the in-kernel combine's
        # round trips cost less than one workgroup per pair walking the whole context.
        # Round 6, with the one-round-trip split combine (profiles/r6/attn_combine/splits_ab.jsonl, one box,
        # interleaved): a single (row, kv head) pair -- gemma:2b's MQA at batch 1 -- takes 16 splits of >= 3 blocks
        # (1,235 -> 1,256 tok/s); qwen2:1.5b (2 pairs) lost 0.6 % at 12 or 16 and llama3.1:8b (8 pairs) gained 0.5 %
        # at 12, so the others keep 8.  CAIN_ATTN_FEW_SPLITS / CAIN_ATTN_MIN_BLOCKS override both for A/B runs.
        one = M * Hkv == 1
        cap = int(os.environ.get("CAIN_ATTN_FEW_SPLITS", "0") or 0) or (16 if one else 8)
        min_blocks = int(os.environ.get("CAIN_ATTN_MIN_BLOCKS", "0") or 0) or (3 if one else 4)
        few = min(cap, T_max // (32 * min_blocks), 64 // (M * Hkv))
        return int(max(1, min(64, max(few, math.ceil((T_max // 32) / 64)))))
    ns = max(1, min(T_max // 128, math.ceil(256 / (M * Hkv))))
    return int(max(1, min(64, ns)))


def _load_ckpt(ckpt, cfg: ModelConfig, device, weight_dtype: str) -> ModelWeights:
    w = load_hf_weights(ckpt, cfg, device=device)
    _attach_native(w, ckpt, cfg, weight_dtype, device)
    return w


def _attach_native(weights: ModelWeights, path, cfg: ModelConfig, weight_dtype: str, device) -> None:
    """A GGUF checkpoint run on a GGUF block format (weight_dtype q4_0 / q4_k / q4_k_m): keep its blocks as stored
    (models/q4.py gguf_q4_native: the 4-bit format's and Q6_K's, whatever mix the file holds) for pack_for_engine,
    instead of re-quantising the decoded values."""
    from ..models.gguf import GGUFFile, is_gguf

    if weight_dtype in Q4_DTYPES and path and is_gguf(path):
        from ..models.q4 import gguf_q4_native
        from ..models.weights import _q4_format

        weights.native = gguf_q4_native(GGUFFile(path), cfg, _q4_format(weight_dtype), device=device)


def common_prefix(a: Sequence[int], b: Sequence[int]) -> int:
    """Length of the longest common prefix of two token lists."""
    n = min(len(a), len(b))
    for i in range(n):
        if a[i] != b[i]:
            return i
    return n


def plan_prefix_reuse(records: Sequence[Sequence[int]], free_slots: Sequence[int], live_slots: Sequence[int],
                      prompts: Sequence[Sequence[int]], copy_min: Optional[int] = None):
    """Which cache slot each new request takes and how much of its prompt that slot already holds.

    ``records[s]``: the tokens whose KV slot ``s`` holds at positions ``0 .. len - 1`` (for a live row the lower
    bound known at the last poll); ``free_slots``: the free list in its own order (today's choice is its last
    element, ``pop()``); ``live_slots``: slots of rows that are decoding.  Returns ``[(slot, n, donor)]`` per request,
    in order: the request prefills from position ``n`` (0: everything), after positions ``[0, n)`` of ``donor`` were
    copied to ``slot`` when ``donor`` is not None.  Nothing is modified.

    * ``n`` is a longest common token prefix, at most ``len(prompt) - 1``: the last prompt token is the first decode
      step's input and always runs.
    * The free slot with the longest match is reused in place (any ``n >= 1``; among equals the one ``pop()`` would
      reach first).
    * A slot that cannot be taken -- live, or free but claimed in place by an earlier request of this call, whose
      old contents stay put until the prefill that follows the copies -- is a donor when its match is longer than
      the best free slot's by at least ``copy_min``: the request takes the next free slot in ``pop()`` order and
      copies.  A slot that is the destination of a copy is never a donor, and the records are the ones from before
      the call, so requests admitted together never feed each other.
    * With nothing to reuse the slots are exactly ``free_slots.pop()`` per request."""
    copy_min = PREFIX_COPY_MIN if copy_min is None else int(copy_min)
    free = list(free_slots)
    donors = list(live_slots)  # slots whose contents are readable during this call but cannot be taken
    out = []
    for p in prompts:
        if not free:
            raise ValueError("more requests than free slots")
        cap = len(p) - 1
        best_slot, best_n = None, 0
        for s in reversed(free):
            n = min(common_prefix(records[s], p), cap) if records[s] else 0
            if n > best_n:
                best_slot, best_n = s, n
        donor, donor_n = None, 0
        for s in donors:
            n = min(common_prefix(records[s], p), cap) if records[s] else 0
            if n > donor_n:
                donor, donor_n = s, n
        if donor is not None and donor_n >= best_n + max(1, copy_min):
            slot = free.pop()
            out.append((slot, donor_n, donor))
        elif best_slot is not None:
            free.remove(best_slot)
            donors.append(best_slot)
            out.append((best_slot, best_n, None))
        else:
            slot = free.pop()
            donors.append(slot)  # (an empty or unrelated record: it can still serve a later request of this call)
            out.append((slot, 0, None))
    return out


def taken_record(record: Sequence[int], n: int, prompt: Sequence[int]) -> List[int]:
    """The record of a slot taken with reuse ``n`` for ``prompt``, once its prefill ran: whatever the slot held past
    position ``n`` is stale and goes, the prompt's tokens ``n .. len - 2`` follow."""
    if list(record[:n]) != list(prompt[:n]):
        raise ValueError(f"slot record and prompt differ inside the reused prefix ({n} tokens)")
    return list(record[:n]) + [int(t) for t in prompt[n:len(prompt) - 1]]


SPEC_STOP_REFUSAL = ("stop strings cannot be combined with speculative decoding (one step commits several tokens; "
                     "token ids go in stop_ids)")


class _PieceDecoder:
    """``decode`` by the byte pieces of ``DecodeEngine.set_json_vocab`` (a character cut at the end decodes to
    U+FFFD, which ``StreamDecoder`` holds back)."""

    def __init__(self, eng: "DecodeEngine"):
        self.eng = eng

    def decode(self, ids) -> str:
        return self.eng._json_text([int(t) for t in ids])


class DecodeEngine:
    @classmethod
    def from_pretrained(cls, path: str, device: Union[str, torch.device] = "cuda", name: Optional[str] = None,
                        **kw) -> "DecodeEngine":
        """An engine on a Hugging Face checkpoint directory (``config.json`` + safetensors + ``tokenizer.json``;
        ``models/hf.py``): the same kernels and options as a tag's engine (``weight_dtype="fp4"`` quantises the
        checkpoint's bf16 weights to MXFP4 at load, as the packing of random weights does)."""
        cfg, weights, tok = load_pretrained(path, name=name, device=torch.device(device))
        _attach_native(weights, path, cfg, kw.get("weight_dtype", "bf16"), torch.device(device))
        return cls(cfg, device=device, weights=weights, tokenizer=tok, **kw)

    def __init__(self, model: Union[str, ModelConfig], device: Union[str, torch.device] = "cuda",
                 max_batch: int = 16, max_context: int = 2048, seed: int = 0, backend: Optional[str] = None,
                 steps_per_graph: int = 8, weights: Optional[ModelWeights] = None, tokenizer=None,
                 keep_natural: bool = False, weight_dtype: str = "bf16", kv_dtype: str = "bf16", cu_limit: int = 0,
                 prefix_cache: Optional[bool] = None, speculative: Optional[int] = None,
                 draft_model: Union[None, str, ModelWeights] = None, draft_weight_dtype: Optional[str] = None):
        """``weight_dtype="fp8"``: GEMM weights quantised per row to e4m3 (half the weight bytes per decode step):
        forwards of up to 16 rows run W8A16 (gemm_w8.hip, bf16 activations), wider ones W8A8 (wgemm8.hip: the
        activations quantised per row to e4m3, fp8 MFMA) up to 256 rows; CAIN_W8A8=0 keeps W8A16 only (<= 64
        rows).
        ``weight_dtype="fp4"``: OCP MXFP4 GEMM weights (e2m1, one e8m0 scale per 32 k; 0.53 bytes per parameter),
        the reference's 4-bit precision class: W4A16 few-row kernels (gemm_w4.hip) up to 16 rows per forward, W4A8
        above (wgemm8.hip FP4: the same bytes on the block-scaled fp4 x fp8 MFMA, activations per row to e4m3) up to
        256; every GEMM K (d_model, q_dim, ffn) must be a multiple of 128 (>= 512 for W4A8).
        ``weight_dtype="q4_0" / "q4_k"``: llama.cpp's GGUF 4-bit blocks (Ollama's default builds) run natively
        (gemm_qstream.hip: the block values as stored, scales applied per block; forwards of more rows than its LDS copy
        holds on gemm_qtile.hip, one pass over the weights per 64 rows) up to 64 rows per
        forward; every GEMM K must be a multiple of 256.
        ``weight_dtype="q4_k_m"``: Q4_K with the output head and the attn_v / ffn_down matrices of part of the
        layers in Q6_K (gemm_qstream.hip), the mix of Ollama's default Q4_K_M files (models/gguf.py q4_k_m_type) -- what
        random-init and Hugging Face weights are laid out in.  A GGUF file loaded on ``q4_k`` or ``q4_k_m`` keeps
        whatever mix of Q4_K and Q6_K tensors it stores (``weights.native["requantized"]`` lists the tensors of any
        other type -- Q5_K, Q8_0, F16 ... -- and a Q6_K gate / up, which are re-quantised to Q4_K); a layer whose V
        is Q6_K beside Q4_K q / k runs its QKV projection as two launches.
        ``kv_dtype="fp8"``: the KV cache holds e4m3 elements (half the attention bytes per decode step and half
        the cache memory; csrc/attention.hip KV8).
        ``cu_limit``: run every kernel on a stream whose hardware queue may use only that many CUs (a multiple of
        8; runtime.hip cain_stream_create_cu_limited) and size the grids for them -- the batch-1 energy lever
        measured by tools/cu_sweep.py.  0: the whole device.
        ``prefix_cache``: the continuous batch (HIP backend) keeps a record of the tokens each cache slot holds
        (``slot_tokens``) and a new request prefills only what differs from the best matching slot
        (``plan_prefix_reuse``; a prefix held by a slot that is still decoding is copied, csrc/kv_prefix.hip).  Off
        by default (None: ``CAIN_PREFIX_CACHE=1`` turns it on): without it every admit prefills from position 0 and
        the caches hold exactly what the requests wrote.
        ``speculative``: K in 0 .. 7 drafts per sequence and decode step (engine/speculative.py: n-gram lookup in the
        request's own tokens, or drafts given to ``generate``), verified K + 1 rows per sequence in one forward; a
        draft is kept only when it is the token the sampler draws, so drafts change the number of steps, not the
        tokens (a K + 1-row forward rounds differently from a 1-row one: against a plain engine, equal up to near-ties).  0 (default; None: ``CAIN_SPECULATIVE``): off, nothing changes.  A
        batch then holds at most ``rows per forward // (K + 1)`` sequences; not together with ``prefix_cache`` or
        ``logprobs``.
        ``draft_model`` (needs ``speculative > 0``; None: ``CAIN_DRAFT_MODEL``): a smaller model with the same
        tokenizer -- a tag, a checkpoint path or ``ModelWeights`` -- proposes each step's K drafts instead of the
        n-gram lookup (engine/speculative.py "Draft model"): an inner engine ``self.draft`` on this engine's device
        and stream with its own weights (``draft_weight_dtype``, default ``weight_dtype``), plan and KV cache, run
        inside the same decode graphs (csrc/runtime.hip forward_spec_model).  The first draft forward has two rows
        per sequence, so a batch holds at most 32 sequences (64 rows: what every weight format's forward takes).
        The tokens stay those of the engine without a draft model; what changes is how many drafts are accepted."""
        self.cfg = get_config(model) if isinstance(model, str) else model
        self._json_pieces: Optional[List[bytes]] = None  # JSON mode's vocabulary, made at first use (_json_vocab)
        self._json_lock = threading.Lock()
        self._json_custom = False  # ... given by set_json_vocab: the text of a JSON row is spelt with it
        self._gr: Optional[Dict] = None  # JSON mode's device buffers (hip backend), made at first use (_gr_bufs)
        self._last_json: Optional[List[Optional[str]]] = None
        self._pieces: Optional[List[bytes]] = None  # the tokenizer's byte pieces, made at first use (_piece_vocab)
        self._st: Optional[Dict] = None  # the stop sequences' device buffers (hip backend), made at first use
        self._last_stop: Optional[List[Optional[tuple]]] = None  # per row of the last generate: (hit_start, index)
        if weight_dtype not in WEIGHT_DTYPES:
            raise ValueError(f"weight_dtype must be one of {WEIGHT_DTYPES}, got {weight_dtype!r}")
        if weight_dtype == "fp4" and any(k % 128 for k in (self.cfg.d_model, self.cfg.q_dim, self.cfg.ffn)):
            raise ValueError(f"weight_dtype='fp4' needs d_model, q_dim and ffn to be multiples of 128 ({self.cfg.name})")
        if weight_dtype in Q4_DTYPES and any(k % 256 for k in (self.cfg.d_model, self.cfg.q_dim, self.cfg.ffn)):
            raise ValueError(f"weight_dtype={weight_dtype!r} needs d_model, q_dim and ffn to be multiples of 256 "
                             f"({self.cfg.name})")
        if kv_dtype not in ("bf16", "fp8"):
            raise ValueError(f"kv_dtype must be 'bf16' or 'fp8', got {kv_dtype!r}")
        self.weight_dtype = weight_dtype
        self.kv_dtype = kv_dtype
        self.cu_limit = int(cu_limit)
        self.prefix_cache = (os.environ.get("CAIN_PREFIX_CACHE", "0") == "1") if prefix_cache is None \
            else bool(prefix_cache)
        self.speculative = int(os.environ.get("CAIN_SPECULATIVE", "0") or 0) if speculative is None \
            else int(speculative)
        if not 0 <= self.speculative <= K_MAX:
            raise ValueError(f"speculative must be in 0..{K_MAX}, got {self.speculative}")
        if self.speculative and self.prefix_cache:
            raise ValueError("speculative decoding and prefix_cache cannot be combined (the slot records assume one "
                             "token per step)")
        if draft_model is None and self.speculative:  # (the environment names the draft of speculative engines only)
            draft_model = os.environ.get("CAIN_DRAFT_MODEL") or None
        if draft_model is not None and not self.speculative:
            raise ValueError("draft_model needs speculative > 0")
        self.draft: Optional["DecodeEngine"] = None  # the draft model's inner engine (speculative.py "Draft model")
        self._specd: Optional[Dict] = None  # its device buffers (hip backend), made at first use (_spec_draft_bufs)
        self.prefill_rows_total = 0  # rows fed to prefill forwards so far
        if self.cu_limit and (self.cu_limit < 0 or self.cu_limit % 8):
            raise ValueError(f"cu_limit must be a positive multiple of 8 (or 0), got {cu_limit}")
        # W8A8 needs whole 128-deep stages, >= 4 of them, on every GEMM's K (all real configs; not the tiny ones)
        self.w8a8 = (weight_dtype == "fp8" and os.environ.get("CAIN_W8A8", "1") != "0"
                     and all(k % 128 == 0 and k >= 512 for k in (self.cfg.d_model, self.cfg.q_dim, self.cfg.ffn)))
        # MXFP4 above 16 rows: W4A8 on the same packed bytes (csrc/wgemm8.hip FP4), same shape rule as W8A8
        self.w4a8 = (weight_dtype == "fp4"
                     and all(k % 128 == 0 and k >= 512 for k in (self.cfg.d_model, self.cfg.q_dim, self.cfg.ffn)))
        row_cap = W8_MAX_ROWS if (weight_dtype == "fp4" and not self.w4a8) or (weight_dtype == "fp8" and not self.w8a8) \
            or weight_dtype in Q4_DTYPES else MAX_ROWS
        self.device = torch.device(device)
        if backend is None:
            backend = "hip" if self.device.type == "cuda" else "torch"
        self.backend = backend
        self.row_cap = int(row_cap)
        # speculative: a forward verifies K + 1 rows per sequence, so fewer sequences fit the rows of one forward
        self.max_batch = int(max(1, min(max_batch, row_cap // (self.speculative + 1))))
        if draft_model is not None:  # the draft model's first forward: 2 rows per sequence, whatever its format
            self.max_batch = min(self.max_batch, W8_MAX_ROWS // 2)
        # prompt tokens per prefill forward: the engine's own row count when that is wider (a 256-row engine
        # prefills 256 tokens per forward on the wide GEMM: half the launches of 128-row chunks)
        self.prefill_chunk = int(min(int(os.environ.get("CAIN_PREFILL_ROWS", "0") or 0)
                                     or max(PREFILL_ROWS, self.max_batch), row_cap))
        self.T_max = int(math.ceil(min(max_context, self.cfg.max_context) / 32) * 32)
        self.seed = seed
        self.steps_per_graph = max(1, int(steps_per_graph))
        # a checkpoint registered under the tag (CAIN_CHECKPOINTS, models/hf.py): its weights and tokenizer
        ckpt = checkpoint_for(model) if isinstance(model, str) and weights is None else None
        if tokenizer is None and ckpt:
            tokenizer = load_tokenizer(ckpt, self.cfg)
        self.tokenizer = tokenizer or get_tokenizer(self.cfg)
        self.keep_natural = keep_natural
        t0 = time.perf_counter_ns()
        if weights is None:
            weights = (_load_ckpt(ckpt, self.cfg, self.device, weight_dtype) if ckpt
                       else random_weights(self.cfg, device=self.device, seed=seed))
        self.weights = weights
        if backend == "hip":
            self._init_hip()
        elif backend == "torch":
            from ..models.reference import ReferenceModel
            # fp8 / fp4: the oracle runs on the dequantised weights the kernels multiply by
            ref_w = roundtrip_weights(weights, weight_dtype)
            self.ref = ReferenceModel(ref_w, memo_weights=self.device.type == "cpu", kv_dtype=kv_dtype)
        else:
            raise ValueError(f"unknown backend {backend!r}")
        if draft_model is not None:
            self._init_draft(draft_model, draft_weight_dtype or weight_dtype)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self.load_duration_ns = time.perf_counter_ns() - t0
        self._first_call = True
        self.last_ttft_ns = 0
        # per cache slot: the tokens whose KV the slot holds at positions 0 .. len - 1 (prefix_cache; else unused)
        self.slot_tokens: List[List[int]] = [[] for _ in range(self.max_batch)]

    def _init_draft(self, draft_model, weight_dtype: str) -> None:
        """The draft model's inner engine: the target's cache slots, ``T_max``, device and stream, no speculation of
        its own.  ``draft_model``: ``ModelWeights``, a checkpoint path or a tag (``CAIN_CHECKPOINTS`` resolves it as
        it does the target's)."""
        from ..models.hf import checkpoint_config
        from ..models.tokenizer import SyntheticTokenizer

        is_path = isinstance(draft_model, str) and os.path.exists(draft_model)
        cfg = draft_model.cfg if isinstance(draft_model, ModelWeights) else \
            checkpoint_config(draft_model) if is_path else get_config(draft_model)
        if cfg.max_context < self.T_max:
            raise ValueError(f"draft model {cfg.name}: max_context {cfg.max_context} is below the engine's context "
                             f"({self.T_max})")
        kw = dict(device=self.device, max_batch=self.max_batch, max_context=self.T_max, seed=self.seed,
                  backend=self.backend, steps_per_graph=self.steps_per_graph, keep_natural=self.keep_natural,
                  weight_dtype=weight_dtype, kv_dtype=self.kv_dtype, prefix_cache=False, speculative=0)
        if isinstance(draft_model, ModelWeights):
            d = DecodeEngine(cfg, weights=draft_model, **kw)
        elif is_path:
            d = DecodeEngine.from_pretrained(draft_model, **kw)
        else:
            d = DecodeEngine(draft_model, **kw)
        a, b = self.tokenizer, d.tokenizer
        if not isinstance(a, SyntheticTokenizer) and not isinstance(b, SyntheticTokenizer):
            for t in range(min(self.cfg.vocab, d.cfg.vocab)):
                if a.piece(t) != b.piece(t):
                    d.close()
                    raise ValueError(f"draft model {d.cfg.name}: token {t} is {b.piece(t)!r}, the target's is "
                                     f"{a.piece(t)!r} (a draft model needs the target's tokenizer)")
        if d.T_max != self.T_max or d.max_batch != self.max_batch:
            d.close()
            raise ValueError(f"draft model {d.cfg.name}: {d.max_batch} slots of {d.T_max} positions, the engine has "
                             f"{self.max_batch} of {self.T_max}")
        if self.backend == "hip":
            if 2 * self.max_batch > min(d.rows["tok"].shape[0], d.row_cap):
                d.close()
                raise ValueError(f"draft model {d.cfg.name}: its forwards take {d.rows['tok'].shape[0]} rows, the "
                                 f"first draft forward needs {2 * self.max_batch}")
            d.stream, d.cu_limit = self.stream, self.cu_limit  # one stream: the draft forwards sit in the same graphs
        self.draft = d

    # ---------------------------------------------------------------- hip setup
    def _init_hip(self) -> None:
        self.lib = ops.load()
        cfg, dev = self.cfg, self.device
        if self.device.type != "cuda":
            raise ValueError("hip backend needs a GPU device")
        w8a8 = self.w8a8 and max(self.max_batch, self.prefill_chunk) > W8A8_MIN_ROWS
        w4a8 = self.w4a8 and max(self.max_batch, self.prefill_chunk) > W8A8_MIN_ROWS
        packed = pack_for_engine(self.weights, free_natural=not self.keep_natural, weight_dtype=self.weight_dtype,
                                 w8a8=w8a8)
        torch.cuda.synchronize(dev)
        S, T, L = self.max_batch, self.T_max, cfg.n_layers
        bf = torch.bfloat16
        kv_layer = S * cfg.n_kv_heads * T * cfg.head_dim
        # zero-init: positions past a row's length must hold finite values (masked P = 0 multiplies them)
        kv_t = torch.uint8 if self.kv_dtype == "fp8" else bf
        self.kcache = torch.zeros(L * kv_layer, device=dev, dtype=kv_t)
        self.vtcache = torch.zeros(L * kv_layer, device=dev, dtype=kv_t)
        inv = rope_inv_freq(cfg)
        ang = np.arange(T, dtype=np.float64)[:, None] * inv[None, :]
        self.cos_t = torch.tensor(np.cos(ang), dtype=torch.float32, device=dev).contiguous()
        self.sin_t = torch.tensor(np.sin(ang), dtype=torch.float32, device=dev).contiguous()
        # rows any forward of this engine can have (speculative: K + 1 rows per sequence)
        R = max(self.max_batch * (self.speculative + 1), self.prefill_chunk)
        z = lambda *s, dt=bf: torch.zeros(*s, device=dev, dtype=dt)  # noqa: E731
        self.buf = dict(x=z(R, cfg.d_model), q=z(R, cfg.q_dim), attn=z(R, cfg.q_dim), act=z(R, cfg.ffn),
                        logits=z(R, cfg.vocab, dt=torch.float32), counters=z(R * cfg.n_kv_heads, dt=torch.int32))
        max_ms = max(m * attention_splits(m, cfg.n_kv_heads, T) for m in range(1, R + 1))
        self.part_o = z(max_ms * cfg.n_heads * cfg.head_dim, dt=torch.float32)
        self.part_ml = z(max(ops.attention_ml_floats(m, cfg.n_heads, cfg.n_kv_heads,
                                                     attention_splits(m, cfg.n_kv_heads, T))
                             for m in range(1, R + 1)), dt=torch.float32)
        i32 = torch.int32
        self.rows = dict(tok=z(R, dt=i32), pos=z(R, dt=i32), slot=torch.full((R,), -1, device=dev, dtype=i32),
                         n_gen=z(R, dt=i32), max_new=z(R, dt=i32), done=z(R, dt=i32), hist=z(R * 64, dt=i32))
        self.gen = z(R, self.T_max, dt=i32)
        self.prefill_rows = dict(tok=z(R, dt=i32), pos=z(R, dt=i32), slot=torch.full((R,), -1, device=dev, dtype=i32))
        self.sample_params = ops.sample_params_tensor(
            [dict(temperature=0.0, top_p=1.0, repeat_penalty=1.0, top_k=1, repeat_last_n=0, eos_id=-1, seed=0)] * R,
            dev)
        # the rows' further options (ops.sample_ext_tensor), beside sample_params: the captured graphs hold this
        # buffer's pointer, a request changes its contents
        self.sample_ext = ops.sample_ext_tensor([{}] * R, dev)
        if self.weight_dtype in Q4_DTYPES:
            self._check_gguf_shapes(packed)
        self._layers = (ops.CainLayer * L)()
        for i, lp in enumerate(packed["layers"]):
            self._layers[i] = ops.CainLayer(*(_ptr(lp.get(k)) for k in ops.LAYER_FIELDS),
                                            *(MFMT[lp[k]] if k in lp else 0 for k in ops.LAYER_FORMATS),
                                            _ptr(lp.get("wv")), _ptr(lp.get("sv")))
        self._packed = packed
        d = ops.CainPlanDesc()
        d.n_layers, d.d, d.H, d.Hkv, d.hd = L, cfg.d_model, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
        d.ffn, d.V, d.act_kind, d.T_max, d.Mpad = cfg.ffn, cfg.vocab, 1 if cfg.act == "gelu_tanh" else 0, T, R
        d.nsplit, d.waves = 1, 0
        d.eps = cfg.norm_eps
        d.embed_scale = float(torch.tensor(math.sqrt(cfg.d_model), dtype=bf).float()) if cfg.embed_scale else 1.0
        d.attn_scale = 1.0 / math.sqrt(cfg.head_dim)
        d.embed, d.lm_head = _ptr(self.weights.embed), _ptr(packed["lm_head"])
        d.layers = ctypes.cast(self._layers, ctypes.c_void_p).value
        d.kcache, d.vtcache, d.kv_layer_elems = _ptr(self.kcache), _ptr(self.vtcache), kv_layer
        d.kv8 = int(self.kv_dtype == "fp8")
        d.cos_t, d.sin_t = _ptr(self.cos_t), _ptr(self.sin_t)
        for k in ("x", "q", "attn", "act", "logits", "counters"):
            setattr(d, k, _ptr(self.buf[k]))
        d.part_o, d.part_ml = _ptr(self.part_o), _ptr(self.part_ml)
        self.wgemm_plans = self._wide_gemm_plans(R)
        # split-K workspace of the batched / wide GEMMs and of the skinny kernel's split grids (M <= 16 on narrow
        # outputs): largest need over this model's GEMM shapes at every row count (after any
        # CAIN_WGEMM_PLANS override, which may pick larger split counts than the default rule)
        shapes = [(cfg.qkv_dim, cfg.d_model), (cfg.d_model, cfg.q_dim), (2 * cfg.ffn, cfg.d_model),
                  (cfg.d_model, cfg.ffn), (cfg.vocab, cfg.d_model)]
        ws = max([ops.gemm_ws_bytes(n, k, m) for n, k in shapes for m in range(1, R + 1)] + [0])
        if self.weight_dtype == "fp4":  # split-K tickets + partials of the few-row MXFP4 stream kernel
            ws = max([ws] + [int(self.lib.cain_gemm_w4_ws_bytes(n, k, 1)) for n, k in shapes])
        if w8a8 or w4a8:
            ws = max([ws] + [int(self.lib.cain_w8a8_ws_bytes(n, k, m)) for n, k in shapes for m in range(17, R + 1)])
            kmax = max(cfg.d_model, cfg.q_dim, cfg.ffn)
            self.x8 = torch.zeros(R, kmax, device=dev, dtype=torch.uint8)
            self.xs = torch.zeros(R, device=dev, dtype=torch.float32)
            d.lm_head8, d.x8, d.xs, d.x8_ld = _ptr(packed.get("lm_head8")), _ptr(self.x8), _ptr(self.xs), kmax
        self.gemm_ws = torch.zeros(max(ws, 16) // 4 + 1, device=dev, dtype=torch.int32)
        d.gemm_ws, d.gemm_ws_bytes = _ptr(self.gemm_ws), ws
        d.wfmt, d.lm_head_scale = WFMT[self.weight_dtype], _ptr(packed.get("lm_head_scale"))
        d.q4_gain = int(bool(packed.get("q4_gain")))  # GGUF blocks as stored: gains applied to the activations
        d.flm_head = MFMT[packed["flm_head"]] if "flm_head" in packed else 0
        self._desc = d
        self._lp: Optional[Dict[str, torch.Tensor]] = None  # logprob buffers, allocated at first use (_lp_bufs)
        self._pool: Optional[Dict[str, torch.Tensor]] = None  # embedding pooling buffers, likewise (_pool_bufs)
        self._spec: Optional[Dict] = None  # speculative buffers, allocated at first use (_spec_bufs)
        self._plans: Dict[int, int] = {}
        self._graphs: Dict[tuple, int] = {}
        self._cu_stream = None
        if self.cu_limit and self.cu_limit < torch.cuda.get_device_properties(dev).multi_processor_count:
            with torch.cuda.device(dev):
                h = self.lib.cain_stream_create_cu_limited(self.cu_limit)
            if not h:
                raise RuntimeError(f"hipExtStreamCreateWithCUMask failed for {self.cu_limit} CUs")
            self._cu_stream = h
            self.stream = torch.cuda.ExternalStream(h, device=dev)
        else:
            self.cu_limit = 0
            self.stream = torch.cuda.Stream(device=dev)

    def _check_gguf_shapes(self, packed) -> None:
        """Refuse a model one of whose GEMMs the GGUF stream kernels cannot hold a single activation row of in LDS
        (cain_gemm_q4_rows / cain_gemm_q6_rows == 0 for its K, epilogue and format): such a forward would fail at
        its first launch of that shape."""
        from ..ops import EPI_F32, EPI_GELU, EPI_QKV_ROPE, EPI_RESID, EPI_SILU

        cfg = self.cfg
        act = EPI_GELU if cfg.act == "gelu_tanh" else EPI_SILU
        gemms = [("lm_head", packed.get("flm_head"), cfg.d_model, EPI_F32)]
        for i, lp in enumerate(packed["layers"]):
            gemms += [(f"layer {i} {n}", lp.get(f), k, e) for n, f, k, e in (
                ("wqkv", "fqkv", cfg.d_model, EPI_QKV_ROPE), ("wv", "fv", cfg.d_model, EPI_QKV_ROPE),
                ("wo", "fo", cfg.q_dim, EPI_RESID), ("wgu", "fgu", cfg.d_model, act),
                ("wdown", "fdown", cfg.ffn, EPI_RESID)) if n in lp]
        for name, f, k, epi in gemms:
            rows = self.lib.cain_gemm_q6_rows(k, epi) if f == 2 else self.lib.cain_gemm_q4_rows(k, epi)
            if int(rows) < 1:
                raise ValueError(f"{cfg.name}: {name} (K = {k}, {'Q6_K' if f == 2 else 'Q4'}) does not fit the GGUF "
                                 f"stream kernel's LDS copy of one activation row")

    def _wide_gemm_plans(self, R: int) -> list:
        """Split plans of the wide-batch GEMM (csrc/wgemm.hip) this engine runs, per projection shape at its
        widest forward: the default rule, or ``CAIN_WGEMM_PLANS="N:K:BM:KS[:VARIANT],..."`` (explicit per-shape
        plans for in-graph A/B runs; measured in the graph-replayed decode, never by isolated timings -- an
        isolated autotune's winners did not move the headline, profiles/wgemm_r2.md)."""
        for spec in filter(None, os.environ.get("CAIN_WGEMM_PLANS", "").split(",")):
            f = [int(x) for x in spec.split(":")]
            ops.set_wide_gemm_plan(f[0], f[1], f[2], f[3], f[4] if len(f) > 4 else -1)
        cfg = self.cfg
        shapes = [(cfg.qkv_dim, cfg.d_model), (cfg.d_model, cfg.q_dim), (2 * cfg.ffn, cfg.d_model),
                  (cfg.d_model, cfg.ffn), (cfg.vocab, cfg.d_model)]
        out = []
        if self.weight_dtype == "bf16" and R > 64:
            for n, k in shapes:
                if ops.wide_gemm_eligible(n, k, R):
                    ks, v = ops.wide_gemm_plan(n, k, R)
                    out.append(dict(n=n, k=k, m=R, ks=ks, variant=v))
        return out

    def _plan(self, M: int) -> int:
        """One native plan per attention split count (nsplit depends on the row count)."""
        ns = attention_splits(M, self.cfg.n_kv_heads, self.T_max)
        if ns not in self._plans:
            self._desc.nsplit = ns
            self._plans[ns] = self.lib.cain_plan_create(ctypes.byref(self._desc))
        return self._plans[ns]

    def _rows_struct(self, rows: Dict[str, torch.Tensor], with_sampling: bool) -> ops.CainRows:
        r = ops.CainRows()
        r.tok, r.pos, r.slot = _ptr(rows["tok"]), _ptr(rows["pos"]), _ptr(rows["slot"])
        if with_sampling:
            r.n_gen, r.max_new, r.done = _ptr(rows["n_gen"]), _ptr(rows["max_new"]), _ptr(rows["done"])
            r.hist, r.gen, r.ldg = _ptr(rows["hist"]), _ptr(self.gen), self.gen.stride(0)
            r.sample_params = _ptr(self.sample_params)
            r.sample_ext = _ptr(self.sample_ext)
        return r

    def _lp_bufs(self) -> Dict[str, torch.Tensor]:
        """Device buffers of the token log-probabilities (csrc/logprob.hip), made when a request first asks: per row
        ``topn`` (-1: not wanted; ``s_topn``: of ``score``'s rows), rings indexed like ``gen`` (``lp [R, T]``, ``top_id / top_lp [R, T, 20]``), the
        scratch between the two launches of a decode step, and the per-row targets and results of ``score``."""
        if self._lp is None:
            dev, R, T, K = self.device, self.gen.shape[0], self.T_max, TOP_LOGPROBS_MAX
            z = lambda *s, dt=torch.float32: torch.zeros(*s, device=dev, dtype=dt)  # noqa: E731
            self._lp = dict(topn=torch.full((R,), -1, device=dev, dtype=torch.int32), lp=z(R, T),
                            top_id=z(R, T, K, dt=torch.int32), top_lp=z(R, T, K), keep=ops.logprob_keep(R, dev),
                            target=z(R, dt=torch.int32), s_lp=z(R),
                            s_topn=torch.full((R,), -1, device=dev, dtype=torch.int32), s_top_id=z(R, K, dt=torch.int32),
                            s_top_lp=z(R, K))
        return self._lp

    def _lp_struct(self, decode: bool, nmax: int = TOP_LOGPROBS_MAX) -> ops.CainLogprob:
        b = self._lp_bufs()
        q = ops.CainLogprob()
        q.topn, q.nmax = _ptr(b["topn" if decode else "s_topn"]), int(nmax)
        if decode:
            assert b["lp"].stride(0) == self.gen.stride(0)
            q.lp, q.top_id, q.top_lp, q.keep = _ptr(b["lp"]), _ptr(b["top_id"]), _ptr(b["top_lp"]), _ptr(b["keep"])
        else:
            q.lp, q.top_id, q.top_lp, q.target = (_ptr(b["s_lp"]), _ptr(b["s_top_id"]), _ptr(b["s_top_lp"]),
                                                  _ptr(b["target"]))
        return q

    # ---------------------------------------------------------------- JSON mode
    def set_json_vocab(self, pieces: Sequence[bytes]) -> None:
        """The bytes each token id appends to the output, for JSON mode (``generate(format="json")``), instead of the
        tokenizer's own pieces: random-init tags have a synthetic tokenizer with no punctuation, so tests and
        benchmarks on random weights supply a vocabulary.  Ids past ``len(pieces)`` are empty (never allowed); the
        text of a JSON-mode row is then these bytes.  Raises ValueError when the vocabulary cannot spell JSON."""
        pieces = [bytes(p) for p in pieces]
        if len(pieces) > self.cfg.vocab:
            raise ValueError(f"{len(pieces)} pieces for a vocabulary of {self.cfg.vocab}")
        pieces += [b""] * (self.cfg.vocab - len(pieces))
        jsonmode.check_vocabulary(pieces)
        with self._json_lock:
            self._json_pieces, self._json_custom = pieces, True
        self._gr = self._st = None
        for key in [k for k in getattr(self, "_graphs", {}) if "gr" in k or "st" in k]:  # ... captured the old table
            self.lib.cain_graph_destroy(ctypes.c_void_p(self._graphs.pop(key)))

    def _json_vocab(self) -> List[bytes]:
        with self._json_lock:  # (a server's handler threads and its scheduler thread may both ask first)
            if self._json_pieces is None:
                pieces = self._pieces or jsonmode.token_bytes(self.tokenizer, self.cfg.vocab)
                jsonmode.check_vocabulary(pieces)
                self._json_pieces = self._pieces = pieces
            return self._json_pieces

    def _piece_vocab(self) -> List[bytes]:
        """The bytes each token id appends to a row's stream, for the stop sequences: ``set_json_vocab``'s pieces when
        given, else the tokenizer's own -- JSON mode's table without its ``check_vocabulary``, which only JSON needs."""
        with self._json_lock:
            if self._json_custom:
                return self._json_pieces
            if self._pieces is None:
                self._pieces = jsonmode.token_bytes(self.tokenizer, self.cfg.vocab)
            return self._pieces

    def _json_text(self, toks: Sequence[int]) -> str:
        return b"".join(self._json_pieces[t] for t in toks).decode("utf-8", errors="replace")

    def text_decoder(self, json_row: bool = False, stop_row: bool = False):
        """What turns a row's token ids into text (``.decode(ids)``): the tokenizer, or -- for a JSON-mode row or a
        row with stop strings of an engine whose vocabulary ``set_json_vocab`` supplied -- that vocabulary's bytes."""
        return _PieceDecoder(self) if (json_row or stop_row) and self._json_custom else self.tokenizer

    def stop_cut(self, toks: Sequence[int], text: str, hit_start: int) -> str:
        """``text`` (the decoder's text of all of ``toks``) of a row whose stop string starts at byte ``hit_start`` of
        its stream, cut there (engine/stopseq.py ``cut_text``)."""
        pieces = self._piece_vocab()
        return stopseq.cut_text(text, b"".join(pieces[t] if 0 <= t < len(pieces) else b"" for t in toks), hit_start)

    # ---------------------------------------------------------------- stop sequences
    def _st_bufs(self) -> Dict:
        """Device buffers of the stop sequences (csrc/stopseq.hip): per decode row the flag, the match state and the
        strings, and the vocabulary's piece table (JSON mode's tensors when it has made them: the same pieces)."""
        if self._st is None:
            R, dev = self.gen.shape[0], self.device
            pieces = self._piece_vocab()
            table = {k: self._gr[k] for k in ("V", "piece_off", "piece_bytes")} if self._gr is not None \
                else ops.json_table(pieces, dev)
            on, ln, by = ops.stop_table([()] * R, dev)
            self._st = dict(table, stop_on=on, stop_len=ln, stop_bytes=by,
                            sstate=ops.stop_states([stopseq.INITIAL] * R, dev))
        return self._st

    def _st_struct(self):
        b, q = self._st_bufs(), ops.CainStop()
        q.stop_on, q.sstate, q.stop_len, q.stop_bytes = (_ptr(b["stop_on"]), _ptr(b["sstate"]), _ptr(b["stop_len"]),
                                                         _ptr(b["stop_bytes"]))
        q.piece_off, q.piece_bytes = _ptr(b["piece_off"]), _ptr(b["piece_bytes"])
        return q

    def _st_begin(self, rows: slice, stops: Sequence[Sequence[str]]) -> None:
        """Decode rows ``rows`` start requests: their stop strings, every state at the start of a stream."""
        b = self._st_bufs()
        on, ln, by = ops.stop_table_host(stops)
        b["stop_on"][rows].copy_(on)
        b["stop_len"][rows].copy_(ln)
        b["stop_bytes"][rows].copy_(by)
        b["sstate"][rows].copy_(ops.stop_states([stopseq.INITIAL] * len(stops), "cpu"))

    def _st_hits(self, n: int, stops: Sequence[Sequence[str]]) -> List[Optional[tuple]]:
        """Per decode row ``0 .. n - 1``: ``(hit_start, index)`` of the stop string that ended it, or None."""
        st = ops.stop_states_host(self._st_bufs()["sstate"][:n])
        return [(s[3], s[4]) if stops[i] and s[3] >= 0 else None for i, s in enumerate(st)]

    def _gr_bufs(self) -> Dict:
        """Device buffers of JSON mode (csrc/grammar.hip): per decode row the mode flag and the automaton state, and
        the vocabulary's piece table."""
        if self._gr is None:
            R = self.gen.shape[0]
            self._gr = dict(ops.json_table(self._json_vocab(), self.device),
                            gram_on=torch.zeros(R, device=self.device, dtype=torch.int32),
                            gstate=torch.zeros(R, 4, device=self.device, dtype=torch.int32))
        return self._gr

    def _gr_struct(self):
        b, g = self._gr_bufs(), ops.CainGrammar()
        g.gram_on, g.gstate = _ptr(b["gram_on"]), _ptr(b["gstate"])
        g.piece_off, g.piece_bytes = _ptr(b["piece_off"]), _ptr(b["piece_bytes"])
        return g

    def _gr_begin(self, rows: slice, fmt: Sequence[bool]) -> None:
        """Decode rows ``rows`` start requests: JSON mode per ``fmt``, every state at the start of a document."""
        b = self._gr_bufs()
        b["gram_on"][rows].copy_(torch.tensor([int(f) for f in fmt], dtype=torch.int32))
        b["gstate"][rows].zero_()  # jsonmode.INITIAL

    def _gr_states(self, n: int, fmt: Sequence[bool]) -> List[Optional[str]]:
        names = {jsonmode.DONE: "done", jsonmode.FAIL: "fail"}
        st = ops.json_states_host(self._gr_bufs()["gstate"][:n])
        return [names.get(jsonmode.sid_of(s), "open") if f else None for s, f in zip(st, fmt)]

    @contextlib.contextmanager
    def _cu_budget(self):
        """Around every native call that launches or captures for this engine's stream: the launch sizing of a
        CU-limited engine (0: the whole device)."""
        self.lib.cain_set_cu_budget(self.cu_limit)
        try:
            yield
        finally:
            self.lib.cain_set_cu_budget(0)

    def _stream_h(self) -> ctypes.c_void_p:
        return ctypes.c_void_p(self.stream.cuda_stream)

    def _step(self, M: int, rows, want_logits: bool, want_sample: bool, lp: Optional[ops.CainLogprob] = None,
              gr: Optional[ops.CainGrammar] = None, st: Optional[ops.CainStop] = None,
              spec_mode: Optional[int] = None, pool: Optional[ops.CainPool] = None) -> ops.CainStep:
        """The call record of one step (csrc/cain_api.h CainStep): a forward over ``M`` rows with the given feature
        records, or -- ``spec_mode`` given (0: n-gram drafts, 1: the given drafts) -- a speculative step over ``M``
        sequences, whose drafts the draft model proposes where the engine has one.  The record points into the
        others, so it holds them (``keep``) for as long as it lives."""
        spec = spec_mode is not None
        s = ops.CainStep(plan=self._plan(M * (self.speculative + 1) if spec else M), M=M,
                         want_logits=int(want_logits), want_sample=int(want_sample))
        sp = sd = None
        if spec and self.draft is not None:
            s.draft2, s.draft1 = self.draft._plan(2 * M), self.draft._plan(M)
            sp, sd = ops.spec_struct(self._spec_bufs(), 1), ops.spec_draft_struct(self._spec_draft_bufs())
        elif spec:
            sp = ops.spec_struct(self._spec_bufs(), spec_mode)
        s.keep = (self._rows_struct(rows, bool(want_sample)), lp, gr, st, sp, sd, pool)
        for name, rec in zip(("rows", "lp", "gr", "st", "spec", "spec_draft", "pool"), s.keep):
            if rec is not None:
                setattr(s, name, ctypes.pointer(rec))
        return s

    def _forward(self, M: int, rows, want_logits: bool, want_sample: bool, lp: Optional[ops.CainLogprob] = None,
                 gr=None, st=None, pool: Optional[ops.CainPool] = None) -> None:
        step = self._step(M, rows, want_logits, want_sample, lp, gr, st, pool=pool)
        with self._cu_budget():
            ops.step_run(step, self._stream_h())

    def _captured(self, key: tuple, steps: int, make_step) -> int:
        """The cached graph ``key``: ``steps`` steps of ``make_step()``'s record, captured at first use."""
        g = self._graphs.get(key)
        if g is None:
            step = make_step()
            with self._cu_budget():
                g = self._graphs[key] = ops.step_capture(step, steps, self._stream_h())
        return g

    def _graph(self, M: int, steps: int, lp: bool = False, gr: bool = False, st: bool = False) -> int:
        """``lp``: the steps also compute token log-probabilities (for the rows whose ``topn`` says so when the graph
        runs) -- a cache entry of its own; without it the graph is launch for launch the one it always was.
        ``gr``: the steps run JSON mode's mask and advance (for the rows whose ``gram_on`` says so), likewise.
        ``st``: the steps match the stop sequences (for the rows whose ``stop_on`` says so), likewise."""
        key = (M, steps) + (("lp",) if lp else ()) + (("gr",) if gr else ()) + (("st",) if st else ())
        return self._captured(key, steps, lambda: self._step(
            M, self.rows, True, True, self._lp_struct(True) if lp else None, self._gr_struct() if gr else None,
            self._st_struct() if st else None))

    def _run_graphs(self, M: int, nsteps: int, lp: bool = False, gr: bool = False, st: bool = False,
                    spec_mode: Optional[int] = None) -> None:
        """``nsteps`` decode steps over the first ``M`` decode rows, replayed from the cached graphs: chunks of
        ``steps_per_graph`` steps, then the remainder as one-step graphs.  ``spec_mode`` given: speculative steps."""
        k, stream_h = self.steps_per_graph, self._stream_h()
        for n, count in ((k, nsteps // k), (1, nsteps % k)):
            if not count:
                continue
            g = self._graph_spec(M, n, spec_mode) if spec_mode is not None else self._graph(M, n, lp, gr, st)
            for _ in range(count):
                rc = self.lib.cain_graph_launch(ctypes.c_void_p(g), stream_h)
                if rc != 0:
                    raise RuntimeError(f"hipGraphLaunch failed rc={rc}")

    # ---------------------------------------------------------------- speculative decoding
    def _spec_bufs(self) -> Dict:
        """Device buffers of speculative decoding (csrc/spec.h), made when the mode first runs."""
        if self._spec is None:
            self._spec = ops.spec_alloc(self.max_batch, self.speculative, self.max_batch, self.T_max, self.cfg.vocab,
                                        self.device)
        return self._spec

    def _spec_begin(self, rows: Sequence[int], slots: Sequence[int], ids, drafts=None) -> None:
        """Decode rows ``rows`` start requests ``ids`` in cache slots ``slots``: their records hold the prompts, their
        counters start at zero, their given drafts (``drafts[i]``: ids by generated index, or None) are stored."""
        b = self._spec_bufs()
        rec = torch.zeros(len(ids), self.T_max, dtype=torch.int32)
        giv = torch.full((len(ids), self.T_max), -1, dtype=torch.int32)
        for i, p in enumerate(ids):
            rec[i, :len(p)] = torch.tensor(p, dtype=torch.int32)
            if drafts is not None and drafts[i] is not None:
                g = [int(t) for t in drafts[i]][: self.T_max]
                if any(t >= self.cfg.vocab for t in g):
                    raise ValueError(f"draft id outside the vocabulary ({self.cfg.vocab})")
                giv[i, :len(g)] = torch.tensor(g, dtype=torch.int32)
        ri = torch.tensor(list(rows), dtype=torch.long, device=self.device)
        b["seq"][torch.tensor(list(slots), dtype=torch.long, device=self.device)] = rec.to(self.device)
        b["given"][ri] = giv.to(self.device)
        for k in ("drafted", "accepted", "n_step"):
            b[k][ri] = 0
        if self.draft is not None:  # the draft cache of each slot: prompt[:-1], as the target's prefill
            dm = self.draft
            dm._forget_slots(slots)
            dm._prefill([[draft_token(t, dm.cfg.vocab, dm.cfg.bos_id) for t in p] for p in ids], list(slots))
            self._spec_draft_bufs()["dvalid"][torch.tensor(list(slots), dtype=torch.long, device=self.device)] = \
                torch.tensor([len(p) - 1 for p in ids], dtype=torch.int32).to(self.device)

    def _spec_draft_bufs(self) -> Dict:
        """Device buffers of draft-model mode (csrc/spec.h CainSpecDraft), made when the mode first runs."""
        if self._specd is None:
            self._specd = ops.spec_draft_alloc(self._spec_bufs(), self.draft.cfg.vocab, self.draft.cfg.bos_id)
        return self._specd

    def _spec_stats(self, row: int) -> Dict:
        """Counters of decode row ``row``: drafts proposed, drafts accepted, live steps, tokens per step."""
        b = self._spec_bufs()
        n = int(b["n_step"][row])
        return dict(draft_count=int(b["drafted"][row]), draft_accepted=int(b["accepted"][row]), decode_steps=n,
                    step_tokens=b["step_tokens"][row, :min(n, self.T_max)].cpu().tolist())

    def _forward_spec(self, B: int, mode: int) -> None:
        step = self._step(B, self.rows, True, True, spec_mode=mode)
        with self._cu_budget():
            ops.step_run(step, self._stream_h())

    def _graph_spec(self, B: int, steps: int, mode: int) -> int:
        """``steps`` speculative steps (draft -> verify forward over ``B (K + 1)`` rows -> accept) over ``B``
        sequences as one graph; cache entries of their own, beside the plain graphs."""
        key = (B, steps, "spec", "draft" if self.draft is not None else mode)
        return self._captured(key, steps, lambda: self._step(B, self.rows, True, True, spec_mode=mode))

    def close(self) -> None:
        if getattr(self, "draft", None) is not None:
            self.draft.close()
        lib = getattr(self, "lib", None)
        if lib is None:
            return
        for g in self._graphs.values():
            lib.cain_graph_destroy(ctypes.c_void_p(g))
        for p in self._plans.values():
            lib.cain_plan_destroy(ctypes.c_void_p(p))
        self._graphs, self._plans = {}, {}
        if getattr(self, "_cu_stream", None):
            self.stream.synchronize()
            lib.cain_stream_destroy(ctypes.c_void_p(self._cu_stream))
            self._cu_stream = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- generation
    def encode(self, prompt: Union[str, Sequence[int]]) -> List[int]:
        if isinstance(prompt, str):
            return self.tokenizer.encode(prompt)
        return [int(t) for t in prompt]

    def generate(self, prompts: Sequence[Union[str, Sequence[int]]], num_predict: Union[int, Sequence[int]] = 128,
                 options: Union[None, Dict, Sequence[Optional[Dict]]] = None, use_graph: bool = True,
                 on_tokens=None, context: Optional[Sequence[Optional[Sequence[int]]]] = None,
                 logprobs: Union[bool, Sequence[bool]] = False,
                 top_logprobs: Union[int, Sequence[int]] = 0,
                 drafts: Optional[Sequence[Optional[Sequence[int]]]] = None,
                 format: Union[None, str, Sequence[Optional[str]]] = None) -> List[GenResult]:
        """Generate for a batch of prompts (ids or text).  ``on_tokens(list_per_row)`` streams newly
        generated ids every ``steps_per_graph`` decode steps (and stops early once every row is done).
        ``context[i]``: token ids prepended to row i's encoded prompt (Ollama's ``context`` of an earlier answer).
        ``logprobs`` (one flag or one per row): each result carries the log-probability of every generated token --
        the natural-log softmax of the model's own logits, temperature 1, before the repeat penalty and top-k /
        top-p -- and the ``top_logprobs`` (0 .. 20) most likely ``(id, logprob)`` of that distribution per token,
        logit descending, index ascending on ties.  On the HIP backend both are computed on the device inside the
        decode graphs (csrc/logprob.hip); the tokens are the same with and without.  With logprobs asked for,
        ``on_tokens`` gets a second argument: per row ``(logprobs, top_logprobs)`` of the new tokens, or None.
        ``drafts`` (speculative engines): per row the draft token of every generated index (a negative id ends a
        step's draft; None: no drafts for that row); this call then verifies these instead of the n-gram lookup's.
        ``format="json"`` (one value or one per row; or the per-row option key ``"format"``): Ollama's JSON mode --
        the row's generated tokens are constrained, step by step, to those whose bytes continue an RFC 8259 document
        whose top-level value is an object (engine/jsonmode.py; on the HIP backend a mask on the logits inside the
        decode graphs, csrc/grammar.hip).  The row ends on the token that closes the object (``done_reason`` "stop",
        no EOS needed); a row whose budget runs out first holds a viable prefix ("length").  The state starts fresh
        per request; the prompt is not constrained.  Not together with speculative decoding.
        ``options["stop"]`` (a string or up to 8 strings of up to 32 UTF-8 bytes): Ollama's stop sequences
        (engine/stopseq.py; on the HIP backend matched on the sampled tokens' bytes inside the decode graphs,
        csrc/stopseq.hip).  The row ends on the token that completes a stop string (``done_reason`` "stop",
        ``stop_hit`` names the string); ``tokens`` keeps that token, ``text`` is cut where the string starts.  Not
        together with speculative decoding; the three stop token **ids** are ``options["stop_ids"]``."""
        prompts = list(prompts)
        B = len(prompts)
        if B == 0:
            return []
        want = _want_logprobs(logprobs, top_logprobs, B)
        opts = list(options) if isinstance(options, (list, tuple)) else [options] * B
        fmt = _want_format(format, opts, B)
        if self.speculative and any(fmt):
            raise ValueError("format cannot be combined with speculative decoding (the K + 1 expanded rows would "
                             "each need the state after their drafts)")
        if any(fmt):
            self._json_vocab()  # (ValueError: the vocabulary cannot spell JSON)
        if self.speculative and any(w >= 0 for w in want):
            raise ValueError("logprobs cannot be combined with speculative decoding")
        if drafts is not None and not self.speculative:
            raise ValueError("drafts need an engine with speculative > 0")
        if drafts is not None and self.draft is not None:
            raise ValueError("drafts cannot be combined with a draft model (the draft model writes the drafts)")
        if drafts is not None and len(drafts) != B:
            raise ValueError(f"{len(drafts)} drafts for {B} prompts")
        if B > self.max_batch:
            out = []
            for i in range(0, B, self.max_batch):
                sl = slice(i, i + self.max_batch)
                nps = num_predict[sl] if not isinstance(num_predict, int) else num_predict
                ops_ = options[sl] if isinstance(options, (list, tuple)) else options
                out += self.generate(prompts[sl], nps, ops_, use_graph, on_tokens,
                                     context[sl] if context is not None else None,
                                     [w >= 0 for w in want[sl]], [max(w, 0) for w in want[sl]],
                                     drafts[sl] if drafts is not None else None,
                                     ["json" if f else None for f in fmt[sl]])
            return out
        if context is not None and len(context) != B:
            raise ValueError(f"{len(context)} contexts for {B} prompts")
        ids = [([int(t) for t in context[i]] if context is not None and context[i] else []) + self.encode(p)
               or [self.cfg.bos_id] for i, p in enumerate(prompts)]
        nps = [int(num_predict)] * B if isinstance(num_predict, int) else [int(x) for x in num_predict]
        row_opts = [_row_options(o, self.cfg, i, self.seed) for i, o in enumerate(opts)]
        if self.speculative and any(o["stop_strs"] for o in row_opts):
            raise ValueError(SPEC_STOP_REFUSAL)
        if self.speculative and any(ext_active(o) for o in row_opts):
            raise ValueError(SPEC_EXT_REFUSAL)
        for i in range(B):
            budget = self.T_max - len(ids[i])
            if budget < 1:
                raise ValueError(f"prompt of {len(ids[i])} tokens exceeds the context ({self.T_max})")
            nps[i] = max(1, min(nps[i], budget))
        t0 = time.perf_counter_ns()
        lps = None  # per row (logprobs, top_logprobs) or None
        self._last_spec = None
        self._last_json = None
        self._last_stop = None
        if self.backend == "torch" and self.speculative:
            gen, t_pref, t_dec = self._generate_torch_spec(ids, nps, row_opts, drafts)
            if on_tokens is not None:
                on_tokens(gen)
        elif self.backend == "torch":
            gen, t_pref, t_dec, lps = self._generate_torch(ids, nps, row_opts, want, fmt)
            if on_tokens is not None:
                on_tokens(gen, lps) if lps is not None else on_tokens(gen)
        else:
            gen, t_pref, t_dec, lps = self._generate_hip(ids, nps, row_opts, use_graph, on_tokens, want=want,
                                                         drafts=drafts, fmt=fmt)
        total = time.perf_counter_ns() - t0
        load = self.load_duration_ns if self._first_call else 0
        self._first_call = False
        steps = max(nps)
        self.last_prefill_ns, self.last_decode_ns = t_pref, t_dec
        out = []
        for i in range(B):
            toks = gen[i]
            js = self._last_json[i] if self._last_json is not None else None
            hit = self._last_stop[i] if self._last_stop is not None else None
            reason = "stop" if _stopped(toks, row_opts[i]) or js == "done" or hit is not None else "length"
            text = self.text_decoder(js is not None, bool(row_opts[i]["stop_strs"])).decode(toks)
            if hit is not None:
                text = self.stop_cut(toks, text, hit[0])
            out.append(GenResult(self.cfg.name, ids[i], toks, text, reason, json_state=js,
                                 stop_hit=row_opts[i]["stop_strs"][hit[1]] if hit is not None else None,
                                 load_duration_ns=load, prompt_eval_duration_ns=t_pref,
                                 eval_duration_ns=int(t_dec * len(toks) / max(1, steps)),
                                 total_duration_ns=total + load))
            if lps is not None and lps[i] is not None:
                out[-1].logprobs, out[-1].top_logprobs = lps[i]
            if self._last_spec is not None:
                for k, v in self._last_spec[i].items():
                    setattr(out[-1], k, v)
        return out

    def _read_logprobs(self, row: int, lo: int, hi: int, n: int):
        """(logprobs, top_logprobs) of tokens ``lo .. hi - 1`` of decode row ``row`` from the device rings."""
        b = self._lp_bufs()
        if hi <= lo:
            return [], []
        lp = b["lp"][row, lo:hi].cpu().tolist()
        if n <= 0:
            return lp, [[] for _ in lp]
        ti, tl = b["top_id"][row, lo:hi, :n].cpu().tolist(), b["top_lp"][row, lo:hi, :n].cpu().tolist()
        return lp, [list(zip(a, c)) for a, c in zip(ti, tl)]

    def _generate_hip(self, ids, nps, row_opts, use_graph, on_tokens=None, check_every: int = 1, want=None,
                      drafts=None, fmt=None):
        dev = self.device
        B = len(ids)
        with_lp = want is not None and any(w >= 0 for w in want)
        with_gr = fmt is not None and any(fmt)  # some row in JSON mode: the graphs with the mask and the advance
        stops = [o["stop_strs"] for o in row_opts]
        with_st = any(stops)  # some row has stop strings: the graphs with the match after the sampler
        spec = self.speculative > 0  # K + 1 rows per sequence and step: speculative graphs, done polled per chunk
        spec_mode = int(drafts is not None)
        self._forget_slots(range(B))
        with torch.cuda.stream(self.stream):
            # ---- prefill: all prompt tokens except the last, in <=prefill_chunk-row chunks
            t0 = time.perf_counter_ns()
            self._prefill(ids)
            # ---- decode rows
            r = self.rows
            r["tok"][:B].copy_(torch.tensor([p[-1] for p in ids], dtype=torch.int32))
            r["pos"][:B].copy_(torch.tensor([len(p) - 1 for p in ids], dtype=torch.int32))
            r["slot"][:B].copy_(torch.arange(B, dtype=torch.int32))
            r["n_gen"][:B].zero_()
            r["done"][:B].zero_()
            r["max_new"][:B].copy_(torch.tensor(nps, dtype=torch.int32))
            self.sample_params[: ops.SAMPLE_BYTES * B].copy_(ops.sample_params_tensor(row_opts, "cpu").to(dev))
            self.sample_ext[: ops.SAMPLE_EXT_BYTES * B].copy_(ops.sample_ext_tensor(row_opts, "cpu").to(dev))
            lq = None
            if with_lp:
                self._lp_bufs()["topn"][:B].copy_(torch.tensor(want, dtype=torch.int32))
                lq = self._lp_struct(True, max(want))
            if spec:
                self._spec_begin(range(B), range(B), ids, drafts)
            gq = None
            if with_gr:
                self._gr_begin(slice(0, B), fmt)
                gq = self._gr_struct()
            sq = None
            if with_st:
                self._st_begin(slice(0, B), stops)
                sq = self._st_struct()
            self.stream.synchronize()
            t1 = time.perf_counter_ns()
            steps = max(nps)
            feats = {k: v for k, v in (("lp", lq), ("gr", gq), ("st", sq)) if v is not None}

            def launch(nsteps: int) -> None:
                if use_graph:
                    self._run_graphs(B, nsteps, with_lp, with_gr, with_st, spec_mode if spec else None)
                    return
                for _ in range(nsteps):
                    if spec:
                        self._forward_spec(B, spec_mode)
                    else:  # (without a feature, the call it always was: wrappers of _forward see the same arguments)
                        self._forward(B, r, want_logits=True, want_sample=True, **feats)

            # first token on its own so time-to-first-token is measured exactly
            launch(1)
            self.stream.synchronize()
            t_first = time.perf_counter_ns()
            done_steps = 1
            emitted = [0] * B
            # (speculative: a step commits up to K + 1 tokens, so rows finish in fewer steps than tokens)
            # (JSON mode: a row ends when its object closes; stop sequences: when a string completes)
            watch = spec or with_gr or with_st or on_tokens is not None or \
                any(o["eos_id"] >= 0 or o["stop"] for o in row_opts)
            chunk = self.steps_per_graph * max(1, int(check_every))

            def emit(new, ng) -> None:
                if with_lp:
                    on_tokens(new, [self._read_logprobs(i, emitted[i], ng[i], want[i]) if want[i] >= 0 else None
                                    for i in range(B)])
                else:
                    on_tokens(new)
                for i in range(B):
                    emitted[i] = ng[i]

            def poll() -> bool:
                ng = r["n_gen"][:B].cpu().tolist()
                if on_tokens is not None:
                    emit([self.gen[i, emitted[i]: ng[i]].cpu().tolist() if ng[i] > emitted[i] else []
                          for i in range(B)], ng)
                return bool(r["done"][:B].all())

            if watch and poll():
                done_steps = steps
            while done_steps < steps:
                n = min(chunk if watch else steps, steps - done_steps)
                launch(n)
                done_steps += n
                if watch and done_steps < steps and poll():
                    break
            n_gen = r["n_gen"][:B].cpu().tolist()
            gen = self.gen[:B].cpu()
            if on_tokens is not None:
                emit([gen[i, emitted[i]: n_gen[i]].tolist() for i in range(B)], n_gen)
            lps = [self._read_logprobs(i, 0, n_gen[i], want[i]) if want[i] >= 0 else None
                   for i in range(B)] if with_lp else None
            if spec:
                self._last_spec = [self._spec_stats(i) for i in range(B)]
            if with_gr:
                self._last_json = self._gr_states(B, fmt)
            if with_st:
                self._last_stop = self._st_hits(B, stops)
            t2 = time.perf_counter_ns()
        self.last_ttft_ns = t_first - t0
        return [gen[i, : n_gen[i]].tolist() for i in range(B)], t1 - t0, t2 - t1, lps

    @torch.no_grad()
    def last_logits(self, prompts: Sequence[Union[str, Sequence[int]]]) -> torch.Tensor:
        """fp32 logits [B, V] of the next token after each prompt (numerics tests / debugging)."""
        ids = [self.encode(p) for p in prompts]
        B = len(ids)
        if self.backend == "torch":
            return torch.stack([self.ref.forward(torch.tensor([p], device=self.device))[0, -1] for p in ids])
        assert B <= self.max_batch
        self._forget_slots(range(B))
        with torch.cuda.stream(self.stream):
            self._prefill(ids)
            r = self.rows
            r["tok"][:B].copy_(torch.tensor([p[-1] for p in ids], dtype=torch.int32))
            r["pos"][:B].copy_(torch.tensor([len(p) - 1 for p in ids], dtype=torch.int32))
            r["slot"][:B].copy_(torch.arange(B, dtype=torch.int32))
            self._forward(B, r, want_logits=True, want_sample=False)
            out = self.buf["logits"][:B].clone()
            self.stream.synchronize()
        return out

    @torch.no_grad()
    def score(self, prompts: Sequence[Union[str, Sequence[int]]], top_logprobs: int = 0) -> List[ScoreResult]:
        """Teacher-forced log-probabilities: for each prompt (ids or text) of n tokens the logprob of tokens
        1 .. n - 1, token j scored by the logits at position j - 1 (same definition as ``generate(logprobs=True)``),
        with the ``top_logprobs`` most likely alternatives per position.  HIP backend: the prefill forward with the
        LM head, log-softmax and the target's logprob on the device per chunk (csrc/logprob.hip); the cache slots it
        writes lose their prefix-cache records.  Torch backend: float64 log-softmax of the oracle's logits."""
        n_top = int(top_logprobs or 0)
        if not 0 <= n_top <= TOP_LOGPROBS_MAX:
            raise ValueError(f"top_logprobs must be in 0..{TOP_LOGPROBS_MAX}, got {n_top}")
        ids = [self.encode(p) or [self.cfg.bos_id] for p in prompts]
        for p in ids:
            if len(p) > self.T_max:
                raise ValueError(f"prompt of {len(p)} tokens exceeds the context ({self.T_max})")
        out: List[ScoreResult] = []
        if self.backend == "torch":
            for p in ids:
                res = ScoreResult(list(p), [], [])
                if len(p) > 1:
                    lg = self.ref.forward(torch.tensor([p], device=self.device))[0].float().cpu()
                    for j in range(1, len(p)):
                        ls, top = logprob_host(lg[j - 1], n_top)
                        res.logprobs.append(float(ls[p[j]]))
                        res.top_logprobs.append(top)
                out.append(res)
            return out
        for i in range(0, len(ids), self.max_batch):
            group = ids[i:i + self.max_batch]
            self._forget_slots(range(len(group)))
            with torch.cuda.stream(self.stream):
                lps, tops = self._prefill(group, score_top=n_top)
            at = 0
            for p in group:
                n = len(p) - 1
                out.append(ScoreResult(list(p), lps[at:at + n], tops[at:at + n]))
                at += n
        return out

    # ---------------------------------------------------------------- embeddings
    def _pool_bufs(self) -> Dict[str, torch.Tensor]:
        """Device buffers of embedding pooling (csrc/pool.hip), made at first use: the fp32 final gain -- the model's
        own, unfolded, whatever the weight format -- the accumulators, counts and results per cache slot, and per
        prefill row the RMSNorm scale and the run table."""
        if self._pool is None:
            dev, d, R = self.device, self.cfg.d_model, self.prefill_rows["tok"].shape[0]
            z = lambda *s, dt=torch.float32: torch.zeros(*s, device=dev, dtype=dt)  # noqa: E731
            self._pool = dict(gain=self._packed["final_gain"].to(dev).float().contiguous(), acc=z(self.max_batch, d),
                              cnt=z(self.max_batch, dt=torch.int32), out=z(self.max_batch, d), rinv=z(R),
                              seg_off=z(R + 1, dt=torch.int32), seg_dst=z(R, dt=torch.int32))
        return self._pool

    def _pool_struct(self, runs: int, mode: int) -> ops.CainPool:
        b = self._pool_bufs()
        return ops.CainPool(gain=_ptr(b["gain"]), seg_off=_ptr(b["seg_off"]), seg_dst=_ptr(b["seg_dst"]),
                            acc=_ptr(b["acc"]), cnt=_ptr(b["cnt"]), rinv=_ptr(b["rinv"]), S=runs, mode=mode)

    @torch.no_grad()
    def embed(self, prompts: Sequence[Union[str, Sequence[int]]], pooling: str = "last", normalize: bool = True,
              truncate: bool = True, slots: Optional[Sequence[int]] = None) -> List[EmbedResult]:
        """Embeddings of prompts (ids or text, encoded as ``generate`` encodes them; an empty prompt embeds
        ``[bos_id]``).  The hidden state of a prompt of n tokens is the residual stream after the last layer at each
        position under the model's own final RMSNorm with its own gain (``weights.final_gain``: Gemma's 1 + w
        included) -- what the LM head multiplies, before any fold.  ``pooling="last"``: the vector at position n - 1;
        ``"mean"``: the fp32 sum over positions 0 .. n - 1 in ascending order, divided by n.  ``normalize``: the
        pooled vector is L2-normalised.  ``truncate``: a prompt beyond the context keeps its first ``T_max`` tokens
        (``truncated`` says so); without it such a prompt raises ValueError.
        HIP backend: all n tokens go through prefill chunks, each carrying the pool record (csrc/pool.hip), then one
        finishing launch and one copy of the vectors: no LM head, no sampler, no decode forward.  It writes cache slots
        ``slots`` (default 0 .. B - 1 per pass of up to ``max_batch`` prompts), whose prefix-cache records die; on a
        speculative engine the forward is a plain one and the draft cache is not written.  Torch backend: the
        oracle's ``hidden``, pooled in fp32."""
        if pooling not in POOLINGS:
            raise ValueError(f"pooling must be one of {POOLINGS}, got {pooling!r}")
        ids, cut = [], []
        for p in prompts:
            t = self.encode(p) or [self.cfg.bos_id]
            if len(t) > self.T_max and not truncate:
                raise ValueError(f"input of {len(t)} tokens exceeds the context ({self.T_max}) and truncate is off")
            cut.append(len(t) > self.T_max)
            ids.append(t[: self.T_max])
        if self.backend == "torch":
            vecs = []
            for p in ids:
                h = self.ref.hidden(torch.tensor([p], device=self.device))[0].float()
                if pooling == "last":
                    v = h[-1]
                else:
                    v = torch.zeros_like(h[0])
                    for j in range(h.shape[0]):  # ascending position order, as the kernel
                        v = v + h[j]
                    v = v / float(h.shape[0])
                if normalize:
                    nrm = v.pow(2).sum().sqrt()
                    v = v / nrm if float(nrm) > 0 else v
                vecs.append(v.cpu().tolist())
        else:
            width = self.max_batch if slots is None else len(slots)
            if width < 1:
                raise ValueError("embed needs at least one cache slot")
            mode = ops.POOL_MODES[pooling]
            vecs = []
            for i in range(0, len(ids), width):
                group = ids[i:i + width]
                use = list(range(len(group))) if slots is None else [int(s) for s in slots[:len(group)]]
                self._forget_slots(use)
                b = self._pool_bufs()
                with torch.cuda.stream(self.stream):
                    b["acc"].zero_()
                    b["cnt"].zero_()
                    if self._specd is not None:  # the draft cache no longer continues what these slots hold
                        self._specd["dvalid"][torch.tensor(use, dtype=torch.long, device=self.device)] = 0
                    self._prefill(group, use, pool_mode=mode)
                    with self._cu_budget():
                        rc = ops.pool_finish(b["acc"], b["cnt"], b["out"], normalize)
                    if rc != 0:
                        raise RuntimeError(f"cain_pool_finish failed (rc={rc})")
                    out = b["out"][:len(group)].cpu()
                    self.stream.synchronize()
                vecs += out.tolist()
        return [EmbedResult(v, len(p), c) for v, p, c in zip(vecs, ids, cut)]

    def _forget_slots(self, slots) -> None:
        """These slots are about to be written outside the continuous batch's bookkeeping: their records die."""
        for s in slots:
            self.slot_tokens[s] = []

    def _prefill(self, ids, slots: Optional[Sequence[int]] = None, start: Optional[Sequence[int]] = None,
                 score_top: Optional[int] = None, pool_mode: Optional[int] = None):
        """All prompt tokens but the last through the forward, into KV-cache slot ``slots[b]`` (default b).
        ``pool_mode`` (``embed``; ops.POOL_*): the last token goes through too, and every chunk carries the pool
        record -- its runs are the chunk's stretches of one prompt each, accumulated into row b of the pool buffers
        (``last``: only the runs that end a prompt).
        ``start[b]``: row b's slot already holds positions ``< start[b]`` of this prompt; tokens
        ``ids[b][start[b]:-1]`` go in at positions ``start[b] ..`` (default: everything from 0).
        ``score_top`` (``score``): every chunk also runs the LM head and scores each row's next token on the device,
        with that many alternatives; returns the flat rows' (logprobs, top_logprobs)."""
        flat_tok, flat_pos, flat_slot, flat_next, flat_seq = [], [], [], [], []
        for b, p in enumerate(ids):
            j0 = 0 if start is None else int(start[b])
            for j in range(j0, len(p) - (pool_mode is None)):
                flat_tok.append(p[j])
                flat_pos.append(j)
                flat_slot.append(b if slots is None else int(slots[b]))
                flat_next.append(p[j + 1] if j + 1 < len(p) else -1)
                flat_seq.append(b)
        lps: List[float] = []
        tops: List[List[tuple]] = []
        self.prefill_rows_total += len(flat_tok)
        pr = self.prefill_rows
        for c in range(0, len(flat_tok), self.prefill_chunk):
            n = min(self.prefill_chunk, len(flat_tok) - c)
            pr["tok"][:n].copy_(torch.tensor(flat_tok[c:c + n], dtype=torch.int32))
            pr["pos"][:n].copy_(torch.tensor(flat_pos[c:c + n], dtype=torch.int32))
            pr["slot"][:n].copy_(torch.tensor(flat_slot[c:c + n], dtype=torch.int32))
            if pool_mode is not None:
                # the chunk's runs: [c + off[s], c + off[s + 1]) are consecutive positions of prompt dst[s]
                off = [0] + [j for j in range(1, n) if flat_seq[c + j] != flat_seq[c + j - 1]] + [n]
                dst = [flat_seq[c + o] for o in off[:-1]]
                # `last` takes only the runs that end their prompt: every run but the chunk's final one does
                if pool_mode == ops.POOL_LAST and flat_pos[c + n - 1] != len(ids[dst[-1]]) - 1:
                    off, dst = off[:-1], dst[:-1]
                pb = self._pool_bufs()
                if dst:
                    pb["seg_off"][:len(off)].copy_(torch.tensor(off, dtype=torch.int32))
                    pb["seg_dst"][:len(dst)].copy_(torch.tensor(dst, dtype=torch.int32))
                self._forward(n, pr, want_logits=False, want_sample=False,
                              pool=self._pool_struct(len(dst), pool_mode) if dst else None)
                continue
            if score_top is None:
                self._forward(n, pr, want_logits=False, want_sample=False)
                continue
            b = self._lp_bufs()
            b["target"][:n].copy_(torch.tensor(flat_next[c:c + n], dtype=torch.int32))
            b["s_topn"][:n].fill_(score_top)
            self._forward(n, pr, want_logits=True, want_sample=False, lp=self._lp_struct(False, score_top))
            lps += b["s_lp"][:n].cpu().tolist()
            if score_top > 0:
                ti, tl = b["s_top_id"][:n, :score_top].cpu().tolist(), b["s_top_lp"][:n, :score_top].cpu().tolist()
                tops += [list(zip(a, v)) for a, v in zip(ti, tl)]
            else:
                tops += [[] for _ in range(n)]
        if score_top is not None:
            return lps, tops

    # ------------------------------------------------------------ continuous batching
    def continuous(self) -> "ContinuousBatch":
        """A persistent decode batch that requests join and leave between graph chunks (the server's
        continuous batching, serve/server.py); HIP backend only."""
        if self.backend != "hip":
            raise RuntimeError("continuous batching needs the hip backend")
        return ContinuousBatch(self)

    def _generate_torch(self, ids, nps, row_opts, want=None, fmt=None):
        """Oracle backend with a KV cache (one token of compute per step), sampled on the host; logprobs (``want``
        per row: -1 or the number of alternatives) by ``logprob_host`` of the same logits.  JSON mode (``fmt`` per
        row): the Python automaton masks the logits before the sampler with the device's values and ends the row by
        the device's rule (engine/jsonmode.py).  Stop sequences (``row_opts[i]["stop_strs"]``): the Python rule
        (engine/stopseq.py) over each token's piece, after JSON mode's advance."""
        t0 = time.perf_counter_ns()
        gens = []
        with_st = any(o["stop_strs"] for o in row_opts)
        spieces = self._piece_vocab() if with_st else None
        hits: List[Optional[tuple]] = [None] * len(ids)
        with_gr = fmt is not None and any(fmt)
        pieces = self._json_vocab() if with_gr else None
        jstates: List[Optional[str]] = [None] * len(ids)
        with_lp = want is not None and any(w >= 0 for w in want)
        lps: list = [([], []) if with_lp and want[i] >= 0 else None for i in range(len(ids))]
        for i, p in enumerate(ids):
            o = row_opts[i]
            rng = np.random.default_rng(o["seed"])
            out = []
            cache: list = []
            step = torch.tensor([list(p)], device=self.device)
            js = jsonmode.INITIAL if with_gr and fmt[i] else None
            sstops, ss = stopseq.stop_bytes(o["stop_strs"]), stopseq.INITIAL
            for _ in range(nps[i]):
                logits = self.ref.forward(step, cache=cache, last_only=True)[0, -1].float().cpu()
                if js is None:
                    nxt = sample_host(logits, out, o, rng)
                else:  # (logprobs below stay those of the raw logits)
                    masked = jsonmode.mask_logits_host(logits.numpy().copy(), js, pieces)
                    nxt = sample_host(torch.from_numpy(masked), out, o, rng)
                    js, ok = jsonmode.advance(js, pieces[nxt])
                    if not ok:  # a masked token drawn: taken back, the row ends
                        break
                if lps[i] is not None:
                    ls, top = logprob_host(logits, want[i])
                    lps[i][0].append(float(ls[nxt]))
                    lps[i][1].append(top)
                out.append(nxt)
                step = torch.tensor([[nxt]], device=self.device)
                if sstops:
                    ss, _ = stopseq.advance(ss, spieces[nxt], sstops)
                if _stopped(out, o) or (js is not None and jsonmode.sid_of(js) == jsonmode.DONE) or ss[3] >= 0:
                    break
            if js is not None:
                jstates[i] = {jsonmode.DONE: "done", jsonmode.FAIL: "fail"}.get(jsonmode.sid_of(js), "open")
            if ss[3] >= 0:
                hits[i] = (ss[3], ss[4])
            gens.append(out)
        if with_st:
            self._last_stop = hits
        if with_gr:
            self._last_json = jstates
        t1 = time.perf_counter_ns()
        return gens, 0, t1 - t0, lps if with_lp else None

    def _generate_torch_spec(self, ids, nps, row_opts, drafts=None):
        """The oracle backend under the speculative rule (engine/speculative.py): per step the drafts of the host
        rule, one oracle forward over the K + 1 rows, the host sampler per row, the host accept.  The random stream
        is numpy's, one draw per sampled token, so each row samples from the generator state plain decoding has at
        its generated index and the state is set back to the one after the last committed token.  With a draft model
        the drafts are its own: its forwards on a cache of its own, sampled from the state the step starts in."""
        t0 = time.perf_counter_ns()
        K, V = self.speculative, self.cfg.vocab
        gens, stats = [], []
        for i, p in enumerate(ids):
            o = row_opts[i]
            rng = np.random.default_rng(o["seed"])
            given = drafts[i] if drafts is not None and drafts[i] is not None else None
            st = SeqState(tok=p[-1], pos=len(p) - 1, max_new=nps[i], eos_id=o["eos_id"], stop=o["stop"], seq=list(p))
            cache: list = []
            fed = 0  # positions the cache holds
            dm, dcache, dvalid = self.draft, [], len(p) - 1
            if dm is not None and len(p) > 1:  # the draft cache: prompt[:-1]
                dm.ref.forward(torch.tensor([[draft_token(t, dm.cfg.vocab, dm.cfg.bos_id) for t in p[:-1]]],
                                            device=self.device), cache=dcache)
            while not st.done:
                pos0, d = st.pos, 0
                if dm is not None:
                    # the draft model's forwards, sampled from the generator state the target rows start from
                    d, catch_up, own = draft_model_rows(st.seq, st.pos, st.n_gen, K, self.T_max, st.max_new, dvalid,
                                                        dm.cfg.vocab, dm.cfg.bos_id)
                    state0, dj, feed = rng.bit_generator.state, [], [r[0] for r in (catch_up, own) if r[2] >= 0]
                    for _ in range(d):
                        lg = dm.ref.forward(torch.tensor([feed], device=self.device), cache=dcache,
                                            last_only=True)[0, -1].float().cpu()
                        dj.append(sample_host(lg, st.gen + dj, o, rng))
                        feed = [draft_token(dj[-1], dm.cfg.vocab, dm.cfg.bos_id)]
                    rng.bit_generator.state = state0
                    given = [-1] * self.T_max
                    draft_model_given(given, st.n_gen, dj, K)
                dr = spec_draft_host(st.seq, st.pos, st.n_gen, K, self.T_max, st.max_new,
                                     given=[] if drafts is not None and given is None else given, vocab=V)
                step = torch.tensor([st.seq[fed: st.pos + 1] + dr], device=self.device)
                logits = self.ref.forward(step, cache=cache)[0, -(len(dr) + 1):].float().cpu()
                sampled, states = [], [rng.bit_generator.state]
                for j in range(len(dr) + 1):
                    sampled.append(sample_host(logits[j], st.gen + dr[:j], o, rng))
                    states.append(rng.bit_generator.state)
                c = st.commit_step(dr, sampled, self.T_max)
                rng.bit_generator.state = states[c]
                fed = st.pos
                for li in range(len(cache)):  # rejected rows leave the cache
                    cache[li] = [cache[li][0][:, :fed], cache[li][1][:, :fed]]
                if d > 0:
                    dvalid = dvalid_after(pos0, d, st.pos)
                    for li in range(len(dcache)):
                        dcache[li] = [dcache[li][0][:, :dvalid], dcache[li][1][:, :dvalid]]
            gens.append(list(st.gen))
            stats.append(dict(draft_count=st.drafted, draft_accepted=st.accepted, decode_steps=len(st.step_tokens),
                              step_tokens=list(st.step_tokens)))
        self._last_spec = stats
        return gens, 0, time.perf_counter_ns() - t0


SAMPLE_TOPK_MAX = 256  # the kernels' top-k clamp (csrc/sample.hip SS_KMAX): top_k <= 0 or above it means this many
SAMPLE_HIST = 64       # ids the repeat penalty can look back on (csrc/sample.hip HIST)


def sample_host_candidates(logits: torch.Tensor, history: List[int], o: Dict):
    """What the samplers of csrc/sample.hip draw from, computed on the host: ``(ids, probs, cut)`` -- the top-k
    candidate ids after the repeat penalty (value descending, index ascending; the penalty in float32, each distinct
    recent id inside the vocabulary once), their probabilities at the temperature (float64, normalised over the
    candidates) and the number of leading candidates the cut keeps (the shorter of the top-p prefix -- the smallest
    whose cumulative probability is >= top_p -- and the ``min_p`` prefix).  The penalty stage follows sample.hip's
    header: the repeat penalty, then ``v - fmaf(count, frequency_penalty, presence_penalty)`` with the id's count in
    the window; the three further keys may be absent (neutral).  Greedy (temperature <= 0): the argmax alone, the
    lowest index on ties; ``min_p`` is ignored."""
    lg = logits.detach().to(torch.float32).cpu().numpy().copy()
    V = lg.shape[0]
    rp = np.float32(o["repeat_penalty"])
    pp, fp = np.float32(o.get("presence_penalty", 0.0)), np.float32(o.get("frequency_penalty", 0.0))
    ext = pp != np.float32(0.0) or fp != np.float32(0.0)
    if (rp != np.float32(1.0) or ext) and o["repeat_last_n"] > 0:
        n = min(int(o["repeat_last_n"]), SAMPLE_HIST, len(history))
        window = history[len(history) - n:]
        for t in set(window):
            if 0 <= t < V:
                v = lg[t]
                if rp != np.float32(1.0):
                    v = np.float32(v / rp) if v > 0 else np.float32(v * rp)
                if ext:  # v - fmaf(count, frequency, presence): the product and sum rounded once, then the difference
                    v = np.float32(v - np.float32(np.float64(window.count(t)) * np.float64(fp) + np.float64(pp)))
                lg[t] = v
    if o["temperature"] <= 0:
        return np.array([int(np.argmax(lg))]), np.ones(1), 1
    k = o["top_k"] if 0 < o["top_k"] <= SAMPLE_TOPK_MAX else SAMPLE_TOPK_MAX
    k = min(k, V)
    cand = np.flatnonzero(lg >= np.partition(lg, V - k)[V - k])  # every element >= the k-th largest (ties included)
    ids = cand[np.lexsort((cand, -lg[cand].astype(np.float64)))][:k]  # value descending, index ascending
    vals = lg[ids].astype(np.float64)
    p = np.exp((vals - vals[0]) * np.float64(np.float32(1.0) / np.float32(o["temperature"])))
    p /= p.sum()
    cut = len(ids)
    top_p = np.float64(np.float32(o["top_p"]))
    if 0 < top_p < 1:
        cut = min(int(np.searchsorted(np.cumsum(p), top_p, side="left")) + 1, len(ids))
    min_p = np.float64(np.float32(o.get("min_p", 0.0)))
    if min_p > 0:  # the prefix with exp((v_i - v_0) / T) >= min_p (p[i] / p[0]: the same ratio), candidate 0 always
        cut = min(cut, max(1, int(np.count_nonzero(p / p[0] >= min_p))))
    return ids, p, cut


def sample_host(logits: torch.Tensor, history: List[int], o: Dict, rng) -> int:
    """Host mirror of csrc/sample.hip: the same candidates, order, probabilities and top-p cut
    (sample_host_candidates); only the random stream differs (numpy's, the kernels hash seed and token index)."""
    ids, p, cut = sample_host_candidates(logits, history, o)
    if o["temperature"] <= 0:
        return int(ids[0])
    p = p[:cut] / p[:cut].sum()
    return int(ids[int(rng.choice(cut, p=p))])


class ContinuousBatch:
    """Rows ``[0, n)`` of the engine's decode state are the live requests; each owns a KV-cache slot for its
    lifetime (``slot`` column), so rows can be compacted when requests leave while their caches stay put.

    * ``admit(prompts, num_predict, options)`` prefills new requests into free slots and appends them as rows
      ``n .. n+k-1`` (between graph chunks only);
    * ``step(steps)`` runs ``steps`` decode steps over the ``n`` live rows (hipGraphs per row count, cached);
    * ``poll()`` returns, per live row, the tokens generated since the previous poll and whether it finished;
    * ``retire(rows)`` drops finished rows, moving the last live rows into the holes (device-side copies of the
      row state, generated ids and sampling parameters) and freeing their slots.

    A request that arrives while others decode waits at most one chunk (``steps_per_graph`` steps) plus its own
    prefill, instead of the whole earlier batch (static batching)."""

    def __init__(self, eng: DecodeEngine):
        self.eng = eng
        self.n = 0
        self.free_slots = list(range(eng.max_batch))[::-1]
        self.row_slot: List[int] = []
        self.emitted: List[int] = []
        self.prompt_tokens: List[List[int]] = []
        self.options: List[Dict] = []
        self.reused: List[int] = []  # per live row: leading prompt tokens its slot already held at admit
        self.want: List[int] = []  # per live row: -1 (no logprobs) or its number of top_logprobs
        self.fmt: List[bool] = []  # per live row: JSON mode
        self.stops: List[tuple] = []  # per live row: its stop strings (options.stop)
        # prefix-cache bookkeeping per live row (engine.slot_tokens): steps run since admit, the newest polled
        # token (its KV is not written yet), done at the last poll, last position already dropped from the record
        self._steps: List[int] = []
        self._pending: List[Optional[int]] = []
        self._done: List[bool] = []
        self._trimmed: List[bool] = []

    def _row_lists(self):
        return (self.row_slot, self.emitted, self.prompt_tokens, self.options, self.reused, self.want, self.fmt,
                self.stops, self._steps,
                self._pending, self._done, self._trimmed)

    def _trim_idled(self) -> None:
        """A row that finished keeps stepping with its batch and rewrites its last position with the K / V of its
        last token (module docstring): once a row known to be done has run further steps, that position no longer
        holds the token the record names, so the record loses it."""
        eng = self.eng
        for i in range(self.n):
            if self._done[i] and not self._trimmed[i] and self._steps[i] > self.emitted[i]:
                rec = eng.slot_tokens[self.row_slot[i]]
                if rec and len(rec) == len(self.prompt_tokens[i]) + self.emitted[i] - 1:
                    rec.pop()
                self._trimmed[i] = True

    @property
    def capacity(self) -> int:
        return len(self.free_slots)

    def admit(self, prompts: Sequence[Union[str, Sequence[int]]], num_predict: Sequence[int],
              options: Sequence[Optional[Dict]], logprobs: Union[bool, Sequence[bool]] = False,
              top_logprobs: Union[int, Sequence[int]] = 0,
              format: Union[None, str, Sequence[Optional[str]]] = None) -> List[int]:
        """``logprobs`` / ``top_logprobs`` per request (or one value for all) as ``DecodeEngine.generate``: rows that
        ask and rows that do not decode together (``logprobs(row)`` reads a row's).  ``format`` likewise ("json" per
        request, or the option key ``"format"``): a JSON-mode row's automaton state starts fresh here and moves with
        the row (``json_state(row)`` reads how it stands).  ``options[i]["stop"]``: the request's stop strings, as
        ``generate``'s (``stop_hit(row)`` reads whether one ended the row)."""
        eng = self.eng
        k = len(prompts)
        if k == 0:
            return []
        want = _want_logprobs(logprobs, top_logprobs, k)
        if eng.speculative and any(w >= 0 for w in want):
            raise ValueError("logprobs cannot be combined with speculative decoding")
        fmt = _want_format(format, list(options), k)
        if eng.speculative and any(fmt):
            raise ValueError("format cannot be combined with speculative decoding (the K + 1 expanded rows would "
                             "each need the state after their drafts)")
        if any(fmt):
            eng._json_vocab()
        if k > len(self.free_slots):
            raise ValueError(f"{k} requests but only {len(self.free_slots)} free rows")
        ids = [eng.encode(p) or [eng.cfg.bos_id] for p in prompts]
        nps, row_opts = [], []
        for i, (p, n, o) in enumerate(zip(ids, num_predict, options)):
            budget = eng.T_max - len(p)
            if budget < 1:
                raise ValueError(f"prompt of {len(p)} tokens exceeds the context ({eng.T_max})")
            nps.append(max(1, min(int(n), budget)))
            row_opts.append(_row_options(o, eng.cfg, self.n + i, eng.seed))
        stops = [o["stop_strs"] for o in row_opts]
        if eng.speculative and any(stops):
            raise ValueError(SPEC_STOP_REFUSAL)
        if eng.speculative and any(ext_active(o) for o in row_opts):
            raise ValueError(SPEC_EXT_REFUSAL)
        if eng.prefix_cache:
            self._trim_idled()
            plan = plan_prefix_reuse(eng.slot_tokens, self.free_slots, self.row_slot, ids, PREFIX_COPY_MIN)
            slots, start = [s for s, _, _ in plan], [n for _, n, _ in plan]
            for s in slots:
                self.free_slots.remove(s)
            copies = [(d, s, n) for s, n, d in plan if d is not None and n > 0]
        else:
            slots, start, copies = [self.free_slots.pop() for _ in range(k)], None, []
        rows = list(range(self.n, self.n + k))
        r = eng.rows
        # the records the slots have once this call's copies and prefill ran (a copy's destination: the donor's)
        records = [taken_record(eng.slot_tokens[s if d is None else d], n, p) for (s, n, d), p in zip(plan, ids)] \
            if eng.prefix_cache else []
        eng._forget_slots(slots)
        with torch.cuda.stream(eng.stream):
            if copies:  # every donor's prefix in one launch, before any prefill of this call writes a slot
                cfg = eng.cfg
                with eng._cu_budget():
                    rc = ops.kv_copy_prefix(eng.kcache, eng.vtcache, cfg.n_layers, eng.max_batch, cfg.n_kv_heads,
                                            cfg.head_dim, eng.T_max, copies, stream=eng.stream)
                if rc != 0:
                    raise RuntimeError(f"cain_kv_copy_prefix refused {copies} (rc={rc})")
            eng._prefill(ids, slots, start)
            sl = slice(self.n, self.n + k)
            r["tok"][sl].copy_(torch.tensor([p[-1] for p in ids], dtype=torch.int32))
            r["pos"][sl].copy_(torch.tensor([len(p) - 1 for p in ids], dtype=torch.int32))
            r["slot"][sl].copy_(torch.tensor(slots, dtype=torch.int32))
            r["n_gen"][sl].zero_()
            r["done"][sl].zero_()
            r["max_new"][sl].copy_(torch.tensor(nps, dtype=torch.int32))
            eng.sample_params[ops.SAMPLE_BYTES * self.n: ops.SAMPLE_BYTES * (self.n + k)].copy_(ops.sample_params_tensor(row_opts, "cpu").to(eng.device))
            eng.sample_ext[ops.SAMPLE_EXT_BYTES * self.n: ops.SAMPLE_EXT_BYTES * (self.n + k)].copy_(
                ops.sample_ext_tensor(row_opts, "cpu").to(eng.device))
            if eng._lp is not None or any(w >= 0 for w in want):
                eng._lp_bufs()["topn"][sl].copy_(torch.tensor(want, dtype=torch.int32))
            if eng.speculative:
                eng._spec_begin(rows, slots, ids)
            if eng._gr is not None or any(fmt):
                eng._gr_begin(sl, fmt)
            if eng._st is not None or any(stops):
                eng._st_begin(sl, stops)
        self.want += want
        self.fmt += fmt
        self.stops += stops
        self.n += k
        self.row_slot += slots
        self.emitted += [0] * k
        self.prompt_tokens += ids
        self.options += row_opts
        self.reused += list(start) if start is not None else [0] * k
        self._steps += [0] * k
        self._pending += [None] * k
        self._done += [False] * k
        self._trimmed += [False] * k
        if eng.prefix_cache:
            for s, rec in zip(slots, records):
                eng.slot_tokens[s] = rec
        return rows

    def embed(self, prompts: Sequence[Union[str, Sequence[int]]], pooling: str = "last", normalize: bool = True,
              truncate: bool = True) -> List[EmbedResult]:
        """``DecodeEngine.embed`` between graph chunks, on currently free cache slots only -- those with an empty
        prefix-cache record first, then the shortest records -- in passes of as many prompts as there are free
        slots.  The slots stay free (their records die); no live row's slot or decode state is touched."""
        if not self.free_slots:
            raise ValueError("no free slot to embed on")
        eng = self.eng
        order = sorted(self.free_slots, key=lambda s: len(eng.slot_tokens[s]))
        return eng.embed(prompts, pooling=pooling, normalize=normalize, truncate=truncate, slots=order)

    def step(self, steps: Optional[int] = None) -> None:
        eng = self.eng
        if self.n == 0:
            return
        steps = steps or eng.steps_per_graph
        for i in range(self.n):
            self._steps[i] += steps
        with torch.cuda.stream(eng.stream):
            # the graphs with the logprobs, JSON mode's mask and advance, the stop match: where some live row wants
            # them; speculative engines: each step drafts (n-gram lookup), verifies K + 1 rows per live row and commits
            eng._run_graphs(self.n, steps, any(w >= 0 for w in self.want), any(self.fmt), any(self.stops),
                            0 if eng.speculative else None)

    def spec_stats(self, row: int) -> Optional[Dict]:
        """Speculative counters of a live row (``GenResult``'s fields of that name); None when the mode is off."""
        if not self.eng.speculative:
            return None
        with torch.cuda.stream(self.eng.stream):
            return self.eng._spec_stats(row)

    def json_state(self, row: int) -> Optional[str]:
        """How a live JSON-mode row's document stands ("done", "open", "fail": ``GenResult.json_state``); None for a
        row that is not in the mode."""
        if not self.fmt[row]:
            return None
        with torch.cuda.stream(self.eng.stream):
            return self.eng._gr_states(row + 1, [False] * row + [True])[row]

    def stop_hit(self, row: int) -> Optional[tuple]:
        """``(hit_start, index)`` of the stop string that ended a live row (the byte offset in its stream where the
        text is cut, the index in its list); None for a row without stop strings or one that hit none."""
        if not self.stops[row]:
            return None
        with torch.cuda.stream(self.eng.stream):
            return self.eng._st_hits(row + 1, [()] * row + [self.stops[row]])[row]

    def logprobs(self, row: int, lo: int = 0, hi: Optional[int] = None):
        """``(logprobs, top_logprobs)`` of tokens ``lo .. hi - 1`` (default: all polled so far) of a live row that
        asked for them; None for a row that did not."""
        if self.want[row] < 0:
            return None
        with torch.cuda.stream(self.eng.stream):
            return self.eng._read_logprobs(row, lo, self.emitted[row] if hi is None else hi, self.want[row])

    def poll(self):
        """([new token ids per live row], [finished flag per live row])."""
        eng = self.eng
        if self.n == 0:
            return [], []
        with torch.cuda.stream(eng.stream):
            ng = eng.rows["n_gen"][: self.n].cpu().tolist()
            done = eng.rows["done"][: self.n].cpu().tolist()
            hi = max(ng)
            gen = eng.gen[: self.n, :hi].cpu() if hi else None
        new, seen = [], list(self.emitted)
        for i in range(self.n):
            new.append(gen[i, self.emitted[i]: ng[i]].tolist() if ng[i] > self.emitted[i] else [])
            self.emitted[i] = ng[i]
        if eng.prefix_cache:
            # a row that produced g holds prompt + g[:-1]: each step wrote the KV of the token it consumed
            for i, fresh in enumerate(new):
                if fresh:
                    rec = eng.slot_tokens[self.row_slot[i]]
                    # (a record cleared behind this batch's back -- a static generate on the engine -- stays cleared)
                    if len(rec) == len(self.prompt_tokens[i]) - 1 + seen[i]:
                        rec.append(self.prompt_tokens[i][-1] if self._pending[i] is None else self._pending[i])
                        rec.extend(fresh[:-1])
                    self._pending[i] = fresh[-1]
                self._done[i] = bool(done[i])
            self._trim_idled()
        return new, [bool(d) for d in done]

    def tokens(self, row: int) -> List[int]:
        ng = int(self.eng.rows["n_gen"][row])
        return self.eng.gen[row, :ng].cpu().tolist()

    def retire(self, rows: Sequence[int]) -> Dict[int, int]:
        """Drop ``rows``; returns {old row index: new row index} for the rows that moved into the holes."""
        eng = self.eng
        dead = sorted(set(int(x) for x in rows))
        if not dead:
            return {}
        keep = [i for i in range(self.n) if i not in set(dead)]
        n_new = len(keep)
        moves = {}
        holes = [h for h in dead if h < n_new]
        movers = [j for j in keep if j >= n_new]
        for h, j in zip(holes, movers):
            moves[j] = h
        if eng.prefix_cache:
            self._trim_idled()
        for h in dead:
            self.free_slots.append(self.row_slot[h])
        if moves:
            r = eng.rows
            with torch.cuda.stream(eng.stream):
                # index tensors made on the engine's stream: the copies below run there, so the caching allocator
                # cannot hand these blocks out again before the gathers have read them
                src = torch.tensor(list(moves.keys()), device=eng.device, dtype=torch.long)
                dst = torch.tensor(list(moves.values()), device=eng.device, dtype=torch.long)
                for key in ("tok", "pos", "slot", "n_gen", "max_new", "done"):
                    r[key][dst] = r[key][src]
                h64 = r["hist"].view(-1, 64)
                h64[dst] = h64[src]
                eng.gen[dst] = eng.gen[src]
                sp = eng.sample_params.view(-1, ops.SAMPLE_BYTES)
                sp[dst] = sp[src]
                sx = eng.sample_ext.view(-1, ops.SAMPLE_EXT_BYTES)
                sx[dst] = sx[src]
                if eng._lp is not None:
                    for key in ("topn", "lp", "top_id", "top_lp"):
                        eng._lp[key][dst] = eng._lp[key][src]
                if eng._gr is not None:
                    for key in ("gram_on", "gstate"):
                        eng._gr[key][dst] = eng._gr[key][src]
                if eng._st is not None:
                    for key in ("stop_on", "sstate", "stop_len", "stop_bytes"):
                        eng._st[key][dst] = eng._st[key][src]
                if eng._spec is not None:  # (the records are per slot and stay)
                    for key in ("given", "drafted", "accepted", "n_step", "step_tokens"):
                        eng._spec[key][dst] = eng._spec[key][src]
            for j, h in moves.items():
                for lst in self._row_lists():
                    lst[h] = lst[j]
        with torch.cuda.stream(eng.stream):
            eng.rows["slot"][n_new: self.n].fill_(-1)  # vacated rows: skipped by the sampler
            if eng._gr is not None:
                eng._gr["gram_on"][n_new: self.n].zero_()
            if eng._st is not None:
                eng._st["stop_on"][n_new: self.n].zero_()
        self.n = n_new
        for lst in self._row_lists():
            del lst[n_new:]
        return moves
