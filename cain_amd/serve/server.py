"""Ollama-compatible HTTP server over the decode engine.

The reference's both arms talk to an Ollama server on port 11434
(experiment/RunnerConfig.py:122-131; ``POST /api/generate`` with
``{"model", "prompt", "stream": false}``).  This module is that server, backed
by ``cain_amd.engine.DecodeEngine`` (HIP kernels on the GPU this process owns),
so the on-device arm (localhost) and the remote arm (another GPU / host) speak
the same protocol as the reference.  SURVEY §2.3 row 1, §5.8.

Endpoints: ``POST /api/generate`` (stream NDJSON or one JSON), ``POST /api/chat``,
``GET /api/tags``, ``POST /api/show``, ``GET /api/ps``, ``GET /api/version``,
``POST /api/pull`` (no-op: weights are random-init, nothing is downloaded),
``GET /`` ("Ollama is running").  Response statistics use Ollama's field names
and units (ns): ``total_duration``, ``load_duration``, ``prompt_eval_count``,
``prompt_eval_duration``, ``eval_count``, ``eval_duration``.

Concurrency: one worker thread per model owns the GPU work; HTTP handler
threads only enqueue and stream results back.  On the HIP backend the worker
runs **continuous batching** (``EngineBackend.serve_queue`` over
``engine.ContinuousBatch``): a request joins the running decode batch at the
next graph boundary (every ``steps_per_graph`` decode steps) and leaves it as
soon as it finishes, so a late request waits one chunk plus its own prefill
rather than the whole earlier batch.  Other backends (torch oracle, fake) and
``--static-batching`` collect the requests that arrive within
``batch_window_ms`` into one batch and run it to completion (trial batching on
the server side).

Prefix reuse: ``/api/generate`` takes Ollama's ``context`` (token ids of an earlier answer, prepended to the new
prompt's tokens) at all times and returns one when asked to (a request that sent one, or ``--prefix-cache``).  With
``--prefix-cache`` the continuous batch keeps each cache slot's tokens and a request prefills only what differs from
the best matching slot (engine.plan_prefix_reuse): a chat's next turn, or requests behind one system prompt, skip
the shared prefix; the final JSON then carries ``prompt_cached_count``.  Off by default: responses keep their size
and every request computes its whole prompt, as the study's measurements assume.

Log-probabilities: ``"logprobs": true`` (and ``"top_logprobs": n``, 0 .. 20) on ``/api/generate`` and ``/api/chat``
adds ``"logprobs": [{"token", "logprob", "bytes", "id", "top_logprobs": [{"token", "logprob", "bytes", "id"}]}]`` to
the response, one entry per generated token (streaming: each piece carries the entries of its own tokens).  A token's
logprob is the natural-log softmax of the model's own logits: temperature 1, before the repeat penalty and top-k /
top-p; the alternatives are the n most likely tokens of that distribution.  ``id`` (the token id) is this server's
addition: random-weight vocabularies detokenise badly.  Requests that do not ask get exactly the keys they always got.

JSON mode: ``"format": "json"`` on ``/api/generate`` and ``/api/chat`` constrains the generated tokens to an RFC 8259
document whose top-level value is an object (engine/jsonmode.py; on the HIP backend a logit mask inside the decode
graphs, csrc/grammar.hip).  The row ends on the brace that closes the object (``done_reason: "stop"``); a row whose
``num_predict`` runs out first returns a prefix that can still be completed (``"length"``).  Absent or ``""``: free
text, exactly as before.  A JSON schema object or any other value is a 400; so is ``format`` on a ``--speculative``
server, and on a model whose vocabulary cannot spell JSON (the synthetic tokenizer of the random-init tags).

Stop sequences: ``options.stop`` (a string or a list of up to 8 strings of up to 32 UTF-8 bytes) on ``/api/generate``
and ``/api/chat`` ends the generation on the token that completes one of the strings (engine/stopseq.py; on the HIP
backend matched inside the decode graphs, csrc/stopseq.hip): ``done_reason: "stop"``, the response without the string
and what followed it inside that token, ``eval_count`` with that token.  While such a row streams, the server holds
back the longest end of its output that may yet begin a stop string (``StopStreamer``), so the streamed pieces
concatenate to exactly the non-streamed response.  Anything else in ``stop`` is a 400; so is ``stop`` on a
``--speculative`` server.  Special tokens cannot be matched as text (their pieces are empty): they are what the
template's turn-end ids and the engine's ``stop_ids`` are for.

Tracing: started with ``--trace-dir DIR``, the engine backend records every decode batch
with ``torch.profiler`` (host ops + GPU kernels) and writes a Chrome trace to DIR; the response JSON
names it in ``cain_trace`` so the client can file it with its run (the study moves it into run_dir).

Length policy: random weights rarely emit EOS, so when a request does not set
``options.num_predict`` the server derives it from the prompt: "In N words ..."
(the study's prompt template, experiment/RunnerConfig.py:120) maps to
⌈4/3·N⌉ tokens; anything else gets 128 tokens.
"""
from __future__ import annotations

import argparse
import datetime
import json
import os
import queue
import re
import sys
import threading
import time
from dataclasses import dataclass, field
from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer
from typing import Any, Callable, Dict, List, Optional

from ..models.tokenizer import StreamDecoder, tokens_for_words

VERSION = "0.5.0-cain-amd"
_WORDS = re.compile(r"\bin\s+(\d+)\s+words\b", re.IGNORECASE)
DEFAULT_NUM_PREDICT = 128


def default_num_predict(prompt: str) -> int:
    m = _WORDS.search(prompt or "")
    return tokens_for_words(int(m.group(1))) if m else DEFAULT_NUM_PREDICT


def _now() -> str:
    return datetime.datetime.now(datetime.timezone.utc).isoformat().replace("+00:00", "Z")


@dataclass
class Job:
    model: str
    prompt: Any                      # str or token ids
    num_predict: int
    options: Dict[str, Any]
    stream: Optional[Callable[[str], None]] = None   # receives text pieces
    done: threading.Event = field(default_factory=threading.Event)
    result: Any = None
    error: Optional[BaseException] = None
    t_submit: float = field(default_factory=time.perf_counter)
    trace_file: Optional[str] = None  # Chrome trace of the batch that decoded this job (--trace-dir)
    context: Optional[List[int]] = None  # token ids that go in front of the prompt's (Ollama's ``context``)
    want_context: bool = False       # the response carries ``context``
    logprobs: bool = False           # the response carries ``logprobs`` (one entry per generated token)
    top_logprobs: int = 0            # alternatives per entry (0 .. 20)
    lp_entries: List[Dict[str, Any]] = field(default_factory=list)  # the entries produced so far
    format: Optional[str] = None     # "json": Ollama's JSON mode (engine/jsonmode.py)


@dataclass
class EmbedJob:
    """The scheduler's second job kind: the inputs of one ``/api/embed`` / ``/api/embeddings`` request, embedded raw
    (no chat template) by the model's worker thread between decode chunks (``Backend.embed``)."""
    model: str
    inputs: List[str]
    truncate: bool = True
    done: threading.Event = field(default_factory=threading.Event)
    result: Any = None               # List[EmbedResult]
    error: Optional[BaseException] = None
    t_submit: float = field(default_factory=time.perf_counter)


EMBED_POOLINGS = ("last", "mean")


def embed_pooling_setting(value: Optional[str] = None) -> str:
    """The server's pooling mode: ``value`` (``serve --embed-pooling``), else ``CAIN_EMBED_POOLING``, else "last"."""
    mode = value or os.environ.get("CAIN_EMBED_POOLING") or "last"
    if mode not in EMBED_POOLINGS:
        raise ValueError(f"embed pooling must be one of {EMBED_POOLINGS}, got {mode!r}")
    return mode


def logprob_entries(tok, ids, lps, tops) -> List[Dict[str, Any]]:
    """The response's ``logprobs`` entries of tokens ``ids`` with logprobs ``lps`` and alternatives ``tops``."""
    def one(i: int, lp: float) -> Dict[str, Any]:
        text = tok.decode([int(i)])
        return {"token": text, "logprob": float(lp), "bytes": list(text.encode("utf-8")), "id": int(i)}

    return [dict(one(i, lp), top_logprobs=[one(a, v) for a, v in top]) for i, lp, top in zip(ids, lps, tops)]


class StopStreamer:
    """The streamed text of a row with stop strings, in ``StreamDecoder``'s place.  After every ``push`` the text sent
    so far is a prefix of whatever the row's final text can still be: the host runs the row's stop rule over the new
    tokens' pieces (engine/stopseq.py) and sends the decoded text cut before the longest end of the stream that is a
    proper prefix of a stop string -- or, once a string completed, cut where the engine cuts it.  ``finish(text)``
    sends what remains of the final text.  (Each push decodes the whole row: stop rows only.)"""

    def __init__(self, eng, stops, decoder):
        from ..engine import stopseq

        self.rule, self.pieces, self.dec = stopseq, eng._piece_vocab(), decoder
        self.stops = stopseq.stop_bytes(stops)
        self.ids: List[int] = []
        self.raw = bytearray()
        self.state = stopseq.INITIAL
        self.sent = ""

    def push(self, ids) -> str:
        for t in ids:
            piece = self.pieces[t] if 0 <= int(t) < len(self.pieces) else b""
            self.ids.append(int(t))
            self.raw += piece
            if self.state[3] < 0:
                self.state, _ = self.rule.advance(self.state, piece, self.stops)
        raw = bytes(self.raw)
        cut = self.state[3] if self.state[3] >= 0 else len(raw) - self.rule.held_back(raw, self.stops)
        text = self.rule.cut_text(self.dec.decode(self.ids), raw, cut)
        if text.endswith("\ufffd") or len(text) <= len(self.sent) or not text.startswith(self.sent):
            return ""  # (a character still split over tokens, or nothing new)
        piece, self.sent = text[len(self.sent):], text
        return piece

    def finish(self, text: str) -> str:
        piece, self.sent = text[len(self.sent):], text
        return piece


class Backend:
    """Interface: decode a batch of jobs for one model."""

    def models(self) -> List[str]:
        raise NotImplementedError

    def run(self, model: str, jobs: List[Job]) -> None:
        raise NotImplementedError

    def prompt_for(self, model: str, body: Dict[str, Any], chat: bool) -> Any:
        """The decoder input of a request: Ollama's prompt handling.  A model without a chat template (every
        random-init tag) gets the text as given (a chat's turns as "role: content" lines); ``EngineBackend`` renders
        a checkpoint's template."""
        if chat:
            return "\n".join(f"{m.get('role', 'user')}: {m.get('content', '')}" for m in body.get("messages") or [])
        prompt = body.get("prompt", "")
        return f"{body['system']}\n{prompt}" if body.get("system") else prompt

    def max_batch(self, model: str) -> int:
        return 1

    def embed(self, model: str, job: "EmbedJob", cb=None) -> None:
        """Fill ``job.result`` with one ``EmbedResult`` per input (``cb``: the model's continuous batch, when the
        worker runs one: the embedding then takes its free slots only)."""
        raise NotImplementedError

    embed_pooling = "last"  # the server's pooling mode (embed_pooling_setting)

    def model_info(self, model: str) -> Dict[str, Any]:
        return {}

    def check_format(self, model: str, fmt: str) -> None:
        """Raise ValueError when this backend cannot serve ``format: fmt`` for ``model`` (default: the field is
        accepted and ignored, as a backend without a model does)."""

    def check_stop(self, model: str, stops) -> None:
        """Raise ValueError when this backend cannot serve ``options.stop`` for ``model`` (default: the option is
        accepted; a backend without a model ignores it, as it ignores the sampling options)."""

    def check_sampling(self, model: str, ext: Dict[str, float]) -> None:
        """Raise ValueError when this backend cannot serve the non-neutral ``min_p`` / ``presence_penalty`` /
        ``frequency_penalty`` of ``ext`` for ``model`` (default: accepted, as the other sampling options are)."""

    def vocab_size(self, model: str) -> Optional[int]:
        """Token ids a request's ``context`` may hold are below this (None: not checked)."""
        return None

    prefix_cache = False
    logprobs = True  # requests may ask for token log-probabilities


# Ollama's quantization_level names for the engine's weight storage
QUANT_LEVEL = {"bf16": "BF16", "fp8": "F8_E4M3", "fp4": "MXFP4", "q4_0": "Q4_0", "q4_k": "Q4_K", "q4_k_m": "Q4_K_M"}


def register_checkpoints(specs: Optional[List[str]]) -> List[str]:
    """``--checkpoint TAG=PATH`` options: added to ``CAIN_CHECKPOINTS`` (so engines, and processes started from
    here, load the checkpoint for TAG; models/hf.py); returns the tags."""
    from ..models.hf import registered_checkpoints

    if not specs:
        return []
    os.environ["CAIN_CHECKPOINTS"] = ",".join(filter(None, [os.environ.get("CAIN_CHECKPOINTS", "")] + list(specs)))
    from ..models.hf import checkpoint_for

    registered_checkpoints()  # validates the syntax
    tags = [s.partition("=")[0].strip() for s in specs]
    for t in tags:
        try:
            path = checkpoint_for(t)  # resolves "ollama" entries to the local store's blob
        except (OSError, ValueError) as exc:
            raise SystemExit(f"--checkpoint {t}: {exc}")
        if not (os.path.isdir(path) or os.path.isfile(path)):
            raise SystemExit(f"--checkpoint {t}: {path} is neither a checkpoint directory nor a GGUF file")
    return tags


class EngineBackend(Backend):
    """Backed by one DecodeEngine per model on ``device`` (created on first use, then resident)."""

    def __init__(self, models: List[str], device: str = "cuda:0", max_batch: int = 16, max_context: int = 2048,
                 backend: Optional[str] = None, seed: int = 0, preload: bool = False, steps_per_graph: int = 8,
                 trace_dir: Optional[str] = None, weight_dtype: str = "bf16", continuous: bool = True,
                 kv_dtype: str = "bf16", prefix_cache: bool = False, speculative: int = 0,
                 draft_model: Optional[str] = None, embed_pooling: Optional[str] = None):
        self._models = list(models)
        self.embed_pooling = embed_pooling_setting(embed_pooling)
        self.prefix_cache = bool(prefix_cache)
        self.speculative = int(speculative)  # drafts per decode step (engine/speculative.py); 0: off
        if not 0 <= self.speculative <= 7:
            raise ValueError(f"speculative must be in 0..7, got {speculative}")
        if self.speculative and self.prefix_cache:
            raise ValueError("speculative decoding and prefix_cache cannot be combined")
        self.draft_model = draft_model or None  # tag of the model that drafts (engine/speculative.py "Draft model")
        if self.draft_model and not self.speculative:
            raise ValueError("draft_model needs speculative > 0")
        self.kv_dtype = kv_dtype
        # continuous batching needs the HIP engine; tracing records whole static batches
        self.continuous = continuous and not trace_dir
        self.weight_dtype = weight_dtype
        self.trace_dir = trace_dir
        self._trace_seq = 0
        self.device = device
        self._max_batch = max_batch
        self.max_context = max_context
        self.backend = backend
        self.seed = seed
        self.steps_per_graph = steps_per_graph
        self.engines: Dict[str, Any] = {}
        self._lock = threading.Lock()
        if preload:
            for m in self._models:
                self.engine(m)

    def models(self) -> List[str]:
        return list(self._models)

    def max_batch(self, model: str) -> int:
        return self._max_batch

    @property
    def speculative_label(self) -> str:
        """What ``/api/show`` and ``/api/ps`` report as "speculative" ("": the mode is off)."""
        if not self.speculative:
            return ""
        return f"draft:{self.draft_model}-k{self.speculative}" if self.draft_model else f"ngram-k{self.speculative}"

    def engine(self, model: str):
        from ..engine import DecodeEngine

        with self._lock:
            eng = self.engines.get(model)
            if eng is None:
                if model not in self._models:
                    raise KeyError(f"model '{model}' not found, try pulling it first")
                eng = DecodeEngine(model, device=self.device, max_batch=self._max_batch,
                                   max_context=self.max_context, backend=self.backend, seed=self.seed,
                                   steps_per_graph=self.steps_per_graph, weight_dtype=self.weight_dtype,
                                   kv_dtype=self.kv_dtype, prefix_cache=self.prefix_cache,
                                   speculative=self.speculative, draft_model=self.draft_model)
                self.engines[model] = eng
            return eng

    def prompt_for(self, model: str, body: Dict[str, Any], chat: bool) -> Any:
        """As Ollama: a model with a chat template (a checkpoint's) gets ``/api/generate``'s prompt as one user turn
        (after ``system``) and ``/api/chat``'s messages through the template, with the generation prompt; ``raw``
        skips it.  The rendered text is tokenized without a second BOS (the template writes its own)."""
        from ..models.hf import checkpoint_for

        # only a checkpoint brings a template: random-init tags keep the lazy engine load in the scheduler thread
        tok = (getattr(self.engine(model), "tokenizer", None)
               if model in self._models and checkpoint_for(model) else None)
        if tok is None or not getattr(tok, "chat_template", None) or body.get("raw"):
            return super().prompt_for(model, body, chat)
        if chat:
            msgs = [{"role": m.get("role", "user"), "content": m.get("content", "")} for m in body.get("messages") or []]
        else:
            msgs = ([{"role": "system", "content": body["system"]}] if body.get("system") else []) + \
                   [{"role": "user", "content": body.get("prompt", "")}]
        return tok.encode(tok.render_chat(msgs), add_bos=False)

    def vocab_size(self, model: str) -> Optional[int]:
        from ..models import get_config

        return int(get_config(model).vocab) if model in self._models else None

    def model_info(self, model: str) -> Dict[str, Any]:
        from ..models import get_config
        from ..models.hf import checkpoint_for

        cfg = get_config(model)
        ckpt = checkpoint_for(model)
        info = cfg.as_dict() | ({"checkpoint": ckpt} if ckpt else {"weights": "random-init"})
        info["embedding_length"] = int(cfg.d_model)  # the floats of an /api/embed vector
        out = {"details": {"family": cfg.family or cfg.name.split(":")[0],
                           "parameter_size": f"{cfg.n_params() / 1e9:.1f}B",
                           "quantization_level": QUANT_LEVEL[self.weight_dtype], "format": "cain-packed",
                           "embed_pooling": self.embed_pooling},
               "model_info": info}
        if self.speculative:
            out["details"]["speculative"] = self.speculative_label
        if ckpt:  # as Ollama's show: the prompt template and the stop tokens (a checkpoint's)
            from ..models.hf import load_tokenizer

            tok = load_tokenizer(ckpt, cfg)
            if tok is not None:
                out["template"] = tok.chat_template or ""
                stops = [i for i in (cfg.eos_id, *cfg.stop_ids) if i >= 0]
                out["parameters"] = "\n".join(f"stop {json.dumps(tok.tok.id_to_token(i))}" for i in stops
                                               if tok.tok.id_to_token(i) is not None)
        return out

    def check_format(self, model: str, fmt: str) -> None:
        if self.speculative:
            raise ValueError("format cannot be combined with speculative decoding (--speculative)")
        # ValueError: the model's vocabulary cannot spell JSON.  An engine that is loaded answers for its own vocabulary
        # (set_json_vocab included) and a checkpoint's engine is loaded here, as prompt_for does; a random-init tag that
        # is not loaded yet keeps its lazy load in the scheduler thread: its synthetic tokenizer is judged on its own.
        from ..models.hf import checkpoint_for

        with self._lock:
            eng = self.engines.get(model)
        if eng is None and model in self._models and not checkpoint_for(model):
            from ..engine import jsonmode
            from ..models.config import get_config
            from ..models.tokenizer import get_tokenizer

            cfg = get_config(model)
            jsonmode.check_vocabulary(jsonmode.token_bytes(get_tokenizer(cfg), cfg.vocab))
            return
        self.engine(model)._json_vocab()

    def check_stop(self, model: str, stops) -> None:
        if stops and self.speculative:
            raise ValueError("stop strings cannot be combined with speculative decoding (--speculative)")

    def check_sampling(self, model: str, ext: Dict[str, float]) -> None:
        if self.speculative:
            raise ValueError("min_p, presence_penalty and frequency_penalty cannot be combined with speculative "
                             "decoding (--speculative)")

    @staticmethod
    def _stream_decoder(eng, j: Job):
        """What turns a streamed job's new token ids into the text pieces to send."""
        stops = j.options.get("stop") if j.options else None
        dec = eng.text_decoder(bool(j.format), bool(stops))
        return StopStreamer(eng, stops, dec) if stops else StreamDecoder(dec)

    def embed(self, model: str, job: EmbedJob, cb=None) -> None:
        src = cb if cb is not None else self.engine(model)
        job.result = src.embed(job.inputs, pooling=self.embed_pooling, normalize=True, truncate=job.truncate)

    def run(self, model: str, jobs: List[Job]) -> None:
        eng = self.engine(model)
        tok = eng.tokenizer
        streams = [j.stream for j in jobs]
        decs = [self._stream_decoder(eng, j) if j.stream is not None else None for j in jobs]

        def on_tokens(new_per_row: List[List[int]], lps=None) -> None:
            for r, (j, d, ids) in enumerate(zip(jobs, decs, new_per_row)):
                if j.stream is not None and ids:
                    piece = d.push(ids)
                    if j.logprobs:  # the entries of this piece's tokens travel with it (the text may be held back)
                        ents = logprob_entries(tok, ids, *lps[r])
                        j.lp_entries += ents
                        j.stream((piece, ents))
                    elif piece:
                        j.stream(piece)

        def gen():
            kw = dict(logprobs=[j.logprobs for j in jobs], top_logprobs=[j.top_logprobs for j in jobs]) \
                if any(j.logprobs for j in jobs) else {}
            if any(j.format for j in jobs):
                kw["format"] = [j.format for j in jobs]
            return eng.generate([j.prompt for j in jobs], [j.num_predict for j in jobs], [j.options for j in jobs],
                                on_tokens=on_tokens if any(streams) else None,
                                context=[j.context for j in jobs] if any(j.context for j in jobs) else None, **kw)

        if self.trace_dir:
            res, path = self._traced(model, gen)
            for j in jobs:
                j.trace_file = path
        else:
            res = gen()
        ttft = getattr(eng, "last_ttft_ns", 0)
        for j, d, r in zip(jobs, decs, res):
            if j.stream is not None:
                # text held back at a length cutoff inside a character; a stop row: what remains of its final text
                tail = d.finish(r.text) if isinstance(d, StopStreamer) else d.flush()
                if tail:
                    j.stream(tail)
            if j.logprobs and j.stream is None:
                j.lp_entries = logprob_entries(tok, r.tokens, r.logprobs, r.top_logprobs)
            j.result = r
            j.ttft_ns = ttft


    def serve_queue(self, model: str, q: "queue.Queue[Job]") -> bool:
        """Continuous batching loop of one model (never returns on the HIP engine; False: not supported here,
        the scheduler falls back to static batches)."""
        eng = self.engine(model)
        if eng.backend != "hip":
            return False
        cb = eng.continuous()
        tok = eng.tokenizer
        # row -> {job, t0 (admission start), t_pre (prefill done), t_first (first token on the host)}
        live: Dict[int, Dict[str, Any]] = {}
        while True:
            pending: List[Job] = []
            if cb.n == 0:
                pending.append(q.get())  # idle: block for the next request
            while len(pending) < cb.capacity:
                try:
                    pending.append(q.get_nowait())
                except queue.Empty:
                    break
            # the second job kind: embeddings run here, between graph chunks, on free slots (the queue is only read
            # while a slot is free: with none they wait, as a generate job does); a failure is that request's own
            for j in [j for j in pending if isinstance(j, EmbedJob)]:
                try:
                    self.embed(model, j, cb)
                except Exception as exc:  # noqa: BLE001
                    j.error = exc
                j.done.set()
            pending = [j for j in pending if not isinstance(j, EmbedJob)]
            try:
                self._cb_iteration(model, eng, cb, tok, live, pending)
            except Exception as exc:  # noqa: BLE001 - fail every request in flight, start a fresh batch
                for st in live.values():
                    st["job"].error = exc
                    st["job"].done.set()
                for j in pending:
                    if not j.done.is_set():
                        j.error = exc
                        j.done.set()
                live.clear()
                cb = eng.continuous()

    @staticmethod
    def _cb_iteration(model: str, eng, cb, tok, live: Dict[int, Dict[str, Any]], pending: List[Job]) -> None:
        """One continuous-batching iteration: admit ``pending`` (each request validated on its own: a prompt over
        the context fails that request only), then one graph chunk over every live row, then hand out tokens and
        finish the rows that are done.  Timing matches the static path (engine._generate_hip): the newly admitted
        rows' first token is decoded by a one-step graph and synchronised, so ``t_first`` is exact;
        ``eval_duration`` runs from the end of admission (first token included), ``ttft`` from its start."""
        from ..engine.engine import GenResult, _stopped

        ok: List[Job] = []
        ids: List[List[int]] = []
        for j in pending:
            try:
                p = list(j.context or []) + eng.encode(j.prompt) or [eng.cfg.bos_id]
                if len(p) >= eng.T_max:
                    raise ValueError(f"prompt of {len(p)} tokens exceeds the context ({eng.T_max})")
            except Exception as exc:  # noqa: BLE001 - reported to this request only
                j.error = exc
                j.done.set()
                continue
            ok.append(j)
            ids.append(p)
        if ok:
            t0 = time.perf_counter_ns()
            rows = cb.admit(ids, [j.num_predict for j in ok], [j.options for j in ok],
                            [j.logprobs for j in ok], [j.top_logprobs for j in ok],
                            **({"format": [j.format for j in ok]} if any(j.format for j in ok) else {}))
            eng.stream.synchronize()
            t_pre = time.perf_counter_ns()
            cb.step(1)  # the new rows' first token on its own (the live rows advance one step with them)
            eng.stream.synchronize()
            t_first = time.perf_counter_ns()
            for r, j in zip(rows, ok):
                live[r] = {"job": j, "t0": t0, "t_pre": t_pre, "t_first": t_first,
                           "dec": EngineBackend._stream_decoder(eng, j) if j.stream is not None else None}
        cb.step()
        new, fin = cb.poll()
        now = time.perf_counter_ns()
        for r, new_ids in enumerate(new):
            j = live[r]["job"]
            if new_ids and j.logprobs:
                j.lp_entries += logprob_entries(tok, new_ids, *cb.logprobs(r, cb.emitted[r] - len(new_ids)))
            if new_ids and j.stream is not None:
                piece = live[r]["dec"].push(new_ids)
                if j.logprobs:
                    j.stream((piece, j.lp_entries[-len(new_ids):]))
                elif piece:
                    j.stream(piece)
        done_rows = [r for r, f in enumerate(fin) if f]
        for r in done_rows:
            st, j = live[r], live[r]["job"]
            toks = cb.tokens(r)
            js = cb.json_state(r)  # JSON mode: the row ended on the brace that closes its object
            hit = cb.stop_hit(r)  # stop sequences: the row ended on the token that completed one of its strings
            text = eng.text_decoder(js is not None, bool(cb.stops[r])).decode(toks)
            if hit is not None:
                text = eng.stop_cut(toks, text, hit[0])
            if j.stream is not None:
                tail = st["dec"].finish(text) if isinstance(st["dec"], StopStreamer) else st["dec"].flush()
                if tail:
                    j.stream(tail)
            reason = "stop" if _stopped(toks, cb.options[r]) or js == "done" or hit is not None else "length"
            j.result = GenResult(model, list(cb.prompt_tokens[r]), toks, text, reason, json_state=js,
                                 stop_hit=cb.stops[r][hit[1]] if hit is not None else None,
                                 load_duration_ns=0, prompt_eval_duration_ns=int(st["t_pre"] - st["t0"]),
                                 eval_duration_ns=int(now - st["t_pre"]),
                                 total_duration_ns=int(now - j.t_submit * 1e9), prompt_cached=int(cb.reused[r]),
                                 **(cb.spec_stats(r) or {}))
            j.ttft_ns = int(st["t_first"] - st["t0"])
            j.done.set()
        if done_rows:
            moves = cb.retire(done_rows)
            kept = {moves.get(r, r): st for r, st in live.items() if r not in set(done_rows)}
            live.clear()
            live.update(kept)

    def _traced(self, model: str, fn):
        """Run ``fn`` under torch.profiler (CPU + GPU activity) and export a Chrome trace."""
        import os
        from pathlib import Path

        import torch
        from torch.profiler import ProfilerActivity, profile

        acts = [ProfilerActivity.CPU]
        if torch.cuda.is_available():
            acts.append(ProfilerActivity.CUDA)
        with profile(activities=acts) as prof:
            res = fn()
        self._trace_seq += 1
        out = Path(self.trace_dir)
        out.mkdir(parents=True, exist_ok=True)
        path = out / f"trace_{os.getpid()}_{self._trace_seq:05d}_{model.replace(':', '_').replace('/', '_')}.json"
        prof.export_chrome_trace(str(path))
        return res, str(path)


class FakeBackend(Backend):
    """Canned generations with controllable latency (tests / plumbing runs without a GPU).
    ``fail`` makes every request raise; ``hang_s`` sleeps before answering (timeout tests)."""

    logprobs = False  # no model behind this backend: nothing to take a probability from

    def __init__(self, models=("qwen2:1.5b",), tokens_per_s: float = 2000.0, prefill_s: float = 0.0,
                 fail: bool = False, hang_s: float = 0.0):
        self._models = list(models)
        self.tokens_per_s = tokens_per_s
        self.prefill_s = prefill_s
        self.fail = fail
        self.hang_s = hang_s
        self.calls: List[Dict[str, Any]] = []

    def models(self) -> List[str]:
        return list(self._models)

    def max_batch(self, model: str) -> int:
        return 8

    EMBED_DIM = 64

    def model_info(self, model: str) -> Dict[str, Any]:
        return {"details": {"embed_pooling": self.embed_pooling}, "model_info": {"embedding_length": self.EMBED_DIM}}

    def embed(self, model: str, job: EmbedJob, cb=None) -> None:
        """A deterministic unit vector per input, seeded by the text alone; inputs beyond 2048 synthetic tokens count
        as over the context."""
        import hashlib

        import numpy as np

        from ..engine.engine import EmbedResult
        from ..models.tokenizer import SyntheticTokenizer

        if self.fail:
            raise RuntimeError("fake backend failure")
        tok, ctx, out = SyntheticTokenizer(32000), 2048, []
        for text in job.inputs:
            n = max(1, len(tok.encode(text)))
            if n > ctx and not job.truncate:
                raise ValueError(f"input of {n} tokens exceeds the context ({ctx}) and truncate is off")
            seed = int.from_bytes(hashlib.sha256(text.encode("utf-8")).digest()[:8], "little")
            v = np.random.default_rng(seed).standard_normal(self.EMBED_DIM)
            out.append(EmbedResult((v / np.linalg.norm(v)).tolist(), min(n, ctx), n > ctx))
        job.result = out

    def run(self, model: str, jobs: List[Job]) -> None:
        from ..engine.engine import GenResult
        from ..models.tokenizer import SyntheticTokenizer

        if self.hang_s:
            time.sleep(self.hang_s)
        if self.fail:
            raise RuntimeError("fake backend failure")
        tok = SyntheticTokenizer(32000)
        t0 = time.perf_counter_ns()
        time.sleep(self.prefill_s)
        n = max(j.num_predict for j in jobs)
        time.sleep(n / self.tokens_per_s)
        dt = time.perf_counter_ns() - t0
        for i, j in enumerate(jobs):
            ids = [16 + (i * 131 + k * 7919) % 31000 for k in range(j.num_predict)]
            text = tok.decode(ids)
            if j.stream:
                j.stream(text)
            prompt_ids = tok.encode(j.prompt) if isinstance(j.prompt, str) else list(j.prompt)
            j.result = GenResult(model, prompt_ids, ids, text, "length", 0, int(self.prefill_s * 1e9), dt, dt)
            j.ttft_ns = int(self.prefill_s * 1e9)
            self.calls.append({"model": model, "prompt": j.prompt, "num_predict": j.num_predict})


class Scheduler:
    """Per-model job queues; a worker thread per model batches jobs that arrive together."""

    def __init__(self, backend: Backend, batch_window_ms: float = 5.0):
        self.backend = backend
        self.window = batch_window_ms / 1000.0
        self.queues: Dict[str, "queue.Queue[Job]"] = {}
        self.threads: Dict[str, threading.Thread] = {}
        self.lock = threading.Lock()
        self.loaded_at: Dict[str, float] = {}

    def submit(self, job: Job) -> Job:
        if job.model not in self.backend.models():
            raise KeyError(f"model '{job.model}' not found, try pulling it first")
        with self.lock:
            q = self.queues.get(job.model)
            if q is None:
                q = self.queues[job.model] = queue.Queue()
                t = threading.Thread(target=self._worker, args=(job.model, q), daemon=True,
                                     name=f"cain-sched-{job.model}")
                self.threads[job.model] = t
                self.loaded_at[job.model] = time.time()
                t.start()
        q.put(job)
        return job

    def _worker(self, model: str, q: "queue.Queue[Job]") -> None:
        if getattr(self.backend, "continuous", False):
            try:
                if self.backend.serve_queue(model, q) is not False:
                    return
            except BaseException as exc:  # noqa: BLE001 - e.g. the model failed to load
                while True:  # fail every request of this model rather than hang it
                    j = q.get()
                    j.error = exc
                    j.done.set()
        while True:
            first = q.get()
            batch = [first]
            deadline = time.perf_counter() + self.window
            cap = self.backend.max_batch(model)
            while len(batch) < cap and not isinstance(first, EmbedJob):
                rem = deadline - time.perf_counter()
                if rem <= 0:
                    break
                try:
                    batch.append(q.get(timeout=rem))
                except queue.Empty:
                    break
            # static batches: an embed job runs on its own, between two batches (one that arrived inside a batch's
            # window right after that batch)
            embeds = [j for j in batch if isinstance(j, EmbedJob)]
            batch = [j for j in batch if not isinstance(j, EmbedJob)]
            try:
                if batch:
                    self.backend.run(model, batch)
            except BaseException as exc:  # noqa: BLE001 - reported per job
                for j in batch:
                    j.error = exc
            for j in batch:
                j.done.set()
            for j in embeds:
                try:
                    self.backend.embed(model, j)
                except BaseException as exc:  # noqa: BLE001 - reported to this request
                    j.error = exc
                j.done.set()


def _result_json(job: Job, created: Optional[str] = None) -> Dict[str, Any]:
    r = job.result
    d = r.ollama_json(created or _now(), context=job.want_context)
    d["cain_ttft_ns"] = int(getattr(job, "ttft_ns", 0))
    if job.trace_file:
        d["cain_trace"] = job.trace_file
    if job.logprobs:
        d["logprobs"] = list(job.lp_entries)
    return d


class OllamaHandler(BaseHTTPRequestHandler):
    server_version = "cain-amd-ollama/" + VERSION
    protocol_version = "HTTP/1.1"
    scheduler: Scheduler = None  # set by make_server

    def log_message(self, fmt, *args):  # keep stdout for the experiment logs
        if getattr(self.server, "verbose", False):
            sys.stderr.write("[serve] " + (fmt % args) + "\n")

    # -- helpers -------------------------------------------------------------
    def _send_json(self, code: int, obj: Any) -> None:
        body = json.dumps(obj).encode()
        self.send_response(code)
        self.send_header("Content-Type", "application/json; charset=utf-8")
        self.send_header("Content-Length", str(len(body)))
        self.end_headers()
        self.wfile.write(body)

    def _body(self) -> Dict[str, Any]:
        n = int(self.headers.get("Content-Length") or 0)
        raw = self.rfile.read(n) if n else b""
        if not raw:
            return {}
        return json.loads(raw.decode("utf-8"))

    # -- routes ----------------------------------------------------------------
    def do_GET(self):  # noqa: N802
        if self.path in ("/", ""):
            body = b"Ollama is running"
            self.send_response(200)
            self.send_header("Content-Type", "text/plain")
            self.send_header("Content-Length", str(len(body)))
            self.end_headers()
            self.wfile.write(body)
        elif self.path == "/api/version":
            self._send_json(200, {"version": VERSION})
        elif self.path == "/api/tags":
            be = self.scheduler.backend
            self._send_json(200, {"models": [{"name": m, "model": m, "modified_at": _now(), "size": 0,
                                              "details": be.model_info(m).get("details", {})} for m in be.models()]})
        elif self.path == "/api/ps":
            be = self.scheduler.backend
            self._send_json(200, {"models": [{"name": m, "model": m, "expires_at": "2999-01-01T00:00:00Z",
                                              "prefix_cache": bool(getattr(be, "prefix_cache", False)),
                                              **({"speculative": getattr(be, "speculative_label", "")
                                                  or f"ngram-k{be.speculative}"}
                                                 if getattr(be, "speculative", 0) else {})}
                                             for m in self.scheduler.queues]})
        else:
            self._send_json(404, {"error": "not found"})

    def do_POST(self):  # noqa: N802
        try:
            body = self._body()
        except (ValueError, UnicodeDecodeError) as exc:
            return self._send_json(400, {"error": f"invalid JSON: {exc}"})
        if self.path == "/api/generate":
            return self._generate(body, chat=False)
        if self.path == "/api/chat":
            return self._generate(body, chat=True)
        if self.path == "/api/embed":
            return self._embed(body, legacy=False)
        if self.path == "/api/embeddings":
            return self._embed(body, legacy=True)
        if self.path == "/api/show":
            m = body.get("model") or body.get("name")
            if m not in self.scheduler.backend.models():
                return self._send_json(404, {"error": f"model '{m}' not found"})
            return self._send_json(200, self.scheduler.backend.model_info(m))
        if self.path == "/api/pull":
            m = body.get("model") or body.get("name")
            ok = m in self.scheduler.backend.models()
            return self._send_json(200 if ok else 404, {"status": "success"} if ok else {"error": "unknown model"})
        return self._send_json(404, {"error": "not found"})

    def _embed(self, body: Dict[str, Any], legacy: bool) -> None:
        """``POST /api/embed`` ({"model", "input": str | [str], "truncate"}; ``options`` and ``keep_alive`` accepted and
        ignored) and the older ``POST /api/embeddings`` ({"model", "prompt"}): the inputs embedded raw, L2-normalised
        on both routes, pooled as the server is set (``--embed-pooling``).  A missing or unknown model answers as
        ``/api/generate`` does (400 / 404)."""
        t0 = time.perf_counter_ns()
        model = body.get("model")
        if not model:
            return self._send_json(400, {"error": "model is required"})
        if legacy:
            inputs: Any = body.get("prompt", "")
            if not isinstance(inputs, str):
                return self._send_json(400, {"error": "prompt must be a string"})
            inputs = [inputs]
        else:
            inputs = body.get("input", [])
            inputs = [inputs] if isinstance(inputs, str) else inputs
            if not isinstance(inputs, list) or any(not isinstance(x, str) for x in inputs):
                return self._send_json(400, {"error": "input must be a string or a list of strings"})
        truncate = body.get("truncate", True)
        if not isinstance(truncate, bool):
            return self._send_json(400, {"error": "truncate must be true or false"})
        if model not in self.scheduler.backend.models():
            return self._send_json(404, {"error": f"model '{model}' not found, try pulling it first"})
        engines = getattr(self.scheduler.backend, "engines", {})
        loaded = model in engines  # (else this request pays the model's load, and reports it)
        job = EmbedJob(model, list(inputs), truncate)
        if inputs:
            self.scheduler.submit(job)
            job.done.wait()
        else:
            job.result = []
        if isinstance(job.error, ValueError):  # an over-long input with truncate: false
            return self._send_json(400, {"error": str(job.error)})
        if job.error is not None:
            return self._send_json(500, {"error": str(job.error)})
        if legacy:
            return self._send_json(200, {"embedding": job.result[0].embedding})
        load_ns = 0 if loaded else int(getattr(engines.get(model), "load_duration_ns", 0))
        return self._send_json(200, {"model": model, "embeddings": [r.embedding for r in job.result],
                                     "total_duration": int(time.perf_counter_ns() - t0), "load_duration": load_ns,
                                     "prompt_eval_count": sum(r.prompt_eval_count for r in job.result)})

    def _generate(self, body: Dict[str, Any], chat: bool) -> None:
        model = body.get("model")
        if not model:
            return self._send_json(400, {"error": "model is required"})
        if chat:
            msgs = body.get("messages") or []
            text = msgs[-1].get("content", "") if msgs else ""
        else:
            text = body.get("prompt", "")
        try:
            prompt = self.scheduler.backend.prompt_for(model, body, chat)
        except KeyError as exc:
            return self._send_json(404, {"error": str(exc).strip("'\"")})
        except Exception as exc:  # noqa: BLE001 - a template that fails to render, a model that fails to load
            return self._send_json(400, {"error": f"{type(exc).__name__}: {exc}"})
        context = None
        if not chat and body.get("context") is not None:
            context = body["context"]
            vocab = self.scheduler.backend.vocab_size(model)
            if not isinstance(context, list) or any(isinstance(t, bool) or not isinstance(t, int) for t in context):
                return self._send_json(400, {"error": "context must be a list of token ids"})
            if any(t < 0 or (vocab is not None and t >= vocab) for t in context):
                return self._send_json(400, {"error": f"context holds a token id outside the vocabulary ({vocab})"})
        want_lp, n_top = body.get("logprobs", False), body.get("top_logprobs", 0)
        if not isinstance(want_lp, bool):
            return self._send_json(400, {"error": "logprobs must be true or false"})
        if isinstance(n_top, bool) or not isinstance(n_top, int) or not 0 <= n_top <= 20:
            return self._send_json(400, {"error": "top_logprobs must be an integer in 0..20"})
        if n_top and not want_lp:
            return self._send_json(400, {"error": "top_logprobs needs logprobs: true"})
        if want_lp and not getattr(self.scheduler.backend, "logprobs", False):
            return self._send_json(400, {"error": "logprobs: no model behind this backend"})
        if want_lp and getattr(self.scheduler.backend, "speculative", 0):
            return self._send_json(400, {"error": "logprobs cannot be combined with speculative decoding "
                                                  "(--speculative)"})
        # Ollama's format: absent or "" -- free text; "json" -- JSON mode; a JSON schema (an object) is not supported
        # (the engine's per-row option key "format" counts as the field: it gets the same checks and travels as the
        # job's format, not inside the sampling options)
        opts = dict(body.get("options") or {})
        opt_fmt = opts.pop("format", None)
        fmt = body.get("format")
        if fmt in (None, ""):
            fmt = opt_fmt
        if isinstance(fmt, dict):
            return self._send_json(400, {"error": 'format: JSON schema is not supported, only "json"'})
        if fmt not in (None, "", "json"):
            return self._send_json(400, {"error": 'format must be "json" or absent'})
        fmt = fmt or None
        if fmt:
            try:
                self.scheduler.backend.check_format(model, fmt)
            except KeyError as exc:
                return self._send_json(404, {"error": str(exc).strip("'\"")})
            except ValueError as exc:
                return self._send_json(400, {"error": str(exc)})
        # Ollama's options.stop: a string or a list of strings (engine/stopseq.py has the limits)
        if opts.get("stop") is not None:
            from ..engine.stopseq import parse_stop

            try:
                opts["stop"] = list(parse_stop(opts["stop"]))
                self.scheduler.backend.check_stop(model, opts["stop"])
            except ValueError as exc:
                return self._send_json(400, {"error": str(exc)})
        # min_p, presence_penalty, frequency_penalty: their ranges (README "Sampling options"), and what the backend
        # cannot combine them with
        if any(opts.get(k) is not None for k in ("min_p", "presence_penalty", "frequency_penalty")):
            from ..engine.engine import ext_active, ext_options

            try:
                ext = ext_options(opts)
                if ext_active(ext):
                    self.scheduler.backend.check_sampling(model, ext)
            except ValueError as exc:
                return self._send_json(400, {"error": str(exc)})
        n = opts.get("num_predict")
        # the length policy reads the user's words ("In N words ..."), not the template around them
        num_predict = int(n) if n is not None and int(n) > 0 else default_num_predict(text)
        stream = body.get("stream", True)
        created = _now()
        chunks: "queue.Queue[str]" = queue.Queue()
        job = Job(model, prompt, num_predict, opts, stream=chunks.put if stream else None, context=context,
                  want_context=not chat and (context is not None or bool(getattr(self.scheduler.backend,
                                                                                "prefix_cache", False))),
                  logprobs=want_lp, top_logprobs=n_top, format=fmt)
        try:
            self.scheduler.submit(job)
        except KeyError as exc:
            return self._send_json(404, {"error": str(exc).strip("'\"")})
        if not stream:
            job.done.wait()
            if job.error is not None:
                return self._send_json(500, {"error": str(job.error)})
            d = _result_json(job, created)
            if chat:
                d["message"] = {"role": "assistant", "content": d.pop("response")}
            return self._send_json(200, d)
        # NDJSON streaming (chunked transfer encoding)
        self.send_response(200)
        self.send_header("Content-Type", "application/x-ndjson")
        self.send_header("Transfer-Encoding", "chunked")
        self.end_headers()

        def emit(obj) -> None:
            data = (json.dumps(obj) + "\n").encode()
            self.wfile.write(f"{len(data):x}\r\n".encode() + data + b"\r\n")
            self.wfile.flush()

        while not (job.done.is_set() and chunks.empty()):
            try:
                piece = chunks.get(timeout=0.05)
            except queue.Empty:
                continue
            ents = None
            if isinstance(piece, tuple):
                piece, ents = piece
            part = {"model": model, "created_at": _now(), "done": False}
            if ents is not None:
                part["logprobs"] = ents
            if chat:
                part["message"] = {"role": "assistant", "content": piece}
            else:
                part["response"] = piece
            emit(part)
        if job.error is not None:
            emit({"error": str(job.error)})
        else:
            d = _result_json(job, created)
            d["response"] = ""
            if job.logprobs:
                d["logprobs"] = []  # every entry went out with its piece
            if chat:
                d.pop("response")
                d["message"] = {"role": "assistant", "content": ""}
            emit(d)
        self.wfile.write(b"0\r\n\r\n")
        self.wfile.flush()


def make_server(backend: Backend, host: str = "127.0.0.1", port: int = 11434, batch_window_ms: float = 5.0,
                verbose: bool = False) -> ThreadingHTTPServer:
    sched = Scheduler(backend, batch_window_ms)
    handler = type("BoundOllamaHandler", (OllamaHandler,), {"scheduler": sched})
    srv = ThreadingHTTPServer((host, port), handler)
    srv.daemon_threads = True
    srv.verbose = verbose
    srv.scheduler = sched
    return srv


class ServerThread:
    """Run a server in a background thread (tests, in-process remote arm)."""

    def __init__(self, backend: Backend, host: str = "127.0.0.1", port: int = 0, **kw):
        self.server = make_server(backend, host, port, **kw)
        self.thread = threading.Thread(target=self.server.serve_forever, daemon=True, name="cain-ollama")

    @property
    def url(self) -> str:
        h, p = self.server.server_address[:2]
        return f"http://{h}:{p}"

    def __enter__(self):
        self.thread.start()
        return self

    def __exit__(self, *exc):
        self.server.shutdown()
        self.server.server_close()


def main(argv: Optional[List[str]] = None) -> None:
    from ..models import MODELS, TINY

    ap = argparse.ArgumentParser(prog="python -m cain_amd serve")
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=11434)
    ap.add_argument("--models", default=",".join(MODELS), help="comma-separated model tags to serve")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--max-context", type=int, default=2048)
    ap.add_argument("--batch-window-ms", type=float, default=5.0)
    ap.add_argument("--backend", choices=["hip", "torch", "fake"], default=None)
    ap.add_argument("--preload", action="store_true", help="load every model at startup (all stay resident)")
    ap.add_argument("--fake-tok-s", type=float, default=2000.0, help="fake backend: modelled decode rate")
    ap.add_argument("--fake-prefill-s", type=float, default=0.0, help="fake backend: modelled time to first token")
    ap.add_argument("--trace-dir", default=None, help="write a torch.profiler Chrome trace of every decode batch here")
    ap.add_argument("--weights", choices=list(QUANT_LEVEL), default="bf16",
                    help="GEMM weight storage (fp8: e4m3 per-row scaled; W8A8 above 16 rows, W8A16 below)")
    ap.add_argument("--kv", choices=["bf16", "fp8"], default="bf16", help="KV-cache storage (fp8: e4m3)")
    ap.add_argument("--static-batching", action="store_true",
                    help="batch requests that arrive within --batch-window-ms and run each batch to completion "
                         "(default on the HIP engine: continuous batching)")
    ap.add_argument("--prefix-cache", action="store_true",
                    help="keep each cache slot's tokens between requests and prefill only what differs from the best "
                         "matching slot (continuous batching on the HIP engine); responses carry 'context'")
    ap.add_argument("--speculative", type=int, default=0, metavar="K",
                    help="speculative decoding: K (1..7) n-gram drafts from the request's own tokens per decode step, "
                         "verified K + 1 rows per weight pass; the tokens are plain decoding's (not with "
                         "--prefix-cache or logprobs)")
    ap.add_argument("--draft-model", default=None, metavar="TAG[=PATH]",
                    help="with --speculative: a smaller model with the same tokenizer proposes the K drafts inside "
                         "the decode graphs instead of the n-gram lookup (PATH: its checkpoint, as --checkpoint)")
    ap.add_argument("--checkpoint", action="append", metavar="TAG=PATH",
                    help="serve a Hugging Face checkpoint directory or GGUF file under TAG (repeatable; models/hf.py); "
                         "PATH 'ollama' takes the blob a local Ollama store keeps for TAG")
    ap.add_argument("--embed-pooling", choices=list(EMBED_POOLINGS), default=None,
                    help="/api/embed and /api/embeddings: the position(s) an embedding is pooled over (default: "
                         "CAIN_EMBED_POOLING, else last)")
    ap.add_argument("-v", "--verbose", action="store_true")
    ns = ap.parse_args(argv)
    ck_tags = register_checkpoints(ns.checkpoint)
    models = [m for m in ns.models.split(",") if m]
    models += [t for t in ck_tags if t not in models]
    for m in models:
        if m not in MODELS and m not in TINY and m not in ck_tags:
            raise SystemExit(f"unknown model {m}")
    if not 0 <= ns.speculative <= 7:
        raise SystemExit("--speculative must be in 0..7")
    if ns.speculative and ns.prefix_cache:
        raise SystemExit("--speculative and --prefix-cache cannot be combined")
    draft = _draft_model_arg(ns.draft_model, ns.speculative)
    if ns.backend == "fake":
        be: Backend = FakeBackend(models, tokens_per_s=ns.fake_tok_s, prefill_s=ns.fake_prefill_s)
        be.embed_pooling = embed_pooling_setting(ns.embed_pooling)
    else:
        be = EngineBackend(models, device=ns.device, max_batch=ns.max_batch, max_context=ns.max_context,
                           backend=ns.backend, preload=ns.preload, trace_dir=ns.trace_dir, weight_dtype=ns.weights,
                           continuous=not ns.static_batching, kv_dtype=ns.kv, prefix_cache=ns.prefix_cache,
                           speculative=ns.speculative, draft_model=draft, embed_pooling=ns.embed_pooling)
    srv = make_server(be, ns.host, ns.port, ns.batch_window_ms, ns.verbose)
    print(f"[serve] Ollama-compatible API on http://{ns.host}:{srv.server_address[1]} models={models}", flush=True)
    try:
        srv.serve_forever()
    except KeyboardInterrupt:  # pragma: no cover
        pass


def _draft_model_arg(arg: Optional[str], speculative: int) -> Optional[str]:
    """``--draft-model TAG[=PATH]``: the tag, its checkpoint registered when a path is given."""
    if not arg:
        return None
    if not speculative:
        raise SystemExit("--draft-model needs --speculative K")
    if "=" in arg:
        register_checkpoints([arg])
    return arg.split("=", 1)[0]


def generate_main(argv: Optional[List[str]] = None) -> None:
    """``python -m cain_amd generate --model M --prompt P``: one local generation, Ollama JSON on stdout."""
    ap = argparse.ArgumentParser(prog="python -m cain_amd generate")
    ap.add_argument("--model", required=True)
    ap.add_argument("--prompt", required=True)
    ap.add_argument("--num-predict", type=int, default=None)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--temperature", type=float, default=None)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--weights", choices=list(QUANT_LEVEL), default="bf16")
    ap.add_argument("--kv", choices=["bf16", "fp8"], default="bf16")
    ap.add_argument("--checkpoint", metavar="PATH", help="a Hugging Face checkpoint directory, served as --model")
    ap.add_argument("--speculative", type=int, default=0, metavar="K", help="speculative decoding with K n-gram drafts")
    ap.add_argument("--draft-model", default=None, metavar="TAG[=PATH]",
                    help="with --speculative: the model that proposes the drafts")
    ap.add_argument("--format", choices=["json"], default=None,
                    help="json: constrain the output to a JSON object (Ollama's format: \"json\")")
    ap.add_argument("--stop", action="append", metavar="STR",
                    help="end the generation where STR appears in the output (repeatable, up to 8; Ollama's "
                         "options.stop)")
    ns = ap.parse_args(argv)
    if ns.checkpoint:
        register_checkpoints([f"{ns.model}={ns.checkpoint}"])
    be = EngineBackend([ns.model], device=ns.device, max_batch=1, weight_dtype=ns.weights, kv_dtype=ns.kv,
                       speculative=ns.speculative, draft_model=_draft_model_arg(ns.draft_model, ns.speculative))
    opts = {k: v for k, v in (("temperature", ns.temperature), ("seed", ns.seed)) if v is not None}
    if ns.stop:
        from ..engine.stopseq import parse_stop

        try:
            opts["stop"] = list(parse_stop(ns.stop))
            be.check_stop(ns.model, opts["stop"])
        except ValueError as exc:
            raise SystemExit(f"--stop: {exc}")
    job = Job(ns.model, ns.prompt, ns.num_predict or default_num_predict(ns.prompt), opts, format=ns.format)
    if ns.format:
        try:
            be.check_format(ns.model, ns.format)
        except ValueError as exc:
            raise SystemExit(f"--format {ns.format}: {exc}")
    be.run(ns.model, [job])
    print(json.dumps(_result_json(job)))


def embed_main(argv: Optional[List[str]] = None) -> None:
    """``python -m cain_amd embed --model M (--input TEXT ... | --file F)``: the texts' embeddings (--file: one per
    non-empty line) from a local engine, one JSON line on stdout."""
    ap = argparse.ArgumentParser(prog="python -m cain_amd embed")
    ap.add_argument("--model", required=True)
    ap.add_argument("--weights", choices=list(QUANT_LEVEL), default="bf16")
    ap.add_argument("--kv", choices=["bf16", "fp8"], default="bf16")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--backend", choices=["hip", "torch"], default=None)
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--max-context", type=int, default=2048)
    ap.add_argument("--checkpoint", metavar="PATH", help="a Hugging Face checkpoint directory, served as --model")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--input", nargs="+", metavar="TEXT")
    src.add_argument("--file", metavar="F", help="one input per non-empty line")
    ap.add_argument("--pooling", choices=list(EMBED_POOLINGS), default="last")
    ap.add_argument("--no-normalize", action="store_true", help="the pooled vector as it is, not L2-normalised")
    ap.add_argument("--no-truncate", action="store_true", help="refuse an input beyond the context instead of cutting it")
    ns = ap.parse_args(argv)
    if ns.checkpoint:
        register_checkpoints([f"{ns.model}={ns.checkpoint}"])
    if ns.file:
        with open(ns.file, encoding="utf-8") as fh:
            inputs = [ln.rstrip("\n") for ln in fh if ln.strip()]
    else:
        inputs = list(ns.input)
    be = EngineBackend([ns.model], device=ns.device, max_batch=ns.max_batch, max_context=ns.max_context,
                       backend=ns.backend, weight_dtype=ns.weights, kv_dtype=ns.kv)
    eng = be.engine(ns.model)
    try:
        t0 = time.perf_counter()
        res = eng.embed(inputs, pooling=ns.pooling, normalize=not ns.no_normalize, truncate=not ns.no_truncate)
        dt = time.perf_counter() - t0
    except ValueError as exc:
        raise SystemExit(f"embed: {exc}")
    n = sum(r.prompt_eval_count for r in res)
    print(json.dumps({"model": ns.model, "weights": ns.weights, "pooling": ns.pooling, "dim": int(eng.cfg.d_model),
                      "inputs": len(inputs), "prompt_eval_count": n, "tok_per_s": n / dt if dt > 0 else 0.0,
                      "embeddings": [r.embedding for r in res]}))
