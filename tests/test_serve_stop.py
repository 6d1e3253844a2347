"""Ollama's ``options.stop`` on ``/api/generate`` and ``/api/chat``, on the torch backend (no GPU): the response is cut
at the stop string, streamed and non-streamed responses agree, nothing that is later cut is ever streamed, the 400s,
and requests without ``stop`` keep their keys."""
import http.client
import json

import pytest

from cain_amd.serve.server import EngineBackend, FakeBackend, ServerThread, StopStreamer
from stopseq_cases import boundary_stop

MODEL = "tiny-llama3.1:8b"
PLAIN_KEYS = {"model", "created_at", "response", "done", "done_reason", "context", "total_duration", "load_duration",
              "prompt_eval_count", "prompt_eval_duration", "eval_count", "eval_duration", "cain_ttft_ns"}
OPTS = {"temperature": 0.0, "num_predict": 40}


def _post(server, path, body):
    conn = http.client.HTTPConnection(*server.server.server_address[:2])
    conn.request("POST", path, json.dumps(body))
    r = conn.getresponse()
    raw = r.read().decode()
    conn.close()
    return r.status, raw


def _bodies(extra):
    return (("/api/generate", {"model": MODEL, "prompt": "tell me a story", "stream": False, **extra}),
            ("/api/chat", {"model": MODEL, "messages": [{"role": "user", "content": "tell me a story"}],
                           "stream": False, **extra}))


def _text(path, d):
    return d["message"]["content"] if path == "/api/chat" else d["response"]


@pytest.fixture(scope="module")
def backend():
    return EngineBackend([MODEL], device="cpu", max_batch=2, max_context=256)


@pytest.fixture(scope="module")
def server(backend):
    with ServerThread(backend) as s:
        yield s


def _free_and_stop(server, backend, path, body):
    """The free response of ``body`` and a stop string inside it that spans a token boundary (stopseq_cases)."""
    status, raw = _post(server, path, {**body, "options": OPTS})
    assert status == 200, raw
    free = json.loads(raw)
    eng = backend.engine(MODEL)
    toks = eng.generate([backend.prompt_for(MODEL, body, chat=path == "/api/chat")], 40,
                        {"temperature": 0.0})[0].tokens
    assert eng.tokenizer.decode(toks) == _text(path, free)
    pieces = eng._piece_vocab()
    found = boundary_stop([pieces[t] for t in toks])
    assert found is not None
    st, n_tok, hit_start = found
    raw_bytes = b"".join(pieces[t] for t in toks[:n_tok])
    return free, st.decode(), n_tok, raw_bytes[:hit_start].decode().lstrip()


def test_stop_cuts_the_response_on_both_endpoints(server, backend):
    for path, body in _bodies({}):
        free, stop, n_tok, want = _free_and_stop(server, backend, path, body)
        assert stop in _text(path, free) and free["done_reason"] == "length" and free["eval_count"] == 40
        for value in (stop, [stop], ["\x00never", stop]):  # a string or a list
            status, raw = _post(server, path, {**body, "options": {**OPTS, "stop": value}})
            assert status == 200, raw
            d = json.loads(raw)
            print(path, "free:", repr(_text(path, free)), "stop:", repr(stop), "got:", repr(_text(path, d)))
            assert _text(path, d) == want and stop not in _text(path, d)
            assert d["done_reason"] == "stop" and d["eval_count"] == n_tok
            assert set(d) == set(free)  # no new keys


def test_streamed_and_whole_responses_agree(server, backend):
    for path, body in _bodies({}):
        free, stop, n_tok, want = _free_and_stop(server, backend, path, body)
        opts = {**OPTS, "stop": [stop]}
        status, raw = _post(server, path, {**body, "stream": True, "options": opts, "logprobs": True})
        lines = [json.loads(ln) for ln in raw.splitlines() if ln.startswith("{")]
        assert status == 200 and lines[-1]["done"] and lines[-1]["done_reason"] == "stop"
        assert lines[-1]["eval_count"] == n_tok
        sent = ""
        for ln in lines:  # no prefix of what was streamed exceeds the final text
            sent += _text(path, ln)
            assert want.startswith(sent), (sent, want)
        assert sent == want and stop not in sent
        # logprob entries are not held back: one per generated token, the final one included
        assert sum(len(ln.get("logprobs") or []) for ln in lines) == n_tok


def test_stop_streamer_holds_back_what_may_become_a_stop(backend):
    """Token by token (the server pushes a graph's worth at a time; one at a time is the hardest case): after every
    push the text sent is a prefix of the final text, a never-matching string releases everything at the end."""
    eng = backend.engine(MODEL)
    toks = eng.generate([[1, 40, 41, 42]], 40, {"temperature": 0.0, "eos_id": -1})[0].tokens
    pieces = eng._piece_vocab()
    st, n_tok, hit_start = boundary_stop([pieces[t] for t in toks])
    res = eng.generate([[1, 40, 41, 42]], 40, {"temperature": 0.0, "eos_id": -1, "stop": [st.decode()]})[0]
    s = StopStreamer(eng, [st.decode()], eng.tokenizer)
    sent = ""
    for t in res.tokens:
        sent += s.push([t])
        assert res.text.startswith(sent)
    assert sent + s.finish(res.text) == res.text
    full = eng.tokenizer.decode(toks)
    near = st.decode()[:-1] + "\x00"  # all but the last byte occur: held, then released
    s = StopStreamer(eng, [near], eng.tokenizer)
    sent, held = "", False
    for t in toks:
        sent += s.push([t])
        assert full.startswith(sent)
        held |= len(sent) < len(eng.tokenizer.decode(s.ids))
    assert held and sent + s.finish(full) == full


@pytest.mark.parametrize("stop,msg", [([1, 2], "stop_ids"), (7, "stop_ids"), ("", "empty"), (["a", ""], "empty"),
                                      (["x"] * 9, "limit is 8"), ("y" * 33, "33 bytes"), ({"a": 1}, "stop_ids"),
                                      (["é" * 17], "34 bytes")])
def test_bad_stop_is_400(server, stop, msg):
    for path, body in _bodies({"options": {"num_predict": 3, "stop": stop}}):
        status, raw = _post(server, path, body)
        assert status == 400 and msg in json.loads(raw)["error"], raw


def test_stop_on_a_speculative_server_is_400():
    with ServerThread(EngineBackend([MODEL], device="cpu", max_batch=2, max_context=128, speculative=2)) as s:
        for path, body in _bodies({"options": {"num_predict": 3, "stop": ["a"]}}):
            status, raw = _post(s, path, body)
            assert status == 400 and "speculative" in json.loads(raw)["error"]
        status, _ = _post(s, "/api/generate", {"model": MODEL, "prompt": "x", "stream": False,
                                               "options": {"num_predict": 3, "stop": []}})
        assert status == 200  # an empty list is no stop


def test_requests_without_stop_keep_their_keys(server, backend):
    opts = {"temperature": 0.8, "seed": 4, "num_predict": 9}
    eng = backend.engine(MODEL)
    for path, body in _bodies({"options": opts}):
        d = json.loads(_post(server, path, body)[1])
        keys = PLAIN_KEYS - {"response"} | {"message"} if path == "/api/chat" else PLAIN_KEYS
        assert set(d) == keys and d["eval_count"] == 9 and d["done_reason"] == "length"
        if path == "/api/generate":
            prompt = backend.prompt_for(MODEL, body, chat=False)
            assert d["response"] == eng.generate([prompt], 9, {"temperature": 0.8, "seed": 4})[0].text


def test_fake_backend_ignores_stop():
    with ServerThread(FakeBackend([MODEL])) as s:
        status, raw = _post(s, "/api/generate", {"model": MODEL, "prompt": "x", "stream": False,
                                                 "options": {"num_predict": 3, "stop": ["a"]}})
        assert status == 200 and json.loads(raw)["done"] and json.loads(raw)["eval_count"] == 3
