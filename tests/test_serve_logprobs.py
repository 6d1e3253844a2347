"""``logprobs`` / ``top_logprobs`` of the Ollama-compatible server and client, on the torch backend (no GPU)."""
import http.client
import json

import pytest

from cain_amd.client.ollama import OllamaClient, OllamaError
from cain_amd.serve.server import EngineBackend, FakeBackend, ServerThread

MODEL = "tiny-qwen2:1.5b"
OPTS = {"temperature": 0.8, "seed": 4, "num_predict": 7}
ENTRY_KEYS = {"token", "logprob", "bytes", "id", "top_logprobs"}


@pytest.fixture(scope="module")
def server():
    with ServerThread(EngineBackend([MODEL], device="cpu", max_batch=2, max_context=128)) as s:
        yield s


def _check_entries(entries, n_tokens, n_top):
    assert len(entries) == n_tokens
    for e in entries:
        assert set(e) == ENTRY_KEYS and e["logprob"] <= 0 and isinstance(e["id"], int)
        assert bytes(e["bytes"]).decode("utf-8") == e["token"]
        assert len(e["top_logprobs"]) == n_top
        for t in e["top_logprobs"]:
            assert set(t) == ENTRY_KEYS - {"top_logprobs"} and bytes(t["bytes"]).decode("utf-8") == t["token"]
        lps = [t["logprob"] for t in e["top_logprobs"]]
        assert lps == sorted(lps, reverse=True)
        assert not lps or e["logprob"] <= lps[0] + 1e-12  # nothing is more likely than the first alternative


def test_non_stream_shape_and_old_keys(server):
    c = OllamaClient(server.url)
    plain = c.generate(MODEL, "hello world", options=OPTS)
    r = c.generate(MODEL, "hello world", options=OPTS, logprobs=True, top_logprobs=3)
    assert plain.logprobs is None and "logprobs" not in plain.data
    assert set(r.data) == set(plain.data) | {"logprobs"}
    assert set(plain.data) == {"model", "created_at", "response", "done", "done_reason", "context", "total_duration",
                               "load_duration", "prompt_eval_count", "prompt_eval_duration", "eval_count",
                               "eval_duration", "cain_ttft_ns"}
    assert r.text == plain.text and r.eval_count == 7
    _check_entries(r.logprobs, 7, 3)
    _check_entries(c.generate(MODEL, "hello world", options=OPTS, logprobs=True).logprobs, 7, 0)
    chat = c.chat(MODEL, [{"role": "user", "content": "hi"}], options=OPTS, logprobs=True, top_logprobs=2)
    _check_entries(chat.logprobs, 7, 2)
    plain_chat = c.chat(MODEL, [{"role": "user", "content": "hi"}], options=OPTS)
    assert "logprobs" not in plain_chat.data and set(chat.data) == set(plain_chat.data) | {"logprobs"}


def test_stream_pieces_concatenate_to_the_non_stream_list(server):
    c = OllamaClient(server.url)
    whole = c.generate(MODEL, "stream me", options=OPTS, logprobs=True, top_logprobs=2)
    streamed = c.generate(MODEL, "stream me", stream=True, options=OPTS, logprobs=True, top_logprobs=2)
    assert streamed.text == whole.text
    assert streamed.logprobs == whole.logprobs
    plain = c.generate(MODEL, "stream me", stream=True, options=OPTS)
    assert "logprobs" not in plain.data
    # on the wire: the entries ride in the pieces, every line of a plain request has the old keys only
    conn = http.client.HTTPConnection(*server.server.server_address[:2])
    conn.request("POST", "/api/generate", json.dumps({"model": MODEL, "prompt": "stream me", "options": OPTS,
                                                      "logprobs": True, "top_logprobs": 2}))
    lines = [json.loads(ln) for ln in conn.getresponse().read().decode().splitlines() if ln.startswith("{")]
    conn.close()
    assert sum((ln["logprobs"] for ln in lines if not ln["done"]), []) == whole.logprobs
    assert lines[-1]["done"] and lines[-1]["logprobs"] == []


@pytest.mark.parametrize("fields,msg", [({"logprobs": True, "top_logprobs": 21}, "0..20"),
                                        ({"logprobs": True, "top_logprobs": -1}, "0..20"),
                                        ({"top_logprobs": 3}, "needs logprobs")])
def test_bad_requests_are_400(server, fields, msg):
    for path, body in (("/api/generate", {"model": MODEL, "prompt": "x"}),
                       ("/api/chat", {"model": MODEL, "messages": [{"role": "user", "content": "x"}]})):
        conn = http.client.HTTPConnection(*server.server.server_address[:2])
        conn.request("POST", path, json.dumps({**body, **fields, "stream": False}))
        r = conn.getresponse()
        assert r.status == 400 and msg in json.loads(r.read())["error"]
        conn.close()


def test_fake_backend_refuses_logprobs():
    with ServerThread(FakeBackend(["m:1b"])) as s:
        c = OllamaClient(s.url)
        with pytest.raises(OllamaError, match="400.*no model behind this backend"):
            c.generate("m:1b", "x", options={"num_predict": 2}, logprobs=True)
        assert c.generate("m:1b", "x", options={"num_predict": 2}).eval_count == 2
