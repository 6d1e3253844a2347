"""Ollama's ``format`` field on ``/api/generate`` and ``/api/chat``, on the torch backend (no GPU)."""
import http.client
import json

import pytest

from cain_amd.engine import jsonmode as jm
from cain_amd.serve.server import EngineBackend, FakeBackend, ServerThread
from jsonmode_vocab import json_test_vocabulary

MODEL = "tiny-llama3.1:8b"
PLAIN_KEYS = {"model", "created_at", "response", "done", "done_reason", "context", "total_duration", "load_duration",
              "prompt_eval_count", "prompt_eval_duration", "eval_count", "eval_duration", "cain_ttft_ns"}


def _post(server, path, body):
    conn = http.client.HTTPConnection(*server.server.server_address[:2])
    conn.request("POST", path, json.dumps(body))
    r = conn.getresponse()
    raw = r.read().decode()
    conn.close()
    return r.status, raw


def _bodies(extra):
    return (("/api/generate", {"model": MODEL, "prompt": "an object please", "stream": False, **extra}),
            ("/api/chat", {"model": MODEL, "messages": [{"role": "user", "content": "an object please"}],
                           "stream": False, **extra}))


@pytest.fixture(scope="module")
def backend():
    be = EngineBackend([MODEL], device="cpu", max_batch=2, max_context=256)
    return be


@pytest.fixture(scope="module")
def server(backend):
    with ServerThread(backend) as s:
        yield s


def _text(path, d):
    return d["message"]["content"] if path == "/api/chat" else d["response"]


def test_json_needs_a_vocabulary_that_spells_json(server, backend):
    """(runs first: the random-init tag's synthetic tokenizer has no punctuation)"""
    assert backend.engine(MODEL)._json_pieces is None
    for path, body in _bodies({"format": "json"}):
        status, raw = _post(server, path, body)
        assert status == 400 and "vocabulary cannot spell JSON" in json.loads(raw)["error"]


def test_format_json_on_both_endpoints(server, backend):
    backend.engine(MODEL).set_json_vocab(json_test_vocabulary())
    seen = set()
    for seed in range(4):
        for budget in (6, 200):
            opts = {"temperature": 1.0, "seed": seed, "num_predict": budget}
            for path, body in _bodies({"format": "json", "options": opts}):
                status, raw = _post(server, path, body)
                assert status == 200, raw
                d = json.loads(raw)
                text = _text(path, d)
                seen.add(d["done_reason"])
                if d["done_reason"] == "stop":
                    assert text.endswith("}") and isinstance(json.loads(text), dict) and d["eval_count"] <= budget
                else:
                    assert d["done_reason"] == "length" and d["eval_count"] == budget
                    assert jm.viable(text.encode("utf-8").rstrip(b"\xef\xbf\xbd"))  # (a character cut at the budget)
    assert seen == {"stop", "length"}


def test_format_json_streams_the_same_text(server, backend):
    backend.engine(MODEL).set_json_vocab(json_test_vocabulary())
    opts = {"temperature": 1.0, "seed": 2, "num_predict": 200}
    whole = json.loads(_post(server, "/api/generate", {"model": MODEL, "prompt": "p", "stream": False,
                                                       "format": "json", "options": opts})[1])
    status, raw = _post(server, "/api/generate", {"model": MODEL, "prompt": "p", "format": "json", "options": opts})
    lines = [json.loads(ln) for ln in raw.splitlines() if ln.startswith("{")]
    assert status == 200 and lines[-1]["done"] and lines[-1]["done_reason"] == whole["done_reason"]
    assert "".join(ln["response"] for ln in lines) == whole["response"]


@pytest.mark.parametrize("fmt,msg", [({"type": "object", "properties": {}}, 'format: JSON schema is not supported, '
                                                                             'only "json"'),
                                     ("xml", "format"), (7, "format"), (["json"], "format"), (True, "format")])
def test_other_formats_are_400(server, fmt, msg):
    for path, body in _bodies({"format": fmt}):
        status, raw = _post(server, path, body)
        assert status == 400 and msg in json.loads(raw)["error"]


def test_absent_or_empty_format_changes_nothing(server, backend):
    opts = {"temperature": 0.8, "seed": 4, "num_predict": 9}
    eng = backend.engine(MODEL)
    for path, body in _bodies({"options": opts}):
        absent = json.loads(_post(server, path, body)[1])
        empty = json.loads(_post(server, path, {**body, "format": ""})[1])
        keys = PLAIN_KEYS - {"response"} | {"message"} if path == "/api/chat" else PLAIN_KEYS
        assert set(absent) == set(empty) == keys
        assert _text(path, absent) == _text(path, empty) and absent["eval_count"] == 9
        if path == "/api/generate":  # the text the engine gives for the prompt with no format at all
            prompt = backend.prompt_for(MODEL, body, chat=False)
            assert absent["response"] == eng.generate([prompt], 9, {"temperature": 0.8, "seed": 4})[0].text


def test_format_on_a_speculative_server_is_400():
    with ServerThread(EngineBackend([MODEL], device="cpu", max_batch=2, max_context=128, speculative=2)) as s:
        for path, body in _bodies({"format": "json"}):
            status, raw = _post(s, path, body)
            assert status == 400 and "speculative" in json.loads(raw)["error"]
        status, _ = _post(s, "/api/generate", {"model": MODEL, "prompt": "x", "stream": False,
                                               "options": {"num_predict": 3}})
        assert status == 200


def test_fake_backend_ignores_the_field():
    with ServerThread(FakeBackend([MODEL])) as s:
        status, raw = _post(s, "/api/generate", {"model": MODEL, "prompt": "x", "stream": False, "format": "json",
                                                 "options": {"num_predict": 3}})
        assert status == 200 and json.loads(raw)["done"]


def test_options_format_is_the_field(server, backend):
    """``options.format`` (the engine's per-row key) gets the field's checks and the field's decoder."""
    backend.engine(MODEL).set_json_vocab(json_test_vocabulary())
    opts = {"temperature": 1.0, "seed": 2, "num_predict": 200}
    for path, body in _bodies({}):
        top = json.loads(_post(server, path, {**body, "format": "json", "options": opts})[1])
        via = _post(server, path, {**body, "options": {**opts, "format": "json"}})
        assert via[0] == 200 and _text(path, json.loads(via[1])) == _text(path, top)
        assert json.loads(via[1])["done_reason"] == top["done_reason"]
        status, raw = _post(server, path, {**body, "options": {**opts, "format": "xml"}})
        assert status == 400 and "format" in json.loads(raw)["error"]
    with ServerThread(EngineBackend([MODEL], device="cpu", max_batch=2, max_context=128, speculative=2)) as s:
        status, raw = _post(s, "/api/generate", {"model": MODEL, "prompt": "x", "stream": False,
                                                 "options": {"format": "json"}})
        assert status == 400 and "speculative" in json.loads(raw)["error"]


def test_unloaded_random_init_tag_is_judged_without_loading_it():
    be = EngineBackend([MODEL], device="cpu", max_batch=2, max_context=128)
    with ServerThread(be) as s:
        status, raw = _post(s, "/api/generate", {"model": MODEL, "prompt": "x", "stream": False, "format": "json"})
        assert status == 400 and "vocabulary cannot spell JSON" in json.loads(raw)["error"]
        assert MODEL not in be.engines  # the load stays with the scheduler thread
