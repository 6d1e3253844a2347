"""``--speculative`` of the Ollama-compatible server, on the torch backend (no GPU): the same answer, two more keys,
no logprobs."""
import http.client
import json

import pytest

from cain_amd.client.ollama import OllamaClient
from cain_amd.serve.server import EngineBackend, ServerThread

MODEL = "tiny-qwen2:1.5b"
PROMPT = "the cat sat on the mat and the cat sat on the mat and the cat"
SPEC_KEYS = {"draft_count", "draft_accepted_count"}


@pytest.fixture(scope="module")
def servers():
    kw = dict(device="cpu", max_batch=2, max_context=128)
    with ServerThread(EngineBackend([MODEL], **kw)) as plain, \
            ServerThread(EngineBackend([MODEL], speculative=3, **kw)) as spec:
        yield plain, spec


@pytest.mark.parametrize("opts", [{"temperature": 0.0, "num_predict": 20},
                                  {"temperature": 0.8, "seed": 4, "num_predict": 20}], ids=["greedy", "seeded"])
def test_same_response_and_two_new_keys(servers, opts):
    plain, spec = (OllamaClient(s.url) for s in servers)
    a, b = plain.generate(MODEL, PROMPT, options=opts), spec.generate(MODEL, PROMPT, options=opts)
    assert a.text == b.text and a.eval_count == b.eval_count == 20
    assert set(b.data) == set(a.data) | SPEC_KEYS and not SPEC_KEYS & set(a.data)
    assert 0 <= b.data["draft_accepted_count"] <= b.data["draft_count"]
    ca = plain.chat(MODEL, [{"role": "user", "content": PROMPT}], options=opts)
    cb = spec.chat(MODEL, [{"role": "user", "content": PROMPT}], options=opts)
    assert ca.text == cb.text and set(cb.data) == set(ca.data) | SPEC_KEYS
    sb = spec.generate(MODEL, PROMPT, stream=True, options=opts)
    assert sb.text == a.text and SPEC_KEYS <= set(sb.data)


def _post(server, path, body):
    conn = http.client.HTTPConnection(*server.server.server_address[:2])
    conn.request("POST", path, json.dumps(body))
    r = conn.getresponse()
    out = r.status, json.loads(r.read())
    conn.close()
    return out


def test_logprobs_with_speculative_is_400(servers):
    plain, spec = servers
    body = {"model": MODEL, "prompt": "x", "stream": False, "logprobs": True, "options": {"num_predict": 2}}
    status, d = _post(spec, "/api/generate", body)
    assert status == 400 and "speculative" in d["error"]
    status, d = _post(spec, "/api/chat", {**body, "messages": [{"role": "user", "content": "x"}]})
    assert status == 400 and "speculative" in d["error"]
    assert _post(plain, "/api/generate", body)[0] == 200


def test_show_and_ps_name_the_mode(servers):
    plain, spec = servers
    OllamaClient(spec.url).generate(MODEL, "x", options={"num_predict": 1})  # (/api/ps lists models with a queue)
    OllamaClient(plain.url).generate(MODEL, "x", options={"num_predict": 1})
    assert _post(spec, "/api/show", {"model": MODEL})[1]["details"]["speculative"] == "ngram-k3"
    assert "speculative" not in _post(plain, "/api/show", {"model": MODEL})[1]["details"]
    for s, want in ((spec, "ngram-k3"), (plain, None)):
        conn = http.client.HTTPConnection(*s.server.server_address[:2])
        conn.request("GET", "/api/ps")
        models = json.loads(conn.getresponse().read())["models"]
        conn.close()
        assert models and all(m.get("speculative") == want for m in models)


def test_backend_refuses_prefix_cache_with_speculative():
    with pytest.raises(ValueError, match="prefix_cache"):
        EngineBackend([MODEL], device="cpu", speculative=2, prefix_cache=True)
