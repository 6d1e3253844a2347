"""``POST /api/embed`` and ``POST /api/embeddings`` (no GPU): on ``FakeBackend`` and on ``EngineBackend`` with the
torch backend -- both routes and both client calls, a string, a list and ``[]`` as ``input``, the refusals,
``prompt_eval_count`` summed, ``/api/show``'s ``embedding_length`` and pooling mode, an embed request posted while a
streamed generation is in flight, and the vector against ``DecodeEngine.embed``'s."""
import http.client
import json
import threading

import numpy as np
import pytest

from cain_amd.client.ollama import CurlRequest, OllamaClient, OllamaError
from cain_amd.serve.server import EngineBackend, FakeBackend, ServerThread, embed_pooling_setting

MODEL = "tiny-llama3.1:8b"
CTX = 64


def _post(server, path, body):
    conn = http.client.HTTPConnection(*server.server.server_address[:2])
    conn.request("POST", path, json.dumps(body))
    r = conn.getresponse()
    raw = r.read().decode()
    conn.close()
    return r.status, json.loads(raw)


@pytest.fixture(scope="module")
def backend():
    return EngineBackend([MODEL], device="cpu", max_batch=2, max_context=CTX)


@pytest.fixture(scope="module")
def server(backend):
    with ServerThread(backend) as s:
        yield s


@pytest.fixture(scope="module")
def fake():
    with ServerThread(FakeBackend([MODEL])) as s:
        yield s


@pytest.fixture(params=["fake", "engine"])
def any_server(request, fake, server):
    return fake if request.param == "fake" else server


def test_both_routes_and_input_forms(any_server):
    s = any_server
    st, one = _post(s, "/api/embed", {"model": MODEL, "input": "a red fox"})
    assert st == 200 and set(one) == {"model", "embeddings", "total_duration", "load_duration", "prompt_eval_count"}
    assert one["model"] == MODEL and len(one["embeddings"]) == 1 and one["total_duration"] > 0
    st, many = _post(s, "/api/embed", {"model": MODEL, "input": ["a red fox", "two dogs", ""], "options": {"x": 1},
                                       "keep_alive": "5m"})
    assert st == 200 and len(many["embeddings"]) == 3
    assert many["embeddings"][0] == one["embeddings"][0]  # the same text, the same vector
    assert many["embeddings"][0] != many["embeddings"][1]
    for v in many["embeddings"]:
        assert abs(np.linalg.norm(v) - 1.0) < 1e-5
    singles = [_post(s, "/api/embed", {"model": MODEL, "input": t})[1]["prompt_eval_count"]
               for t in ("a red fox", "two dogs", "")]
    assert many["prompt_eval_count"] == sum(singles) and min(singles) >= 1
    st, none = _post(s, "/api/embed", {"model": MODEL, "input": []})
    assert st == 200 and none["embeddings"] == [] and none["prompt_eval_count"] == 0
    st, old = _post(s, "/api/embeddings", {"model": MODEL, "prompt": "a red fox"})
    assert st == 200 and set(old) == {"embedding"} and old["embedding"] == one["embeddings"][0]


def test_client_calls(any_server):
    c = OllamaClient(any_server.url)
    r = c.embed(MODEL, ["a red fox", "two dogs"])
    assert len(r.embeddings) == 2 and r.prompt_eval_count >= 2 and r.wall_s > 0
    assert c.embed(MODEL, "a red fox").embeddings[0] == r.embeddings[0]
    assert c.embeddings(MODEL, "a red fox") == r.embeddings[0]
    with pytest.raises(OllamaError):
        c.embed("nope:1b", "x")


def test_curl_wrapper_builds_the_embed_request():
    args = CurlRequest("127.0.0.1:1", MODEL, input=["a", 'b "q"'], truncate=False).arguments()
    assert args[-3] == "http://127.0.0.1:1/api/embed"
    assert json.loads(args[-1]) == {"model": MODEL, "input": ["a", 'b "q"'], "truncate": False}
    gen = CurlRequest("127.0.0.1:1", MODEL, "hi", options={"num_predict": 2}).arguments()
    assert gen[-3].endswith("/api/generate") and json.loads(gen[-1])["prompt"] == "hi"


def test_refusals(any_server):
    s = any_server
    for body in ({"model": MODEL, "input": ["ok", 3]}, {"model": MODEL, "input": 7}, {"model": MODEL, "input": [["x"]]},
                 {"input": "x"}, {"model": MODEL, "input": "x", "truncate": "no"}):
        st, d = _post(s, "/api/embed", body)
        assert st == 400 and d["error"], body
    assert _post(s, "/api/embeddings", {"prompt": "x"})[0] == 400
    assert _post(s, "/api/embeddings", {"model": MODEL, "prompt": ["x"]})[0] == 400
    # an unknown model: what /api/generate answers
    gen = _post(s, "/api/generate", {"model": "nope:1b", "prompt": "x", "stream": False})
    for path, body in (("/api/embed", {"model": "nope:1b", "input": "x"}),
                       ("/api/embeddings", {"model": "nope:1b", "prompt": "x"})):
        st, d = _post(s, path, body)
        assert st == gen[0] and "not found" in d["error"]


def test_over_long_input(any_server, backend):
    s = any_server
    long = "word " * 3000
    st, d = _post(s, "/api/embed", {"model": MODEL, "input": ["short", long], "truncate": False})
    assert st == 400 and "context" in d["error"]
    st, d = _post(s, "/api/embed", {"model": MODEL, "input": ["short", long]})
    assert st == 200 and len(d["embeddings"]) == 2
    if s.server.scheduler.backend is backend:
        eng = backend.engine(MODEL)
        assert len(eng.encode(long)) > eng.T_max
        assert d["prompt_eval_count"] == eng.T_max + len(eng.encode("short"))


def test_show_reports_length_and_pooling(fake, server, backend):
    st, d = _post(server, "/api/show", {"model": MODEL})
    assert st == 200 and d["model_info"]["embedding_length"] == backend.engine(MODEL).cfg.d_model
    assert d["details"]["embed_pooling"] == "last"
    st, d = _post(fake, "/api/show", {"model": MODEL})
    assert d["model_info"]["embedding_length"] == FakeBackend.EMBED_DIM and d["details"]["embed_pooling"] == "last"


def test_vector_is_the_engines_and_the_pooling_setting_reaches_it(server, backend, monkeypatch):
    eng = backend.engine(MODEL)
    texts = ["a red fox", "two dogs in the yard"]
    got = _post(server, "/api/embed", {"model": MODEL, "input": texts})[1]["embeddings"]
    assert got == [r.embedding for r in eng.embed(texts)]  # raw text: no chat template
    mean = EngineBackend([MODEL], device="cpu", max_batch=2, max_context=CTX, embed_pooling="mean")
    mean.engines[MODEL] = eng
    with ServerThread(mean) as s:
        got = _post(s, "/api/embed", {"model": MODEL, "input": texts})[1]["embeddings"]
        assert _post(s, "/api/show", {"model": MODEL})[1]["details"]["embed_pooling"] == "mean"
    assert got == [r.embedding for r in eng.embed(texts, pooling="mean")]
    assert got != [r.embedding for r in eng.embed(texts)]
    monkeypatch.setenv("CAIN_EMBED_POOLING", "mean")
    assert embed_pooling_setting() == "mean" and embed_pooling_setting("last") == "last"
    monkeypatch.setenv("CAIN_EMBED_POOLING", "max")
    with pytest.raises(ValueError):
        embed_pooling_setting()


def test_embed_while_a_streamed_generation_is_in_flight(server):
    c = OllamaClient(server.url)
    opts = {"temperature": 0.0, "num_predict": 24}
    alone = c.generate(MODEL, "tell me a story", stream=True, options=opts).text
    want = c.embed(MODEL, "a red fox").embeddings
    got = {}
    started = threading.Event()

    def embed_now():
        started.wait(30)
        got["e"] = c.embed(MODEL, "a red fox").embeddings

    t = threading.Thread(target=embed_now)
    t.start()
    streamed = c.generate(MODEL, "tell me a story", stream=True, options=opts, on_chunk=lambda _: started.set())
    started.set()
    t.join(60)
    assert not t.is_alive() and got["e"] == want
    assert streamed.text == alone
