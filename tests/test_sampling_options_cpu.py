"""``min_p``, ``presence_penalty`` and ``frequency_penalty`` on the torch backend and through the server (no GPU):
what ``_row_options`` accepts and refuses, the 400s on both endpoints, the refusal next to speculative decoding,
neutral values leaving seeded tokens alone, and a presence penalty large enough that no id can recur inside the
penalty window."""
import http.client
import json
import math

import pytest

from cain_amd.engine import DecodeEngine
from cain_amd.engine.engine import SAMPLE_EXT_DEFAULTS, _row_options
from cain_amd.serve.server import EngineBackend, FakeBackend, ServerThread

MODEL = "tiny-gemma:2b"  # random-init Gemma repeats itself under greedy decoding (README): the control below shows it
KEYS = ("min_p", "presence_penalty", "frequency_penalty")
BAD = [({"min_p": 1.5}, "min_p"), ({"min_p": -0.1}, "min_p"), ({"min_p": "0.1"}, "min_p"),
       ({"presence_penalty": -0.5}, "presence_penalty"), ({"frequency_penalty": -1e-9}, "frequency_penalty"),
       ({"presence_penalty": [1]}, "presence_penalty"), ({"frequency_penalty": True}, "frequency_penalty")]
NON_FINITE = [{"min_p": math.nan}, {"presence_penalty": math.inf}, {"frequency_penalty": math.nan}]


def repeats(tokens, window=64):
    """Positions whose id already occurs among the ``window`` tokens before it."""
    return [i for i in range(len(tokens)) if tokens[i] in tokens[max(0, i - window):i]]


@pytest.fixture(scope="module")
def eng():
    e = DecodeEngine(MODEL, device="cpu", max_batch=2, max_context=512, seed=3)
    assert e.cfg.vocab > 65
    return e


def test_row_options_accept_and_validate(eng):
    assert {k: _row_options(None, eng.cfg, 0, 0)[k] for k in KEYS} == SAMPLE_EXT_DEFAULTS == dict.fromkeys(KEYS, 0.0)
    o = _row_options({"min_p": 0.05, "presence_penalty": 1, "frequency_penalty": 0.25, "temperature": 1.2}, eng.cfg, 0, 0)
    assert (o["min_p"], o["presence_penalty"], o["frequency_penalty"], o["temperature"]) == (0.05, 1.0, 0.25, 1.2)
    assert all(isinstance(o[k], float) for k in KEYS)
    o = _row_options({"min_p": None, "presence_penalty": None, "frequency_penalty": 0}, eng.cfg, 0, 0)  # None: default
    assert [o[k] for k in KEYS] == [0.0, 0.0, 0.0]
    assert _row_options({"min_p": 1.0}, eng.cfg, 0, 0)["min_p"] == 1.0 and _row_options({"min_p": 0}, eng.cfg, 0, 0)
    for bad, name in BAD + [(b, next(iter(b))) for b in NON_FINITE]:
        with pytest.raises(ValueError, match=name):
            _row_options(bad, eng.cfg, 0, 0)
        with pytest.raises(ValueError, match=name):
            eng.generate(["x"], 2, bad)
    # the options this project does not implement stay ignored
    assert "typical_p" not in _row_options({"typical_p": 0.5, "tfs_z": 2.0, "mirostat": 1}, eng.cfg, 0, 0)


def test_neutral_values_leave_seeded_tokens_alone(eng):
    base = dict(temperature=0.9, seed=5, eos_id=-1)
    a = eng.generate(["hello"], 24, base)[0].tokens
    b = eng.generate(["hello"], 24, dict(base, min_p=0.0, presence_penalty=0.0, frequency_penalty=0))[0].tokens
    c = eng.generate(["hello"], 24, dict(base, min_p=0.9))[0].tokens
    assert a == b and len(a) == 24
    assert c != a  # and a non-neutral value is not dropped on the way


def test_presence_penalty_keeps_ids_out_of_the_window(eng):
    greedy = dict(temperature=0.0, repeat_penalty=1.0, repeat_last_n=64, eos_id=-1)
    control = eng.generate(["tell me a story"], 150, greedy)[0].tokens
    assert len(control) == 150 and len(repeats(control)) > 100  # the control repeats itself: the test shows something
    got = eng.generate(["tell me a story"], 150, dict(greedy, presence_penalty=1000.0))[0].tokens
    assert len(got) == 150 and repeats(got) == []
    assert got[0] == control[0]  # nothing to penalise before the first token
    # a window of 8: an id may come back after 8 others, never sooner
    got8 = eng.generate(["tell me a story"], 150, dict(greedy, presence_penalty=1000.0, repeat_last_n=8))[0].tokens
    assert repeats(got8, 8) == [] and repeats(got8) != []


def test_frequency_penalty_grows_with_the_count(eng):
    """Greedy with a frequency penalty of 0.5 and nothing else: every token is the argmax of the torch oracle's
    logits minus 0.5 per earlier occurrence in the window, which sample_host_candidates computes (checked against the
    reference in test_sampler_ext_ref.py); here only that the option reaches it: the output differs from the
    control's and from the presence-only output."""
    greedy = dict(temperature=0.0, repeat_penalty=1.0, repeat_last_n=64, eos_id=-1)
    control = eng.generate(["tell me a story"], 60, greedy)[0].tokens
    freq = eng.generate(["tell me a story"], 60, dict(greedy, frequency_penalty=0.5))[0].tokens
    assert freq != control and len(repeats(freq)) < len(repeats(control))


def test_speculative_engine_refuses_non_neutral_values():
    spec = DecodeEngine(MODEL, device="cpu", max_batch=2, max_context=128, seed=3, speculative=2)
    for k in KEYS:
        with pytest.raises(ValueError, match="speculative"):
            spec.generate(["x"], 3, {k: 0.5})
        with pytest.raises(ValueError, match="speculative"):
            spec.generate(["x"], 3, {k: 0.5}, drafts=[[1, 2]])
    assert len(spec.generate(["x"], 3, {"min_p": 0.0, "presence_penalty": 0, "eos_id": -1})[0].tokens) == 3


# ---- the server

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


@pytest.fixture(scope="module")
def backend():
    return EngineBackend([MODEL], device="cpu", max_batch=2, max_context=256)


@pytest.fixture(scope="module")
def server(backend):
    with ServerThread(backend) as s:
        yield s


@pytest.mark.parametrize("bad,name", BAD)
def test_out_of_range_is_400(server, bad, name):
    for path, body in _bodies({"options": {"num_predict": 3, **bad}}):
        status, raw = _post(server, path, body)
        assert status == 400 and name in json.loads(raw)["error"], raw


def test_options_reach_the_engine_through_the_server(server, backend):
    opts = {"temperature": 0.0, "repeat_penalty": 1.0, "eos_id": -1, "num_predict": 80}
    eng = backend.engine(MODEL)
    for path, body in _bodies({}):
        prompt = backend.prompt_for(MODEL, body, chat=path == "/api/chat")
        status, raw = _post(server, path, {**body, "options": {**opts, "presence_penalty": 1000.0}})
        assert status == 200, raw
        d = json.loads(raw)
        want = eng.generate([prompt], 80, {**opts, "presence_penalty": 1000.0})[0]
        assert (d["message"]["content"] if path == "/api/chat" else d["response"]) == want.text
        assert repeats(want.tokens) == [] and d["eval_count"] == 80
        free = eng.generate([prompt], 80, opts)[0]
        assert repeats(free.tokens) != [] and free.text != want.text
        # neutral values and null are accepted
        status, raw = _post(server, path, {**body, "options": {**opts, "min_p": 0, "presence_penalty": None,
                                                               "frequency_penalty": 0.0}})
        assert status == 200 and json.loads(raw)["eval_count"] == 80


def test_speculative_server_refuses_non_neutral_values():
    with ServerThread(EngineBackend([MODEL], device="cpu", max_batch=2, max_context=128, speculative=2)) as s:
        for k in KEYS:
            for path, body in _bodies({"options": {"num_predict": 3, k: 0.25}}):
                status, raw = _post(s, path, body)
                assert status == 400 and "speculative" in json.loads(raw)["error"], raw
        for path, body in _bodies({"options": {"num_predict": 3, "min_p": 0.0, "presence_penalty": 0}}):
            assert _post(s, path, body)[0] == 200  # neutral values are no request for the feature
        status, raw = _post(s, "/api/generate", {"model": MODEL, "prompt": "x", "stream": False,
                                                 "options": {"num_predict": 3, "min_p": 2}})
        assert status == 400 and "min_p" in json.loads(raw)["error"]  # the range is checked first


def test_fake_backend_checks_the_range_and_ignores_the_rest():
    with ServerThread(FakeBackend([MODEL])) as s:
        body = {"model": MODEL, "prompt": "x", "stream": False}
        assert _post(s, "/api/generate", {**body, "options": {"num_predict": 3, "min_p": 0.1}})[0] == 200
        assert _post(s, "/api/generate", {**body, "options": {"num_predict": 3, "min_p": 7}})[0] == 400
