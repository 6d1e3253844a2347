"""Draft-model speculative decoding without a GPU: the host rule (engine/speculative.py "Draft model") on hand-written
cases, the torch backend decoding with it, its refusals, and the server's ``--draft-model``."""
import dataclasses
import http.client
import json
import math

import pytest

from cain_amd.client.ollama import OllamaClient
from cain_amd.engine import speculative as sp
from cain_amd.engine.engine import DecodeEngine
from cain_amd.models import get_config
from cain_amd.models.weights import random_weights
from cain_amd.serve.server import EngineBackend, ServerThread

T = 64          # context of the hand-written cases
DV, DBOS = 100, 1  # draft vocabulary and bos id of the hand-written cases
T_MAX = 256
TARGET, DRAFT = "tiny-qwen2:7b", "tiny-qwen2:1.5b"
PROMPT = "In 100 words, please give me information about India"
GREEDY = dict(temperature=0.0, repeat_penalty=1.0, eos_id=-1)
SEEDED = dict(temperature=0.8, seed=21, eos_id=-1)
NB = sp.NO_BUDGET


def rows(seq, dvalid, K=3, ng=0, max_new=1000, T_max=T, **kw):
    return sp.draft_model_rows(seq, len(seq) - 1, ng, K, T_max, max_new, dvalid, DV, DBOS, **kw)


# ------------------------------------------------------------------------------------------ the rule, by hand
def test_catch_up_of_one_row_and_of_two():
    s = [5, 6, 7, 8]  # pos 3
    # the draft cache holds positions 0 .. 2: the sequence's own row only
    assert rows(s, 3) == (3, sp.MASKED_ROW, (8, 3, 0, 0, NB, 0))
    # it ends one short (the step before accepted every draft): seq[2] at position 2 first, KV only (done = 1)
    assert rows(s, 2, ng=4, slot=2) == (3, (7, 2, 2, 4, NB, 1), (8, 3, 2, 4, NB, 0))


def test_d_clipped_by_the_context_and_by_the_budget():
    s = list(range(10, 10 + T - 2))  # pos T - 3: two positions left
    assert rows(s, T - 3, K=7)[0] == 2
    assert rows([5, 6, 7], 2, K=7, ng=7, max_new=10)[0] == 2  # two more tokens after this one
    assert rows([5, 6, 7], 2, K=7, ng=9, max_new=10) == (0, sp.MASKED_ROW, sp.MASKED_ROW)  # the last token: no row
    assert rows(list(range(T)), T - 1, K=3) == (0, sp.MASKED_ROW, sp.MASKED_ROW)


def test_done_and_masked_sequences_run_no_row():
    assert rows([5, 6, 7], 2, done=True) == (0, sp.MASKED_ROW, sp.MASKED_ROW)
    assert rows([5, 6, 7], 2, slot=-1) == (0, sp.MASKED_ROW, sp.MASKED_ROW)


def test_token_outside_the_draft_vocabulary_enters_as_bos():
    assert sp.draft_token(DV - 1, DV, DBOS) == DV - 1 and sp.draft_token(DV, DV, DBOS) == DBOS
    d, catch_up, own = rows([5, DV + 3, DV], 1)
    assert catch_up[0] == DBOS and own[0] == DBOS and catch_up[1:3] == (1, 0) and own[1:3] == (2, 0)
    assert sp.draft_model_next(DV + 7, 1, 2, 0, 3, 0, DV, DBOS) == (DBOS, 3, 0, 1, NB, 0)


def test_next_rows_and_given():
    # pos 9, ng 4, d = 2 of K = 3: forward 2 runs d_1 at position 10 with n_gen 5, forward 3 is masked
    assert sp.draft_model_next(41, 1, 9, 4, 2, 1, DV, DBOS) == (41, 10, 1, 5, NB, 0)
    assert sp.draft_model_next(42, 2, 9, 4, 2, 1, DV, DBOS) == sp.MASKED_ROW
    g = [7] * 12
    sp.draft_model_given(g, 4, [41, 42], 3)
    assert g == [7, 7, 7, 7, 41, 42, -1, 7, 7, 7, 7, 7]
    g = [7] * 12
    sp.draft_model_given(g, 4, [41, 42, 43], 3)  # d == K: no end mark
    assert g == [7, 7, 7, 7, 41, 42, 43, 7, 7, 7, 7, 7]
    assert sp.given_draft([7, 7, 7, 7, 41, 42, -1, 7], 4, 3) == [41, 42]


@pytest.mark.parametrize("a", [0, 1, 2, 3])
def test_dvalid_after_a_step(a):
    """d = 3 drafts from pos 9: the draft cache holds positions 9, 10, 11 (tok, d_1, d_2).  With a < d accepted the
    next step needs one row, with a == d two (position pos + d was never run by the draft model)."""
    drafts = [41, 42, 43]
    sampled = [t if j < a else 99 for j, t in enumerate(drafts)] + [50]
    st = sp.SeqState(tok=8, pos=9, max_new=100, seq=list(range(10)))
    assert st.commit_step(drafts, sampled, T) == a + 1 and st.pos == 9 + a + 1
    dv = sp.dvalid_after(9, 3, st.pos)
    assert dv == min(9 + 3, 9 + a + 1)
    d, catch_up, own = sp.draft_model_rows(st.seq, st.pos, st.n_gen, 3, T, st.max_new, dv, DV, DBOS)
    assert own[:2] == (st.tok, st.pos)
    assert (catch_up == sp.MASKED_ROW) == (a < 3)
    if a == 3:
        assert catch_up[:2] == (43, 12) and catch_up[5] == 1


def test_one_token_prompt():
    """Nothing to prefill: dvalid = 0 = pos, the first step runs the prompt's token alone."""
    assert rows([9], 0) == (3, sp.MASKED_ROW, (9, 0, 0, 0, NB, 0))


# ------------------------------------------------------------------------------------------ the torch backend
KW = dict(device="cpu", max_batch=1, max_context=T_MAX, seed=13)


@pytest.fixture(scope="module")
def target_weights():
    return random_weights(get_config(TARGET), device="cpu", seed=13)


def _rule_d(prompt_len, step_tokens, K, n):
    pos, ng, out = prompt_len - 1, 0, 0
    for c in step_tokens:
        out += sp.clip(K, pos, ng, K, T_MAX, n)
        pos, ng = pos + c, ng + c
    return out


@pytest.mark.parametrize("K", [3, 7])
@pytest.mark.parametrize("opts", [GREEDY, SEEDED], ids=["greedy", "seeded"])
def test_any_draft_same_tokens(target_weights, K, opts):
    n = 40
    base = DecodeEngine(TARGET, weights=target_weights, speculative=K, **KW).generate([PROMPT], n, [opts],
                                                                                      drafts=[[]])[0]
    eng = DecodeEngine(TARGET, weights=target_weights, speculative=K, draft_model=DRAFT, **KW)
    assert eng.draft is not None and eng.draft.cfg.name == DRAFT and eng.draft.speculative == 0
    r = eng.generate([PROMPT], n, [opts])[0]
    assert r.tokens == base.tokens and len(r.tokens) == n
    assert r.eval_count == sum(r.step_tokens) and r.decode_steps == len(r.step_tokens)
    assert r.draft_count == _rule_d(len(r.prompt_tokens), r.step_tokens, K, n)
    assert 0 <= r.draft_accepted <= r.draft_count
    j = r.ollama_json()
    assert j["draft_count"] == r.draft_count and j["draft_accepted_count"] == r.draft_accepted


@pytest.mark.parametrize("K", [3, 7])
def test_self_draft_accepts_everything(target_weights, K):
    n = 41
    plain = DecodeEngine(TARGET, weights=target_weights, **KW).generate([PROMPT], n, [GREEDY])[0]
    given = DecodeEngine(TARGET, weights=target_weights, speculative=K, **KW)
    g = given.generate([PROMPT], n, [GREEDY], drafts=[plain.tokens])[0]
    # the input is one on which the K + 1-row forward itself reproduces plain decoding at every row
    assert g.tokens == plain.tokens and g.draft_accepted == g.draft_count and g.decode_steps == math.ceil(n / (K + 1))
    eng = DecodeEngine(TARGET, weights=target_weights, speculative=K, draft_model=target_weights, **KW)
    r = eng.generate([PROMPT], n, [GREEDY])[0]
    assert r.tokens == plain.tokens
    assert r.draft_accepted == r.draft_count == g.draft_count
    assert r.decode_steps == math.ceil(n / (K + 1)) and r.step_tokens == g.step_tokens


def test_one_token_prompt_and_context_end(target_weights):
    eng = DecodeEngine(TARGET, weights=target_weights, speculative=3, draft_model=DRAFT, device="cpu", max_batch=1,
                       max_context=32, seed=13)
    base = DecodeEngine(TARGET, weights=target_weights, speculative=3, device="cpu", max_batch=1, max_context=32,
                        seed=13)
    for prompt in ([7], list(range(20, 20 + 29))):
        r = eng.generate([prompt], 100, [GREEDY])[0]
        assert r.tokens == base.generate([prompt], 100, [GREEDY], drafts=[[]])[0].tokens
        assert len(r.tokens) == 32 - len(prompt)


# ------------------------------------------------------------------------------------------ refusals
class _Pieces:
    """A "real" tokenizer as far as the check goes: not the synthetic one, ``piece`` per id."""

    def __init__(self, shift=None):
        self.shift = shift

    def piece(self, t):
        return f"p{t + 1 if t == self.shift else t}"

    def encode(self, text, add_bos=True):
        return [1, 20, 21]

    def decode(self, ids):
        return " ".join(map(str, ids))


def test_refusals(target_weights, monkeypatch):
    kw = dict(device="cpu", max_context=64)
    with pytest.raises(ValueError, match="speculative"):
        DecodeEngine(TARGET, draft_model=DRAFT, **kw)
    short = random_weights(dataclasses.replace(get_config(DRAFT), max_context=32), device="cpu", seed=1)
    with pytest.raises(ValueError, match="max_context"):
        DecodeEngine(TARGET, speculative=3, draft_model=short, **kw)
    eng = DecodeEngine(TARGET, weights=target_weights, speculative=3, draft_model=DRAFT, **kw)
    with pytest.raises(ValueError, match="draft model"):
        eng.generate([[1, 2]], 4, drafts=[[5]])
    with pytest.raises(ValueError, match="logprobs"):
        eng.generate([[1, 2]], 4, logprobs=True)
    with pytest.raises(ValueError, match="format"):
        eng.generate([[1, 2]], 4, format="json")
    with pytest.raises(ValueError, match="prefix_cache"):
        DecodeEngine(TARGET, speculative=3, draft_model=DRAFT, prefix_cache=True, **kw)
    # two real tokenizers: equal pieces pass, one differing piece inside the common id range does not
    from cain_amd.engine import engine as engine_mod

    monkeypatch.setattr(engine_mod, "get_tokenizer", lambda cfg: _Pieces(5 if cfg.name == DRAFT else None))
    with pytest.raises(ValueError, match="tokenizer"):
        DecodeEngine(TARGET, weights=target_weights, speculative=3, draft_model=DRAFT, **kw)
    monkeypatch.setattr(engine_mod, "get_tokenizer", lambda cfg: _Pieces())
    assert DecodeEngine(TARGET, weights=target_weights, speculative=3, draft_model=DRAFT, **kw).draft is not None


def test_env_switch(target_weights, monkeypatch):
    monkeypatch.setenv("CAIN_DRAFT_MODEL", DRAFT)
    eng = DecodeEngine(TARGET, weights=target_weights, device="cpu", max_context=64, speculative=2)
    assert eng.draft is not None and eng.draft.cfg.name == DRAFT
    monkeypatch.delenv("CAIN_DRAFT_MODEL")
    assert DecodeEngine(TARGET, weights=target_weights, device="cpu", max_context=64, speculative=2).draft is None
    from cain_amd.experiments.study import StudySettings

    monkeypatch.setenv("CAIN_STUDY_DRAFT_MODEL", DRAFT)
    assert StudySettings.from_env().draft_model == DRAFT


# ------------------------------------------------------------------------------------------ the server
def _post(server, path, body):
    conn = http.client.HTTPConnection(*server.server.server_address[:2])
    conn.request("POST", path, json.dumps(body))
    out = json.loads(conn.getresponse().read())
    conn.close()
    return out


def test_server_names_the_draft_model_and_counts_drafts():
    with pytest.raises(ValueError, match="speculative"):
        EngineBackend([TARGET], device="cpu", draft_model=DRAFT)
    kw = dict(device="cpu", max_batch=2, max_context=128)
    with ServerThread(EngineBackend([TARGET], speculative=3, draft_model=DRAFT, **kw)) as srv, \
            ServerThread(EngineBackend([TARGET], speculative=3, **kw)) as ngram:
        opts = {"temperature": 0.0, "num_predict": 12}
        r = OllamaClient(srv.url).generate(TARGET, PROMPT, options=opts)
        assert r.eval_count == 12 and 0 <= r.data["draft_accepted_count"] <= r.data["draft_count"]
        assert r.data["draft_count"] > 0  # a draft model always drafts; the n-gram lookup needs a repeat
        assert r.text == OllamaClient(ngram.url).generate(TARGET, PROMPT, options=opts).text
        label = f"draft:{DRAFT}-k3"
        assert _post(srv, "/api/show", {"model": TARGET})["details"]["speculative"] == label
        conn = http.client.HTTPConnection(*srv.server.server_address[:2])
        conn.request("GET", "/api/ps")
        models = json.loads(conn.getresponse().read())["models"]
        conn.close()
        assert models and all(m.get("speculative") == label for m in models)
