"""``min_p``, ``presence_penalty`` and ``frequency_penalty`` through the HIP engine (test-size configs, bf16): the
rows' SampleExt records reach the graph-replayed decode, move with a row that continuous batching compacts, differ
per row of a batch, leave neutral requests' tokens alone and leave the logprobs the model's own."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import test_logprob_gpu as tlg  # noqa: E402  (the decode-vs-score bound of its engines)
from cain_amd.engine import DecodeEngine  # noqa: E402

MODEL = "tiny-gemma:2b"  # random-init Gemma repeats itself under greedy decoding: the controls show it
GREEDY = dict(temperature=0.0, repeat_penalty=1.0, repeat_last_n=64, eos_id=-1)
PROMPT = "tell me a story"


def repeats(tokens, window=64):
    """Positions whose id already occurs among the ``window`` tokens before it."""
    return [i for i in range(len(tokens)) if tokens[i] in tokens[max(0, i - window):i]]


@pytest.fixture(scope="module")
def eng():
    e = DecodeEngine(MODEL, device="cuda", max_batch=4, max_context=512, seed=3, steps_per_graph=4)
    assert e.cfg.vocab > 65
    yield e
    e.close()


def test_presence_penalty_through_graph_replay(eng):
    control = eng.generate([PROMPT], 150, GREEDY)[0].tokens
    assert len(control) == 150 and repeats(control) != []
    got = eng.generate([PROMPT], 150, dict(GREEDY, presence_penalty=1000.0))[0].tokens
    assert eng._graphs  # the decode ran from captured graphs
    assert len(got) == 150 and repeats(got) == []
    assert got[0] == control[0]
    # the graphs captured above serve the next request's values: the record's contents change, not its address
    n_graphs = len(eng._graphs)
    again = eng.generate([PROMPT], 150, GREEDY)[0].tokens
    assert again == control and len(eng._graphs) == n_graphs
    eager = eng.generate([PROMPT], 150, dict(GREEDY, presence_penalty=1000.0), use_graph=False)[0].tokens
    assert eager == got


def test_neutral_values_leave_seeded_tokens_alone(eng):
    base = dict(temperature=0.9, seed=5, eos_id=-1)
    a = eng.generate(["hello"], 40, base)[0].tokens
    b = eng.generate(["hello"], 40, dict(base, min_p=0.0, presence_penalty=0.0, frequency_penalty=0))[0].tokens
    assert a == b and len(a) == 40


def test_record_moves_with_a_compacted_row(eng):
    control = eng.generate([PROMPT], 200, GREEDY)[0].tokens
    assert repeats(control) != []
    cb = eng.continuous()
    rows = cb.admit(["hello there", PROMPT], [8, 200], [None, dict(GREEDY, presence_penalty=1000.0)])
    assert rows == [0, 1]
    owner, out, moved = {0: "A", 1: "B"}, {"A": [], "B": []}, False
    for _ in range(400):
        cb.step()
        new, fin = cb.poll()
        for r, ids in enumerate(new):
            out[owner[r]] += ids
        dead = [r for r, f in enumerate(fin) if f]
        if dead:
            moves = cb.retire(dead)
            moved |= moves == {1: 0}
            owner = {moves.get(r, r): o for r, o in owner.items() if r not in dead}
        if cb.n == 0:
            break
    assert cb.n == 0 and moved and 1 <= len(out["A"]) <= 8
    assert len(out["B"]) == 200 and repeats(out["B"]) == []  # most of it generated from row 0, after the move


def test_mixed_batch_gives_each_row_its_own_values(eng):
    opts = [GREEDY, dict(GREEDY, presence_penalty=1000.0), dict(GREEDY, presence_penalty=1000.0, repeat_last_n=8),
            dict(GREEDY, temperature=0.9, seed=11, min_p=1.0)]
    res = [r.tokens for r in eng.generate([PROMPT] * 4, 60, opts)]
    assert all(len(t) == 60 for t in res)
    assert repeats(res[0]) != []
    assert repeats(res[1]) == []
    assert repeats(res[2], 8) == [] and repeats(res[2]) != []
    # min_p 1.0 keeps only the candidates that tie with the first: a sampling row draws its greedy tokens
    assert res[3] == res[0]


def test_logprobs_stay_the_models_own():
    """A penalised row's logprobs are those of the raw distribution: equal to score() on the generated text within
    the bound tests/test_logprob_gpu.py holds decode against score to, though the tokens are not the raw argmax."""
    key = ("tiny-llama3.1:8b", "bf16")
    e = tlg._engine(*key)
    p = tlg._prompt(9, 21)
    opts = dict(GREEDY, presence_penalty=1000.0, frequency_penalty=0.5)
    r = e.generate([p], 32, [opts], logprobs=True, top_logprobs=2)[0]
    s = e.score([p + r.tokens])[0]
    e.close()
    assert len(r.tokens) == 32 and repeats(r.tokens) == []
    d = float(np.abs(np.array(r.logprobs) - np.array(s.logprobs[len(p) - 1:])).max())
    print(f"penalised decode vs score: max |dlogprob| {d:.4e}")
    assert d <= tlg.ORACLE_BOUND[key]
    assert any(t[0][0] != tok for t, tok in zip(r.top_logprobs, r.tokens))  # the penalty did change the tokens
