"""Token log-probabilities on the torch backend (the host definition: float64 log-softmax of the fp32 oracle's
logits), ``score``, and the ``perplexity`` command -- no GPU."""
import json
import math

import numpy as np
import pytest
import torch

from cain_amd.engine import DecodeEngine, logprob_host
from cain_amd.engine.perplexity import perplexity, windows
from cain_amd.models.reference import ReferenceModel

MODEL = "tiny-llama3.1:8b"


@pytest.fixture(scope="module")
def eng():
    return DecodeEngine(MODEL, device="cpu", max_context=128, seed=2)


def _ref_logprobs(eng, ids):
    """float64 log-softmax rows [n, V] of ReferenceModel.forward over ``ids``, computed here from the definition."""
    lg = ReferenceModel(eng.weights).forward(torch.tensor([ids]))[0].double()
    return (lg - torch.logsumexp(lg, dim=-1, keepdim=True)).numpy()


def test_score_matches_reference(eng):
    p = np.random.default_rng(0).integers(3, 1000, size=17).tolist()
    res = eng.score([p, p[:5]], top_logprobs=4)
    ls = _ref_logprobs(eng, p)
    assert res[0].tokens == p and len(res[0].logprobs) == 16 and len(res[1].logprobs) == 4
    for j in range(1, 17):
        assert abs(res[0].logprobs[j - 1] - ls[j - 1, p[j]]) < 1e-6
        top = res[0].top_logprobs[j - 1]
        order = np.lexsort((np.arange(ls.shape[1]), -ls[j - 1]))[:4]
        assert [i for i, _ in top] == order.tolist()
        assert all(abs(v - ls[j - 1, i]) < 1e-6 for i, v in top)
    assert res[1].logprobs == pytest.approx(res[0].logprobs[:4], abs=1e-6)
    assert res[0].nll == pytest.approx(-sum(res[0].logprobs))
    assert eng.score([[7]])[0].logprobs == []


def test_generate_logprobs_match_reference_and_tokens_unchanged(eng):
    opts = [dict(temperature=0.8, repeat_penalty=1.3, seed=5, eos_id=-1), dict(temperature=0.0, eos_id=-1)]
    prompts = [[5, 6, 7, 8], [9, 10]]
    off = eng.generate(prompts, 6, opts)
    on = eng.generate(prompts, 6, opts, logprobs=[True, False], top_logprobs=[3, 0])
    assert [r.tokens for r in on] == [r.tokens for r in off]
    assert off[0].logprobs is None and on[1].logprobs is None and on[1].top_logprobs is None
    r = on[0]
    ls = _ref_logprobs(eng, prompts[0] + r.tokens)
    assert len(r.logprobs) == 6 and all(len(t) == 3 for t in r.top_logprobs)
    for k, t in enumerate(r.tokens):
        row = ls[len(prompts[0]) - 1 + k]  # raw logits: the repeat penalty (1.3) is not in the logprob
        assert abs(r.logprobs[k] - row[t]) < 1e-6
        assert [i for i, _ in r.top_logprobs[k]] == np.lexsort((np.arange(row.size), -row))[:3].tolist()
    both = eng.generate(prompts, 3, opts, logprobs=True)
    assert all(len(x.logprobs) == 3 and x.top_logprobs == [[], [], []] for x in both)


def test_top_logprobs_order_with_forced_tie():
    lg = torch.full((64,), -1.0)
    lg[[40, 3, 17]] = 2.0   # three-way tie for first place: index ascending
    lg[[9, 50]] = 1.0       # tie straddling the 4th place
    ls, top = logprob_host(lg, 4)
    assert [i for i, _ in top] == [3, 17, 40, 9]
    assert top[0][1] == top[1][1] == top[2][1] > top[3][1]
    assert abs(sum(math.exp(v) for v in ls) - 1.0) < 1e-12
    assert logprob_host(lg, 0)[1] == []
    assert [i for i, _ in logprob_host(lg, 64)[1]][:6] == [3, 17, 40, 9, 50, 0]


def test_bad_arguments(eng):
    with pytest.raises(ValueError, match="exceeds the context"):
        eng.score([list(range(3, 3 + eng.T_max + 1))])
    assert len(eng.score([list(range(3, 3 + eng.T_max))])[0].logprobs) == eng.T_max - 1
    with pytest.raises(ValueError, match="top_logprobs"):
        eng.score([[1, 2, 3]], top_logprobs=21)
    with pytest.raises(ValueError, match="top_logprobs"):
        eng.generate([[1, 2]], 2, logprobs=True, top_logprobs=21)
    with pytest.raises(ValueError, match="needs logprobs"):
        eng.generate([[1, 2]], 2, top_logprobs=2)


def test_perplexity(eng, capsys, tmp_path):
    ids = np.random.default_rng(3).integers(3, 1000, size=45).tolist()
    assert [len(w) for w in windows(ids, 16)] == [16, 16, 13] and [len(w) for w in windows(ids[:33], 16)] == [16, 16]
    res = perplexity(eng, ids, ctx=16, batch=2)
    scored = [lp for r in eng.score(windows(ids, 16)) for lp in r.logprobs]
    assert res["windows"] == 3 and res["tokens_scored"] == 42 == len(scored)
    assert res["nll_mean"] == pytest.approx(-np.mean(scored), rel=1e-12)
    assert res["ppl"] == pytest.approx(math.exp(res["nll_mean"]), rel=1e-12)
    # the command: one JSON line with the documented keys
    from cain_amd.runner.cli import main

    text = tmp_path / "t.txt"
    text.write_text("the quick brown fox jumps over the lazy dog, again and again and again")
    assert main(["perplexity", "--model", MODEL, "--file", str(text), "--ctx", "8", "--batch", "2", "--device", "cpu",
                 "--max-context", "128"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert list(out) == ["model", "weights", "kv", "ctx", "windows", "tokens_scored", "nll_mean", "ppl", "tok_per_s"]
    assert out["model"] == MODEL and out["weights"] == "bf16" and out["kv"] == "bf16" and out["ctx"] == 8
    assert out["ppl"] == pytest.approx(math.exp(out["nll_mean"]), rel=1e-12)
