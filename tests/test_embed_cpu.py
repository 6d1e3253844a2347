"""``DecodeEngine.embed`` on the torch backend against the fp32 oracle's ``hidden`` pooled in float64: both poolings,
with and without normalisation, the model's own final gain (Gemma's 1 + w, and the true gain beside a gain-folded
model -- a unit gain is the negative control and must miss by far), truncation both ways, the empty prompt, more
prompts than ``max_batch`` and a bad pooling value."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).parent))

from engine_state import FAMILIES, prompt_ids  # noqa: E402

from cain_amd.engine.engine import DecodeEngine, EmbedResult  # noqa: E402
from cain_amd.models import get_config  # noqa: E402
from cain_amd.models.reference import ReferenceModel  # noqa: E402
from cain_amd.models.weights import effective_gain, final_gain, random_weights, roundtrip_weights  # noqa: E402

GEMMA = "tiny-gemma:7b"
T_MAX = 64
TOL = 2e-5  # fp32 pooling and normalisation of O(1) values against float64: a few 1e-7 per element


def weights_with_gains(model: str, seed: int = 5):
    """Random weights whose final norm's stored gain is not the neutral one (random init stores 1, Gemma 0)."""
    cfg = get_config(model)
    w = random_weights(cfg, device="cpu", seed=seed)
    g = torch.Generator().manual_seed(seed)
    w.final_norm = (w.final_norm.float() + 0.5 * torch.randn(cfg.d_model, generator=g)).to(w.final_norm.dtype)
    return w


@pytest.fixture(scope="module", params=FAMILIES)
def family(request):
    w = weights_with_gains(request.param)
    eng = DecodeEngine(request.param, device="cpu", max_batch=2, max_context=T_MAX, weights=w)
    return eng, ReferenceModel(w)


def pooled(ref, ids, pooling, normalize=True, gain=None):
    """float64 pooling of the oracle's hidden states; ``gain``: norm the residual stream with this gain instead."""
    h = ref.hidden(torch.tensor([ids])).double()[0].numpy()
    if gain is not None:
        h = h / final_gain(ref.mw).double().numpy() * gain.double().numpy()
    v = h[-1] if pooling == "last" else h.sum(0) / len(ids)
    return v / np.sqrt((v * v).sum()) if normalize else v


@pytest.mark.parametrize("pooling", ["last", "mean"])
def test_embed_is_the_oracles_hidden_pooled(family, pooling):
    eng, ref = family
    prompts = [prompt_ids(n, eng.cfg.vocab, 3 + n) for n in (1, 2, 19)]
    res = eng.embed(prompts, pooling=pooling)
    assert [type(r) for r in res] == [EmbedResult] * 3
    for r, p in zip(res, prompts):
        assert r.prompt_eval_count == len(p) and not r.truncated and len(r.embedding) == eng.cfg.d_model
        assert np.abs(np.array(r.embedding) - pooled(ref, p, pooling)).max() < TOL
        assert abs(np.linalg.norm(r.embedding) - 1.0) < 1e-5
    raw = eng.embed(prompts, pooling=pooling, normalize=False)
    for r, p in zip(raw, prompts):
        want = pooled(ref, p, pooling, normalize=False)
        assert np.abs(np.array(r.embedding) - want).max() < TOL * max(1.0, np.abs(want).max())
        assert abs(np.linalg.norm(r.embedding) - 1.0) > 0.1  # not a unit vector: nothing normalised it


def test_gemma_gain_is_one_plus_w_not_the_unit_gain():
    w = weights_with_gains(GEMMA)
    eng = DecodeEngine(GEMMA, device="cpu", max_batch=2, max_context=T_MAX, weights=w)
    ref = ReferenceModel(w)
    p = prompt_ids(9, eng.cfg.vocab, 1)
    got = np.array(eng.embed([p])[0].embedding)
    assert torch.equal(final_gain(w), effective_gain(w.cfg, w.final_norm))
    assert torch.equal(final_gain(w), (w.final_norm.float() + 1.0).to(w.final_norm.dtype))  # 1 + w, in bf16
    assert np.abs(got - pooled(ref, p, "last")).max() < TOL
    unit = pooled(ref, p, "last", gain=torch.ones(eng.cfg.d_model))
    stored = pooled(ref, p, "last", gain=w.final_norm)  # w without the 1
    assert np.abs(got - unit).max() > 1000 * TOL and np.abs(got - stored).max() > 1000 * TOL


@pytest.mark.parametrize("weight_dtype", ["fp8", "q4_k_m"])
def test_folded_model_keeps_the_true_gain(weight_dtype):
    """The torch backend of a quantised engine runs a gain-folded copy (unit ``final_norm``): the true gain travels
    beside it, and the embedding is normed with it."""
    w = weights_with_gains("tiny-llama3.1:8b")
    true_gain = final_gain(w).clone()
    eng = DecodeEngine("tiny-llama3.1:8b", device="cpu", max_batch=2, max_context=T_MAX, weights=w,
                       weight_dtype=weight_dtype)
    folded = roundtrip_weights(w, weight_dtype)
    assert torch.equal(final_gain(folded), true_gain)
    assert torch.equal(effective_gain(folded.cfg, folded.final_norm), torch.ones_like(true_gain))
    ref = ReferenceModel(folded)
    p = prompt_ids(11, eng.cfg.vocab, 2)
    got = np.array(eng.embed([p], pooling="mean")[0].embedding)
    assert np.abs(got - pooled(ref, p, "mean")).max() < TOL
    assert np.abs(got - pooled(ref, p, "mean", gain=torch.ones(eng.cfg.d_model))).max() > 1000 * TOL
    # forward keeps its behaviour: the logits of the folded copy are those of its unit final_norm and folded head
    lg = ref.forward(torch.tensor([p]))
    x = ref.hidden(torch.tensor([p])) / true_gain.float()
    assert torch.allclose(lg, x @ folded.lm_head.float().t(), atol=1e-4)


def test_truncate_both_ways(family):
    eng, ref = family
    long = prompt_ids(T_MAX + 7, eng.cfg.vocab, 8)
    r = eng.embed([long, long[:5]], truncate=True)
    assert (r[0].truncated, r[0].prompt_eval_count) == (True, T_MAX)
    assert (r[1].truncated, r[1].prompt_eval_count) == (False, 5)
    assert np.abs(np.array(r[0].embedding) - pooled(ref, long[:T_MAX], "last")).max() < TOL
    with pytest.raises(ValueError):
        eng.embed([long], truncate=False)
    assert not eng.embed([long[:T_MAX]], truncate=False)[0].truncated


def test_empty_prompt_embeds_bos(family):
    eng, ref = family
    r = eng.embed([[], ""])
    for x in r:
        assert x.prompt_eval_count == 1
        assert np.abs(np.array(x.embedding) - pooled(ref, [eng.cfg.bos_id], "last")).max() < TOL


def test_more_prompts_than_max_batch(family):
    eng, ref = family
    prompts = [prompt_ids(3 + i, eng.cfg.vocab, 40 + i) for i in range(2 * eng.max_batch + 1)]
    res = eng.embed(prompts, pooling="mean")
    assert len(res) == len(prompts)
    for r, p in zip(res, prompts):
        assert np.abs(np.array(r.embedding) - pooled(ref, p, "mean")).max() < TOL
    assert eng.embed([]) == []


def test_text_prompts_encode_as_generate(family):
    eng, ref = family
    ids = eng.encode("the quick brown fox")
    r = eng.embed(["the quick brown fox"])[0]
    assert r.prompt_eval_count == len(ids)
    assert np.abs(np.array(r.embedding) - pooled(ref, ids, "last")).max() < TOL


def test_bad_pooling_value(family):
    eng, _ = family
    with pytest.raises(ValueError):
        eng.embed([[3, 4]], pooling="max")
