"""``DecodeEngine.embed`` on the HIP backend against the fp32 oracle's ``hidden``: tiny models of every family, every
weight format with a bf16 and an fp8 KV cache, prompt lengths around the prefill chunk (one and two prompts per call,
so a chunk holds a sequence boundary and a sequence spans chunks), both poolings.  Then the engine's state: a
generation after an embedding, and a live row of a continuous batch around one, keep their tokens -- and the live
slot's KV its bits; and two embeddings of the same batch are bitwise equal.

The accuracy bounds are twice the worst case measured on an MI355X per weight format over this file's own cases
(profiles/r19/embeddings/README.md has the table); the oracle's embedding of the same prompt with its last token
changed is the negative control and must miss them."""
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

sys.path.insert(0, str(Path(__file__).parent))

from engine_state import FAMILIES, GREEDY, LLAMA, prompt_ids, read_kv  # noqa: E402

from cain_amd.engine.engine import DecodeEngine  # noqa: E402
from cain_amd.models import get_config  # noqa: E402
from cain_amd.models.reference import ReferenceModel  # noqa: E402
from cain_amd.models.weights import random_weights, roundtrip_weights  # noqa: E402

CHUNK = 16   # CAIN_PREFILL_ROWS of every engine here
T_MAX = 128
LENGTHS = (1, 2, CHUNK - 1, CHUNK, CHUNK + 1)
FORMATS = ("bf16", "fp8", "fp4", "q4_k_m")
# (cosine distance, max |delta| of the unit vectors): twice the worst case of each weight format on an MI355X, both KV
# formats and both poolings taken together (profiles/r19/embeddings/README.md).  Measured worst cases: bf16 6.113e-05 / 3.790e-03, fp8 8.238e-05 / 3.180e-03, fp4 3.045e-05 / 2.057e-03,
# q4_k_m 2.093e-04 / 5.909e-03 (each format's worst is on the fp8 KV cache); the controls' nearest miss is 2.2e-02 /
# 4.0e-02
BOUNDS = {"bf16": (2 * 6.113e-05, 2 * 3.790e-03), "fp8": (2 * 8.238e-05, 2 * 3.180e-03),
          "fp4": (2 * 3.045e-05, 2 * 2.057e-03), "q4_k_m": (2 * 2.093e-04, 2 * 5.909e-03)}


def _fits(model: str, wd: str) -> bool:
    cfg = get_config(model)
    ks = (cfg.d_model, cfg.q_dim, cfg.ffn)
    return not ((wd == "fp4" and any(k % 128 for k in ks)) or (wd == "q4_k_m" and any(k % 256 for k in ks)))


CASES = [(m, wd, "bf16") for m in FAMILIES for wd in FORMATS if _fits(m, wd)] + \
        [(LLAMA, wd, "fp8") for wd in FORMATS]


@pytest.fixture(autouse=True)
def _sync():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:  # a GPU fault: nothing more may run on the device
        pytest.exit(f"GPU error, stopping the session: {exc}", returncode=3)


def make(model, wd="bf16", kv="bf16", seed=11, **kw):
    """(engine, oracle) on random weights whose final gain is not the neutral one."""
    cfg = get_config(model)
    w = random_weights(cfg, device="cuda", seed=seed)
    g = torch.Generator().manual_seed(seed)
    w.final_norm = (w.final_norm.float() + 0.5 * torch.randn(cfg.d_model, generator=g).cuda()).to(w.final_norm.dtype)
    old = os.environ.get("CAIN_PREFILL_ROWS")
    os.environ["CAIN_PREFILL_ROWS"] = str(CHUNK)
    try:
        eng = DecodeEngine(model, device="cuda", max_batch=4, max_context=T_MAX, seed=seed, weights=w,
                           keep_natural=True, weight_dtype=wd, kv_dtype=kv, steps_per_graph=4, **kw)
    finally:
        if old is None:
            del os.environ["CAIN_PREFILL_ROWS"]
        else:
            os.environ["CAIN_PREFILL_ROWS"] = old
    assert eng.prefill_chunk == CHUNK
    return eng, ReferenceModel(roundtrip_weights(w, wd), kv_dtype=kv)


def oracle(ref, ids, pooling):
    h = ref.hidden(torch.tensor([ids], device="cuda")).double()[0].cpu().numpy()
    v = h[-1] if pooling == "last" else h.sum(0) / len(ids)
    return v / np.sqrt((v * v).sum())


def distance(got, want):
    got = np.asarray(got, dtype=np.float64)
    return 1.0 - float(got @ want) / float(np.linalg.norm(got) * np.linalg.norm(want)), float(np.abs(got - want).max())


@pytest.mark.parametrize("model,wd,kv", CASES, ids=[f"{m}-{w}-kv{k}" for m, w, k in CASES])
def test_embed_against_the_oracle(model, wd, kv):
    eng, ref = make(model, wd, kv)
    vocab = eng.cfg.vocab
    prompts = [prompt_ids(n, vocab, 100 + n) for n in LENGTHS]
    # calls: each length alone; then pairs of different lengths (a boundary inside a chunk, a prompt across chunks)
    calls = [[p] for p in prompts] + [[prompts[4], prompts[1]], [prompts[2], prompts[3], prompts[0]]]
    cos_max, abs_max = BOUNDS[wd]
    worst = [0.0, 0.0]
    control = [np.inf, np.inf]
    for pooling in ("last", "mean"):
        for call in calls:
            res = eng.embed(call, pooling=pooling)
            for r, p in zip(res, call):
                assert r.prompt_eval_count == len(p) and len(r.embedding) == eng.cfg.d_model
                assert np.isfinite(r.embedding).all() and abs(np.linalg.norm(r.embedding) - 1.0) < 1e-5
                c, a = distance(r.embedding, oracle(ref, p, pooling))
                worst = [max(worst[0], c), max(worst[1], a)]
                other = p[:-1] + [3 + (p[-1] - 3 + vocab // 2) % (vocab - 3)]  # the last token changed
                if pooling == "last" or len(p) <= 2:
                    nc, na = distance(r.embedding, oracle(ref, other, pooling))
                    control = [min(control[0], nc), min(control[1], na)]
    print(f"EMBED_ACCURACY {model} {wd} kv={kv}: cos {worst[0]:.3e} maxabs {worst[1]:.3e}; "
          f"control cos {control[0]:.3e} maxabs {control[1]:.3e}")
    assert worst[0] <= cos_max and worst[1] <= abs_max, (worst, BOUNDS[wd])
    assert control[0] > cos_max and control[1] > abs_max, (control, BOUNDS[wd])


def test_two_embeds_of_one_batch_are_bitwise_equal():
    eng, _ = make(LLAMA)
    batch = [prompt_ids(n, eng.cfg.vocab, 7 + n) for n in (CHUNK + 1, 3, 1)]
    for pooling in ("last", "mean"):
        a, b = eng.embed(batch, pooling=pooling), eng.embed(batch, pooling=pooling)
        assert [r.embedding for r in a] == [r.embedding for r in b]
    # more prompts than slots: passes of max_batch, the same vectors
    many = [prompt_ids(2 + i, eng.cfg.vocab, 50 + i) for i in range(eng.max_batch + 2)]
    assert [r.embedding for r in eng.embed(many)] == [eng.embed([p])[0].embedding for p in many]


def test_generate_after_embed_is_a_fresh_engines():
    opts = dict(temperature=0.8, top_k=40, seed=7, eos_id=-1)
    fresh, _ = make(LLAMA)
    used, _ = make(LLAMA)
    prompts = [prompt_ids(n, fresh.cfg.vocab, 20 + n) for n in (5, CHUNK + 3)]
    used.embed([prompt_ids(n, fresh.cfg.vocab, 90 + n) for n in (CHUNK + 2, 4, 9)], pooling="mean")
    want = [r.tokens for r in fresh.generate(prompts, 16, opts)]
    assert [r.tokens for r in used.generate(prompts, 16, opts)] == want


@pytest.mark.parametrize("kw", [{}, {"speculative": 2}], ids=["plain", "speculative"])
def test_embed_beside_a_live_row_changes_nothing_of_it(kw):
    def run(embed_mid):
        eng, ref = make(LLAMA, **kw)
        cb = eng.continuous()
        cb.admit([prompt_ids(6, eng.cfg.vocab, 1)], [24], [GREEDY])
        cb.step(4)
        if embed_mid:
            slot, free = cb.row_slot[0], list(cb.free_slots)
            before = [b[:, slot].clone() for b in read_kv(eng)[2:]]
            texts = [prompt_ids(CHUNK + 1, eng.cfg.vocab, 2), prompt_ids(3, eng.cfg.vocab, 3)]
            res = cb.embed(texts, pooling="mean")
            after = [b[:, slot] for b in read_kv(eng)[2:]]
            assert all(torch.equal(x, y) for x, y in zip(before, after))  # the live slot's KV, bit for bit
            assert cb.free_slots == free and slot not in free and cb.n == 1
            if not kw:
                for r, p in zip(res, texts):
                    assert distance(r.embedding, oracle(ref, p, "mean"))[0] <= BOUNDS["bf16"][0]
        for _ in range(6):
            cb.step(4)
        cb.poll()
        return cb.tokens(0)

    assert run(True) == run(False)


def test_no_free_slot_and_bad_arguments():
    eng, _ = make(LLAMA)
    cb = eng.continuous()
    cb.admit([prompt_ids(3, eng.cfg.vocab, i) for i in range(eng.max_batch)], [4] * eng.max_batch,
             [GREEDY] * eng.max_batch)
    with pytest.raises(ValueError):
        cb.embed([[3, 4]])
    with pytest.raises(ValueError):
        eng.embed([[3, 4]], pooling="max")
    with pytest.raises(ValueError):
        eng.embed([prompt_ids(T_MAX + 1, eng.cfg.vocab, 5)], truncate=False)
    r = eng.embed([prompt_ids(T_MAX + 1, eng.cfg.vocab, 5)])[0]
    assert r.truncated and r.prompt_eval_count == T_MAX
