"""Prefix KV reuse, the parts that need no GPU: the torch mirror of the prefix copy against the definition, the slot
matching rule (``engine.plan_prefix_reuse``) and Ollama's ``context`` round trip through the torch backend and the
in-process server."""
import json
import urllib.error
import urllib.request

import pytest
import torch

from cain_amd import ops
from cain_amd.client import OllamaClient
from cain_amd.engine import DecodeEngine
from cain_amd.engine.engine import plan_prefix_reuse, taken_record
from cain_amd.serve import EngineBackend, ServerThread

N_LIST = (0, 1, 15, 16, 17, 31, 32, 33, 47, 64, 96)
T_MAX = 96


# ------------------------------------------------------------------------------------------ kv_copy_prefix_ref
@pytest.mark.parametrize("hd", (64, 128, 256))
@pytest.mark.parametrize("n", N_LIST)
def test_ref_copies_the_prefix_and_nothing_else(n, hd):
    """Caches packed from natural [T, hd] tensors of distinct integers: after the copy the destination's positions
    < n unpack to the source's, and every other element of both caches is what it was."""
    L, S, H = 2, 3, 2
    count = L * S * H * T_MAX * hd
    k_nat = torch.arange(count, dtype=torch.int32).view(L, S, H, T_MAX, hd)
    v_nat = k_nat + count
    kc, vc = ops.pack_kcache(k_nat).flatten(), ops.pack_vcache(v_nat).flatten()
    ops.kv_copy_prefix_ref(kc, vc, L, S, H, hd, T_MAX, [(0, 2, n)])
    k_got = ops.unpack_kcache(kc.view(L, S, H, T_MAX, hd))
    v_got = ops.unpack_vcache(vc.view(L, S, H, hd, T_MAX))
    k_want, v_want = k_nat.clone(), v_nat.clone()
    k_want[:, 2, :, :n] = k_nat[:, 0, :, :n]
    v_want[:, 2, :, :n] = v_nat[:, 0, :, :n]
    assert torch.equal(k_got, k_want) and torch.equal(v_got, v_want)
    # positions < n really moved (distinct values: equal to the source means taken from the source)
    if n:
        assert torch.equal(k_got[:, 2, :, :n], k_nat[:, 0, :, :n]) and not torch.equal(k_got[:, 2], k_nat[:, 2])


def test_ref_several_pairs_read_the_caches_as_they_were():
    L, S, H, hd = 1, 4, 1, 64
    count = L * S * H * T_MAX * hd
    k_nat = torch.arange(count, dtype=torch.int32).view(L, S, H, T_MAX, hd)
    kc, vc = ops.pack_kcache(k_nat).flatten(), ops.pack_vcache(k_nat + count).flatten()
    ops.kv_copy_prefix_ref(kc, vc, L, S, H, hd, T_MAX, [(0, 1, 33), (0, 3, 17)])
    k_got = ops.unpack_kcache(kc.view(L, S, H, T_MAX, hd))
    want = k_nat.clone()
    want[:, 1, :, :33] = k_nat[:, 0, :, :33]
    want[:, 3, :, :17] = k_nat[:, 0, :, :17]
    assert torch.equal(k_got, want)


# ------------------------------------------------------------------------------------------ plan_prefix_reuse
FREE = [3, 2, 1, 0]  # a fresh batch's free list: pop() hands out 0, 1, 2, 3


def test_plan_empty_records_keep_todays_slot_order():
    recs = [[] for _ in range(4)]
    plan = plan_prefix_reuse(recs, FREE, [], [[1, 2, 3], [4, 5], [6]], 4)
    assert plan == [(0, 0, None), (1, 0, None), (2, 0, None)]
    # whatever order retire() left the free list in
    assert plan_prefix_reuse(recs, [1, 3, 0], [2], [[1, 2, 3], [7, 8]], 4) == [(0, 0, None), (3, 0, None)]


def test_plan_in_place_beats_copy():
    """A free slot with the longest match is taken as it is; a live slot that matches no longer by copy_min is not a
    reason to copy."""
    a = list(range(100, 140))
    recs = [[], a[:30], [], a[:33]]
    plan = plan_prefix_reuse(recs, [2, 1, 0], [3], [a], 4)
    assert plan == [(1, 30, None)]  # 33 - 30 < 4
    # equal matches: the slot pop() reaches first
    recs = [a[:30], a[:30], [], []]
    assert plan_prefix_reuse(recs, [2, 1, 0], [], [a], 4) == [(0, 30, None)]
    # reuse in place from a single token on
    assert plan_prefix_reuse([[], a[:1], []], [2, 1, 0], [], [a], 4) == [(1, 1, None)]


def test_plan_copies_only_from_copy_min():
    a = list(range(100, 140))
    recs = [[], a[:10], [], a[:20]]
    assert plan_prefix_reuse(recs, [2, 1, 0], [3], [a], 11) == [(1, 10, None)]
    assert plan_prefix_reuse(recs, [2, 1, 0], [3], [a], 10) == [(0, 20, 3)]  # next free slot in pop() order
    # no free slot matches at all: the live donor's whole match is what a copy saves
    recs = [[], [], [], a[:20]]
    assert plan_prefix_reuse(recs, [2, 1, 0], [3], [a], 21) == [(0, 0, None)]
    assert plan_prefix_reuse(recs, [2, 1, 0], [3], [a], 20) == [(0, 20, 3)]


def test_plan_caps_at_prompt_length_minus_one():
    """The last prompt token is the first decode step's input: never reused, in place or by copy."""
    a = list(range(100, 140))
    assert plan_prefix_reuse([a + [7, 8], []], [1, 0], [], [a], 4) == [(0, len(a) - 1, None)]
    assert plan_prefix_reuse([a + [7, 8], []], [1], [0], [a], 4) == [(1, len(a) - 1, 0)]
    assert plan_prefix_reuse([a, []], [1, 0], [], [a + [9]], 4) == [(0, len(a), None)]  # record + 1 token: all of it
    assert plan_prefix_reuse([[5], []], [1, 0], [], [[5]], 4) == [(0, 0, None)]  # a one-token prompt reuses nothing


def test_plan_live_donor_gives_only_its_polled_tokens():
    """A live row's record is the lower bound known at the last poll: a prompt that agrees with the row further than
    that still gets only the recorded length."""
    a = list(range(100, 180))
    recs = [[], [], a[:40]]  # the row has decoded past 40 since, but nobody polled
    assert plan_prefix_reuse(recs, [1, 0], [2], [a], 8) == [(0, 40, 2)]


def test_plan_same_call_siblings_are_not_donors():
    """Two requests with one new prefix admitted together: neither holds it yet, both prefill it.  A free slot an
    earlier request of the call claimed in place still serves with what it held before the call."""
    a = list(range(100, 160))
    recs = [[] for _ in range(4)]
    assert plan_prefix_reuse(recs, FREE, [], [a, a], 4) == [(0, 0, None), (1, 0, None)]
    recs = [[], a[:50], [], []]
    plan = plan_prefix_reuse(recs, FREE, [], [a, a], 4)
    assert plan == [(1, 50, None), (0, 50, 1)]
    # the destination of a copy is never a source: a third sibling copies from the original holder
    plan = plan_prefix_reuse(recs, FREE, [], [a, a, a], 4)
    assert plan == [(1, 50, None), (0, 50, 1), (2, 50, 1)]
    assert len({s for s, _, _ in plan}) == 3


def test_plan_leaves_its_arguments_alone():
    recs, free, live = [[1, 2, 3], []], [1, 0], []
    plan_prefix_reuse(recs, free, live, [[1, 2, 3, 4]], 4)
    assert recs == [[1, 2, 3], []] and free == [1, 0] and live == []
    with pytest.raises(ValueError):
        plan_prefix_reuse(recs, [0], [], [[1], [2]], 4)


def test_taken_slot_stale_record_is_truncated():
    """Taking a slot with reuse n drops what it held past n before the prompt's tokens follow, so the next call
    cannot match the stale tail."""
    stale = [1, 2, 3, 4, 5, 6, 7, 8]
    prompt = [1, 2, 3, 9, 9, 9, 7]
    ((slot, n, donor),) = plan_prefix_reuse([stale, []], [1, 0], [], [prompt], 4)
    assert (slot, n, donor) == (0, 3, None)
    rec = taken_record(stale, n, prompt)
    assert rec == [1, 2, 3, 9, 9, 9]
    assert plan_prefix_reuse([rec, []], [1, 0], [], [stale], 4) == [(0, 3, None)]
    with pytest.raises(ValueError):
        taken_record(stale, 4, prompt)


# ------------------------------------------------------------------------------------------ context round trip
MODEL = "tiny-qwen2:1.5b"
GREEDY = {"temperature": 0, "repeat_penalty": 1.0, "num_predict": 6}


def _post(url, body):
    req = urllib.request.Request(url + "/api/generate", data=json.dumps(body).encode(),
                                 headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(req, timeout=120) as r:
        return json.loads(r.read())


def test_engine_generate_prepends_context():
    eng = DecodeEngine(MODEL, device="cpu", max_batch=2, max_context=64)
    opts = dict(temperature=0.0, repeat_penalty=1.0, eos_id=-1)
    ctx = [11, 12, 13, 14]
    tail = eng.encode("hello")
    (with_ctx,) = eng.generate(["hello"], 5, [opts], context=[ctx])
    (joined,) = eng.generate([ctx + tail], 5, [opts])
    assert with_ctx.prompt_tokens == ctx + tail and with_ctx.tokens == joined.tokens
    assert with_ctx.prompt_eval_count == len(ctx) + len(tail)
    assert with_ctx.ollama_json(context=True)["context"] == ctx + tail + with_ctx.tokens
    assert with_ctx.ollama_json()["context"] == [] and "prompt_cached_count" not in with_ctx.ollama_json()
    with pytest.raises(ValueError):
        eng.generate(["a", "b"], 5, [opts, opts], context=[ctx])


def test_server_context_round_trip():
    """The response's context is the prompt's ids plus the generated ids, and sending it back with a new prompt gives
    the tokens of one request whose prompt is the concatenated tokens."""
    be = EngineBackend([MODEL], device="cpu", max_batch=2, max_context=128, prefix_cache=True)
    with ServerThread(be) as s:
        c = OllamaClient(s.url)
        first = c.generate(MODEL, "tell me about India", options=GREEDY)
        eng = be.engine(MODEL)
        ctx = first.data["context"]
        p1 = eng.encode("tell me about India")
        assert ctx[: len(p1)] == p1 and len(ctx) == len(p1) + first.eval_count
        assert eng.tokenizer.decode(ctx[len(p1):]) == first.text
        second = c.generate(MODEL, "and its rivers", options=GREEDY, context=ctx)
        p2 = eng.encode("and its rivers")
        assert second.prompt_eval_count == len(ctx) + len(p2)
        assert second.data["context"][: len(ctx) + len(p2)] == ctx + p2
        (joined,) = eng.generate([ctx + p2], 6, [dict(temperature=0.0, repeat_penalty=1.0)])
        assert second.data["context"][len(ctx) + len(p2):] == joined.tokens
        ps = c.get("/api/ps")["models"]
        assert ps and all(m["prefix_cache"] is True for m in ps)


def test_server_context_only_when_asked():
    """Without the flag a response carries a context only when the request sent one; a bad id is refused."""
    be = EngineBackend([MODEL], device="cpu", max_batch=2, max_context=128)
    vocab = be.vocab_size(MODEL)
    with ServerThread(be) as s:
        plain = _post(s.url, {"model": MODEL, "prompt": "hello", "stream": False, "options": GREEDY})
        assert plain["context"] == [] and "prompt_cached_count" not in plain
        sent = _post(s.url, {"model": MODEL, "prompt": "hello", "stream": False, "options": GREEDY,
                             "context": [5, 6, 7]})
        assert sent["context"][:3] == [5, 6, 7] and len(sent["context"]) == sent["prompt_eval_count"] + 6
        chat = OllamaClient(s.url).chat(MODEL, [{"role": "user", "content": "hi"}], options=GREEDY)
        assert chat.data["context"] == []
        for bad in ([1, vocab], [vocab + 5], [-1], "abc", [1.5], [True]):
            with pytest.raises(urllib.error.HTTPError) as e:
                _post(s.url, {"model": MODEL, "prompt": "hello", "stream": False, "options": GREEDY, "context": bad})
            assert e.value.code == 400, bad
        ok = _post(s.url, {"model": MODEL, "prompt": "hello", "stream": False, "options": GREEDY,
                           "context": [vocab - 1]})
        assert ok["context"][0] == vocab - 1
