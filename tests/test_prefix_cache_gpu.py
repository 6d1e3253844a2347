"""Prefix KV reuse on the GPU: the prefix copy kernel held bitwise to its torch mirror over the whole of both caches,
and the continuous batch with ``prefix_cache=True`` checked where its state is recorded -- the KV cache per position
against the oracle (``tests/engine_state.py``), the sentinel everywhere nothing should have been written, the rows a
prefill was spared, and the tokens against an engine that computes every prompt from position 0."""
import json
import sys
import urllib.request
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

sys.path.insert(0, str(Path(__file__).parent))

import engine_state as es  # noqa: E402
from cain_amd import ops  # noqa: E402
from cain_amd.engine import DecodeEngine  # noqa: E402
from cain_amd.engine import engine as engine_mod  # noqa: E402
from cain_amd.models import random_weights  # noqa: E402
from cain_amd.serve import EngineBackend, ServerThread  # noqa: E402

# ------------------------------------------------------------------------------------------ the kernel alone
N_LIST = (0, 1, 15, 16, 17, 31, 32, 33, 47, 64, 96)
L, S, T_MAX = 2, 5, 96


def _pattern(kv8: bool, Hkv: int, hd: int, salt: int) -> torch.Tensor:
    """Natural [L, S, Hkv, T, hd] bits, one distinct vector per (layer, slot, head, position): 16-bit elements start
    at 7 x the vector's number (< 2^16), 8-bit ones spell the number in their first two elements; the other dims add
    a stride, so neighbouring elements differ too."""
    nvec = L * S * Hkv * T_MAX
    idx = (torch.arange(nvec, dtype=torch.int64) + salt).view(L, S, Hkv, T_MAX, 1)
    d = torch.arange(hd, dtype=torch.int64).view(1, 1, 1, 1, hd)
    if kv8:
        assert nvec + salt < 1 << 16
        return (((idx >> (8 * (d & 1))) & 0xFF) + 37 * (d >> 1)).remainder(256).to(torch.uint8)
    assert 7 * (nvec + salt) < 1 << 16
    return (7 * idx + 8191 * d).remainder(1 << 16).to(torch.int32).to(torch.int16)


def _caches(kv8: bool, Hkv: int, hd: int):
    k = ops.pack_kcache(_pattern(kv8, Hkv, hd, 0)).flatten()
    v = ops.pack_vcache(_pattern(kv8, Hkv, hd, 1000)).flatten()
    return k, v


def _check_copy(k0, v0, Hkv, hd, pairs, tag):
    kg, vg = k0.cuda(), v0.cuda()
    rc = ops.kv_copy_prefix(kg, vg, L, S, Hkv, hd, T_MAX, pairs)
    torch.cuda.synchronize()
    assert rc == 0, (tag, rc)
    kr, vr = k0.clone(), v0.clone()
    ops.kv_copy_prefix_ref(kr, vr, L, S, Hkv, hd, T_MAX, pairs)
    assert torch.equal(kg.cpu(), kr), f"{tag}: K cache differs from the mirror"
    assert torch.equal(vg.cpu(), vr), f"{tag}: V^T cache differs from the mirror"
    if any(n for _, _, n in pairs):
        assert not torch.equal(kr, k0) and not torch.equal(vr, v0)  # the mirror did copy something


@pytest.mark.parametrize("Hkv", (1, 2, 8))
@pytest.mark.parametrize("hd", (64, 128, 256))
@pytest.mark.parametrize("kv", ("bf16", "fp8"))
def test_copy_kernel_equals_the_mirror_bitwise(kv, hd, Hkv):
    """One pair at every n of the list (n = T_max among them), then three pairs in one call with one source feeding
    two destinations: the whole of both caches equals the mirror's, copied and untouched bytes alike."""
    k0, v0 = _caches(kv == "fp8", Hkv, hd)
    for n in N_LIST:
        _check_copy(k0, v0, Hkv, hd, [(1, 3, n)], f"{kv} hd{hd} Hkv{Hkv} n={n}")
    _check_copy(k0, v0, Hkv, hd, [(0, 2, 33), (0, 4, 47), (1, 3, 17)], f"{kv} hd{hd} Hkv{Hkv} three pairs")
    _check_copy(k0, v0, Hkv, hd, [(4, 0, T_MAX), (4, 1, 0), (2, 3, 64)], f"{kv} hd{hd} Hkv{Hkv} full, empty, 64")


@pytest.mark.parametrize("kv", ("bf16", "fp8"))
def test_copy_kernel_refusals_leave_the_caches_alone(kv):
    """Argument checks that return -1 before any launch; nothing to copy returns 0; the caches keep their bits."""
    Hkv, hd = 2, 64
    k0, v0 = _caches(kv == "fp8", Hkv, hd)
    kg, vg = k0.cuda(), v0.cuda()

    def call(pairs, S_=S, hd_=hd, T_=T_MAX):
        # (the buffers' real size is passed along, so a wrong hd or T_max cannot name memory outside them)
        return ops.kv_copy_prefix(kg, vg, L, S_, Hkv, hd_, T_, pairs, kv_layer_elems=S * Hkv * T_MAX * hd)

    refused = {
        "257 pairs": lambda: call([(0, 1, 0)] * 257),
        "source slot S": lambda: call([(S, 1, 8)]),
        "destination slot S": lambda: call([(0, S, 8)]),
        "negative slot": lambda: call([(-1, 1, 8)]),
        "n < 0": lambda: call([(0, 1, -1)]),
        "n > T_max": lambda: call([(0, 1, T_MAX + 1)]),
        "src == dst": lambda: call([(2, 2, 8)]),
        "a destination twice": lambda: call([(0, 1, 8), (2, 1, 8)]),
        "destination of one, source of another": lambda: call([(0, 1, 8), (1, 2, 8)]),
        "hd % 32": lambda: call([(0, 1, 8)], hd_=48),
        "T_max % 32": lambda: call([(0, 1, 8)], T_=80),
    }
    for what, fn in refused.items():
        assert fn() == -1, what
    lib = ops.load()
    arr = (ops.ci * 1)(0)
    assert lib.cain_kv_copy_prefix(ops._p(kg), ops._p(vg), S * Hkv * T_MAX * hd, L, S, Hkv, hd, T_MAX,
                                   int(kv == "fp8"), arr, arr, arr, -1, None) == -1, "pairs < 0"
    assert call([]) == 0 and call([(0, 1, 0), (2, 3, 0)]) == 0 and call([(2, 2, 0)]) == 0
    torch.cuda.synchronize()
    assert torch.equal(kg.cpu(), k0) and torch.equal(vg.cpu(), v0)


# ------------------------------------------------------------------------------------------ the engine
CASES = {
    "bf16": es.Case("prefix-bf16", es.LLAMA, (30,), (12,)),
    "fp8": es.Case("prefix-kvfp8", es.LLAMA, (30,), (12,), kv_dtype="fp8"),
    "q4_k": es.Case("prefix-q4_k", es.LLAMA, (30,), (12,), weight_dtype="q4_k"),
}
_models: dict = {}


def _shared(case):
    """(weights, (oracle, baseline, None)) of a case, built once per weight / cache format."""
    key = (case.weight_dtype, case.kv_dtype)
    if key not in _models:
        w = random_weights(case.config(), device="cuda", seed=case.seed)
        _models[key] = (w, es.models_for(w, case))
    return _models[key]


def _engine(case, prefix_cache, steps_per_graph=4):
    eng = DecodeEngine(case.config(), device="cuda", max_batch=4, max_context=es.T_MAX, keep_natural=True,
                       seed=case.seed, weights=_shared(case)[0], weight_dtype=case.weight_dtype,
                       kv_dtype=case.kv_dtype, steps_per_graph=steps_per_graph, prefix_cache=prefix_cache)
    assert eng.T_max == es.T_MAX
    es.poison(eng)
    return eng


def _verify(eng, case, rows, tag):
    """Every written vector within the oracle limits of engine_state.py, everything else the sentinel."""
    K, V, kb, vb = es.read_kv(eng)
    want, lim, base = es.expectations(_shared(case)[1], rows, eng.max_batch, None, case.compare_layers)
    got = es.layer_max((K, V), want)
    print(f"PREFIX_STATE {tag}: K engine {got[0]} baseline {base[0]} limit {lim[0]}; "
          f"V engine {got[1]} baseline {base[1]} limit {lim[1]}")
    es.compare((K, V), want, lim, tag)
    es.assert_untouched((kb, vb), want.written, case.kv_dtype, tag=tag)


def _run(cb, steps):
    """``steps`` decode steps, one poll: the tokens per live row."""
    cb.step(steps)
    new, fin = cb.poll()
    return new, fin


def _same_or_tie(case, prompt, got, want, tag):
    """Greedy tokens equal, or the first difference is a near-tie of the oracle's teacher-forced logits (the rule
    of the engine tests: the margin below 0.05 of the logits' standard deviation); nothing after it is compared."""
    assert len(got) == len(want), tag
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            ref = _shared(case)[1][0]
            lg = ref.forward(torch.tensor([list(prompt) + list(want[:i])], device="cuda"))[0, -1]
            assert abs(float(lg[a] - lg[b])) < 0.05 * float(lg.std()), (tag, i, a, b)
            return


def _fresh_tokens(case, prompt, n):
    eng = _engine(case, prefix_cache=False)
    cb = eng.continuous()
    cb.admit([prompt], [n], [es.GREEDY])
    (toks,), _ = _run(cb, n)
    eng.close()
    return toks


@pytest.mark.parametrize("fmt", list(CASES))
def test_in_place_reuse_after_retire(fmt):
    """A (30 ids, 12 tokens) runs to its end and retires; B is A's prompt, A's tokens and 7 new ids.  B takes A's slot
    and prefills 7 rows: the 41 positions A wrote stay, B's cache is the oracle's within the limits, the rest is the
    sentinel, and B's tokens are those of an engine that computes all of B."""
    case = CASES[fmt]
    vocab = case.config().vocab
    A = case.prompts()[0]
    eng = _engine(case, prefix_cache=True)
    cb = eng.continuous()
    (ra,) = cb.admit([A], [12], [es.GREEDY])
    slot_a = cb.row_slot[ra]
    assert cb.reused == [0] and eng.prefill_rows_total == len(A) - 1
    (tok_a,), fin = _run(cb, 12)
    assert fin == [True] and len(tok_a) == 12
    assert eng.slot_tokens[slot_a] == A + tok_a[:-1]
    cb.retire([ra])
    B = A + tok_a + es.prompt_ids(7, vocab, 99)
    n = len(A) + len(tok_a) - 1
    before = eng.prefill_rows_total
    (rb,) = cb.admit([B], [9], [es.GREEDY])
    assert cb.reused == [n] and cb.row_slot[rb] == slot_a
    assert eng.prefill_rows_total - before == len(B) - 1 - n == 7
    assert eng.slot_tokens[slot_a] == B[:-1]
    (tok_b,), fin = _run(cb, 9)
    assert fin == [True] and len(tok_b) == 9
    assert eng.slot_tokens[slot_a] == B + tok_b[:-1]
    _verify(eng, case, {slot_a: es.expected_inputs(B, tok_b, idled=False)}, f"{case.id}-in-place")
    eng.close()
    _same_or_tie(case, B, tok_b, _fresh_tokens(case, B, 9), case.id)


@pytest.mark.parametrize("k", (33, 64))
def test_reuse_by_copy_from_a_live_row(k, monkeypatch):
    """A (70 ids) is decoding; B and C arrive with A's first k ids and their own tails, copy_min forced to 32: one
    copy launch gives both the k positions.  The admit leaves A's slot bit for bit, B's and C's positions < k are
    A's bits, and all three decode on to the oracle's cache."""
    monkeypatch.setattr(engine_mod, "PREFIX_COPY_MIN", 32)
    case = CASES["bf16"]
    vocab = case.config().vocab
    A = es.prompt_ids(70, vocab, 5)
    B = A[:k] + es.prompt_ids(5, vocab, 6)
    C = A[:k] + es.prompt_ids(6, vocab, 7)
    eng = _engine(case, prefix_cache=True)
    cb = eng.continuous()
    cb.admit([A], [16], [es.GREEDY])
    out = {0: [], 1: [], 2: []}
    new, _ = _run(cb, 4)
    out[0] += new[0]
    assert eng.slot_tokens[cb.row_slot[0]] == A + out[0][:-1]
    _, _, kb0, vb0 = es.read_kv(eng)
    before = eng.prefill_rows_total
    assert cb.admit([B, C], [12, 12], [es.GREEDY] * 2) == [1, 2]
    sa, sb, sc = cb.row_slot
    assert cb.reused == [0, k, k] and len({sa, sb, sc}) == 3
    assert eng.prefill_rows_total - before == (len(B) - 1 - k) + (len(C) - 1 - k)
    _, _, kb1, vb1 = es.read_kv(eng)
    assert torch.equal(kb1[:, sa], kb0[:, sa]) and torch.equal(vb1[:, sa], vb0[:, sa]), "the admit changed A's slot"
    for s in (sb, sc):
        assert torch.equal(kb1[:, s, :, :k], kb1[:, sa, :, :k]) and torch.equal(vb1[:, s, :, :k], vb1[:, sa, :, :k])
    new, fin = _run(cb, 12)  # A's last 12 tokens, all of B's and C's: nobody idles
    for r in range(3):
        out[r] += new[r]
    assert fin == [True] * 3 and [len(out[r]) for r in range(3)] == [16, 12, 12]
    rows = {s: es.expected_inputs(p, out[r], idled=False) for r, (s, p) in enumerate(((sa, A), (sb, B), (sc, C)))}
    _verify(eng, case, rows, f"{case.id}-copy-{k}")
    eng.close()
    _same_or_tie(case, B, out[1], _fresh_tokens(case, B, 12), f"copy-{k}-B")


def test_off_by_default(monkeypatch):
    monkeypatch.delenv("CAIN_PREFIX_CACHE", raising=False)
    case = CASES["bf16"]
    eng = DecodeEngine(case.config(), device="cuda", max_batch=4, max_context=es.T_MAX, seed=case.seed,
                       weights=_shared(case)[0], steps_per_graph=4, keep_natural=True)
    assert eng.prefix_cache is False
    A = case.prompts()[0]
    cb = eng.continuous()
    cb.admit([A], [8], [es.GREEDY])
    (tok_a,), _ = _run(cb, 8)
    cb.retire([0])
    B, C = A + tok_a + [5, 6], A[:20]
    cb.admit([B, C], [4, 4], [es.GREEDY] * 2)
    assert cb.reused == [0, 0]
    assert eng.prefill_rows_total == (len(A) - 1) + (len(B) - 1) + (len(C) - 1)
    _run(cb, 4)
    assert eng.slot_tokens == [[] for _ in range(4)]
    eng.close()


def test_last_token_rule():
    """A prompt that is a slot's whole record plus one token reuses all of the record -- len - 1 positions, no
    prefill row at all -- and its first decode step writes the one position the record does not cover."""
    case = CASES["bf16"]
    A = es.prompt_ids(20, case.config().vocab, 11)
    eng = _engine(case, prefix_cache=True)
    cb = eng.continuous()
    cb.admit([A], [1], [es.GREEDY])
    (tok_a,), fin = _run(cb, 1)
    assert fin == [True] and eng.slot_tokens[cb.row_slot[0]] == A  # positions 0 .. 19: the whole prompt, no more
    slot = cb.row_slot[0]
    cb.retire([0])
    B = A + [7]
    before = eng.prefill_rows_total
    cb.admit([B], [5], [es.GREEDY])
    assert cb.reused == [len(B) - 1] and cb.row_slot == [slot] and eng.prefill_rows_total == before
    (tok_b,), _ = _run(cb, 5)
    _verify(eng, case, {slot: es.expected_inputs(B, tok_b, idled=False)}, "last-token")
    cb.retire([0])
    # a prompt shorter than the record: capped at its own length - 1
    cb.admit([B[:10]], [1], [es.GREEDY])
    assert cb.reused == [9]
    eng.close()
    _same_or_tie(case, B, tok_b, _fresh_tokens(case, B, 5), "last-token")


def test_idled_row_loses_its_last_position():
    """A row that finished mid-chunk went on stepping and rewrote its last position with its last token's K / V: the
    record drops that position, so the next request computes it again and its cache is the oracle's."""
    case = CASES["bf16"]
    A = case.prompts()[0]
    eng = _engine(case, prefix_cache=True)
    cb = eng.continuous()
    cb.admit([A], [6], [es.GREEDY])
    (tok_a,), fin = _run(cb, 8)  # two chunks of 4: done after 6, two idle steps
    assert fin == [True] and len(tok_a) == 6
    slot = cb.row_slot[0]
    assert eng.slot_tokens[slot] == (A + tok_a)[: len(A) + 6 - 2]
    cb.retire([0])
    B = A + tok_a + [9, 10]
    cb.admit([B], [4], [es.GREEDY])
    assert cb.reused == [len(A) + 6 - 2]
    (tok_b,), _ = _run(cb, 4)
    _verify(eng, case, {slot: es.expected_inputs(B, tok_b, idled=False)}, "idled")
    eng.close()


def test_static_generate_clears_the_records():
    case = CASES["bf16"]
    A = case.prompts()[0]
    eng = _engine(case, prefix_cache=True)
    cb = eng.continuous()
    cb.admit([A], [4], [es.GREEDY])
    _run(cb, 4)
    slot = cb.row_slot[0]
    cb.retire([0])
    assert eng.slot_tokens[slot]
    eng.generate([A[:5]] * 4, 2, [es.GREEDY] * 4)
    assert eng.slot_tokens == [[] for _ in range(4)]
    cb.admit([A], [2], [es.GREEDY])
    assert cb.reused == [0]
    eng.close()


# ------------------------------------------------------------------------------------------ the server
def _chat(url, messages):
    body = {"model": es.LLAMA, "messages": messages, "stream": False,
            "options": {"temperature": 0, "repeat_penalty": 1.0, "num_predict": 8}}
    req = urllib.request.Request(url + "/api/chat", data=json.dumps(body).encode(),
                                 headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(req, timeout=300) as r:
        return json.loads(r.read())


def _two_turns(prefix_cache):
    be = EngineBackend([es.LLAMA], device="cuda:0", max_batch=4, max_context=512, preload=True, steps_per_graph=8,
                       prefix_cache=prefix_cache)
    with ServerThread(be, port=0) as srv:
        msgs = [{"role": "user", "content": "In 20 words, please give me information about the rivers of India"}]
        first = _chat(srv.url, msgs)
        msgs += [{"role": "assistant", "content": first["message"]["content"]},
                 {"role": "user", "content": "and which of them is the longest?"}]
        second = _chat(srv.url, msgs)
    return first, second


def test_server_second_chat_turn_hits_the_cache():
    first, second = _two_turns(True)
    plain1, plain2 = _two_turns(False)
    assert "prompt_cached_count" not in first and "prompt_cached_count" not in plain2
    assert 0 < second["prompt_cached_count"] < second["prompt_eval_count"]
    assert second["prompt_eval_count"] == plain2["prompt_eval_count"]  # the full prompt length, cached or not
    assert first["message"]["content"] == plain1["message"]["content"]
    assert second["message"]["content"] == plain2["message"]["content"]
