"""The decoder's state, checked where it is recorded: after every scenario the KV cache the engine built is compared
per (layer, slot, kv head, position) with the fp32 oracle's K / V of the engine's own tokens (teacher forced, idle
rows included), within 3 x the bf16-eager baseline's largest per-vector error of that layer (never above 0.25), and
every element no row should have written is bit-identical to the sentinel the caches were poisoned with
(``tests/engine_state.py``).  Exact by construction, so asserted bitwise: graph replay equals eager launches, values
past a row's length cannot influence a result, and neither can the slot number."""
import functools
import sys
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
from cain_amd.models import random_weights  # noqa: E402


@functools.lru_cache(maxsize=None)
def _shared(case):
    """(weights, (oracle, baseline, a8 baseline)) of a case, built once."""
    w = random_weights(case.config(), device="cuda", seed=case.seed)
    return w, es.models_for(w, case)


def _engine(case, **kw):
    eng = DecodeEngine(case.config(), device="cuda", max_batch=case.max_batch, max_context=es.T_MAX, keep_natural=True,
                       seed=case.seed, weights=_shared(case)[0], weight_dtype=case.weight_dtype,
                       kv_dtype=case.kv_dtype, **kw)
    assert eng.T_max == es.T_MAX
    es.poison(eng)
    return eng


def _fmt(xs):
    return "[" + ", ".join(f"{x:.4f}" for x in xs) + "]"


def _verify(eng, case, rows, tag, n_prefill=None, snapshot=None, snapshot_slots=()):
    """Every written vector of every compared layer within its limit, everything else untouched.  ``rows``: {slot:
    the tokens at its positions 0 .. p_last}.  Prints the engine's and the baseline's maxima per layer."""
    K, V, kb, vb = es.read_kv(eng)
    want, lim, base = es.expectations(_shared(case)[1], rows, eng.max_batch, n_prefill, case.compare_layers)
    got = es.layer_max((K, V), want)
    print(f"ENGINE_STATE {tag}: K engine {_fmt(got[0])} baseline {_fmt(base[0])} limit {_fmt(lim[0])}; "
          f"V engine {_fmt(got[1])} baseline {_fmt(base[1])} limit {_fmt(lim[1])}")
    es.compare((K, V), want, lim, tag)
    es.assert_untouched((kb, vb), want.written, case.kv_dtype, snapshot, snapshot_slots, tag)
    return kb, vb


def _generate(eng, case, use_graph=True):
    res = eng.generate(case.prompts(), list(case.predict), [es.GREEDY] * len(case.lengths), use_graph=use_graph)
    toks = [r.tokens for r in res]
    assert tuple(len(t) for t in toks) == case.tokens_predicted()
    steps = max(case.tokens_predicted())
    # a row with fewer tokens than the batch's longest idles while the others step
    rows = {i: es.expected_inputs(p, t, idled=len(t) < steps) for i, (p, t) in enumerate(zip(case.prompts(), toks))}
    return res, toks, rows


def _record_steps(eng):
    """The logits of every decode forward, cloned on the engine's stream right after it."""
    log = []
    forward = eng._forward

    def recording(M, rows, want_logits, want_sample):
        forward(M, rows, want_logits, want_sample)
        if want_sample:
            log.append(eng.buf["logits"][:M].clone())

    eng._forward = recording
    return log


# ------------------------------------------------------------------------------------------ a. static generate
@pytest.mark.parametrize("name", es.FAMILIES)
def test_static_generate_every_family(name):
    """Prompts of 1, 2 and 33 ids (the first has no prefill row), 20 / 3 / 11 tokens: two rows idle; one single step,
    two graphs of 8 and three singles.  The same requests on eager launches give the same bits everywhere."""
    case = es.STATIC[name]
    eng = _engine(case, steps_per_graph=8)
    _, toks, rows = _generate(eng, case)
    logits = eng.buf["logits"][:3].clone()
    kb, vb = _verify(eng, case, rows, case.id)
    eager = _engine(case, steps_per_graph=8)
    _, toks2, _ = _generate(eager, case, use_graph=False)
    _, _, kb2, vb2 = es.read_kv(eager)
    assert toks2 == toks
    assert torch.equal(eager.buf["logits"][:3], logits)
    assert torch.equal(kb2, kb) and torch.equal(vb2, vb)
    eng.close()
    eager.close()


# ------------------------------------------------------------------------------------------ b. prefill chunking
@pytest.mark.parametrize("chunk", es.CHUNK_ROWS)
def test_prefill_chunking(chunk, monkeypatch):
    """116 prefill rows of four prompts (70, 9, 1, 40 ids) in chunks of 5 / 16 / 17 / 64 / 128 rows: chunks straddle
    prompts, one holds rows of three slots, and every final chunk is shorter than the one before it, so the row
    buffers still hold the previous chunk's slots and positions past row n."""
    case = es.CHUNKED
    if chunk is None:
        monkeypatch.delenv("CAIN_PREFILL_ROWS", raising=False)
    else:
        monkeypatch.setenv("CAIN_PREFILL_ROWS", str(chunk))
    eng = _engine(case)
    assert eng.prefill_chunk == (chunk or 128)
    prompts = case.prompts()
    got = eng.last_logits(prompts)
    ref = _shared(case)[1][0]
    for i, p in enumerate(prompts):
        want = ref.forward(torch.tensor([p], device="cuda"))[0, -1]
        assert torch.nn.functional.cosine_similarity(got[i], want, dim=0) > 0.995, (chunk, i)
    _verify(eng, case, dict(enumerate(prompts)), f"{case.id}-{chunk or 'unset'}")
    eng.close()


# ------------------------------------------------------------------------------------------ c. formats
@pytest.mark.parametrize("w,kv", list(es.FORMATS))
def test_weight_and_cache_formats(w, kv):
    case = es.FORMATS[w, kv]
    eng = _engine(case, steps_per_graph=8)
    if w == "q4_k_m":
        # the two-layer config has the split V launch in layer 1 (Q6_K V rows beside Q4_K q / k)
        assert ["wv" in lp for lp in eng._packed["layers"]] == [False, True]
    _, _, rows = _generate(eng, case)
    _verify(eng, case, rows, case.id)
    eng.close()


@pytest.mark.parametrize("w", list(es.A8))
def test_a8_prefill_a16_decode(w):
    """d_model 512: the 55-row prefill chunk runs the W8A8 / W4A8 kernel, the 3-row decode the few-row A16 kernels;
    the baseline quantises activations for the prefill positions only.  Layer 0 is compared (the baseline's own
    layer-1 error times 3 is over the cap); the sentinel check covers both layers."""
    case = es.A8[w]
    eng = _engine(case, steps_per_graph=8)
    assert eng.w8a8 if w == "fp8" else eng.w4a8
    assert eng.prefill_chunk > 16 and sum(case.lengths) - len(case.lengths) > 16
    _, _, rows = _generate(eng, case)
    _verify(eng, case, rows, case.id, n_prefill={i: L - 1 for i, L in enumerate(case.lengths)})
    eng.close()


def test_q4k_tile_kernels_at_40_rows():
    """40 prompts of 2 ids: a 40-row prefill chunk and a 40-row decode, both on the tile kernels of gemm_qtile.hip."""
    case = es.QTILE
    cfg = case.config()
    lib = ops.load()
    act = ops.EPI_GELU if cfg.act == "gelu_tanh" else ops.EPI_SILU
    for K, epi in ((cfg.d_model, ops.EPI_QKV_ROPE), (cfg.q_dim, ops.EPI_RESID), (cfg.d_model, act),
                   (cfg.ffn, ops.EPI_RESID), (cfg.d_model, ops.EPI_F32)):
        # one pass over the weights where the stream kernels would need several: the tile path
        assert ops.gemm_q_passes(1, K, 40, epi) == 1 and 0 < int(lib.cain_gemm_q4_rows(K, epi)) < 40, (K, epi)
    eng = _engine(case, steps_per_graph=8)
    assert eng.max_batch == 40 and eng.prefill_chunk >= 40
    _, _, rows = _generate(eng, case)
    _verify(eng, case, rows, case.id)
    eng.close()


# ------------------------------------------------------------------------------------------ d. context full
def test_context_full_rows_stop_and_idle():
    """Rows of 253 and 255 ids in a context of 256 clamp to 3 and 1 tokens and idle while a 4-id row generates 20:
    position 255 is never written, and the neighbours' vectors are intact."""
    case = es.FULL
    eng = _engine(case, steps_per_graph=8)
    res, toks, rows = _generate(eng, case)
    assert [len(t) for t in toks] == [3, 1, 20] and all(r.done_reason == "length" for r in res)
    kb, vb = _verify(eng, case, rows, case.id)
    s = es.sentinel_bits(case.kv_dtype).cuda()
    assert bool((kb[:, :, :, es.T_MAX - 1] == s).all()) and bool((vb[:, :, :, es.T_MAX - 1] == s).all())
    # the full rows' tokens: the oracle's teacher-forced argmax unless a near-tie (test_engine_gpu.py's rule)
    ref = _shared(case)[1][0]
    for i in (0, 1):
        p = case.prompts()[i]
        lg = ref.forward(torch.tensor([p + toks[i][:-1]], device="cuda"))[0, len(p) - 1:]
        for step, t in enumerate(toks[i]):
            best = int(lg[step].argmax())
            assert best == t or float(lg[step, best] - lg[step, t]) < 0.05 * float(lg[step].std()), (i, step, best, t)
    eng.close()


# ------------------------------------------------------------------------------------------ e. continuous batch
def _pump(cb, owner, out, until):
    """Step whole chunks, collecting tokens per request and retiring finished rows, until ``until()``."""
    for _ in range(64):
        cb.step()
        new, fin = cb.poll()
        for r, ids in enumerate(new):
            out[owner[r]] += ids
        dead = [r for r, f in enumerate(fin) if f]
        if dead:
            moves = cb.retire(dead)
            alive = {moves.get(r, r): o for r, o in owner.items() if r not in dead}
            owner.clear()
            owner.update(alive)
        if until():
            return
    raise AssertionError("the script did not reach its end")


def test_continuous_batch_scripted():
    """A (30 ids, 24 tokens), B (5, 3) and C (12, 40) join; B then A leave, so C moves into a hole twice; D (3, 6)
    then takes A's freed slot.  Every request's vectors sit in its own slot; D's slot past D's length still holds A's
    vectors bit for bit; B's slot stays as B left it; the slot nobody used is all sentinel."""
    case = es.CONT
    P = dict(zip("ABCD", case.prompts()))
    n_new = dict(zip("ABCD", case.predict))
    eng = _engine(case, steps_per_graph=4)
    cb = eng.continuous()
    assert cb.admit([P[k] for k in "ABC"], [n_new[k] for k in "ABC"], [es.GREEDY] * 3) == [0, 1, 2]
    slot = dict(zip("ABC", cb.row_slot))
    owner = {0: "A", 1: "B", 2: "C"}
    out = {k: [] for k in "ABCD"}
    _pump(cb, owner, out, lambda: set(owner.values()) == {"C"})
    assert owner == {0: "C"} and cb.n == 1 and [len(out[k]) for k in "ABC"] == [24, 3, 24]
    # a row admitted at a chunk boundary idles unless its last token ends a chunk
    idled = {k: n_new[k] % eng.steps_per_graph != 0 for k in "ABCD"}
    rows = {slot[k]: es.expected_inputs(P[k], out[k], idled[k] and k != "C") for k in "ABC"}
    snap = _verify(eng, case, rows, f"{case.id}-before-D")
    (d_row,) = cb.admit([P["D"]], [n_new["D"]], [es.GREEDY])
    slot["D"] = cb.row_slot[d_row]
    owner[d_row] = "D"
    assert slot["D"] == slot["A"] and len(set(slot[k] for k in "ABC")) == 3
    _pump(cb, owner, out, lambda: cb.n == 0)
    assert [len(out[k]) for k in "ABCD"] == [24, 3, 40, 6] and cb.capacity == 4
    rows = {slot[k]: es.expected_inputs(P[k], out[k], idled[k]) for k in "BCD"}
    assert len(rows[slot["D"]]) < len(P["A"])  # A's vectors remain past D's p_last
    _verify(eng, case, rows, f"{case.id}-end", snapshot=snap, snapshot_slots=(slot["D"],))
    eng.close()


# ------------------------------------------------------------------------------------------ f. masked positions
def test_masked_positions_cannot_matter():
    """The requests of (a) in poisoned caches, and again in caches that a longer generation filled in every slot:
    the same tokens and, after every single step, the same logits bit for bit."""
    case = es.STATIC[es.LLAMA]
    clean = _engine(case)
    log_a = _record_steps(clean)
    _, toks_a, rows = _generate(clean, case, use_graph=False)
    used = _engine(case)
    vocab = case.config().vocab
    filler = [es.prompt_ids(50, vocab, 500 + i) for i in range(case.max_batch)]
    used.generate(filler, 30, [es.GREEDY] * len(filler))
    snap = es.read_kv(used)[2:]
    log_b = _record_steps(used)
    _, toks_b, _ = _generate(used, case, use_graph=False)
    assert toks_b == toks_a
    assert len(log_a) == len(log_b) == max(case.predict)
    for step, (a, b) in enumerate(zip(log_a, log_b)):
        assert torch.equal(a, b), step
    _verify(clean, case, rows, f"{case.id}-poisoned")
    _verify(used, case, rows, f"{case.id}-used", snapshot=snap, snapshot_slots=range(case.max_batch))
    clean.close()
    used.close()


# ------------------------------------------------------------------------------------------ g. the slot number
def _run_continuous(case, free_slots=None):
    """The case's requests through a continuous batch, one step at a time, rows retired as they finish (so none
    idles): (engine, slot per request, tokens per request, logits after every step)."""
    eng = _engine(case, steps_per_graph=4)
    cb = eng.continuous()
    if free_slots is not None:
        cb.free_slots = list(free_slots)
    n = len(case.lengths)
    cb.admit(case.prompts(), list(case.predict), [es.GREEDY] * n)
    slot = list(cb.row_slot)
    owner = dict(enumerate(range(n)))
    out = [[] for _ in range(n)]
    steps = []
    while cb.n:
        cb.step(1)
        with torch.cuda.stream(eng.stream):
            steps.append(eng.buf["logits"][: cb.n].clone())
        new, fin = cb.poll()
        for r, ids in enumerate(new):
            out[owner[r]] += ids
        dead = [r for r, f in enumerate(fin) if f]
        if dead:
            moves = cb.retire(dead)
            owner = {moves.get(r, r): o for r, o in owner.items() if r not in dead}
        assert len(steps) <= max(case.predict)
    return eng, slot, out, steps


def test_slot_number_cannot_matter():
    """The same requests in the same row order on two engines, the second handing out other slots: tokens, logits
    after every step and each request's cache contents are bitwise equal.  (No kernel's summation order depends on
    the slot: it only enters the cache addresses of the QKV epilogue and of attention's loads.)"""
    case = es.STATIC[es.LLAMA]
    a, slot_a, out_a, steps_a = _run_continuous(case)
    b, slot_b, out_b, steps_b = _run_continuous(case, free_slots=[0, 2, 3, 1])
    assert slot_a == [0, 1, 2] and slot_b == [1, 3, 2]
    assert out_a == out_b and tuple(len(t) for t in out_a) == case.predict
    assert len(steps_a) == len(steps_b) == max(case.predict)
    for step, (x, y) in enumerate(zip(steps_a, steps_b)):
        assert torch.equal(x, y), step
    bits = []
    for eng, slot, out in ((a, slot_a, out_a), (b, slot_b, out_b)):
        rows = {slot[i]: es.expected_inputs(p, out[i], idled=False) for i, p in enumerate(case.prompts())}
        bits.append(_verify(eng, case, rows, f"{case.id}-slots-{''.join(map(str, slot))}"))
    for i in range(len(case.lengths)):
        for x, y in zip(bits[0], bits[1]):
            assert torch.equal(x[:, slot_a[i]], y[:, slot_b[i]]), i
    a.close()
    b.close()
