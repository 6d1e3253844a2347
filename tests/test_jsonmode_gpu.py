"""JSON mode on the GPU: the two kernels of csrc/grammar.hip through their ``ops`` wrappers against the Python automaton
(engine/jsonmode.py), then the engine.  Everything is compared as integers or bit patterns: no tolerance, except the
one logprob case, which uses tests/test_logprob_gpu.py's stated rule.
"""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from cain_amd import ops  # noqa: E402
from cain_amd.engine import jsonmode as jm  # noqa: E402
from cain_amd.engine.engine import DecodeEngine, logprob_host  # noqa: E402
from jsonmode_vocab import json_test_vocabulary  # noqa: E402

DEV = torch.device("cuda")
PIECES = json_test_vocabulary()
POISON = -12345.5

# one prefix per state the issue lists (start, after {, inside a key, mid-escape, mid-\\u, mid-UTF-8 with a restricted
# second byte owed, after -, after 0, inside a literal, after a value in an array at depth 64, a whitespace run of 16,
# DONE), then further ones
LISTED = [b"", b"{", b'{"na', b'{"a\\', b'{"a":"\\u0', b'{"a":"\xe0', b'{"a":-', b'{"a":0', b'{"a":tr',
          b'{"a":' + b"[" * 63 + b'"x"', b"{" + b" " * 16, b"{}"]
EXTRA = [b'{"a":"\xf4', b'{"a":"\xf0\x9f', b'{"a":12', b'{"a":[1.5e', b'{"a":"x",']
STATES = [jm.run(p) for p in LISTED + EXTRA]
OFF_ROWS = {3: {1: (0, 0)}, 17: {1: (0, 0), 4: (1, 1), 9: (0, 1)}}  # M -> row -> (gram_on, done); other rows are live


def mask_rows(M):
    """(states, gram_on, done) of the M rows of a mask case.  The live rows take the states in order -- at M = 17 the 14
    live rows are every listed state and two more, M = 3 and M = 1 take the rest -- and the rows that are off or done
    hold a copy of the start state, so no state is spent on a row the kernel must skip."""
    first = {17: 0, 3: 14, 1: 16}[M]
    rows, on, done, k = [], [], [], 0
    for m in range(M):
        if m in OFF_ROWS.get(M, {}):
            g, d = OFF_ROWS[M][m]
            rows.append(STATES[0])
        else:
            g, d = (7 if m == 13 else 1), 0  # any non-zero value is on
            rows.append(STATES[(first + k) % len(STATES)])
            k += 1
        on.append(g)
        done.append(d)
    return rows, on, done


def _i32(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _tokenise(data: bytes, pieces) -> list:
    """Greedy longest-match ids of ``data``."""
    by_len = sorted(((p, i) for i, p in enumerate(pieces) if p), key=lambda x: -len(x[0]))
    out, at = [], 0
    while at < len(data):
        p, i = next((p, i) for p, i in by_len if data.startswith(p, at))
        out.append(i)
        at += len(p)
    return out


def test_states_cover_what_the_issue_lists():
    assert all(s is not None for s in STATES)
    sids = [jm.sid_of(s) for s in STATES]
    for want in (jm.START, jm.OBJ_OPEN, jm.STR, jm.STR_ESC, jm.STR_HEX, jm.STR_UTF8, jm.NUM_MINUS, jm.NUM_ZERO,
                 jm.LIT, jm.AFTER_VALUE, jm.DONE):
        assert want in sids
    assert STATES[9][1] & 0xFF == 64 and (STATES[10][0] >> 12) & 31 == 16
    assert (STATES[5][0] >> 8) & 7 == jm.U_A0_BF and (STATES[4][0] >> 5) & 7 == 3  # restricted byte owed; 3 hex owed
    live = {M: [s for s, g, d in zip(*mask_rows(M)) if g and not d] for M in (1, 3, 17)}
    assert all(s in live[17] for s in STATES[:len(LISTED)])  # every listed state is masked from, as a live row
    assert all(any(s in v for v in live.values()) for s in STATES)
    for M in (3, 17):  # and rows that are off, done, or both exist
        assert {(bool(g), bool(d)) for _, g, d in zip(*mask_rows(M))} >= {(False, False), (True, False)}
    assert {(bool(g), bool(d)) for _, g, d in zip(*mask_rows(17))} == {(False, False), (True, False), (True, True),
                                                                       (False, True)}


@pytest.mark.parametrize("with_cmax", [False, True], ids=["plain", "cmax"])
@pytest.mark.parametrize("M", [1, 3, 17])
@pytest.mark.parametrize("V,ldl", [(1024, 1024), (1040, 1056)])
def test_mask_kernel(V, ldl, M, with_cmax):
    pieces = PIECES + [b'"k":', b"\xf0\x9f\x98", b"{", b" ", b"", b"}", b"]", b",", b"9", b'"', b"\\", b"u", b"\xa0",
                       b"\x80", b"e", b"."][: V - 1024]
    table = ops.json_table(pieces, DEV)
    g = torch.Generator().manual_seed(V * 31 + M)
    lg = torch.randn(M, ldl, generator=g) * 4.0
    lg[:, V:] = POISON
    rows, on, done = mask_rows(M)
    cm0 = torch.full((M, V // 16), POISON)
    logits, cmax = lg.to(DEV), cm0.to(DEV) if with_cmax else None
    rc = ops.json_mask(logits, V, torch.tensor(on, dtype=torch.int32, device=DEV),
                       torch.tensor(done, dtype=torch.int32, device=DEV), ops.json_states(rows, DEV), table, cmax)
    torch.cuda.synchronize()
    assert rc == 0
    want = lg.clone().numpy()
    for m in range(M):
        if on[m] and not done[m]:
            ok = set(jm.allowed_ids(rows[m], pieces))
            bad = np.array([t for t in range(V) if t not in ok], dtype=np.uint32)
            want[m, bad] = -(((np.uint32(227) << np.uint32(23)) | bad).view(np.float32))
            assert len(ok) == V - len(bad) and (len(ok) > 0) == (jm.sid_of(rows[m]) != jm.DONE)
    got = logits.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))  # masked ids, their values, the rest, the pad
    for m in range(M):  # about -1e30, distinct, decreasing with the id
        if on[m] and not done[m] and jm.sid_of(rows[m]) == jm.DONE:
            assert want[m, 0] == -2.0 ** 100 and (np.diff(want[m, :V]) < 0).all() and want[m, V - 1] > -2.0 ** 101
    if with_cmax:
        cm = cm0.numpy().copy()
        for m in range(M):
            if on[m] and not done[m]:
                cm[m] = want[m, :V].reshape(-1, 16).max(1)
        assert np.array_equal(_i32(cmax), cm.view(np.int32))


def test_mask_refusals():
    table = ops.json_table(PIECES, DEV)
    lg = torch.zeros(1, 1024, device=DEV)
    z = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = ops.json_states([jm.INITIAL], DEV)
    lib = ops.load()
    args = lambda V, ldl, cm=None: (ops._p(lg), ldl, V, 1, ops._p(z), ops._p(z), ops._p(st), ops._p(table["piece_off"]),  # noqa: E731
                                    ops._p(table["piece_bytes"]), cm, None)
    assert lib.cain_json_mask(*args((1 << 23) + 16, (1 << 23) + 16)) != 0  # ids must fit the mantissa
    assert lib.cain_json_mask(*args(1024, 1000)) != 0
    assert lib.cain_json_mask(*args(1000, 1024, ops._p(lg))) != 0  # chunk maxima need whole 16-column chunks
    torch.cuda.synchronize()
    assert float(lg.abs().max()) == 0.0
    with pytest.raises(ValueError):
        ops.json_table([b"x"] * ((1 << 23) + 1), "cpu")


def test_advance_kernel():
    """Nine rows stepped together, the sampler played by the host: three documents to their end, one row off, one row
    done from the start, one that is handed an invalid token at its fourth step, one whose budget ends inside its
    document and is stepped on (only the consumed-token count tells the kernel that it wrote nothing new), and two
    that are handed a token id outside the table."""
    docs = [b'{"name": "caf\xc3\xa9 \\u00e9\\n", "id": [1, -2.5e+3, true, null], "o": {}}',
            b'{\n  "a": {"b": [[], {"c": false}]},\n  "d": "\xf0\x9f\x98\x80"\n}', b"{}"]
    scripts = [_tokenise(d, PIECES) for d in docs]
    scripts.append(scripts[0])                      # row 3: gram_on 0
    scripts.append(scripts[1])                      # row 4: done before the first step
    bad = scripts[0][:3] + [PIECES.index(b"}}")] + scripts[0][3:]
    scripts.append(bad)                             # row 5: an invalid token at step 3
    scripts.append(scripts[0][:5])                  # row 6: its budget ends mid-document, then it idles
    scripts.append(scripts[1][:2] + [len(PIECES)])  # row 7: a token id one past the table
    scripts.append([-1])                            # row 8: a negative token id
    M, T = len(scripts), 64
    table = ops.json_table(PIECES, DEV)
    on_h = [1, 1, 1, 0, 1, 1, 1, 1, 1]
    on = torch.tensor(on_h, dtype=torch.int32, device=DEV)
    gen = torch.full((M, T), -1, dtype=torch.int32)
    n_gen = [0] * M
    done = [0, 0, 0, 0, 1, 0, 0, 0, 0]
    states = [jm.INITIAL] * M
    d_gen, d_st = gen.to(DEV), ops.json_states(states, DEV)
    for step in range(max(map(len, scripts)) + 2):
        wrote = []
        for m in range(M):  # the sampler, played by the host: a live row writes its next token
            if not done[m] and n_gen[m] < len(scripts[m]):
                d_gen[m, n_gen[m]] = scripts[m][n_gen[m]]
                n_gen[m] += 1
                wrote.append(m)
                if n_gen[m] == len(scripts[m]):
                    done[m] = 1  # its budget
        d_ng = torch.tensor(n_gen, dtype=torch.int32, device=DEV)
        d_done = torch.tensor(done, dtype=torch.int32, device=DEV)
        assert ops.json_advance(on, d_gen, d_ng, d_done, d_st, table) == 0
        torch.cuda.synchronize()
        for m in wrote:  # what the kernel must have done
            if on_h[m]:
                tok = scripts[m][n_gen[m] - 1]
                states[m], ok = jm.advance(states[m], PIECES[tok] if 0 <= tok < len(PIECES) else b"")
                if not ok:
                    n_gen[m] -= 1
                    done[m] = 1
                elif jm.sid_of(states[m]) == jm.DONE:
                    done[m] = 1
        assert ops.json_states_host(d_st) == states, step
        assert d_ng.cpu().tolist() == n_gen and d_done.cpu().tolist() == done, step
    assert [jm.sid_of(s) for s in states[:6]] == [jm.DONE, jm.DONE, jm.DONE, jm.START, jm.START, jm.FAIL]
    assert n_gen[5] == 3 and n_gen[4] == 0 and n_gen[0] == len(scripts[0])
    # row 6 was stepped len(scripts[0]) - 3 more times after its budget: five tokens consumed, the document open
    want6 = jm.INITIAL
    for t in scripts[0][:5]:
        want6, _ = jm.advance(want6, PIECES[t])
    assert n_gen[6] == 5 and states[6] == want6
    assert states[6][1] >> 8 == 5 and jm.sid_of(states[6]) not in (jm.DONE, jm.FAIL, jm.START)
    assert [jm.sid_of(states[m]) for m in (7, 8)] == [jm.FAIL, jm.FAIL] and n_gen[7:] == [2, 0] and done[7:] == [1, 1]
    assert states[0][1] >> 8 == len(scripts[0])  # tokens consumed


# ---------------------------------------------------------------- engine
ENGINES = [("tiny-llama3.1:8b", "bf16"), ("tiny-llama3.1:8b", "fp4"), ("tiny-gemma:2b", "bf16"),
           ("tiny-gemma:2b", "fp4")]


def _engine(name, wd, vocab=True, **kw):
    eng = DecodeEngine(name, device="cuda", max_batch=8, max_context=256, seed=3, steps_per_graph=4, weight_dtype=wd,
                       **kw)
    if vocab:
        eng.set_json_vocab(PIECES)
    return eng


def _prompt(n, seed):
    return np.random.default_rng(seed).integers(16, 1000, size=n).tolist()


def _check_json_row(r, budget):
    s = jm.INITIAL
    for t in r.tokens:
        assert jm.token_ok(s, PIECES[t]), (r.tokens, t)
        s, _ = jm.advance(s, PIECES[t])
    data = b"".join(PIECES[t] for t in r.tokens)
    assert r.json_state in ("done", "open")
    if len(r.tokens) < budget:
        assert r.json_state == "done"
    if r.json_state == "done":
        assert r.done_reason == "stop" and data.endswith(b"}") and isinstance(json.loads(data.decode("utf-8")), dict)
    else:
        assert r.done_reason == "length" and len(r.tokens) == budget and jm.viable(data)


@pytest.mark.parametrize("name,wd", ENGINES)
def test_engine_json_rows_and_untouched_neighbours(name, wd):
    """Batch 1, and batch 5 with rows 1 and 3 in JSON mode, graphs on: JSON rows are viable at every token and end on
    the closing brace; the other rows' tokens are bitwise those of the same batch with no JSON row; an engine with a
    vocabulary installed but no JSON request equals one that never had one."""
    eng = _engine(name, wd)
    bare = _engine(name, wd, vocab=False)
    prompts = [_prompt(4 + 2 * i, 60 + i) for i in range(5)]
    opts = [dict(temperature=0.9, repeat_penalty=1.1, seed=200 + i, eos_id=-1) for i in range(5)]
    one = eng.generate(prompts[:1], 96, opts[:1], format="json")[0]
    nps = [48, 6, 48, 48, 48]  # (row 1: a JSON row whose budget ends first and that idles for 42 more steps)
    off = eng.generate(prompts, nps, opts)
    mixed = eng.generate(prompts, nps, opts, format=[None, "json", None, "json", None])
    never = bare.generate(prompts, nps, opts)
    keys = set(eng._graphs)
    eng.close()
    bare.close()
    assert (1, 1, "gr") in keys and (5, 4, "gr") in keys and (5, 4) in keys  # graphs of their own
    _check_json_row(one, 96)
    for i in (1, 3):
        _check_json_row(mixed[i], nps[i])
    for i in (0, 2, 4):
        assert mixed[i].tokens == off[i].tokens and mixed[i].json_state is None and len(off[i].tokens) == 48
    assert [r.tokens for r in off] == [r.tokens for r in never]


def test_engine_wide_top_k_draws_only_accepted_tokens():
    """top_k = 1,000 (the kernels clamp to 256) from states that accept fewer than 40 tokens, on every sampler kernel
    the runtime can pick: the masked values are distinct, so they rank below every accepted token and draw
    probability exactly 0."""
    assert len(jm.allowed_ids(jm.INITIAL, PIECES)) < 40 and len(jm.allowed_ids(jm.run(b'{"a"'), PIECES)) < 40
    eng = _engine("tiny-llama3.1:8b", "bf16")
    mode0 = ops.sample_cm_mode()
    try:
        for mode in (3, 1, 0):
            ops.set_sample_cm(mode)
            prompts = [_prompt(5, 80 + i) for i in range(3)]
            opts = [dict(temperature=2.0, top_k=1000, top_p=1.0, repeat_penalty=1.0, seed=mode * 10 + i, eos_id=-1)
                    for i in range(3)]
            res = eng.generate(prompts, 24, opts, use_graph=False, format="json")  # (eager: the mode is read per forward)
            for r in res:
                _check_json_row(r, 24)
    finally:
        ops.set_sample_cm(mode0)
        eng.close()


def test_engine_logprobs_stay_the_raw_distribution():
    """A JSON row with logprobs: its tokens are those without logprobs; graph replay and eager steps give bitwise the
    same logprobs; and EVERY generated token's logprob and alternatives are those of the step's raw logits (host
    float64 log-softmax, test_logprob_gpu.py's tolerance rule), not of the masked ones.  The raw logits of a step: in
    the eager run each decode forward is preceded by the same forward without sampler, logprobs and mask -- same
    kernels, same single row, same inputs, so bitwise the logits the step's LM head then writes -- and the logits
    buffer is copied before the step's mask and sampler change it."""
    tol = lambda ref: 2e-5 * max(1.0, abs(ref) / 32.0)  # noqa: E731
    eng = _engine("tiny-llama3.1:8b", "bf16")
    p = _prompt(7, 91)
    for seed in range(40):  # a document that stays open for a while: history, nesting, states beyond the start
        o = dict(temperature=0.8, repeat_penalty=1.1, seed=seed, eos_id=-1)
        a = eng.generate([p], 24, [o], format="json")[0]
        if len(a.tokens) >= 12:
            break
    assert len(a.tokens) >= 12
    b = eng.generate([p], 24, [o], format="json", logprobs=True, top_logprobs=3)[0]
    keys = set(eng._graphs)
    raw, forward = [], eng._forward

    def spy(M, rows, want_logits, want_sample, **kw):
        if want_sample:
            forward(M, rows, want_logits=True, want_sample=False)
            raw.append(eng.buf["logits"][0].clone())
        return forward(M, rows, want_logits=want_logits, want_sample=want_sample, **kw)

    eng._forward = spy
    c = eng.generate([p], 24, [o], use_graph=False, format="json", logprobs=True, top_logprobs=3)[0]
    eng._forward = forward
    raw = [r.cpu() for r in raw]
    eng.close()
    assert a.tokens == b.tokens == c.tokens and len(b.logprobs) == len(b.tokens) and (1, 1, "lp", "gr") in keys
    assert any(k[1] == 4 and k[2:] == ("lp", "gr") for k in keys)  # whole chunks ran as graphs
    _check_json_row(b, 24)
    assert np.array_equal(np.float32(b.logprobs).view(np.int32), np.float32(c.logprobs).view(np.int32))
    assert b.top_logprobs == c.top_logprobs
    assert len(raw) >= len(c.tokens)
    s, n_masked_top = jm.INITIAL, 0
    for j, t in enumerate(c.tokens):
        ls, top = logprob_host(raw[j], 3)
        assert abs(c.logprobs[j] - ls[t]) <= tol(ls[t]), j
        assert [i for i, _ in c.top_logprobs[j]] == [i for i, _ in top], j
        assert all(abs(x - y) <= tol(y) for (_, x), (_, y) in zip(c.top_logprobs[j], top)), j
        n_masked_top += sum(not jm.token_ok(s, PIECES[i]) for i, _ in top)
        s, _ = jm.advance(s, PIECES[t])
    assert n_masked_top > 0  # the alternatives are the model's own: some of them the grammar forbids


def test_continuous_batch_moves_the_state_with_the_row():
    """Row 0 (plain, short) retires while row 1 (JSON) is inside its document: the JSON row moves to index 0 and
    continues from its state -- its tokens are those of the same request run alone."""
    eng = _engine("tiny-llama3.1:8b", "bf16")
    for seed in range(40):  # a request whose document is still open when the plain row retires (4 steps in)
        oj = dict(temperature=0.9, seed=seed, eos_id=-1)
        alone = eng.generate([_prompt(6, 7)], 40, [oj], format="json")[0]
        if len(alone.tokens) >= 10:
            break
    assert len(alone.tokens) >= 10
    cb = eng.continuous()
    assert cb.admit([_prompt(5, 8), _prompt(6, 7)], [4, 40], [dict(temperature=0.0, eos_id=-1), oj],
                    format=[None, "json"]) == [0, 1]
    cb.step()
    _, fin = cb.poll()
    assert fin[0] and not fin[1] and cb.json_state(0) is None and cb.json_state(1) == "open"
    assert cb.retire([0]) == {1: 0}
    assert cb.json_state(0) == "open"
    for _ in range(12):
        cb.step()
        _, fin = cb.poll()
        if fin[0]:
            break
    toks, state = cb.tokens(0), cb.json_state(0)
    eng.close()
    assert fin[0] and toks == alone.tokens and state == alone.json_state
