"""Stop sequences on the GPU: the kernel of csrc/stopseq.hip through its ``ops`` wrapper against the Python rule
(engine/stopseq.py), step by step, then the engine.  Everything is compared as integers or bytes: no tolerance.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from cain_amd import ops  # noqa: E402
from cain_amd.engine import jsonmode as jm  # noqa: E402
from cain_amd.engine import stopseq as ss  # noqa: E402
from cain_amd.engine.engine import DecodeEngine  # noqa: E402
from engine_state import assert_untouched, poison, read_kv  # noqa: E402
from jsonmode_vocab import json_test_vocabulary  # noqa: E402
from stopseq_cases import boundary_stop, brute_force, named_cases, random_cases  # noqa: E402

DEV = torch.device("cuda")
POISON = 0xA5


def _cases(M):
    """M (stops, pieces) rows: the named cases first (the 32 one-byte tokens, both tie rules, the long pieces), then
    seeded random ones with a 70 .. 130 byte piece in every third."""
    named = [(s, p) for _, s, p in named_cases()]
    if M == 1:
        return [next((s, p) for n, s, p in named_cases() if n.startswith("a long piece, two strings"))]
    if M == 5:
        pick = ("32 bytes, 32 one-byte tokens", "equal starts: the lowest index", "suffix of another, one token",
                "a long piece, the match past its 64th byte", "near miss")
        return [next((s, p) for n, s, p in named_cases() if n == name) for name in pick]
    return (named + random_cases(seed=900 + M, n=M, long_every=3))[:M]


@pytest.mark.parametrize("M", [1, 5, 256])
def test_kernel_against_the_python_rule_step_by_step(M):
    rng = np.random.default_rng(M)
    cases = _cases(M)
    vocab = [b"", b""] + sorted({p for _, ps in cases for p in ps if p} | {b"x"})
    ids = {p: i for i, p in enumerate(vocab) if i >= 1}  # (id 0: an empty piece no case uses; 1: the empty piece)
    table = ops.json_table(vocab, DEV)
    V = len(vocab)
    # special rows: off rows hold poison for a state and must keep it; a row that is done from the start; in the
    # 5-row case row 4 ("near miss", which never hits) is a JSON-mode row whose first token JSON mode takes back
    off = set() if M == 1 else ({2} if M == 5 else set(range(7, M, 16)))
    done0 = set() if M < 256 else set(range(11, M, 32))
    json_row = 4 if M == 5 else None
    steps = max(len(p) for _, p in cases) * 3 // 2 + 8  # (rows idle in ~15 % of the steps)
    ldg = steps + 2
    on_h = [0 if m in off else (3 if m % 5 == 1 else 1) for m in range(M)]  # any non-zero value is on
    d_on, d_len, d_bytes = ops.stop_table([s for s, _ in cases], DEV)
    assert d_on.cpu().tolist() == [1] * M
    d_on = torch.tensor(on_h, dtype=torch.int32, device=DEV)
    state_h = np.full((M, ss.STATE_BYTES), POISON, dtype=np.uint8)
    exp = {}
    for m in range(M):
        if m not in off:
            exp[m] = ss.INITIAL
            state_h[m] = np.frombuffer(ss.state_bytes(ss.INITIAL), dtype=np.uint8)
    d_state = torch.from_numpy(state_h.copy()).to(DEV)
    gen = np.full((M, ldg), -7, dtype=np.int32)
    n_gen = np.zeros(M, dtype=np.int32)
    done = np.array([int(m in done0) for m in range(M)], dtype=np.int32)
    d_done = torch.from_numpy(done.copy()).to(DEV)
    fed = [0] * M  # pieces of its case each row has drawn
    gram_on = torch.tensor([int(m == json_row) for m in range(M)], dtype=torch.int32, device=DEV)
    gstate = ops.json_states([jm.INITIAL] * M, DEV)
    n_hits = n_idle = 0
    for t in range(steps):
        # the sampler's part, on the host: every live row draws its next piece -- or, now and then, nothing
        for m in range(M):
            forced = m == json_row and t == 0
            if done[m] or fed[m] >= len(cases[m][1]) or (M > 1 and not forced and rng.random() < 0.15):
                n_idle += 1
                continue
            piece = cases[m][1][fed[m]]
            tok = V + 5 if (piece == b"" and fed[m] % 2) else ids[piece]  # an id past the table appends nothing
            if m == json_row and t == 0:
                tok = ids[b"x"]  # not JSON: json_advance takes it back (and it is not one of the row's pieces)
            else:
                fed[m] += 1
            gen[m, n_gen[m]] = tok
            n_gen[m] += 1
            if m in exp and not (m == json_row and t == 0):
                exp[m], hit = ss.advance(exp[m], piece if tok < V else b"", ss.stop_bytes(cases[m][0]))
                if hit:
                    done[m] = 1
                    n_hits += 1
        d_gen, d_ng = torch.from_numpy(gen.copy()).to(DEV), torch.from_numpy(n_gen.copy()).to(DEV)
        if json_row is not None:
            assert ops.json_advance(gram_on, d_gen, d_ng, d_done, gstate, table) == 0
            if t == 0:  # the token is gone and the row is done: the stop kernel must not consume it
                n_gen[json_row] -= 1
                done[json_row] = 1
        assert ops.stop_advance(d_on, d_gen, d_ng, d_done, d_state, d_len, d_bytes, table) == 0
        torch.cuda.synchronize()
        for m in exp:
            state_h[m] = np.frombuffer(ss.state_bytes(exp[m]), dtype=np.uint8)
        got = d_state.cpu().numpy()
        bad = np.flatnonzero((got != state_h).any(1))
        assert bad.size == 0, (t, bad[:4].tolist(), [ss.state_from_bytes(got[m].tobytes()) for m in bad[:2]],
                               [exp.get(int(m)) for m in bad[:2]])
        assert d_done.cpu().numpy().tolist() == done.tolist(), t
        assert d_ng.cpu().numpy().tolist() == n_gen.tolist(), t
    # the outcome is the definition's (the reference of the CPU tests), for every row that ran its whole case
    for m, (stops, pieces) in enumerate(cases):
        if m in off or m in done0 or m == json_row:
            continue
        want = brute_force(stops, pieces)
        if want is None:
            assert exp[m][3] == -1 and (fed[m] < len(pieces) or exp[m][1] == len(pieces))
        elif fed[m] >= want[0]:
            assert (exp[m][1], exp[m][3], exp[m][4]) == want, m
    for m in off | done0:
        assert fed[m] > 0 or m in done0
    assert n_hits >= (1 if M < 256 else 60) and (M == 1 or n_idle > 0)
    if M == 5:
        assert done.tolist() == [1, 1, 0, 1, 1] and n_gen[4] == 0


def test_entry_refusals():
    lib = ops.load()
    table = ops.json_table([b"", b"a"], DEV)
    z = torch.zeros(64, dtype=torch.int32, device=DEV)
    st = ops.stop_states([ss.INITIAL], DEV)
    on, ln, by = ops.stop_table([["a"]], DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    good = [1, 2, p(on), p(z), 8, p(z), p(z), p(st), p(ln), p(by), p(table["piece_off"]), p(table["piece_bytes"])]
    assert lib.cain_stop_advance(*good, None) == 0
    for i in (2, 3, 5, 6, 7, 8, 9, 10, 11):  # each pointer null
        bad = list(good)
        bad[i] = None
        assert lib.cain_stop_advance(*bad, None) == -1, i
    for i, v in ((0, 0), (0, -3), (1, 0), (1, (1 << 23) + 1), (4, 0)):  # M, V, ldg
        bad = list(good)
        bad[i] = v
        assert lib.cain_stop_advance(*bad, None) == -1, (i, v)
    torch.cuda.synchronize()
    assert ops.stop_states_host(st) == [ss.INITIAL]  # (n_gen was 0: nothing consumed)


# ---------------------------------------------------------------- engine
def _engine(**kw):
    return DecodeEngine("tiny-llama3.1:8b", device="cuda", max_batch=4, max_context=256, seed=3, steps_per_graph=8,
                        **kw)


def _prompt(n, seed):
    return np.random.default_rng(seed).integers(16, 1000, size=n).tolist()


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


@pytest.mark.parametrize("options", [dict(temperature=0.0), dict(temperature=0.9, seed=11)], ids=["greedy", "seeded"])
def test_engine_stops_inside_a_graph(eng, options):
    """The free run, then the same request with a stop string that spans a token boundary and whose final token sits
    inside a decode graph: exactly the free run's tokens up to that token, the cut text, and a KV cache that still
    holds the poison above the final position (the row drew nothing after its stop)."""
    opts = dict(options, eos_id=-1)
    prompt = _prompt(6, 5)
    free = eng.generate([prompt], 40, opts)[0]
    assert len(free.tokens) == 40 and free.done_reason == "length"
    pieces = eng._piece_vocab()
    found = boundary_stop([pieces[t] for t in free.tokens])
    assert found is not None, free.tokens
    st, n_tok, hit_start = found
    assert (n_tok - 1) % 8 != 0 and n_tok < 40
    stop = st.decode()
    poison(eng)
    r = eng.generate([prompt], 40, dict(opts, stop=["\x00never", stop]))[0]
    kv = read_kv(eng)
    assert (1, 8, "st") in eng._graphs and (1, 1, "st") in eng._graphs
    assert r.tokens == free.tokens[:n_tok] and r.eval_count == n_tok  # exact, not rounded up to the graph
    assert r.done_reason == "stop" and r.stop_hit == stop
    raw = b"".join(pieces[t] for t in r.tokens)
    assert r.text == raw[:hit_start].decode().lstrip() and stop not in r.text
    written = torch.zeros(eng.max_batch, eng.T_max, dtype=torch.bool)
    # the prompt, then every generated token: the sampler had moved the row on to its final token's position before
    # the match ended the row (as under JSON mode's closing brace), so the idle steps that finish the graph write that
    # token's K / V there -- the final position; nothing above it
    written[0, : len(prompt) + n_tok] = True
    assert_untouched((kv[2], kv[3]), written, tag="stop row")
    eager = eng.generate([prompt], 40, dict(opts, stop=["\x00never", stop]), use_graph=False)[0]
    assert (eager.tokens, eager.text, eager.stop_hit, eager.done_reason) == (r.tokens, r.text, stop, "stop")
    same = eng.generate([prompt], 40, dict(opts, stop="\x00never"))[0]
    assert same.tokens == free.tokens and same.text == free.text and same.done_reason == "length"
    lp = eng.generate([prompt], 40, dict(opts, stop=stop), logprobs=True, top_logprobs=2)[0]
    assert lp.tokens == r.tokens and len(lp.logprobs) == n_tok and (1, 8, "lp", "st") in eng._graphs


def test_graph_without_a_stop_row_is_the_plain_graph():
    """A request without stop strings runs the graphs it always ran: the plain capture entry, which hands the runtime a
    null stop record (so the launches are today's), no stop buffers, and -- on an engine that did serve stop rows --
    the same tokens from the same cached plain graphs."""
    e = _engine()
    calls = []
    graph = e._graph

    def spy(M, steps, lp=False, gr=False, st=False):
        calls.append((M, steps, lp, gr, st))
        return graph(M, steps, lp, gr, st)

    e._graph = spy
    prompt, opts = _prompt(6, 5), dict(temperature=0.0, eos_id=-1)
    a = e.generate([prompt], 20, opts)[0]
    assert e._st is None and set(e._graphs) == {(1, 1), (1, 8)} and all(not c[4] for c in calls)
    e.generate([prompt], 20, dict(opts, stop="\x00never"))
    assert e._st is not None and {(1, 1, "st"), (1, 8, "st")} <= set(e._graphs)
    plain = {k: e._graphs[k] for k in ((1, 1), (1, 8))}
    b = e.generate([prompt], 20, opts)[0]
    assert {k: e._graphs[k] for k in plain} == plain and a.tokens == b.tokens and len(a.tokens) == 20
    e.close()


def test_json_row_with_a_stop_string():
    e = _engine()
    vocab = json_test_vocabulary()
    e.set_json_vocab(vocab)
    full = vocab + [b""] * (e.cfg.vocab - len(vocab))
    for seed in range(40):  # a free JSON run long enough to stop inside: the first such seed
        o = dict(temperature=0.9, seed=seed, eos_id=-1)
        free = e.generate([_prompt(6, 7)], 60, o, format="json")[0]
        if len(free.tokens) >= 12:
            break
    assert len(free.tokens) >= 12
    raw = b"".join(full[t] for t in free.tokens)
    found = boundary_stop([full[t] for t in free.tokens[:-1]], lo=1)  # (before the last token: the document is open)
    assert found is not None
    st, n_tok, hit_start = found
    r = e.generate([_prompt(6, 7)], 60, dict(o, stop=[st.decode()]), format="json")[0]
    late = e.generate([_prompt(6, 7)], 60, dict(o, stop=["\x00"]), format="json")[0]
    keys = set(e._graphs)
    e.close()
    assert (1, 8, "gr", "st") in keys or n_tok < 9
    assert r.tokens == free.tokens[:n_tok] and r.stop_hit == st.decode() and r.done_reason == "stop"
    assert r.text == raw[:hit_start].decode("utf-8", "replace") and r.json_state == "open"
    # a stop string that never occurs: the closing brace (or the budget) ends the row, as without it
    assert late.tokens == free.tokens and late.stop_hit is None and late.json_state == free.json_state
    assert late.done_reason == free.done_reason and late.text == free.text


def test_continuous_batch_rows_leave_and_slots_start_fresh(eng):
    opts = dict(temperature=0.0, eos_id=-1)
    prompts = [_prompt(5, 21), _prompt(7, 22), _prompt(4, 23)]
    free = eng.generate(prompts, 40, opts)
    pieces = eng._piece_vocab()
    found = boundary_stop([pieces[t] for t in free[0].tokens])
    assert found is not None
    st, n_tok, hit_start = found
    stop = st.decode()
    cb = eng.continuous()
    rows = cb.admit(prompts, [40, 40, 40], [dict(opts, stop=["\x00a", stop]), dict(opts, stop=["\x00b"]), opts])
    assert rows == [0, 1, 2]
    cb.step(1)
    fin = [False] * 3
    for _ in range(8):
        cb.step()
        _, fin = cb.poll()
        if fin[0]:
            break
    assert fin == [True, False, False]
    assert cb.tokens(0) == free[0].tokens[:n_tok] and cb.stop_hit(0) == (hit_start, 1)
    assert cb.stop_hit(1) is None and cb.stop_hit(2) is None
    slot = cb.row_slot[0]
    assert cb.retire([0]) == {2: 0}  # the row without stops moves into the hole, its (off) stop state with it
    assert cb.stops == [(), ("\x00b",)] and eng._st["stop_on"][:3].cpu().tolist() == [0, 1, 0]
    new = cb.admit([prompts[0]], [12], [opts])  # the same prompt into the freed slot, without the stop string
    assert new == [2] and cb.row_slot[2] == slot
    cb.step(1)
    out = {}
    for _ in range(8):
        cb.step()
        _, fin = cb.poll()
        for r in [i for i, f in enumerate(fin) if f and i not in out]:
            out[r] = cb.tokens(r)
        if len(out) == 3:
            break
    assert len(out[2]) == 12 and cb.stop_hit(2) is None  # it ran to its length, through where the old request stopped
    assert len(out[0]) == 40 and len(out[1]) == 40 and cb.stop_hit(1) is None
    assert ops.stop_states_host(eng._st["sstate"][2:3])[0] == ss.INITIAL  # (off rows are not advanced)
    cb.retire([0, 1, 2])
