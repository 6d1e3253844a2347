"""Speculative decoding on the GPU: the draft / accept kernels of csrc/spec.hip against the host rule and the
sequential host sampler, and engines decoding with it against the oracle and against plain decoding."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import engine_state as es  # noqa: E402
import sampler_ref as sr  # noqa: E402
from cain_amd import ops  # noqa: E402
from cain_amd.engine import DecodeEngine  # noqa: E402
from cain_amd.engine import speculative as sp  # noqa: E402
from cain_amd.models.reference import ReferenceModel  # noqa: E402

DEV = "cuda"
T_MAX = 256
V = 512
GREEDY = dict(temperature=0.0, top_p=1.0, repeat_penalty=1.0, top_k=1, repeat_last_n=0, eos_id=-1, seed=0)
PROMPTS = ["In 100 words, please give me information about India",
           "In 500 words, please give me information about Elizabeth II, Queen of the United Kingdom and more",
           "hi"]
ENGINE_GREEDY = dict(temperature=0.0, repeat_penalty=1.0, eos_id=-1)


def dev_rows(state):
    return {k: torch.tensor(np.asarray(state[k]), dtype=torch.int32, device=DEV).contiguous() for k in ops.ROW_KEYS}


# ------------------------------------------------------------------------------------------ draft kernel
def _sequences():
    """(record, pos, ng, max_new, done, masked) of every case: the hand-written ones of tests/test_spec_cpu.py, the
    edge positions, and random records over 4 symbols (many matches at every n-gram length)."""
    rng = np.random.default_rng(5)
    hand = [[1, 2, 3, 4, 5], [7], [9, 1, 2, 3, 7, 8, 1, 2, 3], [5, 2, 3, 6, 4, 2, 3], [5, 3, 6, 4, 2, 3],
            [1, 2, 3, 4, 1, 2, 3, 5, 1, 2, 3], [1, 2, 3, 4, 9, 3, 6, 1, 2, 3], [4, 4], [1, 7, 7, 7, 7], [3, 3, 3],
            [3, 5, 3]]
    out = [(s, len(s) - 1, int(rng.choice([0, 5, 62, 63, 64, 130])), 10_000, 0, False) for s in hand]
    for pos in (0, 1, 2, 3, 63, 64, 65, 200, T_MAX - 4, T_MAX - 3, T_MAX - 2, T_MAX - 1):
        for _ in range(2):
            rec = rng.integers(0, 4, pos + 1).tolist()
            out.append((rec, pos, int(rng.choice([0, 1, 62, 63, 64, 65, 199])), 10_000, 0, False))
    rec = rng.integers(0, 4, 120).tolist()
    out += [(rec, 119, 7, 9, 0, False), (rec, 119, 7, 8, 0, False), (rec, 119, 7, 10, 0, False),  # max_new clips
            (rec, 119, 7, 10_000, 1, False), (rec, 119, 7, 10_000, 0, True)]                    # done, masked
    return out


@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("mode", [0, 1], ids=["ngram", "given"])
def test_draft_kernel_matches_the_rule(K, R, mode):
    rng = np.random.default_rng(100 * K + 10 * R + mode)
    seqs = _sequences()
    seqs += seqs[: (-len(seqs)) % R]
    slots = R + 2
    for g in range(0, len(seqs), R):
        group = seqs[g: g + R]
        spec = ops.spec_alloc(R, K, slots, T_MAX, V, DEV)
        use = rng.permutation(slots)[:R]  # rows do not sit in their own slot
        state = dict(tok=[], pos=[], slot=[], n_gen=[], max_new=[], done=[], hist=rng.integers(0, V, (R, 64)))
        seq = rng.integers(0, 4, (slots, T_MAX))  # (other slots and the positions past pos hold plausible tokens too)
        given = rng.integers(0, V, (R, T_MAX))
        given[rng.random((R, T_MAX)) < 0.15] = -1
        given[rng.random((R, T_MAX)) < 0.02] = V + 3
        opts = []
        for r, (rec, pos, ng, mn, dn, masked) in enumerate(group):
            seq[use[r], : pos + 1] = rec
            for k, v in zip(("tok", "pos", "slot", "n_gen", "max_new", "done"),
                            (rec[pos], pos, -1 if masked else use[r], ng, mn, dn)):
                state[k].append(v)
            opts.append(dict(GREEDY, temperature=0.5 + r, top_k=7 + r, seed=1000 + r, eos_id=3 + r, stop=(r, 2 * r)))
        params = ops.sample_params_tensor(opts, DEV)
        spec["seq"].copy_(torch.tensor(seq, dtype=torch.int32))
        spec["given"].copy_(torch.tensor(given, dtype=torch.int32))
        rows = dev_rows(state)
        ops.spec_draft(rows, params, spec, R, mode, T_MAX)
        torch.cuda.synchronize()
        want = ops.spec_draft_ref(rows, params, spec, R, mode, T_MAX)
        n = R * (K + 1)
        for k, w in want.items():
            got = spec[k].cpu().numpy()
            got = got.reshape(-1, ops.SAMPLE_BYTES)[:n] if k == "x_params" else got[: len(w)]
            assert np.array_equal(got, w), (k, g, [s[1:] for s in group], got.tolist(), w.tolist())
        if mode == 0:  # the rule itself, spelled out once more
            for r, (rec, pos, ng, mn, dn, masked) in enumerate(group):
                d = [] if dn or masked else sp.ngram_draft(rec, pos, K)[: sp.clip(K, pos, ng, K, T_MAX, mn)]
                assert want["nd"][r] == len(d) and want["draft"][r, : len(d)].tolist() == d


def test_draft_and_accept_refuse_bad_arguments():
    spec = ops.spec_alloc(2, 3, 2, T_MAX, V, DEV)
    lib = ops.load()
    s = ops.spec_struct(spec, 0)
    s.K = 8
    import ctypes
    z = torch.zeros(64 * 2, dtype=torch.int32, device=DEV)
    p = [ctypes.c_void_p(z.data_ptr())] * 8
    assert lib.cain_spec_draft(ctypes.byref(s), 2, T_MAX, *p, None) == -1
    s = ops.spec_struct(spec, 0)
    assert lib.cain_spec_draft(ctypes.byref(s), 2, T_MAX + 1, *p, None) == -1  # the record is narrower than T_max
    assert lib.cain_spec_draft(ctypes.byref(s), 0, T_MAX, *p, None) == -1


# ------------------------------------------------------------------------------------------ sampler + accept
KINDS = {"greedy": dict(GREEDY),
         "sampled": dict(temperature=0.8, top_p=0.9, repeat_penalty=1.0, top_k=40, repeat_last_n=0, eos_id=-1),
         "penalty": dict(temperature=0.8, top_p=0.9, repeat_penalty=1.1, top_k=40, repeat_last_n=64, eos_id=-1)}


def _sequential_picks(logits, ring, ng, opts):
    """The tokens plain decoding draws from rows 0 .. K in turn (stream index ng + j, the ring growing by each
    pick); every row must be decided under sampler_ref's rule."""
    ring = list(ring)
    picks = []
    for j in range(logits.shape[0]):
        ref = sr.reference_detail(logits[j], ring, ng + j, opts)
        assert ref.decided, ("an undecided row in constructed logits", j)
        picks.append(int(ref.token))
        ring[(ng + j) & 63] = picks[-1]
    return picks


def _run_step(K, seqs):
    """``seqs``: per sequence dict(logits [K + 1, V], opts, ng, pos, max_new, drafts).  One device step in given
    mode -- draft kernel, the sampler over the expanded rows, accept kernel -- and the expected state: the start
    state advanced token by token with sampler_ref.advance_reference.  Returns (device state, expected, spec)."""
    R = len(seqs)
    rng = np.random.default_rng(77)
    state = sr.new_state(R, V, rng, [s["ng"] for s in seqs], pos=[s["pos"] for s in seqs],
                         max_new=[s["max_new"] for s in seqs])
    state["slot"] = np.arange(R, dtype=np.int32)[::-1].copy()
    spec = ops.spec_alloc(R, K, R, T_MAX, V, DEV)
    given = np.full((R, T_MAX), -1)
    for r, s in enumerate(seqs):
        given[r, s["ng"]: s["ng"] + len(s["drafts"])] = s["drafts"]
    spec["given"].copy_(torch.tensor(given, dtype=torch.int32))
    seq0 = rng.integers(0, V, (R, T_MAX))
    spec["seq"].copy_(torch.tensor(seq0, dtype=torch.int32))
    opts = [s["opts"] for s in seqs]
    params = ops.sample_params_tensor(opts, DEV)
    rows = dev_rows(state)
    gen = torch.tensor(state["gen"], dtype=torch.int32, device=DEV)
    logits = torch.tensor(np.concatenate([s["logits"] for s in seqs]), dtype=torch.float32, device=DEV)
    ops.spec_draft(rows, params, spec, R, 1, T_MAX)
    ops.sample(logits, spec["x_tok"], spec["x_pos"], spec["x_gen"], spec["x_n_gen"], spec["x_max_new"],
               spec["x_done"], spec["x_hist"], spec["x_slot"], spec["x_params"], T_MAX)
    ops.spec_accept(rows, gen, params, spec, R, T_MAX)
    torch.cuda.synchronize()
    got = {k: rows[k].cpu().numpy() for k in ops.ROW_KEYS}
    got["hist"] = got["hist"].reshape(R, 64)
    got["gen"] = gen.cpu().numpy()
    # expected: the sequential reference, token by token
    want = {k: np.array(state[k], copy=True) for k in sr.STATE_KEYS}
    counts, seq_want = [], seq0.copy()
    for r, s in enumerate(seqs):
        picks = _sequential_picks(s["logits"], state["hist"][r], s["ng"], s["opts"])
        d = len(sp.draft([], s["pos"], s["ng"], K, T_MAX, s["max_new"], given=given[r], vocab=V))
        a = sp.accepted_length(s["drafts"][:d], picks)
        c = 0
        for j in range(a + 1):
            if want["done"][r]:
                break
            one = [0] * R
            one[r] = picks[j]
            mask = {k: np.array(want[k], copy=True) for k in sr.STATE_KEYS}
            mask["slot"] = np.where(np.arange(R) == r, mask["slot"], -1)  # advance this row only
            p_before = int(want["pos"][r])
            adv = sr.advance_reference(mask, one, opts, T_MAX)
            for k in sr.STATE_KEYS:
                if k != "slot":
                    want[k][r] = adv[k][r]
            if p_before + 1 < T_MAX:
                seq_want[state["slot"][r], p_before + 1] = picks[j]
            c += 1
        counts.append((d, a, c))
    for k in sr.STATE_KEYS:
        assert np.array_equal(got[k], want[k]), (k, got[k].tolist(), want[k].tolist())
    assert np.array_equal(spec["seq"].cpu().numpy(), seq_want)
    assert spec["drafted"].cpu().tolist() == [d for d, _, _ in counts]
    assert spec["accepted"].cpu().tolist() == [c - 1 for _, _, c in counts]
    assert spec["step_tokens"][:, 0].cpu().tolist() == [c for _, _, c in counts]
    assert spec["n_step"].cpu().tolist() == [1] * R
    # ... and the array form of the host rule says the same
    ref = ops.spec_accept_ref(dev_rows(state), torch.tensor(state["gen"]), params, _before_accept(spec, seq0), R, T_MAX)
    for k in sr.STATE_KEYS:
        assert np.array_equal(ref[k], want[k]), ("spec_accept_ref", k)
    assert np.array_equal(ref["seq"], seq_want)
    return got, counts


def _before_accept(spec, seq0):
    s = dict(spec)
    s["seq"] = torch.tensor(seq0, dtype=torch.int32)
    for k in ("drafted", "accepted", "n_step", "step_tokens"):
        s[k] = torch.zeros_like(spec[k])
    return s


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("K", [3, 7])
def test_sampler_and_accept_match_the_sequential_reference(kind, K):
    """Drafts taken from the reference's own picks so that acceptance lengths 0, 1, K - 1 and K all occur; then a
    stop id in the middle of an accepted run, and the max_new / T_max truncations."""
    rng = np.random.default_rng(len(kind) * 10 + K)
    seqs, targets = [], [0, 1, K - 1, K, K, K, K]
    for r, a in enumerate(targets):
        opts = dict(KINDS[kind], seed=500 + r)
        ng, pos, max_new = [0, 3, 62, 64, 9, 20, 130][r], 40 + r, 10_000
        logits = (rng.standard_normal((K + 1, V)) * 4).astype(np.float32)
        picks = _sequential_picks(logits, sr.new_state(len(targets), V, np.random.default_rng(77), 0)["hist"][r], ng,
                                  opts)
        drafts = list(picks[:K])
        if a < K:
            drafts[a] = (drafts[a] + 1) % V  # draft a + 1 is not the token row a draws
        if r == 4:
            opts["eos_id"] = picks[1]  # a stop id inside the accepted run: t_0, t_1 and no more
            if picks[0] == picks[1]:
                opts["eos_id"] = -1
        if r == 5:
            max_new = ng + 2           # the budget clips the draft to one token
        if r == 6:
            pos = T_MAX - 2            # the context too; the second token ends the sequence
        seqs.append(dict(logits=logits, opts=opts, ng=ng, pos=pos, max_new=max_new, drafts=drafts))
    _, counts = _run_step(K, seqs)
    assert [c[1] for c in counts[:4]] == [0, 1, K - 1, K] and [c[2] for c in counts[:4]] == [1, 2, K, K + 1]
    assert counts[5][0] == 1 and counts[6][0] == 1 and counts[5][2] == 2 and counts[6][2] == 2


def test_a_draft_in_the_ring_changes_the_next_pick():
    """Repeat penalty: row 1's logits favour the token row 0 draws; with that draft written into row 1's ring the
    penalty moves the pick to the runner-up, as it does in plain decoding."""
    K = 3
    opts = dict(GREEDY, repeat_penalty=1.5, repeat_last_n=64)
    logits = np.full((K + 1, V), -1.0, dtype=np.float32)
    X, Y, Z = 17, 300, 45
    logits[0, X] = 5.0
    logits[1, X], logits[1, Y] = 5.0, 4.0   # X / 1.5 < Y once X is in the ring
    logits[2, Z] = 3.0
    logits[3, Z], logits[3, 9] = 3.0, 2.5   # and again: Z / 1.5 < 9's logit
    ring = sr.new_state(1, V, np.random.default_rng(77), 0)["hist"][0]
    assert not {X, Y, Z, 9} & set(ring[:0].tolist())
    assert _sequential_picks(logits, ring, 0, opts) == [X, Y, Z, 9]
    assert sr.reference_detail(logits[1], ring, 0, opts).token == X  # without the draft in the ring
    got, counts = _run_step(K, [dict(logits=logits, opts=opts, ng=0, pos=30, max_new=100, drafts=[X, Y, Z])])
    assert counts == [(3, 3, 4)] and got["gen"][0, :4].tolist() == [X, Y, Z, 9]


# ------------------------------------------------------------------------------------------ engines
def _oracle_logits(ref, p_ids, toks):
    """fp32 logits that predicted each of ``toks`` after ``p_ids`` (teacher forcing)."""
    seq = torch.tensor([list(p_ids) + list(toks[:-1])], device=DEV)
    return ref.forward(seq)[0, len(p_ids) - 1:].float()


def _teacher_forced(ref, p_ids, toks, tie=0.05):
    """tests/test_engine_gpu.py's criterion: each token is the oracle's argmax or within a near-tie of it."""
    lg = _oracle_logits(ref, p_ids, toks)
    exact = 0
    for s, t in enumerate(toks):
        best = int(lg[s].argmax())
        if best == t:
            exact += 1
        else:
            margin = float(lg[s, best] - lg[s, t])
            assert margin < tie * float(lg[s].std()), (s, best, t, margin)
    return exact


def _first_near_tie(ref, p_ids, toks, tie=0.05):
    """The first generated index at which the oracle's top two logits are a near-tie (len(toks): none)."""
    lg = _oracle_logits(ref, p_ids, toks)
    top = lg.topk(2, dim=-1).values
    near = (top[:, 0] - top[:, 1]) < tie * lg.std(dim=-1)
    hit = near.nonzero()
    return int(hit[0]) if len(hit) else len(toks)


@pytest.mark.parametrize("name,dtype", [("tiny-llama3.1:8b", "bf16"), ("tiny-llama3.1:8b", "q4_k"),
                                        ("tiny-qwen2:1.5b", "bf16"), ("tiny-qwen2:1.5b", "fp4"),
                                        ("tiny-phi3:3.8b", "bf16"), ("tiny-phi3:3.8b", "fp4")])
def test_engine_greedy_ngram_tracks_the_oracle(name, dtype):
    case = es.Case("spec", name, (), (), weight_dtype=dtype)
    eng = DecodeEngine(name, device=DEV, max_batch=4, max_context=T_MAX, keep_natural=True, seed=13,
                       steps_per_graph=8, weight_dtype=dtype, speculative=3)
    models = es.models_for(eng.weights, case)
    res = eng.generate(PROMPTS, 48, [ENGINE_GREEDY] * 3)
    exact = total = 0
    rows = {}
    for i, r in enumerate(res):
        assert sum(r.step_tokens) == r.eval_count == 48 and r.decode_steps == len(r.step_tokens)
        assert r.draft_accepted == 48 - r.decode_steps and 0 <= r.draft_accepted <= r.draft_count
        exact += _teacher_forced(models[0], r.prompt_tokens, r.tokens)
        total += 48
        rows[i] = (list(r.prompt_tokens) + list(r.tokens))[: len(r.prompt_tokens) + 48 - 2]  # positions < final pos
    assert exact / total > 0.9, (exact, total)
    want, limit, _ = es.expectations(models, rows, eng.max_batch)
    es.compare(es.read_kv(eng)[:2], want, limit, tag=f"spec-{name}-{dtype}")
    print(f"{name} {dtype}: steps {[r.decode_steps for r in res]} drafted {[r.draft_count for r in res]} "
          f"accepted {[r.draft_accepted for r in res]}")
    eng.close()


def _expected_counts(K, given, toks, max_new):
    """Tokens per step of the host rule when the sampler draws ``toks``."""
    out, ng = [], 0
    while ng < len(toks):
        d = sp.given_draft(given, ng, K)[: max(0, min(K, max_new - 1 - ng))]
        a = sp.accepted_length(d, toks[ng: ng + len(d)])
        out.append(a + 1)
        ng += a + 1
    return out


@pytest.mark.parametrize("K", [3, 7])
@pytest.mark.parametrize("opts", [ENGINE_GREEDY, dict(temperature=0.8, seed=21, eos_id=-1)], ids=["greedy", "seeded"])
def test_engine_given_drafts_follow_plain_decoding(K, opts):
    name, n = "tiny-llama3.1:8b", 48
    kw = dict(device=DEV, max_batch=1, max_context=T_MAX, keep_natural=True, seed=13, steps_per_graph=4)
    plain = DecodeEngine(name, **kw)
    base = plain.generate(PROMPTS[:1], n, [opts])[0]
    ref = ReferenceModel(plain.weights)
    prefix = _first_near_tie(ref, base.prompt_tokens, base.tokens)
    spec = DecodeEngine(name, weights=plain.weights, speculative=K, **kw)
    corrupt = [t if i % 5 != 4 else (t + 1) % spec.cfg.vocab for i, t in enumerate(base.tokens)]
    for given, label in ((base.tokens, "own"), (corrupt, "corrupted")):
        r = spec.generate(PROMPTS[:1], n, [opts], drafts=[given])[0]
        assert r.eval_count == n == sum(r.step_tokens)
        assert r.tokens[:prefix] == base.tokens[:prefix], (label, prefix)
        want = _expected_counts(K, given, base.tokens, n)
        at = 0
        for got, w in zip(r.step_tokens, want):  # the steps that lie inside the equal prefix
            if at + K + 1 > prefix:
                break
            assert got == w, (label, at, r.step_tokens, want)
            assert label != "own" or got == min(K + 1, n - at)
            at += got
        print(f"K={K} {label}: prefix {prefix}, steps {r.decode_steps}, accepted {r.draft_accepted}/{r.draft_count}")
        if label == "own":
            assert r.draft_accepted > 0 and r.decode_steps < n
    # the eager path runs the same steps as the graphs
    g = spec.generate(PROMPTS[:1], 12, [opts], drafts=[base.tokens])[0]
    e = spec.generate(PROMPTS[:1], 12, [opts], drafts=[base.tokens], use_graph=False)[0]
    assert g.tokens == e.tokens and g.step_tokens == e.step_tokens
    plain.close()
    spec.close()


def test_continuous_batch():
    """Three requests, one admitted later, a short one retired while the others decode."""
    eng = DecodeEngine("tiny-llama3.1:8b", device=DEV, max_batch=4, max_context=T_MAX, keep_natural=True, seed=13,
                       steps_per_graph=4, speculative=3)
    ref = ReferenceModel(eng.weights)
    cb = eng.continuous()
    assert cb.capacity == 4
    budget = {0: 40, 1: 6, 2: 30}
    prompts = {i: eng.encode(PROMPTS[i]) for i in range(3)}
    live = dict(zip(cb.admit([prompts[0], prompts[1]], [budget[0], budget[1]], [ENGINE_GREEDY] * 2), (0, 1)))
    out = {i: [] for i in range(3)}
    stats, admitted_late, rounds = {}, False, 0
    while live:
        rounds += 1
        assert rounds < 100
        cb.step()
        new, fin = cb.poll()
        for row, ids in enumerate(new):
            out[live[row]] += ids
        done_rows = [row for row, f in enumerate(fin) if f]
        for row in done_rows:
            stats[live[row]] = cb.spec_stats(row)
        if done_rows:
            assert len(live) > len(done_rows) or admitted_late  # the short row leaves while others decode
            moves = cb.retire(done_rows)
            live = {moves.get(row, row): i for row, i in live.items() if row not in done_rows}
        if not admitted_late and rounds == 2:
            live[cb.admit([prompts[2]], [budget[2]], [ENGINE_GREEDY])[0]] = 2
            admitted_late = True
    exact = 0
    for i in range(3):
        assert len(out[i]) == budget[i]  # no row exceeds max_new
        assert sum(stats[i]["step_tokens"]) == budget[i]
        exact += _teacher_forced(ref, prompts[i], out[i])
    assert exact / sum(budget.values()) > 0.9
    with pytest.raises(ValueError, match="logprobs"):
        cb.admit([prompts[0]], [4], [ENGINE_GREEDY], logprobs=True)
    eng.close()


def test_context_end():
    """A prompt of T_max - 3 tokens with K = 7 ends done, writes nothing past T_max - 1 and nothing into the
    neighbouring slots."""
    eng = DecodeEngine("tiny-llama3.1:8b", device=DEV, max_batch=3, max_context=T_MAX, seed=13, steps_per_graph=4,
                       speculative=7)
    assert eng.max_batch == 3
    es.poison(eng)
    # (a repeating prompt: the n-gram lookup drafts from the first step on)
    prompt = (es.prompt_ids(11, eng.cfg.vocab, 3) * 30)[: T_MAX - 3]
    r = eng.generate([prompt], 100, [ENGINE_GREEDY])[0]
    assert r.eval_count == 3 and r.done_reason == "length" and sum(r.step_tokens) == 3
    # (the engine's budget is T_max - len(prompt) = 3 tokens: the third ends the row, its position stays T_max - 2)
    assert int(eng.rows["done"][0]) == 1 and int(eng.rows["pos"][0]) == T_MAX - 2
    assert r.draft_count <= 2  # never a draft row at or past T_max - 1 + 1, nor past the budget
    bits = es.read_kv(eng)[2:]
    written = torch.zeros(eng.max_batch, T_MAX, dtype=torch.bool)
    written[0] = True  # slot 0 may hold anything; slots 1 and 2 keep every sentinel
    es.assert_untouched(bits, written, tag="context-end")
    assert eng._spec_bufs()["seq"][0, : T_MAX].cpu().tolist()[: T_MAX - 3] == prompt
    eng.close()


def test_row_limit():
    eng = DecodeEngine("tiny-llama3.1:8b", device=DEV, max_batch=40, max_context=T_MAX, weight_dtype="q4_k",
                       speculative=7)
    assert eng.max_batch == 64 // 8 and eng.continuous().capacity == 8
    import ctypes

    lib = ops.load()
    rs, s = eng._rows_struct(eng.rows, True), ops.spec_struct(eng._spec_bufs(), 0)
    step = ops.CainStep(plan=eng._plan(64), rows=ctypes.pointer(rs), spec=ctypes.pointer(s), M=9, want_logits=1,
                        want_sample=1)
    rc = lib.cain_step_run(ctypes.byref(step), ctypes.c_void_p(eng.stream.cuda_stream))
    assert rc == -1  # 9 x 8 rows are more than a forward of this plan may have; nothing launched
    eng.close()


OFF_SCRIPT = r"""
import json, sys
from cain_amd.engine import DecodeEngine
P = ["In 100 words, please give me information about India", "hi"]
O = [dict(temperature=0.8, seed=5, eos_id=-1), dict(temperature=0.0, eos_id=-1)]
kw = dict(device="cuda", max_batch=2, max_context=256, seed=13, steps_per_graph=4)
def run(**extra):
    e = DecodeEngine("tiny-llama3.1:8b", **kw, **extra)
    out = [r.tokens for r in e.generate(P, 14, O)]
    keys = sorted(e._graphs)
    e.close()
    return out, keys
before, keys_before = run()
spec, keys_spec = run(speculative=3)
after, keys_after = run(speculative=0)
print(json.dumps(dict(before=before, after=after, spec=spec, keys_before=keys_before, keys_after=keys_after,
                      keys_spec=[list(map(str, k)) for k in keys_spec])))
"""


def test_off_means_off():
    """An engine with speculative=0 gives the tokens the same engine gave before any speculative engine existed in
    the process, from graphs under the old cache keys (a fresh process: this one has run speculative engines)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", OFF_SCRIPT], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["before"] == d["after"]
    assert d["keys_before"] == d["keys_after"] == [[2, 1], [2, 4]]
    assert all("spec" in k for k in d["keys_spec"]) and d["keys_spec"]
