"""Draft-model speculative decoding on the GPU: the kernels of csrc/spec.hip's draft-model mode against the host rule,
engines with a draft model against the same engines without one, and what both KV caches hold afterwards."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import engine_state as es  # noqa: E402
import test_spec_gpu as tsg  # noqa: E402
from cain_amd import ops  # noqa: E402
from cain_amd.engine import DecodeEngine  # noqa: E402
from cain_amd.engine import speculative as sp  # noqa: E402
from cain_amd.models.reference import ReferenceModel  # noqa: E402

DEV = "cuda"
T_MAX = 256
V = tsg.V
DV, DBOS = 3, 1  # the kernels' draft vocabulary: the records hold ids 0 .. 9, so ids >= DV occur in every group
PROMPTS = tsg.PROMPTS
GREEDY = tsg.ENGINE_GREEDY
SEEDED = dict(temperature=0.8, seed=21, eos_id=-1)
PAIRS = {"qwen2-bf16": ("tiny-qwen2:7b", "tiny-qwen2:1.5b", "bf16"),
         "llama-q4_k": ("tiny-llama3.1:8b", "tiny-mistral:7b", "q4_k")}


def _engine(target, draft, dtype="bf16", K=3, **kw):
    kw = dict(dict(device=DEV, max_batch=4, max_context=T_MAX, keep_natural=True, seed=13, steps_per_graph=4,
                   weight_dtype=dtype), **kw)
    return DecodeEngine(target, speculative=K, draft_model=draft, **kw)


# ------------------------------------------------------------------------------------------ kernels
def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert np.array_equal(got, want), (what, got.tolist(), want.tolist())


@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("R", [1, 3])
def test_kernels_match_the_rule(K, R):
    rng = np.random.default_rng(1000 * K + R)
    seqs = tsg._sequences()
    seqs += seqs[: (-len(seqs)) % R]
    slots = R + 2
    for g in range(0, len(seqs), R):
        group = seqs[g: g + R]
        spec = ops.spec_alloc(R, K, slots, T_MAX, V, DEV)
        sd = ops.spec_draft_alloc(spec, DV, DBOS)
        use = rng.permutation(slots)[:R]  # rows do not sit in their own slot
        state = dict(tok=[], pos=[], slot=[], n_gen=[], max_new=[], done=[], hist=rng.integers(0, V, (R, 64)))
        seq = rng.integers(0, 10, (slots, T_MAX))
        dvalid = rng.integers(0, T_MAX, slots)
        opts = []
        for r, (rec, pos, ng, mn, dn, masked) in enumerate(group):
            seq[use[r], : pos + 1] = rec
            dvalid[use[r]] = pos - (g // R + r) % 2  # dvalid == pos and dvalid == pos - 1, in turn
            for k, v in zip(("tok", "pos", "slot", "n_gen", "max_new", "done"),
                            (rec[pos], pos, -1 if masked else use[r], ng, mn, dn)):
                state[k].append(v)
            opts.append(dict(tsg.GREEDY, temperature=0.5 + r, top_k=7 + r, seed=1000 + r, eos_id=3 + r, stop=(r, 2 * r)))
        params = ops.sample_params_tensor(opts, DEV)
        spec["seq"].copy_(torch.tensor(seq, dtype=torch.int32))
        spec["given"].copy_(torch.tensor(rng.integers(0, V, (R, T_MAX)), dtype=torch.int32))
        sd["dvalid"].copy_(torch.tensor(dvalid, dtype=torch.int32))
        for k in ("p0", "nd", *ops._SPECD_ROWS, "r_hist"):
            sd[k].fill_(-7)  # (an entry the kernel leaves out shows)
        rows = tsg.dev_rows(state)
        # ---- the rows of the first draft forward
        want = ops.spec_model_rows_ref(rows, params, sd, R, T_MAX)
        ops.spec_model_rows(rows, params, sd, R, T_MAX)
        torch.cuda.synchronize()
        for k, w in want.items():
            got = sd[k].cpu().numpy()
            _same(got.reshape(-1, ops.SAMPLE_BYTES) if k == "r_params" else got, w, (k, g))
        assert int(sd["r_pos"].max()) < T_MAX
        for r, (rec, pos, ng, mn, dn, masked) in enumerate(group):  # the rule itself, spelled out once more
            d = 0 if dn or masked else sp.clip(K, pos, ng, K, T_MAX, mn)
            assert want["nd"][r] == d
            assert (want["r_slot"][R + r] >= 0) == (d > 0 and pos >= 1 and dvalid[use[r]] == pos - 1)
            if d > 0:
                assert want["r_tok"][r] == (rec[pos] if rec[pos] < DV else DBOS) and want["r_done"][r] == 0
        # ---- forwards 2 .. K: the sampler's output stands in row r (ids >= DV among them), the next kernel follows
        for j in range(1, K + 1):
            sd["r_tok"][:R].copy_(torch.tensor(rng.integers(0, 6, R), dtype=torch.int32))
            want = ops.spec_model_next_ref(rows, sd, R, j)
            ops.spec_model_next(rows, sd, R, j, T_MAX)
            torch.cuda.synchronize()
            for k, w in want.items():
                _same(sd[k][:R] if k != "given" else sd[k], w, (k, g, j))
            assert int(sd["r_pos"].max()) < T_MAX
        nd, given = sd["nd"].cpu().numpy(), sd["given"].cpu().numpy()
        for r, (rec, pos, ng, mn, dn, masked) in enumerate(group):
            assert int(sd["r_slot"][r]) == -1  # every row is masked once its last forward ran
            if not dn and not masked:  # what given mode reads back is the d tokens, ended
                assert len(sp.given_draft(given[r], ng, K)) >= nd[r] and (nd[r] == K or given[r, ng + nd[r]] == -1)
        # ---- after accept: the sequences moved by 1 .. d + 1 tokens
        moved = {k: v.clone() for k, v in rows.items()}
        moved["pos"] += torch.tensor([int(rng.integers(1, n + 2)) for n in nd], dtype=torch.int32, device=DEV)
        want = ops.spec_dvalid_ref(moved, sd, R)
        ops.spec_dvalid(moved, sd, R, T_MAX)
        torch.cuda.synchronize()
        _same(sd["dvalid"], want, ("dvalid", g))


# ------------------------------------------------------------------------------------------ engines
@pytest.mark.parametrize("K", [3, 7])
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_engine_tokens_are_the_engine_without_a_draft_model(pair, K):
    target, draft, dtype = PAIRS[pair]
    n = 48
    eng = _engine(target, draft, dtype, K)
    base = DecodeEngine(target, device=DEV, max_batch=4, max_context=T_MAX, seed=13, steps_per_graph=4,
                        weight_dtype=dtype, weights=eng.weights, keep_natural=True, speculative=K)
    assert eng.max_batch == base.max_batch and eng.draft.max_batch == eng.max_batch and eng.draft.T_max == T_MAX
    for opts in (GREEDY, SEEDED):
        want = base.generate(PROMPTS, n, [opts] * 3)
        got = eng.generate(PROMPTS, n, [opts] * 3)
        eager = eng.generate(PROMPTS, n, [opts] * 3, use_graph=False)
        for w, r, e in zip(want, got, eager):
            assert r.tokens == w.tokens and len(r.tokens) == n
            assert r.eval_count == sum(r.step_tokens) and r.decode_steps == len(r.step_tokens)
            assert 0 <= r.draft_accepted <= r.draft_count
            assert e.tokens == r.tokens and e.step_tokens == r.step_tokens  # the eager path runs the same steps
        print(f"{pair} K={K}: steps {[r.decode_steps for r in got]} accepted "
              f"{[r.draft_accepted for r in got]} of {[r.draft_count for r in got]}")
    assert all(isinstance(k[3], str) and k[3] == "draft" for k in eng._graphs if "spec" in k)
    eng.close()
    base.close()


@pytest.mark.parametrize("K", [3, 7])
def test_self_draft_accepts_inside_the_tie_free_prefix(K):
    name, n = "tiny-llama3.1:8b", 48
    kw = dict(device=DEV, max_batch=1, max_context=T_MAX, keep_natural=True, seed=13, steps_per_graph=4)
    plain = DecodeEngine(name, **kw)
    base = plain.generate(PROMPTS[:1], n, [GREEDY])[0]
    prefix = tsg._first_near_tie(ReferenceModel(plain.weights), base.prompt_tokens, base.tokens)
    eng = DecodeEngine(name, weights=plain.weights, speculative=K, draft_model=plain.weights, **kw)
    r = eng.generate(PROMPTS[:1], n, [GREEDY])[0]
    assert r.eval_count == n == sum(r.step_tokens) and r.tokens[:prefix] == base.tokens[:prefix]
    at = 0
    for got in r.step_tokens:
        if at + K + 1 > prefix:
            break
        assert got == min(K + 1, n - at), (at, prefix, r.step_tokens)
        at += got
    print(f"self-draft K={K}: prefix {prefix}, steps {r.decode_steps}, accepted {r.draft_accepted}/{r.draft_count}")
    assert at > 0 or prefix < K + 1
    plain.close()
    eng.close()


def test_both_caches_hold_the_records():
    target, draft, n, K = "tiny-qwen2:7b", "tiny-qwen2:1.5b", 48, 3
    eng = _engine(target, draft, "bf16", K)
    es.poison(eng)
    es.poison(eng.draft)
    res = eng.generate(PROMPTS, n, [GREEDY] * 3)
    eng.stream.synchronize()
    dvalid = eng._spec_draft_bufs()["dvalid"].cpu().tolist()
    pos = eng.rows["pos"][:3].cpu().tolist()
    rec = eng._spec_bufs()["seq"].cpu().tolist()
    rows_t, rows_d = {}, {}
    for i, r in enumerate(res):
        assert len(r.tokens) == n and pos[i] == len(r.prompt_tokens) + n - 2
        full = list(r.prompt_tokens) + list(r.tokens)
        assert rec[i][: pos[i] + 1] == full[: pos[i] + 1]
        assert len(r.prompt_tokens) - 1 <= dvalid[i] <= pos[i]
        rows_t[i] = full[: len(r.prompt_tokens) + n - 2]  # positions < final pos
        rows_d[i] = full[: dvalid[i]]
    for e, rows, tag in ((eng, rows_t, "target"), (eng.draft, rows_d, "draft")):
        models = es.models_for(e.weights, es.Case(tag, e.cfg.name, (), ()))
        want, limit, _ = es.expectations(models, rows, e.max_batch)
        got = es.read_kv(e)
        es.compare(got[:2], want, limit, tag=f"draft-model-{tag}")
        # beyond pos + K of a used slot, and the unused slot, the sentinel stands bit for bit
        written = torch.zeros(e.max_batch, T_MAX, dtype=torch.bool)
        for i in range(3):
            written[i, : pos[i] + K + 1] = True
        es.assert_untouched(got[2:], written, tag=f"draft-model-{tag}")
    eng.close()


def _schedule(eng):
    """tests/test_spec_gpu.py test_continuous_batch's schedule: three requests, one admitted later, a short one retired
    while the others decode.  Returns the tokens and the step counts per request."""
    cb = eng.continuous()
    budget = {0: 40, 1: 6, 2: 30}
    prompts = {i: eng.encode(PROMPTS[i]) for i in range(3)}
    live = dict(zip(cb.admit([prompts[0], prompts[1]], [budget[0], budget[1]], [GREEDY] * 2), (0, 1)))
    out, stats, admitted_late, rounds = {i: [] for i in range(3)}, {}, False, 0
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
            moves = cb.retire(done_rows)
            live = {moves.get(row, row): i for row, i in live.items() if row not in done_rows}
        if not admitted_late and rounds == 2:
            live[cb.admit([prompts[2]], [budget[2]], [GREEDY])[0]] = 2
            admitted_late = True
    for i in range(3):
        assert len(out[i]) == budget[i] == sum(stats[i]["step_tokens"])
    return out, stats


def test_continuous_batch():
    eng = _engine("tiny-qwen2:7b", "tiny-qwen2:1.5b")
    base = DecodeEngine("tiny-qwen2:7b", device=DEV, max_batch=4, max_context=T_MAX, seed=13, steps_per_graph=4,
                        weights=eng.weights, keep_natural=True, speculative=3)
    want, _ = _schedule(base)
    got, stats = _schedule(eng)
    assert got == want
    assert all(s["draft_count"] > 0 for s in stats.values())
    eng.close()
    base.close()


def test_context_end():
    """A prompt of T_max - 3 tokens with K = 7: the row ends at T_max, neither cache is written outside slot 0 and no
    draft row stands at or past T_max."""
    eng = _engine("tiny-qwen2:7b", "tiny-qwen2:1.5b", K=7, max_batch=3, keep_natural=False)
    es.poison(eng)
    es.poison(eng.draft)
    prompt = es.prompt_ids(T_MAX - 3, eng.cfg.vocab, 11)
    r = eng.generate([prompt], 100, [GREEDY])[0]
    assert r.eval_count == 3 and r.done_reason == "length" and sum(r.step_tokens) == 3
    assert int(eng.rows["done"][0]) == 1 and int(eng.rows["pos"][0]) == T_MAX - 2
    assert r.draft_count <= 3  # d = 2 at the first step, at most 1 at a second
    sd = eng._spec_draft_bufs()
    assert int(sd["r_pos"].max()) < T_MAX - 1 and int(sd["dvalid"][0]) <= T_MAX - 2
    written = torch.zeros(eng.max_batch, T_MAX, dtype=torch.bool)
    written[0] = True  # slot 0 may hold anything; slots 1 and 2 keep every sentinel
    for e in (eng, eng.draft):
        es.assert_untouched(es.read_kv(e)[2:], written, tag=f"context-end-{e.cfg.name}")
    eng.close()


def test_entries_refuse_bad_arguments():
    eng = _engine("tiny-llama3.1:8b", "tiny-mistral:7b", K=1, max_batch=2, keep_natural=False,
                  draft_weight_dtype="q4_k")
    small = DecodeEngine("tiny-mistral:7b", device=DEV, max_batch=2, max_context=128, weight_dtype="q4_k")
    lib = ops.load()
    ok = eng._step(2, eng.rows, True, True, spec_mode=0)  # the engine's own record of a step over 2 sequences
    plan, d2, d1 = ok.plan, ok.draft2, ok.draft1
    rs, s, sd = ok.keep[0], ok.keep[4], ok.keep[5]
    stream = ctypes.c_void_p(eng.stream.cuda_stream)
    err = ctypes.c_int(0)
    bufs = eng._spec_draft_bufs()
    bufs["nd"].fill_(-7)

    def both(plan, d2, d1, R, s, sd, rs=rs):
        step = ops.CainStep(plan=plan, draft2=d2, draft1=d1, rows=ctypes.pointer(rs), spec=ctypes.pointer(s),
                            spec_draft=ctypes.pointer(sd), M=R, want_logits=1, want_sample=1)
        rc = lib.cain_step_run(ctypes.byref(step), stream)
        g = lib.cain_step_capture(ctypes.byref(step), 1, stream, ctypes.byref(err))
        return rc, g, err.value

    bad = ops.spec_struct(eng._spec_bufs(), 1)
    bad.K = 8
    bad_sd = ops.spec_draft_struct(bufs)
    bad_sd.K = 8
    assert both(plan, d2, d1, 2, bad, bad_sd) == (-1, None, -1)
    assert both(plan, d2, d1, 0, s, sd) == (-1, None, -1)
    p128 = small._plan(4)
    assert both(plan, p128, p128, 2, s, sd) == (-1, None, -1)  # plans of different T_max
    assert both(plan, d2, d1, 2, ops.spec_struct(eng._spec_bufs(), 0), sd) == (-1, None, -1)  # not given mode
    null = ops.spec_draft_struct(bufs)
    null.dvalid = None
    assert both(plan, d2, d1, 2, s, null) == (-1, None, -1)
    # 2 R above the rows of the draft plan: a bf16 target takes 33 x 2 rows, a q4_k draft plan 64
    wide = DecodeEngine("tiny-llama3.1:8b", device=DEV, max_batch=64, max_context=T_MAX, speculative=1)
    spec33 = ops.spec_alloc(40, 1, 2, T_MAX, wide.cfg.vocab, DEV)
    sd33 = ops.spec_draft_alloc(spec33, eng.draft.cfg.vocab, eng.draft.cfg.bos_id)
    rs_w = wide._rows_struct(wide.rows, True)
    assert eng.draft.weight_dtype == "q4_k" and eng.draft.row_cap == 64
    assert both(wide._plan(66), d2, d1, 33, ops.spec_struct(spec33, 1), ops.spec_draft_struct(sd33), rs_w) == \
        (-1, None, -1)
    torch.cuda.synchronize()
    assert bufs["nd"].cpu().tolist() == [-7] * eng.max_batch  # nothing was launched
    # ... and the same arguments unchanged are accepted (the engine's own call)
    assert eng.generate(PROMPTS[:2], 6, [GREEDY] * 2)[0].eval_count == 6
    for e in (eng, small, wide):
        e.close()
