"""Host-side checks of ``tests/engine_state.py``: ``expected_inputs`` on idle and busy rows, the sentinel's magnitude,
the 0.25 cap on the limit of every case of ``tests/test_engine_state_gpu.py``, a table of planted state faults that
the per-position check must name -- and a control showing that the first three of them pass the criteria the engine
tests used until now (cos > 0.995 on the last logits, same greedy token)."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).parent))

import engine_state as es  # noqa: E402
from cain_amd.models import get_config, random_weights  # noqa: E402
from cain_amd.models.reference import ReferenceModel  # noqa: E402
from cain_amd.models.tokenizer import get_tokenizer  # noqa: E402


# ------------------------------------------------------------------------------------------- expected_inputs
def test_expected_inputs_busy_row():
    # L = 3, n = 4: positions 0 .. 5 hold the prompt and every generated token but the last
    assert es.expected_inputs([7, 8, 9], [20, 21, 22, 23], idled=False) == [7, 8, 9, 20, 21, 22]


def test_expected_inputs_idled_row():
    # the idle forwards rewrite p_last = 5 with the last token's K / V, in place of tokens[n-2]
    assert es.expected_inputs([7, 8, 9], [20, 21, 22, 23], idled=True) == [7, 8, 9, 20, 21, 23]


def test_expected_inputs_one_token():
    assert es.expected_inputs([7, 8, 9], [20], idled=False) == [7, 8, 9]
    assert es.expected_inputs([7, 8, 9], [20], idled=True) == [7, 8, 20]  # in place of the prompt's last token
    assert es.expected_inputs([7], [20], idled=True) == [20]
    assert es.expected_inputs([7, 8, 9], [], idled=False) == [7, 8, 9]  # last_logits: the whole prompt


def test_case_lengths():
    assert es.FULL.tokens_predicted() == (3, 1, 20) and es.FULL.written() == (255, 255, 23)
    assert es.STATIC[es.LLAMA].written() == (20, 4, 43)
    assert es.CHUNKED.written() == (70, 9, 1, 40)
    for c in es.ALL_CASES:
        assert len(c.lengths) <= c.max_batch and max(c.written()) < es.T_MAX, c.id
        assert [len(p) for p in c.prompts()] == list(c.lengths)
    assert len({c.id for c in es.ALL_CASES}) == len(es.ALL_CASES)


def test_sentinel_bits_are_finite_and_exact():
    assert int(es.sentinel_bits("bf16")) == 0x4640 and int(es.sentinel_bits("fp8")) == 0x76
    assert float(es.sentinel_bits("bf16").view(torch.bfloat16)) == es.SENTINEL["bf16"]
    assert float(es.sentinel_bits("fp8").view(torch.float8_e4m3fn).float()) == es.SENTINEL["fp8"]


# ------------------------------------------------------------------------------- the cap and the sentinel, per case
def _case_rows(case):
    """{slot: tokens at positions 0 .. p_last}: the case's prompts, continued by fixed ids of the generated length
    (the limits' dependence on which tokens follow is what the 3 x margin is for)."""
    vocab = case.config().vocab
    return {i: p + es.prompt_ids(w - len(p), vocab, 1000 + i) for i, (p, w) in enumerate(zip(case.prompts(),
                                                                                               case.written()))}


@pytest.mark.parametrize("case", es.ALL_CASES, ids=[c.id for c in es.ALL_CASES])
def test_limit_is_under_the_cap_and_sentinel_is_large(case):
    """3 x the eager baseline's largest per-vector error stays <= 0.25 in every layer, for K and V, and the sentinel
    is >= 100 x the largest |K| or |V| the oracle produces."""
    torch.manual_seed(0)
    w = random_weights(case.config(), device="cpu", seed=case.seed)
    models = es.models_for(w, case)
    rows = _case_rows(case)
    n_prefill = {i: L - 1 for i, L in enumerate(case.lengths)}
    want, lim, base = es.expectations(models, rows, len(rows), n_prefill, case.compare_layers)
    for what, m in zip("KV", base):
        for l, x in enumerate(m):
            assert es.MARGIN * x <= es.CAP, (case.id, what, l, x)
    big = max(float((want.K.abs() * want.written[None, :, None, :, None]).max()),
              float((want.V.abs() * want.written[None, :, None, :, None]).max()))
    print(f"{case.id}: baseline max K {base[0]} V {base[1]}; largest |K|, |V| {big:.3f}")
    assert es.SENTINEL[case.kv_dtype] >= 100.0 * big, (case.id, big)


# ------------------------------------------------------------------------------------------- planted faults
# an emulated cache: the oracle's K / V rounded to bf16 where the rows wrote, the sentinel elsewhere.  Four kv heads
# (tiny-phi3) so a wrong-head fault exists; slot 2 is a full row (p_last = T_max - 2), slot 3 was never used.
EMU_MODEL = "tiny-phi3:3.8b"
EMU_LEN = {0: 43, 1: 12, 2: es.T_MAX - 1}
SLOTS = 4


@pytest.fixture(scope="module")
def emu():
    cfg = get_config(EMU_MODEL)
    w = random_weights(cfg, device="cpu", seed=5)
    case = es.Case("emu", EMU_MODEL, tuple(EMU_LEN.values()), (0, 0, 0))
    models = es.models_for(w, case)
    rows = {s: es.prompt_ids(n, cfg.vocab, 70 + s) for s, n in EMU_LEN.items()}
    want, lim, _ = es.expectations(models, rows, SLOTS)
    other = es.oracle_kv(models[0], es.prompt_ids(64, cfg.vocab, 99))  # the slot's previous occupant
    sent = es.SENTINEL["bf16"]
    wr = want.written[None, :, None, :, None]
    K = torch.where(wr, want.K, torch.tensor(sent)).bfloat16()
    V = torch.where(wr, want.V, torch.tensor(sent)).bfloat16()
    return dict(cfg=cfg, ref=models[0], rows=rows, want=want, lim=lim, K=K, V=V, other=other)


def _check(emu, K, V):
    """(vectors over the limit, first untouched violation) of an emulated cache."""
    bad = es.find_bad((K.float(), V.float()), emu["want"], emu["lim"])
    hit = es.find_touched((K.view(torch.int16), V.view(torch.int16)), emu["want"].written, es.sentinel_bits("bf16"))
    return bad, hit


def test_clean_emulated_cache_passes(emu):
    bad, hit = _check(emu, emu["K"], emu["V"])
    assert bad == [] and hit is None
    es.compare((emu["K"].float(), emu["V"].float()), emu["want"], emu["lim"])
    es.assert_untouched((emu["K"].view(torch.int16), emu["V"].view(torch.int16)), emu["want"].written)
    assert all(0 < x <= es.CAP for m in emu["lim"] for x in m)


def _never_written(e, K, V):
    K[:, 0, :, 17], V[:, 0, :, 17] = es.SENTINEL["bf16"], es.SENTINEL["bf16"]
    return ("K", 0, 0, 0, 17), None


def _swapped(e, K, V):
    for t in (K, V):
        a = t[:, 0, :, 9].clone()
        t[:, 0, :, 9] = t[:, 0, :, 30]
        t[:, 0, :, 30] = a
    return ("K", 0, 0, 0, 9), None


def _previous_occupant(e, K, V):
    for l, (k, v) in enumerate(e["other"]):
        K[l, 1, :, 5], V[l, 1, :, 5] = k[5].bfloat16(), v[5].bfloat16()
    return ("K", 0, 1, 0, 5), None


def _slot_plus_one(e, K, V):
    # slot 0's position 40 went to slot 1, which is past slot 1's own length
    K[:, 1, :, 40], V[:, 1, :, 40] = K[:, 0, :, 40].clone(), V[:, 0, :, 40].clone()
    K[:, 0, :, 40], V[:, 0, :, 40] = es.SENTINEL["bf16"], es.SENTINEL["bf16"]
    return ("K", 0, 0, 0, 40), ("K", 0, 1, 0, 40)


def _past_the_end(e, K, V):
    K[:, 1, :, 12], V[:, 1, :, 12] = K[:, 1, :, 11].clone(), V[:, 1, :, 11].clone()
    return None, ("K", 0, 1, 0, 12)


def _last_position_of_full_row(e, K, V):
    K[1, 2, 3, es.T_MAX - 1] = K[1, 2, 3, es.T_MAX - 2].clone()
    return None, ("K", 1, 2, 3, es.T_MAX - 1)


def _wrong_kv_head(e, K, V):
    V[1, 0, 2, 21] = V[1, 0, 3, 21].clone()
    return ("V", 1, 0, 2, 21), None


def _no_rope(e, K, V):
    # layer 0's K depends on the token alone: the same forward at position 0 is K before RoPE
    ids = torch.tensor([e["rows"][0]])
    c: list = []
    e["ref"].forward(ids, positions=torch.zeros_like(ids), cache=c)
    K[0, 0, :, 17] = c[0][0][0, 17].bfloat16()
    return ("K", 0, 0, 0, 17), None


FAULTS = [_never_written, _swapped, _previous_occupant, _slot_plus_one, _past_the_end, _last_position_of_full_row,
          _wrong_kv_head, _no_rope]


@pytest.mark.parametrize("fault", FAULTS, ids=[f.__name__.strip("_") for f in FAULTS])
def test_planted_fault_is_named(emu, fault):
    K, V = emu["K"].clone(), emu["V"].clone()
    first_bad, first_hit = fault(emu, K, V)
    bad, hit = _check(emu, K, V)
    if first_bad is None:
        assert bad == []
    else:
        assert bad and bad[0][:5] == first_bad, bad[:3]
        assert all(b[5] > 0.5 for b in bad), bad[:3]  # order 1 or above, never marginal
        with pytest.raises(AssertionError, match=r"first \('%s', %d, %d, %d, %d," % first_bad):
            es.compare((K.float(), V.float()), emu["want"], emu["lim"], "emu")
    assert hit == first_hit
    if first_hit is not None:
        with pytest.raises(AssertionError, match=r"first at \('%s', %d, %d, %d, %d\)" % first_hit):
            es.assert_untouched((K.view(torch.int16), V.view(torch.int16)), emu["want"].written, tag="emu")


def test_snapshot_slots_are_held_to_the_snapshot(emu):
    """A reused slot past its new row's length must equal what its previous occupant left, not the sentinel."""
    K, V = emu["K"].clone(), emu["V"].clone()
    snap = (K.view(torch.int16).clone(), V.view(torch.int16).clone())
    written = emu["want"].written.clone()
    written[0, 8:] = False  # slot 0 reused by a row of 8 positions
    bits = (K.view(torch.int16), V.view(torch.int16))
    assert es.find_touched(bits, written, es.sentinel_bits("bf16")) == ("K", 0, 0, 0, 8)
    assert es.find_touched(bits, written, es.sentinel_bits("bf16"), snap, (0,)) is None
    V[1, 0, 1, 20, 3] = 0.5
    assert es.find_touched(bits, written, es.sentinel_bits("bf16"), snap, (0,)) == ("V", 1, 0, 1, 20)


# ------------------------------------------------------------------------------------------- the gap, demonstrated
PROMPTS = ["In 100 words, please give me information about India",
           "In 500 words, please give me information about Elizabeth II, Queen of the United Kingdom and more",
           " ".join(f"word{i}" for i in range(160))]
# the one (fault, prompt) pair the old cosine does notice: a zeroed position among 16 (cos 0.9913; 0.9976 among 29)
SEEN_BY_COSINE = {("never_written", 0)}


@pytest.mark.parametrize("fault", ["never_written", "swapped", "previous_occupant"])
def test_old_criterion_passes_a_state_fault(fault):
    """The criteria of test_engine_gpu.py (cos > 0.995 on the last logits, same greedy token) do not see a missing
    (zero, as the engine's caches start), swapped or stale KV position: planted into the oracle's cache before the
    last token's forward, on the prompts of that file that are long enough to hold them (17, 30 and 321 ids; "hi"
    has 2).  Only the zeroed position of the 17-id prompt drops the cosine below 0.995; its greedy token stays."""
    cfg = get_config(es.LLAMA)
    ref = ReferenceModel(random_weights(cfg, device="cpu", seed=3))
    tok = get_tokenizer(cfg)
    seqs = [tok.encode(p) for p in PROMPTS]
    for i, ids in enumerate(seqs):
        assert len(ids) > 12
        c: list = []
        ref.forward(torch.tensor([ids[:-1]]), cache=c)
        stale: list = []
        ref.forward(torch.tensor([seqs[0 if i == 1 else 1][:-1]]), cache=stale)
        bad = [[k.clone(), v.clone()] for k, v in c]
        for l, (k, v) in enumerate(bad):
            if fault == "never_written":
                k[0, 5], v[0, 5] = 0.0, 0.0
            elif fault == "swapped":
                for t, o in ((k, c[l][0]), (v, c[l][1])):
                    t[0, 3], t[0, 9] = o[0, 9], o[0, 3]
            else:
                k[0, 5], v[0, 5] = stale[l][0][0, 5], stale[l][1][0, 5]
        last = torch.tensor([ids[-1:]])
        clean = ref.forward(last, cache=[[k.clone(), v.clone()] for k, v in c])[0, -1]
        got = ref.forward(last, cache=bad)[0, -1]
        assert not torch.equal(got, clean)  # the fault is in the logits, far below the criterion
        cos = float(torch.nn.functional.cosine_similarity(got, clean, dim=0))
        print(f"{fault}: prompt {i} ({len(ids)} ids) cos {cos:.6f}")
        assert int(got.argmax()) == int(clean.argmax()), (fault, i)
        assert cos > 0.995 or (fault, i) in SEEN_BY_COSINE, (fault, i, cos)
