"""Speculative decoding on the host (no GPU): the rule of engine/speculative.py on hand-written sequences, and the
torch backend decoding with it -- the tokens are plain decoding's."""
import pytest

from cain_amd.engine import speculative as sp
from cain_amd.engine.engine import DecodeEngine

T = 64  # context of the hand-written cases


def d(seq, K=3, ng=0, max_new=100, T_max=T, **kw):
    return sp.draft(seq, len(seq) - 1, ng, K, T_max, max_new, **kw)


# ---------------------------------------------------------------- draft
def test_no_match():
    assert d([1, 2, 3, 4, 5]) == []
    assert d([7]) == []  # pos 0: nothing before the token


def test_match_at_three():
    #    0  1  2  3  4  5  6  7  8
    s = [9, 1, 2, 3, 7, 8, 1, 2, 3]  # suffix (1 2 3) ends at i = 3: drafts seq[4 .. 6]
    assert d(s) == [7, 8, 1]
    assert d(s, K=1) == [7]
    assert d(s, K=7) == [7, 8, 1, 2, 3]  # stops at pos: seq[4 .. min(3 + 7, 8)]


def test_fallback_to_two_and_one():
    assert d([5, 2, 3, 6, 4, 2, 3]) == [6, 4, 2]  # (4 2 3) never occurred, (2 3) ends at 2
    assert d([5, 3, 6, 4, 2, 3]) == [6, 4, 2]     # (2 3) never occurred, (3) at 1
    assert sp.ngram_draft([5, 3, 6, 4, 2, 3], 5, 2) == [6, 4]


def test_most_recent_match_wins():
    #    0  1  2  3  4  5  6  7  8  9 10
    s = [1, 2, 3, 4, 1, 2, 3, 5, 1, 2, 3]
    assert d(s) == [5, 1, 2]  # i = 6, not i = 2
    # a longer n-gram wins over a more recent shorter one
    s = [1, 2, 3, 4, 9, 3, 6, 1, 2, 3]
    assert d(s) == [4, 9, 3]


def test_match_ending_just_before_pos_gives_one():
    assert d([4, 4]) == [4]          # n = 1 at i = 0 = pos - 1
    assert d([1, 7, 7, 7, 7]) == [7]  # n = 3 at i = 3 = pos - 1: seq[4 .. 4]


def test_pos_smaller_than_n():
    assert d([3, 3, 3]) == [3]  # pos = 2: n = 3 skipped, n = 2 matches at i = 1
    assert sp.ngram_draft([3, 5, 3], 2, 3) == [5, 3]  # n = 3 and (5 3) skipped / absent; n = 1 at i = 0


def test_clipping():
    s = [1, 2, 3, 4, 5, 6, 1, 2, 3]
    assert d(s, K=3) == [4, 5, 6]
    assert d(s, K=3, T_max=len(s) + 2) == [4, 5]  # pos + d <= T_max - 1
    assert d(s, K=3, T_max=len(s) + 1) == [4]
    assert d(s, K=3, T_max=len(s)) == []
    assert d(s, K=3, ng=5, max_new=8) == [4, 5]   # ng + d <= max_new - 1
    assert d(s, K=3, ng=7, max_new=8) == []
    assert sp.clip(3, 10, 0, 3, 64, 100) == 3


def test_done_and_masked_draft_nothing():
    s = [1, 2, 3, 4, 1, 2, 3]
    assert d(s) == [4, 1, 2]
    assert d(s, done=True) == []
    assert d(s, slot=-1) == []


def test_given_mode():
    s = [1, 2, 3, 4, 1, 2, 3]
    g = [10, 11, 12, 13, -1, 15, 16]
    assert d(s, given=g) == [10, 11, 12]
    assert d(s, given=g, ng=2) == [12, 13]   # -1 ends the draft
    assert d(s, given=g, ng=4) == []
    assert d(s, given=g, ng=5, vocab=16) == [15]
    assert d(s, given=g, ng=1, max_new=3) == [11]
    assert d(s, given=[], ng=0) == []


def test_draft_ring():
    ring = list(range(100, 164))
    assert sp.draft_ring(ring, 5, [7, 8, 9], 0) == ring
    r2 = sp.draft_ring(ring, 62, [7, 8, 9], 3)  # wraps: indices 62, 63, 0
    assert (r2[62], r2[63], r2[0]) == (7, 8, 9) and r2[1:62] == ring[1:62]
    assert sp.draft_ring(ring, 62, [7, 8, 9], 1)[63] == ring[63]


# ---------------------------------------------------------------- accept
def state(**kw):
    base = dict(tok=3, pos=6, max_new=50, seq=[1, 2, 3, 4, 1, 2, 3])
    base.update(kw)
    return sp.SeqState(**base)


def test_accept_all():
    st = state()
    assert st.commit_step([4, 1, 2], [4, 1, 2, 9], T) == 4
    assert st.gen == [4, 1, 2, 9] and (st.tok, st.pos, st.n_gen, st.done) == (9, 10, 4, False)
    assert st.seq == [1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 9] and st.seq[st.pos] == st.tok
    assert st.hist[:4] == [4, 1, 2, 9] and (st.drafted, st.accepted, st.step_tokens) == (3, 3, [4])


def test_reject_at_zero_and_in_the_middle():
    st = state()
    assert st.commit_step([4, 1, 2], [8, 1, 2, 9], T) == 1  # row 0 drew 8, not draft 1
    assert st.gen == [8] and (st.tok, st.pos, st.drafted, st.accepted) == (8, 7, 3, 0)
    st = state()
    assert st.commit_step([4, 1, 2], [4, 7, 2, 9], T) == 2  # draft 2 wrong: t_0, t_1 stay
    assert st.gen == [4, 7] and (st.tok, st.pos, st.accepted) == (7, 8, 1)
    assert sp.accepted_length([4, 1, 2], [4, 1, 5, 2]) == 2
    st = state()
    assert st.commit_step([], [5], T) == 1 and st.gen == [5]  # no drafts: plain decode


def test_stop_id_inside_an_accepted_run():
    st = state(eos_id=1)
    assert st.commit_step([4, 1, 2], [4, 1, 2, 9], T) == 2
    assert st.gen == [4, 1] and st.done and st.pos == 7 and st.tok == 1  # (a done row keeps its position)
    assert st.accepted == 1 and st.commit_step([2], [2, 9], T) == 0 and st.gen == [4, 1]
    st = state(stop=(-1, 2, -1))
    assert st.commit_step([4, 1, 2], [4, 1, 2, 9], T) == 3 and st.done


def test_budget_and_context_end_the_run():
    st = state(max_new=2)
    assert st.commit_step([4, 1, 2], [4, 1, 2, 9], T) == 2 and st.done and st.n_gen == 2
    st = state()
    # T_max = 8: 4 goes to position 7, the last one; 9 (drawn there) ends the sequence as plain decode's token does
    assert st.commit_step([4], [4, 9], 8) == 2 and st.done and st.pos == 7 and st.gen == [4, 9]
    assert st.seq == [1, 2, 3, 4, 1, 2, 3, 4]
    st = state()
    assert st.commit_step([], [4], 7) == 1 and st.done and st.pos == 6 and st.seq == [1, 2, 3, 4, 1, 2, 3]


# ---------------------------------------------------------------- the torch backend
PROMPTS = [[1, 2, 3, 4, 5, 2, 3, 4], [9, 8, 7, 9, 8]]
N = 24


@pytest.fixture(scope="module", params=["tiny-llama3.1:8b", "tiny-qwen2:1.5b"])
def engines(request):
    kw = dict(device="cpu", max_context=128, max_batch=2)
    return DecodeEngine(request.param, **kw), DecodeEngine(request.param, speculative=3, **kw)


@pytest.mark.parametrize("opts", [dict(temperature=0.0, eos_id=-1), dict(temperature=0.8, seed=11, eos_id=-1)],
                         ids=["greedy", "seeded"])
def test_torch_backend_tokens_equal_plain(engines, opts):
    plain, spec = engines
    a = plain.generate(PROMPTS, N, opts)
    b = spec.generate(PROMPTS, N, opts)
    c = spec.generate(PROMPTS, N, opts, drafts=[r.tokens for r in a])
    for ra, rb, rc in zip(a, b, c):
        assert ra.draft_count is None and ra.decode_steps is None and "draft_count" not in ra.ollama_json()
        assert rb.tokens == ra.tokens and rc.tokens == ra.tokens
        for r in (rb, rc):
            assert sum(r.step_tokens) == r.eval_count == N and r.decode_steps == len(r.step_tokens)
            assert r.draft_accepted == r.eval_count - r.decode_steps
            j = r.ollama_json()
            assert j["draft_count"] == r.draft_count and j["draft_accepted_count"] == r.draft_accepted
        # drafts = the plain run's own tokens: every draft is accepted, K + 1 tokens per step
        assert rc.decode_steps == N // 4 < rc.eval_count and rc.step_tokens == [4] * (N // 4)
        assert rc.draft_accepted == rc.draft_count == N - N // 4


def test_torch_backend_stop_id_and_partial_drafts(engines):
    plain, spec = engines
    ref = plain.generate(PROMPTS[:1], N, dict(temperature=0.0, eos_id=-1))[0].tokens
    stop = ref[9]
    first = ref.index(stop)
    a = plain.generate(PROMPTS[:1], N, dict(temperature=0.0, eos_id=stop))[0]
    wrong = [t if i % 5 else (t + 1) % 50 for i, t in enumerate(ref)]  # every 5th draft is not the token
    b = spec.generate(PROMPTS[:1], N, dict(temperature=0.0, eos_id=stop), drafts=[wrong])[0]
    assert a.tokens == b.tokens == ref[:first + 1] and b.done_reason == a.done_reason == "stop"
    assert sum(b.step_tokens) == b.eval_count and max(b.step_tokens) <= 4
    c = spec.generate(PROMPTS[:1], N, dict(temperature=0.0, eos_id=-1), drafts=[None])[0]
    assert c.tokens == ref and c.draft_count == 0 and c.decode_steps == N


def test_refusals():
    with pytest.raises(ValueError, match="speculative"):
        DecodeEngine("tiny-qwen2:1.5b", device="cpu", speculative=8)
    with pytest.raises(ValueError, match="prefix_cache"):
        DecodeEngine("tiny-qwen2:1.5b", device="cpu", speculative=2, prefix_cache=True)
    eng = DecodeEngine("tiny-qwen2:1.5b", device="cpu", max_context=64, speculative=2)
    with pytest.raises(ValueError, match="logprobs"):
        eng.generate([[1, 2]], 4, logprobs=True)
    with pytest.raises(ValueError, match="drafts"):
        DecodeEngine("tiny-qwen2:1.5b", device="cpu", max_context=64).generate([[1, 2]], 4, drafts=[[1]])


def test_env_switch(monkeypatch):
    monkeypatch.setenv("CAIN_SPECULATIVE", "2")
    assert DecodeEngine("tiny-qwen2:1.5b", device="cpu", max_context=64).speculative == 2
    assert DecodeEngine("tiny-qwen2:1.5b", device="cpu", max_context=64, speculative=0).speculative == 0
    monkeypatch.delenv("CAIN_SPECULATIVE")
    assert DecodeEngine("tiny-qwen2:1.5b", device="cpu", max_context=64).speculative == 0
    from cain_amd.experiments.study import StudySettings

    monkeypatch.setenv("CAIN_STUDY_SPECULATIVE", "3")
    assert StudySettings().speculative == 0 and StudySettings.from_env().speculative == 3
