"""Stop sequences on the CPU: the Python rule against the brute-force definition, the C++ header against the Python
rule, option validation, the text cut on three kinds of tokenizer, and the torch backend end to end.

Reference: ``stopseq_cases.brute_force`` -- the definition of the stop computed with ``bytes.find`` over the whole
stream (smallest end offset, the token that holds it, the minimum start among the occurrences that end by that
token's last byte, the lowest index on ties).  It shares no code with the incremental rule.
"""
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

from cain_amd.engine import stopseq as ss
from stopseq_cases import all_cases, boundary_stop, brute_force, named_cases, random_cases

ROOT = Path(__file__).resolve().parent.parent
HEADER_DIR = ROOT / "cain_amd" / "ops" / "csrc"
HOST_SRC = ROOT / "tests" / "csrc" / "stop_match_host.cpp"


def check_case(stops, pieces, name=""):
    state, n = ss.run(pieces, stops)
    want = brute_force(stops, pieces)
    stream = b"".join(pieces)
    if want is None:
        assert n == len(pieces) and state[3:] == (-1, -1), (name, stops, pieces)
    else:
        assert (n, state[3], state[4]) == want, (name, stops, pieces, state, want)
        assert stream[state[3]:].startswith(stops[state[4]])
    assert state[1] == n and state[2] == len(b"".join(pieces[:n]))
    assert state[0] == (bytes(ss.TAIL) + b"".join(pieces[:n]))[-ss.TAIL:]
    return want


def test_named_cases_against_the_definition():
    got = {name: check_case(s, p, name) for name, s, p in named_cases()}
    assert got["self-overlap"] == (3, 1, 0)  # aab in aaab: the second a starts it
    assert got["prefix of another"] == (2, 1, 1)  # "ab" completes a token before "abcd" could
    assert got["prefix of another, one token"] == (2, 1, 0)  # both end in the token, equal starts: index 0
    assert got["suffix of another, one token"] == (2, 1, 1)  # "abc" starts before "bc"
    assert got["equal starts: the lowest index"] == (1, 1, 0)
    assert got["32 bytes, 32 one-byte tokens"] == (33, 1, 0)
    assert got["32 bytes, starts 31 back"] == (2, 2, 0)
    assert got["ends on the last byte of a token"] == (2, 4, 0)
    assert got["ends on the first byte of a token"] == (2, 4, 0)
    assert got["near miss"] is None and got["never"] is None
    assert got["empty pieces inside a match"] == (6, 0, 0)
    assert got["a long piece, the match past its 64th byte"] == (2, 71, 0)
    assert got["a long piece, two strings, the later end starts first"] == (2, 0, 1)


def test_random_cases_against_the_definition():
    cases = random_cases(seed=2025, n=4000)
    hits = sum(check_case(s, p) is not None for s, p in cases)
    assert 1000 < hits < 3800  # both outcomes are well represented
    assert sum(any(len(x) >= 70 for x in p) for _, p in cases) > 300


def test_states_round_trip():
    for stops, pieces in random_cases(seed=3, n=50):
        s = ss.INITIAL
        for p in pieces:
            s, _ = ss.advance(s, p, stops)
            b = ss.state_bytes(s)
            assert len(b) == ss.STATE_BYTES == 48 and ss.state_from_bytes(b) == s


# ---------------------------------------------------------------- the C++ header
def _build(tmp_path, flags, name):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / name
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, f"-I{HEADER_DIR}", str(HOST_SRC), "-o",
                        str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in " ".join(flags) and "cannot find" in r.stderr and "san" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                                              "-fno-sanitize-recover=all")], ids=["plain", "asan-ubsan"])
def test_header_on_the_host_equals_the_python_rule(tmp_path, flags):
    exe = _build(tmp_path, flags, "stop_match_host")
    cases = all_cases(seed=77, n=1500)
    u32 = lambda v: struct.pack("<I", v)  # noqa: E731
    blob = b"".join(u32(len(s)) + b"".join(u32(len(x)) + x for x in s) + u32(len(p)) +
                    b"".join(u32(len(x)) + x for x in p) for s, p in cases)
    r = subprocess.run([str(exe)], input=blob, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = iter(r.stdout.decode().split("\n"))
    for stops, pieces in cases:
        s, hit = ss.INITIAL, False
        for p in pieces:
            if hit:
                break
            s, hit = ss.advance(s, p, stops)
            assert next(lines) == f"{ss.state_bytes(s).hex()} {int(hit)}", (stops, pieces)
        assert next(lines) == "--"
    assert next(lines) == ""


# ---------------------------------------------------------------- options
def test_option_validation():
    assert ss.parse_stop(None) == () and ss.parse_stop([]) == ()
    assert ss.parse_stop("\n\n") == ("\n\n",) and ss.parse_stop(("a", "é" * 16)) == ("a", "é" * 16)
    assert len(ss.parse_stop(["x"] * 8)) == 8
    with pytest.raises(ValueError, match="stop_ids"):
        ss.parse_stop([1, 2])
    with pytest.raises(ValueError, match="stop_ids"):
        ss.parse_stop(7)
    with pytest.raises(ValueError, match="stop_ids"):
        ss.parse_stop(["ok", b"bytes"])
    with pytest.raises(ValueError, match="empty"):
        ss.parse_stop(["a", ""])
    with pytest.raises(ValueError, match="limit is 8"):
        ss.parse_stop(["x"] * 9)
    with pytest.raises(ValueError, match="33 bytes"):
        ss.parse_stop(["a" * 33])
    with pytest.raises(ValueError, match="34 bytes"):
        ss.parse_stop(["é" * 17])  # 17 characters, 34 bytes


@pytest.fixture(scope="module")
def engine():
    from cain_amd.engine.engine import DecodeEngine

    return DecodeEngine("tiny-llama3.1:8b", device="cpu", backend="torch", max_batch=4, max_context=256)


def test_engine_refusals(engine):
    from cain_amd.engine.engine import DecodeEngine

    for bad, match in (([3], "stop_ids"), ("", "empty"), (["x"] * 9, "limit is 8"), ("y" * 33, "33 bytes")):
        with pytest.raises(ValueError, match=match):
            engine.generate([[1, 5, 9]], 4, {"stop": bad})
    with pytest.raises(ValueError, match="33 bytes"):
        engine.generate([[1, 5, 9], [1, 6]], 4, [None, {"stop": ["fine", "y" * 33]}])  # one dict per row
    spec = DecodeEngine("tiny-llama3.1:8b", device="cpu", backend="torch", max_batch=2, max_context=128,
                        speculative=2)
    with pytest.raises(ValueError, match="speculative"):
        spec.generate([[1, 2, 3]], 4, {"stop": ["a"]})
    r = spec.generate([[1, 2, 3]], 4, {"stop_ids": [5], "eos_id": -1})[0]  # the ids are another option
    assert len(r.tokens) == 4 and r.stop_hit is None


# ---------------------------------------------------------------- the text cut
def test_text_cut_synthetic_tokenizer(engine):
    tok = engine.tokenizer
    pieces = engine._piece_vocab()
    assert pieces[:16] == [b""] * 16 and pieces[17] == tok.piece(17).encode()
    spaced = next(t for t in range(16, 400) if tok.piece(t).startswith(" "))
    bare = next(t for t in range(16, 400) if not tok.piece(t).startswith(" "))
    toks = [spaced, bare, 3, spaced, bare]  # (3: a special token, empty)
    raw = b"".join(pieces[t] for t in toks)
    full = tok.decode(toks)
    assert full == raw.decode().lstrip() and raw.startswith(b" ")
    for hit_start in range(len(raw) + 1):
        assert ss.cut_text(full, raw, hit_start) == raw[:hit_start].decode().lstrip(), hit_start
    assert ss.cut_text(full, raw, 0) == ""  # a hit inside the stripped leading space: floored at the empty string
    assert engine.stop_cut(toks, full, 3) == raw[:3].decode().lstrip()


def test_text_cut_byte_level_and_sentencepiece():
    from cain_amd.engine import jsonmode as jm

    inv = {b: ch for ch, b in jm._gpt2_byte_table().items()}

    class Tok:  # the calls token_bytes makes of a tokenizers.Tokenizer, and a decode of its kind
        def __init__(self, pieces, special=(), sp=False):
            self.pieces, self.special_ids, self.sp = pieces, special, sp

        def get_vocab_size(self):
            return len(self.pieces)

        def id_to_token(self, i):
            return self.pieces[i]

        def decode(self, ids):
            raw = b"".join(table[i] for i in ids)
            text = raw.decode("utf-8", "replace")
            return text[1:] if self.sp and text.startswith(" ") else text  # SentencePiece drops the word mark up front

    bl = Tok(["<|eot|>"] + ["".join(inv[b] for b in w) for w in (b" caf", b"\xc3", b"\xa9", b"!\n", b"\n", b" ok")],
             special=(0,))
    table = jm.token_bytes(bl, 7)
    assert table == [b"", b" caf", b"\xc3", b"\xa9", b"!\n", b"\n", b" ok"]
    toks = [1, 2, 3, 0, 4, 5, 6]
    raw = b"".join(table[t] for t in toks)
    state, n = ss.run([table[t] for t in toks], [b"\n\n"])
    assert (n, state[3]) == (6, 7) == brute_force([b"\n\n"], [table[t] for t in toks])[:2]
    assert ss.cut_text(bl.decode(toks[:n]), raw[:9], state[3]) == " café!" and raw[:9] == b" caf\xc3\xa9!\n\n"
    state, n = ss.run([table[t] for t in toks], ["é!".encode()])  # the string starts inside a character's bytes' token
    assert (n, state[3]) == (5, 4) and ss.cut_text(bl.decode(toks[:n]), b" caf\xc3\xa9!\n", 4) == " caf"
    # a cut inside a character (the string is its second byte's successor only): the half character decodes to U+FFFD
    assert ss.cut_text(" café!", b" caf\xc3\xa9!", 5) == " caf"

    sp = Tok(["<unk>", "<s>", "</s>", "▁Hi", "▁there", "<0x0A>", "<0xC3>", "<0xA9>", "."], sp=True)
    table = jm.token_bytes(sp, 9)
    assert table == [b"", b"", b"", b" Hi", b" there", b"\n", b"\xc3", b"\xa9", b"."]
    toks = [3, 4, 8, 5, 5, 3]
    pieces = [table[t] for t in toks]
    state, n = ss.run(pieces, [b".\n", b"\n\n"])
    assert (n, state[3], state[4]) == (4, 9, 0) == brute_force([b".\n", b"\n\n"], pieces)
    raw = b"".join(pieces[:n])
    assert sp.decode(toks[:n]) == "Hi there.\n" and ss.cut_text(sp.decode(toks[:n]), raw, state[3]) == "Hi there"
    state, n = ss.run(pieces, [b" Hi"])  # a hit inside the stripped leading space
    assert (n, state[3]) == (1, 0) and ss.cut_text(sp.decode(toks[:1]), b" Hi", 0) == ""


def test_held_back():
    assert ss.held_back("abc\n", ["\n\n"]) == 1 and ss.held_back("abc", ["\n\n"]) == 0
    assert ss.held_back("xxab", ["abc", "b!"]) == 2 and ss.held_back("xxab", ["b!", "abc"]) == 2
    assert ss.held_back("ab", ["ab"]) == 0 and ss.held_back("aba", ["ab"]) == 1  # proper prefixes only: the whole
    # string is the rule's to find
    assert ss.held_back(b"..\xc3", ["é".encode()]) == 1 and ss.held_back("", ["a"]) == 0


# ---------------------------------------------------------------- engine (torch backend)
@pytest.mark.parametrize("options", [dict(temperature=0.0), dict(temperature=0.9, seed=11)], ids=["greedy", "seeded"])
def test_engine_stops_inside_the_free_run(engine, options):
    opts = dict(options, eos_id=-1)
    prompt = [1, 40, 41, 42]
    free = engine.generate([prompt], 40, opts)[0]
    assert len(free.tokens) == 40 and free.done_reason == "length" and free.stop_hit is None
    pieces = engine._piece_vocab()
    found = boundary_stop([pieces[t] for t in free.tokens])
    assert found is not None, free.tokens
    st, n_tok, hit_start = found
    stop = st.decode()
    assert (n_tok - 1) % 8 != 0  # the final token's generated index: inside a decode graph, not at its end
    r = engine.generate([prompt], 40, dict(opts, stop=["\x00never", stop]))[0]
    print("free:", repr(free.text), "stop:", repr(stop), "got:", repr(r.text), len(r.tokens))
    assert r.tokens == free.tokens[:n_tok]
    assert r.done_reason == "stop" and r.stop_hit == stop and r.eval_count == n_tok
    raw = b"".join(pieces[t] for t in r.tokens)
    assert r.text == raw[:hit_start].decode().lstrip() and stop not in r.text
    assert engine.tokenizer.decode(r.tokens).startswith(r.text)
    # a string that never occurs changes nothing; one string as a plain str; logprobs cover every token
    same = engine.generate([prompt], 40, dict(opts, stop="\x00never"))[0]
    assert same.tokens == free.tokens and same.text == free.text and same.done_reason == "length"
    lp = engine.generate([prompt], 40, dict(opts, stop=stop), logprobs=True)[0]
    assert lp.tokens == r.tokens and len(lp.logprobs) == n_tok and lp.text == r.text


def test_engine_rows_with_and_without_stops(engine):
    opts = dict(temperature=0.0, eos_id=-1)
    prompts = [[1, 40, 41, 42], [1, 300, 7]]
    free = engine.generate(prompts, 24, opts)
    pieces = engine._piece_vocab()
    found = boundary_stop([pieces[t] for t in free[1].tokens])
    assert found is not None
    st, n_tok, _ = found
    res = engine.generate(prompts, 24, [opts, dict(opts, stop=[st.decode()])])
    assert res[0].tokens == free[0].tokens and res[0].stop_hit is None and res[0].done_reason == "length"
    assert res[1].tokens == free[1].tokens[:n_tok] and res[1].stop_hit == st.decode()


def test_engine_custom_pieces_spell_stop_rows():
    """An engine given ``set_json_vocab`` pieces matches on those and spells stop rows with them; JSON mode and a stop
    string together end on whichever comes first."""
    from cain_amd.engine.engine import DecodeEngine
    from jsonmode_vocab import json_test_vocabulary

    eng = DecodeEngine("tiny-llama3.1:8b", device="cpu", backend="torch", max_batch=2, max_context=256)
    vocab = json_test_vocabulary()
    eng.set_json_vocab(vocab)
    full = vocab + [b""] * (eng.cfg.vocab - len(vocab))
    for seed in range(16):  # a free JSON run long enough to stop inside: the first such seed
        o = dict(temperature=0.9, seed=seed, eos_id=-1)
        free = eng.generate([[1, 50, 60]], 60, o, format="json")[0]
        if len(free.tokens) >= 12:
            break
    assert len(free.tokens) >= 12
    raw = b"".join(full[t] for t in free.tokens)
    assert free.text == raw.decode("utf-8", "replace")
    found = boundary_stop([full[t] for t in free.tokens[:-1]], lo=1)  # (before the last token: the document is open)
    assert found is not None
    st, n_tok, hit_start = found
    r = eng.generate([[1, 50, 60]], 60, dict(o, stop=[st.decode()]), format="json")[0]
    assert r.tokens == free.tokens[:n_tok] and r.stop_hit == st.decode() and r.done_reason == "stop"
    assert r.text == raw[:hit_start].decode("utf-8", "replace") and r.json_state == "open"
    if free.json_state == "done":  # a stop string that would only come after the closing brace never gets to act
        late = eng.generate([[1, 50, 60]], 60, dict(o, stop=["\x00"]), format="json")[0]
        assert late.tokens == free.tokens and late.stop_hit is None and late.json_state == "done"
