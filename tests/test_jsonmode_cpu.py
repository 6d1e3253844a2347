"""JSON mode on the CPU: the automaton against Python's own parser, the C++ header against the Python automaton, the
vocabulary's byte pieces and check, and the torch backend end to end.

Reference: ``json.loads`` on the strictly decoded bytes (jsonmode_vocab.parser_ok).  The automaton has two rules the
parser lacks -- whitespace runs <= 16, depth <= 64 -- so every input compared against the parser is asserted to stay
within both, and the caps have tests of their own.  One more difference is by design (the issue's DONE rule): the
document ends on its closing brace, so trailing whitespace, which the parser skips, is rejected; for such inputs the
test asserts both halves -- the automaton rejects the input and accepts it without the trailing whitespace exactly
when the parser accepts it.
"""
import itertools
import json
import random
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

from cain_amd.engine import jsonmode as jm
from jsonmode_vocab import (WS, expected_accept, json_test_vocabulary, parser_ok, random_document, within_caps)

ROOT = Path(__file__).resolve().parent.parent
HEADER_DIR = ROOT / "cain_amd" / "ops" / "csrc"
HOST_SRC = ROOT / "tests" / "csrc" / "json_pda_host.cpp"


def check_against_parser(b: bytes) -> None:
    assert within_caps(b), b
    assert jm.accepts(b) == expected_accept(b), b
    core = b.rstrip(WS)
    if core != b:  # trailing whitespace: the parser's verdict holds for the document without it
        assert jm.accepts(core) == parser_ok(b), b


def mutations(seed: int, n_docs: int, per_doc: int):
    rng = random.Random(seed)
    pool = b'{}[]:,"\\/0123456789-+.eEtrufalsn \t\n\r\x00\x1f\x7f\x80\xbf\xc0\xc2\xe0\xed\xf0\xf4\xf5\xffabu'
    out = []
    for _ in range(n_docs):
        doc = random_document(rng)
        out.append(doc)
        for _ in range(per_doc):
            for _attempt in range(8):
                i = rng.randrange(len(doc))
                kind = rng.randrange(3)
                c = bytes([rng.choice(pool)])
                m = doc[:i] + c + doc[i + 1:] if kind == 0 else doc[:i] + c + doc[i:] if kind == 1 \
                    else doc[:i] + doc[i + 1:]
                if within_caps(m):
                    out.append(m)
                    break
    return out


def test_every_short_string_against_the_parser():
    """Every byte string of length <= 5 over 12 bytes, bare, and -- since no object with a member fits 5 bytes --
    every string of length <= 5 over 12 value bytes as the value of ``{"":...}``.  The automaton runs as a depth-first
    walk (one step per string); the parser sees every string."""
    for alphabet, head, tail in ((b'{}[]:,"\\01- ', b"", b""), (b'[],"\\01-.e{ ', b'{"":', b"}")):
        n = 0
        start = jm.run(head)

        def walk(prefix: bytes, state):
            nonlocal n
            n += 1
            doc = head + prefix + tail
            end = None if state is None else jm.run(tail, state)
            got = end is not None and jm.sid_of(end) == jm.DONE
            assert within_caps(doc)
            assert got == expected_accept(doc), doc
            if len(prefix) < 5:
                for c in alphabet:
                    walk(prefix + bytes([c]), None if state is None else jm.step(state, c))

        walk(b"", start)
        assert n == sum(12 ** k for k in range(6))


def test_mutated_documents_against_the_parser():
    inputs = mutations(seed=20251, n_docs=400, per_doc=8)
    # an invalid first / continuation pair from each restricted range, and the valid neighbour of each
    for pair, ok in ((b"\xe0\x9f\x80", False), (b"\xe0\xa0\x80", True), (b"\xed\xa0\x80", False),
                     (b"\xed\x9f\xbf", True), (b"\xf0\x8f\x80\x80", False), (b"\xf0\x90\x80\x80", True),
                     (b"\xf4\x90\x80\x80", False), (b"\xf4\x8f\xbf\xbf", True), (b"\xc0\x80", False),
                     (b"\xc1\xbf", False), (b"\xc2\x80", True), (b"\xf5\x80\x80\x80", False), (b"\x80", False),
                     (b"\xe2\x82", False), (b"\xe2\x82\xac", True)):
        doc = b'{"k' + pair + b'":"' + pair + b'"}'
        assert parser_ok(doc) == ok
        inputs.append(doc)
    inputs += [b'{"a":"\\ud800"}', b'{"a":"\\u12G4"}', b'{"a":"\\u123"}', b'{"a":"\\x"}', b'{"a":"\t"}',
               b'{"a":01}', b'{"a":-}', b'{"a":1.}', b'{"a":.5}', b'{"a":1e}', b'{"a":1e+}', b'{"a":-0.0e-0}',
               b'{"a":NaN}', b'{"a":Infinity}', b'{"a":-Infinity}', b'{"a":tru}', b'{"a":nulll}', b'[]', b'"a"', b'1',
               b' {"a" : [ 1 , 2 ] } ', b'{"a":1,}', b'{,}', b'{"a"}', b'{"a":}', b'{"a":[1,]}', b'{"a":1 "b":2}',
               b'{"a":1}{"b":2}', b'{"a":1}x', b'\xef\xbb\xbf{}', b'{"a":[1 2]}', b'{"a":{"b":[{}]}}', b'']
    assert len(inputs) > 3000
    n_ok = 0
    for b in inputs:
        check_against_parser(b)
        n_ok += jm.accepts(b)
    assert 400 <= n_ok < len(inputs) - 1000  # both verdicts are well represented


def test_the_two_caps():
    for n in (1, 16):
        assert jm.accepts(b'{"a":' + b" " * n + b"1}")
    s = jm.run(b'{"a":' + b" \t\n\r" * 4)
    assert s is not None and all(jm.step(s, c) is None for c in WS) and jm.step(s, ord("1")) is not None
    assert not jm.viable(b"{" + b"\n" * 17)
    assert jm.viable(b'{"a":1' + b" " * 16) and not jm.viable(b'{"a":1' + b" " * 17)  # a run that a number's end starts
    deep = b'{"a":' + b"[" * 63
    assert jm.viable(deep) and jm.run(deep)[1] & 0xFF == 64
    assert jm.accepts(deep + b"]" * 63 + b"}") and parser_ok(deep + b"]" * 63 + b"}")
    assert not jm.viable(deep + b"[") and not jm.viable(deep + b"{") and jm.viable(deep + b"1")
    nest = b'{"a":' * 64
    assert jm.viable(nest) and not jm.viable(nest + b"{") and jm.accepts(nest + b"0" + b"}" * 64)
    assert jm.run(b"{}") is not None and all(jm.step(jm.run(b"{}"), c) is None for c in range(256))  # DONE


def test_no_doomed_live_state():
    rng = random.Random(77)
    n = 0
    for doc in mutations(seed=5, n_docs=150, per_doc=4):
        cuts = {rng.randrange(len(doc) + 1) for _ in range(6)} if doc else {0}
        for cut in cuts:
            p = doc[:cut]
            if not jm.viable(p):
                continue
            tail = jm.close(p)
            assert jm.accepts(p + tail), p
            if within_caps(p + tail):
                assert parser_ok(p + tail), p
                n += 1
    assert n > 1500
    for s in jm.control_configurations():  # and from every configuration of the vocabulary check, by single bytes
        assert any(jm.step(s, c) is not None for c in range(256)), s


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


def _prefix_state(b: bytes):
    s, ok = jm.INITIAL, True
    for c in b:
        t = jm.step(s, c)
        if t is None:
            ok = False
            break
        s = t
    return ok, s


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                                              "-fno-sanitize-recover=all")], ids=["plain", "asan-ubsan"])
def test_header_on_the_host_equals_the_python_automaton(tmp_path, flags):
    exe = _build(tmp_path, flags, "json_pda_host")
    inputs = mutations(seed=99, n_docs=120, per_doc=6)
    inputs += [bytes(p) for k in range(4) for p in itertools.product(b'{}[]:,"\\01-.et \xc3\xa9', repeat=k)]
    inputs += [b'{"a":' + b"[" * 70, b"{" + b" " * 20, b'{"a":"\\u00e9\xf0\x9f\x98\x80"}', b'{"a":false,"b":null}']
    blob = b"".join(struct.pack("<I", len(b)) + b for b in inputs)
    r = subprocess.run([str(exe)], input=blob, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(inputs)
    for b, line in zip(inputs, lines):
        ok, s = _prefix_state(b)
        want = (int(ok and jm.sid_of(s) == jm.DONE), int(ok), s[0], s[1], s[2])
        assert tuple(int(x) for x in line.split()) == want, b


# ---------------------------------------------------------------- tokens
def test_token_bytes_byte_level_and_sentencepiece():
    table = jm._gpt2_byte_table()
    inv = {b: ch for ch, b in table.items()}
    assert len(table) == 256 and inv[0x20] == "\u0120" and inv[0x0A] == "\u010a" and inv[ord("a")] == "a"

    class Tok:  # the two calls token_bytes makes of a tokenizers.Tokenizer
        def __init__(self, pieces, special=()):
            self.pieces, self.special_ids = pieces, special

        def get_vocab_size(self):
            return len(self.pieces)

        def id_to_token(self, i):
            return self.pieces[i]

    bl = Tok(["<|begin|>", "<|end|>", "\u0120{", '":', "\u010a\u0120\u0120", "\u00c3", "\u00a9", "true", "\u00e2\u0124\u00ac"],
             special=(0, 1))
    got = jm.token_bytes(bl, 12)
    assert got == [b"", b"", b" {", b'":', b"\n  ", b"\xc3", b"\xa9", b"true", b"\xe2\x82\xac", b"", b"", b""]
    sp = Tok(["<unk>", "<s>", "</s>", "<0x0A>", "<0xC3>", "<0xA9>", "\u2581{", '":', "\u2581\u2581", "é", "<0x7B>"])
    assert jm.token_bytes(sp, 11) == [b"", b"", b"", b"\n", b"\xc3", b"\xa9", b" {", b'":', b"  ", b"\xc3\xa9", b"{"]
    try:
        from tokenizers import Tokenizer, models
    except ImportError:
        return
    vocab = {inv[b]: b for b in range(256)}
    vocab.update({"\u0120{": 256, '":': 257, "<|eot|>": 258})
    tk = Tokenizer(models.BPE(vocab=vocab, merges=[]))
    tk.add_special_tokens(["<|eot|>"])
    got = jm.token_bytes(tk, 260)
    assert got[:256] == [bytes([b]) for b in range(256)] and got[256:] == [b" {", b'":', b"", b""]


def test_vocabulary_check():
    from cain_amd.models.config import get_config
    from cain_amd.models.tokenizer import SyntheticTokenizer

    pieces = json_test_vocabulary()
    assert len(pieces) == 1024 and pieces[:16] == [b""] * 16 and pieces[16:272] == [bytes([b]) for b in range(256)]
    jm.check_vocabulary(pieces)
    cfg = get_config("tiny-llama3.1:8b")
    with pytest.raises(ValueError, match="vocabulary cannot spell JSON"):
        jm.check_vocabulary(jm.token_bytes(SyntheticTokenizer(cfg.vocab), cfg.vocab))
    no_quote = [p for p in pieces if p != b'"']
    with pytest.raises(ValueError, match="vocabulary cannot spell JSON"):
        jm.check_vocabulary(no_quote)
    off, flat = jm.piece_table(pieces)
    assert off[0] == 0 and off[-1] == len(flat) == sum(map(len, pieces))
    assert bytes(flat[off[300]:off[301]]) == pieces[300]


# ---------------------------------------------------------------- engine (torch backend)
@pytest.fixture(scope="module")
def engine():
    from cain_amd.engine.engine import DecodeEngine

    eng = DecodeEngine("tiny-llama3.1:8b", device="cpu", backend="torch", max_batch=4, max_context=256)
    return eng


def test_engine_refuses_without_a_json_vocabulary(engine):
    assert engine._json_pieces is None
    with pytest.raises(ValueError, match="vocabulary cannot spell JSON"):
        engine.generate([[1, 5, 9]], 4, format="json")
    with pytest.raises(ValueError, match="format"):
        engine.generate([[1, 5, 9]], 4, format="xml")


@pytest.mark.parametrize("options", [dict(temperature=0.0), dict(temperature=0.9, seed=11),
                                     dict(temperature=1.5, top_k=1000, top_p=1.0, seed=5)],
                         ids=["greedy", "seeded", "wide"])
def test_engine_json_rows_are_viable_at_every_token(engine, options):
    pieces = json_test_vocabulary()
    engine.set_json_vocab(pieces)
    full = pieces + [b""] * (engine.cfg.vocab - len(pieces))
    prompts = [[1, 40, 41, 42], [1, 300, 7], [1, 999]]
    res = engine.generate(prompts, [24, 200, 200], dict(options, eos_id=-1), format=["json", "json", None])
    plain = engine.generate(prompts[2:], [200], dict(options, eos_id=-1))
    assert res[2].tokens == plain[0].tokens and res[2].json_state is None and len(res[2].tokens) == 200
    for r, budget in zip(res[:2], (24, 200)):
        s = jm.INITIAL
        for t in r.tokens:
            assert jm.token_ok(s, full[t]), (r.tokens, t)
            s, ok = jm.advance(s, full[t])
            assert ok
        data = b"".join(full[t] for t in r.tokens)
        assert r.text == data.decode("utf-8", errors="replace")
        if r.json_state == "done":
            assert r.done_reason == "stop" and jm.sid_of(s) == jm.DONE and data.endswith(b"}")
            assert isinstance(json.loads(r.text), dict)
        else:
            assert r.json_state == "open" and r.done_reason == "length" and len(r.tokens) == budget
            assert jm.viable(data) and isinstance(json.loads((data + jm.close(data)).decode("utf-8")), dict)


def test_engine_large_budget_ends_on_the_closing_brace(engine):
    """A row that ends before its budget did so on the closing brace, and its text parses to a dict (no EOS id is set,
    so nothing else can end it)."""
    engine.set_json_vocab(json_test_vocabulary())
    ended = 0
    for seed in range(6):
        r = engine.generate([[1, 17 + seed]], 240, dict(temperature=1.0, seed=seed, eos_id=-1), format="json")[0]
        if len(r.tokens) < 240:
            ended += 1
            assert r.done_reason == "stop" and r.text.endswith("}") and isinstance(json.loads(r.text), dict)
    assert ended >= 1


def test_engine_format_with_logprobs_and_speculative(engine):
    from cain_amd.engine.engine import DecodeEngine

    engine.set_json_vocab(json_test_vocabulary())
    o = dict(temperature=0.7, seed=3, eos_id=-1)
    a = engine.generate([[1, 50, 60]], 12, o, format="json")[0]
    b = engine.generate([[1, 50, 60]], 12, dict(o, format="json"), logprobs=True, top_logprobs=2)[0]
    assert a.tokens == b.tokens and len(b.logprobs) == len(b.tokens)
    assert all(lp <= 0.0 for lp in b.logprobs)  # the model's own distribution, not the masked one
    spec = DecodeEngine("tiny-llama3.1:8b", device="cpu", backend="torch", max_batch=2, max_context=128,
                        speculative=2)
    with pytest.raises(ValueError, match="speculative"):
        spec.generate([[1, 2, 3]], 4, format="json")
