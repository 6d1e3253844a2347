"""Shared by the JSON-mode tests: the 1,024-piece test vocabulary, generated documents and the parser reference."""
from __future__ import annotations

import json
import random
from typing import List

from cain_amd.engine import jsonmode as jm

WS = b" \t\n\r"


def json_test_vocabulary() -> List[bytes]:
    """1,024 pieces: 16 empty specials, the 256 single bytes, then multi-byte fragments -- JSON punctuation glued to
    its neighbours, literals, numbers with a leading space, indentation, split UTF-8 halves -- and seeded filler."""
    frag = [b'{"', b'":', b'", "', b'"}', b'":"', b'": ', b'","', b'{}', b'[]', b'[{', b'}]', b'},', b'],', b'"]',
            b'true', b'false', b'null', b'tru', b'e}', b'nul', b'l,', b' 12', b' 0', b'-1', b'0.5', b'1e', b'e+',
            b'E-3', b'.25', b'123', b'\n  ', b'\n    ', b'\n', b'  ', b' ' * 8, b' ' * 17, b', ', b': ', b' {', b' [',
            b'\\n', b'\\"', b'\\u', b'\\u00', b'00e9', b'\\\\', b'\\x', b'name', b'"name"', b'"id":', b'value', b'"a',
            b'b"', b': "', b'": {', b'": [', b'"},', b'\xc3', b'\xa9', b'\xc3\xa9', b'\xe2\x82', b'\xac', b'\xe2',
            b'\x82\xac', b'\xf0\x9f', b'\x98\x80', b'\xf0', b'\x9f\x98', b'\xed\x9f', b'\xed\xa0', b'\xe0\xa0',
            b'\xe0\x80', b'\xf4\x8f', b'\xf4\x90', b'\xc0\x80', b'a\xcc', b'\x81b', b'01', b'-', b'--', b'1.', b'.e',
            b'}}', b']]', b'}\n', b'} ', b'"\n', b'":{"', b'":["', b'"],"', b'{"a":1}', b'[1,2]', b'tr', b'ue',
            b'fal', b'se', b'nu', b'll']
    frag = [f for f in frag if len(f) > 1]
    rng = random.Random(1234)
    words = "abcdefghijklmnopqrstuvwxyz"
    while 16 + 256 + len(frag) < 1024:
        n = rng.randint(2, 5)
        w = "".join(rng.choice(words) for _ in range(n)).encode()
        kind = rng.randrange(6)
        frag.append((b" " + w, w, b'"' + w, w + b'"', str(rng.randrange(10, 9999)).encode(), w + b'":')[kind])
    pieces = [b""] * 16 + [bytes([b]) for b in range(256)] + frag
    assert len(pieces) == 1024
    return pieces


def parser_ok(b: bytes) -> bool:
    """Python's own parser as the reference: strict UTF-8, ``json.loads`` without its non-standard constants, and
    an object at the top."""
    def no_constant(name):
        raise ValueError(name)

    try:
        return isinstance(json.loads(b.decode("utf-8"), parse_constant=no_constant), dict)
    except (ValueError, RecursionError):
        return False


def within_caps(b: bytes) -> bool:
    """Whitespace runs <= 16 and bracket depth <= 64, judged on the raw bytes (brackets inside strings count too:
    an over-estimate, so a True is safe)."""
    run = depth = 0
    for c in b:
        run = run + 1 if c in WS else 0
        if run > jm.WS_MAX:
            return False
        if c in b"{[":
            depth += 1
            if depth > jm.DEPTH_MAX:
                return False
        elif c in b"}]":
            depth = max(0, depth - 1)
    return True


def expected_accept(b: bytes) -> bool:
    """What the automaton must say of ``b`` (within the caps), by the parser: the parser's verdict, except that the
    automaton's document ends on its closing brace -- J_DONE takes no byte -- so trailing whitespace, which the
    parser skips, is not part of an accepted document."""
    return parser_ok(b) and b[-1:] not in (b" ", b"\t", b"\n", b"\r")


_CHARS = ["a", "Z", "0", " ", "\u00e9", "\u00df", "\u20ac", "\u0800", "\ud7ff", "\ue000", "\uffff", "\U0001f600",
          "\U00010000", "\U0010ffff", '"', "\\", "/", "\b", "\f", "\n", "\r", "\t", "\u001f", "\u007f", "\u0080",
          "\u07ff"]


def random_value(rng: random.Random, depth: int):
    k = rng.randrange(9 if depth > 0 else 6)
    if k == 0:
        return rng.choice([True, False, None])
    if k == 1:
        return rng.choice([0, -0.0, 1, -1, 12, 1.5, -2.25e-3, 1e10, 1E+2, 123456789, 0.1, -0.0001, 5e-324])
    if k in (2, 3, 4, 5):
        return "".join(rng.choice(_CHARS) for _ in range(rng.randrange(0, 5)))
    if k in (6, 7):
        return {"".join(rng.choice(_CHARS) for _ in range(rng.randrange(0, 3))):
                random_value(rng, depth - 1) for _ in range(rng.randrange(0, 3))}
    return [random_value(rng, depth - 1) for _ in range(rng.randrange(0, 4))]


def random_document(rng: random.Random) -> bytes:
    obj = {"".join(rng.choice(_CHARS) for _ in range(rng.randrange(0, 3))): random_value(rng, 3)
           for _ in range(rng.randrange(0, 4))}
    style = rng.randrange(4)
    text = json.dumps(obj, ensure_ascii=style in (0, 2), indent=2 if style >= 2 else None,
                      separators=(",", ":") if style == 0 else None)
    return text.encode("utf-8")
