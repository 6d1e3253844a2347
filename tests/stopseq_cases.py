"""Shared by the stop-sequence tests: the brute-force reference (the definition computed with ``bytes.find`` over the
whole stream, not the incremental rule), the named cases, the seeded random cases, and the search of a free run for a
stop string that spans a token boundary."""
from __future__ import annotations

import random
from typing import List, Optional, Sequence, Tuple

Case = Tuple[List[bytes], List[bytes]]  # (stop strings, pieces)


def brute_force(stops: Sequence[bytes], pieces: Sequence[bytes]) -> Optional[Tuple[int, int, int]]:
    """``(tokens, hit_start, hit_which)`` by the definition, or None when no stop string occurs: ``e`` is the smallest
    end offset of any occurrence in the whole stream, the final token the one that holds byte ``e - 1``, ``hit_start``
    the minimum start over the occurrences that end at or before that token's last byte, the lowest index on ties."""
    stream = b"".join(pieces)
    occ = []  # (start, index, end) of every occurrence
    for k, st in enumerate(stops):
        at = stream.find(st)
        while at >= 0:
            occ.append((at, k, at + len(st)))
            at = stream.find(st, at + 1)
    if not occ:
        return None
    e = min(o[2] for o in occ)
    n_tok, last = 0, 0
    for i, p in enumerate(pieces):  # the token that holds byte e - 1
        last += len(p)
        if last >= e:
            n_tok = i + 1
            break
    start, which, _ = min(o for o in occ if o[2] <= last)
    return n_tok, start, which


def named_cases() -> List[Tuple[str, List[bytes], List[bytes]]]:
    one = [bytes([97 + i % 26]) for i in range(32)]
    return [
        ("self-overlap", [b"aab"], [b"a", b"aa", b"b", b"c"]),
        ("prefix of another", [b"abcd", b"ab"], [b"xa", b"b", b"cd"]),
        ("prefix of another, one token", [b"abcd", b"ab"], [b"x", b"abcd", b"e"]),
        ("suffix of another, one token", [b"bc", b"abc"], [b"x", b"abcz", b"q"]),
        ("suffix of another, listed first wins only on equal starts", [b"c", b"abc", b"ab"], [b"xab", b"c"]),
        ("equal starts: the lowest index", [b"ab", b"abc", b"ab"], [b"zabc"]),
        ("32 bytes, 32 one-byte tokens", [b"".join(one)], [b"q"] + one + [b"r"]),
        ("32 bytes, starts 31 back", [b"".join(one)], [b"zz" + b"".join(one[:31]), one[31] + b"tail"]),
        ("ends on the last byte of a token", [b"end"], [b"the e", b"nd", b" more"]),
        ("ends on the first byte of a token", [b"end"], [b"the en", b"d more", b"x"]),
        ("near miss", [b"stop!"], [b"st", b"op", b"stop", b"?", b"stop", b""]),
        ("empty pieces inside a match", [b"hello"], [b"he", b"", b"l", b"", b"", b"lo", b"x"]),
        ("string longer than the stream so far", [b"abc"], [b"bc", b"abc"]),
        ("zero bytes are bytes", [b"\0\0"], [b"a", b"\0", b"b\0", b"\0"]),
        ("a long piece, the match past its 64th byte", [b"\n\n"], [b"x", b" " * 70 + b"\n\n" + b" " * 40]),
        ("a long piece, two strings, the later end starts first", [b"ccc", b"a" + b"b" * 20 + b"cccc"],
         [b"a", b"b" * 20 + b"cccc" + b"d" * 60]),
        ("utf-8 split over tokens", ["é!".encode()], [b"caf\xc3", b"\xa9", b"!?"]),
        ("never", [b"xyz", b"zzzz"], [b"xy", b"xz", b"zz", b"yz"]),
    ]


def random_cases(seed: int, n: int, long_every: int = 9) -> List[Case]:
    """``n`` seeded cases: an alphabet of 3 or 4 symbols (overlaps are common), 1 .. 8 strings of 1 .. 32 bytes, pieces
    of 0 .. 5 bytes with every ``long_every``-th case holding a few of 70 .. 130 bytes."""
    rng = random.Random(seed)
    out = []
    for c in range(n):
        alpha = b"abcd"[: rng.choice((3, 4))]
        word = lambda k: bytes(rng.choice(alpha) for _ in range(k))  # noqa: E731
        pieces = [word(rng.randint(0, 5)) for _ in range(rng.randint(1, 40))]
        if c % long_every == 0:
            for _ in range(rng.randint(1, 3)):
                pieces.insert(rng.randrange(len(pieces) + 1), word(rng.randint(70, 130)))
        stream = b"".join(pieces)
        stops = []
        for _ in range(rng.randint(1, 8)):
            k = rng.choice((1, 2, 2, 3, 3, 4, 5, 6, 8, 12, 20, 31, 32))
            if stream and rng.random() < 0.6:  # a substring of the stream, sometimes with its last byte changed
                at = rng.randrange(len(stream))
                st = stream[at: at + k]
                if st and rng.random() < 0.3:
                    st = st[:-1] + bytes([rng.choice(alpha)])
            else:
                st = word(k)
            if st:
                stops.append(st)
        out.append((stops or [word(2)], pieces))
    return out


def all_cases(seed: int = 2025, n: int = 3000) -> List[Case]:
    return [(s, p) for _, s, p in named_cases()] + random_cases(seed, n)


def boundary_stop(pieces: Sequence[bytes], lo: int = 2, max_len: int = 12):
    """A stop string for a free run whose tokens' pieces are ``pieces``: a substring of the raw stream that spans a
    token boundary, whose first occurrence in the stream is that one, and whose final token sits at a generated index
    ``i >= lo`` that is no multiple of 8 (so the row must stop inside a decode graph).  Deterministic: the first such
    ``(i, string)`` in order of ``i``, then of length.  Returns ``(string, tokens, hit_start)`` -- the number of
    tokens the stop run returns and the cut offset -- or None."""
    stream = b"".join(pieces)
    ends = []
    at = 0
    for p in pieces:
        at += len(p)
        ends.append(at)
    for i in range(lo, len(pieces)):
        if i % 8 == 0 or not pieces[i]:
            continue
        t0 = ends[i - 1]  # the boundary between token i - 1 and token i
        for back in range(1, max_len):
            for fwd in range(1, min(len(pieces[i]), max_len - back) + 1):
                st = stream[t0 - back: t0 + fwd]
                if t0 - back < 0 or len(st) != back + fwd or stream.find(st) != t0 - back:
                    continue
                try:
                    st.decode("utf-8")
                except UnicodeDecodeError:
                    continue
                got = brute_force([st], pieces)
                if got == (i + 1, t0 - back, 0):
                    return st, i + 1, t0 - back
    return None
