"""Stop sequences (Ollama's ``options.stop``): the rule, stated in plain Python.

A row has 0 to ``STOP_MAX`` = 8 stop strings of 1 to ``STOP_LEN_MAX`` = 32 bytes of UTF-8 each.  Matching is on
**bytes**.  The row's stream is the concatenation of its generated tokens' pieces (``jsonmode.token_bytes``), in
order; special tokens are empty and add nothing; the prompt is not part of the stream.

Advance over one token: append its piece and consider every occurrence of any stop string that *ends* inside this
token's bytes (it may start in earlier tokens, at most 31 bytes back).  None: the state moves on and the row lives.
Else the row is done **on this token**: ``hit_start`` is the smallest start offset among those occurrences, and among
the strings that occur there the lowest index in the request's list wins.  The token stays in the row's tokens; the
bytes from ``hit_start`` on are cut from its text.  Occurrences that end in a later token are never seen: the row has
stopped.

``ops/csrc/stop_match.h`` is the same rule in C++ for the device (csrc/stopseq.hip runs it after the sampler inside
the decode graphs); this file is the statement of the rule, the torch backend's implementation and the tests'
incremental reference, as ``engine/jsonmode.py`` is for JSON mode.

State: ``(tail, n_tok, n_bytes, hit_start, hit_which)`` -- the last 31 bytes of the stream (zero-filled at the front
while the stream is shorter), tokens consumed, bytes consumed, -1 or the cut offset, -1 or the matched index;
``state_bytes`` gives the device's 48-byte ``StopState``.
"""
from __future__ import annotations

import struct
from typing import List, Optional, Sequence, Tuple

STOP_MAX = 8
STOP_LEN_MAX = 32
TAIL = STOP_LEN_MAX - 1
STATE_BYTES = 48

State = Tuple[bytes, int, int, int, int]
INITIAL: State = (bytes(TAIL), 0, 0, -1, -1)


def parse_stop(stop) -> Tuple[str, ...]:
    """A request's ``stop`` option as a tuple of strings (None: none).  Raises ValueError for anything but a string or
    a sequence of 0 .. 8 strings of 1 .. 32 UTF-8 bytes each."""
    if stop is None:
        return ()
    if isinstance(stop, str):
        stop = [stop]
    if isinstance(stop, (bytes, bytearray, dict)) or not hasattr(stop, "__iter__"):
        raise ValueError(f"stop must be a string or a list of strings, got {type(stop).__name__} (token ids go in "
                         f"stop_ids)")
    stop = list(stop)
    for s in stop:
        if not isinstance(s, str):
            raise ValueError(f"stop must hold strings, got {type(s).__name__} (token ids go in stop_ids)")
        if not s:
            raise ValueError("stop holds an empty string")
        n = len(s.encode("utf-8"))
        if n > STOP_LEN_MAX:
            raise ValueError(f"stop string {s!r} is {n} bytes of UTF-8, the limit is {STOP_LEN_MAX}")
    if len(stop) > STOP_MAX:
        raise ValueError(f"{len(stop)} stop strings, the limit is {STOP_MAX}")
    return tuple(stop)


def stop_bytes(stops: Sequence) -> List[bytes]:
    return [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in stops]


def advance(s: State, piece: bytes, stops: Sequence[bytes]) -> Tuple[State, bool]:
    """Consume one token: the new state and whether a stop string ended inside the token's bytes."""
    tail, n_tok, n_bytes, hit_start, hit_which = s
    buf = tail + piece  # byte r of (tail, piece) is buf[TAIL + r]
    best = None
    for j in range(len(piece)):
        for k, st in enumerate(stops):
            r0 = j - len(st) + 1
            if n_bytes + r0 < 0:
                continue  # it would start before the stream does
            if buf[TAIL + r0: TAIL + j + 1] == st and (best is None or (r0, k) < best):
                best = (r0, k)
    if best is not None:
        hit_start, hit_which = n_bytes + best[0], best[1]
    return (buf[len(buf) - TAIL:], n_tok + 1, n_bytes + len(piece), hit_start, hit_which), best is not None


def run(pieces: Sequence[bytes], stops: Sequence[bytes], s: State = INITIAL) -> Tuple[State, int]:
    """Advance over ``pieces`` until a hit: the state and the number of tokens consumed."""
    for i, p in enumerate(pieces):
        s, hit = advance(s, p, stops)
        if hit:
            return s, i + 1
    return s, len(pieces)


def state_bytes(s: State) -> bytes:
    """The device's ``StopState`` (csrc/stop_match.h) of a state."""
    return s[0] + b"\0" + struct.pack("<iiii", s[1], s[2], s[3], s[4])


def state_from_bytes(b: bytes) -> State:
    n_tok, n_bytes, hs, hw = struct.unpack("<iiii", bytes(b[STOP_LEN_MAX:STATE_BYTES]))
    return bytes(b[:TAIL]), n_tok, n_bytes, hs, hw


def cut_text(full: str, raw: bytes, hit_start: int) -> str:
    """The text of a row that hit a stop string: ``full`` (the decoder's text of all its tokens) without the
    characters of ``raw[hit_start:]`` (``raw``: the joined pieces), floored at the empty string -- counted from the
    end, so a tokenizer that strips a leading space is harmless."""
    drop = len(raw[hit_start:].decode("utf-8", "replace"))
    return full[:max(0, len(full) - drop)]


def held_back(text: str, stops: Sequence[str]) -> int:
    """Streaming: the length of the longest suffix of ``text`` that is a proper prefix of one of ``stops`` -- it may
    yet become a stop string, so it is not sent while the row lives."""
    best = 0
    for st in stops:
        for n in range(min(len(st) - 1, len(text)), best, -1):
            if text.endswith(st[:n]):
                best = n
                break
    return best
