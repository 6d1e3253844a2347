"""JSON mode (Ollama's ``format: "json"``): the rule, stated in plain Python.

A byte-level deterministic pushdown recogniser for RFC 8259 JSON whose top-level value is an object -- the top-level
rule of llama.cpp's ``json.gbnf`` (``root ::= object``, quoted from memory), the grammar Ollama hands llama.cpp for
``format: "json"``.  ``ops/csrc/json_pda.h`` is the same automaton in C++ for the device (csrc/grammar.hip masks, at
every decode step, the tokens whose bytes cannot continue the document); this file is the statement of the rule, the
torch backend's implementation and the tests' reference, as ``engine/speculative.py`` is for drafting.

State: ``(ctrl, depth, stack)``, the three words of ``JsonState`` (json_pda.h has the bit layout).  Beyond the RFC:

* whitespace outside strings is at most ``WS_MAX`` = 16 consecutive bytes -- a design constant: a model under a JSON
  grammar can otherwise emit whitespace forever; 16 lets pretty-printed output through depth 7 at two-space indent;
* nesting is at most ``DEPTH_MAX`` = 64 brackets;
* ``DONE`` -- the top-level object closed -- takes no byte, not even whitespace: the closing brace is the row's last
  token, so a generation ends there without any EOS id.
"""
from __future__ import annotations

import functools
from typing import List, Optional, Sequence, Tuple

import numpy as np

(START, OBJ_OPEN, NEXT_KEY, AFTER_KEY, VALUE, ARR_OPEN, AFTER_VALUE, STR, STR_ESC, STR_HEX, STR_UTF8, NUM_MINUS,
 NUM_ZERO, NUM_INT, NUM_DOT, NUM_FRAC, NUM_E, NUM_ESIGN, NUM_EXP, LIT, DONE, FAIL) = range(22)
U_80_BF, U_A0_BF, U_80_9F, U_90_BF, U_80_8F = range(5)
WS_MAX = 16
DEPTH_MAX = 64
V_MAX = 1 << 23  # masked logits carry the token id in the mantissa (csrc/grammar.hip)
LITERALS = (b"true", b"false", b"null")
_WS = frozenset(b" \t\n\r")
_HEX = frozenset(b"0123456789abcdefABCDEF")
_ESC = frozenset(b'"\\/bfnrt')
_DIGITS = frozenset(b"0123456789")
_U_RANGE = {U_80_BF: (0x80, 0xBF), U_A0_BF: (0xA0, 0xBF), U_80_9F: (0x80, 0x9F), U_90_BF: (0x90, 0xBF),
            U_80_8F: (0x80, 0x8F)}

State = Tuple[int, int, int]
INITIAL: State = (START, 0, 0)


def ctrl(sid: int, a: int = 0, b: int = 0, key: int = 0, ws: int = 0) -> int:
    return sid | (a << 5) | (b << 8) | (key << 11) | (ws << 12)


def sid_of(s: State) -> int:
    return s[0] & 31


def step(s: State, c: int) -> Optional[State]:
    """The state after byte ``c``, or None when the byte cannot continue the document."""
    cw, dw, stack = s
    sid, a, b, key, ws = cw & 31, (cw >> 5) & 7, (cw >> 8) & 7, (cw >> 11) & 1, (cw >> 12) & 31
    depth, seen = dw & 0xFF, dw & ~0xFF
    digit = c in _DIGITS
    if sid == STR:
        if c == 0x22:
            return ctrl(AFTER_KEY if key else AFTER_VALUE), dw, stack
        if c == 0x5C:
            return ctrl(STR_ESC, key=key), dw, stack
        if c < 0x20:
            return None
        if c < 0x80:
            return s
        if 0xC2 <= c <= 0xDF:
            return ctrl(STR_UTF8, 1, U_80_BF, key), dw, stack
        if 0xE0 <= c <= 0xEF:
            return ctrl(STR_UTF8, 2, U_A0_BF if c == 0xE0 else U_80_9F if c == 0xED else U_80_BF, key), dw, stack
        if 0xF0 <= c <= 0xF4:
            return ctrl(STR_UTF8, 3, U_90_BF if c == 0xF0 else U_80_8F if c == 0xF4 else U_80_BF, key), dw, stack
        return None
    if sid == STR_ESC:
        if c == 0x75:
            return ctrl(STR_HEX, 4, key=key), dw, stack
        return (ctrl(STR, key=key), dw, stack) if c in _ESC else None
    if sid == STR_HEX:
        if c not in _HEX:
            return None
        return ctrl(STR_HEX, a - 1, key=key) if a > 1 else ctrl(STR, key=key), dw, stack
    if sid == STR_UTF8:
        lo, hi = _U_RANGE[b]
        if not lo <= c <= hi:
            return None
        return ctrl(STR_UTF8, a - 1, U_80_BF, key) if a > 1 else ctrl(STR, key=key), dw, stack
    if sid == LIT:
        word = LITERALS[b]
        if c != word[a]:
            return None
        return ctrl(LIT, a + 1, b) if a + 1 < len(word) else ctrl(AFTER_VALUE), dw, stack
    if NUM_MINUS <= sid <= NUM_EXP:
        e = c in (0x65, 0x45)
        end = -1  # the number may end here: the byte is then one of AFTER_VALUE
        nxt = {
            NUM_MINUS: NUM_ZERO if c == 0x30 else NUM_INT if digit else None,
            NUM_ZERO: NUM_DOT if c == 0x2E else NUM_E if e else end,
            NUM_INT: NUM_INT if digit else NUM_DOT if c == 0x2E else NUM_E if e else end,
            NUM_DOT: NUM_FRAC if digit else None,
            NUM_FRAC: NUM_FRAC if digit else NUM_E if e else end,
            NUM_E: NUM_EXP if digit else NUM_ESIGN if c in (0x2B, 0x2D) else None,
            NUM_ESIGN: NUM_EXP if digit else None,
            NUM_EXP: NUM_EXP if digit else end,
        }[sid]
        if nxt is None:
            return None
        if nxt != end:
            return ctrl(nxt), dw, stack
        sid = AFTER_VALUE
    if sid in (DONE, FAIL):
        return None
    if c in _WS:
        return None if ws >= WS_MAX else (ctrl(sid, ws=ws + 1), dw, stack)
    top_obj = depth > 0 and bool(stack & 1)
    close = False
    if sid in (START, VALUE, ARR_OPEN):
        if sid == ARR_OPEN and c == 0x5D:
            close = True
        elif c == 0x7B or (c == 0x5B and sid != START):
            if depth >= DEPTH_MAX:
                return None
            obj = int(c == 0x7B)
            return ctrl(OBJ_OPEN if obj else ARR_OPEN), seen | (depth + 1), ((stack << 1) | obj) & (2 ** 64 - 1)
        elif sid == START:
            return None
        elif c == 0x22:
            return ctrl(STR), dw, stack
        elif c == 0x2D:
            return ctrl(NUM_MINUS), dw, stack
        elif c == 0x30:
            return ctrl(NUM_ZERO), dw, stack
        elif digit:
            return ctrl(NUM_INT), dw, stack
        elif c in b"tfn":
            return ctrl(LIT, 1, b"tfn".index(c)), dw, stack
        else:
            return None
    elif sid in (OBJ_OPEN, NEXT_KEY):
        if c == 0x22:
            return ctrl(STR, key=1), dw, stack
        if not (sid == OBJ_OPEN and c == 0x7D):
            return None
        close = True
    elif sid == AFTER_KEY:
        return (ctrl(VALUE), dw, stack) if c == 0x3A else None
    else:  # AFTER_VALUE
        if c == 0x2C:
            return ctrl(NEXT_KEY if top_obj else VALUE), dw, stack
        if c != (0x7D if top_obj else 0x5D):
            return None
        close = True
    if not close:
        return None
    return ctrl(DONE if depth == 1 else AFTER_VALUE), seen | (depth - 1), stack >> 1


def run(data: bytes, s: State = INITIAL) -> Optional[State]:
    """The state after ``data``; None: some byte was invalid (``data`` is not a viable prefix from ``s``)."""
    for c in data:
        s = step(s, c)
        if s is None:
            return None
    return s


def viable(data: bytes, s: State = INITIAL) -> bool:
    return run(data, s) is not None


def accepts(data: bytes) -> bool:
    """``data`` is a whole document: every byte valid and the top-level object closed by the last one."""
    s = run(data)
    return s is not None and sid_of(s) == DONE


def token_ok(s: State, piece: bytes) -> bool:
    return len(piece) > 0 and run(piece, s) is not None


def advance(s: State, piece: bytes) -> Tuple[State, bool]:
    """Consume one token: the new state (its token count one up), or the FAIL state when the token is not valid."""
    t = run(piece, s) if piece else None
    if t is None:
        return (ctrl(FAIL), s[1], s[2]), False
    return (t[0], t[1] + 0x100, t[2]), True


def close(prefix: bytes) -> bytes:
    """A completion of a viable prefix: ``prefix + close(prefix)`` is a whole document (no live state is doomed)."""
    s = run(prefix)
    if s is None:
        raise ValueError("not a viable prefix")
    out = bytearray()

    def put(bs: bytes) -> None:
        nonlocal s
        for c in bs:
            s = step(s, c)
            assert s is not None, (prefix, bytes(out), bs)
        out.extend(bs)

    while sid_of(s) != DONE:
        sid, a, b = s[0] & 31, (s[0] >> 5) & 7, (s[0] >> 8) & 7
        top_obj = bool(s[2] & 1)
        if sid == START:
            put(b"{")
        elif sid in (OBJ_OPEN,):
            put(b"}")
        elif sid == NEXT_KEY:
            put(b'"":0')
        elif sid == AFTER_KEY:
            put(b":0")
        elif sid == VALUE:
            put(b"0")
        elif sid == ARR_OPEN:
            put(b"]")
        elif sid == AFTER_VALUE or sid in (NUM_ZERO, NUM_INT, NUM_FRAC, NUM_EXP):
            put(b"}" if top_obj else b"]")
        elif sid == STR:
            put(b'"')
        elif sid == STR_ESC:
            put(b"n")
        elif sid == STR_HEX:
            put(b"0" * a)
        elif sid == STR_UTF8:
            put(bytes([_U_RANGE[b][0]]) + b"\x80" * (a - 1))
        elif sid in (NUM_MINUS, NUM_DOT, NUM_E, NUM_ESIGN):
            put(b"0")
        elif sid == LIT:
            put(LITERALS[b][a:])
        else:
            raise AssertionError(f"state {sid} cannot be closed")
    return bytes(out)


# ---------------------------------------------------------------- vocabulary
@functools.lru_cache(maxsize=None)
def _gpt2_byte_table():
    """GPT-2's byte <-> unicode table (byte-level BPE pieces spell each byte as one printable character)."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(bs, cs)}


def piece_bytes(piece: str, byte_level: bool) -> bytes:
    """The bytes one vocabulary piece stands for: byte-level BPE through GPT-2's table, SentencePiece with its word
    mark as a space and ``<0xNN>`` as that byte."""
    if byte_level:
        table = _gpt2_byte_table()
        try:
            return bytes(table[ch] for ch in piece)
        except KeyError:  # not a byte-level piece (an added token spelt in plain text)
            return piece.encode("utf-8")
    if len(piece) == 6 and piece.startswith("<0x") and piece.endswith(">"):
        try:
            return bytes([int(piece[3:5], 16)])
        except ValueError:
            pass
    return piece.replace("▁", " ").encode("utf-8")


def token_bytes(tokenizer, V: int) -> List[bytes]:
    """One ``bytes`` per token id ``0 .. V - 1``: what the token appends to the output.  Special and control tokens and
    ids beyond the tokenizer's size are empty (never allowed under the grammar).  ``tokenizer``: an ``HFTokenizer``,
    a ``tokenizers.Tokenizer`` or anything with ``id_to_token`` / ``get_vocab_size`` (``special_ids`` optional) --
    byte-level BPE or SentencePiece, told apart by the vocabulary itself; otherwise a tokenizer with ``piece(id)``
    (the synthetic one), whose pieces are taken as text."""
    tok = getattr(tokenizer, "tok", tokenizer)
    out = [b""] * V
    if hasattr(tok, "id_to_token"):
        n = min(V, int(tok.get_vocab_size(with_added_tokens=True)) if _takes_added(tok) else int(tok.get_vocab_size()))
        special = set(int(i) for i in getattr(tok, "special_ids", ()))
        if hasattr(tok, "get_added_tokens_decoder"):
            special |= {int(i) for i, t in tok.get_added_tokens_decoder().items() if getattr(t, "special", True)}
        pieces = [tok.id_to_token(i) for i in range(n)]
        # SentencePiece vocabularies carry byte tokens <0xNN> or the word mark; byte-level BPE spells a space as U+0120
        sp = any(p is not None and (p == "<0x0A>" or "▁" in p) for p in pieces)
        for i, p in enumerate(pieces):
            if p is None or i in special:
                continue
            if sp and len(p) > 2 and p[0] == "<" and p[-1] == ">" and not p.startswith("<0x"):
                continue  # control tokens of a SentencePiece vocabulary: <s>, </s>, <unk>, <pad> ...
            out[i] = piece_bytes(p, byte_level=not sp)
        return out
    n = min(V, int(getattr(tokenizer, "vocab", V)))
    n_special = int(getattr(tokenizer, "n_special", 0))
    for i in range(n_special, n):
        out[i] = tokenizer.piece(i).encode("utf-8")
    return out


def _takes_added(tok) -> bool:
    try:
        tok.get_vocab_size(with_added_tokens=True)
        return True
    except TypeError:
        return False


def control_configurations() -> List[State]:
    """Every control configuration the vocabulary check covers: state id (with its literal / escape / UTF-8
    sub-states) x innermost bracket {none, object, array} x depth {< 64, 64} x whitespace run {< 16, 16}."""
    subs = {LIT: [(a, b) for b, w in enumerate(LITERALS) for a in range(1, len(w))],
            STR_HEX: [(a, 0) for a in range(1, 5)],
            # after the first byte of a 2- / 3- / 4-byte character, and after each further one
            STR_UTF8: [(1, U_80_BF), (2, U_80_BF), (2, U_A0_BF), (2, U_80_9F), (3, U_80_BF), (3, U_90_BF),
                       (3, U_80_8F)]}
    ws_states = (START, OBJ_OPEN, NEXT_KEY, AFTER_KEY, VALUE, ARR_OPEN, AFTER_VALUE)
    out: List[State] = []
    for sid in range(DONE):
        if sid == START:
            stacks = [(0, 0)]
        else:
            # (depth word, stack) with an object at the bottom: depth 1 / 2 / 64 under an object, 2 / 64 under an array
            tops = [1] if sid in (OBJ_OPEN, NEXT_KEY, AFTER_KEY) else [0] if sid == ARR_OPEN else [1, 0]
            stacks = [(d, (1 << (d - 1)) | t) for t in tops for d in (1, 2, DEPTH_MAX) if not (d == 1 and t == 0)]
        keys = (0, 1) if sid in (STR, STR_ESC, STR_HEX, STR_UTF8) else (0,)
        for a, b in subs.get(sid, [(0, 0)]):
            for key in keys:
                for ws in ((0, WS_MAX) if sid in ws_states else (0,)):
                    for d, st in stacks:
                        if key and not st & 1:
                            continue  # a key string sits directly inside an object
                        out.append((ctrl(sid, a, b, key, ws), d, st))
    return out


def check_vocabulary(pieces: Sequence[bytes]) -> None:
    """A sufficient condition for 'this vocabulary can always continue a JSON document': the bytes that exist as
    single-byte tokens take at least one step from every live control configuration.  Raises ValueError otherwise."""
    if len(pieces) > V_MAX:
        raise ValueError(f"JSON mode supports vocabularies up to {V_MAX} tokens, got {len(pieces)}")
    single = sorted({p[0] for p in pieces if len(p) == 1})
    for s in control_configurations():
        if not any(step(s, c) is not None for c in single):
            raise ValueError(f"vocabulary cannot spell JSON: no single-byte token continues state {sid_of(s)} "
                             f"(control word {s[0]:#x}, depth {s[1]}); single-byte tokens: {len(single)}")


def piece_table(pieces: Sequence[bytes]):
    """The device table: ``(piece_off [V + 1] int32, piece_bytes uint8)`` numpy arrays, token t's bytes at
    ``piece_bytes[piece_off[t] : piece_off[t + 1]]`` (at least one byte long, so the array is never empty)."""
    off = np.zeros(len(pieces) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in pieces], out=off[1:])
    if off[-1] >= 2 ** 31:
        raise ValueError("token pieces exceed 2 GiB")
    flat = np.frombuffer(b"".join(pieces) or b"\0", dtype=np.uint8).copy()
    return off.astype(np.int32), flat


# ---------------------------------------------------------------- the mask on the host (torch backend, tests)
def masked_value(t: int) -> float:
    """The logit a rejected token ``t`` gets: ``-(2^100 * (1 + t / 2^23))``, about -1e30, distinct per token and
    decreasing with ``t`` -- no new ties for any sampler, and exp() of it is exactly 0 at any sane temperature."""
    return float(-np.array([(227 << 23) | int(t)], dtype=np.uint32).view(np.float32)[0])


def allowed_ids(s: State, pieces: Sequence[bytes]) -> List[int]:
    return [t for t, p in enumerate(pieces) if token_ok(s, p)]


def mask_logits_host(logits, s: State, pieces: Sequence[bytes]):
    """``logits`` ([V] float32 numpy, modified in place): every token not valid from ``s`` gets its masked value."""
    V = logits.shape[0]
    bad = np.ones(V, dtype=bool)
    bad[[t for t in allowed_ids(s, pieces[:V]) if t < V]] = False
    ids = np.flatnonzero(bad).astype(np.uint32)
    logits[ids] = -(((np.uint32(227) << np.uint32(23)) | ids).view(np.float32))
    return logits
