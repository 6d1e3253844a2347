// JSON mode's automaton, stated once: a byte-level deterministic pushdown recogniser for RFC 8259 JSON whose
// top-level value is an object (llama.cpp's json.gbnf, the grammar Ollama passes for format "json", has
// `root ::= object`; quoted from memory).  Plain C++ with no HIP types: hipcc compiles it for both sides, g++ compiles
// it alone (tests/csrc/json_pda_host.cpp).  engine/jsonmode.py states the same rule in Python, word for word.
//
// Per-row state, 16 bytes:
//   ctrl   bits 0-4 state id, 5-7 `a`, 8-10 `b`, 11 the string is an object key, 12-16 length of the current
//          whitespace run.  (a, b) per state: J_LIT -- bytes of the literal matched so far, which literal (0 true,
//          1 false, 2 null); J_STR_HEX -- hex digits still owed by \uXXXX; J_STR_UTF8 -- continuation bytes still
//          owed, the allowed range of the next one (U_*: Unicode's well-formed UTF-8 table); else 0
//   depth  bits 0-7 open brackets (0 .. 64); bits 8-31 tokens json_advance has consumed (the recogniser proper never
//          reads them: the advance kernel uses them to tell a row that generated this step from one that did not)
//   stack  kinds of the open brackets, innermost at bit 0: 1 object, 0 array
//
// Rules beyond the RFC's grammar: whitespace outside strings is at most JSON_WS_MAX consecutive bytes (a model under
// a JSON grammar can otherwise emit whitespace forever; 16 lets pretty-printed output through depth 7 at two-space
// indent), nesting is at most JSON_DEPTH_MAX, and J_DONE -- the top-level object closed -- takes no byte at all, not
// even whitespace: the closing brace ends the document.  Whitespace before the opening brace is allowed, as the RFC
// allows it.  A number ends on the first byte that cannot extend it; that byte is then a byte of J_AFTER_VALUE.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JSON_HD __host__ __device__
#else
#define JSON_HD
#endif

enum {
  J_START = 0,     // ws | {
  J_OBJ_OPEN,      // after {: ws | " | }
  J_NEXT_KEY,      // after , in an object: ws | "
  J_AFTER_KEY,     // ws | :
  J_VALUE,         // after : or after , in an array: ws | a value's first byte
  J_ARR_OPEN,      // after [: ws | a value's first byte | ]
  J_AFTER_VALUE,   // ws | , | the bracket that closes the innermost open one
  J_STR,           // inside a string
  J_STR_ESC,       // after a backslash
  J_STR_HEX,       // inside \uXXXX
  J_STR_UTF8,      // inside a multi-byte character
  J_NUM_MINUS,     // after -: a digit
  J_NUM_ZERO,      // after a leading 0: . | e | E | end
  J_NUM_INT,       // digit | . | e | E | end
  J_NUM_DOT,       // after .: a digit
  J_NUM_FRAC,      // digit | e | E | end
  J_NUM_E,         // after e: + | - | digit
  J_NUM_ESIGN,     // after the exponent's sign: a digit
  J_NUM_EXP,       // digit | end
  J_LIT,           // inside true / false / null
  J_DONE,          // the top-level object closed: no byte is valid
  J_FAIL,          // json_advance met an invalid token
  J_NSTATES
};
enum { U_80_BF = 0, U_A0_BF, U_80_9F, U_90_BF, U_80_8F };  // allowed range of the next UTF-8 continuation byte

#define JSON_WS_MAX 16
#define JSON_DEPTH_MAX 64

struct JsonState {
  uint32_t ctrl;
  uint32_t depth;
  uint64_t stack;
};

JSON_HD inline uint32_t json_ctrl(uint32_t sid, uint32_t a, uint32_t b, uint32_t key, uint32_t ws) {
  return sid | (a << 5) | (b << 8) | (key << 11) | (ws << 12);
}
JSON_HD inline uint32_t json_sid(const JsonState& s) { return s.ctrl & 31u; }
JSON_HD inline void json_init(JsonState& s) { s.ctrl = J_START, s.depth = 0, s.stack = 0; }

// One byte.  False: the byte cannot continue the document; the state is then unchanged.
JSON_HD inline bool json_step(JsonState& s, uint8_t c) {
  uint32_t sid = s.ctrl & 31u;
  const uint32_t a = (s.ctrl >> 5) & 7u, b = (s.ctrl >> 8) & 7u, key = (s.ctrl >> 11) & 1u, ws = (s.ctrl >> 12) & 31u;
  const uint32_t depth = s.depth & 0xffu, seen = s.depth & ~0xffu;
  const bool is_ws = c == 0x20 || c == 0x09 || c == 0x0a || c == 0x0d;
  const bool digit = c >= '0' && c <= '9';

  // ---- strings: every byte is the string's own
  if (sid == J_STR) {
    if (c == '"') { s.ctrl = json_ctrl(key ? J_AFTER_KEY : J_AFTER_VALUE, 0, 0, 0, 0); return true; }
    if (c == '\\') { s.ctrl = json_ctrl(J_STR_ESC, 0, 0, key, 0); return true; }
    if (c < 0x20) return false;
    if (c < 0x80) return true;
    uint32_t owed, range = U_80_BF;
    if (c >= 0xc2 && c <= 0xdf) owed = 1;
    else if (c >= 0xe0 && c <= 0xef) owed = 2, range = c == 0xe0 ? U_A0_BF : c == 0xed ? U_80_9F : U_80_BF;
    else if (c >= 0xf0 && c <= 0xf4) owed = 3, range = c == 0xf0 ? U_90_BF : c == 0xf4 ? U_80_8F : U_80_BF;
    else return false;  // a continuation byte, C0, C1 or F5 .. FF as the first byte
    s.ctrl = json_ctrl(J_STR_UTF8, owed, range, key, 0);
    return true;
  }
  if (sid == J_STR_ESC) {
    if (c == 'u') { s.ctrl = json_ctrl(J_STR_HEX, 4, 0, key, 0); return true; }
    if (c == '"' || c == '\\' || c == '/' || c == 'b' || c == 'f' || c == 'n' || c == 'r' || c == 't') {
      s.ctrl = json_ctrl(J_STR, 0, 0, key, 0);
      return true;
    }
    return false;
  }
  if (sid == J_STR_HEX) {
    if (!(digit || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F'))) return false;
    s.ctrl = a > 1 ? json_ctrl(J_STR_HEX, a - 1, 0, key, 0) : json_ctrl(J_STR, 0, 0, key, 0);
    return true;
  }
  if (sid == J_STR_UTF8) {
    const uint8_t lo = b == U_A0_BF ? 0xa0 : b == U_90_BF ? 0x90 : 0x80;
    const uint8_t hi = b == U_80_9F ? 0x9f : b == U_80_8F ? 0x8f : 0xbf;
    if (c < lo || c > hi) return false;
    s.ctrl = a > 1 ? json_ctrl(J_STR_UTF8, a - 1, U_80_BF, key, 0) : json_ctrl(J_STR, 0, 0, key, 0);
    return true;
  }
  if (sid == J_LIT) {
    // the literal's bytes, first byte lowest: "true", "false", "null"
    const uint64_t word = b == 0 ? 0x65757274ull : b == 1 ? 0x65736c6166ull : 0x6c6c756eull;
    const uint32_t len = b == 1 ? 5 : 4;
    if (c != (uint8_t)(word >> (8 * a))) return false;
    s.ctrl = a + 1 < len ? json_ctrl(J_LIT, a + 1, b, 0, 0) : json_ctrl(J_AFTER_VALUE, 0, 0, 0, 0);
    return true;
  }
  // ---- numbers: a byte that extends the number, else (where the number may end) a byte of J_AFTER_VALUE
  if (sid >= J_NUM_MINUS && sid <= J_NUM_EXP) {
    const bool e = c == 'e' || c == 'E';
    uint32_t next = J_NSTATES;
    switch (sid) {
      case J_NUM_MINUS: next = c == '0' ? J_NUM_ZERO : digit ? J_NUM_INT : J_FAIL; break;
      case J_NUM_ZERO: next = c == '.' ? J_NUM_DOT : e ? J_NUM_E : J_NSTATES; break;
      case J_NUM_INT: next = digit ? J_NUM_INT : c == '.' ? J_NUM_DOT : e ? J_NUM_E : J_NSTATES; break;
      case J_NUM_DOT: next = digit ? J_NUM_FRAC : J_FAIL; break;
      case J_NUM_FRAC: next = digit ? J_NUM_FRAC : e ? J_NUM_E : J_NSTATES; break;
      case J_NUM_E: next = digit ? J_NUM_EXP : (c == '+' || c == '-') ? J_NUM_ESIGN : J_FAIL; break;
      case J_NUM_ESIGN: next = digit ? J_NUM_EXP : J_FAIL; break;
      default: next = digit ? J_NUM_EXP : J_NSTATES; break;  // J_NUM_EXP
    }
    if (next == J_FAIL) return false;
    if (next != J_NSTATES) { s.ctrl = json_ctrl(next, 0, 0, 0, 0); return true; }
    sid = J_AFTER_VALUE;  // the number ended before this byte (its whitespace run is empty)
  }
  // ---- between tokens
  if (sid == J_DONE || sid == J_FAIL) return false;
  if (is_ws) {
    if (ws >= JSON_WS_MAX) return false;  // (a number's states carry no run: its end starts one)
    s.ctrl = json_ctrl(sid, 0, 0, 0, ws + 1);
    return true;
  }
  const bool top_obj = depth > 0 && (s.stack & 1u);
  bool close = false;
  if (sid == J_START || sid == J_VALUE || sid == J_ARR_OPEN) {
    if (sid == J_ARR_OPEN && c == ']') close = true;
    else if (c == '{' || (c == '[' && sid != J_START)) {
      if (depth >= JSON_DEPTH_MAX) return false;
      s.stack = (s.stack << 1) | (c == '{' ? 1u : 0u);
      s.depth = seen | (depth + 1);
      s.ctrl = json_ctrl(c == '{' ? J_OBJ_OPEN : J_ARR_OPEN, 0, 0, 0, 0);
      return true;
    }
    else if (sid == J_START) return false;
    else if (c == '"') { s.ctrl = json_ctrl(J_STR, 0, 0, 0, 0); return true; }
    else if (c == '-') { s.ctrl = json_ctrl(J_NUM_MINUS, 0, 0, 0, 0); return true; }
    else if (c == '0') { s.ctrl = json_ctrl(J_NUM_ZERO, 0, 0, 0, 0); return true; }
    else if (digit) { s.ctrl = json_ctrl(J_NUM_INT, 0, 0, 0, 0); return true; }
    else if (c == 't' || c == 'f' || c == 'n') {
      s.ctrl = json_ctrl(J_LIT, 1, c == 't' ? 0 : c == 'f' ? 1 : 2, 0, 0);
      return true;
    }
    else return false;
  } else if (sid == J_OBJ_OPEN || sid == J_NEXT_KEY) {
    if (c == '"') { s.ctrl = json_ctrl(J_STR, 0, 0, 1, 0); return true; }
    if (!(sid == J_OBJ_OPEN && c == '}')) return false;
    close = true;
  } else if (sid == J_AFTER_KEY) {
    if (c != ':') return false;
    s.ctrl = json_ctrl(J_VALUE, 0, 0, 0, 0);
    return true;
  } else {  // J_AFTER_VALUE
    if (c == ',') { s.ctrl = json_ctrl(top_obj ? J_NEXT_KEY : J_VALUE, 0, 0, 0, 0); return true; }
    if (c != (top_obj ? '}' : ']')) return false;
    close = true;
  }
  if (!close) return false;
  s.stack >>= 1;
  s.depth = seen | (depth - 1);
  s.ctrl = json_ctrl(depth == 1 ? J_DONE : J_AFTER_VALUE, 0, 0, 0, 0);
  return true;
}

// Whether the bytes of one token continue the document from `s` (a copy advances; an empty piece never does).
JSON_HD inline bool json_token_ok(JsonState s, const uint8_t* p, int n) {
  if (n <= 0) return false;
  for (int i = 0; i < n; ++i)
    if (!json_step(s, p[i])) return false;
  return true;
}

// Consume one token.  False: it was not valid from `s`, which is then J_FAIL (depth and stack as they were).
JSON_HD inline bool json_advance(JsonState& s, const uint8_t* p, int n) {
  JsonState t = s;
  bool ok = n > 0;
  for (int i = 0; ok && i < n; ++i) ok = json_step(t, p[i]);
  if (!ok) {
    s.ctrl = json_ctrl(J_FAIL, 0, 0, 0, 0);
    return false;
  }
  t.depth += 0x100u;
  s = t;
  return true;
}
