// Stop sequences (Ollama's options.stop), the rule stated once: plain C++ with no HIP types -- hipcc compiles it for
// both sides, g++ compiles it alone (tests/csrc/stop_match_host.cpp).  engine/stopseq.py states the same rule in
// Python, word for word.
//
// A row has 0 .. STOP_MAX stop strings of 1 .. STOP_LEN_MAX bytes each (stop_len[k]: 0 for an unused entry;
// stop_bytes[k][0 .. stop_len[k])).  Matching is on bytes.  The row's stream is the concatenation of its generated
// tokens' pieces, in order; an empty piece (a special token) adds nothing.
//
// Advance over one token: append its piece and consider every occurrence of any stop string that ends inside this
// token's bytes (it may start in earlier tokens, at most STOP_LEN_MAX - 1 bytes back: the tail).  None: the state
// moves on.  Else the row is done on this token: hit_start is the smallest start offset among those occurrences,
// hit_which the lowest string index among the occurrences that start there.  The token counts as consumed either way
// (tail, n_tok and n_bytes move over its whole piece).
//
// Per-row state, 48 bytes:
//   tail       the last STOP_LEN_MAX - 1 bytes of the stream, the newest at tail[30] (0 where the stream is shorter);
//              tail[31] is 0
//   n_tok      tokens consumed (the advance kernel tells a row that generated this step from one that did not by it)
//   n_bytes    bytes consumed
//   hit_start  -1, or the byte offset in the stream where the text is cut
//   hit_which  -1, or the index of the matched string
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define STOP_HD __host__ __device__
#else
#define STOP_HD
#endif

#define STOP_MAX 8
#define STOP_LEN_MAX 32
#define STOP_TAIL (STOP_LEN_MAX - 1)
#define STOP_NONE 0x7fffffff

struct StopState {
  uint8_t tail[STOP_LEN_MAX];
  int32_t n_tok;
  int32_t n_bytes;
  int32_t hit_start;
  int32_t hit_which;
};

STOP_HD inline void stop_init(StopState& s) {
  for (int i = 0; i < STOP_LEN_MAX; ++i) s.tail[i] = 0;
  s.n_tok = 0, s.n_bytes = 0, s.hit_start = -1, s.hit_which = -1;
}

// Byte r of (tail, piece): r in [-STOP_TAIL, n), negative r reach back into the tail.
STOP_HD inline uint8_t stop_byte(const uint8_t* tail, const uint8_t* p, int r) {
  return r < 0 ? tail[STOP_TAIL + r] : p[r];
}

// The occurrences that end on byte j of the piece (0 <= j < n): the smallest key (start - piece start + STOP_TAIL) * 8 +
// index among them, or STOP_NONE.  Ordering by key is ordering by (start, index).  n_bytes: stream bytes before the
// piece -- an occurrence cannot start before the stream does.
STOP_HD inline int stop_match_end(const uint8_t* tail, int n_bytes, const uint8_t* p, int j, const int32_t* stop_len,
                                  const uint8_t* stop_bytes) {
  int best = STOP_NONE;
  for (int k = 0; k < STOP_MAX; ++k) {
    const int ls = stop_len[k];
    if (ls < 1 || ls > STOP_LEN_MAX) continue;
    const int r0 = j - ls + 1;  // >= -STOP_TAIL
    if (r0 < 0 && n_bytes < -r0) continue;
    const uint8_t* s = stop_bytes + k * STOP_LEN_MAX;
    bool eq = true;
    for (int i = ls - 1; eq && i >= 0; --i) eq = s[i] == stop_byte(tail, p, r0 + i);  // the newest byte first
    if (eq) {
      const int key = (r0 + STOP_TAIL) * STOP_MAX + k;
      best = key < best ? key : best;
    }
  }
  return best;
}

// Byte i (0 .. STOP_TAIL - 1) of the tail after a piece of n bytes.
STOP_HD inline uint8_t stop_next_tail(const uint8_t* tail, const uint8_t* p, int n, int i) {
  return stop_byte(tail, p, n - STOP_TAIL + i);  // n >= 0: never further back than the tail
}

// Consume one token (n >= 0 bytes).  True: a stop string ended inside it (hit_start / hit_which are set).
STOP_HD inline bool stop_advance(StopState& s, const uint8_t* p, int n, const int32_t* stop_len,
                                 const uint8_t* stop_bytes) {
  int best = STOP_NONE;
  for (int j = 0; j < n; ++j) {
    const int key = stop_match_end(s.tail, s.n_bytes, p, j, stop_len, stop_bytes);
    best = key < best ? key : best;
  }
  uint8_t t[STOP_LEN_MAX];
  for (int i = 0; i < STOP_TAIL; ++i) t[i] = stop_next_tail(s.tail, p, n, i);
  t[STOP_TAIL] = 0;
  for (int i = 0; i < STOP_LEN_MAX; ++i) s.tail[i] = t[i];
  if (best != STOP_NONE) {
    s.hit_start = s.n_bytes + best / STOP_MAX - STOP_TAIL;
    s.hit_which = best % STOP_MAX;
  }
  s.n_tok += 1;
  s.n_bytes += n;
  return best != STOP_NONE;
}
