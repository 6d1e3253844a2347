// Host program around ops/csrc/json_pda.h (the automaton of JSON mode), for tests/test_jsonmode_cpu.py.
// stdin: records of a 4-byte little-endian length and that many bytes.  stdout, one line per record:
//   <accept> <viable> <ctrl> <depth> <stack>
// accept: every byte valid and the state is J_DONE; viable: every byte valid; the state words are those after the
// last valid byte (decimal).  Each record is fed byte by byte through json_step, and again in pieces of 1 .. 3 bytes
// through json_token_ok / json_advance: the two must agree (exit code 2 otherwise).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "json_pda.h"

int main() {
  std::vector<uint8_t> buf;
  for (;;) {
    uint8_t h[4];
    if (fread(h, 1, 4, stdin) != 4) break;
    const uint32_t n = h[0] | (h[1] << 8) | (h[2] << 16) | ((uint32_t)h[3] << 24);
    buf.resize(n);
    if (n && fread(buf.data(), 1, n, stdin) != n) return 3;
    JsonState s;
    json_init(s);
    bool viable = true;
    for (uint32_t i = 0; i < n && viable; ++i) viable = json_step(s, buf[i]);
    // the same bytes as tokens
    JsonState t;
    json_init(t);
    bool tv = true;
    uint32_t tokens = 0;
    for (uint32_t i = 0, k = 1; i < n && tv; i += k, k = k % 3 + 1) {
      const int len = (int)(i + k <= n ? k : n - i);
      const bool ok = json_token_ok(t, buf.data() + i, len);
      tv = json_advance(t, buf.data() + i, len);
      if (ok != tv) return 2;
      tokens += tv;
    }
    if (tv != viable) return 2;
    if (viable && (t.ctrl != s.ctrl || t.stack != s.stack || t.depth != s.depth + (tokens << 8))) return 2;
    if (!viable && json_sid(t) != J_FAIL) return 2;
    if (json_token_ok(s, buf.data(), 0)) return 2;  // an empty piece is never ok
    printf("%d %d %u %u %llu\n", int(viable && json_sid(s) == J_DONE), int(viable), s.ctrl, s.depth,
           (unsigned long long)s.stack);
  }
  return 0;
}
