// stop_match.h on the host (tests/test_stopseq_cpu.py): reads cases from stdin, advances a StopState over each case's
// pieces until a hit, and prints the 48 state bytes in hex and the hit flag after every token.
//
// stdin, little-endian, until EOF: u32 number of strings (<= 8), per string u32 length (1 .. 32) and its bytes;
// u32 number of pieces, per piece u32 length and its bytes.  stdout: one line per consumed token, "--" after a case.
#include <cstdio>
#include <cstring>
#include <vector>

#include "stop_match.h"

static bool read_u32(uint32_t& v) {
  unsigned char b[4];
  if (fread(b, 1, 4, stdin) != 4) return false;
  v = b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
  return true;
}

int main() {
  static_assert(sizeof(StopState) == 48, "StopState is 48 bytes");
  uint32_t ns;
  while (read_u32(ns)) {
    int32_t len[STOP_MAX] = {0};
    uint8_t bytes[STOP_MAX * STOP_LEN_MAX] = {0};
    if (ns > STOP_MAX) return 2;
    for (uint32_t k = 0; k < ns; ++k) {
      uint32_t n;
      if (!read_u32(n) || n < 1 || n > STOP_LEN_MAX) return 2;
      if (fread(bytes + k * STOP_LEN_MAX, 1, n, stdin) != n) return 2;
      len[k] = (int32_t)n;
    }
    uint32_t np;
    if (!read_u32(np)) return 2;
    StopState s;
    stop_init(s);
    bool hit = false;
    for (uint32_t i = 0; i < np; ++i) {
      uint32_t n;
      if (!read_u32(n)) return 2;
      std::vector<uint8_t> piece(n);  // exactly n bytes: a read past the piece is the sanitizer's to catch
      if (n && fread(piece.data(), 1, n, stdin) != n) return 2;
      if (hit) continue;
      hit = stop_advance(s, piece.data(), (int)n, len, bytes);
      unsigned char raw[sizeof(StopState)];
      memcpy(raw, &s, sizeof(s));
      for (unsigned char c : raw) printf("%02x", c);
      printf(" %d\n", (int)hit);
    }
    printf("--\n");
  }
  return 0;
}
