// Stop sequences (Ollama's options.stop) matched inside the captured decode graphs: one launch of a decode step,
// after the sampler (and after JSON mode's advance, which may take the sampled token back), runtime.hip CainStop.
//
// The rule is stop_match.h's; a row's StopState (48 bytes) lives in `sstate`, its strings in stop_len [M][8] /
// stop_bytes [M][8][32].  The vocabulary is JSON mode's piece table: token t appends
// piece_bytes[piece_off[t] .. piece_off[t + 1]) to the row's stream (empty: a special token).
//
//   stop_advance_kernel   one wave per row.  The state counts the tokens it has consumed, so a row that generated
//       nothing this step (done before it, or its token taken back by json_advance) has n_gen == that count and is
//       left alone, as is a row with stop_on == 0: neither its state nor done / n_gen is written.  Otherwise the row
//       consumes gen[m][n_gen[m] - 1]: the lanes split the end positions of the token's bytes (lane, lane + 64, ...:
//       vocabularies have whitespace runs longer than a wave), each lane tests the up to 8 strings against
//       tail + piece from the newest byte back (stop_match_end), one wave reduction takes the minimum of
//       (start, index), and the lanes write the state back: 31 lanes the new tail, one lane each the counters.  A hit
//       sets done[m]; the token stays in gen and n_gen is not reduced.  The old tail, the lengths and the strings sit in
//       LDS (320 bytes); the piece's bytes are read from the table (consecutive lanes, consecutive bytes).
//
// Every value is written with ordinary vector stores; workgroups never talk.
#include "common.h"
#include "stop_match.h"

namespace {

__global__ __launch_bounds__(64) void stop_advance_kernel(int V, const int* __restrict__ stop_on,
                                                          const int* __restrict__ gen, int ldg,
                                                          const int* __restrict__ n_gen, int* __restrict__ done,
                                                          StopState* __restrict__ sstate,
                                                          const int32_t* __restrict__ stop_len,
                                                          const uint8_t* __restrict__ stop_bytes,
                                                          const int* __restrict__ piece_off,
                                                          const uint8_t* __restrict__ piece_bytes) {
  __shared__ __attribute__((aligned(16))) uint8_t tail[STOP_LEN_MAX];
  __shared__ int32_t len[STOP_MAX];
  __shared__ __attribute__((aligned(16))) uint8_t str[STOP_MAX * STOP_LEN_MAX];
  const int m = blockIdx.x, lane = threadIdx.x;
  if (!stop_on[m]) return;  // (every exit before the reduction is the same for the whole wave)
  StopState* S = sstate + m;
  const int ng = n_gen[m], seen = S->n_tok, nb = S->n_bytes;
  if (S->hit_start >= 0 || ng < 1 || ng > ldg || ng != seen + 1) return;  // no new token this step
  const int tok = gen[(size_t)m * ldg + ng - 1];
  if (lane < STOP_LEN_MAX) tail[lane] = S->tail[lane];
  if (lane < STOP_MAX) len[lane] = stop_len[m * STOP_MAX + lane];
  reinterpret_cast<uint32_t*>(str)[lane] =
      reinterpret_cast<const uint32_t*>(stop_bytes + (size_t)m * STOP_MAX * STOP_LEN_MAX)[lane];
  int n = 0;
  const uint8_t* p = piece_bytes;
  if (tok >= 0 && tok < V) {  // an id outside the table appends nothing
    const int o0 = piece_off[tok];
    n = piece_off[tok + 1] - o0;
    n = n > 0 ? n : 0;
    p += o0;
  }
  __syncthreads();
  int best = STOP_NONE;
  for (int j = lane; j < n; j += 64) {
    const int key = stop_match_end(tail, nb, p, j, len, str);
    best = key < best ? key : best;
  }
  for (int o = 32; o >= 1; o >>= 1) {  // all 64 lanes are here; the minimum ends up in every one of them
    const int other = __shfl_xor(best, o, 64);
    best = other < best ? other : best;
  }
  if (lane < STOP_TAIL) S->tail[lane] = stop_next_tail(tail, p, n, lane);
  if (lane == 32) S->n_tok = seen + 1;
  if (lane == 33) S->n_bytes = nb + n;
  if (best != STOP_NONE) {
    if (lane == 34) S->hit_start = nb + best / STOP_MAX - STOP_TAIL;
    if (lane == 35) S->hit_which = best % STOP_MAX;
    if (lane == 36) done[m] = 1;
  }
}

}  // namespace

CAIN_API int cain_stop_state_size() { return int(sizeof(StopState)); }
CAIN_API int cain_stop_max() { return STOP_MAX; }
CAIN_API int cain_stop_len_max() { return STOP_LEN_MAX; }

// After the sampler (and after cain_json_advance).  gen [M][ldg]; sstate [M] StopState; stop_len [M][8] int32;
// stop_bytes [M][8][32]; V: entries of the piece table (piece_off holds V + 1).  Refuses (-1, nothing launched) null
// pointers, M < 1, a V beyond what a piece table can hold (2^23, JSON mode's limit) and ldg < 1.
CAIN_API int cain_stop_advance(int M, int V, const int* stop_on, const int* gen, int ldg, const int* n_gen, int* done,
                               void* sstate, const int32_t* stop_len, const uint8_t* stop_bytes, const int* piece_off,
                               const uint8_t* piece_bytes, hipStream_t st) {
  if (!stop_on || !gen || !n_gen || !done || !sstate || !stop_len || !stop_bytes || !piece_off || !piece_bytes)
    return -1;
  if (M < 1 || V < 1 || V > (1 << 23) || ldg < 1) return -1;
  hipLaunchKernelGGL(stop_advance_kernel, dim3(M), dim3(64), 0, st, V, stop_on, gen, ldg, n_gen, done,
                     static_cast<StopState*>(sstate), stop_len, stop_bytes, piece_off, piece_bytes);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
