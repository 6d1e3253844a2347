// JSON mode (Ollama's format "json") as an on-device grammar mask: two launches of a decode step, one between the LM
// head and the sampler, one after the sampler, both inside the captured decode graphs (runtime.hip CainGrammar).
//
// The rule is json_pda.h's automaton; a row's JsonState (16 bytes) lives in `gstate`.  The vocabulary is a piece table:
// token t appends piece_bytes[piece_off[t] .. piece_off[t + 1]) to the output (empty: a special token, never allowed).
//
//   json_mask_kernel      one thread per (row, token): walks the token's bytes from the row's state; a token that
//       cannot continue the document gets the logit -(2^100 * (1 + t / 2^23)), about -1e30 -- distinct per token and
//       decreasing with t, so no sampler kernel sees a new tie whatever its top_k, index-ascending order is kept, and
//       exp() of it is exactly 0 at any sane temperature (below ~3e-9 the scaled value overflows to -inf).  (Not
//       -inf, not one constant: a hundred thousand equal values at a top-k threshold is a case the samplers'
//       threshold tightening was never run on.)  Accepted tokens' logits are not written.  With `cmax` (the LM head's 16-column chunk maxima, which the chunk-max and lean samplers
//       start from) the row's maxima are rewritten from the masked logits: the 16 tokens of a chunk are the 16 lanes
//       of one DPP row, so the maximum is four row rotations.  Rows that are off (gram_on 0) or done are neither read
//       nor written.
//   json_advance_kernel   one thread per row: consumes the token the sampler just wrote, gen[m][n_gen[m] - 1].  The
//       state counts the tokens it has consumed, so a row that generated nothing this step (done before it) has
//       n_gen == that count and is left alone.  Reaching J_DONE sets done[m]: the closing brace is the row's last
//       token, no EOS id needed.  A token that is not valid from the state -- the sampler's fall-back to its last
//       candidate when its final prefix sum rounds below the draw, ~2^-24 per step without top-p -- is taken back
//       (n_gen[m] -= 1), the state becomes J_FAIL and done[m] is set: no output ever holds an invalid token.
//
// Every value is written with ordinary vector stores; workgroups never talk.
#include "common.h"
#include "json_pda.h"

namespace {

constexpr int GM_THREADS = 256;

template <int CTRL>
__device__ __forceinline__ float row_ror(float v) {  // DPP row_ror: rotate within each row of 16 lanes
  return __builtin_bit_cast(float,
                            __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

__global__ __launch_bounds__(GM_THREADS) void json_mask_kernel(float* __restrict__ logits, int ldl, int V,
                                                               const int* __restrict__ gram_on,
                                                               const int* __restrict__ done,
                                                               const JsonState* __restrict__ gstate,
                                                               const int* __restrict__ piece_off,
                                                               const uint8_t* __restrict__ piece_bytes,
                                                               float* __restrict__ cmax) {
  const int m = blockIdx.y;
  if (!gram_on[m] || done[m]) return;  // the same for every thread of the row
  const int t = blockIdx.x * GM_THREADS + threadIdx.x;
  const bool in = t < V;
  float v = -INFINITY;
  if (in) {
    const JsonState s = gstate[m];
    const int o0 = piece_off[t], o1 = piece_off[t + 1];
    float* p = logits + (size_t)m * ldl + t;
    v = *p;
    if (!json_token_ok(s, piece_bytes + o0, o1 - o0)) {
      v = -__uint_as_float((227u << 23) | (uint32_t)t);
      *p = v;
    }
  }
  if (cmax) {  // V % 16 == 0: a chunk is whole, its 16 lanes are one DPP row; every lane of the wave is active here
    v = fmaxf(v, row_ror<0x128>(v));
    v = fmaxf(v, row_ror<0x124>(v));
    v = fmaxf(v, row_ror<0x122>(v));
    v = fmaxf(v, row_ror<0x121>(v));
    if (in && (t & 15) == 0) cmax[(size_t)m * (V >> 4) + (t >> 4)] = v;
  }
}

__global__ __launch_bounds__(64) void json_advance_kernel(int M, int V, const int* __restrict__ gram_on,
                                                          const int* __restrict__ gen, int ldg,
                                                          int* __restrict__ n_gen, int* __restrict__ done,
                                                          JsonState* __restrict__ gstate,
                                                          const int* __restrict__ piece_off,
                                                          const uint8_t* __restrict__ piece_bytes) {
  const int m = blockIdx.x * 64 + threadIdx.x;
  if (m >= M || !gram_on[m]) return;
  JsonState s = gstate[m];
  const uint32_t sid = json_sid(s);
  if (sid == J_DONE || sid == J_FAIL) return;
  const int ng = n_gen[m];
  if (ng < 1 || ng > ldg || (uint32_t)ng != (s.depth >> 8) + 1u) return;  // no new token: done before this step
  const int tok = gen[(size_t)m * ldg + ng - 1];
  bool ok = tok >= 0 && tok < V;
  if (ok) {
    const int o0 = piece_off[tok];
    ok = json_advance(s, piece_bytes + o0, piece_off[tok + 1] - o0);
  } else {
    s.ctrl = json_ctrl(J_FAIL, 0, 0, 0, 0);
  }
  gstate[m] = s;
  if (!ok) {
    n_gen[m] = ng - 1;
    done[m] = 1;
  } else if (json_sid(s) == J_DONE) {
    done[m] = 1;
  }
}

}  // namespace

CAIN_API int cain_json_state_size() { return int(sizeof(JsonState)); }
CAIN_API int cain_json_vocab_max() { return 1 << 23; }

// Before the sampler.  logits [M][ldl] fp32; gstate [M] JsonState; piece_off [V + 1]; cmax [M][V / 16] or null.
// Refuses (-1, nothing launched) V > 2^23 (the masked value carries the id in the mantissa), ldl < V, and chunk
// maxima of a V that is not whole 16-column chunks.
CAIN_API int cain_json_mask(float* logits, int ldl, int V, int M, const int* gram_on, const int* done,
                            const void* gstate, const int* piece_off, const uint8_t* piece_bytes, float* cmax,
                            hipStream_t st) {
  if (!logits || !gram_on || !done || !gstate || !piece_off || !piece_bytes) return -1;
  if (M < 1 || M > 65535 || V < 1 || V > (1 << 23) || ldl < V || (cmax && V % 16)) return -1;
  hipLaunchKernelGGL(json_mask_kernel, dim3(cdiv(V, GM_THREADS), M), dim3(GM_THREADS), 0, st, logits, ldl, V, gram_on,
                     done, static_cast<const JsonState*>(gstate), piece_off, piece_bytes, cmax);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// After the sampler.  gen [M][ldg]; V: entries of the piece table (a token id outside it is an invalid token).
CAIN_API int cain_json_advance(int M, int V, const int* gram_on, const int* gen, int ldg, int* n_gen, int* done,
                               void* gstate, const int* piece_off, const uint8_t* piece_bytes, hipStream_t st) {
  if (!gram_on || !gen || !n_gen || !done || !gstate || !piece_off || !piece_bytes) return -1;
  if (M < 1 || V < 1 || V > (1 << 23) || ldg < 1) return -1;
  hipLaunchKernelGGL(json_advance_kernel, dim3(cdiv(M, 64)), dim3(64), 0, st, M, V, gram_on, gen, ldg, n_gen, done,
                     static_cast<JsonState*>(gstate), piece_off, piece_bytes);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
