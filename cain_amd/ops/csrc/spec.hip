// Speculative decoding, self-drafting form (engine/speculative.py states the rule; these kernels implement exactly
// it): each decode step proposes up to K tokens per sequence, one ordinary forward over R (K + 1) rows verifies them,
// and the longest correct prefix is committed.
//
//   spec_draft_kernel   one workgroup per sequence.  n-gram mode: the record of the sequence's slot is read once,
//                       lane-linear (a wave instruction covers 256 contiguous bytes), each lane testing the 3- / 2- /
//                       1-token suffix match that ends at its position; a wave ballot per n-gram length and its
//                       highest set bit give "the largest i" without a scan.  Given mode: the caller's drafts.  Then
//                       the K + 1 expanded rows (token, position, slot, generated count, history ring with the drafts
//                       written in, sampling options) are written for the verify forward.
//   spec_accept_kernel  one wave per sequence: lane j holds the token the sampler drew for row j; a ballot finds the
//                       first draft that differs, lane 0 commits t_0 .. t_a with the sampler's advance_row semantics.
//   spec_model_rows_kernel / spec_model_next_kernel / spec_dvalid_kernel
//                       draft-model mode: the rows of the draft model's forwards (first forward from the decode state,
//                       forward j + 1 from the sampler's output of forward j, which also goes into `given`) and the
//                       per-slot count of draft-cache positions that hold the sequence's own tokens.
//
// Integer work only, plain vector loads and stores, no atomics.
#include "cain_api.h"

#include <stdint.h>

namespace {

constexpr int SPEC_THREADS = 256;
constexpr int SPEC_HIST = 64;     // sample.hip HIST
constexpr int SPEC_PARAM_DW = 12;  // sizeof(SampleParams) / 4 (cain_sample_params_size)

// sample.hip SampleParams, the fields the commit needs
struct SpecStops {
  int eos_id;
  int stop[3];
};
__device__ __forceinline__ SpecStops load_stops(const uint32_t* params, int r) {
  const uint32_t* p = params + (size_t)r * SPEC_PARAM_DW;
  return SpecStops{int(p[5]), {int(p[6]), int(p[7]), int(p[8])}};
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_draft_kernel(CainSpec s, int T_max, const int* __restrict__ tok,
                                                                 const int* __restrict__ pos,
                                                                 const int* __restrict__ slot,
                                                                 const int* __restrict__ n_gen,
                                                                 const int* __restrict__ max_new,
                                                                 const int* __restrict__ done,
                                                                 const int* __restrict__ hist,
                                                                 const uint32_t* __restrict__ params) {
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = s.K, K1 = K + 1;
  const int sl = slot[r], p = pos[r], ng = n_gen[r], mn = max_new[r], dn = done[r];
  __shared__ int s_best[3][SPEC_THREADS / 64];
  __shared__ int s_draft[SPEC_K_MAX + 1];
  __shared__ int s_d;
  // drafts this sequence may have: none when it is done, masked or (never in a sound state) outside its buffers
  int cap = 0;
  if (sl >= 0 && sl < s.slots && !dn && p >= 0 && p < T_max && ng >= 0)
    cap = max(0, min(K, min(T_max - 1 - p, mn - 1 - ng)));
  const bool lookup = s.mode == 0 && cap > 0 && p >= 1;  // (uniform over the workgroup)
  if (lookup) {
    const int* q = s.seq + (size_t)sl * s.lds;
    const int s0 = q[p], s1 = q[p - 1], s2 = p >= 2 ? q[p - 2] : 0;
    int b1 = -1, b2 = -1, b3 = -1;
    for (int i0 = wave * 64; i0 < p; i0 += SPEC_THREADS) {  // ascending: a later chunk's match replaces an earlier one
      const int i = i0 + lane;
      const bool m1 = i < p && q[i] == s0;
      const bool m2 = m1 && p >= 2 && i >= 1 && q[i - 1] == s1;
      const bool m3 = m2 && p >= 3 && i >= 2 && q[i - 2] == s2;
      const unsigned long long v1 = __ballot(m1), v2 = __ballot(m2), v3 = __ballot(m3);
      if (v1) b1 = i0 + 63 - __clzll((long long)v1);
      if (v2) b2 = i0 + 63 - __clzll((long long)v2);
      if (v3) b3 = i0 + 63 - __clzll((long long)v3);
    }
    if (lane == 0) s_best[0][wave] = b1, s_best[1][wave] = b2, s_best[2][wave] = b3;
  }
  __syncthreads();
  if (tid == 0) {
    int d = 0;
    if (lookup) {
      const int* q = s.seq + (size_t)sl * s.lds;
      for (int n = 3; n >= 1 && d == 0; --n) {
        int best = -1;
        for (int w = 0; w < SPEC_THREADS / 64; ++w) best = max(best, s_best[n - 1][w]);
        if (best >= 0) {
          d = min(cap, p - best);  // seq[best + 1 .. min(best + K, pos)], clipped
          for (int j = 1; j <= d; ++j) s_draft[j] = q[best + j];
        }
      }
    } else if (s.mode == 1 && s.given) {
      for (int j = 1; j <= cap; ++j) {
        const int at = ng + j - 1;
        const int v = at < s.ldv ? s.given[(size_t)r * s.ldv + at] : -1;
        if (v < 0 || v >= s.vocab) break;
        s_draft[j] = v;
        d = j;
      }
    }
    s_d = d;
    s.nd[r] = d;
    for (int j = 1; j <= K; ++j) s.draft[r * K + j - 1] = j <= d ? s_draft[j] : -1;
  }
  __syncthreads();
  const int d = s_d;
  if (tid < K1) {
    const int j = tid, x = r * K1 + j;
    const bool on = j <= d;  // (row 0 always: d >= 0)
    s.x_tok[x] = j == 0 ? tok[r] : on ? s_draft[j] : 0;
    s.x_pos[x] = j == 0 ? p : on ? p + j : 0;
    s.x_slot[x] = j == 0 ? sl : on ? sl : -1;
    s.x_n_gen[x] = j == 0 ? ng : on ? ng + j : 0;
    s.x_max_new[x] = j == 0 ? mn : on ? 0x7fffffff : 0;
    s.x_done[x] = j == 0 ? dn : 0;
  }
  // row j's history ring: the sequence's with draft[1 .. j] at indices (ng .. ng + j - 1) & 63
  for (int e = tid; e < K1 * SPEC_HIST; e += SPEC_THREADS) {
    const int j = e >> 6, h = e & (SPEC_HIST - 1);
    int v = hist[(size_t)r * SPEC_HIST + h];
    if (j <= d)
      for (int jj = 1; jj <= j; ++jj)
        if (((ng + jj - 1) & (SPEC_HIST - 1)) == h) v = s_draft[jj];
    s.x_hist[((size_t)r * K1 + j) * SPEC_HIST + h] = v;
  }
  // every row samples with the sequence's options (the stream is keyed by seed and generated index, not by row)
  uint32_t* xp = static_cast<uint32_t*>(s.x_params);
  for (int e = tid; e < K1 * SPEC_PARAM_DW; e += SPEC_THREADS)
    xp[(size_t)r * K1 * SPEC_PARAM_DW + e] = params[(size_t)r * SPEC_PARAM_DW + e % SPEC_PARAM_DW];
}

__global__ __launch_bounds__(64) void spec_accept_kernel(CainSpec s, int T_max, int* __restrict__ tok,
                                                         int* __restrict__ pos, const int* __restrict__ slot,
                                                         int* __restrict__ n_gen, const int* __restrict__ max_new,
                                                         int* __restrict__ done, int* __restrict__ hist,
                                                         int* __restrict__ gen, int ldg,
                                                         const uint32_t* __restrict__ params) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int K = s.K, K1 = K + 1;
  const int sl = slot[r];
  if (sl < 0 || sl >= s.slots || done[r]) return;  // (uniform) nothing sampled, nothing committed
  const int d = min(max(s.nd[r], 0), K);
  const int t = lane <= d ? s.x_tok[r * K1 + lane] : -1;  // what the sampler drew for row `lane`
  const int before = __shfl_up(t, 1, 64);
  const int dr = lane >= 1 && lane <= d ? s.draft[r * K + lane - 1] : -1;
  const unsigned long long bad = __ballot(lane >= 1 && lane <= d && before != dr);
  const int a = bad ? __ffsll((long long)bad) - 2 : d;  // drafts 1 .. a are the tokens rows 0 .. a - 1 drew
  const SpecStops P = load_stops(params, r);
  int ng = n_gen[r], p = pos[r], c = 0, last = 0, dn = 0;
  const int mn = max_new[r];
  for (int i = 0; i <= a && !dn && ng < ldg; ++i) {
    const int choice = __shfl(t, i, 64);
    if (lane == 0) {  // sample.hip advance_row, per committed token
      gen[(size_t)r * ldg + ng] = choice;
      hist[(size_t)r * SPEC_HIST + (ng & (SPEC_HIST - 1))] = choice;
      if (p + 1 < T_max) s.seq[(size_t)sl * s.lds + p + 1] = choice;
    }
    ++ng, ++c, last = choice;
    const bool stop = (P.eos_id >= 0 && choice == P.eos_id) || (P.stop[0] >= 0 && choice == P.stop[0]) ||
                      (P.stop[1] >= 0 && choice == P.stop[1]) || (P.stop[2] >= 0 && choice == P.stop[2]);
    if (stop || ng >= mn || p + 1 >= T_max) dn = 1; else ++p;
  }
  if (lane == 0 && c > 0) {
    n_gen[r] = ng;
    tok[r] = last;
    pos[r] = p;
    if (dn) done[r] = 1;
    s.drafted[r] += d;
    s.accepted[r] += c - 1;
    const int k = s.n_step[r];
    s.step_tokens[(size_t)r * s.ldt + k % s.ldt] = c;
    s.n_step[r] = k + 1;
  }
}

// ---- draft-model mode (spec.h CainSpecDraft; engine/speculative.py "Draft model") ----------------------------------
constexpr int SPEC_NO_BUDGET = 0x7fffffff;

__device__ __forceinline__ int draft_token(const CainSpecDraft& s, int t) {
  return t >= 0 && t < s.dvocab ? t : s.dbos;  // the draft embedding is never indexed out of range
}

__device__ __forceinline__ void draft_row(const CainSpecDraft& s, int x, int tok, int pos, int slot, int n_gen,
                                          int max_new, int done) {
  s.r_tok[x] = tok, s.r_pos[x] = pos, s.r_slot[x] = slot, s.r_n_gen[x] = n_gen, s.r_max_new[x] = max_new;
  s.r_done[x] = done;
}

// The rows of the first draft forward, one workgroup per sequence: row r is the sequence's own token at `pos`, sampled
// with the request's options (stop ids off, no budget); row R + r the catch-up at pos - 1, run (KV only: it is
// marked done, which the sampler skips) when the slot's draft cache ends one position short.  A sequence that drafts
// nothing (done, masked, or on its last token) has both rows masked.
__global__ __launch_bounds__(SPEC_THREADS) void spec_model_rows_kernel(CainSpecDraft s, int R, int T_max,
                                                                      const int* __restrict__ tok,
                                                                      const int* __restrict__ pos,
                                                                      const int* __restrict__ slot,
                                                                      const int* __restrict__ n_gen,
                                                                      const int* __restrict__ max_new,
                                                                      const int* __restrict__ done,
                                                                      const int* __restrict__ hist,
                                                                      const uint32_t* __restrict__ params) {
  const int r = blockIdx.x, tid = threadIdx.x;
  const int sl = slot[r], p = pos[r], ng = n_gen[r], mn = max_new[r], dn = done[r];
  const bool live = sl >= 0 && sl < s.slots && !dn && p >= 0 && p < T_max && ng >= 0;
  const int d = live ? max(0, min(s.K, min(T_max - 1 - p, mn - 1 - ng))) : 0;
  if (tid == 0) {
    s.p0[r] = p;
    s.nd[r] = d;
    if (live && d < s.K && ng + d < s.ldv) s.given[(size_t)r * s.ldv + ng + d] = -1;
    const bool catch_up = d > 0 && p >= 1 && s.dvalid[sl] == p - 1;
    if (d > 0) draft_row(s, r, draft_token(s, tok[r]), p, sl, ng, SPEC_NO_BUDGET, 0);
    else draft_row(s, r, 0, 0, -1, 0, 0, 0);
    if (catch_up) draft_row(s, R + r, draft_token(s, s.seq[(size_t)sl * s.lds + p - 1]), p - 1, sl, ng, SPEC_NO_BUDGET, 1);
    else draft_row(s, R + r, 0, 0, -1, 0, 0, 0);
  }
  for (int e = tid; e < 2 * SPEC_HIST; e += SPEC_THREADS) {
    const int x = e < SPEC_HIST ? r : R + r, h = e & (SPEC_HIST - 1);
    s.r_hist[(size_t)x * SPEC_HIST + h] = hist[(size_t)r * SPEC_HIST + h];
  }
  uint32_t* xp = static_cast<uint32_t*>(s.r_params);
  for (int e = tid; e < 2 * SPEC_PARAM_DW; e += SPEC_THREADS) {
    const int x = e < SPEC_PARAM_DW ? r : R + r, w = e % SPEC_PARAM_DW;
    xp[(size_t)x * SPEC_PARAM_DW + w] = w >= 5 && w <= 8 ? 0xffffffffu : params[(size_t)r * SPEC_PARAM_DW + w];
  }
}

// After the sampler of draft forward j (1 .. K): d_j, the token it left in row r, goes into `given` at generated index
// ng + j - 1 and into the row's ring, and row r becomes the input of forward j + 1 -- or is masked when j + 1 > d.
__global__ __launch_bounds__(64) void spec_model_next_kernel(CainSpecDraft s, int R, int j,
                                                             const int* __restrict__ slot,
                                                             const int* __restrict__ n_gen) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= R) return;
  const int d = s.nd[r];
  if (d <= 0 || j > d) return;  // the row is masked already
  const int ng = n_gen[r], dj = s.r_tok[r];
  if (ng + j - 1 < s.ldv) s.given[(size_t)r * s.ldv + ng + j - 1] = dj;
  s.r_hist[(size_t)r * SPEC_HIST + ((ng + j - 1) & (SPEC_HIST - 1))] = dj;
  if (j + 1 <= d) draft_row(s, r, draft_token(s, dj), s.p0[r] + j, slot[r], ng + j, SPEC_NO_BUDGET, 0);
  else draft_row(s, r, 0, 0, -1, 0, 0, 0);
}

// After accept: positions pos0 .. pos0 + d - 1 of the slot's draft cache hold the sequence's token and d_1 .. d_{d-1};
// those below the sequence's new position are tokens of its record.
__global__ __launch_bounds__(64) void spec_dvalid_kernel(CainSpecDraft s, int R, const int* __restrict__ slot,
                                                         const int* __restrict__ pos) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= R) return;
  const int d = s.nd[r], sl = slot[r];
  if (d > 0 && sl >= 0 && sl < s.slots) s.dvalid[sl] = min(s.p0[r] + d, pos[r]);
}

int spec_model_ok(const CainSpecDraft* s, int R, int T_max) {
  if (!s || R < 1 || s->K < 1 || s->K > SPEC_K_MAX || T_max < 1) return 0;
  if (s->dvocab < 1 || s->dbos < 0 || s->dbos >= s->dvocab || s->slots < 1 || s->lds < T_max || s->ldv < 1 ||
      s->ldg < 1)
    return 0;
  return s->seq && s->given && s->dvalid && s->p0 && s->nd && s->r_tok && s->r_pos && s->r_slot && s->r_n_gen &&
         s->r_max_new && s->r_done && s->r_hist && s->r_gen && s->r_params;
}

int spec_ok(const CainSpec* s, int R, int T_max) {
  if (!s || R < 1 || s->K < 1 || s->K > SPEC_K_MAX || (s->mode != 0 && s->mode != 1)) return 0;
  if (s->slots < 1 || s->lds < T_max || T_max < 1 || s->ldt < 1 || s->ldg < 1 || s->vocab < 1) return 0;
  if (s->mode == 1 && (!s->given || s->ldv < 1)) return 0;
  return s->seq && s->x_tok && s->x_pos && s->x_slot && s->x_n_gen && s->x_max_new && s->x_done && s->x_hist &&
         s->x_gen && s->x_params && s->nd && s->draft && s->drafted && s->accepted && s->n_step && s->step_tokens;
}

}  // namespace

// Rows [0, R) of the decode state -> the expanded state of `s` (R (K + 1) rows), drafts into s->nd / s->draft.
CAIN_API int cain_spec_draft(const CainSpec* s, int R, int T_max, const int* tok, const int* pos, const int* slot,
                             const int* n_gen, const int* max_new, const int* done, const int* hist,
                             const void* params, hipStream_t st) {
  if (!spec_ok(s, R, T_max) || !tok || !pos || !slot || !n_gen || !max_new || !done || !hist || !params) return -1;
  hipLaunchKernelGGL(spec_draft_kernel, dim3(R), dim3(SPEC_THREADS), 0, st, *s, T_max, tok, pos, slot, n_gen, max_new,
                     done, hist, static_cast<const uint32_t*>(params));
  return int(hipGetLastError());
}

// After the sampler ran over the expanded rows: commit each sequence's accepted tokens to rows [0, R).
CAIN_API int cain_spec_accept(const CainSpec* s, int R, int T_max, int* tok, int* pos, const int* slot, int* n_gen,
                              const int* max_new, int* done, int* hist, int* gen, int ldg, const void* params,
                              hipStream_t st) {
  if (!spec_ok(s, R, T_max) || !tok || !pos || !slot || !n_gen || !max_new || !done || !hist || !gen || ldg < 1 ||
      !params)
    return -1;
  hipLaunchKernelGGL(spec_accept_kernel, dim3(R), dim3(64), 0, st, *s, T_max, tok, pos, slot, n_gen, max_new, done,
                     hist, gen, ldg, static_cast<const uint32_t*>(params));
  return int(hipGetLastError());
}

CAIN_API int cain_spec_size() { return int(sizeof(CainSpec)); }

// Draft-model mode.  Rows [0, R) of the decode state -> the 2 R rows of the first draft forward.
CAIN_API int cain_spec_model_rows(const CainSpecDraft* s, int R, int T_max, const int* tok, const int* pos,
                                  const int* slot, const int* n_gen, const int* max_new, const int* done,
                                  const int* hist, const void* params, hipStream_t st) {
  if (!spec_model_ok(s, R, T_max) || !tok || !pos || !slot || !n_gen || !max_new || !done || !hist || !params)
    return -1;
  hipLaunchKernelGGL(spec_model_rows_kernel, dim3(R), dim3(SPEC_THREADS), 0, st, *s, R, T_max, tok, pos, slot, n_gen,
                     max_new, done, hist, static_cast<const uint32_t*>(params));
  return int(hipGetLastError());
}

// After draft forward j's sampler: d_j into `given`, rows [0, R) become the input of forward j + 1.
CAIN_API int cain_spec_model_next(const CainSpecDraft* s, int R, int j, int T_max, const int* slot, const int* n_gen,
                                  hipStream_t st) {
  if (!spec_model_ok(s, R, T_max) || j < 1 || j > s->K || !slot || !n_gen) return -1;
  hipLaunchKernelGGL(spec_model_next_kernel, dim3((R + 63) / 64), dim3(64), 0, st, *s, R, j, slot, n_gen);
  return int(hipGetLastError());
}

// After cain_spec_accept: the slots' dvalid from the sequences' new positions.
CAIN_API int cain_spec_dvalid(const CainSpecDraft* s, int R, int T_max, const int* slot, const int* pos,
                              hipStream_t st) {
  if (!spec_model_ok(s, R, T_max) || !slot || !pos) return -1;
  hipLaunchKernelGGL(spec_dvalid_kernel, dim3((R + 63) / 64), dim3(64), 0, st, *s, R, slot, pos);
  return int(hipGetLastError());
}

CAIN_API int cain_spec_draft_size() { return int(sizeof(CainSpecDraft)); }
