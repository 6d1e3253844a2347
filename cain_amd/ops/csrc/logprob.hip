// Token log-probabilities on device: log-softmax statistics of fp32 logits rows, the top-n alternatives and the
// log-probability of one chosen token per row.
//
// Definition: a token's logprob is the natural-log softmax of the model's own logits -- temperature 1, before the
// repeat penalty and before top-k / top-p.  The top-n alternatives are the n most likely ids of that distribution,
// ordered by logit descending and index ascending on ties (the samplers' order, sample.hip rank_candidates).
//
// Three uses of two kernels:
//   (a) logprob_rows_kernel before the sampler of a decode step: (max, log sum) of the row, its top-n into the per-row
//       rings at the index of the token about to be generated (n_gen[m]), and a per-row record (LpKeep) of what the
//       sampler is about to destroy or advance: n_gen, whether the row was live, and the RAW logits of the <= 64 ids
//       of its history ring -- sample_kernel / sample_cm_kernel apply the repeat penalty to exactly those ids in place
//       in the logits buffer;
//   (b) logprob_chosen_kernel after the sampler: the logprob of the token the sampler wrote (gen[m][n_gen before]),
//       its raw logit taken from the record when the id is one of the history ids and from the buffer otherwise (ids
//       outside the history are never modified).  Nothing is ever recomputed by undoing the penalty;
//   (c) logprob_rows_kernel with a target id per row (teacher forcing, DecodeEngine.score): no sampler, the target's
//       logprob comes straight from the row; results are indexed by row.
//
// logprob_rows_kernel: one 1024-thread workgroup per row.  Pass 1 reads the row with 16-byte loads; each thread keeps
// an online (max, sum of exp) pair and its own maximum element, the pairs are merged across lanes (shuffles) and waves
// (LDS).  Top-n (n <= 20): the n-th largest of the 1024 thread maxima is a threshold that keeps every top-n element
// (the n largest thread maxima are n distinct elements >= it), pass 2 gathers the elements >= it into LDS (the row
// is L2-resident: <= 1 MB) and ranks them.  More than LP_CAP such elements (long runs of equal values) take n
// selection passes over the row instead, each the block-wide best element after the previous one in the order.
// Either way the order is exact.  Every value is written with ordinary vector stores; workgroups never talk.
#include "common.h"

namespace {

constexpr int LP_THREADS = 1024;
constexpr int LP_WAVES = LP_THREADS / 64;
constexpr int LP_TOP = 20;    // top_logprobs limit (entries per token in the rings)
constexpr int LP_CAP = 1024;  // gathered candidates pass 2 can rank
constexpr int LP_HIST = 64;   // sample.hip HIST

// What (a) keeps of a decode row for (b).
struct LpKeep {
  int live;   // the row was wanted and live before the sampler ran
  int ng;     // n_gen before the sampler: index of this step's token in the rings
  int nh;     // history ids recorded
  float mx;   // row maximum
  float ls;   // log of the sum of exp(x - mx)
  int pad[3];
  int ids[LP_HIST];
  float raw[LP_HIST];
};

// (value descending, index ascending): a before b
__device__ __forceinline__ bool lp_before(float va, int ia, float vb, int ib) {
  return va > vb || (va == vb && ia < ib);
}

// Block-wide best (value, index) in the order above; every thread calls it and gets the result.  `buf` alternates
// between calls (0 / 1), so one barrier per call is enough.
__device__ __forceinline__ void block_best(float& v, int& i, float (*red_v)[LP_WAVES], int (*red_i)[LP_WAVES],
                                           int buf) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (lp_before(ov, oi, v, i)) { v = ov; i = oi; }
  }
  if ((threadIdx.x & 63) == 0) { red_v[buf][threadIdx.x >> 6] = v; red_i[buf][threadIdx.x >> 6] = i; }
  __syncthreads();
  v = red_v[buf][0];
  i = red_i[buf][0];
#pragma unroll
  for (int w = 1; w < LP_WAVES; ++w) {
    const float ov = red_v[buf][w];
    const int oi = red_i[buf][w];
    if (lp_before(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

__global__ __launch_bounds__(LP_THREADS) void logprob_rows_kernel(
    const float* __restrict__ logits, int ldl, int V, const int* __restrict__ slot, const int* __restrict__ done,
    const int* __restrict__ topn, const int* __restrict__ n_gen, const int* __restrict__ hist, int ldg,
    const int* __restrict__ target, float* __restrict__ lse, float* __restrict__ lp, int* __restrict__ top_id,
    float* __restrict__ top_lp, LpKeep* __restrict__ keep) {
  const int m = blockIdx.x;
  const int tid = threadIdx.x;
  const int want = topn[m];
  const int ng = n_gen ? n_gen[m] : 0;
  // rows not wanted write nothing (a decode row's record only says so); a decode row whose ring is full neither
  if ((slot && slot[m] < 0) || (done && done[m]) || want < 0 || (n_gen && (ng < 0 || ng >= ldg))) {
    if (keep && tid == 0) keep[m].live = 0;
    return;
  }
  const size_t out = n_gen ? (size_t)m * ldg + ng : (size_t)m;  // ring entry (decode) or row (teacher forcing)
  const float* lg = logits + (size_t)m * ldl;
  const f32x4* lg4 = reinterpret_cast<const f32x4*>(lg);
  const int V4 = V >> 2;  // V % 4 == 0 (the entry refuses anything else)

  __shared__ float red_v[2][LP_WAVES];
  __shared__ int red_i[2][LP_WAVES];
  __shared__ float red_m[LP_WAVES], red_s[LP_WAVES];
  __shared__ __attribute__((aligned(16))) float cval[LP_CAP];
  __shared__ __attribute__((aligned(16))) int cidx[LP_CAP];
  __shared__ int s_nc;

  // ---- pass 1: online (max, sum) and the thread's maximum element; 4 16-byte loads in flight per thread
  float mx = -INFINITY, sum = 0.f;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int base = tid; base < V4; base += 4 * LP_THREADS) {
    f32x4 c[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // unconditional loads; chunks past the row re-read the row's last chunk
      const int i4 = base + u * LP_THREADS;
      c[u] = lg4[i4 < V4 ? i4 : V4 - 1];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i4 = base + u * LP_THREADS;
      if (i4 < V4) {
        const float cm = fmaxf(fmaxf(c[u][0], c[u][1]), fmaxf(c[u][2], c[u][3]));
        if (cm > mx) {
          sum = mx == -INFINITY ? 0.f : sum * expf(mx - cm);
          mx = cm;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          sum += expf(c[u][j] - mx);
          if (c[u][j] > bv) { bv = c[u][j]; bi = i4 * 4 + j; }
        }
      }
    }
  }
  // merge across lanes, then waves
  float wm = mx, wsum = sum;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(wm, o, 64);
    const float os = __shfl_xor(wsum, o, 64);
    const float nm = fmaxf(wm, om);
    wsum = (wm == -INFINITY ? 0.f : wsum * expf(wm - nm)) + (om == -INFINITY ? 0.f : os * expf(om - nm));
    wm = nm;
  }
  if ((tid & 63) == 0) { red_m[tid >> 6] = wm; red_s[tid >> 6] = wsum; }
  __syncthreads();
  float M = red_m[0];
#pragma unroll
  for (int w = 1; w < LP_WAVES; ++w) M = fmaxf(M, red_m[w]);
  float S = 0.f;
#pragma unroll
  for (int w = 0; w < LP_WAVES; ++w) S += red_m[w] == -INFINITY ? 0.f : red_s[w] * expf(red_m[w] - M);
  const float LS = logf(S);

  if (tid == 0) {
    if (lse) lse[m] = M + LS;
    if (target) {
      const int t = target[m];
      if (t >= 0 && t < V) lp[out] = (lg[t] - M) - LS;
    }
  }
  if (keep) {
    // the raw logits of the history ring's ids (the newest min(64, n_gen) generated ids: a superset of what any
    // repeat_last_n lets the sampler penalise)
    const int nh = ng < LP_HIST ? ng : LP_HIST;
    if (tid < nh) {
      const int id = hist[(size_t)m * LP_HIST + ((ng - 1 - tid) & (LP_HIST - 1))];
      keep[m].ids[tid] = id;
      keep[m].raw[tid] = (id >= 0 && id < V) ? lg[id] : 0.f;
    }
    if (tid == 0) {
      keep[m].live = 1;
      keep[m].ng = ng;
      keep[m].nh = nh;
      keep[m].mx = M;
      keep[m].ls = LS;
    }
  }

  int K = want < LP_TOP ? want : LP_TOP;
  if (K > V) K = V;
  if (K == 0) return;
  int* o_id = top_id + out * LP_TOP;
  float* o_lp = top_lp + out * LP_TOP;

  // ---- threshold: the K-th largest thread maximum (K rounds of a block-wide best over the maxima not yet taken)
  float tau = -INFINITY;
  {
    bool taken = false;
    for (int r = 0; r < K; ++r) {
      float v = taken ? -INFINITY : bv;
      int i = taken ? 0x7fffffff : tid;
      block_best(v, i, red_v, red_i, r & 1);
      if (i == tid) taken = true;
      tau = v;
    }
  }
  // ---- pass 2: gather the elements >= tau
  if (tid == 0) s_nc = 0;
  __syncthreads();
  for (int base = tid; base < V4; base += 4 * LP_THREADS) {
    f32x4 c[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i4 = base + u * LP_THREADS;
      c[u] = lg4[i4 < V4 ? i4 : V4 - 1];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i4 = base + u * LP_THREADS;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i4 < V4 && c[u][j] >= tau) {
          const int k = atomicAdd(&s_nc, 1);
          if (k < LP_CAP) { cval[k] = c[u][j]; cidx[k] = i4 * 4 + j; }
        }
    }
  }
  __syncthreads();
  const int nc = s_nc;
  if (nc <= LP_CAP) {
    // rank the candidates; the first K in order are the row's top K
    for (int a = tid; a < nc; a += LP_THREADS) {
      const float va = cval[a];
      const int ia = cidx[a];
      int r = 0;
      for (int b = 0; b < nc; ++b) r += lp_before(cval[b], cidx[b], va, ia);
      if (r < K) { o_id[r] = ia; o_lp[r] = (va - M) - LS; }
    }
    return;
  }
  // ---- too many elements tie with the threshold: K selection passes, each the best element after the previous
  float pv = INFINITY;
  int pi = -1;
  for (int r = 0; r < K; ++r) {
    float v = -INFINITY;
    int ix = 0x7fffffff;
    for (int i4 = tid; i4 < V4; i4 += LP_THREADS) {
      const f32x4 c = lg4[i4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int id = i4 * 4 + j;
        if (lp_before(pv, pi, c[j], id) && lp_before(c[j], id, v, ix)) { v = c[j]; ix = id; }
      }
    }
    block_best(v, ix, red_v, red_i, r & 1);
    if (tid == 0) { o_id[r] = ix; o_lp[r] = (v - M) - LS; }
    pv = v;
    pi = ix;
  }
}

// (b): one wave per row; lane j holds history id j, so the lookup is one compare and a ballot.
__global__ __launch_bounds__(64) void logprob_chosen_kernel(const float* __restrict__ logits, int ldl, int V,
                                                            const int* __restrict__ gen, int ldg,
                                                            const LpKeep* __restrict__ keep, float* __restrict__ lp) {
  const int m = blockIdx.x;
  const int lane = threadIdx.x;
  const LpKeep& k = keep[m];
  if (!k.live) return;
  const size_t at = (size_t)m * ldg + k.ng;
  const int id = gen[at];
  if (id < 0 || id >= V) return;
  const int hid = lane < k.nh ? k.ids[lane] : -1;
  const float hraw = lane < k.nh ? k.raw[lane] : 0.f;
  const float braw = logits[(size_t)m * ldl + id];  // right unless the id is a history id: those the sampler may write
  const unsigned long long hit = __ballot(hid == id);
  const int src = hit ? __ffsll((long long)hit) - 1 : 0;
  const float kept = __shfl(hraw, src, 64);  // equal ids hold equal raw values: any hit will do
  if (lane == 0) lp[at] = ((hit ? kept : braw) - k.mx) - k.ls;
}

bool lp_args_ok(const void* logits, int ldl, int V, int M, int nmax) {
  return logits && M >= 1 && V >= 4 && V % 4 == 0 && ldl >= V && ldl % 4 == 0 &&
         (reinterpret_cast<uintptr_t>(logits) & 15) == 0 && nmax >= 0 && nmax <= LP_TOP;
}

}  // namespace

CAIN_API int cain_logprob_top_max() { return LP_TOP; }
CAIN_API long long cain_logprob_keep_bytes(int M) { return (long long)(M > 0 ? M : 0) * (long long)sizeof(LpKeep); }

// Row statistics, teacher-forced when `target` is given: lse[m] (may be null), lp[m] of target[m], the top topn[m]
// (id, logprob) pairs at top_id / top_lp[m * 20 + j].  `nmax`: the largest topn of the call as the host knows it (the
// kernel clamps the device array to 20 whatever it holds).  slot / done may be null (every row live).  Refuses (-1,
// nothing launched) V % 4 != 0, ldl < V, ldl % 4 != 0 (rows must start 16-byte aligned) and nmax outside 0..20.
CAIN_API int cain_logprob_rows(const float* logits, int ldl, int V, int M, const int* slot, const int* done,
                               const int* topn, int nmax, const int* target, float* lse, float* lp, int* top_id,
                               float* top_lp, hipStream_t st) {
  if (!lp_args_ok(logits, ldl, V, M, nmax) || !topn || (target && !lp) || (nmax > 0 && (!top_id || !top_lp))) return -1;
  hipLaunchKernelGGL(logprob_rows_kernel, dim3(M), dim3(LP_THREADS), 0, st, logits, ldl, V, slot, done, topn,
                     (const int*)nullptr, (const int*)nullptr, 0, target, lse, lp, top_id, top_lp, (LpKeep*)nullptr);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// (a) of a decode step, before the sampler: top-n into the rings at n_gen[m] (top_id / top_lp[(m * ldg + n) * 20 + j])
// and the record `keep` (cain_logprob_keep_bytes(M)) for cain_logprob_chosen.
CAIN_API int cain_logprob_pre(const float* logits, int ldl, int V, int M, const int* slot, const int* done,
                              const int* topn, int nmax, const int* n_gen, const int* hist, int ldg, int* top_id,
                              float* top_lp, void* keep, hipStream_t st) {
  if (!lp_args_ok(logits, ldl, V, M, nmax) || !topn || !n_gen || !hist || !keep || ldg < 1 || !top_id || !top_lp)
    return -1;
  hipLaunchKernelGGL(logprob_rows_kernel, dim3(M), dim3(LP_THREADS), 0, st, logits, ldl, V, slot, done, topn, n_gen,
                     hist, ldg, (const int*)nullptr, (float*)nullptr, (float*)nullptr, top_id, top_lp,
                     static_cast<LpKeep*>(keep));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// (b) after the sampler: lp[m * ldg + n] of the token the sampler wrote at gen[m * ldg + n], n = the row's n_gen
// before the step.
CAIN_API int cain_logprob_chosen(const float* logits, int ldl, int V, int M, const int* gen, int ldg, const void* keep,
                                 float* lp, hipStream_t st) {
  if (!lp_args_ok(logits, ldl, V, M, 0) || !gen || !keep || !lp || ldg < 1) return -1;
  hipLaunchKernelGGL(logprob_chosen_kernel, dim3(M), dim3(64), 0, st, logits, ldl, V, gen, ldg,
                     static_cast<const LpKeep*>(keep), lp);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
