// Embedding pooling (CainStep::pool; README "Embeddings").
//
// An embedding is the model's hidden state -- the residual stream after the last layer under the model's own final
// RMSNorm with its own gain, what the LM head multiplies before any fold -- pooled over a prompt's positions: `last`
// takes position n - 1, `mean` the fp32 sum over positions 0 .. n - 1 in ascending order divided by n; the pooled
// vector is then L2-normalised.
//
// cain_pool_rows: two launches on the stream.  pool_rinv_kernel, one workgroup per row, reduces the row's sum of
// squares exactly as rmsnorm_kernel (norm.hip) does -- 16-byte loads, wave shuffle then LDS -- into rinv[row].
// pool_acc_kernel, a grid of (runs, d / 2048), gives each thread 8 columns of one run: it walks the run's rows in
// ascending order with the loads of four rows issued ahead, so a sequence's sum is one serial chain per column
// whatever the chunking (bitwise the same wherever the calls cut it), with no float atomics and no reduction inside
// the loop.  The two roundings of a term and the one of its accumulation are separate instructions (contraction off).
// cain_pool_finish: one workgroup per sequence, acc / cnt and the L2 normalisation.
#include "common.h"

namespace {

constexpr int POOL_D_MAX = 16384;

template <int THREADS>
__device__ __forceinline__ float pool_block_sum(float v, float* sh) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) sh[w] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < THREADS / 64; ++i) t += sh[i];
  return t;
}

// rinv[r] = rms_inv(sum of squares of row r).  Mean mode: the grid is the M rows.  Last mode (seg_off non-null): the
// grid is the S runs, each workgroup takes its run's final row (none of an empty run).
template <int THREADS>
__global__ __launch_bounds__(THREADS) void pool_rinv_kernel(const __bf16* __restrict__ x, int ldx, int M, int d,
                                                            float eps, const int* __restrict__ seg_off,
                                                            float* __restrict__ rinv) {
  __shared__ float sh[THREADS / 64];
  int m = blockIdx.x;
  if (seg_off) {
    const int r0 = seg_off[blockIdx.x], r1 = seg_off[blockIdx.x + 1];
    if (r1 <= r0) return;
    m = r1 - 1;
  }
  if (m < 0 || m >= M) return;
  const bf16x8* xr = reinterpret_cast<const bf16x8*>(x + (size_t)m * ldx);
  const int nv = d >> 3;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // the order of rmsnorm_kernel's sum
    const int idx = threadIdx.x + i * THREADS;
    if (idx < nv) {
      const bf16x8 v = xr[idx];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = bf2f(v[j]);
        ss += f * f;
      }
    }
  }
  const float tot = pool_block_sum<THREADS>(ss, sh);
  if (threadIdx.x == 0) rinv[m] = rms_inv(tot, d, eps);
}

// term = (float(x) * inv) * gain: two roundings.  hipcc contracts a * b + c into an FMA by default, and did so for
// some rows of the unrolled loop and not for others (the sums then depended on where a call cut a sequence):
// contraction is off in everything that forms or adds a term.
__device__ __forceinline__ float pool_term(__bf16 x, float inv, float g) {
#pragma clang fp contract(off)
  return (bf2f(x) * inv) * g;
}
__device__ __forceinline__ float pool_add(float a, float t) {
#pragma clang fp contract(off)
  return a + t;
}

__global__ __launch_bounds__(256) void pool_acc_kernel(const __bf16* __restrict__ x, int ldx, int M, int d,
                                                       const float* __restrict__ gain,
                                                       const int* __restrict__ seg_off,
                                                       const int* __restrict__ seg_dst, int mode,
                                                       float* __restrict__ acc, int* __restrict__ cnt,
                                                       const float* __restrict__ rinv) {
#pragma clang fp contract(off)
  const int s = blockIdx.x;
  int r0 = seg_off[s], r1 = seg_off[s + 1];
  r0 = r0 < 0 ? 0 : r0;
  r1 = r1 > M ? M : r1;
  if (r1 <= r0) return;  // an empty run touches nothing
  const int dst = seg_dst[s];
  if (blockIdx.y == 0 && threadIdx.x == 0) cnt[dst] = mode == POOL_LAST ? 1 : cnt[dst] + (r1 - r0);
  const int c0 = (blockIdx.y * 256 + threadIdx.x) * 8;
  if (c0 >= d) return;
  const f32x4 g0 = *reinterpret_cast<const f32x4*>(gain + c0), g1 = *reinterpret_cast<const f32x4*>(gain + c0 + 4);
  float* ap = acc + (size_t)dst * d + c0;
  const __bf16* xc = x + c0;
  float a[8];
  if (mode == POOL_LAST) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(xc + (size_t)(r1 - 1) * ldx);
    const float inv = rinv[r1 - 1];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = pool_term(v[j], inv, j < 4 ? g0[j] : g1[j - 4]);
  } else {
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(ap), a1 = *reinterpret_cast<const f32x4*>(ap + 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = j < 4 ? a0[j] : a1[j - 4];
    int r = r0;
    for (; r + 4 <= r1; r += 4) {  // four rows' loads in flight, added in ascending order
      bf16x8 v[4];
      float inv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = *reinterpret_cast<const bf16x8*>(xc + (size_t)(r + i) * ldx);
        inv[i] = rinv[r + i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = pool_add(a[j], pool_term(v[i][j], inv[i], j < 4 ? g0[j] : g1[j - 4]));
    }
    for (; r < r1; ++r) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(xc + (size_t)r * ldx);
      const float inv = rinv[r];
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = pool_add(a[j], pool_term(v[j], inv, j < 4 ? g0[j] : g1[j - 4]));
    }
  }
  *reinterpret_cast<f32x4*>(ap) = f32x4{a[0], a[1], a[2], a[3]};
  *reinterpret_cast<f32x4*>(ap + 4) = f32x4{a[4], a[5], a[6], a[7]};
}

// out[b] = v or v / sqrt(sum v^2), v = acc[b] / float(cnt[b]).  Each thread sums the squares of its elements (index
// tid, tid + 256, ...) serially with one FMA per element, then wave shuffle and a serial sum over the four waves: at
// most d / 256 + 6 + 3 roundings on the longest path, each add of a zero partial exact.
__global__ __launch_bounds__(256) void pool_finish_kernel(const float* __restrict__ acc, const int* __restrict__ cnt,
                                                          float* __restrict__ out, int d, int normalize) {
  __shared__ float sh[4];
  const int b = blockIdx.x;
  const int n = cnt[b];
  if (n == 0) return;  // (uniform over the workgroup)
  const float fn = float(n);
  const float* ar = acc + (size_t)b * d;
  float* orow = out + (size_t)b * d;
  float ss = 0.f;
  for (int c = threadIdx.x; c < d; c += 256) {
    const float v = __fdiv_rn(ar[c], fn);
    ss = __fmaf_rn(v, v, ss);
  }
  const float tot = pool_block_sum<256>(ss, sh);
  const float nrm = __fsqrt_rn(tot);
  const bool scale = normalize && nrm > 0.f;  // a zero vector stays zero
  for (int c = threadIdx.x; c < d; c += 256) {
    const float v = __fdiv_rn(ar[c], fn);
    orow[c] = scale ? __fdiv_rn(v, nrm) : v;
  }
}

}  // namespace

CAIN_API int cain_pool_rows(const void* x, int ldx, int M, int d, const float* gain, float eps, const int* seg_off,
                            const int* seg_dst, int S, int mode, float* acc, int* cnt, float* rinv, hipStream_t st) {
  if (d < 8 || d % 8 || d > POOL_D_MAX || ldx % 8 || ldx < d || S < 0 || M < 0 || !gain) return -1;
  if (!x || !seg_off || !seg_dst || !acc || !cnt || !rinv || (mode != POOL_MEAN && mode != POOL_LAST)) return -1;
  if (S == 0 || M == 0) return 0;
  const __bf16* xb = static_cast<const __bf16*>(x);
  const int* so = mode == POOL_LAST ? seg_off : nullptr;
  const int rows = mode == POOL_LAST ? S : M;
  if (d <= 4 * 8 * 256)
    hipLaunchKernelGGL(pool_rinv_kernel<256>, dim3(rows), dim3(256), 0, st, xb, ldx, M, d, eps, so, rinv);
  else
    hipLaunchKernelGGL(pool_rinv_kernel<512>, dim3(rows), dim3(512), 0, st, xb, ldx, M, d, eps, so, rinv);
  hipLaunchKernelGGL(pool_acc_kernel, dim3(S, cdiv(d, 2048)), dim3(256), 0, st, xb, ldx, M, d, gain, seg_off, seg_dst,
                     mode, acc, cnt, rinv);
  return int(hipGetLastError());
}

CAIN_API int cain_pool_finish(const float* acc, const int* cnt, float* out, int B, int d, int normalize,
                              hipStream_t st) {
  if (d < 1 || B < 0 || !acc || !cnt || !out) return -1;
  if (B == 0) return 0;
  hipLaunchKernelGGL(pool_finish_kernel, dim3(B), dim3(256), 0, st, acc, cnt, out, d, normalize);
  return int(hipGetLastError());
}

CAIN_API int cain_pool_size() { return int(sizeof(CainPool)); }
