// W8A8 wide-batch GEMM (fp8 e4m3 weights x fp8 e4m3 activations, fp32 accumulate) for 16 < M <= 256 rows, gfx950.
//
//   Y[m][n] = epilogue( xs[m] * ws[n] * sum_k X8[m][k] * W8[n][k] )
//
// xs: per-row activation scale (amax / 448, times the RMSNorm factor rsqrt(mean(x^2) + eps) for the normed
// projections), written by quant_rows_kernel from the bf16 rows; ws: per-output-row weight scale
// (models/weights.py quantize_fp8_rows).  The reference runs its models 4-bit quantised inside Ollama
// (BASELINE.md); this is the MI355X 8-bit counterpart for the trial-batched decode step, reported
// as its own configuration (bf16 stays the headline).
//
// The LDS-DMA ring and its loader waves, the split-K slabs, the combine and the epilogues are the bf16 kernel's
// (wgemm_ring.h: RingLoader, wg_store_slab16, wg_split, the launch helpers), and so are the LDS images: a
// ring stage is still one 128-B line per X row and 8 x 2 KiB of W, but it now spans 128 k, and
// its two 16-B fragment reads per operand (the bf16 kernel's two 32-k slices) are concatenated into the 32-B
// operands of one block-scaled v_mfma_scale_f32_16x16x128_f8f6f4 (unit e8m0 scales): per k twice the MFMA rate
// of bf16 and half the bytes through HBM, the per-CU load path and LDS.  A and B only need the same k order in
// their 32 bytes: lane (r, g) holds k = 64h + 16g + j (h = read 0/1, j < 16) of the stage in both -- W by its
// packing (pack_mfma_a_fp8_k128: [N/16][K/64][64 lanes][16 B]), X by the XOR-swizzled piece reads.
//
// FP4 = true is the W4A8 form for MXFP4 weights (the reference's 4-bit precision class at trial-batch widths):
// the SAME packed bytes as the few-row W4A16 kernel (models/weights.py pack_mxfp4: [N/16][K/128][64 lanes][16 B],
// lane (r, g) = row 16t + r, k = 128p + 32g + j at nibble j), which are exactly the fp4 A operand of the 16x16x128
// scaled MFMA (cbsz 4: 16 B per lane), and the block scales ([N/16][K/128][64] e8m0 bytes, one per lane = one
// 32-k block) go in as the MFMA's per-lane A scale.  A ring stage is 8 tiles x 1 KiB of W plus their 512 B of
// scales; X (fp8 rows) is read as pieces 2g, 2g + 1 of its 128-B line, the lane's 32 k.  Y = xs[m] * sum.
#include "wgemm_ring.h"

using namespace wg;

namespace {

constexpr int W8_BK = 128;  // k per ring stage (one 128-B X line per row, one scaled MFMA per tile pair)

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ i32x8 cat16(const i32x4& lo, const i32x4& hi) {
  return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

}  // namespace

struct W8Scales {
  const float* xs;  // [M] per-row activation scale
  const float* ws;  // [N] per-output-row weight scale
};

// Scales of one lane's four outputs: rows n = 16 gt + 4 (lane >> 4) + i of W, activation row m (FP4: the weight
// scales were applied inside the MFMA).
template <bool FP4 = false>
__device__ __forceinline__ f32x4 w8_scaled(f32x4 v, const W8Scales& q, int gt, int m, int lane, int M) {
  const float x = q.xs[min(m, M - 1)];
  if constexpr (FP4) return v * x;
  const f32x4 w = *reinterpret_cast<const f32x4*>(q.ws + gt * 16 + (lane >> 4) * 4);
  return v * w * x;
}

// ring loader: fp8 16 W blocks per stage as bf16; fp4 8 blocks + 8 x 64 B of scales, as dword pieces
template <int BM, int DX, int DW, int NDMA, bool FP4>
using W8Ring = RingLoader<BM, DX, DW, NDMA, FP4 ? WG_NT : 16, FP4 ? WG_NT * 1024 + WG_NT * 64 : WgGeo<BM>::W_BYTES,
                          FP4 ? 4 : 0>;

template <int BM, int DX, int DW, int EPI, int NDMA, bool FP4 = false>
__global__ __launch_bounds__(64 * (8 + NDMA), (8 + NDMA) / 4) void wgemm8_kernel(const GemmArgs a, const WgArgs w,
                                                                                  const W8Scales q) {
  using G = WgGeo<BM>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool compute = wave < 8;
  const int wm = wave % G::WM, wn = (wave / G::WM) % G::WN;
  const int ntiles = a.N >> 4;
  const int nblk = (ntiles + WG_NT - 1) / WG_NT;

  int blk, kc;
  wg_block_of(blockIdx.x, w.ks, nblk, w.xcd_blk, blk, kc);
  const int tile0 = blk * WG_NT;
  const int st0 = kc * w.kst;
  const int nst = min(w.kst, (a.K >> 7) - st0);
  // W per tile: fp8 K / 64 blocks of 1 KiB (16 rows x 64 k), two per stage; fp4 K / 128 blocks (16 rows x 128 k)
  // and as many 64-B scale groups, one per stage.  X: e4m3 rows of ldx bytes.
  const W8Ring<BM, DX, DW, NDMA, FP4> ring(smem, wave, lane, a.Wp, FP4 ? a.K >> 7 : a.K >> 6, FP4 ? st0 : st0 * 2,
                                          reinterpret_cast<const char*>(a.X) + (size_t)st0 * W8_BK, a.ldx, a.M,
                                          ntiles, tile0, nst, q.ws);

  const int c = lane & 15, g = lane >> 4;
  int woff[G::TN];
#pragma unroll
  for (int tn = 0; tn < G::TN; ++tn) woff[tn] = (wn * G::TN + tn) * (FP4 ? 1024 : 2048) + lane * 16;
  // X pieces 4h + g: k = 64h + 16g + j, the fp8 B operand's own k order (measured, tools/w4a8_probe.py: byte 16h + j
  // of lane group g meets k 64h + 16g + j of A) -- the fp8 W packing uses the same order; the fp4 A operand holds
  // k = 32g + j at nibble j, which is pack_mxfp4's order
  int xoff[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) xoff[h] = c * 128 + (((4 * h + g) ^ (c >> 1)) << 4);
  const int xrow0 = wm * G::MB * 16 * 128;

  f32x4 acc[G::TN][G::MB];
#pragma unroll
  for (int tn = 0; tn < G::TN; ++tn)
#pragma unroll
    for (int mb = 0; mb < G::MB; ++mb) acc[tn][mb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // one barrier per stage for every wave; after barrier t the loaders refill stage t - 1's slots (every wave's
  // reads of stage t - 1 completed before it: lgkmcnt(0) in ring_barrier)
  if (NDMA && !compute) {  // loader waves: their own loop, so the two roles' registers never overlap
    ring.loader_loop();
  } else {
    if constexpr (!NDMA) ring.prologue();
    for (int t = 0; t < nst; ++t) {
      if constexpr (!NDMA) ring.land(t);
      ring_barrier();
      if constexpr (!NDMA) ring.issue_step(t);
      const char* wbase = ring.w_slot(t);
      const char* xbase = ring.x_slot(t) + xrow0;
      i32x4 b0[G::MB], b1[G::MB], a0[G::TN], a1[G::TN];
      int sa[G::TN];
#pragma unroll
      for (int mb = 0; mb < G::MB; ++mb) {
        b0[mb] = *reinterpret_cast<const i32x4*>(xbase + mb * 2048 + xoff[0]);
        b1[mb] = *reinterpret_cast<const i32x4*>(xbase + mb * 2048 + xoff[1]);
      }
#pragma unroll
      for (int tn = 0; tn < G::TN; ++tn) {
        a0[tn] = *reinterpret_cast<const i32x4*>(wbase + woff[tn]);
        if constexpr (FP4)
          sa[tn] = *reinterpret_cast<const uint8_t*>(wbase + WG_NT * 1024 + (wn * G::TN + tn) * 64 + lane);
        else
          a1[tn] = *reinterpret_cast<const i32x4*>(wbase + 1024 + woff[tn]);
      }
#pragma unroll
      for (int tn = 0; tn < G::TN; ++tn) {
        if constexpr (FP4) {
          const i32x8 av = i32x8{a0[tn][0], a0[tn][1], a0[tn][2], a0[tn][3], 0, 0, 0, 0};  // 16 B of e2m1
#pragma unroll
          for (int mb = 0; mb < G::MB; ++mb)
            acc[tn][mb] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, cat16(b0[mb], b1[mb]), acc[tn][mb],
                                                                           4, 0, 0, sa[tn], 0, 127);
        } else {
          const i32x8 av = cat16(a0[tn], a1[tn]);
#pragma unroll
          for (int mb = 0; mb < G::MB; ++mb)
            acc[tn][mb] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, cat16(b0[mb], b1[mb]), acc[tn][mb],
                                                                           0, 0, 0, 127, 0, 127);
        }
      }
    }
  }
  ring_barrier();
  if (!compute) return;

  // every output gets its row scales (w8_scaled); tiles past N keep their (unused) sums
  if (w.ks > 1) {
    // slabs in fp16 as the bf16 kernel's, already scaled (the scales are linear, so the reduce sums scaled
    // partials): the raw e4m3 x e4m3 sums would overflow fp16
    const int n_units = nblk * WG_NT * G::RB;
#pragma unroll
    for (int tn = 0; tn < G::TN; ++tn)
#pragma unroll
      for (int mb = 0; mb < G::MB; ++mb) {
        const int gt = tile0 + wn * G::TN + tn;
        const int unit = gt * G::RB + wm * G::MB + mb;
        const int m = (wm * G::MB + mb) * 16 + c;
        wg_store_slab16(w.part, wg_slab_at(kc, n_units, unit, lane), acc[tn][mb], [&](const f32x4& v) {
          return gt < ntiles ? w8_scaled<FP4>(v, q, gt, m, lane, a.M) : v;
        });
      }
    return;
  }
#pragma unroll
  for (int tn = 0; tn < G::TN; ++tn) {
    const int gt = tile0 + wn * G::TN + tn;
#pragma unroll
    for (int mb = 0; mb < G::MB; ++mb) {
      const int m = (wm * G::MB + mb) * 16 + c;
      f32x4 v = gt < ntiles ? w8_scaled<FP4>(acc[tn][mb], q, gt, m, lane, a.M) : acc[tn][mb];
      f32x4 pv;
#pragma unroll
      for (int i = 0; i < 4; ++i) pv[i] = __shfl_xor(v[i], 32, 64);
      if (gt < ntiles) {
        const EpiIn e = epi_load_at<EPI>(a, gt, m, lane);
        epi_store<EPI>(a, gt, m, lane, e, [&](int off) { return off ? pv : v; });
      }
    }
  }
}

// Split-K combine + fused epilogue: one wave per 16 x 16 output unit (the slabs hold scaled fp16 partials).  As
// wg_reduce_unit, the epilogue inputs and all KS slab pieces are issued before the first add (KS = 0: runtime
// count); kept apart from it because the QKV epilogue's rounding follows how the compiler fuses its multiply-adds
// with the sum before them (profiles/r10/wide_ring_share/README.md).
template <int BM, int EPI, int KS>
__global__ __launch_bounds__(256) void wgemm8_reduce_kernel(const GemmArgs a, const WgArgs w, const W8Scales q,
                                                            int n_units) {
  constexpr int RB = BM / 16;
  const int lane = threadIdx.x & 63;
  const int unit = wg_reduce_block(blockIdx.x, WG_NT * RB / 4, w.xcd_blk) * 4 + (threadIdx.x >> 6);
  if (unit >= n_units) return;
  const int gt = unit / RB, rb = unit - gt * RB;
  const int ntiles = a.N >> 4;
  const int m = rb * 16 + (lane & 15);
  const bool live = gt < ntiles;
  const EpiIn e = live ? epi_load_at<EPI>(a, gt, m, lane) : EpiIn{};
  const f16x4* src = reinterpret_cast<const f16x4*>(w.part) + (size_t)unit * 64 + lane;  // scaled fp16 partials
  auto widen = [](const f16x4& x) { return f32x4{(float)x[0], (float)x[1], (float)x[2], (float)x[3]}; };
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (KS > 0) {
    f16x4 p[KS];
#pragma unroll
    for (int k = 0; k < KS; ++k) p[k] = src[(size_t)k * n_units * 64];
#pragma unroll
    for (int k = 0; k < KS; ++k) v += widen(p[k]);
  } else {
    for (int k = 0; k < w.ks; ++k) v += widen(src[(size_t)k * n_units * 64]);
  }
  f32x4 pv;
#pragma unroll
  for (int i = 0; i < 4; ++i) pv[i] = __shfl_xor(v[i], 32, 64);
  if (!live) return;
  epi_store<EPI>(a, gt, m, lane, e, [&](int off) { return off ? pv : v; });
}

// Per-row fp8 quantisation of bf16 activations: x8 = e4m3(x / s), s = amax / 448; xs = s * (norm ?
// rsqrt(mean(x^2) + eps) : 1) -- the RMSNorm of the bf16 rows folded into the row scale (gain in W).
// One 256-thread workgroup per row; the row stays in registers between the statistics and the store (one read
// of the row: a second pass over it cost a second L2 round trip in a launch this short).  K % 8 == 0,
// K <= QR_MAXK.
constexpr int QR_THREADS = 256, QR_CHUNKS = 12;  // 16-B chunks per thread
constexpr int QR_MAXK = QR_THREADS * QR_CHUNKS * 8;  // 24,576 = gemma:7b's ffn, the widest GEMM input
__global__ __launch_bounds__(QR_THREADS) void quant_rows_kernel(const __bf16* __restrict__ x, int ldx, int K,
                                                                uint8_t* __restrict__ x8, int ld8,
                                                                float* __restrict__ xs, int norm, float eps) {
  const int m = blockIdx.x;
  const __bf16* row = x + (size_t)m * ldx;
  bf16x8 v[QR_CHUNKS];
#pragma unroll
  for (int c = 0; c < QR_CHUNKS; ++c) {
    const int k = (c * QR_THREADS + threadIdx.x) * 8;
    if (k < K) v[c] = *reinterpret_cast<const bf16x8*>(row + k);
  }
  float amax = 0.f, ss = 0.f;
#pragma unroll
  for (int c = 0; c < QR_CHUNKS; ++c) {
    if ((c * QR_THREADS + threadIdx.x) * 8 < K) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = bf2f(v[c][j]);
        amax = fmaxf(amax, fabsf(f));
        ss += f * f;
      }
    }
  }
  amax = wave_max(amax);
  ss = wave_sum(ss);
  __shared__ float s_a[QR_THREADS / 64], s_s[QR_THREADS / 64];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_a[wave] = amax, s_s[wave] = ss;
  __syncthreads();
  amax = fmaxf(fmaxf(s_a[0], s_a[1]), fmaxf(s_a[2], s_a[3]));
  ss = (s_s[0] + s_s[1]) + (s_s[2] + s_s[3]);
  const float scale = amax > 0.f ? amax / 448.f : 1.f;
  const float inv = 1.f / scale;
  uint8_t* orow = x8 + (size_t)m * ld8;
  typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int c = 0; c < QR_CHUNKS; ++c) {
    const int k = (c * QR_THREADS + threadIdx.x) * 8;
    if (k < K) {
      u32x2_t o;
      o[0] = fp8x4(bf2f(v[c][0]) * inv, bf2f(v[c][1]) * inv, bf2f(v[c][2]) * inv, bf2f(v[c][3]) * inv);
      o[1] = fp8x4(bf2f(v[c][4]) * inv, bf2f(v[c][5]) * inv, bf2f(v[c][6]) * inv, bf2f(v[c][7]) * inv);
      *reinterpret_cast<u32x2_t*>(orow + k) = o;
    }
  }
  if (threadIdx.x == 0) xs[m] = scale * (norm ? rms_inv(ss, K, eps) : 1.f);
}

namespace {

struct W8Plan {
  int bm, nblk, ks, kst;
  size_t part_floats;
};

W8Plan w8_plan(int N, int K, int M) {
  W8Plan p{};
  p.bm = M > 128 ? 256 : 128;
  p.nblk = ((N >> 4) + WG_NT - 1) / WG_NT;
  const WgSplit s = wg_split(p.nblk, K / W8_BK, 256, 8);
  p.ks = s.ks, p.kst = s.kst;
  if (p.ks > 1) p.part_floats = (size_t)p.ks * p.nblk * WG_NT * (p.bm / 16) * 256;
  return p;
}

template <int BM, int DX, int DW, int EPI, int NDMA, bool FP4 = false>
hipError_t w8_launch(const GemmArgs& a, const WgArgs& w, const W8Scales& q, const W8Plan& p, hipStream_t st) {
  using G = WgGeo<BM>;
  constexpr int lds = W8Ring<BM, DX, DW, NDMA, FP4>::LDS_BYTES;
  const hipError_t e =
      wg_launch_lds<&wgemm8_kernel<BM, DX, DW, EPI, NDMA, FP4>, lds>(p.nblk * p.ks, 64 * (8 + NDMA), st, a, w, q);
  if (e != hipSuccess || p.ks == 1) return e;
  const int n_units = p.nblk * WG_NT * G::RB;
  wg_with_ks(w.ks, std::integer_sequence<int, 2, 3, 4, 5, 6, 7, 8>{}, [&](auto KS) {
    hipLaunchKernelGGL((wgemm8_reduce_kernel<BM, EPI, decltype(KS)::value>), dim3((n_units + 3) / 4), dim3(256), 0, st,
                       a, w, q, n_units);
  });
  return hipGetLastError();
}

template <int BM, bool FP4 = false>
hipError_t w8_launch_e(int epi, const GemmArgs& a, const WgArgs& w, const W8Scales& q, const W8Plan& p,
                       hipStream_t st) {
  // 160 KiB rings, as the bf16 defaults; fp4's 8.5-KiB W stages: the same X ring, 6 W stages (147 / 115 KiB)
  constexpr int DX = BM == 256 ? 2 : 3, DW = FP4 ? 5 : (BM == 256 ? 3 : 5);
  return wg_with_epi(epi, [&](auto E) { return w8_launch<BM, DX, DW, decltype(E)::value, 4, FP4>(a, w, q, p, st); });
}

}  // namespace

// Shapes the W8A8 kernel takes: 16 < M <= 256, whole 128-deep stages, >= 4 of them, 16-column tiles.
CAIN_API int cain_w8a8_eligible(int N, int K, int M) {
  return M > 16 && M <= 256 && K % W8_BK == 0 && K >= 4 * W8_BK && N % 16 == 0;
}

// The slabs go after the bf16 paths' counter regions (gemm.hip GEMM_SLAB_OFFSET), which must stay zero when
// the engine shares one workspace between both weight formats' launches.
constexpr long long W8_SLAB_OFFSET = 80 * 1024;

CAIN_API long long cain_w8a8_ws_bytes(int N, int K, int M) {
  if (!cain_w8a8_eligible(N, K, M)) return 0;
  return W8_SLAB_OFFSET + (long long)(w8_plan(N, K, M).part_floats * sizeof(float));
}

CAIN_API int cain_quant_rows(const void* x, int ldx, int K, int M, void* x8, int ld8, float* xs, int norm, float eps,
                             hipStream_t st) {
  if (K % 8 || K > QR_MAXK || ldx % 8 || ld8 % 8 || M < 1) return -1;
  hipLaunchKernelGGL(quant_rows_kernel, dim3(M), dim3(QR_THREADS), 0, st, (const __bf16*)x, ldx, K, (uint8_t*)x8, ld8, xs,
                     norm, eps);
  return int(hipGetLastError());
}

namespace {

// X / ldx of the record: the e4m3 rows of cain_quant_rows and their stride in bytes (norm and eps went into xs)
int w8a8_run(bool fp4, const CainGemm& g, hipStream_t st) {
  const int K = g.K, N = g.N, M = g.M, epi = g.epi & EPI_MASK;
  void* const ws = g.ws;
  if (!cain_w8a8_eligible(N, K, M) || g.ldx % 16) return -1;
  GemmArgs a;
  if (!gemm_args(g, a)) return -1;
  const W8Plan p = w8_plan(N, K, M);
  if (p.ks > 1 && (!ws || W8_SLAB_OFFSET + (long long)(p.part_floats * sizeof(float)) > g.ws_bytes)) return -1;
  WgArgs w{};
  w.ks = p.ks, w.kst = p.kst, w.part = ws ? reinterpret_cast<float*>(static_cast<char*>(ws) + W8_SLAB_OFFSET) : nullptr;
  w.xcd_blk = p.ks > 1 && p.nblk % 8 == 0;  // XCD-local split-K (wgemm_ring.h wg_block_of)
  const W8Scales q{g.xs, static_cast<const float*>(g.sc)};
  hipError_t e;
  if (fp4) e = p.bm == 256 ? w8_launch_e<256, true>(epi, a, w, q, p, st) : w8_launch_e<128, true>(epi, a, w, q, p, st);
  else e = p.bm == 256 ? w8_launch_e<256>(epi, a, w, q, p, st) : w8_launch_e<128>(epi, a, w, q, p, st);
  return int(e);
}

}  // namespace

// Y = epi(xs[m] * sc[n] * X8 . W8^T).  W: pack_mfma_a_fp8_k128; X [M][ldx] e4m3 rows (cain_quant_rows);
// ws: >= cain_w8a8_ws_bytes of scratch; the rest as cain_gemm_bf16 (gemm.hip), including the EPI_KV_FP8 flag.
CAIN_API int cain_gemm_fp8a8(const CainGemm* g, hipStream_t st) { return w8a8_run(false, *g, st); }

// W4A8: Y = epi(xs[m] * X8 . W^T) with MXFP4 weights in the few-row kernel's packing (pack_mxfp4: W
// [N/16][K/128][64][16] e2m1 bytes, sc [N/16][K/128][64] e8m0 bytes); same shapes, workspace and epilogues as
// cain_gemm_fp8a8 (cain_w8a8_eligible, cain_w8a8_ws_bytes).
CAIN_API int cain_gemm_mxfp4a8(const CainGemm* g, hipStream_t st) { return w8a8_run(true, *g, st); }
