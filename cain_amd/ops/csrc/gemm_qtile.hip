// GGUF Q4_0 / Q4_K / Q6_K weights against up to 64 activation rows per launch: ONE pass over the weight bytes per 64
// rows (a prefill chunk, a continuous batch), where the stream kernels (gemm_qstream.hip) hold all rows of
// the whole K in LDS and so stream the matrix once per 1-16 rows.
//
// Arithmetic: the stream kernels', part by part (gemm_qstream.hip's header).  The codes enter the bf16 MFMA unscaled as 128 + q
// (q4_frag / q6_frag), one zero-accumulator MFMA per scale block (16x16x32 per 32-block for Q4, 16x16x16 per
// 16-group for Q6_K), the block's fp32 scale applied to that fp32 partial, and the correction (128 s + o) X_b
// (Q4) / 160 s X_g (Q6_K) summed by v_mfma_f32_16x16x4_f32 over the block sums X of the activations.  The RMSNorm
// sum of squares is taken from the raw row; with a gain, x' = bf16(x gain) is what the MFMAs multiply and what the
// block sums add.  Packed layouts as the stream kernels read them: nothing is repacked.
//
// Shape: a workgroup of 4 waves walks K in 256-wide slabs (one super-block: 2 k quads).  The slab of the launch's
// rows (<= 64 x 256 bf16 = 32 KiB) and its block sums sit in LDS twice: while the waves multiply slab j, the
// threads hold slab j + 1 in registers (loaded before the multiply), then write it -- gain applied, block sums by
// DPP lane sums, squares accumulated -- into the other copy; one barrier per slab.  The footprint does not depend
// on K.  Each wave owns one 16-row weight tile over the whole K (no cross-wave reduction) and NB of the row blocks:
//
//   NB = 2 (Q4 only): 2 tiles x 2 halves of up to 64 rows, or 4 tiles of up to 32 rows
//   NB = 1: 1 tile x 4 row blocks, 2 tiles x 2, or 4 tiles of up to 16 rows
//
// so a narrow N still fills the CUs (q_tile_nb); a tile's bytes read by 2 or 4 waves of one workgroup are still one
// HBM pass.  (Instances of 4 row blocks per wave, and of 2 for Q6_K, spilled 260-840 bytes per lane and measured
// slowest on every shape: profiles/r8/q_tile/README.md; they are not built.)  A wave's weights are double-buffered in
// registers, one slab in
// flight.  LDS rows are 512 B with the 16-byte chunk index xor-ed with the row (mod 16): the A-operand reads (16
// rows x one chunk per ds_read_b128 lane group) and the row-major staging writes are both conflict-free.
//
// Epilogue: per row block the wave transposes its 16 x 16 partial through a private LDS patch into the epilogues'
// lane order (gemm_epi.h, as the stream kernels' tile end) -- all six epilogues, the fp8 KV flag, the chunk maxima
// of EPI_F32, `tile0` for Q6_K.  Rows >= M are clamped on load and never stored.
#include <algorithm>

#include "common.h"
#include "gemm_epi.h"
#include "gemm_q.h"

struct QTArgs {
  const uint8_t* sc;  // block scales (Q4_0 fp16 d; Q4_K sc | m << 8; Q6_K int8): [tiles][KQ][16 rows] x 8 bytes
  const void* dd;     // super-block scales: Q4_K fp16 (d, dmin) pairs, Q6_K fp32 d; [tiles][KQ / 2][16 rows]
  const float* gain;  // RMSNorm gain per k applied while staging (null: none)
  int ntiles;         // N / 16
  int tile0;          // the epilogue's index of weight tile 0 (Q6_K; 0 for Q4)
  int tw;             // weight tiles per workgroup: 4, 2 or 1 (4 / tw row groups of NB blocks each)
};

constexpr int QT_SLAB = 256;       // k per slab
constexpr int QT_ROW_BYTES = 512;  // one row of a slab in LDS

template <int FMT, int NB, int EPI, bool NORM>
__device__ __forceinline__ void qtile_body(const GemmArgs& a, const QTArgs& q) {
  constexpr bool Q6 = FMT == Q6F_K;
  constexpr int NBS = Q6 ? 16 : 8;  // scale blocks per slab
  constexpr int SS = NBS + 1;       // row stride of the sums (odd: the 16 rows of a read spread over the banks)
  __shared__ __attribute__((aligned(16))) char xs[2][64 * QT_ROW_BYTES];
  __shared__ float xsum[2][64 * SS];
  __shared__ __attribute__((aligned(16))) float tr[4][256];
  __shared__ float row_ss[64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int KQ = a.K >> 7;  // 128-wide k quads
  const int NS = a.K >> 8;  // slabs
  const int tsub = wave & (q.tw - 1), rg = wave / q.tw;
  const int tile_raw = (int)blockIdx.x * q.tw + tsub;
  const int tile = min(tile_raw, q.ntiles - 1);  // a partial workgroup's spare waves redo the last tile, unstored
  const int mo = rg * NB * 16;                   // first row of this wave's row blocks
  const int nrows = min(64, (a.M + 15) & ~15);   // rows a slab holds: whole 16-row blocks (rows >= M repeat row M - 1)
  const int m16 = lane & 15, g = lane >> 4;

  // ---- staging: thread t, chunk i -> row (t >> 5) + 8 i, 16-byte k chunk t & 31 of the slab
  const int nst = nrows >> 3;
  const int srow = threadIdx.x >> 5, kc = threadIdx.x & 31;
  const bool gained = q.gain != nullptr;
  bf16x8 xst[8];
  f32x4 gn0 = f32x4{1.f, 1.f, 1.f, 1.f}, gn1 = gn0;
  float ssq[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) ssq[i] = 0.f;
  auto x_load = [&](int j) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < nst) {
        const int r = min(srow + 8 * i, a.M - 1);
        xst[i] = *reinterpret_cast<const bf16x8*>(a.X + (size_t)r * a.ldx + j * QT_SLAB + kc * 8);
      }
    if (gained) {
      gn0 = *reinterpret_cast<const f32x4*>(q.gain + j * QT_SLAB + kc * 8);
      gn1 = *reinterpret_cast<const f32x4*>(q.gain + j * QT_SLAB + kc * 8 + 4);
    }
  };
  auto x_store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < nst) {
        bf16x8 x8 = xst[i];
        if constexpr (NORM) {  // the RAW row's squares
#pragma unroll
          for (int e = 0; e < 8; ++e) ssq[i] += bf2f(x8[e]) * bf2f(x8[e]);
        }
        if (gained) {  // x' = bf16(x * gain): what the MFMAs multiply and the block sums add
#pragma unroll
          for (int e = 0; e < 4; ++e) x8[e] = (__bf16)(bf2f(x8[e]) * gn0[e]), x8[4 + e] = (__bf16)(bf2f(x8[4 + e]) * gn1[e]);
        }
        float sum = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += bf2f(x8[e]);
        const int r = srow + 8 * i;
        *reinterpret_cast<bf16x8*>(xs[buf] + r * QT_ROW_BYTES + ((kc ^ (r & 15)) << 4)) = x8;
        if constexpr (Q6) {  // a 16-group is 2 consecutive chunks: a lane pair
          sum = q6_pair_sum(sum);
          if ((kc & 1) == 0) xsum[buf][r * SS + (kc >> 1)] = sum;
        } else {  // a 32-block is 4 consecutive chunks: a lane quad
          sum = q4_quad_sum(sum);
          if ((kc & 3) == 0) xsum[buf][r * SS + (kc >> 2)] = sum;
        }
      }
  };

  // ---- this wave's weights: one item per slab (2 quads of the lane's weight row 16 tile + m16)
  struct Quad {
    qu32x4 w;   // Q4: the 32 codes; Q6_K: their low nibbles
    qu32x2 hi;  // Q6_K: the high bit pairs
    qu32x2 s;   // the quad's block scales (Q4: 4 x 16 bits; Q6_K: 8 x int8)
  };
  struct Item {
    Quad q[2];
    uint32_t d;  // Q4_K: fp16 (d, dmin); Q6_K: fp32 d
  };
  const uint8_t* wbase = reinterpret_cast<const uint8_t*>(a.Wp);
  auto ldw = [&](const auto* p) { return *p; };  // plain loads: with NB < 4 other waves of the workgroup may re-read them
  auto w_load = [&](Item& it, int j_raw) {
    const int j = min(j_raw, NS - 1);  // past the end: the last slab again (a cache hit), never a branch around the load
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const size_t tq = (size_t)tile * KQ + 2 * j + h;
      if constexpr (Q6) {
        it.q[h].w = ldw(reinterpret_cast<const qu32x4*>(wbase + tq * 1536) + lane);
        it.q[h].hi = ldw(reinterpret_cast<const qu32x2*>(wbase + tq * 1536 + 1024) + lane);
      } else {
        it.q[h].w = ldw(reinterpret_cast<const qu32x4*>(wbase) + tq * 64 + lane);
        it.q[h].hi = qu32x2{0u, 0u};
      }
      it.q[h].s = ldw(reinterpret_cast<const qu32x2*>(q.sc) + tq * 16 + m16);
    }
    if constexpr (FMT == Q4F_0) it.d = 0;
    else it.d = ldw(reinterpret_cast<const uint32_t*>(q.dd) + ((size_t)tile * (KQ >> 1) + j) * 16 + m16);
  };

  // A operand: activation row mo + 16 b + m16, k group g.  The row's swizzle key is m16 for every row block, so one
  // address per MFMA s serves all blocks, both quads (h) and both copies through the instruction's offset.  (Row
  // blocks past the staged rows read LDS nobody wrote: their products are never stored.)
  constexpr int XA = Q6 ? 8 : 4;
  int xa[XA];
#pragma unroll
  for (int s = 0; s < XA; ++s)
    xa[s] = (mo + m16) * QT_ROW_BYTES + (Q6 ? ((((g >> 1) ^ m16) ^ (2 * s)) << 4) + 8 * (g & 1) : ((g ^ m16) ^ (4 * s)) << 4);
  const int sa = (mo + m16) * SS + g;
  // Per slab, acc = sum_b s_nb T_b and corr = sum_b (128 s_nb + o_nb) X_b (Q6_K: 160 s_ng X_g) over the slab's blocks,
  // and their difference joins the running total: the two large sums cancel over 256 k at a time, as the stream
  // kernels' do over each wave's share of K before the waves' partials are added (one sum over the whole K rounded
  // ~3x worse than theirs on random activations).
  f32x4 tot[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) tot[b] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto step = [&](const Item& it, int buf) {
    const char* xb = xs[buf];
    const float* sb = xsum[buf];
    f32x4 acc[NB], corr[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f}, corr[b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const Quad& qd = it.q[h];
      if constexpr (!Q6) {
        // this lane's weight row: the 4 block scales of the quad, and block 4 h + g's correction coefficient
        float sc[4], c2;
        const uint32_t wg = (g & 2) ? qd.s[1] : qd.s[0];
        const uint32_t vg = (g & 1) ? (wg >> 16) : (wg & 0xffffu);
        if constexpr (FMT == Q4F_0) {
#pragma unroll
          for (int s = 0; s < 4; ++s) sc[s] = q4_h2f(qd.s[s >> 1] >> (16 * (s & 1)));
          c2 = 136.f * q4_h2f(vg);  // 128 d + 8 d
        } else {
          const float d = q4_h2f(it.d), dmin = q4_h2f(it.d >> 16);
#pragma unroll
          for (int s = 0; s < 4; ++s) sc[s] = d * float((qd.s[s >> 1] >> (16 * (s & 1))) & 0xffu);
          c2 = 128.f * d * float(vg & 0xffu) + dmin * float(vg >> 8);
        }
        bf16x8 wf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) wf[s] = q4_frag(qd.w[s]);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          f32x4 t[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) {  // k = 128 h + 32 s + 8 g: chunk 16 h + 4 s + g
            const bf16x8 xv = *reinterpret_cast<const bf16x8*>(xb + xa[s] + (b * 16 * QT_ROW_BYTES + h * 256));
            t[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xv, wf[s], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          }
          corr[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(sb[sa + (b * 16 * SS + 4 * h)], c2, corr[b], 0, 0, 0);
#pragma unroll
          for (int s = 0; s < 4; ++s) acc[b] += t[s] * sc[s];
          __builtin_amdgcn_sched_barrier(0);  // one row block's operands and partials live at a time
        }
      } else {
        const float d = __builtin_bit_cast(float, it.d);
        float sc[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) sc[s] = d * q6_i8f(qd.s[s >> 2], s & 3);
        // the correction MFMAs' coefficients: groups 8 h + g and 8 h + 4 + g of this lane's weight row
        const float c0 = (160.f * d) * q6_i8f(qd.s[0], g), c1 = (160.f * d) * q6_i8f(qd.s[1], g);
        qs16x4 wf[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) wf[s] = q6_frag(qd.w, qd.hi, s);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          f32x4 t[8];
#pragma unroll
          for (int s = 0; s < 8; ++s) {  // k = 128 h + 16 s + 4 g: chunk 16 h + 2 s + (g >> 1), its half g & 1
            const qs16x4 xv = *reinterpret_cast<const qs16x4*>(xb + xa[s] + (b * 16 * QT_ROW_BYTES + h * 256));
            t[s] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(xv, wf[s], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          }
          corr[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(sb[sa + (b * 16 * SS + 8 * h)], c0, corr[b], 0, 0, 0);
          corr[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(sb[sa + (b * 16 * SS + 8 * h + 4)], c1, corr[b], 0, 0, 0);
#pragma unroll
          for (int s = 0; s < 8; ++s) acc[b] += t[s] * sc[s];
          __builtin_amdgcn_sched_barrier(0);  // one row block's operands and partials live at a time
        }
      }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) tot[b] += acc[b] - corr[b];
  };

  // ---- the k loop, two slabs per round (constant ring slots and LDS copies): while slab j is multiplied, slab
  // j + 1's weights and activations are in flight; the activations are loaded BEFORE the weights, so waiting for them
  // does not wait for the weights
  Item ring[2];
  w_load(ring[0], 0);
  x_load(0);
  x_store(0);
  q_barrier();
  for (int j0 = 0; j0 < NS; j0 += 2) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int j = j0 + u;
      if (j < NS) {  // uniform over the workgroup: every wave walks the same K
        const bool more = j + 1 < NS;
        if (more) x_load(j + 1);
        w_load(ring[u ^ 1], j + 1);
        __builtin_amdgcn_sched_barrier(0);
        step(ring[u], u);
        if (more) x_store(u ^ 1);
        q_barrier();  // slab j + 1 is written; every wave is done reading slab j
      }
    }
  }
  if constexpr (NORM) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < nst) {  // the 32 lanes of a half wave hold one row's k chunks
        float v = ssq[i];
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if (kc == 0) row_ss[srow + 8 * i] = v;
      }
    q_barrier();
  }

  // ---- epilogue, per row block: D'[m = 4 g + i][n = m16] through the wave's LDS patch into the epilogues' lane
  // order (lane L: activation row L & 15, weight rows 4 (L >> 4) + i)
  if (tile_raw >= q.ntiles) return;
  const int gt = q.tile0 + tile;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int mrow = mo + 16 * b;
    if (mrow >= a.M) break;  // uniform
    const f32x4 v = tot[b];
    __builtin_amdgcn_wave_barrier();  // (the previous block's reads of the patch are issued)
#pragma unroll
    for (int i = 0; i < 4; ++i) tr[wave][(4 * g + i) * 16 + m16] = v[i];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // one wave's LDS accesses run in order; the compiler's too
    __builtin_amdgcn_wave_barrier();
    const int m = mrow + m16;
    const EpiIn pre = epi_load_at<EPI>(a, gt, m, lane);
    auto unit = [&](int L) -> f32x4 {
      const int mm = L & 15;
      f32x4 u = *reinterpret_cast<const f32x4*>(&tr[wave][mm * 16 + 4 * (L >> 4)]);
      if constexpr (NORM) u *= rms_inv(row_ss[min(mrow + mm, a.M - 1)], a.K, a.eps);
      return u;
    };
    if constexpr (EPI == EPI_F32) {  // the LM head: logits + chunk maxima
      const f32x4 u = unit(lane);
      epi_store<EPI>(a, gt, m, lane, pre, [&](int) { return u; });
      epi_cmax(a, gt, m, lane, u);
    } else {
      epi_store<EPI>(a, gt, m, lane, pre, [&](int off) { return unit(lane + off); });
    }
  }
}

template <int FMT, int NB, int EPI, bool NORM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void q4_tile_kernel(const GemmArgs a, const QTArgs q) {
  qtile_body<FMT, NB, EPI, NORM>(a, q);
}

template <int NB, int EPI, bool NORM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void q6_tile_kernel(const GemmArgs a, const QTArgs q) {
  qtile_body<Q6F_K, NB, EPI, NORM>(a, q);
}

// ================================================================ launch
template <int FMT, int EPI, bool NORM>
static hipError_t qt_launch_nb(int nb, const GemmArgs& a, const QTArgs& q, int grid, hipStream_t st) {
  const dim3 g(grid), b(256);
  if constexpr (FMT == Q6F_K) {
    if constexpr (EPI == EPI_SILU || EPI == EPI_GELU) {
      return hipErrorInvalidValue;  // no Q6_K gate/up epilogue (gemm_qstream.hip)
    } else {
      hipLaunchKernelGGL((q6_tile_kernel<1, EPI, NORM>), g, b, 0, st, a, q);
    }
  } else {
    if (nb == 2) hipLaunchKernelGGL((q4_tile_kernel<FMT, 2, EPI, NORM>), g, b, 0, st, a, q);
    else hipLaunchKernelGGL((q4_tile_kernel<FMT, 1, EPI, NORM>), g, b, 0, st, a, q);
  }
  return hipGetLastError();
}

template <int FMT, bool NORM>
static hipError_t qt_launch_epi(int epi, int nb, const GemmArgs& a, const QTArgs& q, int grid, hipStream_t st) {
  switch (epi) {
    case EPI_BF16: return qt_launch_nb<FMT, EPI_BF16, NORM>(nb, a, q, grid, st);
    case EPI_RESID: return qt_launch_nb<FMT, EPI_RESID, NORM>(nb, a, q, grid, st);
    case EPI_F32: return qt_launch_nb<FMT, EPI_F32, NORM>(nb, a, q, grid, st);
    case EPI_SILU: return qt_launch_nb<FMT, EPI_SILU, NORM>(nb, a, q, grid, st);
    case EPI_GELU: return qt_launch_nb<FMT, EPI_GELU, NORM>(nb, a, q, grid, st);
    case EPI_QKV_ROPE: return qt_launch_nb<FMT, EPI_QKV_ROPE, NORM>(nb, a, q, grid, st);
    default: return hipErrorInvalidValue;
  }
}

// Tuning / test switches: the path (-1: the rule q_tile_rule, 0: never the tile kernels, 1: always) and Q4's row
// blocks per wave (0: the rule q_tile_nb)
static int g_q_tile = -1, g_q_tile_nb = 0;
CAIN_API void cain_gemm_q_set_tile(int mode) { g_q_tile = (mode == 0 || mode == 1) ? mode : -1; }
CAIN_API void cain_gemm_q_set_tile_nb(int nb) { g_q_tile_nb = (nb == 1 || nb == 2) ? nb : 0; }

// Row blocks per wave for M rows over `tiles` weight tiles.  Q6_K: 1 (2 measured 1.3-2.7x slower on every shape).  Q4:
// 2 where that still gives every CU of the budget a workgroup, else 1 -- at 64 rows gate/up 94 vs 148 us and the LM
// head 369 vs 639 on 2, QKV / O / down (fewer workgroups than CUs on 2) within 10 % either way, and the same order
// at 17 and 32 rows (profiles/r8/q_tile/README.md).
static int q_tile_nb(int fmt, int tiles, int M, int n_cu) {
  const int nblk = (std::min(M, 64) + 15) / 16;
  if (fmt == Q6F_K || nblk < 2) return 1;
  if (g_q_tile_nb) return g_q_tile_nb;
  const int tw = nblk > 2 ? 2 : 4;  // tiles per workgroup with 2 row blocks per wave
  return (tiles + tw - 1) / tw >= n_cu ? 2 : 1;
}

// The default rule, from the crossovers measured on llama3.1:8b and qwen2:1.5b (profiles/r8/q_tile/README.md): never
// where the stream kernels need one pass; from 17 rows, always (faster on every shape, a tie on one); from 8 to 16
// rows, where the stream kernels need 4 or more passes (at 2-3 passes narrow outputs lost: O 18.7 vs 16.2 us,
// qwen2:1.5b's down 33.8 vs 28.0); below 8 rows never (slower on every shape at 2 and 4 rows but one within 8 %).
static bool q_tile_rule(int fmt, int K, int M, int epi, int stream_rows) {
  (void)fmt, (void)K, (void)epi;
  if (M <= stream_rows) return false;
  return M >= 17 || (M >= 8 && (M + stream_rows - 1) / stream_rows >= 4);
}

bool q_tile_selected(int fmt, int K, int M, int epi, int stream_rows) {
  if (g_q_tile == 0) return false;
  if (g_q_tile == 1) return true;
  return q_tile_rule(fmt, K, M, epi, stream_rows);
}

// How many times cain_gemm_gguf streams the weight matrix for M rows under the current mode; -1 where the entry
// refuses the shape.
CAIN_API int cain_gemm_q_passes(int fmt, int K, int M, int epi) {
  epi &= EPI_MASK;
  if (fmt < Q4F_0 || fmt > Q6F_K || K < 256 || K % 256 || M < 1) return -1;
  const int rows = fmt == Q6F_K ? cain_gemm_q6_rows(K, epi) : cain_gemm_q4_rows(K, epi);
  if (rows <= 0) return -1;
  const int per = q_tile_selected(fmt, K, M, epi, rows) ? 64 : rows;
  return (M + per - 1) / per;
}

hipError_t q_tile_launch(int fmt, const GemmArgs& a, const void* sc, const void* dd, const float* gain, int epi,
                         bool norm, int tile0, hipStream_t st) {
  if (a.M < 1 || a.M > 64 || a.K < QT_SLAB || a.K % QT_SLAB || a.N < 16 || a.N % 16) return hipErrorInvalidValue;
  const int tiles = a.N / 16;
  const int nblk = (a.M + 15) / 16;
  const int nb = q_tile_nb(fmt, tiles, a.M, cain_cu_budget());
  const int rgs = nblk <= nb ? 1 : nblk <= 2 * nb ? 2 : 4;  // row groups of nb blocks that cover the rows
  QTArgs q{};
  q.sc = static_cast<const uint8_t*>(sc), q.dd = dd, q.gain = gain, q.ntiles = tiles, q.tile0 = tile0;
  q.tw = 4 / rgs;
  const int grid = (tiles + q.tw - 1) / q.tw;
  switch (fmt) {
    case Q4F_0:
      return norm ? qt_launch_epi<Q4F_0, true>(epi, nb, a, q, grid, st)
                  : qt_launch_epi<Q4F_0, false>(epi, nb, a, q, grid, st);
    case Q4F_K:
      return norm ? qt_launch_epi<Q4F_K, true>(epi, nb, a, q, grid, st)
                  : qt_launch_epi<Q4F_K, false>(epi, nb, a, q, grid, st);
    case Q6F_K:
      return norm ? qt_launch_epi<Q6F_K, true>(epi, nb, a, q, grid, st)
                  : qt_launch_epi<Q6F_K, false>(epi, nb, a, q, grid, st);
    default: return hipErrorInvalidValue;
  }
}
