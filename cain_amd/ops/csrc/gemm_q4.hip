// GGUF 4-bit weights (llama.cpp's Q4_0 and Q4_K, Ollama's default model builds) for single-stream / few-row
// decode, M <= 16 rows per launch (many rows: gemm_qtile.hip): the weights' VALUES as the file stores them, only
// their layout repacked.
//
// The reference's models are Ollama pulls (/root/reference/README.md:29-30, tags of
// /root/reference/experiment/RunnerConfig.py:80), whose default builds are GGUF Q4_0 / Q4_K_M.
// gemm_w4.hip runs MXFP4, a different 4-bit grid, so a GGUF file reached it re-quantised (VERDICT r5 missing 2).
// Here the block values are exact:
//
//   Q4_0: 32-element blocks, w = d * (q - 8), q in 0..15, d fp16            (4.5 bits per weight)
//   Q4_K: 256-element super-blocks of 8 blocks, w = d * sc * q - dmin * m,  (4.5 bits in the file, 4.625 here:
//         q in 0..15, 6-bit sc / m per block, fp16 d / dmin per super-block  the 6-bit pairs stored as bytes)
//
// No block scale is exact in bf16 once multiplied in, so the codes go into the MFMA unscaled and each block's
// scale is applied to its own partial sum: the MFMA multiplies the ACTIVATIONS (A operand: rows = activation rows m)
// by the codes (B operand: columns = weight rows n), so one lane's four outputs share its weight row n and each
// lane needs just that row's 4 block scales per 128-k quad (8 bytes, one load).  The codes enter as bf16 128 + q
// (one v_perm per pair: exact), so per block b
//
//   sum_k x_k w_k = s_nb * (T_b - 128 X_b) - o_nb X_b = s_nb T_b - (128 s_nb + o_nb) X_b
//
// with T_b = sum_k x_k (128 + q_k) (one v_mfma_f32_16x16x32_bf16 per block, fp32), X_b = sum_k x_k (the block
// sums of the staged activations, computed once per workgroup in LDS), s = d, o = 8 d (Q4_0) or s = d sc,
// o = dmin m (Q4_K).  The per-block scale-and-add is 4 fp32 FMAs per MFMA; the correction term is a
// K/32-deep product of the coefficients (128 s + o) with the block sums, one v_mfma_f32_16x16x4_f32 per quad.
// The products (128 + q) x are exact in fp32, so the cancellation of T_b against 128 X_b costs ~1e-6 relative.
//
// RMSNorm gain: a GGUF file's gains stay separate from its quantised weights (folding them in would change the
// values), so the staging multiplies the activations by the gain (a.gain, fp32 per k; null: none) after the
// row's sum of squares is taken from the raw values; the fused RMSNorm factor is applied at the end, as in every
// other kernel.  Epilogues, the persistent tile stream and the register ring are gemm_w4.hip's stream kernel's.
//
// Layout (cain_amd/models/q4.py pack_q4): codes Wq[(t*KQ + p)*64 + lane], 16 bytes, lane = 16g + r: weight row
// 16t + r, k = 128p + 32s + 8g + j at dword s, byte j & 3, nibble j >> 2 (low nibbles j = 0..3, high 4..7) --
// so the four bytes of a dword turn into the eight bf16 of an MFMA operand with two ANDs and four v_perm_b32.
// Scales Q4_0: fp16 d[(t*KQ + p)*16 + r][4 blocks]; Q4_K: uint16 (sc | m << 8)[(t*KQ + p)*16 + r][4 blocks] and
// fp16x2 (d, dmin)[(t*(KQ/2) + p/2)*16 + r].
#include <algorithm>

#include "common.h"
#include "gemm_epi.h"
#include "gemm_q.h"

struct Q4Args {
  const uint8_t* sc;   // Q4_0: fp16 d; Q4_K: (sc | m << 8) -- [tiles][KQ][16 rows][4 blocks] x 2 bytes
  const uint32_t* dd;  // Q4_K: (d, dmin) fp16 pairs [tiles][KQ / 2][16 rows]
  const float* gain;   // RMSNorm gain per k applied while staging (null: none)
};

__device__ __forceinline__ void q4_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int WAVES>
constexpr int q4_xl_bytes() { return WAVES == 8 ? 57344 : 28672; }  // 2 x (56 + 16) KiB or 4 x (28 + 8) KiB per CU

// activation bytes + their block sums (floats) that the LDS copy holds for M rows of K
__host__ __device__ constexpr long long q4_lds_need(int M, int K) { return (long long)M * K * 2 + (long long)M * (K / 32) * 4; }

template <int WAVES, int U, int EPI, bool NORM, int FMT>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) void q4_stream_kernel(
    const GemmArgs a, const Q4Args q4, int npairs) {
  constexpr int XLB = q4_xl_bytes<WAVES>();
  constexpr int XCH = XLB / (WAVES * 64 * 16);  // 16-byte activation chunks staged per thread (upper bound)
  __shared__ __attribute__((aligned(16))) char q4_xs[XLB];
  // per wave, its 16 x 16 partial in [activation row m][weight row n] order (the epilogues' lane order, read back
  // as one 16-byte vector per lane)
  __shared__ __attribute__((aligned(16))) float red[2][WAVES][256];
  __shared__ float row_ss[16];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int KQ = a.K >> 7;  // 128-wide k quads
  const int NB = a.K >> 5;  // 32-element blocks per row
  const int qmax = (KQ + WAVES - 1) / WAVES;
  const int G = gridDim.x;
  const int my_tiles = (npairs - (int)blockIdx.x + G - 1) / G;
  const int n_items = my_tiles * qmax;
  constexpr int R = U + 1;
  const int n_pad = (n_items + R - 1) / R * R;
  float* xsum = reinterpret_cast<float*>(q4_xs + (size_t)a.M * a.K * 2);  // [M][NB] block sums of x'

  // ---- stage the activation rows (raw), then the weight ring's prologue
  bf16x8 xst[XCH];
  const int cpr = a.K >> 3, nch = a.M * cpr;
#pragma unroll
  for (int i = 0; i < XCH; ++i) {
    const int c = min((int)threadIdx.x + i * WAVES * 64, nch - 1);
    const int r = c / cpr, col = c - r * cpr;
    xst[i] = *reinterpret_cast<const bf16x8*>(a.X + (size_t)r * a.ldx + col * 8);
  }

  struct Quad {
    q4u32x4 w;
    q4u32x2 s;   // this lane's weight row: 4 block scales (Q4_0 fp16 d; Q4_K sc | m << 8)
    uint32_t d;  // Q4_K: (d, dmin) of the row's super-block
  };
  const q4u32x4* wbase = reinterpret_cast<const q4u32x4*>(a.Wp) + lane;
  const int row = lane & 15;
  int ld_t = blockIdx.x, ld_e = 0, ld_i = 0;
  const int last_t = (int)blockIdx.x + (my_tiles - 1) * G;
  auto load_next = [&](Quad& q) {
    // past the end: re-load this wave's last item (a cache hit), never a branch around the load (gemm_w4.hip)
    const bool in = ld_i < n_items;
    const int p = min(wave + (in ? ld_e : qmax - 1) * WAVES, KQ - 1);
    const int t = in ? ld_t : last_t;
    const size_t tq = (size_t)t * KQ + p;
    q.w = __builtin_nontemporal_load(wbase + tq * 64);
    q.s = __builtin_nontemporal_load(reinterpret_cast<const q4u32x2*>(q4.sc) + tq * 16 + row);
    if constexpr (FMT == Q4F_K) q.d = __builtin_nontemporal_load(q4.dd + ((size_t)t * (KQ >> 1) + (p >> 1)) * 16 + row);
    else q.d = 0;
    ++ld_i;
    if (++ld_e == qmax) ld_e = 0, ld_t += G;
  };
  Quad ring[R];
#pragma unroll
  for (int u = 0; u < U; ++u) load_next(ring[u]);

  int cp_t = blockIdx.x;
  EpiIn pre{};
  if (wave == 0 && my_tiles > 0) pre = epi_load_at<EPI>(a, cp_t, lane & 15, lane);
  const bool gained = q4.gain != nullptr;
#pragma unroll
  for (int i = 0; i < XCH; ++i) {
    const int c = (int)threadIdx.x + i * WAVES * 64;
    if (c < nch) *reinterpret_cast<bf16x8*>(q4_xs + (size_t)c * 16) = xst[i];
    if (!gained) {
      // the block sums straight from the staged registers: a 32-element block is 4 consecutive chunks, i.e. the 4
      // lanes of a quad (cpr = K / 8 is a multiple of 4), summed in a fixed order
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += bf2f(xst[i][j]);
      sum = q4_quad_sum(sum);
      if (c < nch && (c & 3) == 0) xsum[c >> 2] = sum;  // chunk c / 4 = row * NB + block
    }
  }
  q4_barrier();
  // sums of squares of the RAW rows (fixed order: wave w owns rows w, w + WAVES, ...); the first tile end's barrier
  // orders them before the epilogue reads them, unless the gain pass below rewrites the rows first
  if constexpr (NORM) {
    for (int r = wave; r < a.M; r += WAVES) {
      const char* xr = q4_xs + (size_t)r * cpr * 16;
      float v = 0.f;
      for (int c = lane; c < cpr; c += 64) {
        const bf16x8 x8 = *reinterpret_cast<const bf16x8*>(xr + (size_t)c * 16);
#pragma unroll
        for (int j = 0; j < 8; ++j) v += bf2f(x8[j]) * bf2f(x8[j]);
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0) row_ss[r] = v;
    }
  }
  if (gained) {
    // a separate gain (weights not gain-folded: a GGUF file's values): x' = bf16(x * gain) in place, then the block
    // sums of x' (the values the MFMAs multiply), one thread per (row, block)
    if constexpr (NORM) q4_barrier();  // the raw rows' sums of squares are taken
    for (int rb = threadIdx.x; rb < a.M * NB; rb += WAVES * 64) {
      const int r = rb / NB, b = rb - r * NB;
      bf16x8* xp = reinterpret_cast<bf16x8*>(q4_xs + ((size_t)r * a.K + b * 32) * 2);
      float sum = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        bf16x8 x8 = xp[c];
        const f32x4 g0 = *reinterpret_cast<const f32x4*>(q4.gain + b * 32 + c * 8);
        const f32x4 g1 = *reinterpret_cast<const f32x4*>(q4.gain + b * 32 + c * 8 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) x8[j] = (__bf16)(bf2f(x8[j]) * g0[j]), x8[4 + j] = (__bf16)(bf2f(x8[4 + j]) * g1[j]);
        xp[c] = x8;
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += bf2f(x8[j]);
      }
      xsum[rb] = sum;
    }
    q4_barrier();
  }

  // A operand: this lane's activation row m = lane & 15 (rows >= M multiply zeros), k group g
  const int g = lane >> 4;
  const int xm = min(lane & 15, a.M - 1);
  const __bf16* xl_row = reinterpret_cast<const __bf16*>(q4_xs) + (size_t)xm * a.K + g * 8;
  const float* xs_row = xsum + (size_t)xm * NB + g;

  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};   // sum_b s_nb T_b
  f32x4 corr = f32x4{0.f, 0.f, 0.f, 0.f};  // sum_b (128 s_nb + o_nb) X_b
  int cp_e = 0, buf = 0;

  // one item: the 4 MFMAs (one per 32-block, zero accumulator) issue back to back, THEN their per-block scale-and-add
  // (sched_barrier): interleaved, every FMA waited out its MFMA's latency (s_nop 2-7 each, profiles/r6).  `on` = 0
  // zeroes a padding item's contribution (past its wave's quads, or past the end), so no branch wraps the MFMAs.
  auto step = [&](const Quad& q, int p_raw, float on) {
    const int p = min(p_raw, KQ - 1);
    // this lane's weight row: the 4 block scales of the quad, and (for the correction MFMA) block 4p + g's
    // coefficient -- the 16-bit entry picked by selects, not a lane-divergent branch
    float sc[4], c2;
    const uint32_t wg = (g & 2) ? q.s[1] : q.s[0];
    const uint32_t vg = (g & 1) ? (wg >> 16) : (wg & 0xffffu);
    if constexpr (FMT == Q4F_0) {
#pragma unroll
      for (int s = 0; s < 4; ++s) sc[s] = on * q4_h2f(q.s[s >> 1] >> (16 * (s & 1)));
      c2 = (136.f * on) * q4_h2f(vg);  // 128 d + 8 d
    } else {
      const float d = on * q4_h2f(q.d), dmin = on * q4_h2f(q.d >> 16);
#pragma unroll
      for (int s = 0; s < 4; ++s) sc[s] = d * float((q.s[s >> 1] >> (16 * (s & 1))) & 0xffu);
      c2 = 128.f * d * float(vg & 0xffu) + dmin * float(vg >> 8);
    }
    f32x4 t[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      // rows >= M read the last row (their outputs are never stored; a row of D depends on that row of A only)
      const bf16x8 xv = *reinterpret_cast<const bf16x8*>(xl_row + p * 128 + s * 32);
      t[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xv, q4_frag(q.w[s]), f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
    // correction: A = the block sums (activation row m, block 4p + g), B = this lane's coefficient (weight row n,
    // block 4p + g); rows >= M hold the last row's sums, whose outputs the epilogue never stores
    corr = __builtin_amdgcn_mfma_f32_16x16x4f32(xs_row[p * 4], c2, corr, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 4; ++s) acc += t[s] * sc[s];
  };

  // tile end: this wave's partial D'[m = 4g + i][n = lane & 15] into LDS; wave 0 sums the waves and reads the
  // TRANSPOSE (the epilogues take lane L = (act row L & 15, weight rows 4 (L >> 4) + i))
  auto tile_end = [&]() {
    const f32x4 v = acc - corr;  // D'[m = 4g + i][n = lane & 15]
#pragma unroll
    for (int i = 0; i < 4; ++i) red[buf][wave][(4 * g + i) * 16 + (lane & 15)] = v[i];
    acc = f32x4{0.f, 0.f, 0.f, 0.f};
    corr = f32x4{0.f, 0.f, 0.f, 0.f};
    q4_barrier();
    if (wave == 0) {
      const int tile = cp_t;
      if (cp_t != (int)blockIdx.x) pre = epi_load_at<EPI>(a, tile, lane & 15, lane);
      auto unit_sum = [&](int L) -> f32x4 {  // lane L: activation row L & 15, weight rows 4 (L >> 4) + i
        const int m = L & 15, off = m * 16 + 4 * (L >> 4);
        f32x4 v = *reinterpret_cast<const f32x4*>(&red[buf][0][off]);
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v += *reinterpret_cast<const f32x4*>(&red[buf][w][off]);
        if constexpr (NORM) v *= rms_inv(row_ss[min(m, a.M - 1)], a.K, a.eps);
        return v;
      };
      if constexpr (EPI == EPI_F32) {  // the LM head: logits + chunk maxima
        const f32x4 v = unit_sum(lane);
        epi_store<EPI>(a, tile, lane & 15, lane, pre, [&](int) { return v; });
        epi_cmax(a, tile, lane & 15, lane, v);
      } else {
        epi_store<EPI>(a, tile, lane & 15, lane, pre, [&](int off) { return unit_sum(lane + off); });
      }
    }
    buf ^= 1;
  };

  for (int i0 = 0; i0 < n_pad; i0 += R) {
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int p = wave + cp_e * WAVES;
      const bool live = i0 + u < n_items;
      load_next(ring[(u + U) % (U + 1)]);
      step(ring[u], p, (live && p < KQ) ? 1.f : 0.f);
      if (live && cp_e == qmax - 1) tile_end();
      if (++cp_e == qmax) cp_e = 0, cp_t += G;
    }
  }
}

// ================================================================ launch
template <bool NORM, int EPI, int FMT>
static hipError_t q4_launch_w(int waves, const GemmArgs& a, const Q4Args& q, int grid, int npairs, hipStream_t st) {
  if (EPI != EPI_QKV_ROPE && waves == 8)  // (the fused QKV epilogue has no 8-wave instance: it spills there)
    hipLaunchKernelGGL((q4_stream_kernel<8, 4, EPI == EPI_QKV_ROPE ? EPI_BF16 : EPI, NORM, FMT>), dim3(grid),
                       dim3(512), 0, st, a, q, npairs);
  else
    hipLaunchKernelGGL((q4_stream_kernel<4, 4, EPI, NORM, FMT>), dim3(grid), dim3(256), 0, st, a, q, npairs);
  return hipGetLastError();
}

template <bool NORM, int FMT>
static hipError_t q4_launch(int epi, int waves, const GemmArgs& a, const Q4Args& q, int grid, int npairs,
                            hipStream_t st) {
  switch (epi) {
    case EPI_BF16: return q4_launch_w<NORM, EPI_BF16, FMT>(waves, a, q, grid, npairs, st);
    case EPI_RESID: return q4_launch_w<NORM, EPI_RESID, FMT>(waves, a, q, grid, npairs, st);
    case EPI_F32: return q4_launch_w<NORM, EPI_F32, FMT>(waves, a, q, grid, npairs, st);
    case EPI_SILU: return q4_launch_w<NORM, EPI_SILU, FMT>(waves, a, q, grid, npairs, st);
    case EPI_GELU: return q4_launch_w<NORM, EPI_GELU, FMT>(waves, a, q, grid, npairs, st);
    case EPI_QKV_ROPE: return q4_launch_w<NORM, EPI_QKV_ROPE, FMT>(4, a, q, grid, npairs, st);  // 8 waves spill it
    default: return hipErrorInvalidValue;
  }
}

// Waves per workgroup: 8 (2 workgroups per CU) where the quads per 8-wave pass leave every wave work and the rows'
// activations and block sums fit its 48 KiB copy; else 4 (4 per CU, 28 KiB); 0: the shape does not fit either.
static int q4_waves(int K, int M, int epi) {
  const int kq = K / 128;
  const bool fit8 = q4_lds_need(M, K) <= q4_xl_bytes<8>(), fit4 = q4_lds_need(M, K) <= q4_xl_bytes<4>();
  if (epi != EPI_QKV_ROPE && kq >= 24 && fit8) return 8;
  if (fit4) return 4;
  return (epi != EPI_QKV_ROPE && fit8) ? 8 : 0;
}

static int q4_rows(int K, int epi) {  // rows per launch at this K and epilogue (0: K too long)
  for (int m = 16; m >= 1; --m)
    if (q4_waves(K, m, epi)) return m;
  return 0;
}
CAIN_API int cain_gemm_q4_rows(int K, int epi) { return q4_rows(K, epi & EPI_MASK); }

CAIN_API float* cain_gemm_cmax_claim(int N);  // gemm.hip

// Same GEMM arguments as cain_gemm_w4 (gemm_w4.hip) plus the format (0 Q4_0, 1 Q4_K), its scale arrays and the
// RMSNorm gain to apply to the activations (null: none).  More rows than the LDS copy holds (cain_gemm_q4_rows) run
// on the tile kernel of gemm_qtile.hip, 64 rows per launch (cain_gemm_q_set_tile(0): as several stream launches).
CAIN_API int cain_gemm_q4(int fmt, const void* Wq, const void* sc, const void* dd, const float* gain, const void* X,
                          int ldx, int K, int N, int M, void* Y, int ldy, const float* bias, int norm, float eps,
                          const int* slot, const int* pos, const float* cos_t, const float* sin_t, void* kc,
                          void* vtc, int H, int Hkv, int hd, int T_max, int epi_flags, hipStream_t st) {
  const int epi = epi_flags & EPI_MASK;
  if (K % 256 || N % 16 || M < 1 || (fmt != Q4F_0 && fmt != Q4F_K) || !Wq || !sc || (fmt == Q4F_K && !dd)) return -1;
  if (epi == EPI_QKV_ROPE && (hd % 16 || (hd / 2) % 8)) return -1;
  const int rows = q4_rows(K, epi);
  if (rows == 0) return -1;
  const int n_cu = cain_cu_budget();
  float* cm = epi == EPI_F32 ? cain_gemm_cmax_claim(N) : nullptr;  // the LM head: the sampler's chunk maxima too
  // many rows (q_tile_selected: more than one pass of the stream kernel, by default): 64 rows per launch of the tile
  // kernel (gemm_qtile.hip), one pass over the weights each
  const bool tile = q_tile_selected(fmt, K, M, epi, rows);
  const int per = tile ? 64 : rows;
  for (int m0 = 0; m0 < M; m0 += per) {
    const int mc = std::min(per, M - m0);
    const int waves = tile ? 4 : q4_waves(K, mc, epi);  // > 0: mc <= rows
    GemmArgs a{};
    a.Wp = reinterpret_cast<const bf16x8*>(Wq);
    a.X = reinterpret_cast<const __bf16*>(X) + (size_t)m0 * ldx;
    a.ldx = ldx, a.K = K, a.N = N, a.M = mc, a.ldy = ldy, a.bias = bias;
    const size_t ybytes = epi == EPI_F32 ? 4 : 2;
    a.Y = static_cast<char*>(Y) + (size_t)m0 * ldy * ybytes;
    a.eps = eps;
    a.slot = slot ? slot + m0 : nullptr, a.pos = pos ? pos + m0 : nullptr, a.cos_t = cos_t, a.sin_t = sin_t;
    a.kc = reinterpret_cast<__bf16*>(kc), a.vtc = reinterpret_cast<__bf16*>(vtc);
    a.H = H, a.Hkv = Hkv, a.hd = hd, a.T_max = T_max, a.kv8 = (epi_flags & EPI_KV_FP8) ? 1 : 0;
    a.msplit = 1;
    if (cm) a.cmax = cm + (size_t)m0 * (N / 16), a.ld_cm = N / 16;
    if (tile) {
      const hipError_t e = q_tile_launch(fmt, a, sc, dd, gain, epi, norm != 0, 0, st);
      if (e != hipSuccess) return int(e);
      continue;
    }
    const Q4Args q{static_cast<const uint8_t*>(sc), static_cast<const uint32_t*>(dd), gain};
    const int npairs = N / 16;
    const int grid = std::min(npairs, n_cu * (waves == 8 ? 2 : 4));
    const hipError_t e = fmt == Q4F_0 ? (norm ? q4_launch<true, Q4F_0>(epi, waves, a, q, grid, npairs, st)
                                              : q4_launch<false, Q4F_0>(epi, waves, a, q, grid, npairs, st))
                                      : (norm ? q4_launch<true, Q4F_K>(epi, waves, a, q, grid, npairs, st)
                                              : q4_launch<false, Q4F_K>(epi, waves, a, q, grid, npairs, st));
    if (e != hipSuccess) return int(e);
  }
  return 0;
}
