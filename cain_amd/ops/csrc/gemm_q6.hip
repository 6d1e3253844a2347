// GGUF Q6_K weights (llama.cpp's 6-bit K-quant: the output head, attn_v and ffn_down tensors of a Q4_K_M file) for
// single-stream / few-row decode, M <= 16 rows per launch: the block VALUES as the file stores them, only their
// layout repacked (gemm_q4.hip's scheme, which this kernel follows part by part).
//
//   Q6_K: 256-element super-blocks of 16 groups of 16, w = d * sc * (q - 32), q in 0..63, int8 sc per group, fp16 d
//         per super-block (6.5625 bits per weight in the file, 6.625 here: d stored as fp32)
//
// The codes enter the bf16 MFMA unscaled as 128 + q (128..191 is exact in bf16: the byte q under the high byte 0x43,
// one v_perm per pair) and each group's scale is applied to its own fp32 partial sum.  A scale covers 16 elements,
// so one v_mfma_f32_16x16x16_bf16 per group (a 16x16x32 would sum two groups into one accumulator): 8 per 128-k
// quad, the MFMA time of gemm_q4.hip's 4 x 16x16x32.  Per group g
//
//   sum_k x_k w_k = s_g (T_g - 160 X_g),   s_g = d sc_g,  T_g = sum_k x_k (128 + q_k),  X_g = sum_k x_k
//
// with the s_g T_g summed by 4 fp32 FMAs per MFMA and the 160 s_g X_g by two v_mfma_f32_16x16x4_f32 per quad over the
// group sums of the staged activations (LDS, [M][K / 16] floats: M K 2.25 bytes with the rows themselves).  The
// products (128 + q) x are exact in fp32; the cancellation of s T against 160 s X leaves at most 2^-24 * 191 |s| per
// element.  RMSNorm gain, epilogues, the persistent tile stream and the register ring are gemm_q4.hip's; `tile0`
// offsets the epilogue's (and the bias's) tile index while the weights are addressed from tile 0 of their own
// buffer, so the V rows of a fused QKV projection can be a launch of their own behind a Q4 launch of the q / k rows.
//
// Layout (cain_amd/models/q4.py pack_q6): per (tile t, quad p) 1536 bytes of codes: [64 lanes x 16 bytes: low nibbles]
// [64 lanes x 8 bytes: high bit pairs], lane = 16g + r: weight row 16t + r; MFMA s (group 8p + s) takes k = 128p + 16s
// + 4g + j from byte j of low dword s >> 1 (nibble s & 1) and of high dword s >> 2 (bits 2 (s & 3) ..): the lane's 4
// codes of an MFMA come out of one dword each.  Scales: int8 sc[(t*KQ + p)*16 + r][8 groups], then fp32
// d[(t*(KQ/2) + p/2)*16 + r], then the optional fp32 gain over K.
#include <algorithm>

#include "common.h"
#include "gemm_epi.h"
#include "gemm_q.h"

struct Q6Args {
  const uint8_t* sc;  // int8 group scales [tiles][KQ][16 rows][8 groups]
  const float* d;     // super-block scales [tiles][KQ / 2][16 rows]
  const float* gain;  // RMSNorm gain per k applied while staging (null: none)
};

__device__ __forceinline__ void q6_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int WAVES>
constexpr int q6_xl_bytes() { return WAVES == 8 ? 57344 : 28672; }  // as gemm_q4.hip: 2 or 4 workgroups per CU

// activation bytes + their group sums (floats) that the LDS copy holds for M rows of K
__host__ __device__ constexpr long long q6_lds_need(int M, int K) { return (long long)M * K * 2 + (long long)M * (K / 16) * 4; }

template <int WAVES, int U, int EPI, bool NORM>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) void q6_stream_kernel(
    const GemmArgs a, const Q6Args q6, int npairs, int tile0) {
  constexpr int XLB = q6_xl_bytes<WAVES>();
  constexpr int XCH = XLB / (WAVES * 64 * 16);  // 16-byte activation chunks staged per thread (upper bound)
  __shared__ __attribute__((aligned(16))) char q6_xs[XLB];
  __shared__ __attribute__((aligned(16))) float red[2][WAVES][256];
  __shared__ float row_ss[16];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int KQ = a.K >> 7;  // 128-wide k quads
  const int NG = a.K >> 4;  // 16-element scale groups per row
  const int qmax = (KQ + WAVES - 1) / WAVES;
  const int G = gridDim.x;
  const int my_tiles = (npairs - (int)blockIdx.x + G - 1) / G;
  const int n_items = my_tiles * qmax;
  constexpr int R = U + 1;
  const int n_pad = (n_items + R - 1) / R * R;
  float* xsum = reinterpret_cast<float*>(q6_xs + (size_t)a.M * a.K * 2);  // [M][NG] group sums of x'

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
    q6u32x4 lo;  // low nibbles of the lane's 32 codes
    q6u32x2 hi;  // their high bit pairs
    q6u32x2 s;   // this lane's weight row: the quad's 8 int8 group scales
    float d;     // the row's super-block scale
  };
  const uint8_t* wbase = reinterpret_cast<const uint8_t*>(a.Wp);
  const int row = lane & 15;
  int ld_t = blockIdx.x, ld_e = 0, ld_i = 0;
  const int last_t = (int)blockIdx.x + (my_tiles - 1) * G;
  auto load_next = [&](Quad& q) {
    // past the end: re-load this wave's last item (a cache hit), never a branch around the load (gemm_w4.hip)
    const bool in = ld_i < n_items;
    const int p = min(wave + (in ? ld_e : qmax - 1) * WAVES, KQ - 1);
    const int t = in ? ld_t : last_t;
    const size_t tq = (size_t)t * KQ + p;
    q.lo = __builtin_nontemporal_load(reinterpret_cast<const q6u32x4*>(wbase + tq * 1536) + lane);
    q.hi = __builtin_nontemporal_load(reinterpret_cast<const q6u32x2*>(wbase + tq * 1536 + 1024) + lane);
    q.s = __builtin_nontemporal_load(reinterpret_cast<const q6u32x2*>(q6.sc) + tq * 16 + row);
    q.d = __builtin_nontemporal_load(q6.d + ((size_t)t * (KQ >> 1) + (p >> 1)) * 16 + row);
    ++ld_i;
    if (++ld_e == qmax) ld_e = 0, ld_t += G;
  };
  Quad ring[R];
#pragma unroll
  for (int u = 0; u < U; ++u) load_next(ring[u]);

  int cp_t = blockIdx.x;
  EpiIn pre{};
  if (wave == 0 && my_tiles > 0) pre = epi_load_at<EPI>(a, tile0 + cp_t, lane & 15, lane);
  const bool gained = q6.gain != nullptr;
#pragma unroll
  for (int i = 0; i < XCH; ++i) {
    const int c = (int)threadIdx.x + i * WAVES * 64;
    if (c < nch) *reinterpret_cast<bf16x8*>(q6_xs + (size_t)c * 16) = xst[i];
    if (!gained) {
      // the group sums straight from the staged registers: a 16-element group is 2 consecutive chunks, i.e. the 2
      // lanes of a pair (cpr = K / 8 is even, so a pair never straddles the end), summed in a fixed order
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += bf2f(xst[i][j]);
      sum = q6_pair_sum(sum);
      if (c < nch && (c & 1) == 0) xsum[c >> 1] = sum;  // chunk c / 2 = row * NG + group
    }
  }
  q6_barrier();
  // sums of squares of the RAW rows (fixed order: wave w owns rows w, w + WAVES, ...)
  if constexpr (NORM) {
    for (int r = wave; r < a.M; r += WAVES) {
      const char* xr = q6_xs + (size_t)r * cpr * 16;
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
    // a separate gain (a GGUF file's values): x' = bf16(x * gain) in place, then the group sums of x' (the values
    // the MFMAs multiply), one thread per (row, group)
    if constexpr (NORM) q6_barrier();  // the raw rows' sums of squares are taken
    for (int rb = threadIdx.x; rb < a.M * NG; rb += WAVES * 64) {
      const int r = rb / NG, b = rb - r * NG;
      bf16x8* xp = reinterpret_cast<bf16x8*>(q6_xs + ((size_t)r * a.K + b * 16) * 2);
      float sum = 0.f;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        bf16x8 x8 = xp[c];
        const f32x4 g0 = *reinterpret_cast<const f32x4*>(q6.gain + b * 16 + c * 8);
        const f32x4 g1 = *reinterpret_cast<const f32x4*>(q6.gain + b * 16 + c * 8 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) x8[j] = (__bf16)(bf2f(x8[j]) * g0[j]), x8[4 + j] = (__bf16)(bf2f(x8[4 + j]) * g1[j]);
        xp[c] = x8;
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += bf2f(x8[j]);
      }
      xsum[rb] = sum;
    }
    q6_barrier();
  }

  // A operand: this lane's activation row m = lane & 15 (rows >= M multiply the last row), k group g
  const int g = lane >> 4;
  const int xm = min(lane & 15, a.M - 1);
  const __bf16* xl_row = reinterpret_cast<const __bf16*>(q6_xs) + (size_t)xm * a.K + g * 4;
  const float* xs_row = xsum + (size_t)xm * NG + g;

  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};   // sum_g s_ng T_g
  f32x4 corr = f32x4{0.f, 0.f, 0.f, 0.f};  // sum_g 160 s_ng X_g
  int cp_e = 0, buf = 0;

  // one item: the 8 MFMAs (one per 16-group, zero accumulator) issue back to back, THEN their per-group scale-and-add
  // (gemm_q4.hip step).  `on` = 0 zeroes a padding item's contribution, so no branch wraps the MFMAs.
  auto step = [&](const Quad& q, int p_raw, float on) {
    const int p = min(p_raw, KQ - 1);
    const float d = on * q.d;
    float sc[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) sc[s] = d * q6_i8f(q.s[s >> 2], s & 3);
    // the correction MFMAs' coefficients: groups 8p + g and 8p + 4 + g of this lane's weight row
    const float c0 = (160.f * d) * q6_i8f(q.s[0], g), c1 = (160.f * d) * q6_i8f(q.s[1], g);
    f32x4 t[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const q6s16x4 xv = *reinterpret_cast<const q6s16x4*>(xl_row + p * 128 + s * 16);
      t[s] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(xv, q6_frag(q.lo, q.hi, s), f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
    // correction: A = the group sums (activation row m, group 8p + 4h + g), B = this lane's coefficient
    corr = __builtin_amdgcn_mfma_f32_16x16x4f32(xs_row[p * 8], c0, corr, 0, 0, 0);
    corr = __builtin_amdgcn_mfma_f32_16x16x4f32(xs_row[p * 8 + 4], c1, corr, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 8; ++s) acc += t[s] * sc[s];
  };

  // tile end: this wave's partial D'[m = 4g + i][n = lane & 15] into LDS; wave 0 sums the waves and reads the
  // TRANSPOSE (the epilogues take lane L = (act row L & 15, weight rows 4 (L >> 4) + i))
  auto tile_end = [&]() {
    const f32x4 v = acc - corr;
#pragma unroll
    for (int i = 0; i < 4; ++i) red[buf][wave][(4 * g + i) * 16 + (lane & 15)] = v[i];
    acc = f32x4{0.f, 0.f, 0.f, 0.f};
    corr = f32x4{0.f, 0.f, 0.f, 0.f};
    q6_barrier();
    if (wave == 0) {
      const int tile = tile0 + cp_t;
      if (cp_t != (int)blockIdx.x) pre = epi_load_at<EPI>(a, tile, lane & 15, lane);
      auto unit_sum = [&](int L) -> f32x4 {
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
template <bool NORM, int EPI>
static hipError_t q6_launch_w(int waves, const GemmArgs& a, const Q6Args& q, int grid, int npairs, int tile0,
                              hipStream_t st) {
  if (EPI != EPI_QKV_ROPE && waves == 8)  // (no 8-wave instance of the fused QKV epilogue, as gemm_q4.hip)
    hipLaunchKernelGGL((q6_stream_kernel<8, 4, EPI == EPI_QKV_ROPE ? EPI_BF16 : EPI, NORM>), dim3(grid), dim3(512), 0,
                       st, a, q, npairs, tile0);
  else  // the fused QKV epilogue's inputs leave registers for a ring of 3 items only (5 spill ~240 VGPRs)
    hipLaunchKernelGGL((q6_stream_kernel<4, EPI == EPI_QKV_ROPE ? 2 : 4, EPI, NORM>), dim3(grid), dim3(256), 0, st, a,
                       q, npairs, tile0);
  return hipGetLastError();
}

// the gate/up activation epilogues are not instantiated: a Q6_K gate / up tensor is re-quantised at load (models/q4.py)
template <bool NORM>
static hipError_t q6_launch(int epi, int waves, const GemmArgs& a, const Q6Args& q, int grid, int npairs, int tile0,
                            hipStream_t st) {
  switch (epi) {
    case EPI_BF16: return q6_launch_w<NORM, EPI_BF16>(waves, a, q, grid, npairs, tile0, st);
    case EPI_RESID: return q6_launch_w<NORM, EPI_RESID>(waves, a, q, grid, npairs, tile0, st);
    case EPI_F32: return q6_launch_w<NORM, EPI_F32>(waves, a, q, grid, npairs, tile0, st);
    case EPI_QKV_ROPE: return q6_launch_w<NORM, EPI_QKV_ROPE>(4, a, q, grid, npairs, tile0, st);
    default: return hipErrorInvalidValue;
  }
}

// Waves per workgroup, as gemm_q4.hip's rule on this kernel's LDS need; 0: the rows do not fit either copy.
static int q6_waves(int K, int M, int epi) {
  const int kq = K / 128;
  const bool fit8 = q6_lds_need(M, K) <= q6_xl_bytes<8>(), fit4 = q6_lds_need(M, K) <= q6_xl_bytes<4>();
  if (epi != EPI_QKV_ROPE && kq >= 24 && fit8) return 8;
  if (fit4) return 4;
  return (epi != EPI_QKV_ROPE && fit8) ? 8 : 0;
}

static int q6_rows(int K, int epi) {  // rows per launch at this K and epilogue (0: K too long)
  if (K < 256 || K % 256) return 0;
  for (int m = 16; m >= 1; --m)
    if (q6_waves(K, m, epi)) return m;
  return 0;
}
CAIN_API int cain_gemm_q6_rows(int K, int epi) { return q6_rows(K, epi & EPI_MASK); }

CAIN_API float* cain_gemm_cmax_claim(int N);  // gemm.hip

// cain_gemm_q4's arguments (fmt: 2, Q6_K; sc: the int8 group scales, dd: the fp32 super-block scales) plus `tile0`,
// the global 16-row tile the first of the N rows is in the epilogue's eyes (output columns, bias, QKV head / V row);
// the weights and scales are addressed from tile 0 of their own buffers.  M > rows runs as several launches; a
// shape whose rows do not fit the LDS copy is refused before anything is launched.
CAIN_API int cain_gemm_q6(int fmt, const void* Wq, const void* sc, const void* dd, const float* gain, const void* X,
                          int ldx, int K, int N, int M, void* Y, int ldy, const float* bias, int norm, float eps,
                          const int* slot, const int* pos, const float* cos_t, const float* sin_t, void* kc,
                          void* vtc, int H, int Hkv, int hd, int T_max, int epi_flags, int tile0, hipStream_t st) {
  const int epi = epi_flags & EPI_MASK;
  if (K < 256 || K % 256 || N < 16 || N % 16 || M < 1 || tile0 < 0 || fmt != Q6F_K || !Wq || !sc || !dd) return -1;
  if (epi != EPI_BF16 && epi != EPI_RESID && epi != EPI_F32 && epi != EPI_QKV_ROPE) return -1;
  if (epi == EPI_QKV_ROPE && (hd % 16 || (hd / 2) % 8)) return -1;
  const int rows = q6_rows(K, epi);
  if (rows == 0) return -1;
  // many rows (q_tile_selected: more than one pass of the stream kernel, by default): 64 rows per launch of the tile
  // kernel (gemm_qtile.hip), one pass over the weights each
  const bool tile = q_tile_selected(fmt, K, M, epi, rows);
  const int per = tile ? 64 : rows;
  for (int m0 = 0; !tile && m0 < M; m0 += rows) {  // every launch's rows must fit before the first is made
    const int mc = std::min(rows, M - m0);
    const int waves = q6_waves(K, mc, epi);
    if (waves == 0 || q6_lds_need(mc, K) > (waves == 8 ? q6_xl_bytes<8>() : q6_xl_bytes<4>())) return -1;
  }
  const int n_cu = cain_cu_budget();
  float* cm = (epi == EPI_F32 && tile0 == 0) ? cain_gemm_cmax_claim(N) : nullptr;  // the LM head's chunk maxima
  for (int m0 = 0; m0 < M; m0 += per) {
    const int mc = std::min(per, M - m0);
    const int waves = tile ? 4 : q6_waves(K, mc, epi);
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
      const hipError_t e = q_tile_launch(fmt, a, sc, dd, gain, epi, norm != 0, tile0, st);
      if (e != hipSuccess) return int(e);
      continue;
    }
    const Q6Args q{static_cast<const uint8_t*>(sc), static_cast<const float*>(dd), gain};
    const int npairs = N / 16;
    const int grid = std::min(npairs, n_cu * (waves == 8 ? 2 : 4));
    const hipError_t e = norm ? q6_launch<true>(epi, waves, a, q, grid, npairs, tile0, st)
                              : q6_launch<false>(epi, waves, a, q, grid, npairs, tile0, st);
    if (e != hipSuccess) return int(e);
  }
  return 0;
}
