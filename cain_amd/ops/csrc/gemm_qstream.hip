// GGUF block-quantised weights (llama.cpp's Q4_0, Q4_K and Q6_K: Ollama's default Q4_0 / Q4_K_M model builds) for
// single-stream / few-row decode, M <= 16 rows per launch (many rows: gemm_qtile.hip): the weights' VALUES as the
// file stores them, only their layout repacked.  gemm_w4.hip runs MXFP4, a different 4-bit grid, so a GGUF file
// reached it re-quantised; here the block values are exact.  One kernel body (qstream_body) serves the formats:
//
//   Q4_0: 32-element blocks, w = d * (q - 8), q in 0..15, fp16 d                          (4.5 bits per weight)
//   Q4_K: 256-element super-blocks of 8 blocks of 32, w = d * sc * q - dmin * m, q in 0..15, 6-bit sc / m per block,
//         fp16 d / dmin per super-block   (4.5 bits in the file, 4.625 here: the 6-bit pairs stored as bytes)
//   Q6_K: 256-element super-blocks of 16 groups of 16, w = d * sc * (q - 32), q in 0..63, int8 sc per group, fp16 d
//         per super-block                 (6.5625 bits in the file, 6.625 here: d stored as fp32)
//
// No block scale is exact in bf16 once multiplied in, so the codes go into the MFMA unscaled and each scale block's
// scale is applied to its own fp32 partial sum: the MFMA multiplies the ACTIVATIONS (A operand: rows = activation
// rows m) by the codes (B operand: columns = weight rows n), so one lane's four outputs share its weight row n and
// each lane needs just that row's block scales per 128-k quad (8 bytes, one load).  The codes enter as bf16 128 + q
// (exact: the byte q under the high byte 0x43, one v_perm per pair), so per scale block b
//
//   sum_k x_k w_k = s_b T_b - c_b X_b,    T_b = sum_k x_k (128 + q_k),  X_b = sum_k x_k
//
//                 block   MFMA for T_b, per quad            s_b      c_b                correction MFMAs per quad
//   Q4_0          32      4 x v_mfma_f32_16x16x32_bf16      d        136 d  (128 + 8)   1 x v_mfma_f32_16x16x4_f32
//   Q4_K          32      4 x v_mfma_f32_16x16x32_bf16      d sc     128 d sc + dmin m  1
//   Q6_K          16      8 x v_mfma_f32_16x16x16_bf16      d sc     160 d sc           2
//
// (a Q6_K scale covers 16 elements: a 16x16x32 would sum two groups into one accumulator; 8 of the narrower MFMAs
// take the time of the 4 wide ones).  s_b T_b is summed by 4 fp32 FMAs per MFMA, c_b X_b by the correction MFMAs
// over the block sums X of the staged activations, computed once per workgroup in LDS ([M][K / block] floats behind
// the rows: M K 2.125 bytes for Q4, 2.25 for Q6_K).  The products (128 + q) x are exact in fp32, so the cancellation
// of s T against c X costs ~1e-6 relative (Q6_K: at most 2^-24 * 191 |s| per element).
//
// RMSNorm gain: a GGUF file's gains stay separate from its quantised weights (folding them in would change the
// values), so the staging multiplies the activations by the gain (fp32 per k; null: none) after the row's sum of
// squares is taken from the raw values; the fused RMSNorm factor is applied at the end, as in every other kernel.
// Epilogues, the persistent tile stream and the register ring are gemm_w4.hip's stream kernel's.  `tile0` offsets
// the epilogue's (and the bias's) tile index while the weights are addressed from tile 0 of their own buffer, so the
// V rows of a fused QKV projection can be a Q6_K launch of their own behind a Q4 launch of the q / k rows.
//
// Layout (cain_amd/models/q4.py pack_q4 / pack_q6), lane = 16g + r: weight row 16t + r of tile t, per 128-k quad p.
//   Q4: codes Wq[(t*KQ + p)*64 + lane], 16 bytes: k = 128p + 32s + 8g + j at dword s, byte j & 3, nibble j >> 2 (low
//     nibbles j = 0..3, high 4..7) -- the four bytes of a dword turn into the eight bf16 of an MFMA operand with two
//     ANDs and four v_perm_b32.  Scales Q4_0: fp16 d[(t*KQ + p)*16 + r][4 blocks]; Q4_K: uint16 (sc | m << 8), same
//     shape, and fp16x2 (d, dmin)[(t*(KQ/2) + p/2)*16 + r].
//   Q6_K: 1536 bytes of codes per (t, p): [64 lanes x 16 bytes: low nibbles][64 lanes x 8 bytes: high bit pairs]; MFMA
//     s (group 8p + s) takes k = 128p + 16s + 4g + j from byte j of low dword s >> 1 (nibble s & 1) and of high dword
//     s >> 2 (bits 2 (s & 3) ..): the lane's 4 codes of an MFMA come out of one dword each.  Scales: int8
//     sc[(t*KQ + p)*16 + r][8 groups], then fp32 d[(t*(KQ/2) + p/2)*16 + r], then the optional fp32 gain over K.
#include <algorithm>

#include "common.h"
#include "gemm_epi.h"
#include "gemm_q.h"

struct QSArgs {
  const uint8_t* sc;   // block scales [tiles][KQ][16 rows] x 8 bytes: Q4_0 fp16 d, Q4_K (sc | m << 8), Q6_K int8
  const uint32_t* dd;  // super-block scales [tiles][KQ / 2][16 rows]: Q4_K fp16 (d, dmin), Q6_K fp32 d
  const float* gain;   // RMSNorm gain per k applied while staging (null: none)
};

template <int WAVES>
constexpr int q_xl_bytes() { return WAVES == 8 ? 57344 : 28672; }  // 2 x (56 + 16) KiB or 4 x (28 + 8) KiB per CU

// (the argument structs by value: by reference, two Q6_K instances took one VGPR more than as kernels of their own)
template <int FMT, int WAVES, int U, int EPI, bool NORM>
__device__ __forceinline__ void qstream_body(const GemmArgs a, const QSArgs q, int npairs, int tile0) {
  constexpr bool Q6 = FMT == Q6F_K;
  constexpr int BLK = Q6 ? 16 : 32;   // elements per scale block
  constexpr int CH = BLK / 8;         // 16-byte activation chunks per block: the lanes of a quad (Q4) or a pair (Q6_K)
  constexpr int CSH = Q6 ? 1 : 2;     // log2 CH
  constexpr int XLB = q_xl_bytes<WAVES>();
  constexpr int XCH = XLB / (WAVES * 64 * 16);  // 16-byte activation chunks staged per thread (upper bound)
  __shared__ __attribute__((aligned(16))) char q_xs[XLB];
  // per wave, its 16 x 16 partial in [activation row m][weight row n] order (the epilogues' lane order, read back
  // as one 16-byte vector per lane)
  __shared__ __attribute__((aligned(16))) float red[2][WAVES][256];
  __shared__ float row_ss[16];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int KQ = a.K >> 7;                 // 128-wide k quads
  const int NB = a.K >> (Q6 ? 4 : 5);      // scale blocks per row
  const int qmax = (KQ + WAVES - 1) / WAVES;
  const int G = gridDim.x;
  const int my_tiles = (npairs - (int)blockIdx.x + G - 1) / G;
  const int n_items = my_tiles * qmax;
  constexpr int R = U + 1;
  const int n_pad = (n_items + R - 1) / R * R;
  float* xsum = reinterpret_cast<float*>(q_xs + (size_t)a.M * a.K * 2);  // [M][NB] block sums of x'

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
    qu32x4 w;    // Q4: the lane's 32 codes; Q6_K: their low nibbles
    qu32x2 hi;   // Q6_K: the high bit pairs (Q4: never touched)
    qu32x2 s;    // this lane's weight row: the quad's block scales (Q4: 4 x 16 bits; Q6_K: 8 x int8)
    uint32_t d;  // the row's super-block scale: Q4_K fp16 (d, dmin), Q6_K fp32 d
  };
  const qu32x4* w4base = reinterpret_cast<const qu32x4*>(a.Wp) + lane;
  const uint8_t* w6base = reinterpret_cast<const uint8_t*>(a.Wp);
  const int row = lane & 15;
  int ld_t = blockIdx.x, ld_e = 0, ld_i = 0;
  const int last_t = (int)blockIdx.x + (my_tiles - 1) * G;
  auto load_next = [&](Quad& qd) {
    // past the end: re-load this wave's last item (a cache hit), never a branch around the load (gemm_w4.hip)
    const bool in = ld_i < n_items;
    const int p = min(wave + (in ? ld_e : qmax - 1) * WAVES, KQ - 1);
    const int t = in ? ld_t : last_t;
    const size_t tq = (size_t)t * KQ + p;
    if constexpr (Q6) {
      qd.w = __builtin_nontemporal_load(reinterpret_cast<const qu32x4*>(w6base + tq * 1536) + lane);
      qd.hi = __builtin_nontemporal_load(reinterpret_cast<const qu32x2*>(w6base + tq * 1536 + 1024) + lane);
    } else {
      qd.w = __builtin_nontemporal_load(w4base + tq * 64);
    }
    qd.s = __builtin_nontemporal_load(reinterpret_cast<const qu32x2*>(q.sc) + tq * 16 + row);
    if constexpr (FMT == Q4F_0) qd.d = 0;
    else qd.d = __builtin_nontemporal_load(q.dd + ((size_t)t * (KQ >> 1) + (p >> 1)) * 16 + row);
    ++ld_i;
    if (++ld_e == qmax) ld_e = 0, ld_t += G;
  };
  Quad ring[R];
#pragma unroll
  for (int u = 0; u < U; ++u) load_next(ring[u]);

  int cp_t = blockIdx.x;
  EpiIn pre{};
  if (wave == 0 && my_tiles > 0) pre = epi_load_at<EPI>(a, tile0 + cp_t, lane & 15, lane);
  const bool gained = q.gain != nullptr;
#pragma unroll
  for (int i = 0; i < XCH; ++i) {
    const int c = (int)threadIdx.x + i * WAVES * 64;
    if (c < nch) *reinterpret_cast<bf16x8*>(q_xs + (size_t)c * 16) = xst[i];
    if (!gained) {
      // the block sums straight from the staged registers: a block is CH consecutive chunks, i.e. the lanes of a
      // quad / pair (cpr = K / 8 is a multiple of 4, so none straddles a row's end), summed in a fixed order
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += bf2f(xst[i][j]);
      if constexpr (Q6) sum = q6_pair_sum(sum);
      else sum = q4_quad_sum(sum);
      if (c < nch && (c & (CH - 1)) == 0) xsum[c >> CSH] = sum;  // chunk c / CH = row * NB + block
    }
  }
  q_barrier();
  // sums of squares of the RAW rows (fixed order: wave w owns rows w, w + WAVES, ...); the first tile end's barrier
  // orders them before the epilogue reads them, unless the gain pass below rewrites the rows first
  if constexpr (NORM) {
    for (int r = wave; r < a.M; r += WAVES) {
      const char* xr = q_xs + (size_t)r * cpr * 16;
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
    if constexpr (NORM) q_barrier();  // the raw rows' sums of squares are taken
    for (int rb = threadIdx.x; rb < a.M * NB; rb += WAVES * 64) {
      const int r = rb / NB, b = rb - r * NB;
      bf16x8* xp = reinterpret_cast<bf16x8*>(q_xs + ((size_t)r * a.K + b * BLK) * 2);
      float sum = 0.f;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        bf16x8 x8 = xp[c];
        const f32x4 g0 = *reinterpret_cast<const f32x4*>(q.gain + b * BLK + c * 8);
        const f32x4 g1 = *reinterpret_cast<const f32x4*>(q.gain + b * BLK + c * 8 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) x8[j] = (__bf16)(bf2f(x8[j]) * g0[j]), x8[4 + j] = (__bf16)(bf2f(x8[4 + j]) * g1[j]);
        xp[c] = x8;
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += bf2f(x8[j]);
      }
      xsum[rb] = sum;
    }
    q_barrier();
  }

  // A operand: this lane's activation row m = lane & 15 (rows >= M read the last row: their outputs are never
  // stored, and a row of D depends on that row of A only), k group g
  const int g = lane >> 4;
  const int xm = min(lane & 15, a.M - 1);
  const __bf16* xl_row = reinterpret_cast<const __bf16*>(q_xs) + (size_t)xm * a.K + g * (BLK / 4);
  const float* xs_row = xsum + (size_t)xm * NB + g;

  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};   // sum_b s_b T_b
  f32x4 corr = f32x4{0.f, 0.f, 0.f, 0.f};  // sum_b c_b X_b
  int cp_e = 0, buf = 0;

  // one item: the MFMAs (one per scale block, zero accumulator) issue back to back, THEN their per-block scale-and-add
  // (sched_barrier): interleaved, every FMA waited out its MFMA's latency (s_nop 2-7 each, profiles/r6).  `on` = 0
  // zeroes a padding item's contribution (past its wave's quads, or past the end), so no branch wraps the MFMAs.
  auto step = [&](const Quad& qd, int p_raw, float on) {
    const int p = min(p_raw, KQ - 1);
    if constexpr (!Q6) {
      // this lane's weight row: the 4 block scales of the quad, and (for the correction MFMA) block 4p + g's
      // coefficient -- the 16-bit entry picked by selects, not a lane-divergent branch
      float sc[4], c2;
      const uint32_t wg = (g & 2) ? qd.s[1] : qd.s[0];
      const uint32_t vg = (g & 1) ? (wg >> 16) : (wg & 0xffffu);
      if constexpr (FMT == Q4F_0) {
#pragma unroll
        for (int s = 0; s < 4; ++s) sc[s] = on * q4_h2f(qd.s[s >> 1] >> (16 * (s & 1)));
        c2 = (136.f * on) * q4_h2f(vg);  // 128 d + 8 d
      } else {
        const float d = on * q4_h2f(qd.d), dmin = on * q4_h2f(qd.d >> 16);
#pragma unroll
        for (int s = 0; s < 4; ++s) sc[s] = d * float((qd.s[s >> 1] >> (16 * (s & 1))) & 0xffu);
        c2 = 128.f * d * float(vg & 0xffu) + dmin * float(vg >> 8);
      }
      f32x4 t[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bf16x8 xv = *reinterpret_cast<const bf16x8*>(xl_row + p * 128 + s * 32);
        t[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xv, q4_frag(qd.w[s]), f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      }
      // correction: A = the block sums (activation row m, block 4p + g), B = this lane's coefficient (weight row n,
      // block 4p + g); rows >= M hold the last row's sums, whose outputs the epilogue never stores
      corr = __builtin_amdgcn_mfma_f32_16x16x4f32(xs_row[p * 4], c2, corr, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < 4; ++s) acc += t[s] * sc[s];
    } else {
      const float d = on * __builtin_bit_cast(float, qd.d);
      float sc[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) sc[s] = d * q6_i8f(qd.s[s >> 2], s & 3);
      // the correction MFMAs' coefficients: groups 8p + g and 8p + 4 + g of this lane's weight row
      const float c0 = (160.f * d) * q6_i8f(qd.s[0], g), c1 = (160.f * d) * q6_i8f(qd.s[1], g);
      f32x4 t[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const qs16x4 xv = *reinterpret_cast<const qs16x4*>(xl_row + p * 128 + s * 16);
        t[s] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(xv, q6_frag(qd.w, qd.hi, s), f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      }
      // correction: A = the group sums (activation row m, group 8p + 4h + g), B = this lane's coefficient
      corr = __builtin_amdgcn_mfma_f32_16x16x4f32(xs_row[p * 8], c0, corr, 0, 0, 0);
      corr = __builtin_amdgcn_mfma_f32_16x16x4f32(xs_row[p * 8 + 4], c1, corr, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < 8; ++s) acc += t[s] * sc[s];
    }
  };

  // tile end: this wave's partial D'[m = 4g + i][n = lane & 15] into LDS; wave 0 sums the waves and reads the
  // TRANSPOSE (the epilogues take lane L = (act row L & 15, weight rows 4 (L >> 4) + i))
  auto tile_end = [&]() {
    const f32x4 v = acc - corr;  // D'[m = 4g + i][n = lane & 15]
#pragma unroll
    for (int i = 0; i < 4; ++i) red[buf][wave][(4 * g + i) * 16 + (lane & 15)] = v[i];
    acc = f32x4{0.f, 0.f, 0.f, 0.f};
    corr = f32x4{0.f, 0.f, 0.f, 0.f};
    q_barrier();
    if (wave == 0) {
      const int tile = tile0 + cp_t;
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

template <int WAVES, int U, int EPI, bool NORM, int FMT>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) void q4_stream_kernel(
    const GemmArgs a, const QSArgs q, int npairs) {
  qstream_body<FMT, WAVES, U, EPI, NORM>(a, q, npairs, 0);
}

template <int WAVES, int U, int EPI, bool NORM>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) void q6_stream_kernel(
    const GemmArgs a, const QSArgs q, int npairs, int tile0) {
  qstream_body<Q6F_K, WAVES, U, EPI, NORM>(a, q, npairs, tile0);
}

// ================================================================ launch
struct QSLaunch {
  const GemmArgs& a;
  const QSArgs& q;
  int waves, grid, npairs, tile0;
  hipStream_t st;
};

template <int FMT, int WAVES, int U, int EPI, bool NORM>
static hipError_t qs_launch_one(const QSLaunch& l) {
  if constexpr (FMT == Q6F_K)
    hipLaunchKernelGGL((q6_stream_kernel<WAVES, U, EPI, NORM>), dim3(l.grid), dim3(WAVES * 64), 0, l.st, l.a, l.q,
                       l.npairs, l.tile0);
  else
    hipLaunchKernelGGL((q4_stream_kernel<WAVES, U, EPI, NORM, FMT>), dim3(l.grid), dim3(WAVES * 64), 0, l.st, l.a, l.q,
                       l.npairs);
  return hipGetLastError();
}

// The instance set.  The fused QKV epilogue has no 8-wave instance (it spills there), and on Q6_K its inputs leave
// registers for a ring of 3 items only (U = 2; 5 items spill ~240 VGPRs).  Q6_K has no gate/up activation epilogue:
// a Q6_K gate / up tensor is re-quantised at load (models/q4.py).
static bool q_stream_instance(int fmt, int epi) {
  if (epi < EPI_BF16 || epi > EPI_QKV_ROPE) return false;
  return !(fmt == Q6F_K && (epi == EPI_SILU || epi == EPI_GELU));
}

template <int FMT, bool NORM, int EPI>
static hipError_t qs_launch_w(const QSLaunch& l) {
  if constexpr (FMT == Q6F_K && (EPI == EPI_SILU || EPI == EPI_GELU)) {
    return hipErrorInvalidValue;
  } else if constexpr (EPI == EPI_QKV_ROPE) {
    return qs_launch_one<FMT, 4, FMT == Q6F_K ? 2 : 4, EPI, NORM>(l);
  } else {
    return l.waves == 8 ? qs_launch_one<FMT, 8, 4, EPI, NORM>(l) : qs_launch_one<FMT, 4, 4, EPI, NORM>(l);
  }
}

template <int FMT, bool NORM>
static hipError_t qs_launch_epi(int epi, const QSLaunch& l) {
  switch (epi) {
    case EPI_BF16: return qs_launch_w<FMT, NORM, EPI_BF16>(l);
    case EPI_RESID: return qs_launch_w<FMT, NORM, EPI_RESID>(l);
    case EPI_F32: return qs_launch_w<FMT, NORM, EPI_F32>(l);
    case EPI_SILU: return qs_launch_w<FMT, NORM, EPI_SILU>(l);
    case EPI_GELU: return qs_launch_w<FMT, NORM, EPI_GELU>(l);
    case EPI_QKV_ROPE: return qs_launch_w<FMT, NORM, EPI_QKV_ROPE>(l);
    default: return hipErrorInvalidValue;
  }
}

static hipError_t qs_launch(int fmt, int epi, bool norm, const QSLaunch& l) {
  switch (fmt) {
    case Q4F_0: return norm ? qs_launch_epi<Q4F_0, true>(epi, l) : qs_launch_epi<Q4F_0, false>(epi, l);
    case Q4F_K: return norm ? qs_launch_epi<Q4F_K, true>(epi, l) : qs_launch_epi<Q4F_K, false>(epi, l);
    case Q6F_K: return norm ? qs_launch_epi<Q6F_K, true>(epi, l) : qs_launch_epi<Q6F_K, false>(epi, l);
    default: return hipErrorInvalidValue;
  }
}

// activation bytes + their block sums (floats) that the LDS copy holds for M rows of K
static long long q_lds_need(int fmt, int M, int K) {
  return (long long)M * K * 2 + (long long)M * (K / (fmt == Q6F_K ? 16 : 32)) * 4;
}

// Waves per workgroup: 8 (2 workgroups per CU) where the quads per 8-wave pass leave every wave work and the rows'
// activations and block sums fit its 56 KiB copy; else 4 (4 per CU, 28 KiB); 0: the shape does not fit either.
static int q_stream_waves(int fmt, int K, int M, int epi) {
  const int kq = K / 128;
  const bool fit8 = q_lds_need(fmt, M, K) <= q_xl_bytes<8>(), fit4 = q_lds_need(fmt, M, K) <= q_xl_bytes<4>();
  if (epi != EPI_QKV_ROPE && kq >= 24 && fit8) return 8;
  if (fit4) return 4;
  return (epi != EPI_QKV_ROPE && fit8) ? 8 : 0;
}

// rows per launch at this K and epilogue (0: K too long, or not whole super-blocks)
static int q_stream_rows(int fmt, int K, int epi) {
  if (K < 256 || K % 256) return 0;
  for (int m = 16; m >= 1; --m)
    if (q_stream_waves(fmt, K, m, epi)) return m;
  return 0;
}

// One GGUF GEMM (g->fmt: Q4_0, Q4_K or Q6_K; sc / dd: the format's scale arrays; gain: the RMSNorm gain to apply to the
// activations, null: none): the few-row stream kernels above, or -- more rows than their LDS copy holds
// (q_stream_rows), where q_tile_selected() -- the tile kernels of gemm_qtile.hip, 64 rows per launch, one pass over the
// weights each (cain_gemm_q_set_tile(0): as several stream launches).  `tile0` (Q6_K only): the global 16-row tile the
// first of the N rows is in the epilogue's eyes (output columns, bias, QKV head / V row); the weights and scales are
// addressed from tile 0 of their own buffers.  A shape or (format, epilogue) pair without a kernel is refused (-1)
// before any launch.
CAIN_API int cain_gemm_gguf(const CainGemm* g, hipStream_t st) {
  const int fmt = g->fmt, K = g->K, N = g->N, M = g->M, tile0 = g->tile0, norm = g->norm, epi = g->epi & EPI_MASK;
  const void *sc = g->sc, *dd = g->dd;
  const float* gain = g->gain;
  if (tile0 != 0 && fmt != Q6F_K) return -1;  // first of all: a tile offset is Q6_K's alone
  if (K < 256 || K % 256 || N < 16 || N % 16 || M < 1 || tile0 < 0 || fmt < Q4F_0 || fmt > Q6F_K) return -1;
  if (!g->W || !sc || (fmt != Q4F_0 && !dd) || !q_stream_instance(fmt, epi)) return -1;
  GemmArgs all;
  if (!gemm_args(*g, all)) return -1;
  all.msplit = 1;
  const int rows = q_stream_rows(fmt, K, epi);
  if (rows == 0) return -1;
  const bool tile = q_tile_selected(fmt, K, M, epi, rows);
  const int per = tile ? 64 : rows;
  const int n_cu = cain_cu_budget();
  // the LM head: the sampler's chunk maxima too (a launch of rows behind tile 0 does not own the buffer)
  float* cm = (epi == EPI_F32 && tile0 == 0) ? cain_gemm_cmax_claim(N) : nullptr;
  for (int m0 = 0; m0 < M; m0 += per) {
    const int mc = std::min(per, M - m0);
    GemmArgs a = all;  // rows m0 .. m0 + mc
    a.X += (size_t)m0 * a.ldx;
    a.M = mc;
    a.Y = static_cast<char*>(a.Y) + (size_t)m0 * a.ldy * (epi == EPI_F32 ? 4 : 2);
    if (a.slot) a.slot += m0;
    if (a.pos) a.pos += m0;
    if (cm) a.cmax = cm + (size_t)m0 * (N / 16), a.ld_cm = N / 16;
    if (tile) {
      const hipError_t e = q_tile_launch(fmt, a, sc, dd, gain, epi, norm != 0, tile0, st);
      if (e != hipSuccess) return int(e);
      continue;
    }
    // the only guard that the LDS copy holds mc x K; never taken: q_lds_need is monotone in M and mc <= rows, so
    // q_stream_waves(fmt, K, mc, epi) > 0 for every launch once it is for `rows`
    const int waves = q_stream_waves(fmt, K, mc, epi);
    if (waves == 0) return -1;
    const QSArgs q{static_cast<const uint8_t*>(sc), static_cast<const uint32_t*>(dd), gain};
    const int npairs = N / 16;
    const int grid = std::min(npairs, n_cu * (waves == 8 ? 2 : 4));
    const hipError_t e = qs_launch(fmt, epi, norm != 0, QSLaunch{a, q, waves, grid, npairs, tile0, st});
    if (e != hipSuccess) return int(e);
  }
  return 0;
}

CAIN_API int cain_gemm_q4_rows(int K, int epi) { return q_stream_rows(Q4F_0, K, epi & EPI_MASK); }  // Q4_K: the same
CAIN_API int cain_gemm_q6_rows(int K, int epi) { return q_stream_rows(Q6F_K, K, epi & EPI_MASK); }
