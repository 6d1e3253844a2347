// Shared by the GGUF weight kernels (gemm_qstream.hip: the few-row stream kernels; gemm_qtile.hip: the many-row
// tile kernels): the formats, the code -> bf16 decodes, the small lane sums and the barrier.  The formats, their
// arithmetic and the packed layouts are in gemm_qstream.hip's header (cain_amd/models/q4.py pack_q4 / pack_q6).
#pragma once
#include "common.h"

enum { Q4F_0 = 0, Q4F_K = 1, Q6F_K = 2 };  // models/q4.py Q4_0, Q4_K, Q6_K

typedef uint32_t qu32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t qu32x2 __attribute__((ext_vector_type(2)));
typedef short qs16x4 __attribute__((ext_vector_type(4)));

// workgroup barrier behind this wave's LDS accesses only (global loads stay in flight across it)
__device__ __forceinline__ void q_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// four codes (one byte lane per k: low nibble k = j, high nibble k = j + 4, j = 0..3) -> bf16 128 + q, k order
__device__ __forceinline__ bf16x8 q4_frag(uint32_t w) {
  const uint32_t lo = w & 0x0f0f0f0fu, hi = (w >> 4) & 0x0f0f0f0fu;
  // v_perm_b32 selector bytes: 0-3 pick the second operand's bytes, 4-7 the first's; 0x43 is bf16 128's high byte
  constexpr uint32_t C43 = 0x43434343u;
  const uint32_t p0 = __builtin_amdgcn_perm(C43, lo, 0x05010400u);  // k0, k1: [lo.b0, 43, lo.b1, 43]
  const uint32_t p1 = __builtin_amdgcn_perm(C43, lo, 0x05030402u);  // k2, k3
  const uint32_t p2 = __builtin_amdgcn_perm(C43, hi, 0x05010400u);  // k4, k5
  const uint32_t p3 = __builtin_amdgcn_perm(C43, hi, 0x05030402u);  // k6, k7
  return __builtin_bit_cast(bf16x8, qu32x4{p0, p1, p2, p3});
}

__device__ __forceinline__ float q4_h2f(uint32_t h) { return float(__builtin_bit_cast(_Float16, (uint16_t)h)); }

// sum over the 4 lanes of a quad (4j .. 4j + 3) by two DPP quad permutations (xor 1, xor 2): no LDS round trip (the
// ds_bpermute of __shfl_xor cost ~6 % of qwen2:1.5b's batch-1 rate in the staging); every lane gets the same value
__device__ __forceinline__ float q4_quad_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
  return v;
}

// the 4 codes of Q6_K MFMA s (bytes j = 0..3 of one low and one high dword) -> bf16 128 + q, k order
__device__ __forceinline__ qs16x4 q6_frag(const qu32x4& lo, const qu32x2& hi, int s) {
  const uint32_t l = (lo[s >> 1] >> (4 * (s & 1))) & 0x0f0f0f0fu;
  const int sh = 2 * (s & 3);  // the pair's bit position; it goes to bits 4..5 of its byte
  const uint32_t h = (sh <= 4 ? hi[s >> 2] << (4 - sh) : hi[s >> 2] >> (sh - 4)) & 0x30303030u;
  const uint32_t b = l | h;
  // v_perm_b32 selector bytes: 0-3 pick the second operand's bytes, 4-7 the first's; 0x43 is bf16 128's high byte
  constexpr uint32_t C43 = 0x43434343u;
  const uint32_t p0 = __builtin_amdgcn_perm(C43, b, 0x05010400u);  // k0, k1
  const uint32_t p1 = __builtin_amdgcn_perm(C43, b, 0x05030402u);  // k2, k3
  return __builtin_bit_cast(qs16x4, qu32x2{p0, p1});
}

__device__ __forceinline__ float q6_i8f(uint32_t w, int byte) { return float(int(int8_t(w >> (8 * byte)))); }

// sum over the 2 lanes of a pair (2j, 2j + 1) by one DPP quad permutation (xor 1); both lanes get the same value
__device__ __forceinline__ float q6_pair_sum(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
}

// ---- the many-row path (gemm_qtile.hip), called by cain_gemm_gguf when q_tile_selected()
struct GemmArgs;
// whether M rows of a (fmt, K, epi) GEMM run on the tile kernels under the current mode (cain_gemm_q_set_tile);
// `stream_rows`: the stream kernel's rows per launch at (K, epi), > 0
bool q_tile_selected(int fmt, int K, int M, int epi, int stream_rows);
// one launch of up to 64 rows (a.M; every row pointer of `a` already offset to the launch's first row)
hipError_t q_tile_launch(int fmt, const GemmArgs& a, const void* sc, const void* dd, const float* gain, int epi,
                         bool norm, int tile0, hipStream_t st);
