// What the wide-batch GEMMs share: bf16 (wgemm.hip) and fp8 W8A8 / MXFP4 W4A8 (wgemm8.hip).  The LDS-DMA
// primitives (also used by attention.hip), the ring loader (RingLoader: sources, issue order, counted waits, the
// loader waves' loop), the workgroup placement, the fp16 slab store, and on the host the split rule (wg_split),
// the epilogue and split-count switches and the launch with dynamic LDS.  The compute loops, the ks == 1
// epilogues and the split-K combines differ per format and stay in the two .hip files.
#pragma once
#include <algorithm>
#include <type_traits>
#include <utility>

#include "common.h"
#include "gemm_epi.h"

struct WgArgs {
  int ks;           // k-splits (workgroups per column block)
  int kst;          // ring stages per split
  float* part;      // [ks][n_units][64 lanes] f32x4 or f16x4 slabs (ks > 1)
  float* part_ss;   // [nblk][ks][BM] per-row partial sums of squares (ks > 1 && NORM)
  uint8_t* part_ex; // [ks][n_units][64 lanes] power-of-two exponent of each non-NORM fp16 slab lane (value = half * 2^ex)
  int xcd_blk;      // 1: a column block's split partners and its reducers share one XCD
  unsigned* counters;  // workspace head (WG_CTR_BYTES, zero at rest): the in-launch combine's words (wgemm.hip)
  unsigned long long* stamps;  // diagnostic build only (wgemm.hip ABL 3): [grid][2 waves][8] timestamps
  long long spin;   // in-launch combine: how long a partner waits for the others (s_memrealtime ticks; 0: never)
};

namespace wg {

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;

constexpr int WG_NT = 8;    // output columns per workgroup: 8 tiles of 16
constexpr int WG_BK = 64;   // k per bf16 ring stage (2 slices of 32)

template <int BM>
struct WgGeo {
  static constexpr int WM = BM == 256 ? 4 : 2;  // waves along M
  static constexpr int WN = 8 / WM;             // waves along N
  static constexpr int MB = BM / 16 / WM;       // 16-row blocks per wave
  static constexpr int TN = WG_NT / WN;         // 16-column tiles per wave
  static constexpr int W_BYTES = WG_NT * 2 * 1024;  // one W stage: 8 tiles x 2 blocks of 1 KiB
  static constexpr int X_BYTES = BM * 128;          // one X stage: BM rows x 128 B
  static constexpr int RB = BM / 16;            // row blocks per tile (split-K slab units)
};

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// wave-uniform runtime count (the pipeline tail issues fewer stages): one uniform branch per value
template <int N = 0>
__device__ __forceinline__ void wait_vmcnt_rt(int n) {
  if constexpr (N >= 30) {
    wait_vmcnt<N>();
  } else {
    if (n <= N) wait_vmcnt<N>();
    else wait_vmcnt_rt<N + 1>(n);
  }
}

// every wave's LDS-DMA of the stage being consumed has landed (its own counted wait before this), and every
// wave has finished reading the slot about to be refilled
__device__ __forceinline__ void ring_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

__device__ __forceinline__ void glds16(const void* src, char* lds_wave_base, int aux_nt) {
  if (aux_nt)
    __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)lds_wave_base, 16, 0, 2);
  else
    __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)lds_wave_base, 16, 0, 0);
}

// The two LDS rings of one workgroup and one wave's share of filling them.  LDS: [DW + 1 W slots of W_STAGE_BYTES]
// [DX + 1 X slots of BM x 128 B].  Per stage a tile's W advances by W_PIECES / 8 blocks of 1 KiB (the packings keep
// them contiguous) and X by one 128-B line per row; bf16 (64 k x 2 B) and fp8 (128 k x 1 B) differ only in how the
// caller derives `blocks_per_tile` and the row pitch.
//   W piece q = lw * WPW + j of a stage: block q % PPT of tile q / PPT, at (tile * blocks_per_tile + first_block +
//   block) * 1024 + lane * 16 -> LDS block q (fragment-major: every fragment read is a lane-linear ds_read_b128).
//   X piece i = lw + NLOAD * j: rows 8i .. 8i + 7, lane -> row r = 8i + (lane >> 3), LDS slot lane & 7 holding the
//   line's 16-B piece (lane & 7) ^ ((r >> 1) & 7) (the read side's XOR swizzle).
//   SCALE_PIECE (MXFP4): the stage's 8 x 64 scale bytes follow its W blocks, as two dword pieces issued by loaders
//   0 and 1 (lane: tile 4 lw + lane / 16, dword lane % 16).
// NDMA: dedicated loader waves 8 .. 8 + NDMA - 1 (0: the 8 MFMA waves issue their own shares).  DMA = false: the
// ablation that issues and waits for nothing.
// Issue order: step u (u < 0: prologue) issues W(u + DW), then X(u + DX); so W(t) is always older than X(t) and
// waiting for X(t) covers both (vmcnt retires in issue order).
template <int BM, int DX, int DW, int NDMA, int W_PIECES, int W_STAGE_BYTES, int SCALE_PIECE = 0, bool DMA = true>
struct RingLoader {
  static constexpr int NX = DX + 1, NW = DW + 1;
  static constexpr int NLOAD = NDMA ? NDMA : 8;   // waves issuing LDS-DMA
  static constexpr int PPT = W_PIECES / WG_NT;    // W blocks per tile per stage
  static constexpr int WPW = W_PIECES / NLOAD;    // W blocks per loader per stage
  static constexpr int XPW = (BM / 8) / NLOAD;    // X row octets per loader per stage
  static constexpr int X_BYTES = BM * 128;
  static constexpr int LDS_BYTES = NW * W_STAGE_BYTES + NX * X_BYTES;
  static_assert(DW >= DX && DX >= 1, "W is issued no later than X of the same stage");
  static_assert(PPT * WG_NT == W_PIECES && WPW * NLOAD == W_PIECES && XPW * NLOAD == BM / 8, "loader split");
  static_assert(SCALE_PIECE == 0 || (SCALE_PIECE == 4 && NLOAD >= 2), "scale pieces: dwords, loaders 0 and 1");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");

  char* const smem;
  const bool loader;
  const int lw, nst;  // loader index; stages of this split
  const int spw;      // scale pieces of this wave per stage
  const char* wsrc[WPW];
  const char* xsrc[XPW];
  const char* ssrc = nullptr;

  __device__ __forceinline__ RingLoader(char* smem_, int wave, int lane, const void* W, int blocks_per_tile,
                                        int first_block, const void* X, size_t pitch_bytes, int M, int ntiles,
                                        int tile0, int nst_, const void* scales = nullptr)
      : smem(smem_), loader(NDMA ? wave >= 8 : true), lw(NDMA ? wave - 8 : wave), nst(nst_),
        spw(SCALE_PIECE && loader && lw < 2 ? 1 : 0) {
#pragma unroll
    for (int j = 0; j < WPW; ++j) {
      const int q = lw * WPW + j, tn = q / PPT, sl = q % PPT;
      wsrc[j] = reinterpret_cast<const char*>(W) +
                ((size_t)min(tile0 + tn, ntiles - 1) * blocks_per_tile + (size_t)first_block + sl) * 1024 + lane * 16;
    }
    if constexpr (SCALE_PIECE != 0) {
      const int tn = 4 * max(min(lw, 1), 0) + (lane >> 4);
      ssrc = reinterpret_cast<const char*>(scales) +
             ((size_t)min(tile0 + tn, ntiles - 1) * blocks_per_tile + (size_t)first_block) * 64 + (lane & 15) * 4;
    }
#pragma unroll
    for (int j = 0; j < XPW; ++j) {
      const int r = 8 * (lw + NLOAD * j) + (lane >> 3);
      const int p = (lane & 7) ^ ((r >> 1) & 7);
      xsrc[j] = reinterpret_cast<const char*>(X) + (size_t)min(r, M - 1) * pitch_bytes + p * 16;
    }
  }

  __device__ __forceinline__ char* w_slot(int t) const { return smem + (t % NW) * W_STAGE_BYTES; }
  __device__ __forceinline__ char* x_slot(int t) const { return smem + NW * W_STAGE_BYTES + (t % NX) * X_BYTES; }

  __device__ __forceinline__ void issue_w(int t) const {  // W stage t (relative to the split's first) into its slot
    if constexpr (!DMA) return;
    char* base = w_slot(t);
#pragma unroll
    for (int j = 0; j < WPW; ++j) glds16(wsrc[j] + (size_t)t * (PPT * 1024), base + (lw * WPW + j) * 1024, 1);
    if constexpr (SCALE_PIECE != 0) {
      if (spw)
        __builtin_amdgcn_global_load_lds((gbl_void_t*)(ssrc + (size_t)t * 64),
                                         (lds_void_t*)(base + W_PIECES * 1024 + lw * 256), 4, 0, 0);
    }
  }
  __device__ __forceinline__ void issue_x(int t) const {
    if constexpr (!DMA) return;
    char* base = x_slot(t);
#pragma unroll
    for (int j = 0; j < XPW; ++j) glds16(xsrc[j] + (size_t)t * 128, base + (lw + NLOAD * j) * 1024, 0);
  }
  // this wave's loads younger than X(t): those of steps t - DX + 1 .. t - 1
  __device__ __forceinline__ int younger_than(int t) const {
    int n = 0;
#pragma unroll
    for (int u = t - DX + 1; u < t; ++u) n += (WPW + spw) * (u + DW < nst) + XPW * (u + DX < nst);
    return n;
  }
  __device__ __forceinline__ void land(int t) const {  // this loader's pieces of stage t have landed
    if constexpr (DMA) {
      if (loader) wait_vmcnt_rt(younger_than(t));
    }
  }
  __device__ __forceinline__ void issue_step(int t) const {
    if (loader) {
      if (t + DW < nst) issue_w(t + DW);
      if (t + DX < nst) issue_x(t + DX);
    }
  }
  __device__ __forceinline__ void prologue() const {  // steps -DW .. -1
    if (loader) {
#pragma unroll
      for (int u = -DW; u < 0; ++u) {
        if (u + DW < nst) issue_w(u + DW);
        if (u + DX >= 0 && u + DX < nst) issue_x(u + DX);
      }
    }
  }
  // A dedicated loader wave's whole run: the prologue, then one barrier per stage, as every compute wave passes; the
  // barrier of stage t retires stage t - 1's slots (every wave's reads of them completed: lgkmcnt(0) in
  // ring_barrier), which take the loads of step t.  after_barrier(t): the caller's hook (timestamps).
  // The closing s_waitcnt costs nothing (land(nst - 1) waited for every load) and is for the compiler, which cannot
  // see the counted waits (inline assembly): the flow graph leads from here past the compute loop, where an LDS-DMA
  // it thinks in flight turns each counted lgkmcnt of the fragment reads into lgkmcnt(0).
  template <class Hook>
  __device__ __forceinline__ void loader_loop(Hook after_barrier) const {
    prologue();
    for (int t = 0; t < nst; ++t) {
      land(t);
      ring_barrier();
      after_barrier(t);
      issue_step(t);
    }
    __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0) lgkmcnt(0)
  }
  __device__ __forceinline__ void loader_loop() const {
    loader_loop([](int) {});
  }
};

// Workgroup -> (column block, k-split) of the wide GEMMs.  xcd_blk (nblk % 8 == 0): XCD x = bid % 8 (round-robin
// dispatch) owns column blocks x, x + 8, ... with all their splits, so the split-K reduce can read the slabs from
// that XCD's L2 (wg_reduce_block); otherwise split-major: the column blocks of one split (which read the same X
// panel) share an XCD.  Speed only, any placement is correct.
__device__ __forceinline__ void wg_block_of(int bid, int ks, int nblk, int xcd_blk, int& blk, int& kc) {
  if (ks == 1) blk = bid, kc = 0;
  else if (xcd_blk) {
    const int j = bid >> 3;
    blk = (bid & 7) + 8 * (j / ks), kc = j % ks;
  } else if ((8 % ks) == 0) kc = bid % ks, blk = bid / ks;
  else kc = bid / nblk, blk = bid - kc * nblk;
}
// Reduce workgroup index (units of per_blk consecutive workgroups per column block) on the XCD of its block.
__device__ __forceinline__ int wg_reduce_block(int bid, int per_blk, int xcd_blk) {
  if (!xcd_blk) return bid;
  const int j = bid >> 3;
  return ((bid & 7) + 8 * (j / per_blk)) * per_blk + j % per_blk;
}

// ---- split-K slabs: unit (gt, rb) = 16 x 16 outputs of tile gt, row block rb, one f32x4 / f16x4 per lane
__device__ __forceinline__ size_t wg_slab_at(int kc, int n_units, int unit, int lane) {
  return ((size_t)kc * n_units + unit) * 64 + lane;
}

// One lane's piece of an fp16 slab: scale(v) clamped to fp16's range (the clamp only bites on non-finite partials).
// COH: write-through, for partners that combine inside this launch.
template <bool COH = false, class Scale>
__device__ __forceinline__ void wg_store_slab16(float* part, size_t e, const f32x4& v, Scale scale) {
  const f32x4 sv = scale(v);
  f16x4 h;
#pragma unroll
  for (int i = 0; i < 4; ++i) h[i] = (_Float16)fminf(fmaxf(sv[i], -65504.f), 65504.f);
  if constexpr (COH)
    __hip_atomic_store(reinterpret_cast<uint64_t*>(part) + e, __builtin_bit_cast(uint64_t, h), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  else
    reinterpret_cast<f16x4*>(part)[e] = h;
}

// ---- host side

// Split rule: ~`target` streaming workgroups (one per CU: the ring takes 115-160 KiB of LDS), at most `ksmax`
// splits; column-block counts >= 128 (gate/up, LM head) run unsplit.
inline int wg_split_want(int nblk, int target, int ksmax) {
  return nblk >= 128 ? 1 : std::max(1, std::min(ksmax, (target + nblk / 2) / nblk));
}
// `want` splits evened out: at least 4 stages per split, kst stages in each but the last.
struct WgSplit {
  int ks, kst;
};
inline WgSplit wg_split_even(int stages, int want) {
  const int ks = std::min(want, std::max(1, stages / 4));
  const int kst = (stages + ks - 1) / ks;
  return WgSplit{(stages + kst - 1) / kst, kst};
}
inline WgSplit wg_split(int nblk, int stages, int target, int ksmax) {
  return wg_split_even(stages, wg_split_want(nblk, target, ksmax));
}

// f(std::integral_constant<int, EPI>) for the runtime epilogue id
template <class F>
inline hipError_t wg_with_epi(int epi, F f) {
  switch (epi) {
#define CAIN_WG_EPI(E) \
  case E: return f(std::integral_constant<int, E>{});
    CAIN_WG_EPI(EPI_BF16) CAIN_WG_EPI(EPI_RESID) CAIN_WG_EPI(EPI_F32) CAIN_WG_EPI(EPI_SILU) CAIN_WG_EPI(EPI_GELU)
    CAIN_WG_EPI(EPI_QKV_ROPE)
#undef CAIN_WG_EPI
    default: return hipErrorInvalidValue;
  }
}

// Launch KERNEL with LDS bytes of dynamic shared memory (raising the kernel's limit on first use)
template <auto KERNEL, int LDS, class... Args>
inline hipError_t wg_launch_lds(int grid, int threads, hipStream_t st, const Args&... args) {
  static const bool attr = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, LDS) == hipSuccess;
  if (!attr) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(threads), LDS, st, args...);
  return hipGetLastError();
}

// f(std::integral_constant<int, K>) for the K of the list that equals ks, else for 0: the combine kernels'
// compile-time split counts (0: the runtime count).  With the list <2, 3> this is
//   ks == 2 ? f(<2>) : ks == 3 ? f(<3>) : f(<0>)      (`||` stops at the first K that matches)
template <int... K, class F>
inline void wg_with_ks(int ks, std::integer_sequence<int, K...>, F f) {
  static_assert(std::is_void_v<decltype(f(std::integral_constant<int, 0>{}))>, "f returns nothing (the comma below)");
  if (!((ks == K && (f(std::integral_constant<int, K>{}), true)) || ...)) f(std::integral_constant<int, 0>{});
}

}  // namespace wg
