// Prefix KV reuse: copy cache positions [0, n) of one slot to the same positions of another, for every layer, both
// caches and every kv head, in one launch (engine.py ContinuousBatch.admit: a request whose prompt shares a prefix
// with a slot that is still decoding starts its prefill behind a copy of that prefix).
//
// Layout (common.h kfrag_off / vfrag_off): inside the [T_max * hd] block of one (layer, slot, kv head), K is blocked
// by 16 positions (16 * hd contiguous elements per block) and V^T by 32 (32 * hd elements per block, the positions
// of a block in the permuted order of P).  So a prefix of whole blocks is one contiguous byte range from the block's
// base -- moved as lane-linear 16-byte vectors, every wave instruction covering whole 128-byte lines -- and only the
// partial last block (n & 15 positions of K, n & 31 of V^T) goes element by element through the offset functions;
// destination positions >= n keep their bits.  Memory-bound streaming: no LDS, no atomics, plain vector loads and
// stores; the grid is sized from cain_cu_budget().
#include "common.h"
#include <algorithm>

#define KVP_MAX_PAIRS 256
#define KVP_THREADS 256
#define KVP_VEC 4                                 // 16-byte vectors in flight per lane
#define KVP_CHUNK (KVP_THREADS * KVP_VEC * 16)    // bytes of one bulk work item

struct KvPrefixArgs {
  uint16_t src[KVP_MAX_PAIRS], dst[KVP_MAX_PAIRS];  // (S <= 65536)
  int n[KVP_MAX_PAIRS];
  int first[KVP_MAX_PAIRS + 1];  // work items before pair i; [pairs]: all of them
};
static_assert(sizeof(KvPrefixArgs) + 64 <= 4096, "the pair table travels as a kernel argument");

// One work item: (pair, layer, cache, kv head, chunk).  chunk < chunks: KVP_CHUNK bytes of the whole-block range;
// chunk == chunks (pairs with n & 31 only): the partial last block.
template <typename E>
__global__ __launch_bounds__(KVP_THREADS) void kv_copy_prefix_kernel(E* kc, E* vtc, long long kv_layer_elems, int L,
                                                                    int Hkv, int hd, int T_max, int pairs,
                                                                    KvPrefixArgs a) {
  const int total = a.first[pairs];
  const size_t head_elems = (size_t)T_max * hd;
  for (int item = blockIdx.x; item < total; item += gridDim.x) {
    int lo = 0, hi = pairs - 1;  // the pair whose items hold this one: first[lo] <= item < first[lo + 1]
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (a.first[mid] <= item) lo = mid; else hi = mid - 1;
    }
    const int n = a.n[lo];
    const size_t kbulk = (size_t)(n >> 4) * 16 * hd * sizeof(E);  // bytes of K's whole blocks (>= V^T's)
    const int chunks = int((kbulk + KVP_CHUNK - 1) / KVP_CHUNK);
    const int per_unit = chunks + ((n & 31) ? 1 : 0);
    int rest = item - a.first[lo];
    const int chunk = rest % per_unit;
    rest /= per_unit;
    const int h = rest % Hkv;
    rest /= Hkv;
    const int is_v = rest & 1;
    const int layer = rest >> 1;
    if (layer >= L) continue;  // (never: first[] counts L * 2 * Hkv * per_unit items per pair)
    E* cache = is_v ? vtc : kc;
    const size_t lbase = (size_t)layer * (size_t)kv_layer_elems;
    const E* s = cache + lbase + ((size_t)a.src[lo] * Hkv + h) * head_elems;
    E* d = cache + lbase + ((size_t)a.dst[lo] * Hkv + h) * head_elems;
    if (chunk < chunks) {
      const size_t bulk = is_v ? (size_t)(n >> 5) * 32 * hd * sizeof(E) : kbulk;
      const size_t nvec = bulk >> 4;
      const uint4* sv = reinterpret_cast<const uint4*>(s);
      uint4* dv = reinterpret_cast<uint4*>(d);
      const size_t v0 = (size_t)chunk * (KVP_THREADS * KVP_VEC) + threadIdx.x;
      uint4 r[KVP_VEC];
#pragma unroll
      for (int i = 0; i < KVP_VEC; ++i) {
        const size_t v = v0 + (size_t)i * KVP_THREADS;
        if (v < nvec) r[i] = sv[v];
      }
#pragma unroll
      for (int i = 0; i < KVP_VEC; ++i) {
        const size_t v = v0 + (size_t)i * KVP_THREADS;
        if (v < nvec) dv[v] = r[i];
      }
    } else if (is_v) {
      // V^T: the n & 31 positions of 32-block n >> 5; a 16-byte vector interleaves positions t and t + 16
      const int t0 = n & ~31, r = n & 31;
      for (int e = threadIdx.x; e < r * hd; e += KVP_THREADS) {
        const size_t o = vfrag_off(t0 + e % r, e / r, hd);
        d[o] = s[o];
      }
    } else {
      // K: the n & 15 positions of 16-block n >> 4 (a whole first half of the 32-block went with the bulk)
      const int t0 = n & ~15, r = n & 15;
      for (int e = threadIdx.x; e < r * hd; e += KVP_THREADS) {
        const size_t o = kfrag_off(t0 + (e >> 3) % r, ((e >> 3) / r) * 8 + (e & 7), hd);
        d[o] = s[o];
      }
    }
  }
}

// src_slot / dst_slot / n_pos: host arrays of `pairs` entries.  -1 without a launch on arguments that name memory
// outside the caches or make the result depend on the order of the pairs; 0 without a launch when nothing is to copy.
CAIN_API int cain_kv_copy_prefix(void* kc, void* vtc, long long kv_layer_elems, int L, int S, int Hkv, int hd,
                                 int T_max, int kv8, const int* src_slot, const int* dst_slot, const int* n_pos,
                                 int pairs, hipStream_t st) {
  if (pairs < 0 || pairs > KVP_MAX_PAIRS) return -1;
  if (L < 1 || S < 1 || S > 65536 || Hkv < 1 || hd < 32 || hd % 32 || T_max < 32 || T_max % 32) return -1;
  if (kv_layer_elems < (long long)S * Hkv * T_max * hd) return -1;
  if (pairs == 0) return 0;
  if (!kc || !vtc || !src_slot || !dst_slot || !n_pos) return -1;
  for (int i = 0; i < pairs; ++i) {
    if (src_slot[i] < 0 || src_slot[i] >= S || dst_slot[i] < 0 || dst_slot[i] >= S) return -1;
    if (n_pos[i] < 0 || n_pos[i] > T_max) return -1;
    if (n_pos[i] > 0 && src_slot[i] == dst_slot[i]) return -1;
    for (int j = 0; j < pairs; ++j) {
      if (j == i) continue;
      if (dst_slot[j] == dst_slot[i]) return -1;  // written twice
      if (src_slot[j] == dst_slot[i]) return -1;  // read by one pair while another writes it
    }
  }
  KvPrefixArgs a;
  const size_t esz = kv8 ? 1 : 2;
  long long total = 0;
  int live = 0;
  for (int i = 0; i < pairs; ++i) {
    const int n = n_pos[i];
    if (n == 0) continue;  // (skipped: the kernel's pair search needs every listed pair to own items)
    a.src[live] = uint16_t(src_slot[i]), a.dst[live] = uint16_t(dst_slot[i]), a.n[live] = n, a.first[live] = int(total);
    const size_t kbulk = (size_t)(n >> 4) * 16 * hd * esz;
    const long long per_unit = (long long)((kbulk + KVP_CHUNK - 1) / KVP_CHUNK) + ((n & 31) ? 1 : 0);
    total += per_unit * L * 2 * Hkv;
    if (total > 0x3fffffff) return -1;
    ++live;
  }
  if (live == 0) return 0;
  a.first[live] = int(total);
  for (int i = live; i < KVP_MAX_PAIRS; ++i) a.src[i] = a.dst[i] = a.n[i] = 0, a.first[i + 1] = int(total);
  // streaming copy: 8 workgroups of 4 waves per CU hide the load latency; the items stride over the grid
  const int grid = int(std::min<long long>(total, (long long)cain_cu_budget() * 8));
  if (kv8)
    hipLaunchKernelGGL(kv_copy_prefix_kernel<uint8_t>, dim3(grid), dim3(KVP_THREADS), 0, st, (uint8_t*)kc,
                       (uint8_t*)vtc, kv_layer_elems, L, Hkv, hd, T_max, live, a);
  else
    hipLaunchKernelGGL(kv_copy_prefix_kernel<uint16_t>, dim3(grid), dim3(KVP_THREADS), 0, st, (uint16_t*)kc,
                       (uint16_t*)vtc, kv_layer_elems, L, Hkv, hd, T_max, live, a);
  return int(hipGetLastError());
}
