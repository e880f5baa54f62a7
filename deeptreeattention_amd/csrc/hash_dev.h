// The counter hash and the streamed count of the sampling kernels (abundance.hip, split.hip, treedata.hip, levels.hip): ONE
// body each, so that their bit equality with deeptreeattention_amd/_hash.py, the NumPy statement, rests on shared code
// ("The counter hash and the streamed count").  Unsigned 64-bit arithmetic, modulo 2^64.
// The streams in use -- a new feature takes a number that is not in this table:
//   0        HASH_STREAM_ABUNDANCE_KEEP   abundance: does the crown keep its label
//   1        HASH_STREAM_ABUNDANCE_DRAW   abundance: the species it is drawn again as
//   0        HASH_STREAM_SPLIT            split search: the order of the candidate plots (its counters are its own)
//   2        DTA_LEVEL_STREAM             levels: the record shuffle of level 2                                  (dta_hip.h)
//   3        DTA_DEAD_FLIP_STREAM         dead_train: is the image flipped (HASH_STREAM_DEAD_FLIP)               (dta_hip.h)
//   16..79   DTA_EPOCH_ORDER_STREAM + level id (below DTA_EPOCH_ORDER_MAX_LEVEL_ID): the epoch orders            (dta_hip.h)
//            level id 63 (DTA_DEAD_ORDER_LEVEL, stream 79): the alive/dead image pool's order
#pragma once
#include "common.h"

namespace dta {

constexpr unsigned long long HASH_GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr unsigned long long HASH_PAD = ~0ull;      // above every draw_key: the low word of a key is an index
constexpr unsigned HASH_STREAM_ABUNDANCE_KEEP = 0, HASH_STREAM_ABUNDANCE_DRAW = 1, HASH_STREAM_SPLIT = 0;

// splitmix64's finaliser
__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the key of one stream of one seed: formed on the host, travels in the argument struct
static inline unsigned long long stream_key(unsigned long long seed, unsigned long long stream) {
  return mix64(seed * HASH_GOLDEN + stream + 1ull);
}
// entry i's draw in a shuffle of n whose first counter is base = (epoch or iteration) * n, and its sort key: distinct for
// distinct i, so a sort by it, or a count of the smaller keys, is exact and stable
__device__ __forceinline__ unsigned long long draw32(unsigned long long base, unsigned long long key, int i) {
  return mix64((base + (unsigned long long)i) * HASH_GOLDEN + key) >> 32;
}
__device__ __forceinline__ unsigned long long draw_key(unsigned long long base, unsigned long long key, int i) {
  return (draw32(base, key, i) << 32) | (unsigned)i;
}

// The streamed count: a lane's place among n entries is the number of entries before its own.  The entries stream through
// the caller's LDS tile(s) in tiles of TILE slots: stage(k, j) fills slot k from entry j (THREADS lanes fill a tile together),
// below(k) says whether slot k counts against this lane, and every lane looks at every slot.  Two rules:
//   * The barriers are in here, so EVERY lane of the workgroup calls this, with the same n.  A whole workgroup may return
//     before the call; a single lane may not -- one without an entry calls with a `below` that is never true, or drops the count.
//   * j runs past n in the last tile: stage() fills such a slot with HASH_PAD, so below() is false for it in every lane.
template <int TILE, int THREADS, typename Stage, typename Below>
__device__ __forceinline__ int streamed_count(int n, Stage stage, Below below) {
  int count = 0;
  for (int t0 = 0; t0 < n; t0 += TILE) {
    __syncthreads();                                         // every lane has read the previous tile
    for (int k = threadIdx.x; k < TILE; k += THREADS) stage(k, t0 + k);
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < TILE; ++k) count += below(k) ? 1 : 0;      // every lane reads the same slot: a broadcast
  }
  return count;
}

}  // namespace dta
