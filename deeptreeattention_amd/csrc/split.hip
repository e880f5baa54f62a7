// Train/test plot split search (reference src/data.py:108-236: sample_plots run config["iterations"] times, one dask future
// each, train_test_split keeps the best).  deeptreeattention_amd/split.py holds the definition (order_np / search_np);
// these kernels equal it bit for bit: the order is the counter hash's shuffle (hash_dev.h, stream HASH_STREAM_SPLIT), the scan
// integer sums and one float64 comparison per species, the choice of the best an integer comparison.
//   k_split_search  ONE WAVEFRONT PER ITERATION, every iteration in one launch.  The wavefront hashes the C candidates into
//                   64-bit keys (draw_key), sorts them in LDS (bitonic, padded with HASH_PAD to a power of two), then walks the
//                   order: lanes over species, 4 per lane (one 16-byte load of a plot's A row, the next plot's row already
//                   in flight), __ballot for "any species of this plot still wanted", so the walk needs no barrier, and it
//                   stops as soon as no species is wanted.  The included plots are listed in LDS as they are met; their B and
//                   R rows are summed afterwards in a loop whose loads do not depend on one another.
//   k_split_best    one workgroup: the lexicographic maximum of (species, train_rows), the earliest iteration on a full tie
// No atomics at all, float or integer: every output element has one writer, so a rerun gives the same bits.  The tables
// (C x 3 x S int32, 12 MB at the limits, 154 KB at 64 plots x 200 species) are left to L2 and the memory-side cache.
#include <math.h>
#include "../../include/dta_hip.h"
#include "common.h"
#include "hash_dev.h"

namespace dta {

constexpr int SPL_WAVE = 64;
constexpr int SPL_BEST_THREADS = 256;
constexpr unsigned SPL_INC = 0x80000000u;   // in the low word of a key once its plot is a test plot (j < 4096 leaves the bit free)

typedef __attribute__((ext_vector_type(4))) int i32x4;

struct SplitArgs {
  const i32x4* rows;      // [C][3][SP / 4]: A, B, R of each candidate plot
  const i32x4* totals;    // [2][SP / 4]: totA, totR
  const int* orders;      // [iterations][C] or null
  int C, S, quads, n;     // quads = SP / 4; n = C rounded up to a power of two, at least 64: the LDS keys
  int min_train, min_test;
  unsigned long long key, first;
  int* species; long long* train_rows; int* test_plots; unsigned char* membership; unsigned char* taxa;
  double floor[DTA_SPLIT_MAX_SPECIES];
};

__global__ __launch_bounds__(SPL_WAVE) void k_split_search(SplitArgs a) {
  extern __shared__ unsigned long long keys[];        // [n]
  unsigned* w = reinterpret_cast<unsigned*>(keys);    // w[2k]: candidate of position k (| SPL_INC); w[2m + 1]: the m-th test plot
  const int lane = threadIdx.x, C = a.C, n = a.n;
  const unsigned long long it = blockIdx.x;
  if (a.orders) {
    const int* o = a.orders + (size_t)it * C;
    for (int k = lane; k < C; k += SPL_WAVE) {
      const int j = o[k];
      keys[k] = (unsigned)(j < 0 ? 0 : j >= C ? C - 1 : j);   // (an entry that is no candidate cannot leave the table)
    }
    __syncthreads();
  } else {
    const unsigned long long base = (a.first + it) * (unsigned long long)C;
    for (int k = lane; k < n; k += SPL_WAVE)
      keys[k] = k < C ? draw_key(base, a.key, k) : HASH_PAD;
    __syncthreads();
    // bitonic sort, ascending; the padding keys are above every real key and end behind position C - 1
    for (int size = 2; size <= n; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int t = lane; t < (n >> 1); t += SPL_WAVE) {
          const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
          const unsigned long long x = keys[i], y = keys[i + stride];
          if ((x > y) == ((i & size) == 0)) { keys[i] = y; keys[i + stride] = x; }
        }
        __syncthreads();
      }
    }
  }

  // the walk: lanes over species
  const int quads = a.quads, s0 = lane * 4;
  const bool on = lane < quads;
  const i32x4 zero = {0, 0, 0, 0};
  double fl[4];
  unsigned valid = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bool v = s0 + q < a.S;
    valid |= v ? 1u << q : 0u;
    fl[q] = v ? a.floor[s0 + q] : 0.0;
  }
  i32x4 cnt = zero;
  unsigned wanted = valid;      // to_sample
  int m = 0;
  const size_t plot = (size_t)3 * quads;
  i32x4 next = on ? a.rows[w[0] * plot + lane] : zero;
  for (int k = 0; k < C; ++k) {
    const unsigned j = w[2 * k];
    const i32x4 cur = next;
    if (k + 1 < C && on) next = a.rows[w[2 * k + 2] * plot + lane];
    const bool hit = (cur[0] > 0 && (wanted & 1u)) || (cur[1] > 0 && (wanted & 2u)) || (cur[2] > 0 && (wanted & 4u)) ||
                     (cur[3] > 0 && (wanted & 8u));
    if (__ballot(hit) == 0ull) continue;
    cnt += cur;
    wanted = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if ((valid >> q & 1u) && !((double)cnt[q] > fl[q])) wanted |= 1u << q;      // strict, as the reference
    if (lane == 0) { w[2 * k] = j | SPL_INC; w[2 * m + 1] = j; }
    ++m;
    if (__ballot(wanted != 0u) == 0ull) break;
  }
  __syncthreads();

  // B and R over the test plots (A over them is cnt)
  i32x4 tb = zero, tr = zero;
  if (on) {
#pragma unroll 4
    for (int i = 0; i < m; ++i) {
      const i32x4* row = a.rows + w[2 * i + 1] * plot + lane;
      tb += row[quads];
      tr += row[2 * quads];
    }
  }
  const i32x4 tot_a = on ? a.totals[lane] : zero, tot_r = on ? a.totals[quads + lane] : zero;
  unsigned kept = 0;     // T
  long long rows = 0;
  int n_species = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bool t = (valid >> q & 1u) && tb[q] >= a.min_test && tot_a[q] - cnt[q] >= a.min_train;
    kept |= t ? 1u << q : 0u;
    rows += t ? (long long)(tot_r[q] - tr[q]) : 0ll;
    n_species += __popcll(__ballot(t));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) rows += __shfl_xor(rows, o);
  if (lane == 0) { a.species[it] = n_species; a.train_rows[it] = rows; a.test_plots[it] = m; }
  if (a.membership) {
    unsigned char* dst = a.membership + (size_t)it * C;
    for (int k = lane; k < C; k += SPL_WAVE) { const unsigned v = w[2 * k]; dst[v & ~SPL_INC] = (unsigned char)(v >> 31); }
  }
  if (a.taxa) {
    unsigned char* dst = a.taxa + (size_t)it * a.S + s0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (valid >> q & 1u) dst[q] = (unsigned char)(kept >> q & 1u);
  }
}

// (species, train_rows) larger first, then the earlier iteration
__device__ __forceinline__ bool spl_better(int sa, long long ra, int ia, int sb, long long rb, int ib) {
  return sa != sb ? sa > sb : ra != rb ? ra > rb : ia < ib;
}

__global__ __launch_bounds__(SPL_BEST_THREADS) void k_split_best(const int* species, const long long* train_rows,
                                                                 const int* test_plots, int iterations, long long* best) {
  __shared__ int s_sp[SPL_BEST_THREADS], s_it[SPL_BEST_THREADS];
  __shared__ long long s_rows[SPL_BEST_THREADS];
  const int tid = threadIdx.x;
  int sp = -1, at = 0x7FFFFFFF;
  long long rows = -1;
  for (long long i = tid; i < iterations; i += SPL_BEST_THREADS) {
    const int s = species[i];
    const long long r = train_rows[i];
    if (spl_better(s, r, (int)i, sp, rows, at)) { sp = s; rows = r; at = (int)i; }
  }
  s_sp[tid] = sp; s_rows[tid] = rows; s_it[tid] = at;
  __syncthreads();
  for (int half = SPL_BEST_THREADS / 2; half > 0; half >>= 1) {
    if (tid < half && spl_better(s_sp[tid + half], s_rows[tid + half], s_it[tid + half], s_sp[tid], s_rows[tid], s_it[tid])) {
      s_sp[tid] = s_sp[tid + half]; s_rows[tid] = s_rows[tid + half]; s_it[tid] = s_it[tid + half];
    }
    __syncthreads();
  }
  if (tid == 0) { best[0] = s_it[0]; best[1] = s_sp[0]; best[2] = s_rows[0]; best[3] = test_plots[s_it[0]]; }
}

}  // namespace dta

using namespace dta;

extern "C" {

int dta_split_search(const int* rows, const int* totals, int candidates, int species, const double* floor, int min_train,
                     int min_test, int iterations, unsigned long long seed, unsigned long long first_iteration,
                     const int* orders, int* out_species, long long* out_train_rows, int* out_test_plots, long long* best,
                     unsigned char* membership, unsigned char* taxa, void* stream) {
  const char* who = "dta_split_search";
  if (!rows || !totals || !floor || !out_species || !out_train_rows || !out_test_plots || !best) {
    dta_set_error("%s: null argument", who);
    return 1;
  }
  if (species < 1 || species > DTA_SPLIT_MAX_SPECIES) {
    dta_set_error("%s: species=%d: 1..%d (DTA_SPLIT_MAX_SPECIES)", who, species, DTA_SPLIT_MAX_SPECIES);
    return 1;
  }
  if (candidates < 1 || candidates > DTA_SPLIT_MAX_CANDIDATES) {
    dta_set_error("%s: candidates=%d: 1..%d (DTA_SPLIT_MAX_CANDIDATES)", who, candidates, DTA_SPLIT_MAX_CANDIDATES);
    return 1;
  }
  if (iterations < 0) { dta_set_error("%s: iterations=%d is negative", who, iterations); return 1; }
  if (min_train < 1 || min_test < 1) { dta_set_error("%s: min_train=%d, min_test=%d: both at least 1", who, min_train, min_test); return 1; }
  if (((uintptr_t)rows | (uintptr_t)totals) & 15) { dta_set_error("%s: rows and totals must be 16-byte aligned", who); return 1; }
  SplitArgs a;
  for (int s = 0; s < species; ++s) {
    if (!std::isfinite(floor[s])) { dta_set_error("%s: floor is not finite (species %d)", who, s); return 1; }
    a.floor[s] = floor[s];
  }
  if (iterations == 0) return 0;                  // empty outputs: nothing to write, nothing launched
  a.rows = (const i32x4*)rows; a.totals = (const i32x4*)totals; a.orders = orders;
  a.C = candidates; a.S = species; a.quads = (species + 3) / 4;
  a.n = SPL_WAVE;
  while (a.n < candidates) a.n <<= 1;
  a.min_train = min_train; a.min_test = min_test;
  a.key = stream_key(seed, HASH_STREAM_SPLIT);
  a.first = first_iteration;
  a.species = out_species; a.train_rows = out_train_rows; a.test_plots = out_test_plots; a.membership = membership; a.taxa = taxa;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_split_search, dim3((unsigned)iterations), dim3(SPL_WAVE), sizeof(unsigned long long) * (size_t)a.n, st, a);
  DTA_CHECK_LAUNCH("k_split_search");
  hipLaunchKernelGGL(k_split_best, dim3(1), dim3(SPL_BEST_THREADS), 0, st, (const int*)out_species,
                     (const long long*)out_train_rows, (const int*)out_test_plots, iterations, best);
  DTA_CHECK_LAUNCH("k_split_best");
  return 0;
}

}  // extern "C"
