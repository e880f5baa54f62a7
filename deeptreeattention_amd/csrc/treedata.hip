// The resident training set (reference src/data.py:239-310 `TreeDataset`, five of them over the same individuals in
// src/models/multi_stage.py:82-219).  deeptreeattention_amd/treedata.py holds the definitions (epoch_order_np / batch_np);
// these kernels equal them bit for bit: the order is the counter hash's shuffle (hash_dev.h, streams DTA_EPOCH_ORDER_STREAM +
// level id), a batch a copy.
//   k_epoch_order   the shuffled order of every level's view in ONE launch (blockIdx.y = level).  A lane owns entry i and
//                   its draw_key; all keys of the level stream through LDS in tiles (hash_dev.h's streamed_count) and the
//                   lane counts the keys below its own: that count is the position of i in the order, exactly, because
//                   the keys are distinct.  n^2 compares, once per epoch.
//   k_pool_batches  the float32 batches of every level x year of one step in ONE launch (blockIdx.y = level * years +
//                   year), with the labels, the pool rows and the level-years' 0/1 flags.  The output of a level-year is
//                   one flat array; a lane owns pieces of four consecutive floats of it (one 16-byte store each), decomposes a
//                   piece's index once and carries it, and looks its source row up again only when the piece steps into the
//                   next crop -- the lanes of dense.hip's gathers, four pieces to a lane.  Not a Src<> policy of that body: the source here is a row of a [N][Y][C][S][S]
//                   pool, float32 or bf16, found through two tables (order, then the view's rows) that differ per level,
//                   where that body reads one float32 raster per launch row.
// Pure copies and integer work: no atomics, one writer per output element, reruns are bit-identical.
#include "../../include/dta_hip.h"
#include "common.h"
#include "hash_dev.h"

namespace dta {

namespace {

constexpr int EO_THREADS = 256;
constexpr int EO_TILE = 1024;      // keys per LDS tile: 8 KB

struct EpochOrderArgs {
  int n[DTA_MAX_LEVELS];
  unsigned long long key[DTA_MAX_LEVELS];     // stream_key(seed, DTA_EPOCH_ORDER_STREAM + level id)
  unsigned long long base[DTA_MAX_LEVELS];    // epoch * n mod 2^64
  int* order[DTA_MAX_LEVELS];
};

__global__ __launch_bounds__(EO_THREADS) void k_epoch_order(EpochOrderArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned long long tile[EO_TILE];
  const int l = blockIdx.y, n = a.n[l];
  if ((long long)blockIdx.x * EO_THREADS >= n) return;         // (the whole workgroup: the grid is as wide as the longest level)
  const unsigned long long key = a.key[l], base = a.base[l];
  const int i = blockIdx.x * EO_THREADS + threadIdx.x;
  const unsigned long long mine = i < n ? draw_key(base, key, i) : 0ull;      // (0: no key is below it)
  const int rank = streamed_count<EO_TILE, EO_THREADS>(
      n, [&](int k, int j) { tile[k] = j < n ? draw_key(base, key, j) : HASH_PAD; },      // hashed again, never read from memory
      [&](int k) { return tile[k] < mine; });
  if (i < n && rank < n) a.order[l][rank] = i;
}

struct PoolLevel {
  const int* order;            // [n] or null: the identity
  const long long* rows;       // [n] entry -> pool row
  const long long* labels;     // [n] or null
  long long n, start;
  int count, flip;
  long long* out_labels;       // [count] or null
  long long* out_rows;         // [count]
  const unsigned char* keep;   // [n][Y] or null: 0 masks the (entry, year) as a missing year (dta_pool_batches_keep)
};

struct PoolArgs {
  const void* pool;            // [N][Y][C][S][S]
  long long N;
  int Y, C, S;
  PoolLevel lv[DTA_MAX_LEVELS];
  float* out[DTA_MAX_YEARS];   // level-major
  float* flags;
  float* clear_next;
};

// The view entry that position p of the level's step brings, or -1.  Every table read is guarded, whatever the tables say.
__device__ __forceinline__ long long pool_entry(const PoolLevel& v, int p) {
  const long long pos = v.start + p;
  if (pos < 0 || pos >= v.n) return -1;
  const long long e = v.order ? (long long)v.order[pos] : pos;
  return e < 0 || e >= v.n ? -1 : e;
}

// A lane's piece of four elements as it was loaded: the bits travel untouched until the store.  set() after zero() only.
template <typename T> struct PoolRaw;
template <> struct PoolRaw<float> {
  f32x4 v;
  __device__ __forceinline__ void zero() { v = f32x4{0.f, 0.f, 0.f, 0.f}; }
  // four consecutive elements at an address that is only element-aligned
  __device__ __forceinline__ void load4(const float* p) { __builtin_memcpy(&v, p, sizeof(v)); }
  __device__ __forceinline__ void set(int k, const float* p) { v[k] = *p; }
  __device__ __forceinline__ float get(int k) const { return v[k]; }
};
template <> struct PoolRaw<bf16_t> {
  u32x2 v;
  __device__ __forceinline__ void zero() { v = u32x2{0u, 0u}; }
  __device__ __forceinline__ void load4(const bf16_t* p) { __builtin_memcpy(&v, p, sizeof(v)); }
  __device__ __forceinline__ void set(int k, const bf16_t* p) { v[k >> 1] |= (unsigned)*p << (16 * (k & 1)); }
  __device__ __forceinline__ float get(int k) const {                                   // widened exactly
    return __uint_as_float((k & 1) ? v[k >> 1] & 0xFFFF0000u : v[k >> 1] << 16);
  }
};

// The crop of position p and this year, or null: nothing to read, the output is zero (a row outside the pool).
template <typename T, bool KEEP>
__device__ __forceinline__ const T* pool_crop(const PoolArgs& a, const PoolLevel& v, int p, int y, size_t per) {
  const long long e = pool_entry(v, p);
  if (e < 0) return nullptr;
  if (KEEP && v.keep && !v.keep[(size_t)e * a.Y + y]) return nullptr;
  const long long row = v.rows[e];
  if (row < 0 || row >= a.N) return nullptr;
  return reinterpret_cast<const T*>(a.pool) + ((size_t)row * a.Y + y) * per;
}

// flags[level * Y + y] = 1 when that batch has a non-zero element on its way out (NaN counts, -0.0 does not), else it
// stays 0: k_gather_years' rule and protocol (dense.hip) -- a wave that wrote a non-zero element stores 1.f once, plain
// stores of one value; flags arrive zeroed, clear_next is the bank the NEXT call sets.
// A lane moves PB_ITER pieces of four floats, 1024 floats apart.  What a piece needs first is its source row -- two
// dependent table reads (order, then rows) before the crop itself can be read -- and one piece per lane left the kernel
// waiting on that chain at full occupancy.  So the lookups of a lane's pieces are written without branches (a position
// or an entry that does not exist reads entry 0 and is dropped afterwards) and issued together, then the loads, then the
// stores.
constexpr int PB_ITER = 4;
constexpr int PB_BLOCK = 256 * 4 * PB_ITER;      // floats per workgroup

// KEEP: the levels may carry a year mask (dta_pool_batches_keep); without it the body is what it was.
template <typename T, bool KEEP>
__device__ __forceinline__ void pool_batches_body(const PoolArgs& a) {
  const int net = blockIdx.y, l = net / a.Y, y = net - l * a.Y;
  const PoolLevel& v = a.lv[l];
  if (a.clear_next && blockIdx.x == 0 && threadIdx.x == 0) a.clear_next[net] = 0.f;
  if (y == 0 && blockIdx.x == 0) {
    for (int p = threadIdx.x; p < v.count; p += 256) {
      const long long e = pool_entry(v, p);
      if (v.out_labels) v.out_labels[p] = e < 0 || !v.labels ? -1 : v.labels[e];
      v.out_rows[p] = e < 0 ? -1 : v.rows[e];
    }
  }
  const int S = a.S, SS = S * S, C = a.C;
  const size_t per = (size_t)C * SS;
  const size_t total = (size_t)v.count * per;
  const size_t first = (size_t)blockIdx.x * PB_BLOCK + (size_t)threadIdx.x * 4;
  if ((size_t)blockIdx.x * PB_BLOCK >= total) return;      // (the whole workgroup: the grid is as wide as the largest batch)
  const bool flip = v.flip != 0, narrow = total <= 0xFFFFFFFFull;
  const T* const pool = reinterpret_cast<const T*>(a.pool);

  // 1. where each piece starts -- decomposed once, in 32 bits where the batch allows it (a 64-bit division would be most
  //    of this kernel's arithmetic) -- and the crop it starts in
  bool live[PB_ITER], ok[PB_ITER];
  int n[PB_ITER], c[PB_ITER], q[PB_ITER];
  long long ent[PB_ITER];
  const T* src[PB_ITER];
#pragma unroll
  for (int it = 0; it < PB_ITER; ++it) {
    const size_t e = first + (size_t)it * 1024;
    live[it] = e < total;
    const size_t ee = live[it] ? e : 0;
    unsigned r;
    if (narrow) {
      n[it] = (int)((unsigned)ee / (unsigned)per);
      r = (unsigned)ee - (unsigned)n[it] * (unsigned)per;
    } else {
      n[it] = (int)(ee / per);
      r = (unsigned)(ee - (size_t)n[it] * per);
    }
    c[it] = (int)(r / (unsigned)SS);
    q[it] = (int)(r - (unsigned)c[it] * (unsigned)SS);
    const long long pos = v.start + n[it];
    ok[it] = pos >= 0 && pos < v.n;
    ent[it] = ok[it] ? pos : 0;
  }
  if (v.order) {
#pragma unroll
    for (int it = 0; it < PB_ITER; ++it) ent[it] = v.order[ent[it]];
#pragma unroll
    for (int it = 0; it < PB_ITER; ++it) {
      ok[it] = ok[it] && ent[it] >= 0 && ent[it] < v.n;
      ent[it] = ok[it] ? ent[it] : 0;
    }
  }
  long long row[PB_ITER];
#pragma unroll
  for (int it = 0; it < PB_ITER; ++it) row[it] = v.rows[ent[it]];
  if (KEEP && v.keep) {      // a masked (entry, year) is a missing year: nothing to read, the output is zero
    unsigned char kept[PB_ITER];
#pragma unroll
    for (int it = 0; it < PB_ITER; ++it) kept[it] = v.keep[(size_t)ent[it] * a.Y + y];
#pragma unroll
    for (int it = 0; it < PB_ITER; ++it) ok[it] = ok[it] && kept[it] != 0;
  }
#pragma unroll
  for (int it = 0; it < PB_ITER; ++it) {
    ok[it] = ok[it] && row[it] >= 0 && row[it] < a.N;
    src[it] = ok[it] ? pool + ((size_t)row[it] * a.Y + y) * per : nullptr;      // null: nothing to read, the output is zero
  }

  // 2. the loads.  A piece that lies in one plane of one crop is four consecutive source elements, one load (a crop's
  //    C*S*S elements need not be a multiple of four: the address is only element-aligned).  Both training flips
  //    together reverse the S*S pixels of a plane, so under flip they are the four that END at pixel SS - 1 - q, and the
  //    store takes them backwards.
  PoolRaw<T> raw[PB_ITER];
  bool whole[PB_ITER];
#pragma unroll
  for (int it = 0; it < PB_ITER; ++it) {
    raw[it].zero();
    whole[it] = live[it] && first + (size_t)it * 1024 + 4 <= total && q[it] + 4 <= SS;
    if (whole[it] && src[it]) raw[it].load4(src[it] + (size_t)c[it] * SS + (flip ? SS - 4 - q[it] : q[it]));
  }
  //    ... and a piece that straddles planes or crops, or ends the batch: element by element, the index carried, the next
  //    crop looked up when the piece steps into it
#pragma unroll
  for (int it = 0; it < PB_ITER; ++it) {
    if (live[it] && !whole[it]) {
      const size_t e = first + (size_t)it * 1024;
      int nn = n[it], cc = c[it], qq = q[it];
      const T* s = src[it];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (e + k < total) {
          if (s) raw[it].set(k, s + (size_t)cc * SS + (flip ? SS - 1 - qq : qq));
          if (++qq == SS) {
            qq = 0;
            if (++cc == C) {
              cc = 0; ++nn;
              if (nn < v.count) s = pool_crop<T, KEEP>(a, v, nn, y, per);
            }
          }
        }
      }
    }
  }

  // 3. the stores
  float* out = a.out[net];
  bool hit = false;
#pragma unroll
  for (int it = 0; it < PB_ITER; ++it) {
    if (live[it]) {
      const size_t e = first + (size_t)it * 1024;
      const bool back = whole[it] && flip;
      float w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float fwd = raw[it].get(k), rev = raw[it].get(3 - k);
        w[k] = back ? rev : fwd;
      }
      if (e + 4 <= total) *reinterpret_cast<f32x4*>(out + e) = f32x4{w[0], w[1], w[2], w[3]};
      else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (e + k < total) out[e + k] = w[k];
      }
      hit = hit || !(w[0] == 0.f && w[1] == 0.f && w[2] == 0.f && w[3] == 0.f);
    }
  }
  const bool any = __any(hit);
  if (any && (threadIdx.x & 63) == 0) a.flags[net] = 1.f;
}

template <typename T>
__global__ __launch_bounds__(256) void k_pool_batches(PoolArgs a) { pool_batches_body<T, false>(a); }

// the same launch for views with a year mask: a masked (entry, year) is gathered as a missing year
template <typename T>
__global__ __launch_bounds__(256) void k_pool_masked(PoolArgs a) { pool_batches_body<T, true>(a); }

}  // namespace

}  // namespace dta

using namespace dta;

extern "C" {

int dta_epoch_order(int levels, const long long* n, const int* level_ids, unsigned long long seed, unsigned long long epoch,
                    int* const* orders, void* stream) {
  const char* who = "dta_epoch_order";
  if (!n || !orders) { dta_set_error("%s: null argument", who); return 1; }
  if (levels < 1 || levels > DTA_MAX_LEVELS) {
    dta_set_error("%s: levels=%d: 1..%d (DTA_MAX_LEVELS)", who, levels, DTA_MAX_LEVELS);
    return 1;
  }
  EpochOrderArgs a;
  long long longest = 0;
  for (int l = 0; l < levels; ++l) {
    if (n[l] < 1 || n[l] > DTA_EPOCH_ORDER_MAX_N) {
      dta_set_error("%s: n=%lld (level %d): 1..%d (DTA_EPOCH_ORDER_MAX_N)", who, n[l], l, DTA_EPOCH_ORDER_MAX_N);
      return 1;
    }
    if (!orders[l]) { dta_set_error("%s: null order table (level %d)", who, l); return 1; }
    const int id = level_ids ? level_ids[l] : l;
    if (id < 0 || id >= DTA_EPOCH_ORDER_MAX_LEVEL_ID) {
      dta_set_error("%s: level id %d (level %d): 0..%d", who, id, l, DTA_EPOCH_ORDER_MAX_LEVEL_ID - 1);
      return 1;
    }
    a.n[l] = (int)n[l];
    a.key[l] = stream_key(seed, (unsigned long long)(DTA_EPOCH_ORDER_STREAM + id));
    a.base[l] = epoch * (unsigned long long)n[l];
    a.order[l] = orders[l];
    if (n[l] > longest) longest = n[l];
  }
  for (int l = levels; l < DTA_MAX_LEVELS; ++l) { a.n[l] = 0; a.key[l] = a.base[l] = 0; a.order[l] = nullptr; }
  const unsigned blocks = (unsigned)((longest + EO_THREADS - 1) / EO_THREADS);
  hipLaunchKernelGGL(k_epoch_order, dim3(blocks, (unsigned)levels), dim3(EO_THREADS), 0, (hipStream_t)stream, a);
  DTA_CHECK_LAUNCH("k_epoch_order");
  return 0;
}

static int pool_batches(const char* who, const void* pool, int dtype, long long pool_rows, int years, int bands, int size,
                        int levels, const dta_pool_level* lv, const unsigned char* const* year_keep, float* const* outs,
                        float* flags, float* clear_next, void* stream) {
  if (!pool || !lv || !outs || !flags) { dta_set_error("%s: null argument", who); return 1; }
  if (dtype != DTA_F32 && dtype != DTA_BF16) { dta_set_error("%s: dtype=%d: DTA_F32 or DTA_BF16", who, dtype); return 1; }
  if (levels < 1 || levels > DTA_MAX_LEVELS) {
    dta_set_error("%s: levels=%d: 1..%d (DTA_MAX_LEVELS)", who, levels, DTA_MAX_LEVELS);
    return 1;
  }
  if (years < 1 || (long long)levels * years > DTA_MAX_YEARS) {
    dta_set_error("%s: levels=%d x years=%d: at most %d networks (DTA_MAX_YEARS)", who, levels, years, DTA_MAX_YEARS);
    return 1;
  }
  if (pool_rows < 1) { dta_set_error("%s: pool_rows=%lld: at least 1", who, pool_rows); return 1; }
  if (bands < 1 || bands > 65536) { dta_set_error("%s: bands=%d: 1..65536", who, bands); return 1; }
  if (size < 1 || size > 4096) { dta_set_error("%s: size=%d: 1..4096", who, size); return 1; }
  PoolArgs a;
  a.pool = pool; a.N = pool_rows; a.Y = years; a.C = bands; a.S = size;
  a.flags = flags; a.clear_next = clear_next;
  const size_t per = (size_t)bands * size * size;
  if (per > 0x7FFFFFFFull) { dta_set_error("%s: bands=%d x size=%d: a crop of more than 2^31 - 1 floats", who, bands, size); return 1; }
  size_t blocks = 0;
  bool masked = false;
  for (int l = 0; l < levels; ++l) {
    const dta_pool_level& s = lv[l];
    if (!s.rows || !s.out_rows) { dta_set_error("%s: null rows or out_rows (level %d)", who, l); return 1; }
    if ((s.labels == nullptr) != (s.out_labels == nullptr)) {
      dta_set_error("%s: labels and out_labels go together (level %d)", who, l);
      return 1;
    }
    if (s.n < 1 || s.start < 0 || s.count < 1 || s.start > s.n - s.count) {
      dta_set_error("%s: start=%lld, count=%d, n=%lld (level %d): 0 <= start, 1 <= count, start + count <= n", who, s.start,
                    s.count, s.n, l);
      return 1;
    }
    PoolLevel& d = a.lv[l];
    d.order = s.order; d.rows = s.rows; d.labels = s.labels; d.n = s.n; d.start = s.start; d.count = s.count;
    d.flip = s.flip; d.out_labels = s.out_labels; d.out_rows = s.out_rows;
    d.keep = year_keep ? year_keep[l] : nullptr;
    masked = masked || d.keep;
    for (int y = 0; y < years; ++y) {
      float* o = outs[l * years + y];
      if (!o || ((uintptr_t)o & 15)) {
        dta_set_error("%s: out of level %d, year %d is null or not 16-byte aligned", who, l, y);
        return 1;
      }
      a.out[l * years + y] = o;
    }
    const size_t b = ((size_t)s.count * per + PB_BLOCK - 1) / PB_BLOCK;
    if (b > blocks) blocks = b;
  }
  if (blocks > 0x7FFFFFFFull) { dta_set_error("%s: a batch of more than 2^41 floats", who); return 1; }
  for (int l = levels; l < DTA_MAX_LEVELS; ++l) a.lv[l] = PoolLevel{nullptr, nullptr, nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr};
  for (int k = levels * years; k < DTA_MAX_YEARS; ++k) a.out[k] = nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (!clear_next && hipMemsetAsync(flags, 0, sizeof(float) * (size_t)levels * years, st) != hipSuccess) {
    dta_set_error("%s: memset failed", who);
    return 1;
  }
  const dim3 grid((unsigned)blocks, (unsigned)(levels * years));
  if (masked) {
    if (dtype == DTA_F32) hipLaunchKernelGGL(k_pool_masked<float>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_pool_masked<bf16_t>, grid, dim3(256), 0, st, a);
  } else {
    if (dtype == DTA_F32) hipLaunchKernelGGL(k_pool_batches<float>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_pool_batches<bf16_t>, grid, dim3(256), 0, st, a);
  }
  DTA_CHECK_LAUNCH("k_pool_batches");
  return 0;
}

int dta_pool_batches(const void* pool, int dtype, long long pool_rows, int years, int bands, int size, int levels,
                     const dta_pool_level* lv, float* const* outs, float* flags, float* clear_next, void* stream) {
  return pool_batches("dta_pool_batches", pool, dtype, pool_rows, years, bands, size, levels, lv, nullptr, outs, flags,
                      clear_next, stream);
}

int dta_pool_batches_keep(const void* pool, int dtype, long long pool_rows, int years, int bands, int size, int levels,
                          const dta_pool_level* lv, const unsigned char* const* year_keep, float* const* outs, float* flags,
                          float* clear_next, void* stream) {
  return pool_batches("dta_pool_batches_keep", pool, dtype, pool_rows, years, bands, size, levels, lv, year_keep, outs,
                      flags, clear_next, stream);
}

}  // extern "C"
