// The five level data sets of the reference's MultiStage.create_datasets (src/models/multi_stage.py:82-219) and the
// loss_weight_<level> buffers of its __init__ (:62-79), from one resident integer table.  deeptreeattention_amd/levels.py
// holds the definition (build_np); these kernels equal it bit for bit.  One short chain on the caller's stream:
//   k_level_count    the record sums behind k1 (CONIFER records) and k2 (records that are neither HEAD, CONIFER nor OAK):
//                    one integer atomic per workgroup.
//   k_level_rank     (train only) a lane owns an individual (blockIdx.y = 0) or a record (1) and a (group, key) pair; the
//                    pairs of its kind stream through LDS in tiles and the lane counts the pairs of ITS group with a smaller
//                    key (hash_dev.h's streamed_count).  Individuals: group = species, key = the rank of the name: pos(i | P) for
//                    every population P that holds the species.  Records of an OAK species: key = (level-2 shuffle key, r),
//                    the counter hash's draw32 in stream DTA_LEVEL_STREAM;
//                    of a CONIFER species: key = r.  A record lane then marks what its count decides: level 2's kept
//                    individuals, level 3's kept (individual, year) pairs, kept-record counts and first kept records.
//   k_level_compact  blockIdx.y = level.  A lane owns an individual; the order keys of the level's kept individuals stream
//                    through LDS (streamed_count again) and the lane counts the smaller ones: that count is its place, exactly,
//                    because the keys are distinct.  Writes rows, labels and year_keep and adds the class counts.
//   k_level_weights  per level: the classes present, 1 / count in float64, / max, the floor, rounded to float32.
// Integer atomics only (sums, one max), whose result does not depend on their order: reruns are bit-identical.
#include "../../include/dta_hip.h"
#include "common.h"
#include "hash_dev.h"

namespace dta {

namespace {

constexpr int LV_THREADS = 256;
constexpr int LV_TILE = 1024;      // pairs per LDS tile: 12 KB
constexpr int LV_LEVELS = DTA_LEVEL_COUNT;
constexpr unsigned long long LV_NONE = HASH_PAD;      // the key of an entry that takes no part: above every real key

struct LevelArgs {
  int N, R, C, Y;
  const int* ind;              // [R]
  const int* year;             // [R]
  const int* sp;               // [N]
  const int* rank;             // [N]
  const int* first;            // [N]
  const int* m;                // [N]
  const unsigned char* present;  // [N][Y]
  const int* cls;              // [C]
  const int* lmap;             // [LEVELS][C]
  const int* species_order;    // [C]
  const int* okey;             // [R] or null: the hashed shuffle
  int train;
  long long other_ceiling, evergreen_ceiling, oaks_ceiling;
  double min_loss_weight;
  unsigned long long key, base;      // stream_key(seed, DTA_LEVEL_STREAM), epoch * R mod 2^64
  // workspace (zero on entry)
  int* sums;                   // [0] CONIFER records, [1] PLAIN records
  int* count_n;                // [LEVELS] kept individuals
  int* cnt;                    // [LEVELS][C + 1] kept records per level label
  int* pos;                    // [N] same-species individuals with a smaller rank
  int* keep2;                  // [N]
  int* first3;                 // [N] 0x7FFFFFFF - (first kept record), 0: none
  int* m3;                     // [N] kept records
  unsigned char* yk3;          // [N][Y]
  // outputs
  long long* rows[LV_LEVELS];
  long long* labels[LV_LEVELS];
  unsigned char* year_keep[LV_LEVELS];
  long long cap[LV_LEVELS];
  int* n_out;                  // [LEVELS]
  int* classes_out;            // [LEVELS]
  float* weight_out;           // [LEVELS][C + 1]
};

// Every table read below is guarded: a code outside its table reads nothing and belongs to no class.
__device__ __forceinline__ int lv_species(const LevelArgs& a, int i) {
  if (i < 0 || i >= a.N) return -1;
  const int s = a.sp[i];
  return s < 0 || s >= a.C ? -1 : s;
}
__device__ __forceinline__ int lv_class(const LevelArgs& a, int s) { return s < 0 ? -1 : a.cls[s]; }

__global__ __launch_bounds__(LV_THREADS) void k_level_count(LevelArgs a) {
  __shared__ int part[2];
  if (threadIdx.x < 2) part[threadIdx.x] = 0;
  __syncthreads();
  int conifer = 0, plain = 0;
  for (long long i = (long long)blockIdx.x * LV_THREADS + threadIdx.x; i < a.N; i += (long long)gridDim.x * LV_THREADS) {
    const int c = lv_class(a, lv_species(a, (int)i));
    const int mi = a.m[i];
    conifer += c == DTA_LEVEL_CONIFER ? mi : 0;
    plain += c == DTA_LEVEL_PLAIN ? mi : 0;
  }
  if (conifer) atomicAdd(&part[0], conifer);
  if (plain) atomicAdd(&part[1], plain);
  __syncthreads();
  if (threadIdx.x < 2 && part[threadIdx.x]) atomicAdd(&a.sums[threadIdx.x], part[threadIdx.x]);
}

// The (group, key) pair of individual j (kind 0) or record j (kind 1); group -1: the entry takes no part.
__device__ __forceinline__ void lv_pair(const LevelArgs& a, int kind, int j, int& g, unsigned long long& k) {
  g = -1; k = LV_NONE;
  if (kind == 0) {
    if (j >= a.N) return;
    g = lv_species(a, j);
    k = (unsigned)a.rank[j];
    return;
  }
  if (j >= a.R) return;
  const int s = lv_species(a, a.ind[j]);
  const int c = lv_class(a, s);
  if (c == DTA_LEVEL_OAK) {
    const unsigned long long draw = a.okey ? (unsigned long long)(unsigned)a.okey[j] : draw32(a.base, a.key, j);
    g = s; k = (draw << 32) | (unsigned)j;
  } else if (c == DTA_LEVEL_CONIFER) {
    g = s; k = (unsigned)j;
  }
}

__global__ __launch_bounds__(LV_THREADS) void k_level_rank(LevelArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned long long tk[LV_TILE];
  __shared__ int tg[LV_TILE];
  const int kind = blockIdx.y, n = kind == 0 ? a.N : a.R;
  if ((long long)blockIdx.x * LV_THREADS >= n) return;         // (the whole workgroup)
  const int i = blockIdx.x * LV_THREADS + threadIdx.x;
  int g; unsigned long long mine;
  lv_pair(a, kind, i, g, mine);
  const int count = streamed_count<LV_TILE, LV_THREADS>(
      n,
      [&](int k, int j) {
        int gj; unsigned long long kj;
        lv_pair(a, kind, j, gj, kj);
        tg[k] = gj < 0 ? -2 : gj;                              // (-2: equals no lane's group)
        tk[k] = kj;
      },
      [&](int k) { return tg[k] == g && tk[k] < mine; });
  if (i >= n || g < 0) return;
  if (kind == 0) { a.pos[i] = count; return; }
  const int who = a.ind[i];                                    // (in range: lv_species said so)
  if (lv_class(a, g) == DTA_LEVEL_OAK) {
    const long long k2 = a.sums[1] / 5;
    if (count < k2) a.keep2[who] = 1;                          // (every writer stores the same value)
  } else if (count < a.evergreen_ceiling) {
    const int y = a.year[i];
    if (y >= 0 && y < a.Y) a.yk3[(size_t)who * a.Y + y] = 1;
    atomicAdd(&a.m3[who], 1);
    atomicMax(&a.first3[who], 0x7FFFFFFF - i);
  }
}

// The order key of individual j in level l, or LV_NONE when the level does not keep it.
__device__ __forceinline__ unsigned long long lv_order_key(const LevelArgs& a, int l, int j) {
  if (j >= a.N) return LV_NONE;
  const int s = lv_species(a, j);
  const int c = lv_class(a, s);
  if (c < DTA_LEVEL_HEAD || c > DTA_LEVEL_PLAIN) return LV_NONE;
  const unsigned long long first = (unsigned)a.first[j];
  bool in;
  switch (l) {
    case 0: in = true; break;
    case 1: in = c != DTA_LEVEL_HEAD; break;
    case 2: in = c == DTA_LEVEL_OAK || c == DTA_LEVEL_PLAIN; break;
    case 3: in = c == DTA_LEVEL_CONIFER; break;
    default: in = c == DTA_LEVEL_OAK; break;
  }
  if (!in) return LV_NONE;
  if (!a.train) return first;
  switch (l) {
    case 0:
      if (c == DTA_LEVEL_HEAD) return first;
      return a.pos[j] < a.other_ceiling ? (1ull << 32) | first : LV_NONE;
    case 1: {
      const long long k1 = ((long long)a.sums[0] + 10) / 11;
      return c == DTA_LEVEL_CONIFER || a.pos[j] < k1 ? first : LV_NONE;
    }
    case 2: return c == DTA_LEVEL_PLAIN || a.keep2[j] ? first : LV_NONE;
    case 3: {
      const int f = a.first3[j];
      if (a.m3[j] < 1 || f < 1) return LV_NONE;
      return ((unsigned long long)(unsigned)a.species_order[s] << 32) | (unsigned)(0x7FFFFFFF - f);
    }
    default: return a.pos[j] < a.oaks_ceiling ? first : LV_NONE;
  }
}

__global__ __launch_bounds__(LV_THREADS) void k_level_compact(LevelArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned long long tile[LV_TILE];
  const int l = blockIdx.y, n = a.N;
  const int i = blockIdx.x * LV_THREADS + threadIdx.x;
  const unsigned long long mine = lv_order_key(a, l, i);
  const int place = streamed_count<LV_TILE, LV_THREADS>(
      n, [&](int k, int j) { tile[k] = lv_order_key(a, l, j); }, [&](int k) { return tile[k] < mine; });
  if (mine == LV_NONE) return;
  const int s = a.sp[i];                                       // (in range: lv_order_key said so)
  const int label = a.lmap[l * a.C + s];
  const bool cut = a.train && l == 3;
  atomicAdd(&a.count_n[l], 1);
  if (label >= 0 && label <= a.C) atomicAdd(&a.cnt[l * (a.C + 1) + label], cut ? a.m3[i] : a.m[i]);
  if (place >= a.cap[l]) return;
  a.rows[l][place] = i;
  a.labels[l][place] = label;
  const unsigned char* keep = cut ? a.yk3 : a.present;
  for (int y = 0; y < a.Y; ++y) a.year_keep[l][(size_t)place * a.Y + y] = keep[(size_t)i * a.Y + y] ? 1 : 0;
}

__global__ __launch_bounds__(LV_THREADS) void k_level_weights(LevelArgs a) {
  __shared__ int s_classes, s_min;
  const int l = blockIdx.x, W = a.C + 1;
  const int* cnt = a.cnt + l * W;
  if (threadIdx.x == 0) { s_classes = 0; s_min = 0x7FFFFFFF; }
  __syncthreads();
  int have = 0, least = 0x7FFFFFFF;
  for (int x = threadIdx.x; x < W; x += LV_THREADS) {
    const int c = cnt[x];
    if (c > 0) { ++have; least = c < least ? c : least; }
  }
  if (have) { atomicAdd(&s_classes, have); atomicMin(&s_min, least); }
  __syncthreads();
  const int classes = s_classes;
  if (threadIdx.x == 0) { a.n_out[l] = a.count_n[l]; a.classes_out[l] = classes; }
  if (!a.weight_out) return;
  const double top = 1.0 / (double)s_min;                      // max of the 1 / count: 1 / (the least count)
  for (int x = threadIdx.x; x < W; x += LV_THREADS) {
    float w = 0.f;
    if (x < classes) {
      double v = a.min_loss_weight;
      if (cnt[x] > 0) {
        v = (1.0 / (double)cnt[x]) / top;
        if (v < a.min_loss_weight) v = a.min_loss_weight;
      }
      w = (float)v;
    }
    a.weight_out[l * W + x] = w;
  }
}

size_t lv_align(size_t v) { return (v + 15) & ~(size_t)15; }

struct LevelSpace { size_t sums, count_n, cnt, pos, keep2, first3, m3, yk3, total; };

LevelSpace lv_space(long long N, int C, int Y) {
  LevelSpace s;
  size_t at = 0;
  s.sums = at;    at += lv_align(sizeof(int) * 2);
  s.count_n = at; at += lv_align(sizeof(int) * LV_LEVELS);
  s.cnt = at;     at += lv_align(sizeof(int) * LV_LEVELS * ((size_t)C + 1));
  s.pos = at;     at += lv_align(sizeof(int) * (size_t)N);
  s.keep2 = at;   at += lv_align(sizeof(int) * (size_t)N);
  s.first3 = at;  at += lv_align(sizeof(int) * (size_t)N);
  s.m3 = at;      at += lv_align(sizeof(int) * (size_t)N);
  s.yk3 = at;     at += lv_align((size_t)N * Y);
  s.total = at;
  return s;
}

bool lv_sizes_ok(long long N, long long R, int C, int Y) {
  return N >= 1 && N <= DTA_EPOCH_ORDER_MAX_N && Y >= 1 && Y <= DTA_MAX_YEARS && R >= N && R <= N * DTA_MAX_YEARS &&
         C >= 1 && C <= DTA_LEVEL_MAX_SPECIES;
}

}  // namespace

}  // namespace dta

using namespace dta;

extern "C" {

size_t dta_level_workspace_bytes(long long individuals, long long records, int species, int years) {
  if (!lv_sizes_ok(individuals, records, species, years)) return 0;
  return lv_space(individuals, species, years).total;
}

int dta_level_build(const dta_level_tables* t, const dta_level_config* cfg, const dta_level_out* out, void* workspace,
                    size_t workspace_bytes, void* stream) {
  const char* who = "dta_level_build";
  if (!t || !cfg || !out || !workspace) { dta_set_error("%s: null argument", who); return 1; }
  if (!lv_sizes_ok(t->individuals, t->records, t->species, t->years)) {
    dta_set_error("%s: individuals=%lld (1..%d), records=%lld (individuals..%d x individuals), species=%d (1..%d), years=%d "
                  "(1..%d)", who, t->individuals, DTA_EPOCH_ORDER_MAX_N, t->records, DTA_MAX_YEARS, t->species,
                  DTA_LEVEL_MAX_SPECIES, t->years, DTA_MAX_YEARS);
    return 1;
  }
  if (!t->ind || !t->year || !t->sp || !t->rank || !t->first || !t->m || !t->present || !t->cls || !t->lmap ||
      !t->species_order) {
    dta_set_error("%s: null table", who);
    return 1;
  }
  if (cfg->train != 0 && cfg->train != 1) { dta_set_error("%s: train=%d: 0 or 1", who, cfg->train); return 1; }
  if (cfg->other_sampling_ceiling < 0 || cfg->evergreen_ceiling < 0 || cfg->oaks_sampling_ceiling < 0) {
    dta_set_error("%s: a ceiling below 0 (%lld, %lld, %lld)", who, cfg->other_sampling_ceiling, cfg->evergreen_ceiling,
                  cfg->oaks_sampling_ceiling);
    return 1;
  }
  if (!(cfg->min_loss_weight >= 0.0 && cfg->min_loss_weight <= 1.0)) {
    dta_set_error("%s: min_loss_weight=%g: 0..1", who, cfg->min_loss_weight);
    return 1;
  }
  if (!out->n || !out->num_classes || (cfg->train && !out->loss_weight)) {
    dta_set_error("%s: null n, num_classes or loss_weight", who);
    return 1;
  }
  const LevelSpace sp = lv_space(t->individuals, t->species, t->years);
  if (workspace_bytes < sp.total || ((uintptr_t)workspace & 15)) {
    dta_set_error("%s: workspace of %zu bytes (needs %zu, 16-byte aligned)", who, workspace_bytes, sp.total);
    return 1;
  }
  LevelArgs a;
  a.N = (int)t->individuals; a.R = (int)t->records; a.C = t->species; a.Y = t->years;
  a.ind = t->ind; a.year = t->year; a.sp = t->sp; a.rank = t->rank; a.first = t->first; a.m = t->m;
  a.present = t->present; a.cls = t->cls; a.lmap = t->lmap; a.species_order = t->species_order; a.okey = t->record_key;
  a.train = cfg->train;
  a.other_ceiling = cfg->other_sampling_ceiling; a.evergreen_ceiling = cfg->evergreen_ceiling;
  a.oaks_ceiling = cfg->oaks_sampling_ceiling; a.min_loss_weight = cfg->min_loss_weight;
  a.key = stream_key(cfg->seed, DTA_LEVEL_STREAM);
  a.base = cfg->epoch * (unsigned long long)t->records;
  char* w = (char*)workspace;
  a.sums = (int*)(w + sp.sums); a.count_n = (int*)(w + sp.count_n); a.cnt = (int*)(w + sp.cnt);
  a.pos = (int*)(w + sp.pos); a.keep2 = (int*)(w + sp.keep2); a.first3 = (int*)(w + sp.first3); a.m3 = (int*)(w + sp.m3);
  a.yk3 = (unsigned char*)(w + sp.yk3);
  for (int l = 0; l < LV_LEVELS; ++l) {
    if (out->capacity[l] < 0 || out->capacity[l] > t->individuals) {
      dta_set_error("%s: capacity=%lld (level %d): 0..individuals", who, out->capacity[l], l);
      return 1;
    }
    if (out->capacity[l] > 0 && (!out->rows[l] || !out->labels[l] || !out->year_keep[l])) {
      dta_set_error("%s: null rows, labels or year_keep (level %d)", who, l);
      return 1;
    }
    a.rows[l] = out->rows[l]; a.labels[l] = out->labels[l]; a.year_keep[l] = out->year_keep[l]; a.cap[l] = out->capacity[l];
  }
  a.n_out = out->n; a.classes_out = out->num_classes; a.weight_out = cfg->train ? out->loss_weight : nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(workspace, 0, sp.total, st) != hipSuccess) { dta_set_error("%s: memset failed", who); return 1; }
  const unsigned nb = (unsigned)((t->individuals + LV_THREADS - 1) / LV_THREADS);
  const unsigned rb = (unsigned)((t->records + LV_THREADS - 1) / LV_THREADS);
  hipLaunchKernelGGL(k_level_count, dim3(nb < 256u ? nb : 256u), dim3(LV_THREADS), 0, st, a);
  DTA_CHECK_LAUNCH("k_level_count");
  if (cfg->train) {
    hipLaunchKernelGGL(k_level_rank, dim3(rb > nb ? rb : nb, 2), dim3(LV_THREADS), 0, st, a);
    DTA_CHECK_LAUNCH("k_level_rank");
  }
  hipLaunchKernelGGL(k_level_compact, dim3(nb, LV_LEVELS), dim3(LV_THREADS), 0, st, a);
  DTA_CHECK_LAUNCH("k_level_compact");
  hipLaunchKernelGGL(k_level_weights, dim3(LV_LEVELS), dim3(LV_THREADS), 0, st, a);
  DTA_CHECK_LAUNCH("k_level_weights");
  return 0;
}

}  // extern "C"
