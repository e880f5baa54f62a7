// Abundance per tile and map cell (reference: src/multinomial.py:run resamples ONE tile, abundance.py:read_shp counts one,
// src/neon_paths.py:bounds_to_geoindex names the tile a crown belongs to).  deeptreeattention_amd/abundance.py holds the
// definitions (cells_np, the group= forms of counts_np / resample_np, summary_np); these kernels equal them bit for bit.
//   k_abundance_cells             the cell of every crown box: float64, every operation rounded on its own
//   k_abundance_gather            the crowns in cell order (the caller sorts `group`): per sorted position the cell, the
//                                 histogram bin of the crown's own label (-1: counted nowhere) and its score
//   k_abundance_resample_grouped  a workgroup owns a FIXED slice of sorted positions and AB_G iterations, whatever the cells'
//                                 sizes: it walks the runs of equal cell inside its slice with the LDS histogram of
//                                 k_abundance_resample and flushes a run's non-zero bins at the run's end; a short run adds
//                                 its draws to the table directly.  The draws are abundance_dev.h's ab_crown, the body
//                                 k_abundance_resample uses, at the crown's index in the WHOLE input.
//   k_abundance_summary           mean and quantiles over the iterations of a table: one lane sorts one column in LDS
// A cell may lie in several slices, so the flushes are 64-bit integer atomic adds (any order gives the same sum); the table
// is cleared by a memset in front of the kernel on the same stream.  No float atomics; nothing is left in the workspace.
#include "../../include/dta_hip.h"
#include "abundance_dev.h"

namespace dta {

// ---------------------------------------------------------------------------------------------------------------------
// which cell a crown is in
// ---------------------------------------------------------------------------------------------------------------------
constexpr double CELL_LIMIT = 9007199254740992.0;       // 2^53: below it a float64 centre, and every difference here, is exact

struct CellArgs {
  const double* boxes; long long n; int rule, cols, rows;
  double ox, oy, size;                                   // DTA_CELLS_CENTRE
  long long iox, ioy, isize;                             // DTA_CELLS_GEOINDEX: integers
  long long* out;
};

// floor(a / b) for b > 0
__device__ __forceinline__ long long floor_div(long long a, long long b) {
  const long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// the index along one axis, or -1: lo / hi are the box's two coordinates on that axis
__device__ __forceinline__ long long cell_axis(const CellArgs& a, double lo, double hi, double o, long long io, int count) {
#pragma clang fp contract(off)
  if (a.rule == DTA_CELLS_GEOINDEX) {
    const double c = (lo + hi) / 2.0;
    if (!(fabs(c) < CELL_LIMIT)) return -1;              // NaN, infinite, or no integer coordinate any more
    const long long k = floor_div((long long)c - io, a.isize);      // the conversion truncates toward zero, as int() does
    return (k >= 0 && k < count) ? k : -1;
  }
  const double k = floor((mul_rounded(lo + hi, 0.5) - o) / a.size);
  return (k >= 0.0 && k < (double)count) ? (long long)k : -1;       // false for NaN
}

__global__ __launch_bounds__(256) void k_abundance_cells(CellArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const double* b = a.boxes + 4 * i;
  const long long col = cell_axis(a, b[0], b[2], a.ox, a.iox, a.cols);
  const long long row = cell_axis(a, b[1], b[3], a.oy, a.ioy, a.rows);
  a.out[i] = (col < 0 || row < 0) ? -1 : row * a.cols + col;
}

// ---------------------------------------------------------------------------------------------------------------------
// grouped counts and resampling
// ---------------------------------------------------------------------------------------------------------------------
constexpr int AB_DIRECT = 32;        // a run shorter than this skips the histogram: its draws go to the table one by one

struct AbRec { int bin; float score; };                  // bin: of the crown's own label; -1: counted nowhere

struct GroupedArgs {
  AbundanceArgs a;                                       // a.label / a.mask: read by the gather only; a.part: unused
  const long long* group_sorted; const long long* order;
  int G;
  int* cell;                                             // workspace: [n], sorted, clamped to -1 .. G
  AbRec* rec;                                            // workspace: [n]
  unsigned long long* out;                               // [iterations][G][S + 1]
};

__global__ __launch_bounds__(AB_THREADS) void k_abundance_gather(GroupedArgs q) {
  const long long p = (long long)blockIdx.x * AB_THREADS + threadIdx.x;
  if (p >= q.a.n) return;
  const long long g = q.group_sorted[p], i = q.order[p];
  q.cell[p] = g < 0 ? -1 : (g >= q.G ? q.G : (int)g);
  AbRec r;
  r.bin = -1; r.score = 0.f;
  // (an order entry outside the input is the caller's mistake: such a position is counted nowhere, nothing is read there)
  if (g >= 0 && g < q.G && i >= 0 && i < q.a.n && !(q.a.mask && q.a.mask[i] == 0)) {
    const long long lab = q.a.label[i];
    r.bin = (lab < 0 || lab >= q.a.S) ? q.a.S : (int)lab;
    if (q.a.score) r.score = q.a.score[i];
  }
  q.rec[p] = r;
}

__global__ __launch_bounds__(AB_THREADS) void k_abundance_resample_grouped(GroupedArgs q) {
  __shared__ unsigned hist[AB_G * (DTA_ABUNDANCE_MAX_SPECIES + 1)];
  const AbundanceArgs& a = q.a;
  const int bins = a.S + 1, tid = threadIdx.x;
  const int t0 = blockIdx.x * AB_G;
  const int nt = a.iterations - t0 < AB_G ? a.iterations - t0 : AB_G;
  for (int e = tid; e < nt * bins; e += AB_THREADS) hist[e] = 0u;
  __syncthreads();
  const long long p0 = (long long)blockIdx.y * a.per;
  const int len = (int)(p0 + a.per < a.n ? a.per : a.n - p0);          // ab_grouped_plan: per < 2^31
  const int* cell = q.cell + p0;
  const AbRec* rec = q.rec + p0;
  const long long* order = q.order + p0;
  const size_t plane = (size_t)q.G * bins;                               // one iteration of the table
  const AbundanceDraw d = ab_draw(a, t0, nt);
  // the runs of equal cell, one after the other: every lane takes the same steps (the barriers below rely on it)
  for (int rs = 0; rs < len;) {
    const int g = __builtin_amdgcn_readfirstlane(cell[rs]);
    int lo = rs + 1, hi = len;                                           // the first position past rs whose cell is not g
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cell[mid] <= g) lo = mid + 1; else hi = mid;
    }
    const int re = __builtin_amdgcn_readfirstlane(lo);
    if (g >= 0 && g < q.G) {
      unsigned long long* dst = q.out + (size_t)t0 * plane + (size_t)g * bins;
      if (re - rs < AB_DIRECT) {
        for (int p = rs + tid; p < re; p += AB_THREADS) {
          if (rec[p].bin < 0) continue;
          ab_crown(d, order[p], rec[p].bin, a.score ? &rec[p].score : nullptr,
                   [&](int t, int bin) { atomicAdd(dst + (size_t)t * plane + bin, 1ull); });
        }
      } else {
        for (int p = rs + tid; p < re; p += AB_THREADS) {
          if (rec[p].bin < 0) continue;
          ab_crown(d, order[p], rec[p].bin, a.score ? &rec[p].score : nullptr,
                   [&](int t, int bin) { atomicAdd(&hist[t * bins + bin], 1u); });
        }
        __syncthreads();
        for (int t = 0; t < nt; ++t)
          for (int b = tid; b < bins; b += AB_THREADS) {
            const unsigned v = hist[t * bins + b];
            if (v) { hist[t * bins + b] = 0u; atomicAdd(dst + (size_t)t * plane + b, (unsigned long long)v); }
          }
        __syncthreads();
      }
    }
    rs = re;
  }
}

struct GroupedPlan { AbundancePlan p; size_t cell_bytes, bytes; };

// the slices are k_abundance_resample's (ab_plan): fixed lengths of sorted positions, whatever the cells' sizes
static int ab_grouped_plan(const char* who, long long n, int species, int iterations, long long groups, GroupedPlan* gp) {
  if (ab_plan(who, n, species, iterations, &gp->p)) return 1;
  if (groups < 1 || groups > 0x7FFFFFFEll) { dta_set_error("%s: groups=%lld: 1..2^31-2", who, groups); return 1; }
  if (gp->p.per > 0x7FFFFFFFll) { dta_set_error("%s: n=%lld: too many crowns per workgroup", who, n); return 1; }
  gp->cell_bytes = ((size_t)n * sizeof(int) + 7) & ~(size_t)7;
  gp->bytes = gp->cell_bytes + (size_t)n * sizeof(AbRec);
  return 0;
}

static int ab_grouped_run(const char* who, GroupedArgs q, long long groups, void* workspace, size_t workspace_bytes,
                          hipStream_t st) {
  GroupedPlan gp;
  if (ab_grouped_plan(who, q.a.n, q.a.S, q.a.iterations, groups, &gp)) return 1;
  if (workspace_bytes < gp.bytes) { dta_set_error("%s: workspace too small: %zu bytes, %zu needed", who, workspace_bytes, gp.bytes); return 1; }
  if ((uintptr_t)workspace & 7) { dta_set_error("%s: the workspace must be 8-byte aligned", who); return 1; }
  if (q.a.iterations == 0) return 0;                    // an empty table: nothing to write
  q.a.per = gp.p.per; q.a.part = nullptr; q.G = (int)groups;
  q.cell = (int*)workspace; q.rec = (AbRec*)((char*)workspace + gp.cell_bytes);
  const size_t out_bytes = sizeof(long long) * (size_t)q.a.iterations * (size_t)groups * (size_t)(q.a.S + 1);
  if (hipMemsetAsync(q.out, 0, out_bytes, st) != hipSuccess) { dta_set_error("%s: clearing the table failed", who); return 1; }
  hipLaunchKernelGGL(k_abundance_gather, dim3((unsigned)((q.a.n + AB_THREADS - 1) / AB_THREADS)), dim3(AB_THREADS), 0, st, q);
  DTA_CHECK_LAUNCH("k_abundance_gather");
  hipLaunchKernelGGL(k_abundance_resample_grouped, dim3(gp.p.groups, gp.p.slices), dim3(AB_THREADS), 0, st, q);
  DTA_CHECK_LAUNCH("k_abundance_resample_grouped");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// mean and quantiles over the iterations
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SUM_LANES = 64;

struct SummaryArgs {
  const long long* table; int T; long long entries; int nq;
  int lower[DTA_ABUNDANCE_SUMMARY_MAX_QUANTILES]; double frac[DTA_ABUNDANCE_SUMMARY_MAX_QUANTILES];
  double* mean; double* quantiles;
};

// One lane owns one entry: its T values form a column of the LDS tile, col[t * 64 + lane] -- adjacent lanes, adjacent
// words.  No lane reads another's column, so there is no barrier, and a lane past the last entry simply leaves.
__global__ __launch_bounds__(SUM_LANES) void k_abundance_summary(SummaryArgs a) {
#pragma clang fp contract(off)
  extern __shared__ long long sum_tile[];
  const long long e = (long long)blockIdx.x * SUM_LANES + threadIdx.x;
  if (e >= a.entries) return;
  long long* col = sum_tile + threadIdx.x;
  long long total = 0;
  for (int t = 0; t < a.T; ++t) {                         // insertion sort while the values arrive
    const long long v = a.table[(size_t)t * a.entries + e];
    total += v;
    int k = t;
    while (k > 0 && col[(k - 1) * SUM_LANES] > v) { col[k * SUM_LANES] = col[(k - 1) * SUM_LANES]; --k; }
    col[k * SUM_LANES] = v;
  }
  a.mean[e] = (double)total / (double)a.T;
  for (int j = 0; j < a.nq; ++j) {
    const int lo = a.lower[j], hi = lo + 1 < a.T ? lo + 1 : a.T - 1;
    const double g = a.frac[j];
    const double x = (double)col[lo * SUM_LANES], y = (double)col[hi * SUM_LANES];
    const double d = y - x;
    a.quantiles[(size_t)j * a.entries + e] = g >= 0.5 ? y - mul_rounded(d, 1.0 - g) : x + mul_rounded(d, g);
  }
}

}  // namespace dta

using namespace dta;

extern "C" {

int dta_abundance_cells(const double* boxes, long long n, int rule, const double* origin, double size, int cols, int rows,
                        long long* cell, void* stream) {
  const char* who = "dta_abundance_cells";
  if (!boxes || !origin || !cell) { dta_set_error("%s: null argument", who); return 1; }
  if (n < 1) { dta_set_error("%s: bad shape: n=%lld", who, n); return 1; }
  if (cols < 1 || rows < 1) { dta_set_error("%s: cols=%d rows=%d: a grid has at least one cell", who, cols, rows); return 1; }
  if (rule != DTA_CELLS_GEOINDEX && rule != DTA_CELLS_CENTRE) { dta_set_error("%s: rule=%d: DTA_CELLS_GEOINDEX or DTA_CELLS_CENTRE", who, rule); return 1; }
  CellArgs a;
  a.boxes = boxes; a.n = n; a.rule = rule; a.cols = cols; a.rows = rows; a.out = cell;
  a.ox = origin[0]; a.oy = origin[1]; a.size = size; a.iox = 0; a.ioy = 0; a.isize = 1;
  if (!(size > 0.0) || !(size <= 1.7976931348623157e308) || !(fabs(a.ox) <= 1.7976931348623157e308) || !(fabs(a.oy) <= 1.7976931348623157e308)) {
    dta_set_error("%s: size must be positive, size and origin finite", who); return 1;
  }
  if (rule == DTA_CELLS_GEOINDEX) {
    if (size != floor(size) || a.ox != floor(a.ox) || a.oy != floor(a.oy) || size > 2147483647.0 || fabs(a.ox) >= CELL_LIMIT ||
        fabs(a.oy) >= CELL_LIMIT) {
      dta_set_error("%s: the geoindex rule takes an integer size (up to 2^31-1) and an integer origin (below 2^53)", who); return 1;
    }
    a.iox = (long long)a.ox; a.ioy = (long long)a.oy; a.isize = (long long)size;
  }
  hipLaunchKernelGGL(k_abundance_cells, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  DTA_CHECK_LAUNCH("k_abundance_cells");
  return 0;
}

size_t dta_abundance_grouped_workspace_bytes(long long n, int species, int iterations, long long groups) {
  GroupedPlan gp;
  if (ab_grouped_plan("dta_abundance_grouped_workspace_bytes", n, species, iterations, groups, &gp)) return 0;
  return gp.bytes;
}

int dta_abundance_resample_grouped(const long long* label, const float* score, const unsigned char* mask,
                                   const long long* group_sorted, const long long* order, long long n, long long groups,
                                   const unsigned int* table, int species, int iterations, unsigned long long seed,
                                   unsigned long long first_iteration, long long* counts, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  const char* who = "dta_abundance_resample_grouped";
  if (!label || !group_sorted || !order || !table || !counts || !workspace) { dta_set_error("%s: null argument", who); return 1; }
  GroupedArgs q;
  q.a.label = label; q.a.score = score; q.a.mask = mask; q.a.n = n; q.a.table = table; q.a.S = species; q.a.iterations = iterations;
  q.a.key_keep = stream_key(seed, HASH_STREAM_ABUNDANCE_KEEP); q.a.key_draw = stream_key(seed, HASH_STREAM_ABUNDANCE_DRAW);
  q.a.first = first_iteration;
  q.group_sorted = group_sorted; q.order = order; q.out = (unsigned long long*)counts;
  return ab_grouped_run(who, q, groups, workspace, workspace_bytes, (hipStream_t)stream);
}

int dta_abundance_counts_grouped(const long long* label, const unsigned char* mask, const long long* group_sorted,
                                 const long long* order, long long n, long long groups, int species, long long* counts,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "dta_abundance_counts_grouped";
  if (!label || !group_sorted || !order || !counts || !workspace) { dta_set_error("%s: null argument", who); return 1; }
  GroupedArgs q;
  q.a.label = label; q.a.score = nullptr; q.a.mask = mask; q.a.n = n; q.a.table = nullptr; q.a.S = species; q.a.iterations = 1;
  q.a.key_keep = 0; q.a.key_draw = 0; q.a.first = 0;
  q.group_sorted = group_sorted; q.order = order; q.out = (unsigned long long*)counts;
  return ab_grouped_run(who, q, groups, workspace, workspace_bytes, (hipStream_t)stream);
}

int dta_abundance_summary(const long long* table, int iterations, long long entries, const int* lower, const double* frac,
                          int quantiles, double* mean, double* out_quantiles, void* stream) {
  const char* who = "dta_abundance_summary";
  if (!table || !mean || (quantiles > 0 && (!lower || !frac || !out_quantiles))) { dta_set_error("%s: null argument", who); return 1; }
  if (iterations < 1 || iterations > DTA_ABUNDANCE_SUMMARY_MAX_ITERATIONS) {
    dta_set_error("%s: iterations=%d: 1..%d (DTA_ABUNDANCE_SUMMARY_MAX_ITERATIONS: one column per lane in LDS)", who, iterations,
                  DTA_ABUNDANCE_SUMMARY_MAX_ITERATIONS);
    return 1;
  }
  if (entries < 1 || entries > 0x7FFFFFFFll * SUM_LANES) { dta_set_error("%s: bad shape: entries=%lld", who, entries); return 1; }
  if (quantiles < 0 || quantiles > DTA_ABUNDANCE_SUMMARY_MAX_QUANTILES) {
    dta_set_error("%s: quantiles=%d: 0..%d (DTA_ABUNDANCE_SUMMARY_MAX_QUANTILES)", who, quantiles, DTA_ABUNDANCE_SUMMARY_MAX_QUANTILES);
    return 1;
  }
  SummaryArgs a;
  a.table = table; a.T = iterations; a.entries = entries; a.nq = quantiles; a.mean = mean; a.quantiles = out_quantiles;
  for (int j = 0; j < DTA_ABUNDANCE_SUMMARY_MAX_QUANTILES; ++j) { a.lower[j] = 0; a.frac[j] = 0.0; }
  for (int j = 0; j < quantiles; ++j) {
    if (lower[j] < 0 || lower[j] >= iterations || !(frac[j] >= 0.0 && frac[j] < 1.0)) {
      dta_set_error("%s: quantile %d: lower=%d frac=%g: 0 <= lower < iterations, 0 <= frac < 1", who, j, lower[j], frac[j]);
      return 1;
    }
    a.lower[j] = lower[j]; a.frac[j] = frac[j];
  }
  const size_t lds = (size_t)iterations * SUM_LANES * sizeof(long long);
  static DevOnce attr_once;
  if (attr_once.first() && hipFuncSetAttribute((const void*)k_abundance_summary, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               DTA_ABUNDANCE_SUMMARY_MAX_ITERATIONS * SUM_LANES * (int)sizeof(long long)) != hipSuccess) {
    dta_set_error("%s: the device refused %d bytes of dynamic LDS", who, DTA_ABUNDANCE_SUMMARY_MAX_ITERATIONS * SUM_LANES * 8);
    return 1;
  }
  hipLaunchKernelGGL(k_abundance_summary, dim3((unsigned)((entries + SUM_LANES - 1) / SUM_LANES)), dim3(SUM_LANES), lds,
                     (hipStream_t)stream, a);
  DTA_CHECK_LAUNCH("k_abundance_summary");
  return 0;
}

}  // extern "C"
