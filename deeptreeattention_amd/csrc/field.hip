// Field records to canopy points: which rows of a raw NEON field table survive (the reference's filter_data,
// src/data.py:22-106: a Python loop over groupby("individual"), a groupby.apply per individual) and the plot code of every
// stem of a contributed megaplot (megaplot.format's create_grid + gpd.sjoin and buffer_plots, src/megaplot.py:41-90: a grid
// of shapely boxes, an O(n^2) loop of shapely buffers).  deeptreeattention_amd/field.py holds the definitions (filter_np,
// plots_np); these kernels equal them bit for bit.
//
// dta_field_filter, one row per lane, the per-individual state in global arrays indexed by the individual code:
//   k_field_shade    steps 1-3 from the flag bits; a row that passed them ORs its shaded / sunny bits into its individual
//                    (atomic OR); fills rows_out with -1
//   k_field_best     steps 1-8 (step 4 reads the finished bits); writes the provisional reason; a row that passed them
//                    raises its individual's maximum height (64-bit atomic max on the order-preserving bit pattern of the
//                    double, +0.0 and -0.0 alike) or, without a height, its latest event as one packed
//                    (event << 32) | ~row (64-bit atomic max: the largest event, the lowest row among equals)
//   k_field_first    the rows at their individual's maximum height: the lowest of them (32-bit atomic max on 2^31 - 1 - row)
//   k_field_pick     blockIdx.y = 0, from the row's side: step 9 and steps 10-13, the final reason and keep;
//                    blockIdx.y = 1, from the individual's side: the kept row of every individual (or none), chosen by
//                    height or by event, and how many of each kind its workgroup holds (plain stores)
//   k_field_compact  a lane owns an individual: the kept ones before it in its workgroup (a scan) and in the workgroups
//                    before (their counts, summed by every workgroup for itself) are its place in rows_out: first the
//                    individuals chosen by height, then those chosen by event, both ascending by code.  Writes count.
// Integer OR / max atomics at device scope only, whose result does not depend on their order: reruns are bit-identical.
// Every table read is guarded: a row whose individual code lies outside 0 .. individuals-1 or whose event code is
// negative takes no part, gets reason 255 and is counted in the error word.
//
// dta_megaplot_plots, one stem per lane:
//   k_megaplot_grid    the cell by one division, then the neighbouring columns and rows of the xs / ys tables checked with
//                      the definition's own comparisons: the lowest code among the cells that hold the point
//   k_megaplot_buffer  the other stems streamed through LDS in chunks (as k_stems_* do): the highest i with
//                      d2(i, j) <= cell * cell, every product and sum rounded on its own
#include "../../include/dta_hip.h"
#include "common.h"

#include <cmath>

// no fused multiply-add in this file: (xi - xj) * (xi - xj) + (yi - yj) * (yi - yj) is the definition's operations one by one
#pragma clang fp contract(off)

namespace dta {

namespace {

constexpr int FD_THREADS = 256;
constexpr int FD_WAVES = FD_THREADS / 64;
constexpr int MP_CHUNK = DTA_MEGAPLOT_CHUNK;
constexpr unsigned char FD_BAD = DTA_FIELD_REASON_BAD_CODE;

struct FieldArgs {
  int N, I;
  const int* ind;                // [N]
  const int* event;              // [N]
  const double* height;          // [N]
  const double* diameter;        // [N]
  const unsigned short* flags;   // [N]
  double min_diameter, min_height;
  // workspace (zero on entry)
  unsigned* shade;               // [I] DTA_FIELD_SHADED | DTA_FIELD_SUNNY over the rows that passed steps 1-3
  unsigned long long* hkey;      // [I] the largest height key, 0: no height
  unsigned long long* ekey;      // [I] the largest (event << 32) | ~row over the rows without a height, 0: none
  int* hrow;                     // [I] 0x7FFFFFFF - (the lowest row at hkey), 0: none
  int* sel;                      // [I] the kept row + 1, negative: chosen by event; 0: none
  int* blocks;                   // [2][nb] kept individuals per workgroup, by height and by event
  int* errors;                   // [1]
  // outputs
  unsigned char* keep;           // [N]
  unsigned char* reason;         // [N]
  long long* rows;               // [N]
  long long* count;              // [1]
  int* errors_out;               // [1] or null
  int nb;                        // workgroups over the individuals
};

// The order-preserving bit pattern of a double that is not NaN: a < b <=> key(a) < key(b), -0.0 and +0.0 alike; never 0.
__device__ __forceinline__ unsigned long long height_key(double h) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(h + 0.0);        // (-0.0 + 0.0 = +0.0)
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ bool fd_code_ok(const FieldArgs& a, int who, int ev) { return who >= 0 && who < a.I && ev >= 0; }

// Steps 1-3, from the flag bits alone.
__device__ __forceinline__ int fd_steps_1_3(unsigned f) {
  if (!(f & DTA_FIELD_COORDS)) return 1;
  if (!(f & DTA_FIELD_GROWTH)) return 2;
  if (!(f & DTA_FIELD_LIVE)) return 3;
  return 0;
}

// Steps 1-8 of row i of individual `who` (in range); shade[] is final.
__device__ __forceinline__ int fd_steps_1_8(const FieldArgs& a, int i, int who, unsigned f) {
  int r = fd_steps_1_3(f);
  if (r) return r;
  const unsigned s = a.shade[who];
  if ((s & DTA_FIELD_SHADED) && !(s & DTA_FIELD_SUNNY)) return 4;
  const double h = a.height[i], d = a.diameter[i];
  if (!(h > a.min_height || h != h)) return 5;
  if (!(d > a.min_diameter)) return 6;
  if (f & DTA_FIELD_TAXON_EXCLUDED) return 7;
  if (f & DTA_FIELD_EVENT_DROPPED) return 8;
  return 0;
}

// Steps 10-13, from the flag bits alone.
__device__ __forceinline__ int fd_steps_10_13(unsigned f) {
  if (f & DTA_FIELD_MULTIBOLE) return 10;
  if (f & DTA_FIELD_KNOWN_ERROR) return 11;
  if (f & DTA_FIELD_PLOT_EXCLUDED) return 12;
  if (f & DTA_FIELD_SITE_EXCLUDED) return 13;
  return 0;
}

// The record of individual `who` (step 9): its row, or -1; by_event: chosen by the latest event.
__device__ __forceinline__ int fd_record(const FieldArgs& a, int who, bool& by_event) {
  by_event = false;
  if (a.hkey[who]) {
    const int v = a.hrow[who];
    return v > 0 ? 0x7FFFFFFF - v : -1;
  }
  const unsigned long long e = a.ekey[who];
  by_event = true;
  return e ? (int)~(unsigned)e : -1;
}

__global__ __launch_bounds__(FD_THREADS) void k_field_shade(FieldArgs a) {
  const long long i = (long long)blockIdx.x * FD_THREADS + threadIdx.x;
  if (i >= a.N) return;
  a.rows[i] = -1;
  const int who = a.ind[i], ev = a.event[i];
  if (!fd_code_ok(a, who, ev)) { atomicAdd(a.errors, 1); return; }
  const unsigned f = a.flags[i];
  const unsigned bits = f & (DTA_FIELD_SHADED | DTA_FIELD_SUNNY);
  if (bits && fd_steps_1_3(f) == 0) atomicOr(&a.shade[who], bits);
}

__global__ __launch_bounds__(FD_THREADS) void k_field_best(FieldArgs a) {
  const long long i = (long long)blockIdx.x * FD_THREADS + threadIdx.x;
  if (i >= a.N) return;
  const int who = a.ind[i], ev = a.event[i];
  if (!fd_code_ok(a, who, ev)) { a.reason[i] = FD_BAD; return; }
  const int r = fd_steps_1_8(a, (int)i, who, a.flags[i]);
  a.reason[i] = (unsigned char)r;
  if (r) return;
  const double h = a.height[i];
  if (h == h) atomicMax(&a.hkey[who], height_key(h));
  else atomicMax(&a.ekey[who], ((unsigned long long)(unsigned)ev << 32) | (unsigned)~(unsigned)i);
}

__global__ __launch_bounds__(FD_THREADS) void k_field_first(FieldArgs a) {
  const long long i = (long long)blockIdx.x * FD_THREADS + threadIdx.x;
  if (i >= a.N || a.reason[i] != 0) return;
  const int who = a.ind[i];                                        // (in range: the reason says so)
  const double h = a.height[i];
  if (h == h && height_key(h) == a.hkey[who]) atomicMax(&a.hrow[who], 0x7FFFFFFF - (int)i);
}

__global__ __launch_bounds__(FD_THREADS) void k_field_pick(FieldArgs a) {
  __shared__ int part[2][FD_WAVES];
  const long long i = (long long)blockIdx.x * FD_THREADS + threadIdx.x;
  if (blockIdx.y == 0) {                                           // the row's side
    if (i >= a.N) return;
    int r = a.reason[i];
    if (r == 0) {
      bool by_event;
      r = fd_record(a, a.ind[i], by_event) == (int)i ? fd_steps_10_13(a.flags[i]) : 9;
      a.reason[i] = (unsigned char)r;
    }
    a.keep[i] = r == 0;
    return;
  }
  if ((long long)blockIdx.x * FD_THREADS >= a.I) return;          // (the whole workgroup)
  bool by_event = false;
  int row = -1;
  if (i < a.I) {                                                   // the individual's side
    row = fd_record(a, (int)i, by_event);
    if (row >= a.N || (row >= 0 && fd_steps_10_13(a.flags[row]))) row = -1;
    a.sel[i] = row < 0 ? 0 : (by_event ? -(row + 1) : row + 1);
  }
  const unsigned long long bh = __ballot(row >= 0 && !by_event), be = __ballot(row >= 0 && by_event);
  if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = __popcll(bh); part[1][threadIdx.x >> 6] = __popcll(be); }
  __syncthreads();
  if (threadIdx.x < 2) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < FD_WAVES; ++w) s += part[threadIdx.x][w];
    a.blocks[threadIdx.x * a.nb + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(FD_THREADS) void k_field_compact(FieldArgs a) {
  __shared__ long long tot[4][FD_WAVES];
  __shared__ int part[2][FD_WAVES];
  // kept individuals, by height and by event: v[0], v[1] in the workgroups before this one, v[2], v[3] in all of them
  long long v[4] = {0, 0, 0, 0};
  for (int b = threadIdx.x; b < a.nb; b += FD_THREADS) {
    const int h = a.blocks[b], e = a.blocks[a.nb + b];
    v[2] += h; v[3] += e;
    if (b < (int)blockIdx.x) { v[0] += h; v[1] += e; }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long i = (long long)blockIdx.x * FD_THREADS + threadIdx.x;
  const int s = i < a.I ? a.sel[i] : 0;
  const unsigned long long bh = __ballot(s > 0), be = __ballot(s < 0);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) tot[k][wave] = v[k];
    part[0][wave] = __popcll(bh); part[1][wave] = __popcll(be);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = 0;
#pragma unroll
    for (int w = 0; w < FD_WAVES; ++w) v[k] += tot[k][w];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.count[0] = v[2] + v[3];
    if (a.errors_out) a.errors_out[0] = a.errors[0];
  }
  if (s == 0) return;
  const int kind = s < 0;
  long long place = kind ? v[2] + v[1] : v[0];                     // those chosen by event follow all chosen by height
  for (int w = 0; w < wave; ++w) place += part[kind][w];
  place += __popcll((kind ? be : bh) & ((1ull << lane) - 1));
  if (place < a.N) a.rows[place] = (kind ? -s : s) - 1;
}

// ---- megaplot ------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(FD_THREADS) void k_megaplot_grid(const double* points, int n, double cell, const double* xs, int nx,
                                                              const double* ys, int ny, int* code) {
  const long long p = (long long)blockIdx.x * FD_THREADS + threadIdx.x;
  if (p >= n) return;
  const double x = points[2 * p], y = points[2 * p + 1];
  int out = -1;
  if (finite_d(x) && finite_d(y)) {
    // the guess: one division, clamped into the table while still a double
    double gx = floor((x - xs[0]) / cell), gy = floor((y - ys[0]) / cell);
    gx = gx == gx ? gx : 0.0; gy = gy == gy ? gy : 0.0;
    gx = gx < 0.0 ? 0.0 : (gx > (double)(nx - 1) ? (double)(nx - 1) : gx);
    gy = gy < 0.0 ? 0.0 : (gy > (double)(ny - 1) ? (double)(ny - 1) : gy);
    const int ix = (int)gx, iy = (int)gy;
    int ci = -1, cj = -1;
    for (int i = ix + 2; i >= ix - 2; --i) {                       // descending: the lowest stays
      if (i < 0 || i >= nx) continue;
      const double hi = xs[i], lo = hi - cell;
      if (lo <= x && x <= hi) ci = i;
    }
    for (int j = iy + 2; j >= iy - 2; --j) {
      if (j < 0 || j >= ny) continue;
      const double lo = ys[j], hi = lo + cell;
      if (lo <= y && y <= hi) cj = j;
    }
    if (ci >= 0 && cj >= 0) out = ci * ny + cj;
  }
  code[p] = out;
}

__global__ __launch_bounds__(FD_THREADS) void k_megaplot_buffer(const double* points, int n, double r2, int* code) {
  __shared__ double sh[2 * MP_CHUNK];
  const int j = blockIdx.x * FD_THREADS + threadIdx.x;
  const bool have = j < n;
  const double xj = have ? points[2 * (size_t)j] : NAN, yj = have ? points[2 * (size_t)j + 1] : NAN;
  int best = -1;
  for (int base = 0; base < n; base += MP_CHUNK) {                 // the same trips, the same barriers in every thread
    const int cnt = n - base < MP_CHUNK ? n - base : MP_CHUNK;
    __syncthreads();                                               // the previous chunk has been read by every lane
    for (int k = threadIdx.x; k < 2 * cnt; k += FD_THREADS) sh[k] = points[2 * (size_t)base + k];
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < cnt; ++k) {
      const double dx = sh[2 * k] - xj, dy = sh[2 * k + 1] - yj;
      const double d2 = mul_rounded(dx, dx) + mul_rounded(dy, dy);
      best = d2 <= r2 ? base + k : best;                           // ascending i: the highest stays; false with a NaN
    }
  }
  if (have) code[j] = best;
}

size_t fd_align(size_t v) { return (v + 15) & ~(size_t)15; }

struct FieldSpace { size_t shade, hkey, ekey, hrow, sel, blocks, errors, total; };

int fd_blocks(long long individuals) { return (int)((individuals + FD_THREADS - 1) / FD_THREADS); }

FieldSpace fd_space(long long I) {
  FieldSpace s;
  size_t at = 0;
  s.hkey = at;   at += fd_align(sizeof(unsigned long long) * (size_t)I);
  s.ekey = at;   at += fd_align(sizeof(unsigned long long) * (size_t)I);
  s.shade = at;  at += fd_align(sizeof(unsigned) * (size_t)I);
  s.hrow = at;   at += fd_align(sizeof(int) * (size_t)I);
  s.sel = at;    at += fd_align(sizeof(int) * (size_t)I);
  s.blocks = at; at += fd_align(sizeof(int) * 2 * (size_t)fd_blocks(I));
  s.errors = at; at += fd_align(sizeof(int));
  s.total = at;
  return s;
}

bool fd_sizes_ok(long long N, long long I) { return N >= 1 && N <= 0x7FFFFFFFll && I >= 1 && I <= N; }

}  // namespace

}  // namespace dta

using namespace dta;

extern "C" {

size_t dta_field_workspace_bytes(long long rows, long long individuals) {
  if (!fd_sizes_ok(rows, individuals)) return 0;
  return fd_space(individuals).total;
}

int dta_field_filter(const int* individual, const int* event, const double* height, const double* diameter,
                     const unsigned short* flags, long long rows, long long individuals, double min_stem_diameter,
                     double min_height, unsigned char* keep_out, unsigned char* reason_out, long long* rows_out,
                     long long* count_out, int* errors_out, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "dta_field_filter";
  if (!individual || !event || !height || !diameter || !flags || !keep_out || !reason_out || !rows_out || !count_out || !workspace) {
    dta_set_error("%s: null argument", who);
    return 1;
  }
  if (rows < 1 || rows > 0x7FFFFFFFll) { dta_set_error("%s: bad shape: rows=%lld (1 .. 2^31 - 1)", who, rows); return 1; }
  if (individuals < 1 || individuals > rows) {
    dta_set_error("%s: bad shape: individuals=%lld (1 .. rows=%lld)", who, individuals, rows);
    return 1;
  }
  if (std::isnan(min_stem_diameter)) { dta_set_error("%s: min_stem_diameter=%g is not a number", who, min_stem_diameter); return 1; }
  if (std::isnan(min_height)) { dta_set_error("%s: min_height=%g is not a number", who, min_height); return 1; }
  const FieldSpace sp = fd_space(individuals);
  if (workspace_bytes < sp.total || ((uintptr_t)workspace & 15)) {
    dta_set_error("%s: workspace of %zu bytes (needs %zu, 16-byte aligned)", who, workspace_bytes, sp.total);
    return 1;
  }
  FieldArgs a;
  a.N = (int)rows; a.I = (int)individuals;
  a.ind = individual; a.event = event; a.height = height; a.diameter = diameter; a.flags = flags;
  a.min_diameter = min_stem_diameter; a.min_height = min_height;
  char* w = (char*)workspace;
  a.shade = (unsigned*)(w + sp.shade); a.hkey = (unsigned long long*)(w + sp.hkey); a.ekey = (unsigned long long*)(w + sp.ekey);
  a.hrow = (int*)(w + sp.hrow); a.sel = (int*)(w + sp.sel); a.blocks = (int*)(w + sp.blocks); a.errors = (int*)(w + sp.errors);
  a.keep = keep_out; a.reason = reason_out; a.rows = rows_out; a.count = count_out; a.errors_out = errors_out;
  a.nb = fd_blocks(individuals);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(workspace, 0, sp.total, st) != hipSuccess) { dta_set_error("%s: memset failed", who); return 1; }
  const unsigned rb = (unsigned)((rows + FD_THREADS - 1) / FD_THREADS), ib = (unsigned)a.nb;
  hipLaunchKernelGGL(k_field_shade, dim3(rb), dim3(FD_THREADS), 0, st, a);
  DTA_CHECK_LAUNCH("k_field_shade");
  hipLaunchKernelGGL(k_field_best, dim3(rb), dim3(FD_THREADS), 0, st, a);
  DTA_CHECK_LAUNCH("k_field_best");
  hipLaunchKernelGGL(k_field_first, dim3(rb), dim3(FD_THREADS), 0, st, a);
  DTA_CHECK_LAUNCH("k_field_first");
  hipLaunchKernelGGL(k_field_pick, dim3(rb > ib ? rb : ib, 2), dim3(FD_THREADS), 0, st, a);
  DTA_CHECK_LAUNCH("k_field_pick");
  hipLaunchKernelGGL(k_field_compact, dim3(ib), dim3(FD_THREADS), 0, st, a);
  DTA_CHECK_LAUNCH("k_field_compact");
  return 0;
}

int dta_megaplot_plots(const double* points, long long n, int rule, double cell, const double* xs, int nx, const double* ys,
                       int ny, int* code_out, void* stream) {
  const char* who = "dta_megaplot_plots";
  if (!points || !code_out) { dta_set_error("%s: null argument", who); return 1; }
  if (rule != DTA_MEGAPLOT_GRID && rule != DTA_MEGAPLOT_BUFFER) {
    dta_set_error("%s: rule=%d: DTA_MEGAPLOT_GRID or DTA_MEGAPLOT_BUFFER", who, rule);
    return 1;
  }
  if (!std::isfinite(cell) || !(cell > 0.0)) { dta_set_error("%s: cell=%g is not a finite number above 0", who, cell); return 1; }
  hipStream_t st = (hipStream_t)stream;
  if (rule == DTA_MEGAPLOT_BUFFER) {
    if (n < 1 || n > DTA_MEGAPLOT_BUFFER_MAX) {
      dta_set_error("%s: bad shape: n=%lld (1 .. %d for the buffer rule, which compares every pair)", who, n,
                    DTA_MEGAPLOT_BUFFER_MAX);
      return 1;
    }
    const double r2 = cell * cell;
    if (!std::isfinite(r2)) { dta_set_error("%s: cell=%g: cell * cell is not finite", who, cell); return 1; }
    hipLaunchKernelGGL(k_megaplot_buffer, dim3((unsigned)((n + FD_THREADS - 1) / FD_THREADS)), dim3(FD_THREADS), 0, st, points,
                       (int)n, r2, code_out);
    DTA_CHECK_LAUNCH("k_megaplot_buffer");
    return 0;
  }
  if (n < 1 || n > 0x7FFFFFFFll) { dta_set_error("%s: bad shape: n=%lld (1 .. 2^31 - 1)", who, n); return 1; }
  if (!xs || !ys) { dta_set_error("%s: null xs or ys table", who); return 1; }
  if (nx < 1 || ny < 1 || (long long)nx * ny > 0x7FFFFFFFll) {
    dta_set_error("%s: bad shape: nx=%d, ny=%d (each >= 1, nx * ny <= 2^31 - 1)", who, nx, ny);
    return 1;
  }
  hipLaunchKernelGGL(k_megaplot_grid, dim3((unsigned)((n + FD_THREADS - 1) / FD_THREADS)), dim3(FD_THREADS), 0, st, points, (int)n,
                     cell, xs, nx, ys, ny, code_out);
  DTA_CHECK_LAUNCH("k_megaplot_grid");
  return 0;
}

}  // extern "C"
