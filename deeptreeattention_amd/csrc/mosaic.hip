// Crown boxes of a tile from a detector's per-window output (reference src/predict.py:112-138 predict_crowns and
// src/generate.py:17-60 predict_trees, i.e. DeepForest's predict_tile: shift every window's boxes by the window origin, then
// greedy non-maximum suppression at IoU 0.15 over the whole tile).  deeptreeattention_amd/mosaic.py holds the definition
// (nms_np, pixel_boxes_np); these kernels equal it bit for bit: float32 throughout, every operation rounded on its own, and
// nothing depends on the order in which the boxes of a cell were filled in.
//   k_mosaic_prep    one box per lane: shift, refuse / mask, pixel box, the cell of the centre, the cell's count (atomic)
//   k_mosaic_scan    one workgroup: exclusive scan of the cell counts -> start[], cursor[]
//   k_mosaic_fill    one box per lane: its place in its cell (atomic cursor) -> sorted[]
//   k_mosaic_pass<0> one parallel round: a workgroup owns MS_THREADS boxes of one cell and stages the boxes of the 3 x 3
//                    cells around it through LDS, MS_CHUNK at a time; an undecided box becomes dropped when a preceding
//                    overlapping box is kept, kept when all of them are dropped.  Decided states are final, so the rounds
//                    update `status` in place with plain loads and stores; a stale read only delays a decision.
//   k_mosaic_list    a round from the third on: the boxes the round before left undecided are a list, one wave per listed
//                    box, its lanes side by side over the neighbours (after two rounds a twentieth of the boxes is left,
//                    spread over nearly every cell: staging a whole neighbourhood for a few lanes costs a full round)
//   k_mosaic_tail    one workgroup finishes whatever is still undecided (a chain of boxes that each depend on the one
//                    before needs as many rounds as it is long): workgroup barriers only, at most one pass per undecided box
//   k_mosaic_pass<1> the winner of every dropped box: the preceding overlapping kept box that comes first in the order
// No sort, no N x N table, no grid-wide barrier, no wait on another workgroup, no host read.
#include "../../include/dta_hip.h"
#include "common.h"

#include <cmath>

// the definition's operations one by one: (x2 - x1) * (y2 - y1), (area_i + area_j) - inter (hipcc contracts by default)
#pragma clang fp contract(off)

namespace dta {

constexpr int MS_THREADS = 256;
constexpr int MS_CHUNK = DTA_MOSAIC_CHUNK;               // boxes staged through LDS at a time
constexpr int MS_TAIL_THREADS = 1024;
constexpr int MS_MAX_SLICES = 64;
constexpr int MS_CELL_ROUNDS = 2;                        // rounds by cells in front of the rounds by list
constexpr int MS_LIST_BLOCKS = 2048;                     // of MS_THREADS threads: 32 waves on each of 256 CUs
constexpr int MS_LIST_UNROLL = 4;                        // neighbours per lane in flight
constexpr unsigned char MS_DROPPED = DTA_MOSAIC_DROPPED, MS_KEPT = DTA_MOSAIC_KEPT, MS_MASKED = DTA_MOSAIC_MASKED,
                        MS_REFUSED = DTA_MOSAIC_REFUSED, MS_UNDECIDED = DTA_MOSAIC_UNDECIDED;
static_assert(MS_CHUNK % MS_THREADS == 0, "a chunk is staged MS_THREADS boxes at a time");

struct MsGrid { float cell; int gx, gy; };

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.4028234663852886e38f; }   // false for NaN, +-inf

// j precedes i: the higher score, the lower index among equal scores
__device__ __forceinline__ bool precedes(float sj, int j, float si, int i) { return sj > si || (sj == si && j < i); }

__device__ __forceinline__ float box_area(const float4& b) { return mul_rounded(b.z - b.x, b.w - b.y); }

// j suppresses i: inter / (area_i + area_j - inter) > thr.  thr >= 0, so a pair with inter == 0 never does (0 / u is 0 or
// NaN) and the division is left to the pairs that do intersect.
__device__ __forceinline__ bool overlaps(const float4& a, float area_a, const float4& b, float area_b, float thr) {
  const float w = fmaxf(0.f, fminf(a.z, b.z) - fmaxf(a.x, b.x));
  const float h = fmaxf(0.f, fminf(a.w, b.w) - fmaxf(a.y, b.y));
  const float inter = mul_rounded(w, h);
  if (!(inter > 0.f)) return false;
  const float uni = (area_a + area_b) - inter;
  return __fdiv_rn(inter, uni) > thr;
}

// the cell of a centre: monotone in the centre, so two boxes whose centres are less than a cell side apart lie in the same
// or in adjacent cells (include/dta_hip.h: why the cell side is a little above max_side)
__device__ __forceinline__ int cell_index(float c, float extent, float cell, int g) {
  c = fminf(fmaxf(c, 0.f), extent);
  const int k = (int)floorf(__fdiv_rn(c, cell));
  return k < g - 1 ? k : g - 1;
}

__device__ __forceinline__ int clamp_to(float v, float hi) { return (int)fminf(fmaxf(v, 0.f), hi); }

__global__ __launch_bounds__(MS_THREADS) void k_mosaic_prep(const float* boxes, const float* scores, const int* window,
                                                            const int* origins, int n_windows, const unsigned char* mask,
                                                            int n, float height, float width, float max_side, MsGrid g,
                                                            unsigned char* status, int* winner, float* boxes_out,
                                                            int* pixel_out, int* cellof, int* count) {
  const int i = blockIdx.x * MS_THREADS + threadIdx.x;
  if (i >= n) return;
  float4 b = reinterpret_cast<const float4*>(boxes)[i];
  bool refused = false;
  if (window) {
    const int w = window[i];
    if (w < 0 || w >= n_windows) refused = true;
    else {
      const float ox = (float)origins[2 * w], oy = (float)origins[2 * w + 1];
      b.x += ox; b.y += oy; b.z += ox; b.w += oy;
    }
  }
  reinterpret_cast<float4*>(boxes_out)[i] = b;
  const bool fin = finite_f(b.x) && finite_f(b.y) && finite_f(b.z) && finite_f(b.w);
  const bool upright = fin && !(b.z < b.x) && !(b.w < b.y);
  int4 p = make_int4(0, 0, 0, 0);
  if (upright) p = make_int4(clamp_to(floorf(b.y), height), clamp_to(floorf(b.x), width), clamp_to(ceilf(b.w), height),
                             clamp_to(ceilf(b.z), width));
  reinterpret_cast<int4*>(pixel_out)[i] = p;
  refused = refused || !upright || !finite_f(scores[i]) || b.z - b.x > max_side || b.w - b.y > max_side;
  const bool masked = mask && mask[i] == 0;
  int c = -1;
  if (!refused && !masked) {
    const int cx = cell_index((b.x + b.z) * 0.5f, width, g.cell, g.gx);
    const int cy = cell_index((b.y + b.w) * 0.5f, height, g.cell, g.gy);
    c = cy * g.gx + cx;
    atomicAdd(count + c, 1);
  }
  cellof[i] = c;
  winner[i] = -1;                                          // (the winner pass visits the boxes that have a cell)
  status[i] = refused ? MS_REFUSED : masked ? MS_MASKED : MS_UNDECIDED;
}

// start[c] = the boxes in the cells below c, start[cells] = all of them; cursor[c] = start[c].  One workgroup.
__global__ __launch_bounds__(MS_TAIL_THREADS) void k_mosaic_scan(const int* count, int cells, int* start, int* cursor) {
  __shared__ int part[MS_TAIL_THREADS];
  const int tid = threadIdx.x;
  const int per = (cells + MS_TAIL_THREADS - 1) / MS_TAIL_THREADS;
  const int lo = tid * per < cells ? tid * per : cells, hi = lo + per < cells ? lo + per : cells;
  int sum = 0;
  for (int c = lo; c < hi; ++c) sum += count[c];
  part[tid] = sum;
  __syncthreads();
  for (int o = 1; o < MS_TAIL_THREADS; o <<= 1) {          // inclusive scan of the threads' sums
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = part[tid] - sum;
  for (int c = lo; c < hi; ++c) { start[c] = run; cursor[c] = run; run += count[c]; }
  if (tid == MS_TAIL_THREADS - 1) start[cells] = part[tid];
}

__global__ __launch_bounds__(MS_THREADS) void k_mosaic_fill(const int* cellof, int n, int* cursor, int* sorted) {
  const int i = blockIdx.x * MS_THREADS + threadIdx.x;
  if (i >= n) return;
  const int c = cellof[i];
  if (c >= 0) sorted[atomicAdd(cursor + c, 1)] = i;
}

// One round (WINNER = false) or the winner pass (WINNER = true).  blockIdx.x: the cell; blockIdx.y, stepping by gridDim.y:
// the slice of MS_THREADS boxes of that cell.  Only kept and undecided neighbours matter to a round and only kept ones to
// the winner pass; the test on the staged state is the same in every lane (one LDS address), so a dropped neighbour costs a
// branch and nothing else.
template <bool WINNER>
__global__ __launch_bounds__(MS_THREADS) void k_mosaic_pass(const float* tile, const float* scores, const int* start,
                                                            const int* sorted, MsGrid g, float thr, unsigned char* status,
                                                            int* winner, int* left, int* n_left) {
  __shared__ float4 sh_box[MS_CHUNK];
  __shared__ float sh_area[MS_CHUNK];
  __shared__ float sh_score[MS_CHUNK];
  __shared__ int sh_idx[MS_CHUNK];
  __shared__ unsigned char sh_state[MS_CHUNK];
  const int tid = threadIdx.x, cell = blockIdx.x;
  const int first = start[cell], mine = start[cell + 1] - first;
  const int cy = cell / g.gx, cx = cell - cy * g.gx;
  const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx < g.gx - 1 ? cx + 1 : cx;
  for (int base = blockIdx.y * MS_THREADS; base < mine; base += gridDim.y * MS_THREADS) {
    const bool have = base + tid < mine;
    int i = -1;
    unsigned char st = MS_KEPT;
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    float s = 0.f, area = 0.f;
    if (have) {
      i = sorted[first + base + tid];
      st = status[i];
      b = reinterpret_cast<const float4*>(tile)[i];
      s = scores[i];
      area = box_area(b);
    }
    const bool live = have && st == (WINNER ? MS_DROPPED : MS_UNDECIDED);
    if (!__syncthreads_or(live)) {                         // (the barrier also frees the LDS of the previous slice)
      if (WINNER && have) winner[i] = st == MS_KEPT ? i : -1;
      continue;
    }
    bool kept_seen = false, blocked = false;
    int best = -1;
    float best_score = 0.f;
    for (int ny = (cy > 0 ? cy - 1 : 0); ny <= (cy < g.gy - 1 ? cy + 1 : cy); ++ny) {
      const int lo = start[ny * g.gx + x0], hi = start[ny * g.gx + x1 + 1];    // three cells of a row lie side by side
      for (int from = lo; from < hi; from += MS_CHUNK) {
        const int cnt = hi - from < MS_CHUNK ? hi - from : MS_CHUNK;
        __syncthreads();                                   // the previous chunk has been read by every lane
        for (int m = tid; m < cnt; m += MS_THREADS) {
          const int j = sorted[from + m];
          const float4 q = reinterpret_cast<const float4*>(tile)[j];
          sh_box[m] = q; sh_area[m] = box_area(q); sh_score[m] = scores[j]; sh_idx[m] = j; sh_state[m] = status[j];
        }
        __syncthreads();
        if (live) {
          for (int m = 0; m < cnt; ++m) {
            const unsigned char sj = sh_state[m];
            if (WINNER ? sj != MS_KEPT : sj == MS_DROPPED) continue;
            const int j = sh_idx[m];
            const float score_j = sh_score[m];
            if (!precedes(score_j, j, s, i) || !overlaps(b, area, sh_box[m], sh_area[m], thr)) continue;
            if (WINNER) {
              if (best < 0 || precedes(score_j, j, best_score, best)) { best = j; best_score = score_j; }
            } else {
              kept_seen |= sj == MS_KEPT;
              blocked |= sj == MS_UNDECIDED;
            }
          }
        }
      }
    }
    if (WINNER) {
      if (have) winner[i] = st == MS_KEPT ? i : best;
    } else if (live && (kept_seen || !blocked)) {
      status[i] = kept_seen ? MS_DROPPED : MS_KEPT;
    } else if (live && left) {
      left[atomicAdd(n_left, 1)] = i;                      // for the rounds by list
    }
  }
}

// One wave decides box i, its lanes side by side over the boxes of the 3 x 3 cells, MS_LIST_UNROLL of them per lane in
// flight: 0 still undecided, else MS_KEPT + 1 or MS_DROPPED + 1, the same in every lane.
__device__ __forceinline__ int wave_decide(const float* tile, const float* scores, const int* start, const int* sorted,
                                           const int* cellof, const MsGrid& g, float thr, const unsigned char* status, int i) {
  const int lane = threadIdx.x & 63;
  const float4 b = reinterpret_cast<const float4*>(tile)[i];
  const float s = scores[i], area = box_area(b);
  const int cell = cellof[i], cy = cell / g.gx, cx = cell - cy * g.gx;
  const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx < g.gx - 1 ? cx + 1 : cx;
  bool kept_seen = false, blocked = false;
  for (int ny = (cy > 0 ? cy - 1 : 0); ny <= (cy < g.gy - 1 ? cy + 1 : cy); ++ny) {
    const int lo = start[ny * g.gx + x0], hi = start[ny * g.gx + x1 + 1];
    for (int from = lo; from < hi; from += 64 * MS_LIST_UNROLL) {
      int j[MS_LIST_UNROLL];
      unsigned char sj[MS_LIST_UNROLL];
      float score_j[MS_LIST_UNROLL];
#pragma unroll
      for (int k = 0; k < MS_LIST_UNROLL; ++k) j[k] = from + 64 * k + lane < hi ? sorted[from + 64 * k + lane] : -1;
#pragma unroll
      for (int k = 0; k < MS_LIST_UNROLL; ++k) sj[k] = j[k] >= 0 ? status[j[k]] : MS_DROPPED;
#pragma unroll
      for (int k = 0; k < MS_LIST_UNROLL; ++k) score_j[k] = sj[k] != MS_DROPPED ? scores[j[k]] : 0.f;
#pragma unroll
      for (int k = 0; k < MS_LIST_UNROLL; ++k) {
        if (sj[k] == MS_DROPPED || !precedes(score_j[k], j[k], s, i)) continue;
        const float4 q = reinterpret_cast<const float4*>(tile)[j[k]];
        if (!overlaps(b, area, q, box_area(q), thr)) continue;
        kept_seen |= sj[k] == MS_KEPT;
        blocked |= sj[k] == MS_UNDECIDED;
      }
      if (__any(kept_seen)) return MS_DROPPED + 1;
    }
  }
  return __any(blocked) ? 0 : MS_KEPT + 1;
}

// A round over the list the round before left: listed[0 .. *n_listed), one wave per box; what stays undecided goes to left[].
__global__ __launch_bounds__(MS_THREADS) void k_mosaic_list(const float* tile, const float* scores, const int* start,
                                                            const int* sorted, const int* cellof, MsGrid g, float thr,
                                                            unsigned char* status, const int* listed, const int* n_listed,
                                                            int* left, int* n_left) {
  const int total = *n_listed, waves = gridDim.x * (MS_THREADS / 64);
  for (int u = (blockIdx.x * MS_THREADS + threadIdx.x) >> 6; u < total; u += waves) {
    const int i = listed[u];
    const int decided = wave_decide(tile, scores, start, sorted, cellof, g, thr, status, i);
    if ((threadIdx.x & 63) == 0) {
      if (decided) status[i] = (unsigned char)(decided - 1);
      else left[atomicAdd(n_left, 1)] = i;
    }
  }
}

// a state another wave of this workgroup may have written in this launch: past the L1
__device__ __forceinline__ unsigned char state_now(const unsigned char* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup.  The undecided boxes are listed once; a pass decides every listed box whose preceding overlapping boxes
// are decided.  The first undecided box in the order is always among them, so every pass decides at least one and the
// loop ends after at most `total` passes; it ends early when a pass finds nothing left.
__global__ __launch_bounds__(MS_TAIL_THREADS) void k_mosaic_tail(const float* tile, const float* scores, const int* start,
                                                                 const int* sorted, const int* cellof, int n, MsGrid g,
                                                                 float thr, unsigned char* status, int* undecided) {
  __shared__ int total_sh;
  const int tid = threadIdx.x;
  if (tid == 0) total_sh = 0;
  __syncthreads();
  for (int i = tid; i < n; i += MS_TAIL_THREADS)
    if (status[i] == MS_UNDECIDED) undecided[atomicAdd(&total_sh, 1)] = i;
  __syncthreads();
  const int total = total_sh;
  for (int pass = 0; pass < total; ++pass) {
    bool left = false;
    for (int u = tid; u < total; u += MS_TAIL_THREADS) {
      const int i = undecided[u];
      if (state_now(status + i) != MS_UNDECIDED) continue;
      const float4 b = reinterpret_cast<const float4*>(tile)[i];
      const float s = scores[i], area = box_area(b);
      const int cell = cellof[i], cy = cell / g.gx, cx = cell - cy * g.gx;
      const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx < g.gx - 1 ? cx + 1 : cx;
      bool kept_seen = false, blocked = false;
      for (int ny = (cy > 0 ? cy - 1 : 0); ny <= (cy < g.gy - 1 ? cy + 1 : cy) && !kept_seen; ++ny) {
        const int lo = start[ny * g.gx + x0], hi = start[ny * g.gx + x1 + 1];
        for (int p = lo; p < hi; ++p) {
          const int j = sorted[p];
          const unsigned char sj = state_now(status + j);
          if (sj == MS_DROPPED || !precedes(scores[j], j, s, i)) continue;
          const float4 q = reinterpret_cast<const float4*>(tile)[j];
          if (!overlaps(b, area, q, box_area(q), thr)) continue;
          if (sj == MS_KEPT) { kept_seen = true; break; }
          blocked = true;
        }
      }
      if (kept_seen || !blocked) __hip_atomic_store(status + i, kept_seen ? MS_DROPPED : MS_KEPT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else left = true;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the write-through stores above have arrived before the barrier
    if (!__syncthreads_or(left)) break;
  }
}

}  // namespace dta

using namespace dta;

namespace {

constexpr long long MS_MAX_N = 1ll << 30;
constexpr int MS_MAX_EXTENT = 1 << 20;
constexpr long long MS_MAX_CELLS = 1ll << 20;

// The cell side and the grid of a call.  Two boxes can only overlap when their centres are less than max_side apart on
// either axis; the centre and its quotient by the side are float32 (each within 2^-24 of a value of at most 2^20, so the
// two together are off by less than a quarter pixel), hence a side of max_side plus a pixel (plus 1/1024 of it, which
// covers a side that rounded down to max_side).  Fewer cells than boxes / 1 (and at most 2^20): wider cells are as correct.
bool plan(const char* who, long long n, int height, int width, float max_side, MsGrid* g) {
  if (n < 1 || n > MS_MAX_N) { dta_set_error("%s: bad shape: n=%lld (1 .. 2^30)", who, n); return false; }
  if (height < 1 || width < 1 || height > MS_MAX_EXTENT || width > MS_MAX_EXTENT) {
    dta_set_error("%s: bad tile: height=%d width=%d (1 .. 2^20)", who, height, width);
    return false;
  }
  if (!(max_side > 0.f) || !(max_side <= (float)MS_MAX_EXTENT)) {
    dta_set_error("%s: max_side=%g is outside (0, 2^20]", who, (double)max_side);
    return false;
  }
  double cell = (double)max_side + (max_side > 1024.f ? (double)max_side / 1024.0 : 1.0);
  const long long cap = n < 64 ? 64 : n < MS_MAX_CELLS ? n : MS_MAX_CELLS;
  for (;;) {
    g->cell = (float)cell;
    g->gx = (int)std::floor((double)width / cell) + 1;
    g->gy = (int)std::floor((double)height / cell) + 1;
    if ((long long)g->gx * g->gy <= cap) return true;
    cell *= 2.0;
  }
}

struct MsLayout { size_t count, listed, start, cursor, sorted, cellof, undecided, list[2], total; };

MsLayout layout(long long n, const MsGrid& g) {
  const size_t cells = (size_t)g.gx * g.gy;
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  MsLayout l;
  l.count = 0;
  l.listed = l.count + up(cells * 4);                      // (behind count: one memset clears both)
  l.start = l.listed + up((DTA_MOSAIC_MAX_ROUNDS + 1) * 4);
  l.cursor = l.start + up((cells + 1) * 4);
  l.sorted = l.cursor + up(cells * 4);
  l.cellof = l.sorted + up((size_t)n * 4);
  l.undecided = l.cellof + up((size_t)n * 4);
  l.list[0] = l.undecided + up((size_t)n * 4);
  l.list[1] = l.list[0] + up((size_t)n * 4);
  l.total = l.list[1] + up((size_t)n * 4);
  return l;
}

}  // namespace

extern "C" size_t dta_mosaic_workspace_bytes(long long n, int height, int width, float max_side) {
  MsGrid g;
  if (!plan("dta_mosaic_workspace_bytes", n, height, width, max_side, &g)) return 0;
  return layout(n, g).total;
}

extern "C" int dta_mosaic_grid(long long n, int height, int width, float max_side, float* cell, int* gx, int* gy) {
  MsGrid g;
  if (!cell || !gx || !gy) { dta_set_error("dta_mosaic_grid: null argument"); return 1; }
  if (!plan("dta_mosaic_grid", n, height, width, max_side, &g)) return 1;
  *cell = g.cell; *gx = g.gx; *gy = g.gy;
  return 0;
}

extern "C" int dta_mosaic(const float* boxes, const float* scores, const int* window, const int* origins,
                          const unsigned char* mask, long long n, const dta_mosaic_options* opt, unsigned char* status_out,
                          int* winner_out, float* boxes_out, int* pixel_boxes_out, void* workspace, size_t workspace_bytes,
                          void* stream) {
  const char* who = "dta_mosaic";
  if (!boxes || !scores || !opt || !status_out || !winner_out || !boxes_out || !pixel_boxes_out || !workspace) {
    dta_set_error("%s: null argument", who);
    return 1;
  }
  if ((window != nullptr) != (origins != nullptr)) { dta_set_error("%s: window and origins go together", who); return 1; }
  if (window && (opt->n_windows < 1)) { dta_set_error("%s: n_windows=%d with a window table", who, opt->n_windows); return 1; }
  if (!(opt->iou_threshold >= 0.f) || !(opt->iou_threshold <= 1.f)) {
    dta_set_error("%s: iou_threshold=%g is outside [0, 1]", who, (double)opt->iou_threshold);
    return 1;
  }
  if (opt->rounds > DTA_MOSAIC_MAX_ROUNDS) { dta_set_error("%s: rounds=%d (at most %d)", who, opt->rounds, DTA_MOSAIC_MAX_ROUNDS); return 1; }
  MsGrid g;
  if (!plan(who, n, opt->height, opt->width, opt->max_side, &g)) return 1;
  const MsLayout l = layout(n, g);
  if (workspace_bytes < l.total || ((uintptr_t)workspace & 15)) {
    dta_set_error("%s: workspace of %zu bytes at %p: %zu bytes, 16-byte aligned, are needed", who, workspace_bytes, workspace, l.total);
    return 1;
  }
  if (((uintptr_t)boxes & 15) || ((uintptr_t)boxes_out & 15) || ((uintptr_t)pixel_boxes_out & 15)) {
    dta_set_error("%s: boxes, boxes_out and pixel_boxes_out must be 16-byte aligned", who);
    return 1;
  }
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* count = (int*)(ws + l.count); int* start = (int*)(ws + l.start); int* cursor = (int*)(ws + l.cursor);
  int* sorted = (int*)(ws + l.sorted); int* cellof = (int*)(ws + l.cellof); int* undecided = (int*)(ws + l.undecided);
  const int cells = g.gx * g.gy, N = (int)n;
  const unsigned per_box = (unsigned)((n + MS_THREADS - 1) / MS_THREADS);
  int* listed = (int*)(ws + l.listed);                     // listed[k]: how many boxes the k-th list holds
  int* list[2] = {(int*)(ws + l.list[0]), (int*)(ws + l.list[1])};
  if (hipMemsetAsync(count, 0, l.start - l.count, s) != hipSuccess) { dta_set_error("%s: hipMemsetAsync failed", who); return 1; }
  hipLaunchKernelGGL(k_mosaic_prep, dim3(per_box), dim3(MS_THREADS), 0, s, boxes, scores, window, origins, opt->n_windows, mask,
                     N, (float)opt->height, (float)opt->width, opt->max_side, g, status_out, winner_out, boxes_out, pixel_boxes_out,
                     cellof, count);
  DTA_CHECK_LAUNCH("k_mosaic_prep");
  hipLaunchKernelGGL(k_mosaic_scan, dim3(1), dim3(MS_TAIL_THREADS), 0, s, count, cells, start, cursor);
  DTA_CHECK_LAUNCH("k_mosaic_scan");
  hipLaunchKernelGGL(k_mosaic_fill, dim3(per_box), dim3(MS_THREADS), 0, s, cellof, N, cursor, sorted);
  DTA_CHECK_LAUNCH("k_mosaic_fill");
  // slices of a cell that run side by side: four times the average cell's, so that one crowded cell is not one workgroup's
  long long slices = (4 * n + (long long)MS_THREADS * cells - 1) / ((long long)MS_THREADS * cells);
  slices = slices < 1 ? 1 : slices > MS_MAX_SLICES ? MS_MAX_SLICES : slices;
  const dim3 grid((unsigned)cells, (unsigned)slices);
  const int rounds = opt->rounds < 0 ? DTA_MOSAIC_ROUNDS : opt->rounds;
  const int cell_rounds = rounds < MS_CELL_ROUNDS ? rounds : MS_CELL_ROUNDS;
  for (int r = 0; r < cell_rounds; ++r) {
    const bool lists = r == cell_rounds - 1 && rounds > cell_rounds;      // the last round by cells lists what it leaves
    hipLaunchKernelGGL(k_mosaic_pass<false>, grid, dim3(MS_THREADS), 0, s, boxes_out, scores, start, sorted, g, opt->iou_threshold,
                       status_out, (int*)nullptr, lists ? list[0] : (int*)nullptr, listed);
    DTA_CHECK_LAUNCH("k_mosaic_pass<round>");
  }
  const unsigned list_blocks = (unsigned)((n + 3) / 4 < MS_LIST_BLOCKS ? (n + 3) / 4 : MS_LIST_BLOCKS);
  for (int k = 0; k < rounds - cell_rounds; ++k) {
    hipLaunchKernelGGL(k_mosaic_list, dim3(list_blocks), dim3(MS_THREADS), 0, s, boxes_out, scores, start, sorted, cellof, g,
                       opt->iou_threshold, status_out, list[k & 1], listed + k, list[(k + 1) & 1], listed + k + 1);
    DTA_CHECK_LAUNCH("k_mosaic_list");
  }
  if (!opt->no_tail) {
    hipLaunchKernelGGL(k_mosaic_tail, dim3(1), dim3(MS_TAIL_THREADS), 0, s, boxes_out, scores, start, sorted, cellof, N, g,
                       opt->iou_threshold, status_out, undecided);
    DTA_CHECK_LAUNCH("k_mosaic_tail");
  }
  hipLaunchKernelGGL(k_mosaic_pass<true>, grid, dim3(MS_THREADS), 0, s, boxes_out, scores, start, sorted, g, opt->iou_threshold,
                     status_out, winner_out, (int*)nullptr, (int*)nullptr);
  DTA_CHECK_LAUNCH("k_mosaic_pass<winner>");
  return 0;
}
