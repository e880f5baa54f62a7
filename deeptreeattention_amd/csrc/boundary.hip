// Site boundary clip (reference abundance.py:24-35, create_prediction_shp.py:33-41, src/multinomial.py:16-19:
// gpd.clip(crowns, boundary), one geometry object per crown on the host).  deeptreeattention_amd/boundary.py holds the
// definition (contains_np, boxes_np, rasterise_np); these kernels equal it bit for bit: float64 throughout, every product
// and every difference rounded on its own, and the parity / any-edge reductions do not depend on the order of the edges.
//   k_boundary_points  one point per lane: the even-odd crossing rule over all edges
//   k_boundary_boxes   one box per lane: segment against filled rectangle (separating axes) over all edges, and the
//                      crossing rule for the corner (x0, y0) from the same products
//   k_boundary_raster  one workgroup per row and per BD_ROW_COLS columns: the edges that straddle the row's centre line are
//                      compacted into LDS first (ballot + prefix count, each wave into its own region), then every cell
//                      looks at those few: H * (E + W * k) edge tests instead of H * W * E
// The first two stage the edge table through LDS in chunks of BD_EDGE_CHUNK edges; every lane reads the same edge (one
// address: a broadcast, no bank conflicts).  No workspace, no atomics, no per-lane arrays.
#include "../../include/dta_hip.h"
#include "common.h"

#include <cmath>

// no fused multiply-add in this file: dx * (cy - ay) - dy * (cx - ax) and (px - ax) * dy < (py - ay) * dx are the
// definition's operations one by one (hipcc contracts by default; see mul_rounded in common.h)
#pragma clang fp contract(off)

namespace dta {

constexpr int BD_THREADS = 256;
constexpr int BD_WAVES = BD_THREADS / 64;
constexpr int BD_EDGE_CHUNK = DTA_BOUNDARY_EDGE_CHUNK;
constexpr int BD_MAX_EDGES = DTA_BOUNDARY_MAX_EDGES;
constexpr int BD_LANE_COLS = 4;                          // the raster kernel: cells per lane ...
constexpr int BD_ROW_COLS = BD_LANE_COLS * BD_THREADS;   // ... and columns of one row per workgroup
static_assert(BD_EDGE_CHUNK % BD_THREADS == 0, "the raster kernel looks at BD_EDGE_CHUNK / BD_THREADS edges per lane and chunk");

struct Bbox { double xmin, ymin, xmax, ymax; };

__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const double w = __shfl_xor(v, o); v = w < v ? w : v; }
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const double w = __shfl_xor(v, o); v = w > v ? w : v; }
  return v;
}

// The bounding box of all edge ends, the same in every thread of the workgroup.  red: BD_WAVES * 4 doubles of LDS.
// (Every workgroup reads the table once more for it; the table stays in L2.)
__device__ __forceinline__ Bbox table_bbox(const double* edges, int E, double* red) {
  const int tid = threadIdx.x;
  double xmin = INFINITY, ymin = INFINITY, xmax = -INFINITY, ymax = -INFINITY;
  for (int v = tid; v < 2 * E; v += BD_THREADS) {          // vertex v: the a end or the b end of edge v / 2
    const double x = edges[2 * (size_t)v], y = edges[2 * (size_t)v + 1];
    xmin = x < xmin ? x : xmin; xmax = x > xmax ? x : xmax;
    ymin = y < ymin ? y : ymin; ymax = y > ymax ? y : ymax;
  }
  xmin = wave_min_d(xmin); ymin = wave_min_d(ymin); xmax = wave_max_d(xmax); ymax = wave_max_d(ymax);
  if ((tid & 63) == 0) {
    double* r = red + 4 * (tid >> 6);
    r[0] = xmin; r[1] = ymin; r[2] = xmax; r[3] = ymax;
  }
  __syncthreads();
  Bbox b = {red[0], red[1], red[2], red[3]};
#pragma unroll
  for (int w = 1; w < BD_WAVES; ++w) {
    b.xmin = red[4 * w] < b.xmin ? red[4 * w] : b.xmin; b.ymin = red[4 * w + 1] < b.ymin ? red[4 * w + 1] : b.ymin;
    b.xmax = red[4 * w + 2] > b.xmax ? red[4 * w + 2] : b.xmax; b.ymax = red[4 * w + 3] > b.ymax ? red[4 * w + 3] : b.ymax;
  }
  return b;
}

// edges [base, base + cnt) -> sh, by all threads of the workgroup; a barrier on either side
__device__ __forceinline__ void stage_edges(const double* edges, int base, int cnt, double* sh) {
  __syncthreads();                                         // the previous chunk has been read by every lane
  const double* src = edges + 4 * (size_t)base;
  for (int k = threadIdx.x; k < 4 * cnt; k += BD_THREADS) sh[k] = src[k];
  __syncthreads();
}

// A point outside the table's bounding box below, above or to the right crosses nothing: no edge straddles a py outside
// [ymin, ymax), and for px > xmax every straddling edge has l >= r (dy > 0) or l <= r (dy < 0) by the monotonicity of
// rounding, so `left` is false.  To the LEFT of the box the count is even only as long as no product ties, which rounding
// does not promise: such a point takes the loop.
__device__ __forceinline__ bool point_may_cross(const Bbox& b, double px, double py) {
  return py >= b.ymin && py < b.ymax && px <= b.xmax;      // (false for a NaN py; a NaN px takes the loop and gets 0)
}

__global__ __launch_bounds__(BD_THREADS) void k_boundary_points(const double* edges, int E, double ox, double oy,
                                                                const double* points, long long n, unsigned char* out) {
  __shared__ double sh[4 * BD_EDGE_CHUNK];
  __shared__ double red[4 * BD_WAVES];
  const long long i = (long long)blockIdx.x * BD_THREADS + threadIdx.x;
  const bool have = i < n;
  double px = 0.0, py = 0.0;
  if (have) { px = points[2 * i] - ox; py = points[2 * i + 1] - oy; }
  const Bbox bb = table_bbox(edges, E, red);
  const bool live = have && point_may_cross(bb, px, py);
  bool in = false;
  for (int base = 0; base < E; base += BD_EDGE_CHUNK) {    // the same trips, the same barriers in every thread
    const int cnt = E - base < BD_EDGE_CHUNK ? E - base : BD_EDGE_CHUNK;
    stage_edges(edges, base, cnt, sh);
    if (live) {
      for (int m = 0; m < cnt; ++m) {
        const double ax = sh[4 * m], ay = sh[4 * m + 1], bx = sh[4 * m + 2], by = sh[4 * m + 3];
        const double dx = bx - ax, dy = by - ay;
        const double l = mul_rounded(px - ax, dy), r = mul_rounded(py - ay, dx);
        const bool straddle = (ay > py) != (by > py);
        const bool left = dy > 0.0 ? l < r : l > r;
        in ^= straddle & left;
      }
    }
  }
  if (have) out[i] = in ? 1 : 0;
}

__global__ __launch_bounds__(BD_THREADS) void k_boundary_boxes(const double* edges, int E, double ox, double oy,
                                                               const double* geo, const int* pix, double tx, double ta,
                                                               double ty, double te, long long n, unsigned char* out) {
  __shared__ double sh[4 * BD_EDGE_CHUNK];
  __shared__ double red[4 * BD_WAVES];
  const long long i = (long long)blockIdx.x * BD_THREADS + threadIdx.x;
  const bool have = i < n;
  double x0 = 0.0, y0 = 0.0, x1 = 0.0, y1 = 0.0;
  if (have) {
    if (pix) {                                             // boundary.py: geo_boxes
      const int* p = pix + 4 * i;
      const double ya = ty + mul_rounded((double)p[0], te), xa = tx + mul_rounded((double)p[1], ta);
      const double yb = ty + mul_rounded((double)p[2], te), xb = tx + mul_rounded((double)p[3], ta);
      x0 = xa < xb ? xa : xb; x1 = xa < xb ? xb : xa;
      y0 = ya < yb ? ya : yb; y1 = ya < yb ? yb : ya;
    } else {
      const double* g = geo + 4 * i;
      x0 = g[0]; y0 = g[1]; x1 = g[2]; y1 = g[3];
    }
    x0 -= ox; x1 -= ox; y0 -= oy; y1 -= oy;
  }
  const bool valid = have && finite_d(x0) && finite_d(y0) && finite_d(x1) && finite_d(y1) && !(x1 < x0) && !(y1 < y0);
  const Bbox bb = table_bbox(edges, E, red);
  // a box that misses the table's bounding box has every edge on the outer side of one of its sides: nothing touches; its
  // corner (x0, y0) may still take the crossing loop (point_may_cross)
  const bool meets = !(x1 < bb.xmin || x0 > bb.xmax || y1 < bb.ymin || y0 > bb.ymax);
  const bool live = valid && (meets || point_may_cross(bb, x0, y0));
  bool touch = false, in = false;
  for (int base = 0; base < E; base += BD_EDGE_CHUNK) {
    const int cnt = E - base < BD_EDGE_CHUNK ? E - base : BD_EDGE_CHUNK;
    stage_edges(edges, base, cnt, sh);
    if (live) {
      for (int m = 0; m < cnt; ++m) {
        const double ax = sh[4 * m], ay = sh[4 * m + 1], bx = sh[4 * m + 2], by = sh[4 * m + 3];
        const double dx = bx - ax, dy = by - ay;
        // & and | on purpose: with && and || hipcc branches around the later tests, and in a wave of unrelated boxes some
        // lane always needs them (measured: 3.25 ms with the branches, 2.88 ms without, profiles/README.md)
        const bool outer = ((ax < x0) & (bx < x0)) | ((ax > x1) & (bx > x1)) | ((ay < y0) & (by < y0)) | ((ay > y1) & (by > y1));
        const double p0 = mul_rounded(dx, y0 - ay), p1 = mul_rounded(dx, y1 - ay);
        const double q0 = mul_rounded(dy, x0 - ax), q1 = mul_rounded(dy, x1 - ax);
        const double s00 = p0 - q0, s10 = p0 - q1, s11 = p1 - q1, s01 = p1 - q0;      // corners (x0,y0) (x1,y0) (x1,y1) (x0,y1)
        const bool pos = (s00 > 0.0) & (s10 > 0.0) & (s11 > 0.0) & (s01 > 0.0);
        const bool neg = (s00 < 0.0) & (s10 < 0.0) & (s11 < 0.0) & (s01 < 0.0);
        touch |= !(outer | pos | neg);
        // the corner (x0, y0) as a point: l = (x0 - ax) * dy = q0, r = (y0 - ay) * dx = p0
        const bool straddle = (ay > y0) != (by > y0);
        const bool left = dy > 0.0 ? q0 < p0 : q0 > p0;
        in ^= straddle & left;
      }
    }
  }
  if (have) out[i] = touch ? 1 : (in ? 2 : 0);
}

// One compacted edge of a row: with py the row's centre line, r = (py - ay) * dx is the same for every cell, and for
// dy < 0 both sides change sign (exactly), so that `left` is l < r throughout: l = (px - ax) * dy.
struct RowEdge { double ax, dy, r; };

__global__ __launch_bounds__(BD_THREADS) void k_boundary_raster(const double* edges, int E, double ox, double oy, int H, int W,
                                                                int segs, double tx, double ta, double ty, double te,
                                                                unsigned char* out) {
  __shared__ RowEdge sh[BD_WAVES][BD_EDGE_CHUNK / BD_WAVES];     // wave w compacts into sh[w]
  __shared__ int kept[BD_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = blockIdx.x / segs, c0 = (blockIdx.x - row * segs) * BD_ROW_COLS + tid;
  const int cols = W - (c0 - tid) < BD_ROW_COLS ? W - (c0 - tid) : BD_ROW_COLS;      // of this workgroup: 1 .. BD_ROW_COLS
  const int trips = (cols + BD_THREADS - 1) / BD_THREADS;                            // the same in every thread
  const double py = (ty + mul_rounded((double)row + 0.5, te)) - oy;
  unsigned par = 0u;                                       // bit u: the cell at column c0 + u * BD_THREADS
  for (int base = 0; base < E; base += BD_EDGE_CHUNK) {
    int mine = 0;                                          // edges this wave has kept (the same in all its lanes)
#pragma unroll
    for (int j = 0; j < BD_EDGE_CHUNK / BD_THREADS; ++j) {
      const int k = base + j * BD_THREADS + tid;
      bool straddle = false;
      RowEdge e = {0.0, 0.0, 0.0};
      if (k < E) {
        const double* g = edges + 4 * (size_t)k;
        const double ax = g[0], ay = g[1], bx = g[2], by = g[3];
        straddle = (ay > py) != (by > py);
        const double dx = bx - ax, dy = by - ay;
        const double r = mul_rounded(py - ay, dx);
        e.ax = ax; e.dy = dy > 0.0 ? dy : -dy; e.r = dy > 0.0 ? r : -r;
      }
      const unsigned long long votes = __ballot(straddle);
      if (straddle) sh[wave][mine + __popcll(votes & ((1ull << lane) - 1ull))] = e;
      mine += __popcll(votes);
    }
    if (lane == 0) kept[wave] = mine;
    __syncthreads();
    for (int u = 0; u < trips; ++u) {
      const long long c = (long long)c0 + u * BD_THREADS;  // (past the row's end in the last trip: computed, not stored)
      const double px = (tx + mul_rounded((double)c + 0.5, ta)) - ox;
      bool in = false;
#pragma unroll
      for (int w = 0; w < BD_WAVES; ++w) {
        const int cnt = kept[w];
        for (int m = 0; m < cnt; ++m) {
          const RowEdge e = sh[w][m];
          in ^= mul_rounded(px - e.ax, e.dy) < e.r;
        }
      }
      par ^= (in ? 1u : 0u) << u;
    }
    __syncthreads();                                       // sh and kept are free for the next chunk
  }
  for (int u = 0; u < trips; ++u) {
    const long long c = (long long)c0 + u * BD_THREADS;
    if (c < W) out[(size_t)row * W + c] = (par >> u) & 1u;
  }
}

}  // namespace dta

using namespace dta;

namespace {

bool finite_h(double v) { return std::isfinite(v); }

bool bad_table(const char* who, const double* edges, int n_edges, const double* org) {
  if (!edges || !org) { dta_set_error("%s: null argument", who); return true; }
  if (n_edges < 3 || n_edges > BD_MAX_EDGES) {
    dta_set_error("%s: n_edges=%d is outside 3 .. %d", who, n_edges, BD_MAX_EDGES);
    return true;
  }
  if (!finite_h(org[0]) || !finite_h(org[1])) { dta_set_error("%s: org is not finite", who); return true; }
  return false;
}

bool bad_transform(const char* who, const double* t) {
  if (!finite_h(t[0]) || !finite_h(t[1]) || !finite_h(t[2]) || !finite_h(t[3])) {
    dta_set_error("%s: transform is not finite", who);
    return true;
  }
  if (t[1] == 0.0 || t[3] == 0.0) { dta_set_error("%s: transform has a=%g e=%g: a pixel size of 0", who, t[1], t[3]); return true; }
  return false;
}

bool bad_count(const char* who, long long n) {
  if (n < 1 || n > 0x7FFFFFFFll) { dta_set_error("%s: bad shape: n=%lld (1 .. 2^31 - 1)", who, n); return true; }
  return false;
}

}  // namespace

extern "C" int dta_boundary_points(const double* edges, int n_edges, const double* org, const double* points, long long n,
                                   unsigned char* out, void* stream) {
  const char* who = "dta_boundary_points";
  if (!points || !out) { dta_set_error("%s: null argument", who); return 1; }
  if (bad_table(who, edges, n_edges, org) || bad_count(who, n)) return 1;
  const unsigned grid = (unsigned)((n + BD_THREADS - 1) / BD_THREADS);
  hipLaunchKernelGGL(k_boundary_points, dim3(grid), dim3(BD_THREADS), 0, (hipStream_t)stream, edges, n_edges, org[0], org[1],
                     points, n, out);
  DTA_CHECK_LAUNCH("k_boundary_points");
  return 0;
}

extern "C" int dta_boundary_boxes(const double* edges, int n_edges, const double* org, const double* geo_boxes,
                                  const int* pixel_boxes, const double* transform, long long n, unsigned char* out,
                                  void* stream) {
  const char* who = "dta_boundary_boxes";
  if (!out) { dta_set_error("%s: null argument", who); return 1; }
  if (bad_table(who, edges, n_edges, org) || bad_count(who, n)) return 1;
  if ((geo_boxes != nullptr) == (pixel_boxes != nullptr)) {
    dta_set_error("%s: exactly one of geo_boxes and pixel_boxes must be given", who);
    return 1;
  }
  if (pixel_boxes && !transform) { dta_set_error("%s: pixel_boxes without a transform", who); return 1; }
  if (geo_boxes && transform) { dta_set_error("%s: geo_boxes with a transform", who); return 1; }
  if (transform && bad_transform(who, transform)) return 1;
  const double t[4] = {transform ? transform[0] : 0.0, transform ? transform[1] : 1.0, transform ? transform[2] : 0.0,
                       transform ? transform[3] : 1.0};
  const unsigned grid = (unsigned)((n + BD_THREADS - 1) / BD_THREADS);
  hipLaunchKernelGGL(k_boundary_boxes, dim3(grid), dim3(BD_THREADS), 0, (hipStream_t)stream, edges, n_edges, org[0], org[1],
                     geo_boxes, pixel_boxes, t[0], t[1], t[2], t[3], n, out);
  DTA_CHECK_LAUNCH("k_boundary_boxes");
  return 0;
}

extern "C" int dta_boundary_raster(const double* edges, int n_edges, const double* org, int height, int width,
                                   const double* transform, unsigned char* out, void* stream) {
  const char* who = "dta_boundary_raster";
  if (!transform || !out) { dta_set_error("%s: null argument", who); return 1; }
  if (bad_table(who, edges, n_edges, org)) return 1;
  if (height < 1 || width < 1) { dta_set_error("%s: bad raster: height=%d width=%d", who, height, width); return 1; }
  if ((long long)height * width > 0x7FFFFFFFll) {
    dta_set_error("%s: raster too large: height=%d x width=%d cells is over int32", who, height, width);
    return 1;
  }
  if (bad_transform(who, transform)) return 1;
  const int segs = (width + BD_ROW_COLS - 1) / BD_ROW_COLS;
  const long long grid = (long long)height * segs;         // <= height * width / BD_ROW_COLS + height
  if (grid > 0x7FFFFFFFll) { dta_set_error("%s: height=%d x width=%d: too many workgroups for one launch", who, height, width); return 1; }
  hipLaunchKernelGGL(k_boundary_raster, dim3((unsigned)grid), dim3(BD_THREADS), 0, (hipStream_t)stream, edges, n_edges, org[0],
                     org[1], height, width, segs, transform[0], transform[1], transform[2], transform[3], out);
  DTA_CHECK_LAUNCH("k_boundary_raster");
  return 0;
}
