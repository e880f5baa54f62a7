// The resize body of the alive/dead kernels (dead.hip: k_rgb_crops, crown boxes of one raster; dead_train.hip: k_image_pool_batch,
// whole images of a resident pool): ONE statement of the tables, the row blend and the store loop, so that the two kernels
// give the same bits for the same pixels (deeptreeattention_amd/dead.py: crops_np is the definition).
//   uint8 plane(s) -> (u8 / 255 - mean) / std through a 256-entry table per channel -> bilinear (align_corners=False, no
//   antialias) to S x S.  The column and row tables (x0, x1, lx / y0, y1, ly) of an image are built once per workgroup in LDS,
//   a lane keeps its columns' entries in registers over all the rows it writes, 16-byte stores along the contiguous axis
//   where the line length allows it, element stores otherwise.
#pragma once
#include "common.h"

// the definition's float32 operations one by one (the weights and the four-term blend; the source position alone is one
// fused multiply-add, written as such)
#pragma clang fp contract(off)

namespace dta {

constexpr int RC_THREADS = 256;
constexpr int RC_MAX_CHANNELS = 4;
constexpr int RC_UNIT_ELEMS = 65536;                // a unit of work: about this many outputs (whole output rows of a crown) ...
constexpr int RC_MIN_UNIT_ELEMS = 8192;             // ... fewer, down to this, where the crowns are too few to give every workgroup one
constexpr int RC_NORM_BYTES = RC_MAX_CHANNELS * 256 * 4;

struct ColEntry { int x0; int dxc; float lx, omlx; };    // dxc: (x1 - x0) | (channel of the element << 1)
struct RowEntry { int a, b; float ly, omly; };           // a, b: offsets of the two source rows' first box column in a plane
static_assert(sizeof(ColEntry) == 16 && sizeof(RowEntry) == 16, "one ds_read_b128 each");

template <int FMT> struct Elem;
template <> struct Elem<FMT_F32> { typedef float T; __device__ static __forceinline__ float cvt(float v) { return v; } };
template <> struct Elem<FMT_BF16> { typedef unsigned short T; __device__ static __forceinline__ unsigned short cvt(float v) { return f2bf(v); } };
template <> struct Elem<FMT_F16> {
  typedef unsigned short T;
  __device__ static __forceinline__ unsigned short cvt(float v) { return __builtin_bit_cast(unsigned short, (_Float16)v); }
};

template <int FMT, int VW>
__device__ __forceinline__ void store_elems(void* out, size_t at, const float (&v)[VW]) {
  typedef typename Elem<FMT>::T T;
  T* p = (T*)out + at;
  if constexpr (VW == 1) {
    *p = Elem<FMT>::cvt(v[0]);
  } else if constexpr (FMT == FMT_F32) {
    static_assert(VW == 4, "");
    f32x4 q = {v[0], v[1], v[2], v[3]};
    *(f32x4*)p = q;
  } else {
    static_assert(VW == 8, "");
    u32x4 q;
    q.x = (unsigned)Elem<FMT>::cvt(v[0]) | ((unsigned)Elem<FMT>::cvt(v[1]) << 16);
    q.y = (unsigned)Elem<FMT>::cvt(v[2]) | ((unsigned)Elem<FMT>::cvt(v[3]) << 16);
    q.z = (unsigned)Elem<FMT>::cvt(v[4]) | ((unsigned)Elem<FMT>::cvt(v[5]) << 16);
    q.w = (unsigned)Elem<FMT>::cvt(v[6]) | ((unsigned)Elem<FMT>::cvt(v[7]) << 16);
    *(u32x4*)p = q;
  }
}

// [C][256]: ToTensor, then Normalize: two correctly rounded float32 divisions per byte value
__device__ __forceinline__ void norm_table(float* nt, int C, const float* mean, const float* stdv, int tid) {
  for (int k = tid; k < C * 256; k += RC_THREADS) nt[k] = ((float)(k & 255) / 255.f - mean[k >> 8]) / stdv[k >> 8];
}

// The two tables of an h x w source whose first sample lies at `base` of a plane with `stride` samples per row.
// flip: output column j takes the entry of column S - 1 - j (a reversal of the finished columns: no arithmetic changes).
// Every lane of the workgroup calls this; the caller puts a barrier on either side.
template <bool CL>
__device__ __forceinline__ void build_tables(RowEntry* rowt, ColEntry* colt, int S, int C, int L, int h, int w, int base,
                                             int stride, bool flip, int tid) {
  const float sy = (float)h / (float)S, sx = (float)w / (float)S;
  for (int i = tid; i < S; i += RC_THREADS) {
    float f = __builtin_fmaf(sy, (float)i + 0.5f, -0.5f);     // fused, as torch's CPU kernel has it (dead.py)
    f = f > 0.f ? f : 0.f;
    int y0 = (int)f;
    y0 = y0 < h - 1 ? y0 : h - 1;            // inside the source whatever the rounding
    const int y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1;
    const float ly = f - (float)y0;
    RowEntry e;
    e.a = base + y0 * stride; e.b = base + y1 * stride; e.ly = ly; e.omly = 1.f - ly;
    rowt[i] = e;
  }
  for (int k = tid; k < L; k += RC_THREADS) {
    const int j = CL ? k / C : k, ch = CL ? k - j * C : 0;
    float f = __builtin_fmaf(sx, (float)(flip ? S - 1 - j : j) + 0.5f, -0.5f);
    f = f > 0.f ? f : 0.f;
    int x0 = (int)f;
    x0 = x0 < w - 1 ? x0 : w - 1;
    const int x1 = x0 + 1 < w - 1 ? x0 + 1 : w - 1;
    const float lx = f - (float)x0;
    ColEntry e;
    e.x0 = x0; e.dxc = (x1 - x0) | (ch << 1); e.lx = lx; e.omlx = 1.f - lx;
    colt[k] = e;
  }
}

// (1 - lx) * p(c, y, x0) + lx * p(c, y, x1) for a lane's VW columns of the source row at offset `row` of a plane
template <int VW>
__device__ __forceinline__ void blend_row(float (&h)[VW], const ColEntry (&ce)[VW], int row, int p, const unsigned char* ras,
                                          size_t plane, const float* nt) {
#pragma unroll
  for (int q = 0; q < VW; ++q) {
    const int ch = p + (ce[q].dxc >> 1);
    const unsigned char* src = ras + (size_t)ch * plane + row;
    const float* t = nt + ch * 256;
    const int xa = ce[q].x0, xb = xa + (ce[q].dxc & 1);
    h[q] = ce[q].omlx * t[src[xa]] + ce[q].lx * t[src[xb]];
  }
}

// This lane's place in a workgroup that writes lines of L elements, VW per store: TPR lanes side by side on a line, RG lines
// at a time.
struct LanePlace { int VPL, TPR, RG, rg, jv0; };
__device__ __forceinline__ LanePlace lane_place(int L, int VW, int tid) {
  LanePlace z;
  z.VPL = L / VW;                                  // (VEC: L is a multiple of VW)
  z.TPR = z.VPL < RC_THREADS ? z.VPL : RC_THREADS;
  z.RG = RC_THREADS / z.TPR;
  z.rg = tid / z.TPR; z.jv0 = tid - z.rg * z.TPR;
  return z;
}

// Output rows [i0, i1) of one image, at element `obase` of out.  CL: channels_last memory ([n][i][j][c]: a line is one
// output row of S * C elements), otherwise [n][c][i][j] (a line is one output row of one channel).  ok false: zeros.
// No barrier in here: lanes that do not fill another line return at once.
template <int FMT, bool CL, int VW>
__device__ __forceinline__ void write_rows(bool ok, const unsigned char* ras, size_t plane, const float* nt, const RowEntry* rowt,
                                           const ColEntry* colt, void* out, size_t obase, int i0, int i1, int S, int L, int planes,
                                           const LanePlace& z) {
  if (z.rg >= z.RG) return;
  // this lane's rows of the unit: consecutive ones, so that a blended source row serves every output row between it and
  // its neighbour (an upsampled crown reads each source sample once per lane, not four per output)
  const int chunk = (i1 - i0 + z.RG - 1) / z.RG;
  const int ia = i0 + z.rg * chunk;
  const int ib = ia + chunk < i1 ? ia + chunk : i1;
  for (int jv = z.jv0; jv < z.VPL; jv += z.TPR) {
    ColEntry ce[VW];
    if (ok) {
#pragma unroll
      for (int q = 0; q < VW; ++q) ce[q] = colt[jv * VW + q];
    }
    for (int p = 0; p < planes; ++p) {
      int ca = -1, cb = -1;                      // the source rows ha / hb hold (offsets are >= 0)
      float ha[VW], hb[VW];
#pragma unroll
      for (int q = 0; q < VW; ++q) ha[q] = hb[q] = 0.f;
      for (int i = ia; i < ib; ++i) {
        float v[VW];
        if (ok) {
          const RowEntry re = rowt[i];
          if (re.a != ca) {                      // the rows only move down: the new upper row is the old lower one, or new
            if (re.a == cb) {
#pragma unroll
              for (int q = 0; q < VW; ++q) ha[q] = hb[q];
            } else {
              blend_row<VW>(ha, ce, re.a, p, ras, plane, nt);
            }
            ca = re.a;
          }
          if (re.b != cb) {
            if (re.b == ca) {                    // y1 == y0: the source's last row (or its only one)
#pragma unroll
              for (int q = 0; q < VW; ++q) hb[q] = ha[q];
            } else {
              blend_row<VW>(hb, ce, re.b, p, ras, plane, nt);
            }
            cb = re.b;
          }
#pragma unroll
          for (int q = 0; q < VW; ++q) v[q] = re.omly * ha[q] + re.ly * hb[q];
        } else {
#pragma unroll
          for (int q = 0; q < VW; ++q) v[q] = 0.f;
        }
        const size_t line = CL ? (size_t)i : (size_t)p * S + i;
        store_elems<FMT, VW>(out, obase + line * L + (size_t)jv * VW, v);
      }
    }
  }
}

// The launch plan both entries use (deeptreeattention_amd/dead.py: launch_plan is this rule): output rows per unit of work.
static inline int rgb_crops_rows_per_unit(long long n, int size, int channels, int max_groups) {
  const int row_elems = size * channels;
  int rb = (RC_UNIT_ELEMS + row_elems - 1) / row_elems;
  rb = rb < size ? rb : size;
  if (n * ((size + rb - 1) / rb) < max_groups) {
    const int want = (int)((max_groups + n - 1) / n);           // units per crown that would fill the launch
    int least = (RC_MIN_UNIT_ELEMS + row_elems - 1) / row_elems;
    least = least < rb ? least : rb;
    const int fill = (size + want - 1) / want;
    rb = fill > least ? fill : least;
  }
  return rb;
}

}  // namespace dta
