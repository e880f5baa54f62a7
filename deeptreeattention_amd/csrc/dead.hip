// Alive/dead crown filter (reference src/models/dead.py: utm_dataset.__getitem__ reads every crown's RGB box plus one metre
// with rasterio and runs ToTensor, Normalize and Resize([224, 224]) on a CPU worker; predict_dead turns the classifier's
// logits into label = argmax, score = max of softmax(sigmoid(logits))).  deeptreeattention_amd/dead.py holds the definition
// (crops_np, head_np); the classifier between the two kernels is a stock network torch runs.
//   k_rgb_crops   box + pad, clipped -> (u8 / 255 - mean) / std -> bilinear (align_corners=False, no antialias) to S x S, for
//                 all crowns of a call.  A pure store stream (S * S * C outputs per crown from a source box of a few
//                 kilobytes): at most RC_MAX_GROUPS workgroups, each with a contiguous share of the output; the column
//                 and row tables (x0, x1, lx / y0, y1, ly) of a crown are built once per workgroup in LDS, a lane keeps its
//                 columns' entries in registers over all the rows it writes, the normalised value of every byte value
//                 comes from a 256-entry table per channel (no division per sample), 16-byte stores along the contiguous
//                 axis where the line length allows it, element stores otherwise.
//   k_dead_head   one thread per crown of a batch: sigmoid, softmax over the two classes, max and argmax (a tie: 0).
#include "../../include/dta_hip.h"
#include "common.h"

// the definition's float32 operations one by one (the weights and the four-term blend; the source position alone is one
// fused multiply-add, written as such)
#pragma clang fp contract(off)

namespace dta {

constexpr int RC_THREADS = 256;
constexpr int RC_MAX_GROUPS = DTA_RGB_CROPS_MAX_GROUPS;
constexpr int RC_MAX_SIZE = DTA_RGB_CROPS_MAX_SIZE;
constexpr int RC_MAX_CHANNELS = 4;
constexpr int RC_UNIT_ELEMS = 65536;                // a unit of work: about this many outputs (whole output rows of a crown) ...
constexpr int RC_MIN_UNIT_ELEMS = 8192;             // ... fewer, down to this, where the crowns are too few to give every workgroup one
constexpr int RC_NORM_BYTES = RC_MAX_CHANNELS * 256 * 4;

struct ColEntry { int x0; int dxc; float lx, omlx; };    // dxc: (x1 - x0) | (channel of the element << 1)
struct RowEntry { int a, b; float ly, omly; };           // a, b: offsets of the two source rows' first box column in a plane
static_assert(sizeof(ColEntry) == 16 && sizeof(RowEntry) == 16, "one ds_read_b128 each");

struct CropArgs {
  const unsigned char* ras; int C, H, W;
  const int* boxes; long long n;
  int S, pad;
  float mean[RC_MAX_CHANNELS], stdv[RC_MAX_CHANNELS];
  void* out; unsigned char* valid;
  int rb, units;                   // output rows per unit; units per crown
  long long total;                 // n * units
};

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

// CL: channels_last memory ([n][i][j][c]: a line is one output row of S * C elements), otherwise [n][c][i][j] (a line is
// one output row of one channel).  VEC: 16-byte stores; the host picks it only where every line starts 16-byte aligned.
template <int FMT, bool CL, bool VEC>
__global__ __launch_bounds__(RC_THREADS) void k_rgb_crops(CropArgs a) {
  constexpr int VW = VEC ? 16 / (int)sizeof(typename Elem<FMT>::T) : 1;
  extern __shared__ __align__(16) unsigned char smem[];
  float* nt = (float*)smem;                                                    // [C][256] normalised byte values
  RowEntry* rowt = (RowEntry*)(smem + RC_NORM_BYTES);                          // [S]
  ColEntry* colt = (ColEntry*)(smem + RC_NORM_BYTES + (size_t)a.S * sizeof(RowEntry));   // [L]
  const int tid = threadIdx.x;
  const int S = a.S, C = a.C, H = a.H, W = a.W;
  const int L = CL ? S * C : S;                    // elements of a line
  const int planes = CL ? 1 : C;                   // lines per output row
  const size_t plane = (size_t)H * W;
  const size_t crown_elems = (size_t)C * S * S;
  for (int k = tid; k < C * 256; k += RC_THREADS)  // ToTensor, then Normalize: two correctly rounded float32 divisions
    nt[k] = ((float)(k & 255) / 255.f - a.mean[k >> 8]) / a.stdv[k >> 8];
  // this lane's place: TPR lanes side by side on a line, RG lines at a time
  const int VPL = L / VW;                          // (VEC: L is a multiple of VW)
  const int TPR = VPL < RC_THREADS ? VPL : RC_THREADS;
  const int RG = RC_THREADS / TPR;
  const int rg = tid / TPR, jv0 = tid - rg * TPR;
  const long long u0 = a.total * (long long)blockIdx.x / (long long)gridDim.x;
  const long long u1 = a.total * ((long long)blockIdx.x + 1) / (long long)gridDim.x;
  long long crown = -1;
  bool ok = false;
  for (long long u = u0; u < u1; ++u) {            // (the same for every thread of the workgroup)
    const long long n = u / a.units;
    const int unit = (int)(u - n * a.units);
    if (n != crown) {
      crown = n;
      __syncthreads();                             // nobody reads the previous crown's tables any more
      const int* b = a.boxes + 4 * n;
      const int b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
      long long r0 = (long long)b0 - a.pad, c0 = (long long)b1 - a.pad, r1 = (long long)b2 + a.pad, c1 = (long long)b3 + a.pad;
      r0 = r0 > 0 ? r0 : 0; c0 = c0 > 0 ? c0 : 0;
      r1 = r1 < H ? r1 : H; c1 = c1 < W ? c1 : W;
      ok = b2 > b0 && b3 > b1 && r1 > r0 && c1 > c0;
      if (ok) {                                    // 0 <= r0 < r1 <= H, 0 <= c0 < c1 <= W
        const int h = (int)(r1 - r0), w = (int)(c1 - c0);
        const int base = (int)r0 * W + (int)c0;    // < H * W <= 2^31 - 1
        const float sy = (float)h / (float)S, sx = (float)w / (float)S;
        for (int i = tid; i < S; i += RC_THREADS) {
          float f = __builtin_fmaf(sy, (float)i + 0.5f, -0.5f);     // fused, as torch's CPU kernel has it (dead.py)
          f = f > 0.f ? f : 0.f;
          int y0 = (int)f;
          y0 = y0 < h - 1 ? y0 : h - 1;            // inside the clipped box whatever the rounding
          const int y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1;
          const float ly = f - (float)y0;
          RowEntry e;
          e.a = base + y0 * W; e.b = base + y1 * W; e.ly = ly; e.omly = 1.f - ly;
          rowt[i] = e;
        }
        for (int k = tid; k < L; k += RC_THREADS) {
          const int j = CL ? k / C : k, ch = CL ? k - j * C : 0;
          float f = __builtin_fmaf(sx, (float)j + 0.5f, -0.5f);
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
      __syncthreads();                             // (the first time round also: the normalisation table is complete)
      if (unit == 0 && tid == 0) a.valid[n] = ok ? 1 : 0;      // the crown's first unit belongs to one workgroup
    }
    const int i0 = unit * a.rb;
    const int i1 = i0 + a.rb < S ? i0 + a.rb : S;
    const size_t obase = (size_t)n * crown_elems;
    if (rg >= RG) continue;                        // lanes that do not fill another line (no barrier depends on them below)
    // this lane's rows of the unit: consecutive ones, so that a blended source row serves every output row between it and
    // its neighbour (an upsampled crown reads each source sample once per lane, not four per output)
    const int chunk = (i1 - i0 + RG - 1) / RG;
    const int ia = i0 + rg * chunk;
    const int ib = ia + chunk < i1 ? ia + chunk : i1;
    for (int jv = jv0; jv < VPL; jv += TPR) {
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
                blend_row<VW>(ha, ce, re.a, p, a.ras, plane, nt);
              }
              ca = re.a;
            }
            if (re.b != cb) {
              if (re.b == ca) {                    // y1 == y0: the box's last row (or its only one)
#pragma unroll
                for (int q = 0; q < VW; ++q) hb[q] = ha[q];
              } else {
                blend_row<VW>(hb, ce, re.b, p, a.ras, plane, nt);
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
          store_elems<FMT, VW>(a.out, obase + line * L + (size_t)jv * VW, v);
        }
      }
    }
  }
}

struct HeadArgs { const void* logits; long long rows, offset; long long* label; float* score; };

template <int FMT>
__global__ __launch_bounds__(256) void k_dead_head(HeadArgs a) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.rows) return;
  const float l0 = ld_fmt(a.logits, (size_t)(2 * r), FMT), l1 = ld_fmt(a.logits, (size_t)(2 * r + 1), FMT);
  const float s0 = 1.f / (1.f + expf(-l0)), s1 = 1.f / (1.f + expf(-l1));
  const float m = s0 > s1 ? s0 : s1;
  const float e0 = expf(s0 - m), e1 = expf(s1 - m);
  const float sum = e0 + e1;
  const float p0 = e0 / sum, p1 = e1 / sum;
  a.label[a.offset + r] = p1 > p0 ? 1 : 0;         // a tie (and a NaN): 0, as np.argmax
  a.score[a.offset + r] = p1 > p0 ? p1 : p0;
}

template <int FMT>
static void launch_crops(const CropArgs& a, int cl, bool vec, unsigned groups, size_t lds, hipStream_t st) {
  if (cl) {
    if (vec) hipLaunchKernelGGL((k_rgb_crops<FMT, true, true>), dim3(groups), dim3(RC_THREADS), lds, st, a);
    else hipLaunchKernelGGL((k_rgb_crops<FMT, true, false>), dim3(groups), dim3(RC_THREADS), lds, st, a);
  } else {
    if (vec) hipLaunchKernelGGL((k_rgb_crops<FMT, false, true>), dim3(groups), dim3(RC_THREADS), lds, st, a);
    else hipLaunchKernelGGL((k_rgb_crops<FMT, false, false>), dim3(groups), dim3(RC_THREADS), lds, st, a);
  }
}

}  // namespace dta

using namespace dta;

extern "C" int dta_rgb_crops(const unsigned char* raster, int channels, int height, int width, const int* boxes, long long n,
                             int size, int pad, const float* mean, const float* std, int dtype, int channels_last, void* out,
                             unsigned char* out_valid, void* stream) {
  const char* who = "dta_rgb_crops";
  if (!raster || !boxes || !mean || !std || !out || !out_valid) { dta_set_error("%s: null argument", who); return 1; }
  if (n < 1 || n > 0x7FFFFFFFll) { dta_set_error("%s: bad shape: n=%lld", who, n); return 1; }
  if (channels < 1 || channels > RC_MAX_CHANNELS) { dta_set_error("%s: channels=%d: 1 to %d", who, channels, RC_MAX_CHANNELS); return 1; }
  if (height < 1 || width < 1) { dta_set_error("%s: bad raster: height=%d width=%d", who, height, width); return 1; }
  if ((long long)channels * height * width > 0x7FFFFFFFll) {
    dta_set_error("%s: raster too large: channels=%d x height=%d x width=%d is over int32", who, channels, height, width);
    return 1;
  }
  if (size < 1 || size > RC_MAX_SIZE) { dta_set_error("%s: size=%d: 1 to %d", who, size, RC_MAX_SIZE); return 1; }
  if (pad < 0) { dta_set_error("%s: pad=%d must be >= 0", who, pad); return 1; }
  if (dtype != DTA_ELEM_F32 && dtype != DTA_ELEM_BF16 && dtype != DTA_ELEM_F16) {
    dta_set_error("%s: dtype=%d: DTA_ELEM_F32, DTA_ELEM_BF16 or DTA_ELEM_F16", who, dtype);
    return 1;
  }
  for (int c = 0; c < channels; ++c) {
    if (!(mean[c] == mean[c]) || !(std[c] == std[c]) || std[c] == 0.f) {
      dta_set_error("%s: channel %d: mean=%g std=%g (std must not be 0, neither may be NaN)", who, c, (double)mean[c], (double)std[c]);
      return 1;
    }
  }
  const int bytes = dtype == DTA_ELEM_F32 ? 4 : 2;
  if ((uintptr_t)out % bytes) { dta_set_error("%s: out is not aligned to its element size", who); return 1; }
  CropArgs a;
  a.ras = raster; a.C = channels; a.H = height; a.W = width; a.boxes = boxes; a.n = n; a.S = size; a.pad = pad;
  for (int c = 0; c < RC_MAX_CHANNELS; ++c) { a.mean[c] = c < channels ? mean[c] : 0.f; a.stdv[c] = c < channels ? std[c] : 1.f; }
  a.out = out; a.valid = out_valid;
  const int row_elems = size * channels;
  int rb = (RC_UNIT_ELEMS + row_elems - 1) / row_elems;
  rb = rb < size ? rb : size;
  if (n * ((size + rb - 1) / rb) < RC_MAX_GROUPS) {             // deeptreeattention_amd/dead.py: launch_plan is this rule
    const int want = (int)((RC_MAX_GROUPS + n - 1) / n);        // units per crown that would fill the launch
    int least = (RC_MIN_UNIT_ELEMS + row_elems - 1) / row_elems;
    least = least < rb ? least : rb;
    const int fill = (size + want - 1) / want;
    rb = fill > least ? fill : least;
  }
  a.rb = rb;
  a.units = (size + a.rb - 1) / a.rb;
  a.total = n * a.units;
  const int line = channels_last ? row_elems : size, vw = 16 / bytes;
  const bool vec = line % vw == 0 && (uintptr_t)out % 16 == 0;      // every line then starts on a 16-byte boundary
  // (developer library only: fewer workgroups for same-box A/B runs of the store stream; never more than the cap)
  static const int cap_env = dev_getenv("DTA_RGB_CROPS_GROUPS") ? atoi(dev_getenv("DTA_RGB_CROPS_GROUPS")) : 0;
  const long long cap = cap_env >= 1 && cap_env < RC_MAX_GROUPS ? cap_env : RC_MAX_GROUPS;
  const unsigned groups = (unsigned)(a.total < cap ? a.total : cap);
  const size_t lds = RC_NORM_BYTES + (size_t)size * sizeof(RowEntry) + (size_t)line * sizeof(ColEntry);   // at most 44 KiB at size 512, 4 channels
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DTA_ELEM_F32) launch_crops<FMT_F32>(a, channels_last, vec, groups, lds, st);
  else if (dtype == DTA_ELEM_BF16) launch_crops<FMT_BF16>(a, channels_last, vec, groups, lds, st);
  else launch_crops<FMT_F16>(a, channels_last, vec, groups, lds, st);
  DTA_CHECK_LAUNCH("k_rgb_crops");
  return 0;
}

extern "C" int dta_dead_head(const void* logits, int dtype, long long rows, long long offset, long long* out_label,
                             float* out_score, void* stream) {
  const char* who = "dta_dead_head";
  if (!logits || !out_label || !out_score) { dta_set_error("%s: null argument", who); return 1; }
  if (rows < 1 || rows > (0x7FFFFFFFll << 8)) { dta_set_error("%s: bad shape: rows=%lld", who, rows); return 1; }
  if (offset < 0) { dta_set_error("%s: offset=%lld must be >= 0", who, offset); return 1; }
  if (dtype != DTA_ELEM_F32 && dtype != DTA_ELEM_BF16 && dtype != DTA_ELEM_F16) {
    dta_set_error("%s: dtype=%d: DTA_ELEM_F32, DTA_ELEM_BF16 or DTA_ELEM_F16", who, dtype);
    return 1;
  }
  HeadArgs a;
  a.logits = logits; a.rows = rows; a.offset = offset; a.label = out_label; a.score = out_score;
  const unsigned groups = (unsigned)((rows + 255) / 256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DTA_ELEM_F32) hipLaunchKernelGGL(k_dead_head<FMT_F32>, dim3(groups), dim3(256), 0, st, a);
  else if (dtype == DTA_ELEM_BF16) hipLaunchKernelGGL(k_dead_head<FMT_BF16>, dim3(groups), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_dead_head<FMT_F16>, dim3(groups), dim3(256), 0, st, a);
  DTA_CHECK_LAUNCH("k_dead_head");
  return 0;
}
