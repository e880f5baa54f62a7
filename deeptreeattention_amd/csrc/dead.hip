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
#include "rgb_crops_dev.h"       // the tables, the row blend and the store loop: shared with dead_train.hip's pool batches

// the definition's float32 operations one by one (the weights and the four-term blend; the source position alone is one
// fused multiply-add, written as such)
#pragma clang fp contract(off)

namespace dta {

constexpr int RC_MAX_GROUPS = DTA_RGB_CROPS_MAX_GROUPS;
constexpr int RC_MAX_SIZE = DTA_RGB_CROPS_MAX_SIZE;

struct CropArgs {
  const unsigned char* ras; int C, H, W;
  const int* boxes; long long n;
  int S, pad;
  float mean[RC_MAX_CHANNELS], stdv[RC_MAX_CHANNELS];
  void* out; unsigned char* valid;
  int rb, units;                   // output rows per unit; units per crown
  long long total;                 // n * units
};

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
  norm_table(nt, C, a.mean, a.stdv, tid);
  const LanePlace z = lane_place(L, VW, tid);
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
      if (ok)                                      // 0 <= r0 < r1 <= H, 0 <= c0 < c1 <= W; the base is < H * W <= 2^31 - 1
        build_tables<CL>(rowt, colt, S, C, L, (int)(r1 - r0), (int)(c1 - c0), (int)r0 * W + (int)c0, W, false, tid);
      __syncthreads();                             // (the first time round also: the normalisation table is complete)
      if (unit == 0 && tid == 0) a.valid[n] = ok ? 1 : 0;      // the crown's first unit belongs to one workgroup
    }
    const int i0 = unit * a.rb;
    const int i1 = i0 + a.rb < S ? i0 + a.rb : S;
    write_rows<FMT, CL, VW>(ok, a.ras, plane, nt, rowt, colt, a.out, (size_t)n * crown_elems, i0, i1, S, L, planes, z);
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
  a.rb = rgb_crops_rows_per_unit(n, size, channels, RC_MAX_GROUPS);
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
