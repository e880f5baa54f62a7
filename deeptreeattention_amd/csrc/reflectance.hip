// Reflectance cube to resident raster (reference src/Hyperspectral.py:152-219 `generate_raster`: drop the water-absorption
// bands, clip to a window, move the bands first; src/utils.py:36-57: drop 10 + 10 bands, min-max every pixel over its
// bands).  A NEON reflectance tile is pixel-interleaved, [rows][cols][426] int16; the resident raster of dense.hip is
// band-first (float32 planes) or chunk-first (bf16 [chunk][pixel][16]).  One pass:
//   k_reflectance_normalise  a strip of cube rows -> its rows of the normalised raster: band selection, column window,
//                            per-pixel min-max and the transpose, through LDS
// The arithmetic is k_raster_normalise's (dense.hip): both take it whole from common.h's minmax_* helpers, so the raster
// equals, bit for bit, the one dta_raster_normalise makes from the host-selected, host-transposed bands.
#include "../../include/dta_hip.h"
#include "kernels.h"

// the multiply and the add of the scaling are rounded SEPARATELY, as in k_raster_normalise
#pragma clang fp contract(off)

namespace dta {

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;
constexpr int RF_THREADS = 256;
constexpr int RF_STAGE_BYTES = 40 * 1024;   // the staged pixels of one workgroup: at least three workgroups per CU (160 KiB)
constexpr int RF_MIN_PIXELS = 8;            // 8 pixels x (1024 float32 bands + padding) fit RF_STAGE_BYTES
constexpr int RF_BATCH = 4;                 // 16-byte loads a lane has in flight while staging

struct ReflArgs {
  const unsigned char* strip;   // [rows][width_src][bands_src] of T
  const int* band_index;        // [C]
  void* out;
  size_t total;                 // bytes of the strip: no load may reach past it
  long long P;                  // out_height * cols: pixels of a plane / a chunk of the whole raster
  int bands_src, width_src, col0, cols, out_row0, C;
  int runs;                     // pixel runs per row: ceil(cols / np)
  int np, np_log2;              // pixels per workgroup (a power of two, 8 .. 256)
  int stride;                   // bytes from one pixel to the next in LDS: a multiple of 4 and an ODD number of dwords
  int sel_bytes;                // bytes of the band-offset table in front of the reduction scratch: 64 per chunk of 16 bands
};

// The LDS pixel stride: the pixel's bytes rounded up to whole dwords, one dword more when that count is even.  Lanes along
// pixels that read one band are then `stride / 4` dwords apart, an odd number: the 32 lanes of a ds_read group fall on 32
// different banks (213 dwords, int16 at 426 bands, is odd already; float32 at 426 bands becomes 427).
inline int lds_stride(int pixel_bytes) {
  int s = (pixel_bytes + 3) & ~3;
  if (((s >> 2) & 1) == 0) s += 4;
  return s;
}

// One workgroup takes a run of at most `np` consecutive pixels of one cube row.  Their bytes are one contiguous piece of
// the strip, b0 .. b0 + n * pixel_bytes, which starts wherever the pixel size puts it (int16 with an odd band count: on a
// 2-byte boundary only).  Staging therefore reads the ALIGNED 16-byte pieces that cover the run -- the strip starts on a
// 16-byte boundary, so the first piece starts inside it; a piece that would end past the strip (only the strip's very last
// one can) is read unit by unit up to the strip's end -- and scatters each piece to LDS in units of UNIT bytes, UNIT the
// largest of 4, 2, 1 that divides the pixel size: a unit never straddles two pixels, and it lands at
// pixel * stride + offset within the pixel.
//   then   lanes along pixels: lane (p, g), p = tid % np, g = tid / np, G = 256 / np groups
//   min/max  group g folds the chunks (of 16 bands) g, g + G, ... of pixel p; the G partial results meet in LDS (min and
//            max do not depend on the order, NaNs passed over as fminf / fmaxf do, so the bits are k_raster_normalise's).
//            The band offsets are read four at a time; the table's tail, past C, repeats band 0: folded again, no guard
//   write  the same chunks per group, so the bands of a lane are the same in both passes
//          TILES: 32 bytes per lane, np * 32 contiguous bytes per chunk;
//          float32: 4 bytes per lane and band, np * 4 contiguous bytes per band
template <typename T, int UNIT, bool TILES>
__global__ __launch_bounds__(RF_THREADS) void k_reflectance_normalise(ReflArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* s_off = reinterpret_cast<int*>(smem);                                 // [NC * 16] byte offset of band k within a pixel
  float* s_red = reinterpret_cast<float*>(smem + a.sel_bytes);               // [2][256] partial min, partial max
  unsigned char* s_pix = smem + a.sel_bytes + 2 * RF_THREADS * sizeof(float);
  const int tid = threadIdx.x;
  const int row = blockIdx.x / a.runs, run = blockIdx.x - row * a.runs;
  const int px0 = run << a.np_log2;
  const int n = a.cols - px0 < a.np ? a.cols - px0 : a.np;                    // the run ends at the row's cols
  const int PB = a.bands_src * (int)sizeof(T);

  const int C = a.C, NC = (C + 15) / 16;
  for (int k = tid; k < NC * 16; k += RF_THREADS) {
    int b = a.band_index[k < C ? k : 0];
    b = b < 0 ? 0 : (b >= a.bands_src ? a.bands_src - 1 : b);                 // never followed out of the pixel
    s_off[k] = b * (int)sizeof(T);
  }

  // ---- stage
  const size_t b0 = ((size_t)row * a.width_src + (size_t)(a.col0 + px0)) * (size_t)PB;
  const size_t A0 = b0 & ~(size_t)15;
  const int head = (int)(b0 - A0), nbytes = n * PB;
  const int pieces = (head + nbytes + 15) >> 4;
  for (int base = 0; base < pieces; base += RF_THREADS * RF_BATCH) {
    u32x4 v[RF_BATCH];
#pragma unroll
    for (int k = 0; k < RF_BATCH; ++k) {
      const int i = base + k * RF_THREADS + tid;
      v[k] = u32x4{0u, 0u, 0u, 0u};
      if (i < pieces) {
        const size_t A = A0 + ((size_t)i << 4);
        if (A + 16 <= a.total) {
          v[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.strip + A));     // read once
        } else {
#pragma unroll
          for (int j = 0; j < 16 / UNIT; ++j) {
            const size_t at = A + (size_t)(j * UNIT);
            if (at + UNIT <= a.total) {
              unsigned u;
              if (UNIT == 4) u = *reinterpret_cast<const unsigned*>(a.strip + at);
              else if (UNIT == 2) u = *reinterpret_cast<const unsigned short*>(a.strip + at);
              else u = a.strip[at];
              v[k][(j * UNIT) >> 2] |= u << (8 * ((j * UNIT) & 3));
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < RF_BATCH; ++k) {
      const int i = base + k * RF_THREADS + tid;
      if (i >= pieces) continue;
      int s = (i << 4) - head;                       // the piece's first byte, counted from the run's first byte
      int pix = 0, w = s;                            // s < 0: the bytes in front of the run (first piece only); w reaches 0 with s
      if (s >= 0) { pix = s / PB; w = s - pix * PB; }
#pragma unroll
      for (int j = 0; j < 16 / UNIT; ++j) {
        if (s >= 0 && s < nbytes) {
          unsigned char* dst = s_pix + pix * a.stride + w;
          const unsigned u = v[k][(j * UNIT) >> 2] >> (8 * ((j * UNIT) & 3));
          if (UNIT == 4) *reinterpret_cast<unsigned*>(dst) = u;
          else if (UNIT == 2) *reinterpret_cast<unsigned short*>(dst) = (unsigned short)u;
          else *dst = (unsigned char)u;
        }
        s += UNIT; w += UNIT;
        if (w == PB) { w = 0; ++pix; }
      }
    }
  }
  __syncthreads();

  // ---- min / max
  const int p = tid & (a.np - 1), g = tid >> a.np_log2, G = RF_THREADS >> a.np_log2;
  const unsigned char* mine = s_pix + p * a.stride;
  const bool live = p < n;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  if (live) {
    for (int ch = g; ch < NC; ch += G) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const i32x4 o = *reinterpret_cast<const i32x4*>(s_off + ch * 16 + q * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = to_f(*reinterpret_cast<const T*>(mine + o[e]));
          lo = fminf(lo, v); hi = fmaxf(hi, v);         // NaNs are passed over, as nanmin / nanmax do
        }
      }
    }
  }
  s_red[tid] = lo; s_red[RF_THREADS + tid] = hi;
  __syncthreads();
  if (!live) return;
  for (int k = 0; k < G; ++k) {
    lo = fminf(lo, s_red[(k << a.np_log2) + p]);
    hi = fmaxf(hi, s_red[RF_THREADS + (k << a.np_log2) + p]);
  }
  float s, m;
  minmax_scale(lo, hi, &s, &m);

  // ---- write
  const size_t pixel = (size_t)(a.out_row0 + row) * a.cols + (size_t)(px0 + p);
  if (!TILES) {
    float* out = reinterpret_cast<float*>(a.out) + pixel;
    for (int ch = g; ch < NC; ch += G) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const i32x4 o = *reinterpret_cast<const i32x4*>(s_off + ch * 16 + q * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = ch * 16 + q * 4 + e;
          if (c < C) out[(size_t)c * a.P] = minmax_apply(to_f(*reinterpret_cast<const T*>(mine + o[e])), s, m);
        }
      }
    }
  } else {
    unsigned short* out = reinterpret_cast<unsigned short*>(a.out);
    for (int ch = g; ch < NC; ch += G) {
      i32x4 o;      // the band offsets four at a time, as the min / max pass reads them: bands are asked for in ascending order
      minmax_store_chunk(out, (size_t)a.P, pixel, ch, C, s, m, [&](int c) {
        if ((c & 3) == 0) o = *reinterpret_cast<const i32x4*>(s_off + c);
        return to_f(*reinterpret_cast<const T*>(mine + o[c & 3]));
      });
    }
  }
}

template <typename T, int UNIT>
void launch_unit(const ReflArgs& a, bool tiles, unsigned groups, size_t lds, hipStream_t st) {
  if (tiles) hipLaunchKernelGGL((k_reflectance_normalise<T, UNIT, true>), dim3(groups), dim3(RF_THREADS), lds, st, a);
  else hipLaunchKernelGGL((k_reflectance_normalise<T, UNIT, false>), dim3(groups), dim3(RF_THREADS), lds, st, a);
}

}  // namespace

}  // namespace dta

using namespace dta;

extern "C" int dta_reflectance_normalise(const dta_reflectance_desc* d, const void* strip, const int* band_index, int bands,
                                         void* out, void* stream) {
  const char* who = "dta_reflectance_normalise";
  if (!d || !strip || !band_index || !out) {
    dta_set_error("%s: null argument: %s", who, !d ? "d" : !strip ? "strip" : !band_index ? "band_index" : "out");
    return 1;
  }
  if (d->bands_src < 1 || d->width_src < 1 || d->rows < 1 || d->cols < 1 || d->out_height < 1 || bands < 1) {
    dta_set_error("%s: bad shape: bands_src=%d width_src=%d rows=%d cols=%d out_height=%d bands=%d (all must be >= 1)", who,
                  d->bands_src, d->width_src, d->rows, d->cols, d->out_height, bands);
    return 1;
  }
  if (d->col0 < 0 || (long long)d->col0 + d->cols > d->width_src) {
    dta_set_error("%s: col0=%d cols=%d: the column window leaves width_src=%d", who, d->col0, d->cols, d->width_src);
    return 1;
  }
  if (d->out_row0 < 0 || (long long)d->out_row0 + d->rows > d->out_height) {
    dta_set_error("%s: out_row0=%d rows=%d: the strip leaves out_height=%d", who, d->out_row0, d->rows, d->out_height);
    return 1;
  }
  if (d->dtype != DTA_CROP_F32 && d->dtype != DTA_CROP_I16 && d->dtype != DTA_CROP_U8) {
    dta_set_error("%s: dtype=%d: DTA_CROP_F32, DTA_CROP_I16 or DTA_CROP_U8", who, d->dtype);
    return 1;
  }
  if ((long long)d->out_height * d->cols >= 0x80000000ll) {
    dta_set_error("%s: raster too large: out_height=%d x cols=%d is over int32", who, d->out_height, d->cols);
    return 1;
  }
  if (d->bands_src > DTA_REFLECTANCE_MAX_BANDS || bands > DTA_REFLECTANCE_MAX_BANDS) {
    dta_set_error("%s: bands_src=%d bands=%d: at most %d", who, d->bands_src, bands, DTA_REFLECTANCE_MAX_BANDS);
    return 1;
  }
  if ((uintptr_t)strip & 15) { dta_set_error("%s: strip is not 16-byte aligned", who); return 1; }
  if ((uintptr_t)out & 15) { dta_set_error("%s: out is not 16-byte aligned", who); return 1; }

  const int esize = d->dtype == DTA_CROP_F32 ? 4 : d->dtype == DTA_CROP_I16 ? 2 : 1;
  const int PB = d->bands_src * esize;
  ReflArgs a;
  a.strip = reinterpret_cast<const unsigned char*>(strip); a.band_index = band_index; a.out = out;
  a.total = (size_t)d->rows * (size_t)d->width_src * (size_t)PB;
  a.P = (long long)d->out_height * d->cols;
  a.bands_src = d->bands_src; a.width_src = d->width_src; a.col0 = d->col0; a.cols = d->cols; a.out_row0 = d->out_row0;
  a.C = bands;
  a.stride = lds_stride(PB);
  // pixels per workgroup: the largest power of two whose staged pixels fit RF_STAGE_BYTES (32 at 426 int16 bands, 27 KiB),
  // no more than the row needs (deeptreeattention_amd/reflectance.py: launch_plan is this rule)
  a.np_log2 = 8;
  while ((1 << a.np_log2) > RF_MIN_PIXELS && ((1 << a.np_log2) * a.stride > RF_STAGE_BYTES || (1 << (a.np_log2 - 1)) >= d->cols))
    --a.np_log2;
  // (developer library only: another number of pixels per workgroup, for same-box A/B runs; 16 to 64, inside the LDS limit)
  static const int np_env = dev_getenv("DTA_REFLECTANCE_PIXELS") ? atoi(dev_getenv("DTA_REFLECTANCE_PIXELS")) : 0;
  if ((np_env == 16 || np_env == 32 || np_env == 64) && np_env * a.stride <= 56 * 1024) a.np_log2 = np_env == 16 ? 4 : np_env == 32 ? 5 : 6;
  a.np = 1 << a.np_log2;
  a.runs = (d->cols + a.np - 1) / a.np;
  a.sel_bytes = ((bands + 15) / 16) * 64;
  const long long groups = (long long)d->rows * a.runs;
  if (groups > 0x7FFFFFFFll) { dta_set_error("%s: rows=%d x %d runs per row: too many workgroups for one launch", who, d->rows, a.runs); return 1; }
  const size_t lds = (size_t)a.sel_bytes + 2 * RF_THREADS * sizeof(float) + (size_t)a.np * a.stride;   // under 48 KiB
  const int unit = PB % 4 == 0 ? 4 : PB % 2 == 0 ? 2 : 1;
  const bool tiles = d->tiles != 0;
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == DTA_CROP_F32) launch_unit<float, 4>(a, tiles, (unsigned)groups, lds, st);
  else if (d->dtype == DTA_CROP_I16) {
    if (unit == 4) launch_unit<short, 4>(a, tiles, (unsigned)groups, lds, st);
    else launch_unit<short, 2>(a, tiles, (unsigned)groups, lds, st);
  } else {
    if (unit == 4) launch_unit<unsigned char, 4>(a, tiles, (unsigned)groups, lds, st);
    else if (unit == 2) launch_unit<unsigned char, 2>(a, tiles, (unsigned)groups, lds, st);
    else launch_unit<unsigned char, 1>(a, tiles, (unsigned)groups, lds, st);
  }
  DTA_CHECK_LAUNCH("k_reflectance_normalise");
  return 0;
}
