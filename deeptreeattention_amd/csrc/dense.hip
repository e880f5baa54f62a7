// Dense per-pixel window prediction over a hyperspectral raster (reference src/patches.py:50-83 `bounds_to_pixel`: one
// 11x11 window per pixel of a crown box, read boundless; src/main.py:165-178).  The reference's preprocessing is per
// pixel position (drop bands, min-max over the bands of that pixel, src/utils.py:36-57) and an SxS window resized to SxS
// with NEAREST is the identity, so the preprocessed window IS the window of the preprocessed raster:
//   k_raster_normalise  the raw raster once -> the resident normalised raster (float32 planes, or bf16 channel chunks)
//   k_gather_windows    N window origins -> the float32 NCHW batch / the first conv's bf16 tiles (pure copies, zero fill)
//   k_crown_reduce      per-window softmax rows, grouped by crown -> mean vector, its top-2 and the window count
// All three are bandwidth-bound copies or short reductions: no atomics, fixed summation order, bit-identical reruns.
#include "../../include/dta_hip.h"
#include "kernels.h"

// k_raster_normalise repeats k_preprocess_crops' arithmetic (preprocess.hip) through the same mul_rounded / to_f
// (common.h): the multiply and the add of the scaling are rounded SEPARATELY, as NumPy's `X *= scale; X += min` does
#pragma clang fp contract(off)

namespace dta {

namespace {

// One lane per pixel, lanes along the row-major pixel index: every band plane is read as whole coalesced runs.  The
// min / max of a pixel live in two registers over a first pass through its bands; the scaling pass reads the bands again
// (a workgroup's strip is 256 pixels x bands, at most a few hundred KB: that second read is expected to be served by L2
// or the memory-side cache).
// TILES: out is bf16 [ceil(C / 16)][P][16] (a lane writes the 32 bytes of one pixel and chunk), else float32 [C][P].
template <typename T, bool TILES>
__global__ __launch_bounds__(256) void k_raster_normalise(RasterArgs a) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.P) return;
  const T* src = reinterpret_cast<const T*>(a.raw) + (size_t)a.c0 * a.P + p;
  const int C = a.C;
  float lo = __builtin_inff(), hi = -__builtin_inff();
#pragma unroll 8
  for (int c = 0; c < C; ++c) {
    const float v = to_f(src[(size_t)c * a.P]);
    lo = fminf(lo, v); hi = fmaxf(hi, v);             // NaNs are passed over, as nanmin / nanmax do
  }
  const float tiny = 10.f * 1.1920928955078125e-07f;   // scikit-learn: ranges below 10 * eps(float32) are "constant"
  float rng = hi - lo;
  if (rng < tiny) rng = 1.f;
  const float s = 1.f / rng;
  const float m = 0.f - mul_rounded(lo, s);
  if (!TILES) {
    float* out = reinterpret_cast<float*>(a.out) + p;
#pragma unroll 8
    for (int c = 0; c < C; ++c) out[(size_t)c * a.P] = mul_rounded(to_f(src[(size_t)c * a.P]), s) + m;
  } else {
    const int NC = (C + 15) / 16;
    unsigned short* out = reinterpret_cast<unsigned short*>(a.out);
    for (int ch = 0; ch < NC; ++ch) {
      unsigned pk[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = ch * 16 + 2 * e;
        const float v0 = c < C ? mul_rounded(to_f(src[(size_t)c * a.P]), s) + m : 0.f;
        const float v1 = c + 1 < C ? mul_rounded(to_f(src[(size_t)(c + 1) * a.P]), s) + m : 0.f;
        pk[e] = pack2_fmt(v0, v1, FMT_BF16);
      }
      u32x4* dst = reinterpret_cast<u32x4*>(out + ((size_t)ch * a.P + p) * 16);
      dst[0] = u32x4{pk[0], pk[1], pk[2], pk[3]};
      dst[1] = u32x4{pk[4], pk[5], pk[6], pk[7]};
    }
  }
}

// float32 NCHW batch [N][C][S][S] out of the float32 raster [C][H][W].  The batch is one flat array; a lane owns four
// consecutive elements of it (one 16-byte store; a window's C*S*S floats are not a multiple of four, so a lane's four
// may straddle rows, planes or windows: the index is decomposed once and carried).  Positions outside the raster: 0.
__global__ __launch_bounds__(256) void k_gather_windows(GatherArgs a) {
  const size_t q4 = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)a.N * a.C * a.S * a.S;
  size_t e = q4 * 4;
  if (e >= total) return;
  const int S = a.S, SS = S * S;
  const size_t per = (size_t)a.C * SS;
  int n = (int)(e / per);
  int r = (int)(e - (size_t)n * per);
  int c = r / SS, q = r - c * SS;
  int i = q / S, j = q - i * S;
  const float* ras = reinterpret_cast<const float*>(a.raster);
  const size_t plane = (size_t)a.H * a.W;
  long long row0 = a.origins[2 * n], col0 = a.origins[2 * n + 1];
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = 0.f;
    if (e + k < total) {
      const long long rr = row0 + i, cc = col0 + j;
      if (rr >= 0 && rr < a.H && cc >= 0 && cc < a.W) v[k] = ras[(size_t)c * plane + (size_t)rr * a.W + (size_t)cc];
      if (++j == S) {
        j = 0;
        if (++i == S) {
          i = 0;
          if (++c == a.C) {
            c = 0; ++n;
            if (n < a.N) { row0 = a.origins[2 * n]; col0 = a.origins[2 * n + 1]; }
          }
        }
      }
    }
  }
  float* out = reinterpret_cast<float*>(a.out);
  if (e + 4 <= total) *reinterpret_cast<f32x4*>(out + e) = f32x4{v[0], v[1], v[2], v[3]};
  else for (int k = 0; e + k < total; ++k) out[e + k] = v[k];
}

// The first conv's bf16 tiles [N][NC][S*S][16] (preprocess.PatchTiles) out of the bf16 raster [NC][P][16]: an element
// (window, chunk, pixel) is a 32-byte copy; a lane moves one 16-byte half of it, consecutive lanes consecutive halves, so
// the stores of a wave are one contiguous run and its loads runs of S pixels (32 * S bytes) of a raster row.
__global__ __launch_bounds__(256) void k_gather_windows_tiles(GatherArgs a) {
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int S = a.S, SS = S * S, NC = (a.C + 15) / 16;
  const size_t total = (size_t)a.N * NC * SS * 2;
  if (id >= total) return;
  const int half = (int)(id & 1);
  const size_t el = id >> 1;
  const int q = (int)(el % SS);
  const size_t t = el / SS;
  const int ch = (int)(t % NC), n = (int)(t / NC);
  const int i = q / S, j = q - i * S;
  const long long rr = (long long)a.origins[2 * n] + i, cc = (long long)a.origins[2 * n + 1] + j;
  u32x4 v = u32x4{0u, 0u, 0u, 0u};
  if (rr >= 0 && rr < a.H && cc >= 0 && cc < a.W) {
    const size_t plane = (size_t)a.H * a.W;
    v = reinterpret_cast<const u32x4*>(a.raster)[((size_t)ch * plane + (size_t)rr * a.W + (size_t)cc) * 2 + half];
  }
  reinterpret_cast<u32x4*>(a.out)[id] = v;
}

// One workgroup per crown.  A thread owns classes t, t + 256, ...: it adds the crown's rows of that class in row order
// (one float32 accumulator, no atomics, no tree: the order is the definition, dense.crown_reduce_np) and divides by the
// count.  Top-2 of the mean as k_softmax_top2 takes it (strictly greater replaces: ties go to the lower class).
__global__ __launch_bounds__(256) void k_crown_reduce(CrownArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int k = blockIdx.x, t = threadIdx.x, classes = a.classes;
  const long long r0 = a.offsets[k], r1 = a.offsets[k + 1];
  const long long cnt = r1 > r0 ? r1 - r0 : 0;
  float* mean = a.mean + (size_t)k * classes;
  if (cnt == 0) {      // an empty crown: count 0, label -1, score 0
    for (int c = t; c < classes; c += 256) mean[c] = 0.f;
    if (t == 0) {
      a.count[k] = 0;
      a.top_idx[2 * k] = -1; a.top_idx[2 * k + 1] = -1;
      a.top_score[2 * k] = 0.f; a.top_score[2 * k + 1] = 0.f;
    }
    return;
  }
  const float fc = (float)cnt;
  float b1 = -1.f, b2 = -1.f;
  int i1 = -1, i2 = -1;
  for (int c = t; c < classes; c += 256) {
    const float* src = a.probs + (size_t)r0 * classes + c;
    float acc = 0.f;
    long long r = 0;
    for (; r + 4 <= cnt; r += 4) {      // four loads in flight, added in row order
      const float v0 = src[(size_t)r * classes], v1 = src[(size_t)(r + 1) * classes];
      const float v2 = src[(size_t)(r + 2) * classes], v3 = src[(size_t)(r + 3) * classes];
      acc += v0; acc += v1; acc += v2; acc += v3;
    }
    for (; r < cnt; ++r) acc += src[(size_t)r * classes];
    const float mv = acc / fc;
    mean[c] = mv;
    if (mv > b1) { b2 = b1; i2 = i1; b1 = mv; i1 = c; }
    else if (mv > b2) { b2 = mv; i2 = c; }
  }
  // the threads' (best, second) pairs, merged by one thread in thread order (= ascending class within equal values)
  float* cs = sm;
  int* ci = reinterpret_cast<int*>(sm + 512);
  cs[2 * t] = b1; cs[2 * t + 1] = b2; ci[2 * t] = i1; ci[2 * t + 1] = i2;
  __syncthreads();
  if (t == 0) {
    float g1 = -1.f, g2 = -1.f;
    int j1 = -1, j2 = -1;
    for (int u = 0; u < 512; ++u) {
      const float v = cs[u];
      const int iv = ci[u];
      if (iv < 0) continue;
      if (v > g1 || (v == g1 && iv < j1)) { g2 = g1; j2 = j1; g1 = v; j1 = iv; }
      else if (v > g2 || (v == g2 && iv < j2)) { g2 = v; j2 = iv; }
    }
    a.count[k] = (int)cnt;
    a.top_idx[2 * k] = j1; a.top_idx[2 * k + 1] = j2;
    a.top_score[2 * k] = j1 < 0 ? 0.f : g1; a.top_score[2 * k + 1] = j2 < 0 ? 0.f : g2;
  }
}

template <typename T>
int launch_normalise_t(const RasterArgs& a, hipStream_t st) {
  const long long blocks = (a.P + 255) / 256;
  if (blocks > 0x7FFFFFFFll) { dta_set_error("dta_raster_normalise: raster too large for one launch"); return 1; }
  const dim3 grid((unsigned)blocks);
  if (a.tiles) hipLaunchKernelGGL((k_raster_normalise<T, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_raster_normalise<T, false>), grid, dim3(256), 0, st, a);
  DTA_CHECK_LAUNCH("k_raster_normalise");
  return 0;
}

}  // namespace

int launch_raster_normalise(const RasterArgs& a, int dtype, hipStream_t st) {
  switch (dtype) {
    case DTA_CROP_F32: return launch_normalise_t<float>(a, st);
    case DTA_CROP_I16: return launch_normalise_t<short>(a, st);
    case DTA_CROP_U8: return launch_normalise_t<unsigned char>(a, st);
    default: dta_set_error("dta_raster_normalise: unknown raw dtype %d", dtype); return 1;
  }
}

int launch_gather_windows(const GatherArgs& a, hipStream_t st) {
  const size_t total = (size_t)a.N * a.C * a.S * a.S, lanes = (total + 3) / 4;
  const size_t blocks = (lanes + 255) / 256;
  if (blocks > 0x7FFFFFFFull) { dta_set_error("dta_gather_windows: batch too large for one launch"); return 1; }
  hipLaunchKernelGGL(k_gather_windows, dim3((unsigned)blocks), dim3(256), 0, st, a);
  DTA_CHECK_LAUNCH("k_gather_windows");
  return 0;
}

int launch_gather_windows_tiles(const GatherArgs& a, hipStream_t st) {
  const size_t total = (size_t)a.N * ((a.C + 15) / 16) * a.S * a.S * 2;
  const size_t blocks = (total + 255) / 256;
  if (blocks > 0x7FFFFFFFull) { dta_set_error("dta_gather_windows_tiles: batch too large for one launch"); return 1; }
  hipLaunchKernelGGL(k_gather_windows_tiles, dim3((unsigned)blocks), dim3(256), 0, st, a);
  DTA_CHECK_LAUNCH("k_gather_windows_tiles");
  return 0;
}

int launch_crown_reduce(const CrownArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_crown_reduce, dim3(a.n_crowns), dim3(256), 1024 * 4, st, a);
  DTA_CHECK_LAUNCH("k_crown_reduce");
  return 0;
}

}  // namespace dta
