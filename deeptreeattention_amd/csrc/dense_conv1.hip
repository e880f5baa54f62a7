// Dense prediction with the first conv computed once per raster instead of once per window ("The first conv
// once per raster").  The first 3x3 conv sits in front of every pool, so its output at a window position depends only on
// the raster pixel p under that position and on which of the nine taps fall outside the window -- one of nine classes
// (top / middle / bottom row of the window) x (left / middle / right column):
//   k_raster_conv1_taps     T[q][dy][dx][n] = sum_k w[n][k][dy+1][dx+1] * x[k][q]      ONE GEMM over the raster's pixels
//   k_raster_conv1_classes  A[p][rc][cc][n] = bias[n] + sum_{dy in R(rc)} sum_{dx in R(cc)} T[p + (dy, dx)][dy][dx][n]
//                           over the raster extended by a one-pixel ring, plus one "far outside" row (the bias alone)
//   k_gather_conv1_windows  conv1(window at o)[i][j][:] = A[o + (i, j)][rc(i)][cc(j)][:]   a pure 16-byte-piece copy
// with R(top / left) = {0, +1}, R(middle) = {-1, 0, +1}, R(bottom / right) = {-1, 0}.  The table A holds what
// launch_conv3x3 writes into the forward's y[0] (pre-BatchNorm, bias included, the plan's y_fmt), so the forward that
// follows the gather skips its first conv and nothing downstream changes.  dense.conv1_table_np / gather_conv1_np are
// the written-down meaning.  No atomics, one float32 accumulator per element, fixed orders: reruns are bit-identical.
// For a multi-stage model (levels x years spectral networks; every level's year-y network reads year y's raster) the
// table of a year holds the levels side by side -- columns 32 l .. 32 l + 31 are level l's year-y first conv -- so a
// raster is read ONCE for all levels:
//   k_raster_conv1_mask           mask[p] = the raster pixel under table position p has a non-zero stored element
//   k_gather_conv1_windows_years  the gather for all levels x years in one launch (blockIdx.y = year), each level's 32
//                                 columns into its (level, year) group's y[0]; sets the years' 0/1 flags from the mask
// Sizes per raster pixel and year: 9 x 32 x levels x 2 B of table in half (4 B in fp32) and 9 x 32 x levels x 4 B of T in
// the scratch, which the years share (they are built one after the other).  5 levels at 256x256: 189 MB of table per year
// plus 377 MB of shared scratch.
#include "kernels.h"

namespace dta {

namespace {

// ---- operand fragments of the tap GEMM: the forward conv's own MFMAs (conv.hip: Frag) on operands read straight from
//      global memory.  A = 32 raster pixels x 16 bands of one chunk, B = 32 columns (tap, n) of k_pack_conv_w's forward
//      image [chunk][tap][n][16] (the flat column index tap * cols + n IS that image's row index).
template <typename T> struct TapFrag;
template <> struct TapFrag<bf16_t> {
  static constexpr int KS = 16;
  typedef bf16x8 reg;
  // raster: bf16 chunks [NC][P][16]; bands past C are zero in the chunks themselves (k_raster_normalise)
  __device__ static __forceinline__ reg load_a(const void* ras, long long P, int C, int chunk, long long p, int ks, int lane) {
    return *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16_t*>(ras) + ((size_t)chunk * P + p) * 16 + ((lane >> 5) << 3));
  }
  __device__ static __forceinline__ reg load_b(const void* wrow, int row, int ks, int lane) {
    return *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16_t*>(wrow) + tl_pos<bf16_t>(row, (lane >> 5) << 3));
  }
  __device__ static __forceinline__ f32x16 mfma(reg a, reg b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct TapFrag<float> {
  static constexpr int KS = 2;
  typedef float reg;
  // raster: float32 planes [C][P]; the contraction is padded to the chunk in the weights only: a band past C reads nothing
  __device__ static __forceinline__ reg load_a(const void* ras, long long P, int C, int chunk, long long p, int ks, int lane) {
    const int kc = chunk * 16 + ks * 2 + (lane >> 5);
    return kc < C ? reinterpret_cast<const float*>(ras)[(size_t)kc * P + p] : 0.f;
  }
  __device__ static __forceinline__ reg load_b(const void* wrow, int row, int ks, int lane) {
    return reinterpret_cast<const float*>(wrow)[tl_pos<float>(row, ks * 2 + (lane >> 5))];
  }
  __device__ static __forceinline__ f32x16 mfma(reg a, reg b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
};

// One workgroup = 4 waves = 256 consecutive pixels x 96 columns (blockIdx.y); a wave owns 64 pixels (two 32-row tiles) x
// three 32-column tiles: 96 accumulator registers.  Both operands come from global memory: a wave's A loads are whole
// runs of 32 pixels (1 KB of a bf16 chunk, 128 B of a float32 plane), the weight image (425 KB for 349 bands x 576
// columns in bf16) stays in L2.  Runs once per raster.
constexpr int TAP_MT = 2, TAP_NT = 3, TAP_COLS = TAP_NT * 32, TAP_ROWS = 4 * TAP_MT * 32;
template <typename T>
__global__ __launch_bounds__(256) void k_raster_conv1_taps(Conv1TapsArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long P = a.P;
  const long long p0 = (long long)blockIdx.x * TAP_ROWS + wave * (TAP_MT * 32);
  const int n0 = blockIdx.y * TAP_COLS;
  const int N = a.N;
  long long pa[TAP_MT];
#pragma unroll
  for (int mt = 0; mt < TAP_MT; ++mt) {
    const long long p = p0 + mt * 32 + (lane & 31);
    pa[mt] = p < P ? p : P - 1;      // rows past the raster repeat the last pixel and are not stored
  }
  int col[TAP_NT];
#pragma unroll
  for (int nt = 0; nt < TAP_NT; ++nt) col[nt] = n0 + nt * 32 + (lane & 31);
  f32x16 acc[TAP_MT][TAP_NT];
#pragma unroll
  for (int mt = 0; mt < TAP_MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < TAP_NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
  const T* wp = reinterpret_cast<const T*>(a.wp);
  for (int chunk = 0; chunk < a.NC; ++chunk) {
    const T* wrow[TAP_NT];
#pragma unroll
    for (int nt = 0; nt < TAP_NT; ++nt) wrow[nt] = wp + ((size_t)chunk * N + col[nt]) * 16;
#pragma unroll
    for (int ks = 0; ks < 16 / TapFrag<T>::KS; ++ks) {
      typename TapFrag<T>::reg af[TAP_MT], bf[TAP_NT];
#pragma unroll
      for (int mt = 0; mt < TAP_MT; ++mt) af[mt] = TapFrag<T>::load_a(a.raster, P, a.C, chunk, pa[mt], ks, lane);
#pragma unroll
      for (int nt = 0; nt < TAP_NT; ++nt) bf[nt] = TapFrag<T>::load_b(wrow[nt], col[nt], ks, lane);
#pragma unroll
      for (int mt = 0; mt < TAP_MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < TAP_NT; ++nt) acc[mt][nt] = TapFrag<T>::mfma(af[mt], bf[nt], acc[mt][nt]);
    }
  }
#pragma unroll
  for (int mt = 0; mt < TAP_MT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long p = p0 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (p < P) {
#pragma unroll
        for (int nt = 0; nt < TAP_NT; ++nt) a.T[(size_t)p * N + col[nt]] = acc[mt][nt][r];
      }
    }
}

// One lane per (position, column n), lanes along n: the nine taps T[p + (dy, dx)][dy][dx][n] of the position are read once
// (zero where p + (dy, dx) is outside the raster) and the nine class sums formed from them, each ONE float32 accumulator:
// the bias first, then the taps in ascending (dy, dx).  Positions: the (H + 2) x (W + 2) grid of the raster with its
// one-pixel ring, row-major, then the far-outside row.
__global__ __launch_bounds__(256) void k_raster_conv1_classes(Conv1ClassArgs a) {
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int cols = a.cols, W2 = a.W + 2;
  const size_t far = a.far_only ? 0 : (size_t)(a.H + 2) * W2;
  if (id >= (far + 1) * cols) return;
  const int n = (int)(id % cols);
  const size_t pos = id / cols;
  const float b = a.bias[n / a.bias_split][n % a.bias_split];
  float t[3][3];
#pragma unroll
  for (int u = 0; u < 3; ++u)
#pragma unroll
    for (int v = 0; v < 3; ++v) t[u][v] = 0.f;
  if (pos < far) {
    const int r = (int)(pos / W2) - 1, c = (int)(pos % W2) - 1;
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const int rr = r + u - 1, cc = c + v - 1;
        if (rr >= 0 && rr < a.H && cc >= 0 && cc < a.W) t[u][v] = a.T[(((size_t)rr * a.W + cc) * 9 + u * 3 + v) * cols + n];
      }
  }
#pragma unroll
  for (int rc = 0; rc < 3; ++rc)
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
      float acc = b;
#pragma unroll
      for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          // top row / left column of the window: the tap at -1 is outside it; bottom / right: the tap at +1
          const bool in = !(rc == 0 && u == 0) && !(rc == 2 && u == 2) && !(cc == 0 && v == 0) && !(cc == 2 && v == 2);
          if (in) acc += t[u][v];
        }
      st_fmt(a.A, (pos * 9 + rc * 3 + cc) * cols + n, acc, a.fmt);
    }
}

// A lane copies one 16-byte piece of one output row (window n, position r = i * 11 + j), consecutive lanes consecutive
// pieces: a wave's stores are one contiguous run, its loads whole table rows.  Origins may lie anywhere: rows and columns
// are 64-bit (as gather_lane, dense.hip), and a position beyond the ring reads the far-outside row.
__global__ __launch_bounds__(256) void k_gather_conv1_windows(Conv1GatherArgs a) {
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int ppr = a.ppr;
  if (id >= (size_t)a.N * 121 * ppr) return;
  const int piece = (int)(id % ppr);
  const size_t row = id / ppr;
  const int n = (int)(row / 121), r = (int)(row - (size_t)n * 121);
  const int i = r / 11, j = r - i * 11;
  const long long rr = (long long)a.origins[2 * n] + i, cc = (long long)a.origins[2 * n + 1] + j;
  const long long W2 = (long long)a.W + 2;
  long long pos = ((long long)a.H + 2) * W2;      // far outside
  if (rr >= -1 && rr <= a.H && cc >= -1 && cc <= a.W) pos = (rr + 1) * W2 + (cc + 1);
  const int cls = (i == 0 ? 0 : (i == 10 ? 2 : 1)) * 3 + (j == 0 ? 0 : (j == 10 ? 2 : 1));
  reinterpret_cast<u32x4*>(a.out)[id] = reinterpret_cast<const u32x4*>(a.A)[((size_t)pos * 9 + cls) * ppr + piece];
}

// One lane per table position, lanes along the positions: a wave reads runs of consecutive pixels (a float32 plane: 4 B
// per lane and band; a bf16 chunk: the pixel's 32 B) and writes 64 consecutive bytes.  The ring and the far-outside row
// are 0.  bf16 chunks hold zeros in the bands past C, so whole chunks are tested; -0 is zero, NaN is not.
template <typename T>
__global__ __launch_bounds__(256) void k_raster_conv1_mask(Conv1MaskArgs a) {
  const size_t pos = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int W2 = a.W + 2;
  const size_t far = (size_t)(a.H + 2) * W2;
  if (pos > far) return;
  bool hit = false;
  const int r = (int)(pos / W2) - 1, c = (int)(pos % W2) - 1;
  if (pos < far && r >= 0 && r < a.H && c >= 0 && c < a.W) {
    const size_t P = (size_t)a.H * a.W, p = (size_t)r * a.W + c;
    if constexpr (sizeof(T) == 2) {
      const u32x4* ras = reinterpret_cast<const u32x4*>(a.raster);
      for (int ch = 0; ch < a.NC; ++ch)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const u32x4 v = ras[((size_t)ch * P + p) * 2 + half];
          hit |= ((v[0] | v[1] | v[2] | v[3]) & 0x7FFF7FFFu) != 0u;
        }
    } else {
      const float* ras = reinterpret_cast<const float*>(a.raster);
      for (int k = 0; k < a.C; ++k) hit |= !(ras[(size_t)k * P + p] == 0.f);
    }
  }
  a.mask[pos] = hit ? 1 : 0;
}

// k_gather_conv1_windows for every (level, year) group of a multi-stage model: blockIdx.y = year, a lane copies one
// 16-byte piece of one output row; consecutive lanes take consecutive pieces of the year's table row (levels * ppl of
// them: a wave's loads are whole table rows), level l's ppl pieces land in group first[l] + year at row stride ppl pieces.
// Position, class and far-outside rules as above; a year with whole == 0 reads its one far-outside row everywhere.
// Flags: dta_gather_windows_years' protocol -- a wave that saw a set mask byte stores 1.f once (plain stores of one
// value: no atomics, any order); flags arrive zeroed, block 0 of each year zeroes clear_next.
__global__ __launch_bounds__(256) void k_gather_conv1_windows_years(Conv1GatherYearsArgs a) {
  const int y = blockIdx.y;
  if (a.clear_next && blockIdx.x == 0 && threadIdx.x == 0) a.clear_next[y] = 0.f;
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int ppl = a.ppl, ppr = a.levels * ppl;
  bool hit = false;
  if (id < (size_t)a.N * 121 * ppr) {
    const int piece = (int)(id % ppr);
    const size_t row = id / ppr;
    const int n = (int)(row / 121), r = (int)(row - (size_t)n * 121);
    const int i = r / 11, j = r - i * 11;
    long long pos = 0;
    if (a.whole[y]) {
      const long long rr = (long long)a.origins[2 * n] + i, cc = (long long)a.origins[2 * n + 1] + j;
      const long long W2 = (long long)a.W + 2;
      pos = ((long long)a.H + 2) * W2;      // far outside
      if (rr >= -1 && rr <= a.H && cc >= -1 && cc <= a.W) pos = (rr + 1) * W2 + (cc + 1);
    }
    const int cls = (i == 0 ? 0 : (i == 10 ? 2 : 1)) * 3 + (j == 0 ? 0 : (j == 10 ? 2 : 1));
    const int l = piece / ppl, q = piece - l * ppl;
    char* dst = reinterpret_cast<char*>(a.out) + (size_t)(a.first[l] + y) * a.group_bytes;
    reinterpret_cast<u32x4*>(dst)[row * ppl + q] = reinterpret_cast<const u32x4*>(a.A[y])[((size_t)pos * 9 + cls) * ppr + piece];
    hit = a.mask[y][pos] != 0;
  }
  if (__any(hit) && (threadIdx.x & 63) == 0) a.flags[y] = 1.f;
}

}  // namespace

int launch_raster_conv1_taps(const Conv1TapsArgs& a, bool bf16, hipStream_t st) {
  if (a.N % TAP_COLS != 0 || a.P < 1) { dta_set_error("dta_raster_conv1_table: %d table columns are no multiple of %d", a.N, TAP_COLS); return 1; }
  const long long blocks = (a.P + TAP_ROWS - 1) / TAP_ROWS;
  if (blocks > 0x7FFFFFFFll) { dta_set_error("dta_raster_conv1_table: raster too large for one launch"); return 1; }
  const dim3 grid((unsigned)blocks, a.N / TAP_COLS);
  if (bf16) hipLaunchKernelGGL(k_raster_conv1_taps<bf16_t>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_raster_conv1_taps<float>, grid, dim3(256), 0, st, a);
  DTA_CHECK_LAUNCH("k_raster_conv1_taps");
  return 0;
}

int launch_raster_conv1_classes(const Conv1ClassArgs& a, hipStream_t st) {
  const size_t total = (a.far_only ? 1 : (size_t)(a.H + 2) * (a.W + 2) + 1) * a.cols, blocks = (total + 255) / 256;
  if (blocks > 0x7FFFFFFFull) { dta_set_error("dta_raster_conv1_table: raster too large for one launch"); return 1; }
  hipLaunchKernelGGL(k_raster_conv1_classes, dim3((unsigned)blocks), dim3(256), 0, st, a);
  DTA_CHECK_LAUNCH("k_raster_conv1_classes");
  return 0;
}

int launch_gather_conv1_windows(const Conv1GatherArgs& a, hipStream_t st) {
  const size_t total = (size_t)a.N * 121 * a.ppr, blocks = (total + 255) / 256;
  if (blocks > 0x7FFFFFFFull) { dta_set_error("dta_gather_conv1_windows: batch too large for one launch"); return 1; }
  hipLaunchKernelGGL(k_gather_conv1_windows, dim3((unsigned)blocks), dim3(256), 0, st, a);
  DTA_CHECK_LAUNCH("k_gather_conv1_windows");
  return 0;
}

int launch_raster_conv1_mask(const Conv1MaskArgs& a, bool bf16, hipStream_t st) {
  const size_t total = (size_t)(a.H + 2) * (a.W + 2) + 1, blocks = (total + 255) / 256;
  if (blocks > 0x7FFFFFFFull) { dta_set_error("dta_conv1_multistage_raster_table: raster too large for one launch"); return 1; }
  if (bf16) hipLaunchKernelGGL(k_raster_conv1_mask<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_raster_conv1_mask<float>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  DTA_CHECK_LAUNCH("k_raster_conv1_mask");
  return 0;
}

int launch_gather_conv1_windows_years(const Conv1GatherYearsArgs& a, hipStream_t st) {
  const size_t total = (size_t)a.N * 121 * a.levels * a.ppl, blocks = (total + 255) / 256;
  if (blocks > 0x7FFFFFFFull) { dta_set_error("dta_conv1_multistage_gather_windows: batch too large for one launch"); return 1; }
  // flags must be zero on entry: cleared here, unless the caller alternates two banks and lets each call clear the other
  if (!a.clear_next && hipMemsetAsync(a.flags, 0, sizeof(float) * a.years, st) != hipSuccess) { dta_set_error("dta_conv1_multistage_gather_windows: memset failed"); return 1; }
  hipLaunchKernelGGL(k_gather_conv1_windows_years, dim3((unsigned)blocks, a.years), dim3(256), 0, st, a);
  DTA_CHECK_LAUNCH("k_gather_conv1_windows_years");
  return 0;
}

}  // namespace dta
