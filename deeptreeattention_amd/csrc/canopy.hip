// Crown height filter (reference src/CHM.py: non_zero_99_quantile through rasterstats.zonal_stats, one Python call and one
// np.nanpercentile per crown; height_rules; src/predict.py:35-42 find_crowns' CHM_height > 3).
// deeptreeattention_amd/canopy.py holds the definition (crown_height_np, min_height_np, height_rules_np); these kernels
// equal it bit for bit: the two order statistics are selected exactly, on the bit patterns of the kept values (all of them
// positive floats or +inf, so the patterns order as unsigned integers), and the interpolation is four float32 operations
// rounded one by one.
//   k_crown_height_wave   one 64-lane wave per crown, four crowns per workgroup: a clipped box of at most CH_WAVE_CELLS cells;
//                         the keys stay in registers, the lo-th key comes from an MSB-first radix select, one bit per round,
//                         counted with ballots
//   k_crown_height_block  one workgroup at a time per crown of more cells (up to 2^24): four passes of 8-bit digit histograms
//                         in LDS, every pass re-reads the box; a workgroup looks at a chunk of crowns and skips the smaller
// Each crown belongs to exactly one of the two, which writes height, count and keep for it.  No workspace, no global
// atomics, no float atomics; a crown's result depends on its own box alone.
#include "../../include/dta_hip.h"
#include "common.h"

// the lerp and the rank are the reference's float32 operations one by one: no fused multiply-add in this file (hipcc
// contracts by default and sees through HIP's __fmul_rn; see mul_rounded in common.h)
#pragma clang fp contract(off)

namespace dta {

constexpr int CH_THREADS = 256;                     // the wave kernel: four crowns per workgroup
constexpr int CH_BLOCK_THREADS = 1024;              // the block kernel: sixteen waves share one crown's cells
constexpr int CH_BLOCK_GRID = 2048;                 // ... and up to here a workgroup per crown, then chunks of crowns
constexpr int CH_WAVE_CELLS = DTA_CROWN_WAVE_CELLS;
constexpr int CH_SLOTS = CH_WAVE_CELLS / 64;        // keys per lane of the wave kernel
constexpr long long CH_MAX_CELLS = 1ll << 24;       // float32(n - 1) is exact up to here
constexpr unsigned CH_NO_KEY = 0xFFFFFFFFu;         // a cell that is not kept: above every kept key (their sign bit is clear)
constexpr unsigned CH_MAX_GRID = 1u << 20;
static_assert(CH_WAVE_CELLS % 64 == 0 && CH_SLOTS >= 1 && CH_SLOTS <= 32, "the wave kernel keeps CH_SLOTS keys per lane");

struct CrownArgs {
  const float* chm; int H, W;
  const int* boxes; long long n;
  float qf, floor;                 // q / 100 as the host's float32 division gives it
  const double* field;
  int mode; double min_height, min_chm, max_diff, limit;
  float* height; int* count; unsigned char* keep;
};

struct Clip { int r0, c0, h, w; };

// the box's intersection with the raster; h or w is 0 for a box that misses it or has no rows / columns
__device__ __forceinline__ Clip clip_box(const int* b, int H, int W) {
  const int r0 = b[0] > 0 ? b[0] : 0, c0 = b[1] > 0 ? b[1] : 0;
  const int r1 = b[2] < H ? b[2] : H, c1 = b[3] < W ? b[3] : W;
  Clip c;
  c.r0 = r0; c.c0 = c0;
  c.h = r1 > r0 ? r1 - r0 : 0;     // subtracted only where both lie in [0, H]: no overflow for any int32 box
  c.w = c1 > c0 ? c1 - c0 : 0;
  return c;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ unsigned wave_min_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned w = (unsigned)__shfl_xor((int)v, o); v = w < v ? w : v; }
  return v;
}

// the two ranks and the weight of n >= 1 kept values (canopy.py: _rank)
__device__ __forceinline__ void crown_rank(int n, float qf, int* lo, int* hi, float* t) {
  const float virt = mul_rounded((float)(n - 1), qf);      // qf <= 1: virt <= n - 1
  int l = (int)virt;                                       // virt >= 0: the floor
  l = l < n - 1 ? l : n - 1;
  *lo = l;
  *hi = l + 1 < n - 1 ? l + 1 : n - 1;
  *t = virt - (float)l;
}

// one crown's three outputs; ka / kb: the lo-th and hi-th smallest kept key (n >= 1), n: the kept count or -1 (refused)
__device__ __forceinline__ void crown_store(const CrownArgs& a, long long i, int n, unsigned ka, unsigned kb, float t) {
  float hgt = __uint_as_float(0x7FC00000u);
  if (n >= 1) {
    const float x = __uint_as_float(ka), y = __uint_as_float(kb);
    const float d = y - x;
    hgt = t >= 0.5f ? y - mul_rounded(d, 1.f - t) : x + mul_rounded(d, t);
  }
  a.height[i] = hgt;
  a.count[i] = n;
  if (a.mode == 0) return;
  const double chm = (double)hgt;
  bool keep;
  if (n < 0) {
    keep = false;
  } else if (a.mode == 1) {
    keep = chm > a.min_height;                             // a NaN height is dropped
  } else {                                                 // src/CHM.py:70-90, in its order, with its comparisons
    const double h = a.field[i];
    if (chm != chm) keep = false;
    else if (h != h) keep = true;
    else if (chm < a.min_chm) keep = false;
    else if (chm > h) keep = !(chm - h >= a.max_diff);
    else keep = !(h - chm >= a.limit);
  }
  a.keep[i] = keep ? 1 : 0;
}

// The lo-th smallest of a wave's keys (the first SLOTS of every lane), bit by bit from the top: of the keys that share the
// bits decided so far, c0 have a 0 next.  Counting is a ballot and a population count per slot, so the counts, the rank
// and the prefix are the same in every lane without any exchange.  Also: how many keys are <= it, and the smallest above it
// (the hi-th value is the same key while enough keys are <= it, otherwise that one).
template <int SLOTS>
__device__ __forceinline__ void wave_select(const unsigned (&key)[CH_SLOTS], int lo, unsigned* kth, int* le, unsigned* above) {
  static_assert(SLOTS <= CH_SLOTS, "");
  unsigned prefix = 0u;
  int k = lo;
  for (int b = 30; b >= 0; --b) {                          // bit 31 is clear in every kept key and set in CH_NO_KEY
    const unsigned care = ~((1u << b) - 1u);               // bit b and everything above it
    int c0 = 0;
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) c0 += __popcll(__ballot((key[j] & care) == prefix));
    if (k >= c0) { k -= c0; prefix |= 1u << b; }
  }
  int n_le = 0;
  unsigned up = CH_NO_KEY;
#pragma unroll
  for (int j = 0; j < SLOTS; ++j) {
    n_le += __popcll(__ballot(key[j] <= prefix));
    up = (key[j] > prefix && key[j] < up) ? key[j] : up;
  }
  *kth = prefix; *le = n_le; *above = wave_min_u(up);
}

__global__ __launch_bounds__(CH_THREADS) void k_crown_height_wave(CrownArgs a) {
  const int lane = threadIdx.x & 63;
  const long long waves = (long long)gridDim.x * (CH_THREADS / 64);
  for (long long i = (long long)blockIdx.x * (CH_THREADS / 64) + (threadIdx.x >> 6); i < a.n; i += waves) {   // wave-uniform
    Clip c = clip_box(a.boxes + 4 * i, a.H, a.W);
    // the same in every lane; said so, the compiler keeps the box, the branches on it and the select's rank in scalars
    c.r0 = __builtin_amdgcn_readfirstlane(c.r0); c.c0 = __builtin_amdgcn_readfirstlane(c.c0);
    c.h = __builtin_amdgcn_readfirstlane(c.h); c.w = __builtin_amdgcn_readfirstlane(c.w);
    const long long area = (long long)c.h * c.w;
    if (area > CH_WAVE_CELLS) continue;                    // k_crown_height_block's crown
    const int cells = (int)area;
    // cell e = lane + 64 j of the box, row-major: (row, col) advance by (64 / w, 64 % w) with one carry
    int row = 0, col = 0, sr = 0, sc = 0;
    if (c.w > 0) { row = lane / c.w; col = lane - row * c.w; sr = 64 / c.w; sc = 64 - sr * c.w; }
    const float* base = a.chm + (size_t)c.r0 * a.W + c.c0;
    unsigned key[CH_SLOTS];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < CH_SLOTS; ++j) {
      unsigned k = CH_NO_KEY;
      if (lane + 64 * j < cells) {                         // inside the clipped box: inside the raster
        const float v = base[(size_t)row * a.W + col];
        if (v >= a.floor) { k = __float_as_uint(v); ++mine; }   // false for NaN, nodata, everything under the floor
      }
      key[j] = k;
      col += sc; row += sr;
      if (col >= c.w) { col -= c.w; ++row; }
    }
    const int n = wave_sum_i(mine);
    if (n == 0) {
      if (lane == 0) crown_store(a, i, 0, 0u, 0u, 0.f);
      continue;
    }
    int lo, hi; float t;
    crown_rank(n, a.qf, &lo, &hi, &t);
    unsigned prefix, above;
    int le;
    if (cells <= 256) wave_select<4>(key, lo, &prefix, &le, &above);          // slots past the box hold CH_NO_KEY: not looked at
    else if (cells <= 512) wave_select<8>(key, lo, &prefix, &le, &above);
    else wave_select<CH_SLOTS>(key, lo, &prefix, &le, &above);
    const unsigned kb = (hi == lo || le >= lo + 2) ? prefix : above;
    if (lane == 0) crown_store(a, i, n, prefix, kb, t);
  }
}

// f(key) for every kept cell of the box, the workgroup's CH_BLOCK_THREADS threads striding over its cells in row-major
// order, four independent loads in flight per thread
template <class F>
__device__ __forceinline__ void scan_box(const CrownArgs& a, const Clip& c, unsigned cells, F f) {
  const int tid = threadIdx.x;
  int row = tid / c.w, col = tid - row * c.w;
  const int sr = CH_BLOCK_THREADS / c.w, sc = CH_BLOCK_THREADS - sr * c.w;
  const float* base = a.chm + (size_t)c.r0 * a.W + c.c0;
  for (unsigned e = tid; e < cells; e += 4 * CH_BLOCK_THREADS) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      // a cell past the box is not read (-1 is under every floor); (row, col) may run past it, nothing follows them there
      v[u] = e + u * CH_BLOCK_THREADS < cells ? base[(size_t)row * a.W + col] : -1.f;
      col += sc; row += sr;
      if (col >= c.w) { col -= c.w; ++row; }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) if (v[u] >= a.floor) f(__float_as_uint(v[u]));
  }
}

// `chunk` consecutive crowns per workgroup (chunk <= CH_BLOCK_THREADS): one thread per crown clips its box and lists the
// crowns of more than CH_WAVE_CELLS cells, then the workgroup works through the list.  With mostly small crowns a
// workgroup looks at its chunk once and is done.
__global__ __launch_bounds__(CH_BLOCK_THREADS) void k_crown_height_block(CrownArgs a, int chunk) {
  __shared__ unsigned hist[256];
  __shared__ unsigned sel[4];        // the chosen digit, the rank left inside its bin, the bin's count, the histogram's total
  __shared__ unsigned red[CH_BLOCK_THREADS / 64];
  __shared__ int todo[CH_BLOCK_THREADS];
  __shared__ int ntodo;
  const int tid = threadIdx.x, lane = tid & 63;
  const long long i0 = (long long)blockIdx.x * chunk;
  if (tid == 0) ntodo = 0;
  __syncthreads();
  if (tid < chunk && i0 + tid < a.n) {
    const Clip c = clip_box(a.boxes + 4 * (i0 + tid), a.H, a.W);
    if ((long long)c.h * c.w > CH_WAVE_CELLS) todo[atomicAdd(&ntodo, 1)] = tid;      // (in any order: a crown's result is its own)
  }
  __syncthreads();
  const int crowns = ntodo;
  for (int m = 0; m < crowns; ++m) {                       // the same for every thread of the workgroup
    const long long i = i0 + todo[m];
    const Clip c = clip_box(a.boxes + 4 * i, a.H, a.W);
    const long long area = (long long)c.h * c.w;
    if (area > CH_MAX_CELLS) {                             // refused: float32(n - 1) would not be exact
      if (tid == 0) crown_store(a, i, -1, 0u, 0u, 0.f);
      continue;
    }
    const unsigned cells = (unsigned)area;
    unsigned prefix = 0u, left = 0u, same = 0u;
    int n = 0, lo = 0, hi = 0;
    float t = 0.f;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      if (tid < 256) hist[tid] = 0u;
      __syncthreads();
      const unsigned want = pass ? prefix >> (shift + 8) : 0u;
      scan_box(a, c, cells, [&](unsigned key) {
        if (pass == 0 || (key >> (shift + 8)) == want) atomicAdd(&hist[(key >> shift) & 255u], 1u);
      });
      __syncthreads();
      if (tid < 64) {                                      // wave 0: four bins per lane, a scan over the lanes, one owner
        unsigned u[4], s = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) { u[j] = hist[4 * lane + j]; s += u[j]; }
        unsigned incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned v = (unsigned)__shfl_up((int)incl, o); incl += lane >= o ? v : 0u; }
        const unsigned total = (unsigned)__shfl((int)incl, 63);
        unsigned k = left;
        if (pass == 0 && total > 0u) { int l, h; float tt; crown_rank((int)total, a.qf, &l, &h, &tt); k = (unsigned)l; }
        const unsigned excl = incl - s;
        if (total > 0u && excl <= k && k < incl) {         // exactly one lane: k < total
          unsigned r = k - excl, cnt = u[0];
          int d = 0;
#pragma unroll
          for (int j = 1; j < 4; ++j) if (d == j - 1 && r >= cnt) { r -= cnt; d = j; cnt = u[j]; }
          sel[0] = 4u * lane + d; sel[1] = r; sel[2] = cnt;
        }
        if (lane == 0) sel[3] = total;
      }
      __syncthreads();
      if (pass == 0) {
        n = (int)sel[3];
        if (n == 0) break;                                 // (the same in every thread)
        crown_rank(n, a.qf, &lo, &hi, &t);
      }
      prefix |= sel[0] << shift; left = sel[1]; same = sel[2];
    }
    if (n == 0) {
      if (tid == 0) crown_store(a, i, 0, 0u, 0u, 0.f);
      __syncthreads();                                     // sel is read before the next crown's wave 0 writes it
      continue;
    }
    // keys below the lo-th: lo - left; equal to it: same
    const unsigned le = (unsigned)lo - left + same;
    unsigned kb = prefix;
    if (hi != lo && le < (unsigned)lo + 2u) {              // the smallest key above it: one more pass over the box
      unsigned above = CH_NO_KEY;
      scan_box(a, c, cells, [&](unsigned key) { above = (key > prefix && key < above) ? key : above; });
      above = wave_min_u(above);
      if (lane == 0) red[tid >> 6] = above;
      __syncthreads();
      kb = red[0];
#pragma unroll
      for (int w = 1; w < CH_BLOCK_THREADS / 64; ++w) kb = red[w] < kb ? red[w] : kb;
    }
    if (tid == 0) crown_store(a, i, n, prefix, kb, t);
    __syncthreads();                                       // hist, sel and red are free for the next crown
  }
}

}  // namespace dta

using namespace dta;

extern "C" int dta_crown_height(const float* chm, int height, int width, const int* boxes, long long n, float q, float floor,
                                const double* field_height, const dta_height_rule* rule, float* out_height, int* out_count,
                                unsigned char* out_keep, void* stream) {
  const char* who = "dta_crown_height";
  if (!chm || !boxes || !out_height || !out_count) { dta_set_error("%s: null argument", who); return 1; }
  if (n < 1) { dta_set_error("%s: bad shape: n=%lld", who, n); return 1; }
  if (height < 1 || width < 1) { dta_set_error("%s: bad raster: height=%d width=%d", who, height, width); return 1; }
  if ((long long)height * width > 0x7FFFFFFFll) {
    dta_set_error("%s: raster too large: height=%d x width=%d cells is over int32", who, height, width);
    return 1;
  }
  if (!(q >= 0.f && q <= 100.f)) { dta_set_error("%s: q=%g is outside [0, 100]", who, (double)q); return 1; }
  if (!(floor > 0.f)) { dta_set_error("%s: floor=%g must be > 0 (kept values order by their bit patterns)", who, (double)floor); return 1; }
  const int mode = rule ? rule->mode : 0;
  if (mode < 0 || mode > 2) { dta_set_error("%s: rule mode=%d: 0 none, 1 min height, 2 height rules", who, mode); return 1; }
  if (mode == 0 && out_keep) { dta_set_error("%s: a keep buffer without a rule", who); return 1; }
  if (mode != 0 && !out_keep) { dta_set_error("%s: a rule without a keep buffer", who); return 1; }
  if (mode == 2 && !field_height) { dta_set_error("%s: height rules (mode 2) without field_height", who); return 1; }
  CrownArgs a;
  a.chm = chm; a.H = height; a.W = width; a.boxes = boxes; a.n = n;
  a.qf = q / 100.f;                                        // the reference's float32(q) / float32(100), rounded here once
  a.floor = floor; a.field = field_height; a.mode = mode;
  a.min_height = rule ? rule->min_height : 0.0;
  a.min_chm = rule ? rule->min_chm : 0.0; a.max_diff = rule ? rule->max_diff : 0.0; a.limit = rule ? rule->limit : 0.0;
  a.height = out_height; a.count = out_count; a.keep = out_keep;
  hipStream_t st = (hipStream_t)stream;
  const long long per = CH_THREADS / 64;
  const long long wg = (n + per - 1) / per;
  hipLaunchKernelGGL(k_crown_height_wave, dim3((unsigned)(wg < CH_MAX_GRID ? wg : CH_MAX_GRID)), dim3(CH_THREADS), 0, st, a);
  DTA_CHECK_LAUNCH("k_crown_height_wave");
  long long chunk = (n + CH_BLOCK_GRID - 1) / CH_BLOCK_GRID;
  chunk = chunk < CH_BLOCK_THREADS ? chunk : CH_BLOCK_THREADS;
  const long long groups = (n + chunk - 1) / chunk;
  if (groups > 0x7FFFFFFFll) { dta_set_error("%s: n=%lld: too many crowns for one launch", who, n); return 1; }
  hipLaunchKernelGGL(k_crown_height_block, dim3((unsigned)groups), dim3(CH_BLOCK_THREADS), 0, st, a, (int)chunk);
  DTA_CHECK_LAUNCH("k_crown_height_block");
  return 0;
}
