// Dense per-pixel window prediction over a hyperspectral raster (reference src/patches.py:50-83 `bounds_to_pixel`: one
// 11x11 window per pixel of a crown box, read boundless; src/main.py:165-178).  The reference's preprocessing is per
// pixel position (drop bands, min-max over the bands of that pixel, src/utils.py:36-57) and an SxS window resized to SxS
// with NEAREST is the identity, so the preprocessed window IS the window of the preprocessed raster:
//   k_raster_normalise  the raw raster once -> the resident normalised raster (float32 planes, or bf16 channel chunks)
//   k_gather[_tiles]<SRC_WINDOW>  N window origins -> the float32 NCHW batch / the first conv's bf16 tiles (pure copies, zero
//                                 fill); launches and errors are named k_gather_windows[_tiles]
//   k_crown_reduce      per-window softmax rows, grouped by crown -> mean vector, its top-2 and the window count
// and for a multi-stage model (levels x years networks on the same windows, engine.MultiStagePredictor):
//   k_gather_years<SRC_WINDOW>  one batch of windows out of every year's raster in ONE launch, with the years' 0/1 flags
//                               (k_gather_windows_years)
//   k_crown_resolve         every level's per-crown mean and top-2, the hierarchy walk on them and the crown's window votes
// and for the reference's production path (one crop per crown box, resized to SxS with NEAREST; src/patches.py:5-30):
//   k_gather[_tiles|_years]<SRC_CROP>  N boxes -> the resized crops, an index selection from the resident raster: the SAME
//                                      three kernels with another source policy (k_gather_crops[_tiles|_years])
// All are bandwidth-bound copies or short reductions: no float atomics, fixed summation order, bit-identical reruns.
#include "../../include/dta_hip.h"
#include "kernels.h"
#include "top2_dev.h"
#include "walk_dev.h"

// k_raster_normalise scales through common.h's minmax_* helpers, as k_preprocess_crops* (preprocess.hip) and
// k_reflectance_normalise (reflectance.hip) do: the multiply and the add are rounded SEPARATELY, as NumPy's
// `X *= scale; X += min` does
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
  float s, m;
  minmax_scale(lo, hi, &s, &m);
  if (!TILES) {
    float* out = reinterpret_cast<float*>(a.out) + p;
#pragma unroll 8
    for (int c = 0; c < C; ++c) out[(size_t)c * a.P] = minmax_apply(to_f(src[(size_t)c * a.P]), s, m);
  } else {
    const int NC = (C + 15) / 16;
    unsigned short* out = reinterpret_cast<unsigned short*>(a.out);
    for (int ch = 0; ch < NC; ++ch)
      minmax_store_chunk(out, (size_t)a.P, (size_t)p, ch, C, s, m, [&](int c) { return to_f(src[(size_t)c * a.P]); });
  }
}

// ---- the gathers: ONE body over a compile-time source policy.  An item is a window origin or a crown box; a policy loads
// item n and says which raster offset output pixel (i, j) of it reads, or false: nothing to read, the output is zero (a position
// off the raster, an empty box).  Every read is guarded, whatever the item says; offsets into the raster are 64-bit.
template <GatherSrc P> struct Src;
// windows: output pixel (i, j) of the window at origin (row, col) is raster pixel (row + i, col + j) -- a pure copy
template <> struct Src<SRC_WINDOW> {
  long long row0, col0;
  __device__ __forceinline__ Src(const GatherArgs& a, int n) : row0(a.items[2 * n]), col0(a.items[2 * n + 1]) {}
  __device__ __forceinline__ bool at(const GatherArgs& a, int i, int j, size_t* off) const {
    const long long rr = row0 + i, cc = col0 + j;
    if (rr < 0 || rr >= a.H || cc < 0 || cc >= a.W) return false;
    *off = (size_t)rr * a.W + (size_t)cc;
    return true;
  }
};
// crops: a crown's box cut out of the raster and resized to S x S with NEAREST (reference src/patches.py:5-30 `crop`,
// src/utils.py:59-79 `load_image`).  The normalisation is per pixel position and a NEAREST resize only selects pixels, so
// the resized, preprocessed crop of a box is an index selection from the normalised raster: output pixel (i, j) reads
// raster pixel (row0 + nearest_src(i, h, S), col0 + nearest_src(j, w, S)) -- nearest_src (common.h) is the very function
// k_preprocess_crops resizes with, which is what makes the two bit-identical.  flip: output (i, j) takes the resized
// pixel (S - 1 - i, S - 1 - j), both training flips (src/augmentation.py:13-14), as k_preprocess_crops applies them.
// A box with no rows or no columns: an all-zero crop (the dataset's fill for a missing crop, data.py:295-296).
template <> struct Src<SRC_CROP> {
  long long row0, col0; int h, w; float sh, sw;
  __device__ __forceinline__ Src(const GatherArgs& a, int n) {
    const int* b = a.items + (size_t)n * 4;
    const int r0 = b[0], c0 = b[1], r1 = b[2], c1 = b[3];
    row0 = r0; col0 = c0;
    h = (int)((unsigned)r1 - (unsigned)r0); w = (int)((unsigned)c1 - (unsigned)c0);      // (a side past 2^31 wraps: guarded reads)
    sh = nearest_scale(h, a.S); sw = nearest_scale(w, a.S);
  }
  __device__ __forceinline__ bool at(const GatherArgs& a, int i, int j, size_t* off) const {
    if (h <= 0 || w <= 0) return false;
    if (a.flip) { i = a.S - 1 - i; j = a.S - 1 - j; }
    const long long rr = row0 + nearest_at(i, sh, h), cc = col0 + nearest_at(j, sw, w);
    if (rr < 0 || rr >= a.H || cc < 0 || cc >= a.W) return false;
    *off = (size_t)rr * a.W + (size_t)cc;
    return true;
  }
};

// float32 NCHW batch [N][C][S][S] out of the float32 raster [C][H][W].  The batch is one flat array; a lane owns four
// consecutive elements of it (one 16-byte store; an item's C*S*S floats are not a multiple of four, so a lane's four may
// straddle rows, planes or items: the index is decomposed once and carried, and a lane that steps into the next item
// loads that item).  The same lane writes the same bytes in k_gather and k_gather_years.
// Returns whether any of the lane's elements is non-zero (NaN counts as non-zero).
template <GatherSrc P>
__device__ __forceinline__ bool gather_lane(const GatherArgs& a, size_t q4) {
  const size_t total = (size_t)a.N * a.C * a.S * a.S;
  const size_t e = q4 * 4;
  if (e >= total) return false;
  const int S = a.S, SS = S * S;
  const size_t per = (size_t)a.C * SS;
  int n = (int)(e / per);
  int r = (int)(e - (size_t)n * per);
  int c = r / SS, q = r - c * SS;
  int i = q / S, j = q - i * S;
  const float* ras = reinterpret_cast<const float*>(a.raster);
  const size_t plane = (size_t)a.H * a.W;
  Src<P> it(a, n);
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = 0.f;
    if (e + k < total) {
      size_t src;
      if (it.at(a, i, j, &src)) v[k] = ras[(size_t)c * plane + src];
      if (++j == S) {
        j = 0;
        if (++i == S) {
          i = 0;
          if (++c == a.C) {
            c = 0; ++n;
            if (n < a.N) it = Src<P>(a, n);
          }
        }
      }
    }
  }
  float* out = reinterpret_cast<float*>(a.out);
  if (e + 4 <= total) *reinterpret_cast<f32x4*>(out + e) = f32x4{v[0], v[1], v[2], v[3]};
  else for (int k = 0; e + k < total; ++k) out[e + k] = v[k];
  return !(v[0] == 0.f && v[1] == 0.f && v[2] == 0.f && v[3] == 0.f);
}
template <GatherSrc P>
__global__ __launch_bounds__(256) void k_gather(GatherArgs a) {
  gather_lane<P>(a, (size_t)blockIdx.x * 256 + threadIdx.x);
}

// The same batch of items out of every year's raster of an ensemble: blockIdx.y = year, every year the lanes and bytes of
// k_gather.  A year without a raster (NULL) writes nothing: its batch is the caller's persistent zero buffer.
// flags[y] = 1 when year y's batch has a non-zero element (NaN counts), else it stays 0 -- what k_year_flags (heads.hip)
// says after reading the finished batch back, here from the values on their way out: a wave that wrote a non-zero element
// stores 1.f once (plain stores of one value: no atomics, any order).  flags arrive zeroed; clear_next is the bank the
// NEXT call sets (dta_year_flags' protocol).
template <GatherSrc P>
__global__ __launch_bounds__(256) void k_gather_years(GatherYearsArgs a) {
  const int y = blockIdx.y;
  if (a.clear_next && blockIdx.x == 0 && threadIdx.x == 0) a.clear_next[y] = 0.f;
  if (!a.rasters[y]) return;
  GatherArgs g = a.g;
  g.raster = a.rasters[y]; g.out = a.outs[y];
  const bool hit = gather_lane<P>(g, (size_t)blockIdx.x * 256 + threadIdx.x);
  const bool any = __any(hit);
  if (any && (threadIdx.x & 63) == 0) a.flags[y] = 1.f;
}

// The first conv's bf16 tiles [N][NC][S*S][16] (preprocess.PatchTiles) out of the bf16 raster [NC][P][16]: an element
// (item, chunk, pixel) is a 32-byte copy; a lane moves one 16-byte half of it, consecutive lanes consecutive halves, so
// the stores of a wave are one contiguous run and its loads runs of S pixels (32 * S bytes) of a raster row for a window,
// the selected pixels of the box's rows for a crop (an upsampled box: the same 32 bytes several times).
template <GatherSrc P>
__global__ __launch_bounds__(256) void k_gather_tiles(GatherArgs a) {
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
  u32x4 v = u32x4{0u, 0u, 0u, 0u};
  size_t src;
  if (Src<P>(a, n).at(a, i, j, &src)) {
    const size_t plane = (size_t)a.H * a.W;
    v = reinterpret_cast<const u32x4*>(a.raster)[((size_t)ch * plane + src) * 2 + half];
  }
  reinterpret_cast<u32x4*>(a.out)[id] = v;
}


// One workgroup per crown.  A thread owns classes t, t + 256, ...: it adds the crown's rows of that class in row order
// (one float32 accumulator, no atomics, no tree: the order is the definition, dense.crown_reduce_np) and divides by the
// count.  Top-2 of the mean as every epilogue takes it (top2_take, top2_dev.h: ties go to the lower class).
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
    top2_take(mv, c, b1, i1, b2, i2);
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

// Every level's k_crown_reduce, the walk on the levels' top-1 (k_hierarchy_resolve) and the crown's window votes in ONE
// launch: workgroup = crown, wave = level (as k_softmax_top2_ensemble: the levels' top-1 of a crown meet in LDS behind one
// barrier, where the first eight lanes walk the table).  A lane owns classes lane, lane + 64, ... of its level: the same
// single float32 accumulator over the crown's rows in row order and the same division as k_crown_reduce, so the mean is
// that kernel's bit for bit; the top-2 is the two largest under (value descending, class ascending), which does not depend
// on how the classes are dealt to lanes.  votes: the workgroup zeroes its own row, then counts its windows' labels into it
// with integer adds (order-independent).
__global__ __launch_bounds__(64 * BLEND_CE_MULTI_MAX) void k_crown_resolve(CrownResolveArgs a) {
  __shared__ int s_cls[BLEND_CE_MULTI_MAX];
  __shared__ float s_score[BLEND_CE_MULTI_MAX];
  const int lane = threadIdx.x & 63, lvl = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), k = blockIdx.x;
  const long long r0 = a.offsets[k], r1 = a.offsets[k + 1];
  const long long cnt = r1 > r0 ? r1 - r0 : 0;
  if (a.votes) {
    int* row = a.votes + (size_t)k * a.e.n_species;
    for (int s = threadIdx.x; s < a.e.n_species; s += blockDim.x) row[s] = 0;
    __threadfence();                                  // the zeros are in place before any wave of this workgroup adds
  }
  {
    const CrownLevel& L = a.lv[lvl];
    const int classes = L.classes;
    float* mean = L.mean ? L.mean + (size_t)k * classes : nullptr;
    const float fc = (float)cnt;
    float b1 = -1.f, b2 = -1.f;
    int i1 = -1, i2 = -1;
    for (int c = lane; c < classes; c += 64) {
      float mv = 0.f;
      if (cnt > 0) {
        const float* src = L.probs + (size_t)r0 * classes + c;
        float acc = 0.f;
        long long r = 0;
        for (; r + 4 <= cnt; r += 4) {      // four loads in flight, added in row order
          const float v0 = src[(size_t)r * classes], v1 = src[(size_t)(r + 1) * classes];
          const float v2 = src[(size_t)(r + 2) * classes], v3 = src[(size_t)(r + 3) * classes];
          acc += v0; acc += v1; acc += v2; acc += v3;
        }
        for (; r < cnt; ++r) acc += src[(size_t)r * classes];
        mv = acc / fc;
        top2_take(mv, c, b1, i1, b2, i2);
      }
      if (mean) mean[c] = mv;               // an empty crown: mean 0, labels -1, scores 0
    }
    top2_wave_merge(b1, i1, b2, i2);
    const float t1 = i1 < 0 ? 0.f : b1, t2 = i2 < 0 ? 0.f : b2;
    if (lane == 0) {
      L.top_idx[2 * (size_t)k] = i1; L.top_idx[2 * (size_t)k + 1] = i2;
      L.top_score[2 * (size_t)k] = t1; L.top_score[2 * (size_t)k + 1] = t2;
      s_cls[lvl] = i1; s_score[lvl] = t1;
    }
  }
  __syncthreads();
  if (a.votes) {
    int* row = a.votes + (size_t)k * a.e.n_species;
    for (long long r = threadIdx.x; r < cnt; r += blockDim.x) {
      const long long s = a.win_label[r0 + r];
      if (s >= 0 && s < a.e.n_species) atomicAdd(row + s, 1);
    }
  }
  if (threadIdx.x >= 64) return;
  if (lane == 0) a.count[k] = (int)cnt;
  const bool mine = lane < a.n;
  hierarchy_walk(a.e, a.n, k, lane < 8, lane, mine ? s_cls[lane & 7] : -1, mine ? s_score[lane & 7] : 0.f);
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

// One launcher per form.  who: the kernel's name, "k_gather_windows" ...; the C entry point's is "dta_" + who from its third
// character on.  lanes: one per 16 bytes of output.
template <GatherSrc P>
int launch_gather(const GatherArgs& a, hipStream_t st) {
  const char* who = P == SRC_WINDOW ? "k_gather_windows" : "k_gather_crops";
  const size_t total = (size_t)a.N * a.C * a.S * a.S, lanes = (total + 3) / 4;
  const size_t blocks = (lanes + 255) / 256;
  if (blocks > 0x7FFFFFFFull) { dta_set_error("dta_%s: batch too large for one launch", who + 2); return 1; }
  hipLaunchKernelGGL(k_gather<P>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  DTA_CHECK_LAUNCH(who);
  return 0;
}

template <GatherSrc P>
int launch_gather_years(const GatherYearsArgs& a, hipStream_t st) {
  const char* who = P == SRC_WINDOW ? "k_gather_windows_years" : "k_gather_crops_years";
  const size_t total = (size_t)a.g.N * a.g.C * a.g.S * a.g.S, lanes = (total + 3) / 4;
  const size_t blocks = (lanes + 255) / 256;
  if (blocks > 0x7FFFFFFFull) { dta_set_error("dta_%s: batch too large for one launch", who + 2); return 1; }
  if (a.years < 1 || a.years > MAXG) { dta_set_error("dta_%s: 1..%d years", who + 2, MAXG); return 1; }
  // flags must be zero on entry: cleared here, unless the caller alternates two banks and lets each call clear the other
  if (!a.clear_next && hipMemsetAsync(a.flags, 0, sizeof(float) * a.years, st) != hipSuccess) { dta_set_error("dta_%s: memset failed", who + 2); return 1; }
  hipLaunchKernelGGL(k_gather_years<P>, dim3((unsigned)blocks, a.years), dim3(256), 0, st, a);
  DTA_CHECK_LAUNCH(who);
  return 0;
}

template <GatherSrc P>
int launch_gather_tiles(const GatherArgs& a, hipStream_t st) {
  const char* who = P == SRC_WINDOW ? "k_gather_windows_tiles" : "k_gather_crops_tiles";
  const size_t total = (size_t)a.N * ((a.C + 15) / 16) * a.S * a.S * 2;
  const size_t blocks = (total + 255) / 256;
  if (blocks > 0x7FFFFFFFull) { dta_set_error("dta_%s: batch too large for one launch", who + 2); return 1; }
  hipLaunchKernelGGL(k_gather_tiles<P>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  DTA_CHECK_LAUNCH(who);
  return 0;
}

template int launch_gather<SRC_WINDOW>(const GatherArgs&, hipStream_t);
template int launch_gather<SRC_CROP>(const GatherArgs&, hipStream_t);
template int launch_gather_years<SRC_WINDOW>(const GatherYearsArgs&, hipStream_t);
template int launch_gather_years<SRC_CROP>(const GatherYearsArgs&, hipStream_t);
template int launch_gather_tiles<SRC_WINDOW>(const GatherArgs&, hipStream_t);
template int launch_gather_tiles<SRC_CROP>(const GatherArgs&, hipStream_t);


int launch_crown_reduce(const CrownArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_crown_reduce, dim3(a.n_crowns), dim3(256), 1024 * 4, st, a);
  DTA_CHECK_LAUNCH("k_crown_reduce");
  return 0;
}

int launch_crown_resolve(const CrownResolveArgs& a, hipStream_t st) {
  if (a.n < 1 || a.n > BLEND_CE_MULTI_MAX) { dta_set_error("dta_crown_resolve: 1..%d levels", BLEND_CE_MULTI_MAX); return 1; }
  hipLaunchKernelGGL(k_crown_resolve, dim3(a.n_crowns), dim3(64 * a.n), 0, st, a);
  DTA_CHECK_LAUNCH("k_crown_resolve");
  return 0;
}

}  // namespace dta
