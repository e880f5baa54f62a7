// Training the alive/dead classifier from a resident image pool (reference train_dead.py, src/models/dead.py: AliveDead --
// an ImageFolder of small RGB images decoded on the main thread, ToTensor, Normalize, Resize([224, 224]) and
// RandomHorizontalFlip per step; loss F.cross_entropy(F.sigmoid(logits), y); accuracy and a confusion matrix per epoch).
// deeptreeattention_amd/dead.py holds the definitions (pool_batch_np, flips_np, loss_np).
//   k_image_pool_batch   k_rgb_crops' scheme (rgb_crops_dev.h: the same tables, row blend and store loop, so the same bits)
//                        with a per-image base, height and width from the pool's table instead of a box in one raster: the
//                        images of a batch come from an index table (or a slice of the epoch's order, read on the device),
//                        a flipped image builds its column table for S - 1 - j, and the labels go out in the same launch.
//                        At most DTA_RGB_CROPS_MAX_GROUPS workgroups, each with a contiguous share of the units; no waiting
//                        between workgroups, no private segment.
//   k_dead_loss          ONE workgroup: the loss of every row, its gradient, the confusion counts; the batch sum is a float64
//                        sum per lane in row order and a fixed tree over the lanes, so a rerun gives the same bits.  No atomics.
#include "../../include/dta_hip.h"
#include "common.h"
#include "hash_dev.h"
#include "rgb_crops_dev.h"

#pragma clang fp contract(off)

namespace dta {

constexpr int IP_MAX_GROUPS = DTA_RGB_CROPS_MAX_GROUPS;
constexpr unsigned HASH_STREAM_DEAD_FLIP = DTA_DEAD_FLIP_STREAM;

struct PoolArgs {
  const unsigned char* data; long long data_bytes;
  const long long* table;          // [n][4]: offset into data, h, w, label
  long long n; int C;
  const void* index; int index64;  // the images of the batch: int32 / int64 [start + B ..], or null for the identity
  long long start, B;
  const unsigned char* flip;       // [B] per place of the batch, or null
  int hash;                        // flips drawn from (key, base + image) instead
  unsigned long long key, base;    // stream_key(seed, HASH_STREAM_DEAD_FLIP); epoch * n mod 2^64
  int S;
  float mean[RC_MAX_CHANNELS], stdv[RC_MAX_CHANNELS];
  void* out; long long* labels;
  int rb, units;                   // output rows per unit; units per image
  long long total;                 // B * units
};

template <int FMT, bool CL, bool VEC>
__global__ __launch_bounds__(RC_THREADS) void k_image_pool_batch(PoolArgs a) {
  constexpr int VW = VEC ? 16 / (int)sizeof(typename Elem<FMT>::T) : 1;
  extern __shared__ __align__(16) unsigned char smem[];
  float* nt = (float*)smem;                                                    // [C][256] normalised byte values
  RowEntry* rowt = (RowEntry*)(smem + RC_NORM_BYTES);                          // [S]
  ColEntry* colt = (ColEntry*)(smem + RC_NORM_BYTES + (size_t)a.S * sizeof(RowEntry));   // [L]
  const int tid = threadIdx.x;
  const int S = a.S, C = a.C;
  const int L = CL ? S * C : S;
  const int planes = CL ? 1 : C;
  const size_t image_elems = (size_t)C * S * S;
  norm_table(nt, C, a.mean, a.stdv, tid);
  const LanePlace z = lane_place(L, VW, tid);
  const long long u0 = a.total * (long long)blockIdx.x / (long long)gridDim.x;
  const long long u1 = a.total * ((long long)blockIdx.x + 1) / (long long)gridDim.x;
  long long place = -1;
  bool ok = false;
  const unsigned char* ras = a.data;
  size_t plane = 0;
  for (long long u = u0; u < u1; ++u) {            // (the same for every thread of the workgroup)
    const long long n = u / a.units;               // the place in the batch
    const int unit = (int)(u - n * a.units);
    if (n != place) {
      place = n;
      __syncthreads();                             // nobody reads the previous image's tables any more
      const long long at = a.start + n;
      const long long img = !a.index ? at : a.index64 ? ((const long long*)a.index)[at] : (long long)((const int*)a.index)[at];
      ok = img >= 0 && img < a.n;
      long long label = -1;
      if (ok) {
        const long long* t = a.table + 4 * img;
        const long long off = t[0], h = t[1], w = t[2];
        // (the table is the pool's own; a row that does not lie inside the pool's bytes is written as zeros, not read)
        ok = h >= 1 && w >= 1 && h * w <= 0x7FFFFFFFll && off >= 0 && off <= a.data_bytes &&
             (long long)C * h * w <= a.data_bytes - off;
        if (ok) {
          label = t[3];
          const bool flip = a.hash ? (mix64((a.base + (unsigned long long)img) * HASH_GOLDEN + a.key) >> 40) < (1ull << 23)
                                   : a.flip ? a.flip[n] != 0 : false;
          ras = a.data + off;
          plane = (size_t)(h * w);
          build_tables<CL>(rowt, colt, S, C, L, (int)h, (int)w, 0, (int)w, flip, tid);
        }
      }
      __syncthreads();                             // (the first time round also: the normalisation table is complete)
      if (unit == 0 && tid == 0) a.labels[n] = label;          // the image's first unit belongs to one workgroup
    }
    const int i0 = unit * a.rb;
    const int i1 = i0 + a.rb < S ? i0 + a.rb : S;
    write_rows<FMT, CL, VW>(ok, ras, plane, nt, rowt, colt, a.out, (size_t)n * image_elems, i0, i1, S, L, planes, z);
  }
}

template <int FMT>
static void launch_pool(const PoolArgs& a, int cl, bool vec, unsigned groups, size_t lds, hipStream_t st) {
  if (cl) {
    if (vec) hipLaunchKernelGGL((k_image_pool_batch<FMT, true, true>), dim3(groups), dim3(RC_THREADS), lds, st, a);
    else hipLaunchKernelGGL((k_image_pool_batch<FMT, true, false>), dim3(groups), dim3(RC_THREADS), lds, st, a);
  } else {
    if (vec) hipLaunchKernelGGL((k_image_pool_batch<FMT, false, true>), dim3(groups), dim3(RC_THREADS), lds, st, a);
    else hipLaunchKernelGGL((k_image_pool_batch<FMT, false, false>), dim3(groups), dim3(RC_THREADS), lds, st, a);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
struct DeadAcc { double loss_sum; long long rows; long long conf[4]; long long bad; };
static_assert(sizeof(DeadAcc) == 8 * DTA_DEAD_ACC_WORDS, "dta_hip.h: the accumulator is DTA_DEAD_ACC_WORDS 8-byte words");

struct LossArgs { const void* logits; const long long* labels; long long rows; float* loss; float* dl; long long* counts; DeadAcc* acc; };

constexpr int DL_THREADS = 256;

// the sum of v over the workgroup, in every lane: a fixed tree
template <typename T>
__device__ __forceinline__ T group_sum(T v, T* s) {
  const int tid = threadIdx.x;
  __syncthreads();                                 // the previous sum has been read
  s[tid] = v;
  __syncthreads();
  for (int d = DL_THREADS / 2; d > 0; d >>= 1) {
    if (tid < d) s[tid] += s[tid + d];
    __syncthreads();
  }
  return s[0];
}

template <int FMT>
__global__ __launch_bounds__(DL_THREADS) void k_dead_loss(LossArgs a) {
  __shared__ double sd[DL_THREADS];
  __shared__ long long sl[DL_THREADS];
  const int tid = threadIdx.x;
  long long mine = 0;
  for (long long r = tid; r < a.rows; r += DL_THREADS) {
    const long long y = a.labels[r];
    mine += (y == 0 || y == 1) ? 1 : 0;
  }
  const long long valid = group_sum<long long>(mine, sl);
  const float bv = (float)valid;
  double sum = 0.0;
  long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;       // conf[label][argmax], flattened
  for (long long r = tid; r < a.rows; r += DL_THREADS) {       // a lane's rows in ascending order
    const long long y = a.labels[r];
    float d0 = 0.f, d1 = 0.f;
    if (y == 0 || y == 1) {
      const float l0 = ld_fmt(a.logits, (size_t)(2 * r), FMT), l1 = ld_fmt(a.logits, (size_t)(2 * r + 1), FMT);
      const float s0 = 1.f / (1.f + expf(-l0)), s1 = 1.f / (1.f + expf(-l1));
      const float m = s0 > s1 ? s0 : s1;
      const float lse = m + logf(expf(s0 - m) + expf(s1 - m));
      sum += (double)(lse - (y ? s1 : s0));
      const float p0 = expf(s0 - lse), p1 = expf(s1 - lse);
      d0 = (p0 - (y ? 0.f : 1.f)) * s0 * (1.f - s0) / bv;
      d1 = (p1 - (y ? 1.f : 0.f)) * s1 * (1.f - s1) / bv;
      const int k = 2 * (int)y + (l1 > l0 ? 1 : 0);            // a tie (and a NaN): 0, as np.argmax
      c0 += k == 0; c1 += k == 1; c2 += k == 2; c3 += k == 3;
    }
    a.dl[2 * r] = d0;
    a.dl[2 * r + 1] = d1;
  }
  const double total = group_sum<double>(sum, sd);
  const long long conf[4] = {group_sum<long long>(c0, sl), group_sum<long long>(c1, sl), group_sum<long long>(c2, sl),
                             group_sum<long long>(c3, sl)};
  if (tid == 0) {
    a.loss[0] = valid > 0 ? (float)(total / (double)valid) : 0.f;
    for (int k = 0; k < 4; ++k) a.counts[k] = conf[k];
    a.counts[4] = a.rows - valid;
    if (a.acc) {                                   // launches of one stream follow each other: a plain read-modify-write
      a.acc->loss_sum += total;
      a.acc->rows += valid;
      for (int k = 0; k < 4; ++k) a.acc->conf[k] += conf[k];
      a.acc->bad += a.rows - valid;
    }
  }
}

}  // namespace dta

using namespace dta;

extern "C" int dta_image_pool_batch(const unsigned char* data, long long data_bytes, const long long* table, long long n,
                                    int channels, const void* index, int index64, long long start, long long count,
                                    const unsigned char* flip, int hash_flips, unsigned long long seed, unsigned long long epoch,
                                    int size, const float* mean, const float* std, int dtype, int channels_last, void* out,
                                    long long* out_labels, void* stream) {
  const char* who = "dta_image_pool_batch";
  if (!data || !table || !mean || !std || !out || !out_labels) { dta_set_error("%s: null argument", who); return 1; }
  if (n < 1 || n > DTA_EPOCH_ORDER_MAX_N) { dta_set_error("%s: bad pool: n=%lld: 1..%d", who, n, DTA_EPOCH_ORDER_MAX_N); return 1; }
  if (data_bytes < 1) { dta_set_error("%s: bad pool: data_bytes=%lld", who, data_bytes); return 1; }
  if (channels < 1 || channels > RC_MAX_CHANNELS) { dta_set_error("%s: channels=%d: 1 to %d", who, channels, RC_MAX_CHANNELS); return 1; }
  if (count < 1 || count > 0x7FFFFFFFll) { dta_set_error("%s: bad shape: count=%lld (B >= 1)", who, count); return 1; }
  if (start < 0 || start > 0x7FFFFFFFll) { dta_set_error("%s: start=%lld must be >= 0", who, start); return 1; }
  if (!index && start + count > n) {
    dta_set_error("%s: start=%lld + count=%lld is past the pool's n=%lld (no index: the identity)", who, start, count, n);
    return 1;
  }
  if (flip && hash_flips) { dta_set_error("%s: flip and hash_flips exclude each other", who); return 1; }
  if (size < 1 || size > DTA_RGB_CROPS_MAX_SIZE) { dta_set_error("%s: size=%d: 1 to %d", who, size, DTA_RGB_CROPS_MAX_SIZE); return 1; }
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
  PoolArgs a;
  a.data = data; a.data_bytes = data_bytes; a.table = table; a.n = n; a.C = channels;
  a.index = index; a.index64 = index64 ? 1 : 0; a.start = start; a.B = count;
  a.flip = flip; a.hash = hash_flips ? 1 : 0;
  a.key = stream_key(seed, (unsigned long long)HASH_STREAM_DEAD_FLIP);
  a.base = epoch * (unsigned long long)n;
  a.S = size;
  for (int c = 0; c < RC_MAX_CHANNELS; ++c) { a.mean[c] = c < channels ? mean[c] : 0.f; a.stdv[c] = c < channels ? std[c] : 1.f; }
  a.out = out; a.labels = out_labels;
  a.rb = rgb_crops_rows_per_unit(count, size, channels, IP_MAX_GROUPS);
  a.units = (size + a.rb - 1) / a.rb;
  a.total = count * a.units;
  const int row_elems = size * channels;
  const int line = channels_last ? row_elems : size, vw = 16 / bytes;
  const bool vec = line % vw == 0 && (uintptr_t)out % 16 == 0;      // every line then starts on a 16-byte boundary
  const unsigned groups = (unsigned)(a.total < IP_MAX_GROUPS ? a.total : IP_MAX_GROUPS);
  const size_t lds = RC_NORM_BYTES + (size_t)size * sizeof(RowEntry) + (size_t)line * sizeof(ColEntry);   // at most 44 KiB
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DTA_ELEM_F32) launch_pool<FMT_F32>(a, channels_last, vec, groups, lds, st);
  else if (dtype == DTA_ELEM_BF16) launch_pool<FMT_BF16>(a, channels_last, vec, groups, lds, st);
  else launch_pool<FMT_F16>(a, channels_last, vec, groups, lds, st);
  DTA_CHECK_LAUNCH("k_image_pool_batch");
  return 0;
}

extern "C" int dta_dead_loss(const void* logits, int dtype, const long long* labels, long long rows, float* out_loss,
                             float* out_dlogits, long long* out_counts, void* accumulator, void* stream) {
  const char* who = "dta_dead_loss";
  if (!logits || !labels || !out_loss || !out_dlogits || !out_counts) { dta_set_error("%s: null argument", who); return 1; }
  if (rows < 1 || rows > DTA_DEAD_LOSS_MAX_ROWS) {
    dta_set_error("%s: bad shape: rows=%lld: 1..%d (B >= 1; one workgroup sums the batch)", who, rows, DTA_DEAD_LOSS_MAX_ROWS);
    return 1;
  }
  if (dtype != DTA_ELEM_F32 && dtype != DTA_ELEM_BF16 && dtype != DTA_ELEM_F16) {
    dta_set_error("%s: dtype=%d: DTA_ELEM_F32, DTA_ELEM_BF16 or DTA_ELEM_F16", who, dtype);
    return 1;
  }
  if ((uintptr_t)accumulator % 8) { dta_set_error("%s: accumulator is not aligned to 8 bytes", who); return 1; }
  LossArgs a;
  a.logits = logits; a.labels = labels; a.rows = rows; a.loss = out_loss; a.dl = out_dlogits; a.counts = out_counts;
  a.acc = (DeadAcc*)accumulator;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DTA_ELEM_F32) hipLaunchKernelGGL(k_dead_loss<FMT_F32>, dim3(1), dim3(DL_THREADS), 0, st, a);
  else if (dtype == DTA_ELEM_BF16) hipLaunchKernelGGL(k_dead_loss<FMT_BF16>, dim3(1), dim3(DL_THREADS), 0, st, a);
  else hipLaunchKernelGGL(k_dead_loss<FMT_F16>, dim3(1), dim3(DL_THREADS), 0, st, a);
  DTA_CHECK_LAUNCH("k_dead_loss");
  return 0;
}
