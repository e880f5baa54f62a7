// Crown-level evaluation: the reference's experiment report (MultiStage.evaluation_scores, multi_stage.py:436-485: one pandas
// group and one torchmetrics call per site; site_confusion / genus_confusion, src/metrics.py:8-72: Python loops over every
// prediction; novel_prediction, :74-107: per-batch argmax indexing on the host) as functions of one grouped confusion table
// conf[g][t][p] = counted crowns of group g with label t and prediction p.  deeptreeattention_amd/evaluate.py holds the
// definitions (count_np, report_np, first_per_individual_np); these kernels equal them bit for bit.
//
//   k_eval_count<COMBINE>  one row per lane, a grid-stride loop.  A counted row adds one to its entry (64-bit integer atomic
//                          add: commutative, so reruns are bit-identical -- the rule of walk_dev.h).  COMBINE: the lanes of a
//                          wave that hold the same entry are added up first -- the first pending lane's key is broadcast,
//                          the ballot of the lanes that hold it is its count, that lane makes one atomic; after EV_ROUNDS
//                          rounds what is left goes out singly.  The counted / skipped tally is summed per workgroup.
//   k_eval_report          workgroup g < G reduces plane g, workgroup G the sum of all planes.  A wave owns a label row t:
//                          its lanes stride over the predictions (coalesced), the row sum is a wave sum, the column sums are
//                          LDS atomics, the off-diagonal entries whose two species share a site bit / a genus id are summed
//                          per lane.  All of that is integer, hence order-free.  Then one lane per species divides, and ONE
//                          lane adds the seen species' accuracies in class order: the definition's left-to-right sum.
//   k_first_min / k_first_mark  the lowest row of every id (integer atomic min), then the compare.
//   k_novel_scores         one wave per row on softmax_top2_row_body (top2_dev.h), the row body of dta_softmax_top2.
#include "../../include/dta_hip.h"
#include "common.h"
#include "top2_dev.h"

// every figure of the report is one division or one addition of doubles, each rounded on its own
#pragma clang fp contract(off)

namespace dta {

namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_WAVES = EV_THREADS / 64;
constexpr int EV_ROUNDS = DTA_EVAL_COMBINE_ROUNDS;
constexpr int EV_MAX_BLOCKS = 2048;            // of the counting launch: two tally atomics per workgroup
constexpr int RP_THREADS = 1024;
constexpr int RP_WAVES = RP_THREADS / 64;
constexpr int EV_S = DTA_EVAL_MAX_SPECIES;
constexpr int EV_W = DTA_EVAL_MAX_SITE_WORDS;

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ void add_ll(long long* at, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(at), (unsigned long long)v);
}

struct CountArgs {
  const long long* labels;       // [N]
  const long long* preds;        // [N]
  const void* group;             // [N] int or long long, or null
  const unsigned char* mask;     // [N] or null
  long long N, G;
  int S, group64;
  long long* conf;               // [G][S][S]
  long long* tally;              // [2]
};

template <bool COMBINE>
__global__ __launch_bounds__(EV_THREADS) void k_eval_count(CountArgs a) {
  __shared__ long long part[2][EV_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long counted = 0, skipped = 0;
  // the same trips in every lane of the workgroup: the ballots and shuffles below are met by whole waves
  for (long long base = (long long)blockIdx.x * EV_THREADS; base < a.N; base += (long long)gridDim.x * EV_THREADS) {
    const long long i = base + threadIdx.x;
    int key = -1;                                                  // the entry's index; -1: nothing to add
    if (i < a.N && (!a.mask || a.mask[i])) {
      const long long t = a.labels[i], p = a.preds[i];
      const long long g = !a.group ? 0 : (a.group64 ? ((const long long*)a.group)[i] : (long long)((const int*)a.group)[i]);
      if (t >= 0 && t < a.S && p >= 0 && p < a.S && g >= 0 && g < a.G) {
        key = (int)((g * a.S + t) * a.S + p);                      // (< 2^31: the host's size rule)
        ++counted;
      } else {
        ++skipped;
      }
    }
    if (COMBINE) {
      unsigned long long pending = __ballot(key >= 0);
#pragma unroll
      for (int r = 0; r < EV_ROUNDS; ++r) {
        if (!pending) break;                                       // (wave-uniform)
        const int first = __ffsll(pending) - 1;
        const int k = __shfl(key, first);
        const unsigned long long same = __ballot(key == k) & pending;
        if (lane == first) add_ll(a.conf + k, __popcll(same));
        pending &= ~same;
      }
      if ((pending >> lane) & 1ull) add_ll(a.conf + key, 1);
    } else {
      if (key >= 0) add_ll(a.conf + key, 1);
    }
  }
  counted = wave_sum_ll(counted); skipped = wave_sum_ll(skipped);
  if (lane == 0) { part[0][wave] = counted; part[1][wave] = skipped; }
  __syncthreads();
  if (threadIdx.x < 2) {
    long long s = 0;
#pragma unroll
    for (int w = 0; w < EV_WAVES; ++w) s += part[threadIdx.x][w];
    if (s) add_ll(a.tally + threadIdx.x, s);
  }
}

struct ReportArgs {
  const long long* conf;               // [G][S][S]
  int S, W;
  long long G;
  const unsigned long long* sites;     // [S][W] or null
  const int* genus;                    // [S] or null
  long long* counts;                   // [G + 1][8]
  double* scores;                      // [G + 1][4]
  double* accuracy;                    // [G + 1][S] or null, with precision and support
  double* precision;
  long long* support;
};

__global__ __launch_bounds__(RP_THREADS) void k_eval_report(ReportArgs a) {
  __shared__ long long s_rows[EV_S], s_cols[EV_S], s_diag[EV_S];
  __shared__ double s_acc[EV_S];
  __shared__ long long s_part[5][RP_WAVES];
  const int S = a.S, W = a.W;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long g = blockIdx.x;
  const bool pooled = g == a.G;
  const size_t plane = (size_t)S * S;
  const long long* base = a.conf + (pooled ? 0 : (size_t)g * plane);
  const long long planes = pooled ? a.G : 1;
  for (int t = tid; t < S; t += RP_THREADS) { s_cols[t] = 0; s_diag[t] = 0; }
  __syncthreads();
  long long ws = 0, wg = 0;                                        // errors within a site / within a genus, this lane's
  for (int t = wave; t < S; t += RP_WAVES) {                       // (t is wave-uniform)
    unsigned long long m0 = 0, m1 = 0, m2 = 0, m3 = 0;             // the label's site bits (named: no indexed array)
    if (a.sites) {
      const unsigned long long* m = a.sites + (size_t)t * W;
      m0 = m[0]; m1 = W > 1 ? m[1] : 0; m2 = W > 2 ? m[2] : 0; m3 = W > 3 ? m[3] : 0;
    }
    const int gt = a.genus ? a.genus[t] : 0;
    long long rs = 0;
#pragma unroll 1
    for (int p = lane; p < S; p += 64) {
      const long long* at = base + (size_t)t * S + p;
      long long v = 0;
#pragma unroll 4
      for (long long k = 0; k < planes; ++k) v += at[(size_t)k * plane];
      if (v == 0) continue;
      rs += v;
      add_ll(&s_cols[p], v);
      if (p == t) { s_diag[t] = v; continue; }
      if (a.sites) {
        const unsigned long long* m = a.sites + (size_t)p * W;
        unsigned long long both = m0 & m[0];
        if (W > 1) both |= m1 & m[1];
        if (W > 2) both |= m2 & m[2];
        if (W > 3) both |= m3 & m[3];
        if (both) ws += v;
      }
      if (a.genus && a.genus[p] == gt) wg += v;
    }
    rs = wave_sum_ll(rs);
    if (lane == 0) s_rows[t] = rs;
  }
  __syncthreads();
  long long tot = 0, cor = 0, seen = 0;
  for (int t = tid; t < S; t += RP_THREADS) {
    const long long r = s_rows[t], c = s_cols[t], d = s_diag[t];
    tot += r; cor += d; seen += r > 0;
    const double acc = r > 0 ? (double)d / (double)r : 0.0;
    const double pre = c > 0 ? (double)d / (double)c : 0.0;
    s_acc[t] = acc;
    if (a.accuracy) {
      const size_t o = (size_t)g * S + t;
      a.accuracy[o] = acc; a.precision[o] = pre; a.support[o] = r;
    }
  }
  tot = wave_sum_ll(tot); cor = wave_sum_ll(cor); seen = wave_sum_ll(seen); ws = wave_sum_ll(ws); wg = wave_sum_ll(wg);
  if (lane == 0) { s_part[0][wave] = tot; s_part[1][wave] = cor; s_part[2][wave] = seen; s_part[3][wave] = ws; s_part[4][wave] = wg; }
  __syncthreads();
  if (tid != 0) return;
  tot = cor = seen = ws = wg = 0;
#pragma unroll 2
  for (int w = 0; w < RP_WAVES; ++w) {
    tot += s_part[0][w]; cor += s_part[1][w]; seen += s_part[2][w]; ws += s_part[3][w]; wg += s_part[4][w];
  }
  double sum = 0.0;                                                // left to right, in class order: the definition's cumsum
#pragma unroll 4
  for (int t = 0; t < S; ++t)
    if (s_rows[t] > 0) sum += s_acc[t];
  const long long wrong = tot - cor;
  long long* c = a.counts + g * 8;
  c[0] = tot; c[1] = cor; c[2] = wrong;
  c[3] = a.sites ? ws : 0; c[4] = a.sites ? wrong - ws : 0;
  c[5] = a.genus ? wg : 0; c[6] = a.genus ? wrong - wg : 0;
  c[7] = seen;
  double* s = a.scores + g * 4;
  s[0] = tot > 0 ? (double)cor / (double)tot : 0.0;
  s[1] = seen > 0 ? sum / (double)seen : 0.0;
  s[2] = a.sites && wrong > 0 ? (double)ws / (double)wrong : 0.0;
  s[3] = a.genus && wrong > 0 ? (double)wg / (double)wrong : 0.0;
}

__device__ __forceinline__ long long id_at(const void* ids, int ids64, long long i) {
  return ids64 ? ((const long long*)ids)[i] : (long long)((const int*)ids)[i];
}

__global__ __launch_bounds__(EV_THREADS) void k_first_min(const void* ids, int ids64, long long N, long long I, int* first) {
  const long long i = (long long)blockIdx.x * EV_THREADS + threadIdx.x;
  if (i >= N) return;
  const long long id = id_at(ids, ids64, i);
  if (id >= 0 && id < I) atomicMin(&first[id], (int)i);
}

__global__ __launch_bounds__(EV_THREADS) void k_first_mark(const void* ids, int ids64, long long N, long long I, const int* first,
                                                           unsigned char* out) {
  const long long i = (long long)blockIdx.x * EV_THREADS + threadIdx.x;
  if (i >= N) return;
  const long long id = id_at(ids, ids64, i);
  out[i] = id >= 0 && id < I && first[id] == (int)i;
}

__global__ __launch_bounds__(EV_THREADS) void k_novel_scores(const float* logits, long long N, int classes, long long* label,
                                                             float* top, float* soft) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * EV_WAVES + (threadIdx.x >> 6);
  if (row >= N) return;                                            // (a whole wave)
  const float* z = logits + (size_t)row * classes;
  const auto zat = [&](int n) __attribute__((always_inline)) { return z[n]; };
  const SoftmaxRow r = softmax_top2_row_body(classes, lane, zat, [&](int, float, float) __attribute__((always_inline)) {});
  bool bad = false;                                                // a NaN among this lane's classes: torch's max gives NaN
  softmax_row_each(r, classes, lane, zat, [&](int, float v) __attribute__((always_inline)) { bad |= v != v; });
  const bool any_bad = __ballot(bad) != 0ull;
  if (lane == 0) {
    label[row] = r.i1;
    soft[row] = r.b1;
    top[row] = any_bad ? __int_as_float(0x7fc00000) : r.mx;
  }
}

bool ev_sizes_ok(int S, long long G) {
  return S >= 1 && S <= EV_S && G >= 1 && G <= 0x7FFFFFFFll / ((long long)S * S);
}

}  // namespace

}  // namespace dta

using namespace dta;

extern "C" {

int dta_eval_count(const long long* labels, const long long* preds, const void* group, int group_is_64,
                   const unsigned char* mask, long long rows, int n_species, long long groups, int form, long long* conf,
                   long long* tally, void* stream) {
  const char* who = "dta_eval_count";
  if (!labels || !preds || !conf || !tally) { dta_set_error("%s: null argument", who); return 1; }
  if (rows < 1 || rows > 0x7FFFFFFFll) { dta_set_error("%s: bad shape: rows=%lld (1 .. 2^31 - 1)", who, rows); return 1; }
  if (n_species < 1 || n_species > EV_S) {
    dta_set_error("%s: bad shape: n_species=%d (1 .. %d)", who, n_species, EV_S);
    return 1;
  }
  if (!ev_sizes_ok(n_species, groups)) {
    dta_set_error("%s: bad shape: groups=%lld (>= 1, groups * n_species * n_species <= 2^31 - 1)", who, groups);
    return 1;
  }
  if (form != DTA_EVAL_COUNT_PLAIN && form != DTA_EVAL_COUNT_COMBINE) {
    dta_set_error("%s: form=%d: DTA_EVAL_COUNT_PLAIN or DTA_EVAL_COUNT_COMBINE", who, form);
    return 1;
  }
  CountArgs a;
  a.labels = labels; a.preds = preds; a.group = group; a.mask = mask; a.N = rows; a.G = groups; a.S = n_species;
  a.group64 = group_is_64 != 0; a.conf = conf; a.tally = tally;
  const long long need = (rows + EV_THREADS - 1) / EV_THREADS;
  const unsigned nb = (unsigned)(need < EV_MAX_BLOCKS ? need : EV_MAX_BLOCKS);
  hipStream_t st = (hipStream_t)stream;
  if (form == DTA_EVAL_COUNT_COMBINE) hipLaunchKernelGGL(k_eval_count<true>, dim3(nb), dim3(EV_THREADS), 0, st, a);
  else hipLaunchKernelGGL(k_eval_count<false>, dim3(nb), dim3(EV_THREADS), 0, st, a);
  DTA_CHECK_LAUNCH("k_eval_count");
  return 0;
}

int dta_eval_report(const long long* conf, int n_species, long long groups, const unsigned long long* site_masks,
                    int site_words, const int* genus, long long* counts, double* scores, double* accuracy,
                    double* precision, long long* support, void* stream) {
  const char* who = "dta_eval_report";
  if (!conf || !counts || !scores) { dta_set_error("%s: null argument", who); return 1; }
  if (n_species < 1 || n_species > EV_S) {
    dta_set_error("%s: bad shape: n_species=%d (1 .. %d)", who, n_species, EV_S);
    return 1;
  }
  if (!ev_sizes_ok(n_species, groups)) {
    dta_set_error("%s: bad shape: groups=%lld (>= 1, groups * n_species * n_species <= 2^31 - 1)", who, groups);
    return 1;
  }
  if (site_masks && (site_words < 1 || site_words > EV_W)) {
    dta_set_error("%s: bad shape: site_words=%d (1 .. %d)", who, site_words, EV_W);
    return 1;
  }
  if ((accuracy != nullptr) != (precision != nullptr) || (accuracy != nullptr) != (support != nullptr)) {
    dta_set_error("%s: accuracy, precision and support go together: all three or none", who);
    return 1;
  }
  ReportArgs a;
  a.conf = conf; a.S = n_species; a.W = site_masks ? site_words : 0; a.G = groups; a.sites = site_masks; a.genus = genus;
  a.counts = counts; a.scores = scores; a.accuracy = accuracy; a.precision = precision; a.support = support;
  hipLaunchKernelGGL(k_eval_report, dim3((unsigned)(groups + 1)), dim3(RP_THREADS), 0, (hipStream_t)stream, a);
  DTA_CHECK_LAUNCH("k_eval_report");
  return 0;
}

int dta_first_rows(const void* ids, int ids_is_64, long long rows, long long n_ids, unsigned char* first_out, int* workspace,
                   void* stream) {
  const char* who = "dta_first_rows";
  if (!ids || !first_out || !workspace) { dta_set_error("%s: null argument", who); return 1; }
  if (rows < 1 || rows > 0x7FFFFFFFll) { dta_set_error("%s: bad shape: rows=%lld (1 .. 2^31 - 1)", who, rows); return 1; }
  if (n_ids < 1 || n_ids > 0x7FFFFFFFll) { dta_set_error("%s: bad shape: n_ids=%lld (1 .. 2^31 - 1)", who, n_ids); return 1; }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetD32Async((hipDeviceptr_t)workspace, 0x7FFFFFFF, (size_t)n_ids, st) != hipSuccess) {
    dta_set_error("%s: fill failed", who);
    return 1;
  }
  const unsigned nb = (unsigned)((rows + EV_THREADS - 1) / EV_THREADS);
  hipLaunchKernelGGL(k_first_min, dim3(nb), dim3(EV_THREADS), 0, st, ids, ids_is_64 != 0, rows, n_ids, workspace);
  DTA_CHECK_LAUNCH("k_first_min");
  hipLaunchKernelGGL(k_first_mark, dim3(nb), dim3(EV_THREADS), 0, st, ids, ids_is_64 != 0, rows, n_ids, (const int*)workspace,
                     first_out);
  DTA_CHECK_LAUNCH("k_first_mark");
  return 0;
}

int dta_novel_scores(const float* logits, long long rows, int classes, long long* label_out, float* top_out,
                     float* softmax_out, void* stream) {
  const char* who = "dta_novel_scores";
  if (!logits || !label_out || !top_out || !softmax_out) { dta_set_error("%s: null argument", who); return 1; }
  if (rows < 1 || rows > 0x7FFFFFFFll) { dta_set_error("%s: bad shape: rows=%lld (1 .. 2^31 - 1)", who, rows); return 1; }
  if (classes < 1 || classes > EV_S) { dta_set_error("%s: bad shape: classes=%d (1 .. %d)", who, classes, EV_S); return 1; }
  const unsigned nb = (unsigned)((rows + EV_WAVES - 1) / EV_WAVES);
  hipLaunchKernelGGL(k_novel_scores, dim3(nb), dim3(EV_THREADS), 0, (hipStream_t)stream, logits, rows, classes, label_out,
                     top_out, softmax_out);
  DTA_CHECK_LAUNCH("k_novel_scores");
  return 0;
}

}  // extern "C"
