// Species abundance with uncertainty (reference src/multinomial.py + sample_multinomial.py: 100 passes of pandas lambdas
// over every predicted crown; abundance.py: the plain count).  deeptreeattention_amd/abundance.py holds the definition
// (resample_np / counts_np); these kernels equal it bit for bit: a draw is decided by 64-bit integer arithmetic (the counter
// hash of hash_dev.h, streams HASH_STREAM_ABUNDANCE_KEEP and _DRAW) and ONE float32 comparison, the counts are integer sums.
//   k_abundance_resample  every iteration of the resampling in ONE launch: a workgroup owns a slice of crowns and a group of
//                         AB_G iterations, counts into an LDS histogram [AB_G][species + 1] and stores it whole (zeros
//                         included) as its slice's partial histogram
//   k_abundance_sum       counts[t][b] = the sum of the slices' partial histograms: a store pass and a per-destination sum
//                         pass instead of global atomics, so nothing has to be cleared and nothing is left behind
// No float atomics, no global atomics at all; the table (species^2 thresholds, 160 KB at 200 species) is left to L2.
#include "../../include/dta_hip.h"
#include "abundance_dev.h"

namespace dta {

// (the constants, AbundanceArgs, the plan and the body of a crown's draws are abundance_dev.h's: abundance_grid.hip counts
// the same draws per cell)
__global__ __launch_bounds__(AB_THREADS) void k_abundance_resample(AbundanceArgs a) {
  __shared__ unsigned hist[AB_G * (DTA_ABUNDANCE_MAX_SPECIES + 1)];
  const int bins = a.S + 1, tid = threadIdx.x;
  const int t0 = blockIdx.x * AB_G;
  const int nt = a.iterations - t0 < AB_G ? a.iterations - t0 : AB_G;
  for (int e = tid; e < nt * bins; e += AB_THREADS) hist[e] = 0u;
  __syncthreads();
  const long long i0 = (long long)blockIdx.y * a.per;
  const long long i1 = i0 + a.per < a.n ? i0 + a.per : a.n;
  const AbundanceDraw d = ab_draw(a, t0, nt);
  for (long long i = i0 + tid; i < i1; i += AB_THREADS) {
    if (a.mask && a.mask[i] == 0) continue;                  // clipped away by the caller: counted nowhere
    ab_crown(d, i, a.label[i], a.score ? a.score + i : nullptr, [&](int t, int bin) { atomicAdd(&hist[t * bins + bin], 1u); });
  }
  __syncthreads();
  unsigned long long* dst = a.part + ((size_t)blockIdx.y * a.iterations + t0) * bins;
  for (int e = tid; e < nt * bins; e += AB_THREADS) dst[e] = hist[e];
}

__global__ __launch_bounds__(AB_THREADS) void k_abundance_sum(const unsigned long long* part, int slices, long long total,
                                                              long long* counts) {
  const long long e = (long long)blockIdx.x * AB_THREADS + threadIdx.x;
  if (e >= total) return;
  unsigned long long s = 0;
  for (int k = 0; k < slices; ++k) s += part[(size_t)k * total + e];
  counts[e] = (long long)s;
}

static int ab_run(const char* who, const AbundancePlan& p, AbundanceArgs a, long long* counts, void* workspace,
                  size_t workspace_bytes, hipStream_t st) {
  if (workspace_bytes < p.bytes) { dta_set_error("%s: workspace too small: %zu bytes, %zu needed", who, workspace_bytes, p.bytes); return 1; }
  if ((uintptr_t)workspace & 7) { dta_set_error("%s: the workspace must be 8-byte aligned", who); return 1; }
  a.per = p.per; a.part = (unsigned long long*)workspace;
  hipLaunchKernelGGL(k_abundance_resample, dim3(p.groups, p.slices), dim3(AB_THREADS), 0, st, a);
  DTA_CHECK_LAUNCH("k_abundance_resample");
  const long long total = (long long)a.iterations * (a.S + 1);
  hipLaunchKernelGGL(k_abundance_sum, dim3((unsigned)((total + AB_THREADS - 1) / AB_THREADS)), dim3(AB_THREADS), 0, st,
                     (const unsigned long long*)workspace, p.slices, total, counts);
  DTA_CHECK_LAUNCH("k_abundance_sum");
  return 0;
}

}  // namespace dta

using namespace dta;

extern "C" {

size_t dta_abundance_workspace_bytes(long long n, int species, int iterations) {
  AbundancePlan p;
  if (ab_plan("dta_abundance_workspace_bytes", n, species, iterations, &p)) return 0;
  return p.bytes;
}

int dta_abundance_resample(const long long* label, const float* score, const unsigned char* mask, long long n,
                           const unsigned int* table, int species, int iterations, unsigned long long seed,
                           unsigned long long first_iteration, long long* counts, void* workspace, size_t workspace_bytes,
                           void* stream) {
  if (!label || !table || !counts || !workspace) { dta_set_error("dta_abundance_resample: null argument"); return 1; }
  AbundancePlan p;
  if (ab_plan("dta_abundance_resample", n, species, iterations, &p)) return 1;
  if (iterations == 0) return 0;                // an empty [0][species + 1]: nothing to write
  AbundanceArgs a;
  a.label = label; a.score = score; a.mask = mask; a.n = n; a.table = table; a.S = species; a.iterations = iterations;
  a.key_keep = stream_key(seed, HASH_STREAM_ABUNDANCE_KEEP); a.key_draw = stream_key(seed, HASH_STREAM_ABUNDANCE_DRAW);
  a.first = first_iteration;
  return ab_run("dta_abundance_resample", p, a, counts, workspace, workspace_bytes, (hipStream_t)stream);
}

int dta_abundance_counts(const long long* label, const unsigned char* mask, long long n, int species, long long* counts,
                         void* workspace, size_t workspace_bytes, void* stream) {
  if (!label || !counts || !workspace) { dta_set_error("dta_abundance_counts: null argument"); return 1; }
  AbundancePlan p;
  if (ab_plan("dta_abundance_counts", n, species, 1, &p)) return 1;
  AbundanceArgs a;
  a.label = label; a.score = nullptr; a.mask = mask; a.n = n; a.table = nullptr; a.S = species; a.iterations = 1;
  a.key_keep = 0; a.key_draw = 0; a.first = 0;
  return ab_run("dta_abundance_counts", p, a, counts, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
