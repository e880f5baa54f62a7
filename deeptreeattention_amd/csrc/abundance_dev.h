// What the abundance kernels share (abundance.hip: the site totals; abundance_grid.hip: the same counts per tile or map
// cell): the launch constants, the argument struct, the plan that slices the crowns, and ONE body for a crown's draws, so
// that "a crown draws the same species whichever cell it is counted in" rests on shared code, not on two copies.
#pragma once
#include "../../include/dta_hip.h"
#include "common.h"
#include "hash_dev.h"

namespace dta {

constexpr int AB_G = 8;              // iterations per workgroup: a crown's label, score and mask byte are read once for them
constexpr int AB_THREADS = 256;
constexpr int AB_CROWNS = 1024;      // a slice is at least this long (while there are crowns) ...
constexpr int AB_WORKGROUPS = 2048;  // ... and longer once slices x iteration groups would pass this many workgroups

struct AbundanceArgs {
  const long long* label; const float* score; const unsigned char* mask; long long n;
  const unsigned* table; int S, iterations;
  unsigned long long key_keep, key_draw, first;   // the two stream keys (host: stream_key) and first_iteration
  long long per;                                  // crowns per slice
  unsigned long long* part;                       // [slices][iterations][S + 1]
};

// What a workgroup's draws depend on beyond the crown: formed ONCE per workgroup, in front of its loop over the crowns, and
// handed to ab_crown by value, so that nothing of it is read again per crown.
struct AbundanceDraw {
  const unsigned* table; int S, nt;                 // nt: the iterations of this workgroup, t0 .. t0 + nt - 1
  unsigned long long key_keep, key_draw;
  unsigned long long first_n;                       // (first + t0) * N: the counter of crown 0 in iteration t0
  unsigned long long step;                          // the counter grows by N per iteration: N * GOLDEN
};
__device__ __forceinline__ AbundanceDraw ab_draw(const AbundanceArgs& a, int t0, int nt) {
  AbundanceDraw d;
  const unsigned long long N = (unsigned long long)a.n;
  d.table = a.table; d.S = a.S; d.nt = nt; d.key_keep = a.key_keep; d.key_draw = a.key_draw;
  d.first_n = (a.first + (unsigned long long)t0) * N;
  d.step = N * HASH_GOLDEN;
  return d;
}

// Crown i (its index in the WHOLE input) in the workgroup's iterations: count(t, bin) once per iteration, t relative to t0.
// lab: its label, any value (outside [0, S): bin S whatever the score); score: where its score lies, or null: every crown
// keeps its label.
template <typename Count>
__device__ __forceinline__ void ab_crown(const AbundanceDraw d, long long i, long long lab, const float* score, Count count) {
  const int S = d.S, nt = d.nt;
  if (lab < 0 || lab >= S || !score) {                       // DEAD / unresolved: bin S; no scores: every crown keeps
    const int bin = (lab < 0 || lab >= S) ? S : (int)lab;
#pragma unroll
    for (int t = 0; t < AB_G; ++t) {                         // nt <= AB_G: peeled, a scalar test between the adds
      if (t >= nt) break;
      count(t, bin);
    }
  } else {
  const int l = (int)lab;
  const float sc = *score;
  const unsigned* row = d.table + (size_t)l * S;
  // ((first + t0 + t) * N + i) * GOLDEN, formed in 64 bits and modulo 2^64 as the mirror forms it; one addition per
  // iteration instead of hash_dev.h's draw at a counter, which would multiply again for every draw
  unsigned long long c = (d.first_n + (unsigned long long)i) * HASH_GOLDEN;
  for (int t = 0; t < nt; ++t, c += d.step) {
    const unsigned r_keep = (unsigned)(mix64(c + d.key_keep) >> 40);
    int bin = l;
    if ((float)r_keep * 0x1p-24f >= sc) {                    // exact in float32; false for a NaN score: it keeps
      const unsigned r_draw = (unsigned)(mix64(c + d.key_draw) >> 40);
      // the number of entries <= r_draw of a non-decreasing row: branch-free binary search, S is the same in every lane
      int base = 0, len = S;
      while (len > 1) {
        const int half = len >> 1;
        base = row[base + half - 1] <= r_draw ? base + half : base;
        len -= half;
      }
      bin = base + (row[base] <= r_draw ? 1 : 0);            // < S: every row ends at 2^24, above every draw
      bin = bin < S ? bin : S - 1;                           // (a table that breaks that rule cannot leave the histogram)
    }
    count(t, bin);
  }
  }
}

struct AbundancePlan { int groups, slices; long long per; size_t bytes; };

// 0 on success; the plan depends on (n, species, iterations) alone, so the workspace queries and the calls agree
static inline int ab_plan(const char* who, long long n, int species, int iterations, AbundancePlan* p) {
  if (n < 1) { dta_set_error("%s: bad shape: n=%lld", who, n); return 1; }
  if (species < 1 || species > DTA_ABUNDANCE_MAX_SPECIES) {
    dta_set_error("%s: species=%d: 1..%d (DTA_ABUNDANCE_MAX_SPECIES)", who, species, DTA_ABUNDANCE_MAX_SPECIES);
    return 1;
  }
  if (iterations < 0) { dta_set_error("%s: iterations=%d is negative", who, iterations); return 1; }
  p->groups = (iterations + AB_G - 1) / AB_G;
  const long long cap = p->groups >= AB_WORKGROUPS ? 1 : AB_WORKGROUPS / (p->groups > 0 ? p->groups : 1);
  long long slices = (n + AB_CROWNS - 1) / AB_CROWNS;
  slices = slices > cap ? cap : slices;
  p->slices = (int)slices;
  p->per = (n + slices - 1) / slices;
  if (p->per > 0xFFFFFFFFll) { dta_set_error("%s: n=%lld: too many crowns per workgroup for 32-bit bins", who, n); return 1; }
  if ((long long)iterations * (species + 1) > 0x7FFFFFFFll * AB_THREADS) { dta_set_error("%s: iterations=%d: too many for one launch", who, iterations); return 1; }
  p->bytes = sizeof(unsigned long long) * (size_t)slices * (size_t)(iterations > 0 ? iterations : 1) * (size_t)(species + 1);
  return 0;
}

}  // namespace dta
