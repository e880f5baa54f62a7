// Device code shared by every prediction / validation epilogue (heads.hip: k_mean_scores, k_softmax_top2, k_softmax_top2_multi,
// k_softmax_top2_ensemble, k_eval_metrics_multi; meta.hip: k_meta_fuse_top2; dense.hip: k_crown_reduce, k_crown_resolve): the mean
// over the kept sources, the softmax of one row of class scores by one wave, and the top-2 under ONE rule -- value descending,
// class ascending, index -1 = empty.  ONE definition each, so that the bit equality the tests claim between these epilogues
// (one-chain prediction against per-level predictors, crown kernels against each other) rests on shared code.
#pragma once
#include "kernels.h"

namespace dta {

// ---- mean over the kept sources (year ensemble, reference year.py:33) -------------------------------------------------
// bit k of use: source k takes part (a bit mask: an indexed array would live in scratch); gate NULL = all nsrc sources
struct KeptSources { unsigned use; float kept, inv; };
__device__ __forceinline__ KeptSources kept_sources(int nsrc, const float* gate) {
  KeptSources s = {0u, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < MAXG; ++k)
    if (k < nsrc && (!gate || gate[k] > 0.f)) { s.use |= 1u << k; s.kept += 1.f; }
  s.inv = 1.f / s.kept;                               // nothing kept: inf, and 0 * inf = NaN below -- an empty mean
  return s;
}
// element i of the mean: the kept sources summed in source order, times 1 / kept
__device__ __forceinline__ float kept_mean(const KeptSources& s, const float* const* src, size_t i) {
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < MAXG; ++k)
    if ((s.use >> k) & 1u) acc += src[k][i];          // (selected, not multiplied: a skipped source's scores may be anything)
  return acc * s.inv;
}

// ---- top-2 ------------------------------------------------------------------------------------------------------------
// A (best, second) pair starts empty, (-1, index -1) twice, and takes candidates one by one: strictly greater replaces, so of
// equal values the one offered first stays (callers offer classes in ascending order) and a NaN is never taken.
// (written as selects: as `if (v > b1) { ... } else if (v > b2) { ... }` on reference parameters the compare-and-replace
//  turns into stores through a selected pointer, and the caller's pair lives in the private segment)
__device__ __forceinline__ void top2_take(float v, int n, float& b1, int& i1, float& b2, int& i2) {
  const bool first = v > b1, second = v > b2;
  b2 = first ? b1 : (second ? v : b2); i2 = first ? i1 : (second ? n : i2);
  b1 = first ? v : b1; i1 = first ? n : i1;
}
// The order of two slots: value descending, index ascending, index -1 (empty) last.  On the states top2_take can leave --
// a taken slot holds a value > -1 (never NaN) and an index >= 0, an empty one exactly (-1, -1) -- this is the same function
// as `ia >= 0 && (ib < 0 || a > b || (a == b && ia < ib))`, the form k_crown_resolve used to spell: taken against taken
// both read a > b || (a == b && ia < ib); taken against empty is true by a > -1 here and by ib < 0 there; empty against
// taken is false by -1 < b here and by ia < 0 there; empty against empty is false in both.
__device__ __forceinline__ bool top2_before(float a, int ia, float b, int ib) {
  return a > b || (a == b && ia >= 0 && (ib < 0 || ia < ib));
}
// the 64 lanes' pairs merged by a shuffle butterfly: every lane returns with the wave's two first slots in that order
__device__ __forceinline__ void top2_wave_merge(float& b1, int& i1, float& b2, int& i2) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob1 = __shfl_xor(b1, o), ob2 = __shfl_xor(b2, o);
    const int oi1 = __shfl_xor(i1, o), oi2 = __shfl_xor(i2, o);
    float n1, n2; int j1, j2;
    if (top2_before(b1, i1, ob1, oi1)) {
      n1 = b1; j1 = i1;
      if (top2_before(b2, i2, ob1, oi1)) { n2 = b2; j2 = i2; } else { n2 = ob1; j2 = oi1; }
    } else {
      n1 = ob1; j1 = oi1;
      if (top2_before(b1, i1, ob2, oi2)) { n2 = b1; j2 = i1; } else { n2 = ob2; j2 = oi2; }
    }
    b1 = n1; i1 = j1; b2 = n2; i2 = j2;
  }
}
// lane 0's store of a row's merged pair, [row][2]; either array may be NULL
__device__ __forceinline__ void top2_store(long long* top_idx, float* top_score, size_t row, float b1, int i1, float b2, int i2) {
  if (top_idx) { top_idx[row * 2] = i1; top_idx[row * 2 + 1] = i2; }
  if (top_score) { top_score[row * 2] = b1; top_score[row * 2 + 1] = b2; }
}

// ---- softmax + top-2 of one row by one wave -----------------------------------------------------------------------------
// What a lane holds of its row afterwards.  The first 256 classes of the row live in registers, four per lane -- as named
// scalars: next to a caller's small arrays (blend_ce_body's) one more array is what the compiler no longer keeps in registers.
struct SoftmaxRow {
  float z0, z1, z2, z3;        // the scores of classes lane, lane + 64, lane + 128, lane + 192
  float mx, inv;               // the row's maximum and 1 / sum of exp(z - mx): probability = __expf(z - mx) * inv
  float b1, b2; int i1, i2;    // the row's top-2 probabilities and classes, on every lane ((-1, -1): C = 1's second, a NaN row)
};
// f(n, z) on this lane's classes in ascending order: the register-held ones, then the tail re-formed through zat(n)
template <typename Z, typename F>
__device__ __forceinline__ void softmax_row_each(const SoftmaxRow& r, int classes, int lane, Z&& zat, F&& f) {
  if (lane < classes) f(lane, r.z0);
  if (lane + 64 < classes) f(lane + 64, r.z1);
  if (lane + 128 < classes) f(lane + 128, r.z2);
  if (lane + 192 < classes) f(lane + 192, r.z3);
  for (int n = lane + 256; n < classes; n += 64) f(n, zat(n));
}
// zat(n): score of class n of the row (global memory, LDS, a mean formed on the fly).  out(n, z, pr): the caller's stores of
// class n's score and probability.  mx is a max over the row; every lane adds __expf(z - mx) over its classes in ascending
// order, then wave_sum; pr = __expf(z - mx) * inv.
template <typename Z, typename Out>
__device__ __forceinline__ SoftmaxRow softmax_top2_row_body(int classes, int lane, Z&& zat, Out&& out) {
  SoftmaxRow r;
  r.z0 = lane < classes ? zat(lane) : -3.4e38f;
  r.z1 = lane + 64 < classes ? zat(lane + 64) : -3.4e38f;
  r.z2 = lane + 128 < classes ? zat(lane + 128) : -3.4e38f;
  r.z3 = lane + 192 < classes ? zat(lane + 192) : -3.4e38f;
  float mx = -3.4e38f;
  softmax_row_each(r, classes, lane, zat, [&](int, float z) __attribute__((always_inline)) { mx = fmaxf(mx, z); });
  mx = wave_max(mx);
  float se = 0.f;
  softmax_row_each(r, classes, lane, zat, [&](int, float z) __attribute__((always_inline)) { se += __expf(z - mx); });
  se = wave_sum(se);
  const float inv = 1.f / se;
  float b1 = -1.f, b2 = -1.f;
  int i1 = -1, i2 = -1;
  softmax_row_each(r, classes, lane, zat, [&](int n, float z) __attribute__((always_inline)) {
    const float pr = __expf(z - mx) * inv;
    out(n, z, pr);
    top2_take(pr, n, b1, i1, b2, i2);
  });
  top2_wave_merge(b1, i1, b2, i2);
  r.mx = mx; r.inv = inv; r.b1 = b1; r.b2 = b2; r.i1 = i1; r.i2 = i2;
  return r;
}

}  // namespace dta
