// Device code shared by the kernels that turn the levels' top-1 classes into one species label (heads.hip:
// k_softmax_top2_ensemble, k_hierarchy_resolve; dense.hip: k_crown_resolve).  ONE definition of the walk, so that a crop,
// a window and a crown are resolved by the same sequence of table lookups.
#pragma once
#include "kernels.h"

namespace dta {

// ------------------------------------------------------------------------------------------------
// The hierarchy walk (reference multi_stage.py:404-434, `MultiStage.ensemble`, as a table: hierarchy.py).  Eight adjacent
// lanes serve one crop, lane k of them holding level k's top-1 class and probability: each looks its class up (one table
// load per level, all in flight together), then the walk itself is at most `levels` register shuffles.  Nothing the table
// or the class indices hold can take a load out of bounds: a class outside its level's range, or an edge that does not
// lead to a later level, ends the walk there (label -1 for the former).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void hierarchy_walk(const HierarchyArgs& e, int levels, int row, bool row_ok, int lane, int cls, float score) {
  const int lvl = lane & 7;
  int lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < BLEND_CE_MULTI_MAX; ++k)
    if (lvl == k) { lo = e.off[k]; hi = e.off[k + 1]; }
  int nx = -1, sp = -1;
  if (row_ok && lvl < levels && cls >= 0 && cls < hi - lo) { nx = e.next[lo + cls]; sp = e.species[lo + cls]; }
  int cur = 0;
#pragma unroll
  for (int s = 1; s < BLEND_CE_MULTI_MAX; ++s) {
    const int nxt = __shfl(nx, cur, 8);
    if (nxt > cur && nxt < levels) cur = nxt;
  }
  const int label = __shfl(sp, cur, 8);
  const float sc = __shfl(score, cur, 8);
  if (row_ok && lvl == 0) {
    e.ens_label[row] = label; e.ens_score[row] = sc; e.ens_level[row] = cur;
    if (e.labels) {
      // rows = label, columns = prediction; 64-bit integer adds commute, so the matrix does not depend on arrival order
      const long long y = e.labels[row];
      if (y >= 0 && y < e.n_species && label >= 0 && label < e.n_species)
        atomicAdd(reinterpret_cast<unsigned long long*>(e.confusion) + (size_t)y * e.n_species + label, 1ull);
    }
  }
}
}  // namespace dta
