// Stand-alone host check of the dta_split_search refusals under AddressSanitizer / UBSan: every call below is refused on the
// host before any launch (or, with iterations = 0, has nothing to launch), so no GPU is needed and none is touched.  Host
// code only; never load it into Python.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         deeptreeattention_amd/csrc/split.hip tools/split_refusals.cpp -o tools/split_refusals && tools/split_refusals
// (split.hip alone: this file supplies the one symbol it takes from capi.hip, dta_set_error)
#include <cstdio>
#include <cstdarg>
#include <cstring>
#include <cmath>
#include "../include/dta_hip.h"
static char g_err[512];
void dta_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
int main() {
  alignas(16) int rows[64], totals[64];
  int sp[4], tp[4], orders[16]; long long tr[4], best[4]; unsigned char mem[16], taxa[16];
  // exactly `species` entries each: a read past the last one is the sanitizer's to report
  const double fl[3] = {3.0, 3.0, 4.0}, fl_nan[3] = {3.0, NAN, 4.0}, fl_inf[3] = {INFINITY, 3.0, 4.0}, fl_last[3] = {3.0, 3.0, -INFINITY};
  double fl_max[DTA_SPLIT_MAX_SPECIES + 1];
  for (double& v : fl_max) v = 3.0;
  int bad = 0, k = 0;
#define REFUSED(call, what) do { g_err[0] = 0; int rc = (call); ++k; if (rc == 0 || !strstr(g_err, what)) { printf("NOT refused: %s -> %d '%s'\n", #call, rc, g_err); ++bad; } } while (0)
#define SEARCH(rows_, totals_, c_, s_, fl_, mtr_, mte_, it_, sp_, tr_, tp_, best_) \
  dta_split_search(rows_, totals_, c_, s_, fl_, mtr_, mte_, it_, 7ull, ~0ull, orders, sp_, tr_, tp_, best_, mem, taxa, nullptr)
  REFUSED(SEARCH(nullptr, totals, 8, 3, fl, 5, 3, 2, sp, tr, tp, best), "null");
  REFUSED(SEARCH(rows, nullptr, 8, 3, fl, 5, 3, 2, sp, tr, tp, best), "null");
  REFUSED(SEARCH(rows, totals, 8, 3, nullptr, 5, 3, 2, sp, tr, tp, best), "null");
  REFUSED(SEARCH(rows, totals, 8, 3, fl, 5, 3, 2, nullptr, tr, tp, best), "null");
  REFUSED(SEARCH(rows, totals, 8, 3, fl, 5, 3, 2, sp, nullptr, tp, best), "null");
  REFUSED(SEARCH(rows, totals, 8, 3, fl, 5, 3, 2, sp, tr, nullptr, best), "null");
  REFUSED(SEARCH(rows, totals, 8, 3, fl, 5, 3, 2, sp, tr, tp, nullptr), "null");
  REFUSED(SEARCH(rows, totals, 8, 0, fl, 5, 3, 2, sp, tr, tp, best), "species=0");
  REFUSED(SEARCH(rows, totals, 8, -4, fl, 5, 3, 2, sp, tr, tp, best), "species=-4");
  REFUSED(SEARCH(rows, totals, 8, DTA_SPLIT_MAX_SPECIES + 1, fl_max, 5, 3, 2, sp, tr, tp, best), "species=257");
  REFUSED(SEARCH(rows, totals, 0, 3, fl, 5, 3, 2, sp, tr, tp, best), "candidates=0");
  REFUSED(SEARCH(rows, totals, -1, 3, fl, 5, 3, 2, sp, tr, tp, best), "candidates=-1");
  REFUSED(SEARCH(rows, totals, DTA_SPLIT_MAX_CANDIDATES + 1, 3, fl, 5, 3, 2, sp, tr, tp, best), "candidates=4097");
  REFUSED(SEARCH(rows, totals, 8, 3, fl, 5, 3, -1, sp, tr, tp, best), "iterations=-1");
  REFUSED(SEARCH(rows, totals, 8, 3, fl, 0, 3, 2, sp, tr, tp, best), "min_train=0");
  REFUSED(SEARCH(rows, totals, 8, 3, fl, 5, 0, 2, sp, tr, tp, best), "min_test=0");
  REFUSED(SEARCH(rows, totals, 8, 3, fl, 5, -2, 2, sp, tr, tp, best), "min_test=-2");
  REFUSED(SEARCH(rows + 1, totals, 8, 3, fl, 5, 3, 2, sp, tr, tp, best), "16-byte aligned");
  REFUSED(SEARCH(rows, totals + 2, 8, 3, fl, 5, 3, 2, sp, tr, tp, best), "16-byte aligned");
  REFUSED(SEARCH(rows, totals, 8, 3, fl_nan, 5, 3, 2, sp, tr, tp, best), "floor is not finite (species 1)");
  REFUSED(SEARCH(rows, totals, 8, 3, fl_inf, 5, 3, 2, sp, tr, tp, best), "floor is not finite (species 0)");
  REFUSED(SEARCH(rows, totals, 8, 3, fl_last, 5, 3, 2, sp, tr, tp, best), "floor is not finite (species 2)");
  REFUSED(SEARCH(rows, totals, 8, 3, fl_nan, 5, 3, 0, sp, tr, tp, best), "floor is not finite");     // before the early return
  ++k;
  if (SEARCH(rows, totals, 8, DTA_SPLIT_MAX_SPECIES, fl_max, 5, 3, 0, sp, tr, tp, best) != 0) {   // 0 iterations: nothing to do
    printf("iterations=0 was refused: '%s'\n", g_err);
    ++bad;
  }
  printf("%d calls, %d wrong\n", k, bad);
  return bad != 0;
}
