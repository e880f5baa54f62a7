// Stand-alone host check of dta_crown_height's refusals under AddressSanitizer / UBSan: every call below is refused on the
// host before any launch, so no GPU is needed and none is touched.  Host code only; never load it into Python.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         deeptreeattention_amd/csrc/canopy.hip tools/canopy_refusals.cpp -o tools/canopy_refusals && tools/canopy_refusals
// (canopy.hip alone: this file supplies the one symbol it takes from capi.hip, dta_set_error)
#include <cstdio>
#include <cstdarg>
#include <cstring>
#include <cmath>
#include "../include/dta_hip.h"
static char g_err[512];
void dta_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
int main() {
  float buf[16]; int ib[16]; unsigned char kb[16]; double fd[4];
  dta_height_rule r1 = {1, 3.0, 0, 0, 0}, r2 = {2, 0, 1, 4, 8}, r3 = {3, 0, 0, 0, 0}, r0 = {0, 0, 0, 0, 0};
  int bad = 0, k = 0;
#define REFUSED(call, what) do { g_err[0] = 0; int rc = (call); ++k; if (rc == 0 || !strstr(g_err, what)) { printf("NOT refused: %s -> %d '%s'\n", #call, rc, g_err); ++bad; } } while (0)
  REFUSED(dta_crown_height(nullptr, 4, 4, ib, 1, 99.f, .5f, nullptr, nullptr, buf, ib, nullptr, nullptr), "null");
  REFUSED(dta_crown_height(buf, 4, 4, nullptr, 1, 99.f, .5f, nullptr, nullptr, buf, ib, nullptr, nullptr), "null");
  REFUSED(dta_crown_height(buf, 4, 4, ib, 1, 99.f, .5f, nullptr, nullptr, nullptr, ib, nullptr, nullptr), "null");
  REFUSED(dta_crown_height(buf, 4, 4, ib, 1, 99.f, .5f, nullptr, nullptr, buf, nullptr, nullptr, nullptr), "null");
  REFUSED(dta_crown_height(buf, 4, 4, ib, 0, 99.f, .5f, nullptr, nullptr, buf, ib, nullptr, nullptr), "n=");
  REFUSED(dta_crown_height(buf, 0, 4, ib, 1, 99.f, .5f, nullptr, nullptr, buf, ib, nullptr, nullptr), "height=");
  REFUSED(dta_crown_height(buf, 4, -1, ib, 1, 99.f, .5f, nullptr, nullptr, buf, ib, nullptr, nullptr), "width=");
  REFUSED(dta_crown_height(buf, 2147483647, 2147483647, ib, 1, 99.f, .5f, nullptr, nullptr, buf, ib, nullptr, nullptr), "int32");
  REFUSED(dta_crown_height(buf, 4, 4, ib, 1, 101.f, .5f, nullptr, nullptr, buf, ib, nullptr, nullptr), "q=");
  REFUSED(dta_crown_height(buf, 4, 4, ib, 1, NAN, .5f, nullptr, nullptr, buf, ib, nullptr, nullptr), "q=");
  REFUSED(dta_crown_height(buf, 4, 4, ib, 1, 99.f, 0.f, nullptr, nullptr, buf, ib, nullptr, nullptr), "floor=");
  REFUSED(dta_crown_height(buf, 4, 4, ib, 1, 99.f, .5f, nullptr, &r2, buf, ib, kb, nullptr), "field_height");
  REFUSED(dta_crown_height(buf, 4, 4, ib, 1, 99.f, .5f, nullptr, &r3, buf, ib, kb, nullptr), "mode");
  REFUSED(dta_crown_height(buf, 4, 4, ib, 1, 99.f, .5f, nullptr, nullptr, buf, ib, kb, nullptr), "without a rule");
  REFUSED(dta_crown_height(buf, 4, 4, ib, 1, 99.f, .5f, nullptr, &r0, buf, ib, kb, nullptr), "without a rule");
  REFUSED(dta_crown_height(buf, 4, 4, ib, 1, 99.f, .5f, nullptr, &r1, buf, ib, nullptr, nullptr), "without a keep");
  REFUSED(dta_crown_height(buf, 4, 4, ib, 1, 99.f, .5f, fd, &r2, buf, ib, nullptr, nullptr), "without a keep");
  printf("%d calls, %d not refused\n", k, bad);
  return bad != 0;
}
