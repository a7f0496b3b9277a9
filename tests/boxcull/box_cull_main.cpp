// Stand-alone host program around houv::box_test_group and houv::box_test_query (houv_amd/csrc/houv_math.h): the group cull of
// the pruned solve's box tests and the per-query test it stands in front of.  Test infrastructure only
// (tests/test_box_cull_host.py).
//   box_cull_main < cases > verdicts
// stdin, binary: int32 number of cases, then per case
//   int32 nmet (1 or 4), int32 mset, int32 count (queries 0 .. count-1 of the 64 lanes are points of the cloud)
//   float q[64][3], float ub[64][4] (bound per metric, -1 = not computed), float lo[3], float hi[3] (the reference box)
// stdout, binary, per case: uint64 mask of the lanes whose own test passes, int32 group verdict, float glo[3], ghi[3], gub[4],
// int32 0.
// The group is formed as the kernel forms it: the box by fminf / fmaxf over the lanes below `count` (NaN left out), the bound
// per metric by fmaxf over ALL lanes, a lane at or past `count` carrying -1.
#include "../../houv_amd/csrc/houv_math.h"
#include <cstdint>
#include <cstdio>

struct Case {
  int32_t nmet, mset, count;
  float q[64][3], ub[64][4], lo[3], hi[3];
};
struct Verdict {
  uint64_t lanes;
  int32_t group;
  float glo[3], ghi[3], gub[4];
  int32_t pad;
};
static_assert(sizeof(Verdict) == 56, "the record tests/boxcull/__init__.py reads");

template <int NMET>
static Verdict run(const Case& c) {
  Verdict v{};
  for (int a = 0; a < 3; ++a) { v.glo[a] = INFINITY; v.ghi[a] = -INFINITY; }
  for (int m = 0; m < 4; ++m) v.gub[m] = -1.0f;
  for (int l = 0; l < 64; ++l) {
    const bool ok = l < c.count;
    for (int a = 0; a < 3 && ok; ++a) { v.glo[a] = fminf(v.glo[a], c.q[l][a]); v.ghi[a] = fmaxf(v.ghi[a], c.q[l][a]); }
    float ub[4];
    for (int m = 0; m < 4; ++m) ub[m] = ok ? c.ub[l][m] : -1.0f;
    for (int m = 0; m < NMET; ++m) v.gub[m] = l == 0 ? ub[m] : fmaxf(v.gub[m], ub[m]);
    if (houv::box_test_query<NMET>(c.q[l], c.lo, c.hi, ub, (unsigned)c.mset)) v.lanes |= 1ull << l;
  }
  v.group = houv::box_test_group<NMET>(v.glo, v.ghi, c.lo, c.hi, v.gub, (unsigned)c.mset) ? 1 : 0;
  return v;
}

int main() {
  int32_t n = 0;
  if (fread(&n, sizeof n, 1, stdin) != 1) return 2;
  static Case c;
  for (int32_t i = 0; i < n; ++i) {
    if (fread(&c, sizeof c, 1, stdin) != 1) return 2;
    if ((c.nmet != 1 && c.nmet != 4) || c.count < 0 || c.count > 64) return 3;
    const Verdict v = c.nmet == 4 ? run<4>(c) : run<1>(c);
    if (fwrite(&v, sizeof v, 1, stdout) != 1) return 4;
  }
  return 0;
}
