// Stand-alone host program around houv::walk_variant (houv_amd/csrc/houv_math.h), the table by which the pruned solve kernels
// pick the compiled metric set of a sweep's box tests and walk from its term mask.  Test infrastructure only
// (tests/test_walk_variants_host.py).
//   walk_variants_main > table
// stdout: one line per mask 0..15: "need variant instantiated cost" (instantiated: 1 when the mask itself is a compiled set;
// cost: walk_step_cost of the mask), then one line "table <walk_variant_table() in hex>".
#include "../../houv_amd/csrc/houv_math.h"
#include <cstdio>

int main() {
  for (unsigned need = 0; need < 16u; ++need)
    printf("%u %u %d %d\n", need, houv::walk_variant(need), houv::walk_instantiated(need) ? 1 : 0, houv::walk_step_cost(need));
  printf("table %llx\n", houv::walk_variant_table());
  return 0;
}
