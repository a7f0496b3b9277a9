// Stand-alone host program around houv::term_anchor_masks (houv_amd/csrc/houv_math.h), the per-term-record rule by which the
// pruned solve kernels decide which Chamfer terms an iteration must compute, with houv::term_masks (the shared-anchor rule)
// beside it for comparison.  Test infrastructure only (tests/test_term_anchors_host.py).
//   term_anchors_main NMET < records > masks
// stdin: records of 82 floats = cd (8, metric * 2 + dir) | fresh pose (R 9 | T 3) | stale poses (4 x (R 9 | T 3)) |
// stale bits (as a float, 0..255) | R 9 | T 3 | radius; stdout: two bytes per record: term_anchor_masks' result, then
// term_masks' result with (cd, fresh pose) as its anchor (bit m = dir 0 of metric m needed, bit 4 + m = dir 1).
#include "../../houv_amd/csrc/houv_math.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
  const int nmet = argc > 1 ? atoi(argv[1]) : 4;
  if (nmet != 1 && nmet != 4) {
    fprintf(stderr, "usage: %s 1|4 < records > masks\n", argv[0]);
    return 2;
  }
  constexpr int kRec = 8 + 12 + 48 + 1 + 12 + 1;
  static_assert(houv::kTermAnchorFloats == 20, "cd | fresh pose is term_masks' anchor");
  float rec[kRec];
  while (fread(rec, sizeof(float), kRec, stdin) == (size_t)kRec) {
    const float *fresh = rec + 8, *stale = rec + 20, *R = rec + 69, *T = rec + 78;
    const unsigned bits = (unsigned)rec[68] & 0xffu;
    const float radius = rec[81];
    const unsigned need = nmet == 4 ? houv::term_anchor_masks<4>(rec, fresh, stale, 1, bits, R, T, radius)
                                    : houv::term_anchor_masks<1>(rec, fresh, stale, 1, bits, R, T, radius);
    const unsigned old = nmet == 4 ? houv::term_masks<4>(rec, R, T, radius) : houv::term_masks<1>(rec, R, T, radius);
    fputc((int)need, stdout);
    fputc((int)old, stdout);
  }
  return 0;
}
