// Stand-alone host program around houv::term_masks (houv_amd/csrc/houv_math.h), the rule by which the pruned solve kernels
// decide which Chamfer terms an iteration must compute.  Test infrastructure only (tests/test_term_masks_host.py).
//   term_masks_main NMET < records > masks
// stdin: records of 33 floats = anchor (8 cd, metric * 2 + dir | R 9 | T 3) | R 9 | T 3 | radius; stdout: one byte per
// record, the function's result (bit m = dir 0 of metric m needed, bit 4 + m = dir 1).
#include "../../houv_amd/csrc/houv_math.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
  const int nmet = argc > 1 ? atoi(argv[1]) : 4;
  if (nmet != 1 && nmet != 4) {
    fprintf(stderr, "usage: %s 1|4 < records > masks\n", argv[0]);
    return 2;
  }
  constexpr int kRec = houv::kTermAnchorFloats + 9 + 3 + 1;
  float rec[kRec];
  while (fread(rec, sizeof(float), kRec, stdin) == (size_t)kRec) {
    const float* R = rec + houv::kTermAnchorFloats;
    const unsigned need = nmet == 4 ? houv::term_masks<4>(rec, R, R + 9, R[12]) : houv::term_masks<1>(rec, R, R + 9, R[12]);
    fputc((int)need, stdout);
  }
  return 0;
}
