// Host compile of houv_amd/csrc/houv_math.h's stage-scheduling arithmetic: for every "ninst n_iters chunk_iters" line on stdin,
// prints one line per ticket: "ticket chunk hypothesis steps_offset item_iters".
#include <stdio.h>

#include "../../houv_amd/csrc/houv_math.h"

int main() {
  int ninst, n_iters, chunk_iters;
  while (scanf("%d %d %d", &ninst, &n_iters, &chunk_iters) == 3) {
    const int items = houv::sched_items(ninst, n_iters, chunk_iters);
    printf("items %d %lld chunks %d\n", items, houv::sched_items64(ninst, n_iters, chunk_iters),
           houv::sched_chunks(n_iters, chunk_iters));
    for (int t = 0; t < items; ++t) {
      const int chunk = t / ninst, h = t - chunk * ninst;
      printf("%d %d %d %d %d\n", t, chunk, h, chunk * chunk_iters, houv::sched_item_iters(n_iters, chunk_iters, chunk));
    }
  }
  return 0;
}
