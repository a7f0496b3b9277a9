// Host restatement of houv_knn_feat's contract (include/houv_hip.h) for the CPU and GPU tests.  Compiled with
// -ffp-contract=off; std::fmaf is the correctly rounded fused operation whatever the host.
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

extern "C" {

// For every row i of x[B,N,C] (row stride ldx floats) the k smallest (distance, index) pairs over all rows j of the same cloud,
// in lexicographic order, with d = 0; for c ascending: t = x[j,c] - x[i,c]; d = fmaf(t, t, d) in fp32.  idx[B,N,k],
// dist[B,N,k] (dist may be null).  k <= N.
void hm_knn_feat(const float* x, int B, int N, int C, int ldx, int k, int* idx, float* dist) {
  std::vector<std::pair<float, int>> row((size_t)N);
  for (int b = 0; b < B; ++b) {
    const float* p = x + (size_t)b * N * ldx;
    for (int i = 0; i < N; ++i) {
      const float* xi = p + (size_t)i * ldx;
      for (int j = 0; j < N; ++j) {
        const float* xj = p + (size_t)j * ldx;
        float d = 0.f;
        for (int c = 0; c < C; ++c) {
          const float t = xj[c] - xi[c];
          d = std::fmaf(t, t, d);
        }
        row[j] = std::make_pair(d, j);
      }
      std::partial_sort(row.begin(), row.begin() + k, row.end());     // pair's operator<: distance, then index
      for (int j = 0; j < k; ++j) {
        idx[((size_t)b * N + i) * k + j] = row[j].second;
        if (dist) dist[((size_t)b * N + i) * k + j] = row[j].first;
      }
    }
  }
}
}
