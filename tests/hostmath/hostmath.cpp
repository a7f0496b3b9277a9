// Host build of houv_amd/csrc/houv_math.h for CPU unit tests (test infrastructure only:
// lets the exact code the HIP kernels inline be checked against the oracle without a GPU).
#include "../../houv_amd/csrc/houv_math.h"
#include <string.h>
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

extern "C" {

// Brute-force restatement of houv_knn's contract: for every point of xyz[B,N,3] the k smallest (distance, index) pairs in
// lexicographic order, with the distance of metric_sqdist<0> (houv_common.h): fmaf(dz, dz, fmaf(dy, dy, dx * dx)) in fp32,
// d = reference - query.  std::fmaf is the correctly rounded fused operation whatever the host; this file is compiled with
// -ffp-contract=off, so dx * dx stays a rounded product.  idx[B,N,k], dist[B,N,k] (dist may be null).
void hm_knn_fmaf(const float* xyz, int B, int N, int k, int* idx, float* dist) {
  std::vector<std::pair<float, int>> row((size_t)N);
  for (int b = 0; b < B; ++b) {
    const float* p = xyz + (size_t)b * N * 3;
    for (int q = 0; q < N; ++q) {
      const float qx = p[q * 3], qy = p[q * 3 + 1], qz = p[q * 3 + 2];
      for (int j = 0; j < N; ++j) {
        const float dx = p[j * 3] - qx, dy = p[j * 3 + 1] - qy, dz = p[j * 3 + 2] - qz;
        row[j] = std::make_pair(std::fmaf(dz, dz, std::fmaf(dy, dy, dx * dx)), j);
      }
      std::partial_sort(row.begin(), row.begin() + k, row.end());     // pair's operator<: distance, then index
      for (int j = 0; j < k; ++j) {
        idx[((size_t)b * N + q) * k + j] = row[j].second;
        if (dist) dist[((size_t)b * N + q) * k + j] = row[j].first;
      }
    }
  }
}

// The same for houv_knn_cross: for every point of query[B,N,3] the k smallest (distance, index) pairs of ref[B,M,3] in
// lexicographic order, same distance expression.  idx[B,N,k], dist[B,N,k] (dist may be null).  k <= M.
void hm_knn_cross_fmaf(const float* query, const float* ref, int B, int N, int M, int k, int* idx, float* dist) {
  std::vector<std::pair<float, int>> row((size_t)M);
  for (int b = 0; b < B; ++b) {
    const float* qp = query + (size_t)b * N * 3;
    const float* rp = ref + (size_t)b * M * 3;
    for (int q = 0; q < N; ++q) {
      const float qx = qp[q * 3], qy = qp[q * 3 + 1], qz = qp[q * 3 + 2];
      for (int j = 0; j < M; ++j) {
        const float dx = rp[j * 3] - qx, dy = rp[j * 3 + 1] - qy, dz = rp[j * 3 + 2] - qz;
        row[j] = std::make_pair(std::fmaf(dz, dz, std::fmaf(dy, dy, dx * dx)), j);
      }
      std::partial_sort(row.begin(), row.begin() + k, row.end());     // pair's operator<: distance, then index
      for (int j = 0; j < k; ++j) {
        idx[((size_t)b * N + q) * k + j] = row[j].second;
        if (dist) dist[((size_t)b * N + q) * k + j] = row[j].first;
      }
    }
  }
}

// params[n,8] -> R[n,9], T[n,3]
void hm_pose_forward(const float* params, int n, int angle_base, int trans_mode, float* R, float* T) {
  for (int i = 0; i < n; ++i) {
    houv::Pose f;
    houv::pose_forward(params + 8 * i, angle_base, trans_mode, f);
    memcpy(R + 9 * i, f.R, sizeof(f.R));
    memcpy(T + 3 * i, f.T, sizeof(f.T));
  }
}

// gT[n,3], M[n,9] -> g[n,8]
void hm_pose_backward(const float* params, int n, int angle_base, int trans_mode, const float* gT, const float* M, float* g) {
  for (int i = 0; i < n; ++i) {
    houv::Pose f;
    houv::pose_forward(params + 8 * i, angle_base, trans_mode, f);
    houv::pose_backward(f, trans_mode, gT + 3 * i, M + 9 * i, g + 8 * i);
  }
}

void hm_adam_f32(float* p, float* m, float* v, const float* g, int n, int step, double lr, double b1, double b2, double eps) {
  for (int i = 0; i < n; ++i) houv::adam_step<float>(p[i], m[i], v[i], g[i], step, lr, b1, b2, eps);
}

void hm_adam_f64(double* p, double* m, double* v, const double* g, int n, int step, double lr, double b1, double b2, double eps) {
  for (int i = 0; i < n; ++i) houv::adam_step<double>(p[i], m[i], v[i], g[i], step, lr, b1, b2, eps);
}

// The fused loop's scalar tail (solve_tail_loss<NMET> then solve_tail_step, nmet = 1 or 4) for n hypotheses, the way the kernels call it: the pose of
// state[0..7], Adam scalars of `step`.  acc[n,8,kAccStride], state[n,24] in/out -> score_loss[n,2], cd[n,8], g[n,8] and the
// stepped parameters' R[n,9], T[n,3].  Returns 0 for an nmet that is not built.
int hm_solve_tail(int nmet, int n, const float* acc, double* state, int k_full, int k_view, float loss_scale, int trans_mode,
                  int angle_base, int f64_params, int step, double lr, double b1, double b2, double eps, float* score_loss,
                  float* cd, float* g, float* R, float* T) {
  if (nmet != 1 && nmet != 4) return 0;
  for (int i = 0; i < n; ++i) {
    double* st = state + 24 * i;
    float p[8];
    for (int k = 0; k < 8; ++k) p[k] = (float)st[k];
    houv::Pose f;
    houv::pose_forward(p, angle_base, trans_mode, f);
    houv::TailLoss r;
    const float* a = acc + (size_t)i * 8 * houv::kAccStride;
    if (nmet == 1)
      houv::solve_tail_loss<1>(a, houv::kAccStride, f, k_full, k_view, loss_scale, trans_mode, r);
    else
      houv::solve_tail_loss<4>(a, houv::kAccStride, f, k_full, k_view, loss_scale, trans_mode, r);
    houv::solve_tail_step(r.g, st, f64_params, houv::adam_scalars(step, lr, b1, b2), b1, b2, eps, angle_base, trans_mode, f);
    score_loss[2 * i] = r.score;
    score_loss[2 * i + 1] = r.loss;
    memcpy(cd + 8 * i, r.cd, sizeof(r.cd));
    memcpy(g + 8 * i, r.g, sizeof(r.g));
    memcpy(R + 9 * i, f.R, sizeof(f.R));
    memcpy(T + 3 * i, f.T, sizeof(f.T));
  }
  return 1;
}

void hm_svd3x3_f32(const float* H, int n, float* U, float* S, float* V) {
  for (int i = 0; i < n; ++i) houv::svd3x3<float>(H + 9 * i, U + 9 * i, S + 3 * i, V + 9 * i);
}

void hm_kabsch_rotation_f32(const float* H, int n, float* R) {
  for (int i = 0; i < n; ++i) houv::kabsch_rotation<float>(H + 9 * i, R + 9 * i);
}
}
