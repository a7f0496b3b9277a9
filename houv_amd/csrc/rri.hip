// rri.hip -- the two device pieces of the DeepGMR head (registration/models/deepgmr.py) that the reference runs on the host:
//
//   houv_rri_features   get_rri_cluster (:54-95): rotation-invariant (|p|, |q_j|, theta_j, phi_j) per point and neighbour.  The
//                       reference copies the tangent vectors to the host, builds a [B*N,k,k,3] cross-product tensor in NumPy and
//                       argpartitions it; here 32 lanes serve one point, lane j owns neighbour j, the k tangent vectors of the
//                       point live in LDS and every lane walks them once.
//   houv_gmm_params     gmm_params (:98-120): responsibility-weighted moments, two passes, one workgroup per cloud, fixed tree.
//   houv_gmm_register   gmm_register (:123-143): the J-term weighted covariance and the closed-form pose, one lane per pair, on
//                       the register-resident Jacobi SVD of houv_math.h in float64 (the reference runs torch.svd on the CPU).
//
// Arithmetic is fp32 (houv_gmm_register: float64 registers on fp32 data) with fixed expression trees (-ffp-contract=off); nothing
// here allocates or uses atomics.
#include "houv_common.h"

namespace houv {
namespace {

// ------------------------------------------------------------------------------------------------------------------
// RRI features
// ------------------------------------------------------------------------------------------------------------------
constexpr int kRriBlock = 256;                    // 4 waves
constexpr int kRriLanes = 32;                     // lanes per point (k <= 31 of them own a neighbour)
constexpr int kRriPoints = kRriBlock / kRriLanes; // 8 points per workgroup, two per wave
constexpr float kTwoPiF = 6.28318530717958648f;   // float32(2 pi), what `psi % (2*np.pi)` adds to a negative fp32 angle

__global__ __launch_bounds__(kRriBlock) void rri_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ idx,
                                                        long long npts, int N, int k, int idx_ld, int idx_skip,
                                                        float* __restrict__ out, int vec_store) {
  // tangent vectors of the workgroup's 8 points, one 32-float row per coordinate: lane j writes column j, every lane of the
  // point then reads column i together (one address per 32-lane half = a broadcast, no bank conflict)
  __shared__ float tx[kRriPoints][kRriLanes], ty[kRriPoints][kRriLanes], tz[kRriPoints][kRriLanes];
  const int slot = threadIdx.x / kRriLanes;
  const int j = threadIdx.x % kRriLanes;
  const long long pt = (long long)blockIdx.x * kRriPoints + slot;     // b*N + n
  const bool live = pt < npts && j < k;

  float rp = 0.f, rq = 0.f, theta = 0.f;
  float pnx = 0.f, pny = 0.f, pnz = 0.f, Tx = 0.f, Ty = 0.f, Tz = 0.f;
  if (live) {
    const long long b = pt / N;
    const float* cloud = xyz + (size_t)b * N * 3;
    const float* p = xyz + (size_t)pt * 3;
    const float px = p[0], py = p[1], pz = p[2];
    int q = idx[(size_t)pt * idx_ld + idx_skip + j];
    q = q < 0 ? 0 : (q >= N ? N - 1 : q);          // an index outside the cloud is clamped into it: never an out-of-bounds read
    const float qx = cloud[(size_t)q * 3 + 0], qy = cloud[(size_t)q * 3 + 1], qz = cloud[(size_t)q * 3 + 2];
    rp = sqrtf((px * px + py * py) + pz * pz);
    rq = sqrtf((qx * qx + qy * qy) + qz * qz);
    pnx = px / rp; pny = py / rp; pnz = pz / rp;   // a zero-norm point: 0/0 = NaN, carried through as IEEE says
    const float qnx = qx / rq, qny = qy / rq, qnz = qz / rq;
    const float dot = (pnx * qnx + pny * qny) + pnz * qnz;
    const float cl = dot < -1.f ? -1.f : (dot > 1.f ? 1.f : dot);     // NaN stays NaN (torch.clamp)
    theta = acosf(cl);
    // deepgmr.py:80: the cosine multiplies the UNNORMALISED p -- not the tangent projection; kept
    Tx = qx - dot * px; Ty = qy - dot * py; Tz = qz - dot * pz;
  }
  tx[slot][j] = Tx; ty[slot][j] = Ty; tz[slot][j] = Tz;
  __syncthreads();

  // phi_j = second smallest of psi[j,i] = atan2((T_i x T_j).pn, T_i.T_j) mod 2 pi over i = 0..k-1, NaNs last
  float m1 = __builtin_inff(), m2 = __builtin_inff();
  int seen = 0;
  if (live) {
    for (int i = 0; i < k; ++i) {
      const float ax = tx[slot][i], ay = ty[slot][i], az = tz[slot][i];
      const float cx = ay * Tz - az * Ty, cy = az * Tx - ax * Tz, cz = ax * Ty - ay * Tx;
      const float s = (cx * pnx + cy * pny) + cz * pnz;
      const float c = (ax * Tx + ay * Ty) + az * Tz;
      float psi = atan2f(s, c);
      if (psi < 0.f) psi += kTwoPiF;
      if (psi == 0.f) psi = 0.f;                   // -0 -> +0
      if (psi == psi) {
        ++seen;
        if (psi < m1) { m2 = m1; m1 = psi; }
        else if (psi < m2) m2 = psi;
      }
    }
    const float phi = seen >= 2 ? m2 : __builtin_nanf("");
    float* o = out + (size_t)pt * 4 * k + 4 * j;   // lane j's four channels are adjacent: the point's row is one 16k-byte run
    if (vec_store) {
      *reinterpret_cast<float4*>(o) = make_float4(rp, rq, theta, phi);
    } else {
      o[0] = rp; o[1] = rq; o[2] = theta; o[3] = phi;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// GMM parameters: pi[J], mu[J,3], sigma[J] of one cloud per workgroup
// ------------------------------------------------------------------------------------------------------------------
constexpr int kGmmBlock = 1024;
constexpr int kGmmChunk = 8;          // a lane sums 8 terms at a time and then the chunk sums: short chains, fixed order

// Sum `v` over the lanes that share component j (lane = r*J + j, r < R): a fixed binary tree over r in LDS, the same for every
// call -> bit-identical results.  `red` holds kGmmBlock floats.  Every lane returns the total of its j.
__device__ __forceinline__ float gmm_tree_sum(float v, float* red, int r, int j, int J, int R, int R2) {
  const int t = threadIdx.x;
  __syncthreads();                    // the previous use of `red` is over
  red[t] = v;
  __syncthreads();
  for (int s = R2 >> 1; s > 0; s >>= 1) {
    if (r < s && r + s < R) red[t] += red[t + s * J];
    __syncthreads();
  }
  return red[j];
}

__global__ __launch_bounds__(kGmmBlock) void gmm_params_kernel(const float* __restrict__ gamma, const float* __restrict__ pts,
                                                               int N, int J, float* __restrict__ pi, float* __restrict__ mu,
                                                               float* __restrict__ sigma) {
  __shared__ float red[kGmmBlock];
  const int b = blockIdx.x;
  const int R = kGmmBlock / J;        // point rows in flight; lanes >= R*J idle (they still meet the barriers)
  int R2 = 1;
  while (R2 < R) R2 <<= 1;
  const int t = threadIdx.x;
  const bool active = t < R * J;
  const int r = active ? t / J : R2;  // idle lanes: a row no tree step touches
  const int j = active ? t % J : 0;
  const float* g = gamma + (size_t)b * N * J;
  const float* p = pts + (size_t)b * N * 3;

  // pass 1: S0 = sum gamma, S = sum gamma p
  float a0 = 0.f, ax = 0.f, ay = 0.f, az = 0.f;
  if (active) {
    for (int n0 = r; n0 < N; n0 += R * kGmmChunk) {
      float c0 = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
#pragma unroll
      for (int u = 0; u < kGmmChunk; ++u) {
        const int n = n0 + u * R;
        if (n < N) {
          const float w = g[(size_t)n * J + j];
          c0 += w; cx += w * p[3 * n + 0]; cy += w * p[3 * n + 1]; cz += w * p[3 * n + 2];
        }
      }
      a0 += c0; ax += cx; ay += cy; az += cz;
    }
  }
  const float s0 = gmm_tree_sum(a0, red, r, j, J, R, R2);
  const float sx = gmm_tree_sum(ax, red, r, j, J, R, R2);
  const float sy = gmm_tree_sum(ay, red, r, j, J, R, R2);
  const float sz = gmm_tree_sum(az, red, r, j, J, R, R2);
  const float pj = s0 / (float)N;
  const float npi = pj * (float)N;    // deepgmr.py:110: Npi = pi * N, not the raw sum
  const float mx = sx / npi, my = sy / npi, mz = sz / npi;

  // pass 2: sum gamma |p - mu|^2 about the mean just found (never E[x^2] - mu^2)
  float ad = 0.f;
  if (active) {
    for (int n0 = r; n0 < N; n0 += R * kGmmChunk) {
      float cd = 0.f;
#pragma unroll
      for (int u = 0; u < kGmmChunk; ++u) {
        const int n = n0 + u * R;
        if (n < N) {
          const float dx = p[3 * n + 0] - mx, dy = p[3 * n + 1] - my, dz = p[3 * n + 2] - mz;
          cd += g[(size_t)n * J + j] * ((dx * dx + dy * dy) + dz * dz);
        }
      }
      ad += cd;
    }
  }
  const float sd = gmm_tree_sum(ad, red, r, j, J, R, R2);
  if (active && r == 0) {
    pi[(size_t)b * J + j] = pj;
    mu[((size_t)b * J + j) * 3 + 0] = mx;
    mu[((size_t)b * J + j) * 3 + 1] = my;
    mu[((size_t)b * J + j) * 3 + 2] = mz;
    sigma[(size_t)b * J + j] = sd / npi;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// GMM registration: one lane per pair
// ------------------------------------------------------------------------------------------------------------------
constexpr int kRegBlock = 64;

__global__ __launch_bounds__(kRegBlock) void gmm_register_kernel(const float* __restrict__ pi_s, const float* __restrict__ mu_s,
                                                                 const float* __restrict__ mu_t,
                                                                 const float* __restrict__ sigma_t, int B, int J,
                                                                 float* __restrict__ T) {
  const int b = blockIdx.x * kRegBlock + threadIdx.x;
  if (b >= B) return;
  const float* w = pi_s + (size_t)b * J;
  const float* ms = mu_s + (size_t)b * J * 3;
  const float* mt = mu_t + (size_t)b * J * 3;
  const float* sg = sigma_t + (size_t)b * J;
  // One lane per pair and J <= a few dozen terms: the arithmetic is free, so the sums and the Jacobi SVD run in float64 registers
  // on the fp32 inputs and T is rounded once at the end.  (In fp32 the ~30 accumulated Jacobi rotations leave V orthogonal to
  // ~2e-6 only, four times the error of a LAPACK fp32 SVD of the same Ms.)
  double cs[3] = {0., 0., 0.}, ct[3] = {0., 0., 0.};          // both centres weighted by pi_s (deepgmr.py:130-131)
  for (int j = 0; j < J; ++j) {
    const double wj = (double)w[j];
#pragma unroll
    for (int i = 0; i < 3; ++i) { cs[i] += wj * (double)ms[3 * j + i]; ct[i] += wj * (double)mt[3 * j + i]; }
  }
  double M[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) M[i] = 0.;
  for (int j = 0; j < J; ++j) {
    const double wj = (double)w[j], inv = 1.0 / (double)sg[j];   // sigma_t = 0: inf/NaN from here on, as the reference's inverse()
    double a[3], c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { a[i] = wj * ((double)ms[3 * j + i] - cs[i]); c[i] = ((double)mt[3 * j + i] - ct[i]) * inv; }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int l = 0; l < 3; ++l) M[i * 3 + l] += a[i] * c[l];
  }
  double U[9], S[3], V[9], VUt[9], R[9];
  svd3x3<double>(M, U, S, V);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int l = 0; l < 3; ++l) VUt[i * 3 + l] = (V[i * 3 + 0] * U[l * 3 + 0] + V[i * 3 + 1] * U[l * 3 + 1]) + V[i * 3 + 2] * U[l * 3 + 2];
  const double d = det3<double>(VUt);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int l = 0; l < 3; ++l) R[i * 3 + l] = (V[i * 3 + 0] * U[l * 3 + 0] + V[i * 3 + 1] * U[l * 3 + 1]) + (V[i * 3 + 2] * d) * U[l * 3 + 2];
  float* o = T + (size_t)b * 16;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    o[i * 4 + 0] = (float)R[i * 3 + 0]; o[i * 4 + 1] = (float)R[i * 3 + 1]; o[i * 4 + 2] = (float)R[i * 3 + 2];
    o[i * 4 + 3] = (float)(ct[i] - ((R[i * 3 + 0] * cs[0] + R[i * 3 + 1] * cs[1]) + R[i * 3 + 2] * cs[2]));
  }
  o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
}

// ------------------------------------------------------------------------------------------------------------------
// Backward of gmm_params with the softmax's folded in: one point per group of J lanes, one pass, nothing of size [B,N,J,3]
// ------------------------------------------------------------------------------------------------------------------
constexpr int kGmmBwdBlock = 256;

__global__ __launch_bounds__(kGmmBwdBlock) void gmm_params_bwd_kernel(const float* __restrict__ gamma, const float* __restrict__ pts,
                                                                      const float* __restrict__ pi, const float* __restrict__ mu,
                                                                      const float* __restrict__ sigma, const float* __restrict__ g_pi,
                                                                      const float* __restrict__ g_mu, const float* __restrict__ g_sigma,
                                                                      long long npts, int N, int J, float* __restrict__ g_logits) {
  __shared__ float prod[kGmmBwdBlock];
  const int P = kGmmBwdBlock / J;      // points per workgroup; lanes >= P*J idle (they still meet the barrier)
  const int t = threadIdx.x;
  const int slot = t / J, j = t % J;
  const long long pt = (long long)blockIdx.x * P + slot;     // b*N + n
  const bool live = slot < P && pt < npts;
  float gam = 0.f, gg = 0.f;
  if (live) {
    const long long b = pt / N;
    const size_t bj = (size_t)b * J + j;
    const float* p = pts + (size_t)pt * 3;
    const float* m = mu + bj * 3;
    const float* gm = g_mu + bj * 3;
    const float dx = p[0] - m[0], dy = p[1] - m[1], dz = p[2] - m[2];
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const float s0 = pi[bj] * (float)N;
    const float dm = (gm[0] * dx + gm[1] * dy) + gm[2] * dz;
    gam = gamma[(size_t)pt * J + j];
    gg = g_pi[bj] / (float)N + (dm + g_sigma[bj] * (d2 - sigma[bj])) / s0;
  }
  prod[t] = gam * gg;
  __syncthreads();
  if (live) {
    float dot = 0.f;
    for (int i = 0; i < J; ++i) dot += prod[slot * J + i];   // the point's J lanes add the same values in the same order
    g_logits[(size_t)pt * J + j] = gam * (gg - dot);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Backward of gmm_register: one lane per pair, float64 registers, the forward recomputed.  The rotation's derivative takes the
// polar form: R = V D U^T is the orthogonal polar factor of Ms^T, so with lam = (s1, s2, D33 s3) and A~ = U^T skew(R^T G_R) U,
//   g_Ms = -2 U B~ U^T R^T,   B~_ij = A~_ij / (lam_i + lam_j)  (i != j),   skew(X) = (X - X^T) / 2.
// The generic SVD backward divides by s_i^2 - s_j^2, which blows up at equal singular values although the terms cancel; the sums
// lam_i + lam_j vanish only where the rotation itself is undetermined.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRegBlock) void gmm_register_bwd_kernel(const float* __restrict__ pi_s, const float* __restrict__ mu_s,
                                                                     const float* __restrict__ mu_t, const float* __restrict__ sigma_t,
                                                                     const float* __restrict__ g_T, int B, int J,
                                                                     float* __restrict__ g_pi_s, float* __restrict__ g_mu_s,
                                                                     float* __restrict__ g_mu_t, float* __restrict__ g_sigma_t) {
  const int b = blockIdx.x * kRegBlock + threadIdx.x;
  if (b >= B) return;
  const float* w = pi_s + (size_t)b * J;
  const float* ms = mu_s + (size_t)b * J * 3;
  const float* mt = mu_t + (size_t)b * J * 3;
  const float* sg = sigma_t + (size_t)b * J;
  const float* gT = g_T + (size_t)b * 16;
  // the forward, as gmm_register_kernel runs it
  double cs[3] = {0., 0., 0.}, ct[3] = {0., 0., 0.};
  for (int j = 0; j < J; ++j) {
    const double wj = (double)w[j];
#pragma unroll
    for (int i = 0; i < 3; ++i) { cs[i] += wj * (double)ms[3 * j + i]; ct[i] += wj * (double)mt[3 * j + i]; }
  }
  double M[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) M[i] = 0.;
  for (int j = 0; j < J; ++j) {
    const double wj = (double)w[j], inv = 1.0 / (double)sg[j];
    double a[3], c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { a[i] = wj * ((double)ms[3 * j + i] - cs[i]); c[i] = ((double)mt[3 * j + i] - ct[i]) * inv; }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int l = 0; l < 3; ++l) M[i * 3 + l] += a[i] * c[l];
  }
  double U[9], S[3], V[9], VUt[9], R[9];
  svd3x3<double>(M, U, S, V);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int l = 0; l < 3; ++l) VUt[i * 3 + l] = (V[i * 3 + 0] * U[l * 3 + 0] + V[i * 3 + 1] * U[l * 3 + 1]) + V[i * 3 + 2] * U[l * 3 + 2];
  const double d = det3<double>(VUt);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int l = 0; l < 3; ++l) R[i * 3 + l] = (V[i * 3 + 0] * U[l * 3 + 0] + V[i * 3 + 1] * U[l * 3 + 1]) + (V[i * 3 + 2] * d) * U[l * 3 + 2];
  const double lam[3] = {S[0], S[1], d * S[2]};

  // G_R = g_T[:3,:3] - g_t c_s^T;  X = R^T G_R;  A = skew(X);  A~ = U^T A U;  B~;  g_Ms = -2 U B~ U^T R^T
  double gt[3], GR[9], X[9], A[9], W[9], At[9], gM[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) gt[i] = (double)gT[i * 4 + 3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int l = 0; l < 3; ++l) GR[i * 3 + l] = (double)gT[i * 4 + l] - gt[i] * cs[l];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int l = 0; l < 3; ++l) X[i * 3 + l] = (R[0 * 3 + i] * GR[0 * 3 + l] + R[1 * 3 + i] * GR[1 * 3 + l]) + R[2 * 3 + i] * GR[2 * 3 + l];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int l = 0; l < 3; ++l) A[i * 3 + l] = 0.5 * (X[i * 3 + l] - X[l * 3 + i]);
#pragma unroll
  for (int i = 0; i < 3; ++i)          // W = A U
#pragma unroll
    for (int l = 0; l < 3; ++l) W[i * 3 + l] = (A[i * 3 + 0] * U[0 * 3 + l] + A[i * 3 + 1] * U[1 * 3 + l]) + A[i * 3 + 2] * U[2 * 3 + l];
#pragma unroll
  for (int i = 0; i < 3; ++i)          // A~ = U^T W, then B~ in place
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      const double v = (U[0 * 3 + i] * W[0 * 3 + l] + U[1 * 3 + i] * W[1 * 3 + l]) + U[2 * 3 + i] * W[2 * 3 + l];
      At[i * 3 + l] = i == l ? 0. : v / (lam[i] + lam[l]);
    }
#pragma unroll
  for (int i = 0; i < 3; ++i)          // W = U B~
#pragma unroll
    for (int l = 0; l < 3; ++l) W[i * 3 + l] = (U[i * 3 + 0] * At[0 * 3 + l] + U[i * 3 + 1] * At[1 * 3 + l]) + U[i * 3 + 2] * At[2 * 3 + l];
#pragma unroll
  for (int i = 0; i < 3; ++i)          // A = W U^T
#pragma unroll
    for (int l = 0; l < 3; ++l) A[i * 3 + l] = (W[i * 3 + 0] * U[l * 3 + 0] + W[i * 3 + 1] * U[l * 3 + 1]) + W[i * 3 + 2] * U[l * 3 + 2];
#pragma unroll
  for (int i = 0; i < 3; ++i)          // g_Ms = -2 A R^T
#pragma unroll
    for (int l = 0; l < 3; ++l) gM[i * 3 + l] = -2. * ((A[i * 3 + 0] * R[l * 3 + 0] + A[i * 3 + 1] * R[l * 3 + 1]) + A[i * 3 + 2] * R[l * 3 + 2]);

  // Ms = sum_j a_j c_j^T with a_j = w_j (ms_j - c_s), c_j = (mt_j - c_t) / sg_j:  g_a_j = g_Ms c_j,  g_c_j = g_Ms^T a_j.
  // First the two centres' totals: g_cs = -R^T g_t - sum_j w_j g_a_j,  g_ct = g_t - sum_j g_c_j / sg_j.
  double gcs[3], gct[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    gcs[i] = -((R[0 * 3 + i] * gt[0] + R[1 * 3 + i] * gt[1]) + R[2 * 3 + i] * gt[2]);
    gct[i] = gt[i];
  }
  for (int j = 0; j < J; ++j) {
    const double wj = (double)w[j], inv = 1.0 / (double)sg[j];
    double a[3], c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { a[i] = wj * ((double)ms[3 * j + i] - cs[i]); c[i] = ((double)mt[3 * j + i] - ct[i]) * inv; }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double ga = (gM[i * 3 + 0] * c[0] + gM[i * 3 + 1] * c[1]) + gM[i * 3 + 2] * c[2];
      const double gc = (gM[0 * 3 + i] * a[0] + gM[1 * 3 + i] * a[1]) + gM[2 * 3 + i] * a[2];
      gcs[i] -= wj * ga;
      gct[i] -= gc * inv;
    }
  }
  for (int j = 0; j < J; ++j) {
    const double wj = (double)w[j], inv = 1.0 / (double)sg[j];
    double a[3], c[3], e[3], ga[3], gc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      e[i] = (double)ms[3 * j + i] - cs[i];
      a[i] = wj * e[i];
      c[i] = ((double)mt[3 * j + i] - ct[i]) * inv;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      ga[i] = (gM[i * 3 + 0] * c[0] + gM[i * 3 + 1] * c[1]) + gM[i * 3 + 2] * c[2];
      gc[i] = (gM[0 * 3 + i] * a[0] + gM[1 * 3 + i] * a[1]) + gM[2 * 3 + i] * a[2];
    }
    double gw = 0., gs = 0.;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      gw += (ga[i] * e[i] + (double)ms[3 * j + i] * gcs[i]) + (double)mt[3 * j + i] * gct[i];
      gs += gc[i] * c[i];
      g_mu_s[((size_t)b * J + j) * 3 + i] = (float)(wj * (ga[i] + gcs[i]));
      g_mu_t[((size_t)b * J + j) * 3 + i] = (float)(gc[i] * inv + wj * gct[i]);
    }
    g_pi_s[(size_t)b * J + j] = (float)gw;
    g_sigma_t[(size_t)b * J + j] = (float)(-gs * inv);
  }
}

}  // namespace
}  // namespace houv

extern "C" int houv_rri_features(const float* xyz, const int32_t* idx, int B, int N, int k, int idx_ld, int idx_skip,
                                 float* out, void* stream) {
  using namespace houv;
  if (B < 0 || N <= 0 || (long long)B * N > 0x7fffffffLL) {
    set_error("houv_rri_features: bad shape B=%d N=%d", B, N);
    return 0;
  }
  if (k < 2 || k > 31) {
    set_error("houv_rri_features: k=%d outside 2..31", k);
    return 0;
  }
  if (idx_skip < 0 || idx_ld <= 0 || (long long)idx_skip + k > idx_ld) {
    set_error("houv_rri_features: idx_skip=%d + k=%d exceeds idx_ld=%d", idx_skip, k, idx_ld);
    return 0;
  }
  if (B == 0) return 1;
  if (!xyz || !idx || !out) {
    set_error("houv_rri_features: null pointer");
    return 0;
  }
  const long long npts = (long long)B * N;
  const int vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  rri_kernel<<<(unsigned)((npts + kRriPoints - 1) / kRriPoints), kRriBlock, 0, (hipStream_t)stream>>>(xyz, idx, npts, N, k, idx_ld,
                                                                                                    idx_skip, out, vec);
  return check_launch("houv_rri_features") ? 1 : 0;
}

extern "C" int houv_gmm_params(const float* gamma, const float* pts, int B, int N, int J, float* pi, float* mu, float* sigma,
                               void* stream) {
  using namespace houv;
  if (B < 0 || N <= 0 || J < 1 || J > 32) {
    set_error("houv_gmm_params: bad shape B=%d N=%d J=%d (J is 1..32)", B, N, J);
    return 0;
  }
  if (B == 0) return 1;
  if (!gamma || !pts || !pi || !mu || !sigma) {
    set_error("houv_gmm_params: null pointer");
    return 0;
  }
  gmm_params_kernel<<<B, kGmmBlock, 0, (hipStream_t)stream>>>(gamma, pts, N, J, pi, mu, sigma);
  return check_launch("houv_gmm_params") ? 1 : 0;
}

extern "C" int houv_gmm_register(const float* pi_s, const float* mu_s, const float* mu_t, const float* sigma_t, int B, int J,
                                 float* T, void* stream) {
  using namespace houv;
  if (B < 0 || J < 1) {
    set_error("houv_gmm_register: bad shape B=%d J=%d", B, J);
    return 0;
  }
  if (B == 0) return 1;
  if (!pi_s || !mu_s || !mu_t || !sigma_t || !T) {
    set_error("houv_gmm_register: null pointer");
    return 0;
  }
  gmm_register_kernel<<<(B + kRegBlock - 1) / kRegBlock, kRegBlock, 0, (hipStream_t)stream>>>(pi_s, mu_s, mu_t, sigma_t, B, J, T);
  return check_launch("houv_gmm_register") ? 1 : 0;
}

extern "C" int houv_gmm_params_backward(const float* gamma, const float* pts, const float* pi, const float* mu, const float* sigma,
                                        const float* g_pi, const float* g_mu, const float* g_sigma, int B, int N, int J,
                                        float* g_logits, void* stream) {
  using namespace houv;
  if (B < 0 || N <= 0 || J < 1 || J > 32 || (long long)B * N > 0x7fffffffLL) {
    set_error("houv_gmm_params_backward: bad shape B=%d N=%d J=%d (J is 1..32)", B, N, J);
    return 0;
  }
  if (B == 0) return 1;
  if (!gamma || !pts || !pi || !mu || !sigma || !g_pi || !g_mu || !g_sigma || !g_logits) {
    set_error("houv_gmm_params_backward: null pointer");
    return 0;
  }
  const long long npts = (long long)B * N;
  const int P = kGmmBwdBlock / J;
  gmm_params_bwd_kernel<<<(unsigned)((npts + P - 1) / P), kGmmBwdBlock, 0, (hipStream_t)stream>>>(gamma, pts, pi, mu, sigma, g_pi, g_mu,
                                                                                                g_sigma, npts, N, J, g_logits);
  return check_launch("houv_gmm_params_backward") ? 1 : 0;
}

extern "C" int houv_gmm_register_backward(const float* pi_s, const float* mu_s, const float* mu_t, const float* sigma_t,
                                          const float* g_T, int B, int J, float* g_pi_s, float* g_mu_s, float* g_mu_t,
                                          float* g_sigma_t, void* stream) {
  using namespace houv;
  if (B < 0 || J < 1) {
    set_error("houv_gmm_register_backward: bad shape B=%d J=%d", B, J);
    return 0;
  }
  if (B == 0) return 1;
  if (!pi_s || !mu_s || !mu_t || !sigma_t || !g_T || !g_pi_s || !g_mu_s || !g_mu_t || !g_sigma_t) {
    set_error("houv_gmm_register_backward: null pointer");
    return 0;
  }
  gmm_register_bwd_kernel<<<(B + kRegBlock - 1) / kRegBlock, kRegBlock, 0, (hipStream_t)stream>>>(pi_s, mu_s, mu_t, sigma_t, g_T, B, J,
                                                                                                g_pi_s, g_mu_s, g_mu_t, g_sigma_t);
  return check_launch("houv_gmm_register_backward") ? 1 : 0;
}
