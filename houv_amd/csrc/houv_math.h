// houv_math.h -- small per-instance math shared by the HIP kernels.
//
// Everything here is `HOUV_HD inline`, written against plain C++ so the very
// same code can be compiled for the host by tests/hostmath (g++) and unit
// tested against the oracle without a GPU.  Citations are to the reference
// tree (Dizzy-cell/HOUV):
//   registration/models/houv.py:69-103      Rodrigues + translation reparam
//   registration/train_utils.py:397-407      the `solve` twin (sigma = sin(s pi))
//   registration/model_utils.py:220-255      SVDHead (Kabsch)
//   torch.optim.Adam (reference: houv.py:118, train_utils.py:389)
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define HOUV_HD __host__ __device__
#else
#define HOUV_HD
#endif

namespace houv {

// houv.py:19 -- pi = acos(0)*2 evaluated in fp32 (= 3.1415927410125732), then used as a Python float
// that multiplies fp32 tensors, i.e. rounded back to fp32 at each use.
constexpr float kPiF = 3.14159274101257324f;

enum TransMode { kTransHouv = 0, kTransSolve = 1 };

HOUV_HD inline float tsqrt(float x) { return sqrtf(x); }     // correctly rounded (no -ffast-math)
HOUV_HD inline double tsqrt(double x) { return sqrt(x); }

// Parameter block layout (8 scalars per hypothesis): V[0..2], a, c[0..2], s
struct Pose {
  float R[9];   // row-major
  float T[3];
  // forward intermediates kept for the backward pass
  float u[3], inv_vnorm, sin_t, cos_t, chat[3], inv_cnorm, sigma, a, s;
};

// houv.py:94-103 (HOUV.forward) / train_utils.py:403-407.
HOUV_HD inline void pose_forward(const float p[8], int angle_base, int trans_mode, Pose& o) {
  const float vx = p[0], vy = p[1], vz = p[2];
  const float vn = sqrtf(vx * vx + vy * vy + vz * vz);           // houv.py:71
  o.inv_vnorm = 1.0f / vn;
  o.u[0] = vx / vn; o.u[1] = vy / vn; o.u[2] = vz / vn;
  o.a = p[3];
  // theta = sin(a*pi)*pi/8 + pi/8 + base*pi/4   (houv.py:96), all fp32 roundings as torch does them
  const float theta = sinf(p[3] * kPiF) * kPiF / 8.0f + kPiF / 8.0f + (float)angle_base * kPiF / 4.0f;
  const float st = sinf(theta), ct = cosf(theta);
  o.sin_t = st; o.cos_t = ct;
  const float ux = o.u[0], uy = o.u[1], uz = o.u[2];
  // A = [u]x (houv.py:78-83);  A*A = u u^T - I (|u|=1) but the reference multiplies it out: keep the product form
  const float A[9] = {0.f, -uz, uy, uz, 0.f, -ux, -uy, ux, 0.f};
  float AA[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      AA[i * 3 + j] = A[i * 3 + 0] * A[0 * 3 + j] + A[i * 3 + 1] * A[1 * 3 + j] + A[i * 3 + 2] * A[2 * 3 + j];
  const float omc = 1.0f - ct;
  for (int i = 0; i < 9; ++i) o.R[i] = ((i % 4 == 0) ? 1.0f : 0.0f) + st * A[i] + omc * AA[i];   // houv.py:85
  o.s = p[7];
  const float sp = sinf(p[7] * kPiF);
  o.sigma = (trans_mode == kTransHouv) ? (sp * 0.125f + 0.125f) : (sp * 1.0f);      // houv.py:99 / train_utils.py:404
  const float cx = p[4], cy = p[5], cz = p[6];
  const float cn = sqrtf(cx * cx + cy * cy + cz * cz);           // houv.py:89
  o.inv_cnorm = 1.0f / cn;
  o.chat[0] = cx / cn; o.chat[1] = cy / cn; o.chat[2] = cz / cn;
  o.T[0] = o.chat[0] * o.sigma; o.T[1] = o.chat[1] * o.sigma; o.T[2] = o.chat[2] * o.sigma;
}

// Closed-form backward of pose_forward (what autograd does through houv.py:69-103).
//   gT[3]  = dL/dT = sum_i G_i
//   M[9]   = dL/dR = sum_i G_i p_i^T   (row-major, p = un-moved source point)
// -> g[8] = dL/d(V, a, c, s)
HOUV_HD inline void pose_backward(const Pose& f, int trans_mode, const float gT[3], const float M[9], float g[8]) {
  const float ux = f.u[0], uy = f.u[1], uz = f.u[2];
  const float A[9] = {0.f, -uz, uy, uz, 0.f, -ux, -uy, ux, 0.f};
  float AA[9], MAt[9], AtM[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      AA[i * 3 + j] = A[i * 3 + 0] * A[0 * 3 + j] + A[i * 3 + 1] * A[1 * 3 + j] + A[i * 3 + 2] * A[2 * 3 + j];
      // (M A^T)_ij = sum_k M_ik A_jk ;  (A^T M)_ij = sum_k A_ki M_kj
      MAt[i * 3 + j] = M[i * 3 + 0] * A[j * 3 + 0] + M[i * 3 + 1] * A[j * 3 + 1] + M[i * 3 + 2] * A[j * 3 + 2];
      AtM[i * 3 + j] = A[0 * 3 + i] * M[0 * 3 + j] + A[1 * 3 + i] * M[1 * 3 + j] + A[2 * 3 + i] * M[2 * 3 + j];
    }
  // dL/dtheta = <M, cos A + sin A^2>
  float dth = 0.f;
  for (int i = 0; i < 9; ++i) dth += M[i] * (f.cos_t * A[i] + f.sin_t * AA[i]);
  // theta = sin(a pi) pi/8 + ...  ->  dtheta/da = cos(a pi) * pi * pi/8
  g[3] = dth * cosf(f.a * kPiF) * kPiF * kPiF / 8.0f;
  // dL/dA = sin M + (1-cos)(M A^T + A^T M)
  float Qm[9];
  const float omc = 1.0f - f.cos_t;
  for (int i = 0; i < 9; ++i) Qm[i] = f.sin_t * M[i] + omc * (MAt[i] + AtM[i]);
  // A01=-u2 A02=u1 A10=u2 A12=-u0 A20=-u1 A21=u0
  const float du0 = Qm[7] - Qm[5], du1 = Qm[2] - Qm[6], du2 = Qm[3] - Qm[1];
  // u = v/|v| -> dv = (I - u u^T)/|v| du
  const float dot_u = ux * du0 + uy * du1 + uz * du2;
  g[0] = (du0 - ux * dot_u) * f.inv_vnorm;
  g[1] = (du1 - uy * dot_u) * f.inv_vnorm;
  g[2] = (du2 - uz * dot_u) * f.inv_vnorm;
  // T = sigma * chat
  const float dot_c = f.chat[0] * gT[0] + f.chat[1] * gT[1] + f.chat[2] * gT[2];
  g[4] = f.sigma * (gT[0] - f.chat[0] * dot_c) * f.inv_cnorm;
  g[5] = f.sigma * (gT[1] - f.chat[1] * dot_c) * f.inv_cnorm;
  g[6] = f.sigma * (gT[2] - f.chat[2] * dot_c) * f.inv_cnorm;
  const float dsig = (trans_mode == kTransHouv) ? (cosf(f.s * kPiF) * kPiF * 0.125f) : (cosf(f.s * kPiF) * kPiF);
  g[7] = dot_c * dsig;
}

// One torch.optim.Adam step (no weight decay / amsgrad) on one scalar, arithmetic type T = float
// (HOUV module, fp32 parameters: houv.py:54-61,118) or double (`solve` twin keeps float64 leaves:
// train_utils.py:381-389).  `step` is 1-based.  Mirrors torch's single-tensor formulation:
//   m += (g-m)(1-b1);  v = v b2 + (1-b2) g g;  p -= (lr/(1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// The step-dependent scalars (torch computes them in Python doubles): shared by all parameters of a step.
struct AdamScalars {
  double step_size, bc2_sqrt;
};
HOUV_HD inline AdamScalars adam_scalars(int step, double lr, double b1, double b2) {
  const double bc1 = 1.0 - pow(b1, (double)step);
  const double bc2 = 1.0 - pow(b2, (double)step);
  return AdamScalars{lr / bc1, sqrt(bc2)};
}
template <typename T>
HOUV_HD inline void adam_step(T& p, T& m, T& v, T g, const AdamScalars& sc, double b1, double b2, double eps) {
  m = m + (g - m) * (T)(1.0 - b1);
  v = v * (T)b2 + ((T)(1.0 - b2) * g) * g;
  const T denom = tsqrt(v) / (T)sc.bc2_sqrt + (T)eps;
  p = p - (T)sc.step_size * (m / denom);
}
template <typename T>
HOUV_HD inline void adam_step(T& p, T& m, T& v, T g, int step, double lr, double b1, double b2, double eps) {
  adam_step<T>(p, m, v, g, adam_scalars(step, lr, b1, b2), b1, b2, eps);
}

// ---------------------------------------------------------------------------------------------
// The per-hypothesis scalar tail of the fused loop (solve.hip, solve_large.hip): what one thread does once both Chamfer
// directions are summed.  Two halves, so that a kernel can store the last iteration's outputs between them:
//   solve_tail_loss   loss and closed-form gradient from the 8 x 13 sums
//   solve_tail_step   Adam step on the 24-double state, pose of the stepped parameters
// Plain `inline` like the rest of this header, on purpose: with __forceinline__ 17 of the solve_kernel instantiations spilled
// more registers than with the same text written out in the kernel; the compiler inlines both anyway (no calls remain).
// ---------------------------------------------------------------------------------------------
constexpr int kAccN = 13;
constexpr int kAccStride = 16;   // row stride (floats) of acc and of the reduction scratch in front of it

struct TailLoss {
  float score, loss;   // the full metric's Chamfer term; 6 * score + the view terms (houv.py:222 / train_utils.py:433)
  float cd[4][2];      // [metric][dir] mean sqrt distance; 0 for metrics >= NMET
  float g[8];          // dloss/d(V, a, c, s) * loss_scale
};

//   acc   [8][acc_stride] floats, slot = metric*2 + dir (dir 0 over the target points, 1 over the moved points), entries
//         S = sum sqrt(d), G[3] = sum c, GP[9] = sum c p^T (kAccN of them); only slots of metrics < NMET are read
//   f     pose_forward of the current parameters
template <int NMET>
HOUV_HD inline void solve_tail_loss(const float* acc, int acc_stride, const Pose& f, int k_full, int k_view, float loss_scale,
                                    int trans_mode, TailLoss& r) {
  float val[NMET];
  int pick[NMET];
  float gT[3] = {0.f, 0.f, 0.f}, Mm[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  bool bad = false;
#pragma unroll
  for (int m = 0; m < 4; ++m) r.cd[m][0] = r.cd[m][1] = 0.f;
#pragma unroll
  for (int m = 0; m < NMET; ++m) {
    const float kk = (float)((m == 0) ? k_full : k_view);
    r.cd[m][0] = acc[(m * 2 + 0) * acc_stride] / kk;   // over target points   (calc_cd_percent's 1st output)
    r.cd[m][1] = acc[(m * 2 + 1) * acc_stride] / kk;   // over moved points    (2nd output)
    // torch.min(cat([first, second])): first wins ties; NaN propagates
    pick[m] = (r.cd[m][0] <= r.cd[m][1]) ? 0 : 1;
    val[m] = r.cd[m][pick[m]];
    if (r.cd[m][0] != r.cd[m][0] || r.cd[m][1] != r.cd[m][1]) { val[m] = NAN; bad = true; }
    const float w = ((m == 0) ? 6.0f : 1.0f) * loss_scale / kk;
    const float* ac = acc + (m * 2 + pick[m]) * acc_stride;
#pragma unroll
    for (int i = 0; i < 3; ++i) gT[i] += w * ac[1 + i];
#pragma unroll
    for (int i = 0; i < 9; ++i) Mm[i] += w * ac[4 + i];
  }
  r.score = val[0];
  r.loss = val[0] * 6.0f;                                  // houv.py:222 / train_utils.py:433
  if constexpr (NMET == 4) r.loss = r.loss + (val[1] + val[2] + val[3]);
  if (bad) {
#pragma unroll
    for (int i = 0; i < 3; ++i) gT[i] = NAN;
#pragma unroll
    for (int i = 0; i < 9; ++i) Mm[i] = NAN;
  }
  pose_backward(f, trans_mode, gT, Mm, r.g);
}

//   state   [24] doubles p | m | v, stepped in place: in fp32 (the doubles then hold float-rounded values) unless f64_params
//   asc     adam_scalars of this step
//   next    pose_forward of the stepped parameters (may be the Pose the gradient came from)
HOUV_HD inline void solve_tail_step(const float g[8], double* state, int f64_params, AdamScalars asc, double beta1, double beta2,
                                    double eps, int angle_base, int trans_mode, Pose& next) {
  if (f64_params) {
    for (int k = 0; k < 8; ++k)
      adam_step<double>(state[k], state[8 + k], state[16 + k], (double)g[k], asc, beta1, beta2, eps);
  } else {
    for (int k = 0; k < 8; ++k) {
      float pp = (float)state[k], mm = (float)state[8 + k], vv = (float)state[16 + k];
      adam_step<float>(pp, mm, vv, g[k], asc, beta1, beta2, eps);
      state[k] = pp; state[8 + k] = mm; state[16 + k] = vv;
    }
  }
  float p[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) p[k] = (float)state[k];
  pose_forward(p, angle_base, trans_mode, next);
}

// ---------------------------------------------------------------------------------------------
// Term masks of the pruned solve (solve.hip, PRUNE != 0): which of the eight Chamfer terms cd[metric][dir] an iteration has
// to compute.  solve_tail_loss takes min(cd[m][0], cd[m][1]) per metric; the loser's value only decides that it lost.  If an
// earlier iteration (the ANCHOR) computed all eight terms and the moved cloud has not travelled far since, the loser is known
// without computing it.
//
// Proof sketch.  Let every moved point R p + T lie within d of its anchor position.  A nearest-neighbour distance -- full or
// in an axis-dropped projection (a projection is 1-Lipschitz), moved -> target or target -> moved -- changes by at most d; so
// does each of the k smallest of them in sorted order, hence their mean: every term is 1-Lipschitz in the displacement.  With
//   d <= ||R - R_anchor||_F * radius + |T - T_anchor|      (radius = max |p| over the source cloud; Frobenius >= spectral norm)
// a term Y with  cd_X + 2 d < cd_Y  at the anchor still satisfies cd_X < cd_Y now: Y loses and need not be computed.
//
// Margin (what fp32 adds to the real-number argument; u = 2^-24 = 6.0e-8):
//   * move_point: 4 roundings per coordinate of magnitudes <= radius + |T_i|, so a computed moved point is within
//     sqrt(3) * 4 u * (radius + |T|) = 4.2e-7 * (radius + |T|) of R p + T; at the anchor and now together
//     4.2e-7 * (2 radius + |T| + |T_anchor|) on d, which enters the inequality doubled: kTermMoveErr = 1e-6 times that sum;
//   * a computed term against the real one on the same computed points: squared distance 3 subtractions, products and two or
//     three FMAs (<= 6 u relative), sqrt (half of that + u = 4 u), a sum of up to 4096 non-negative terms in any grouping
//     (<= 4095 u), the division by k (u): <= 4100 u = 2.5e-4 relative.  It acts on cd_X and cd_Y at the anchor and again now:
//     3 * 2.5e-4 < kTermRel = 1e-3 of (cd_X + cd_Y) covers both to first order with a quarter to spare;
//   * d's own evaluation (21 subtractions / products / sums, two sqrt, radius from one more sqrt: < 30 u relative) is covered
//     by applying kTermRel to 2 d as well;
//   * kTermAbs = 1e-6 absorbs flushed subnormals and makes an exact tie keep both terms.
// A term is dropped only on the STRICT inequality, so never both of a metric; any NaN or Inf among the operands (a term, a
// pose entry, the radius: 0 * Inf included) makes the comparisons false and keeps both terms (the margin takes |cd|, so an
// infinity of either sign turns both sides of its comparisons into Inf or NaN).
//   anchor  [kTermAnchorFloats] = cd[metric * 2 + dir] (8) | R (9) | T (3) of the anchor iteration
//   R, T    the pose the coming iteration moves the cloud with
// Returns the terms needed: bit m = the term of metric m over the target points (dir 0), bit 4 + m = over the moved points
// (dir 1).  Branch-free on purpose (selects on values): the kernels inline it into their scalar tail.
// ---------------------------------------------------------------------------------------------
constexpr int kTermAnchorFloats = 20;
constexpr float kTermRel = 1e-3f;
constexpr float kTermAbs = 1e-6f;
constexpr float kTermMoveErr = 1e-6f;

template <int NMET>
HOUV_HD inline unsigned term_masks(const float* anchor, const float* R, const float* T, float radius) {
  float fr = 0.f, ft = 0.f, tn = 0.f, ta = 0.f;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const float d = R[i] - anchor[8 + i];
    fr += d * d;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float d = T[i] - anchor[17 + i];
    ft += d * d;
    tn += T[i] * T[i];
    ta += anchor[17 + i] * anchor[17 + i];
  }
  const float delta2 = 2.0f * (sqrtf(fr) * radius + sqrtf(ft));
  const float abs_margin = kTermAbs + kTermMoveErr * (2.0f * radius + sqrtf(tn) + sqrtf(ta));
  unsigned need = ((1u << NMET) - 1u) * 0x11u;
#pragma unroll
  for (int m = 0; m < NMET; ++m) {
    const float c0 = anchor[2 * m], c1 = anchor[2 * m + 1];
    const float slack = delta2 + kTermRel * (fabsf(c0) + fabsf(c1) + delta2) + abs_margin;
    const unsigned drop1 = (c0 + slack < c1) ? (0x10u << m) : 0u;   // at most one of the two holds (slack > 0)
    const unsigned drop0 = (c1 + slack < c0) ? (1u << m) : 0u;
    need &= ~(drop0 | drop1);
  }
  return need;
}

// ---------------------------------------------------------------------------------------------
// Term masks with PER-TERM records (the rule solve.hip runs; term_masks above is the shared-anchor rule it grew out of and
// the reference it is tested against).  Every term Z carries its own record: its value cd_Z when it was last computed and
// the pose (R_Z, T_Z) it was computed at.  For metric m with terms X and Y, Y is dropped for the coming iteration iff
//   cd_X + d_X + d_Y + margin < cd_Y        (strictly),
// d_Z bounding how far any moved point now is from where it was at Z's record:
//   d_Z = rho(R, R_Z) * radius + |T - T_Z|.
// Proof: every term is 1-Lipschitz in the displacement (see above), so now  X <= cd_X + d_X  and  Y >= cd_Y - d_Y.
//
// rho bounds the spectral norm ||R - R_Z||_2.  For two exact rotations A, B:  A - B = (A B^T - I) B, and a rotation Q = A B^T
// by the angle t has the eigenvalues 1, e^{+-it}, so Q - I (normal) has the singular values 0, 2 sin(t/2), 2 sin(t/2):
//   ||A - B||_2 = 2 sin(t/2),  ||A - B||_F = sqrt(2) * 2 sin(t/2),  hence  ||A - B||_2 = ||A - B||_F / sqrt(2)  exactly.
// The poses are fp32 outputs of pose_forward, not exact rotations.  Write R = A S (polar decomposition, A orthogonal, S
// symmetric positive semi-definite with eigenvalues s_i): ||R - A||_F^2 = sum (s_i - 1)^2 <= sum (s_i^2 - 1)^2 =
// ||R^T R - I||_F^2 =: defect(R)^2, because |s - 1| <= |s - 1| (s + 1).  With B the polar factor of R_Z and
// e = defect(R) + defect(R_Z):
//   ||R - R_Z||_2 <= ||A - B||_2 + e = ||A - B||_F / sqrt(2) + e <= (||R - R_Z||_F + e) / sqrt(2) + e
//                 <  ||R - R_Z||_F / sqrt(2) + 2 e.
// That needs A B^T to be a ROTATION (for a reflection Q, Q - I has a singular value 2 and the identity fails).  A B^T is
// improper only when exactly one of A, B is; then ||A - B||_2 = 2, so ||R - R_Z||_F >= 2 - e.  The sqrt(2) form is therefore
// taken only where e <= kTermDefectMax = 1e-3 AND ||R - R_Z||_F^2 <= 2 (rotations up to 60 degrees apart; an optimiser step
// is far below), and only where it is the smaller bound; everywhere else rho is the Frobenius norm itself, as in term_masks.
// Each defect is evaluated here in fp32: 9 entries of R^T R - I, each three products of entries <= 1 summed and 1 taken off,
// <= 4 u of error, so <= 12 u = 7.2e-7 on the norm; kTermDefectErr = 1e-6 is added to each.
//
// Margin, re-derived for two records (u = 2^-24):
//   * move_point: a computed moved point is within 4.2e-7 * (radius + |T_pose|) of R p + T at any pose.  The computed X moved
//     by d_X plus that error at X's record pose and now; the same for Y: 4.2e-7 * (4 radius + |T_X| + |T_Y| + 2 |T|)
//     = 8.4e-7 * (2 radius + |T| + (|T_X| + |T_Y|) / 2) <= kTermMoveErr = 1e-6 times that sum (with both records at one
//     pose this is term_masks' margin);
//   * a computed term is within 2.5e-4 relative of the real one on the same computed points, at its record and now:
//     (1 + e)(cd_X / (1 - e) + d_X) < (1 - e)(cd_Y / (1 + e) - d_Y) follows from the rule to first order with
//     3 * 2.5e-4 < kTermRel of (cd_X + cd_Y + d_X + d_Y), which also covers the evaluation of d_X, d_Y themselves (< 60 u);
//   * kTermAbs absorbs flushed subnormals and makes an exact tie keep both terms.
// Strict inequality only, so never both terms of a metric; any NaN or Inf operand (a cd, an entry of any of the poses the
// metric uses, the radius; 0 * Inf included) makes the comparisons false: both terms kept.  Branch-free (selects on values).
//
// At most ONE term per metric is older than the last iteration in the kernels, so the records are passed as
//   cd     [8] = cd[metric * 2 + dir] when last computed
//   fresh  R (9) | T (3): the record pose of every term that is not stale (the pose of the iteration that just ended)
//   stale  R (9) | T (3) per metric, entry i of metric m at stale[(m * 12 + i) * stride]
//   stale_bits  bit m / bit 4 + m set: the record pose of the term (metric m, dir 0 / 1) is stale's; clear: fresh
//   R, T   the pose the coming iteration moves the cloud with
// Returns the terms needed, as term_masks does.
// ---------------------------------------------------------------------------------------------
constexpr float kTermDefectMax = 1e-3f;
constexpr float kTermDefectErr = 1e-6f;

// ||M^T M - I||_F + kTermDefectErr of a row-major 3x3
HOUV_HD inline float term_rot_defect(const float* M) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) {
      const float g = M[i] * M[j] + M[3 + i] * M[3 + j] + M[6 + i] * M[6 + j] - ((i == j) ? 1.0f : 0.0f);
      s += ((i == j) ? 1.0f : 2.0f) * g * g;
    }
  return sqrtf(s) + kTermDefectErr;
}

// d_Z and |T_Z| of one record pose; def_now = term_rot_defect(R)
HOUV_HD inline void term_travel(const float* Rz, const float* Tz, const float* R, const float* T, float def_now, float radius,
                                float& d, float& tz) {
  float fr = 0.f, ft = 0.f, ta = 0.f;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const float e = R[i] - Rz[i];
    fr += e * e;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float e = T[i] - Tz[i];
    ft += e * e;
    ta += Tz[i] * Tz[i];
  }
  const float fro = sqrtf(fr), defect = def_now + term_rot_defect(Rz);
  const float tight = fro * 0.70710683f + 2.0f * defect;   // the constant is 1 / sqrt(2) rounded UP
  const bool ok = (fr <= 2.0f) & (defect <= kTermDefectMax) & (tight < fro);   // any NaN: false, and fro is NaN too
  d = (ok ? tight : fro) * radius + sqrtf(ft);
  tz = sqrtf(ta);
}

template <int NMET>
HOUV_HD inline unsigned term_anchor_masks(const float* cd, const float* fresh, const float* stale, int stride,
                                          unsigned stale_bits, const float* R, const float* T, float radius_in) {
  const float radius = fabsf(radius_in);   // a negative infinity must not turn the slack negative
  const float def_now = term_rot_defect(R);
  const float tn = sqrtf(T[0] * T[0] + T[1] * T[1] + T[2] * T[2]);
  float d_f, t_f;
  term_travel(fresh, fresh + 9, R, T, def_now, radius, d_f, t_f);
  unsigned need = ((1u << NMET) - 1u) * 0x11u;
#pragma unroll
  for (int m = 0; m < NMET; ++m) {
    float Rs[9], Ts[3], d_s, t_s;
#pragma unroll
    for (int i = 0; i < 9; ++i) Rs[i] = stale[(m * 12 + i) * stride];
#pragma unroll
    for (int i = 0; i < 3; ++i) Ts[i] = stale[(m * 12 + 9 + i) * stride];
    term_travel(Rs, Ts, R, T, def_now, radius, d_s, t_s);
    const bool s0 = (stale_bits >> m) & 1u, s1 = (stale_bits >> (4 + m)) & 1u;
    const float d0 = s0 ? d_s : d_f, d1 = s1 ? d_s : d_f;
    const float t0 = s0 ? t_s : t_f, t1 = s1 ? t_s : t_f;
    const float c0 = cd[2 * m], c1 = cd[2 * m + 1];
    const float dd = d0 + d1;
    const float slack = dd + kTermRel * (fabsf(c0) + fabsf(c1) + dd) + kTermAbs +
                        kTermMoveErr * (2.0f * radius + tn + 0.5f * (t0 + t1));
    const unsigned drop1 = (c0 + slack < c1) ? (0x10u << m) : 0u;   // at most one of the two holds (slack > 0)
    const unsigned drop0 = (c1 + slack < c0) ? (1u << m) : 0u;
    need &= ~(drop0 | drop1);
  }
  return need;
}

// Walk variants of the pruned solve (houv_sweep.h, pruned_sweep_sorted).  A direction's four-bit `need` (one half of the word
// above) selects code specialised at compile time for a metric set MSET: a metric outside MSET costs the box tests and the walk
// nothing.  Any MSET that contains `need` is correct -- an extra metric is computed for nothing, as all of them were before -- so
// only the sets of kWalkSets are instantiated and every other mask runs on the cheapest instantiated superset.  15 is always
// present.  The sets were chosen from the histogram of the masks the walks see at 2,048 points (houv_debug_set("solve_walk_hist");
// profiles/r12_walk_variants.txt): greedily by instructions removed under walk_step_cost, until the next set removes less than
// 1 % of a walk step.  Each set is another copy of the box tests and of the walk at both sweep sites (+18 % code for five).
constexpr int kWalkSets[] = {6, 11, 12, 13, 15};
constexpr int kNumWalkSets = (int)(sizeof(kWalkSets) / sizeof(kWalkSets[0]));
// VALU instructions of one walk step (a query against one 32-point sub-tile) that depend on the metric set: per two references
// one fma per metric kept (metric 3's also feeds metric 0), the mul of y^2 for metric 1 alone, one min3 per metric; per step
// five instructions of unit bookkeeping per metric.  The loads, the six subtractions and x^2 are common to all sets.
constexpr int walk_step_cost(unsigned mset) {
  const int k0 = (int)(mset & 1u), k1 = (int)((mset >> 1) & 1u), k2 = (int)((mset >> 2) & 1u), k3 = (int)((mset >> 3) & 1u);
  return 16 * (2 * (k0 + k1 + k2 + ((k0 | k3) ? 1 : 0)) + 2 * k1 + (k0 + k1 + k2 + k3)) + 5 * (k0 + k1 + k2 + k3);
}
constexpr bool walk_instantiated(unsigned mset) {
  for (int i = 0; i < kNumWalkSets; ++i)
    if ((unsigned)kWalkSets[i] == mset) return true;
  return false;
}
// the instantiated set that mask `need` (0..15) runs on: the cheapest one that contains it, the lowest set on a tie
constexpr unsigned walk_variant(unsigned need) {
  unsigned best = 15u;
  for (int i = 0; i < kNumWalkSets; ++i) {
    const unsigned s = (unsigned)kWalkSets[i];
    if ((s & need) == need && walk_step_cost(s) < walk_step_cost(best)) best = s;
  }
  return best;
}
static_assert(walk_instantiated(15u) && walk_variant(15u) == 15u && walk_step_cost(15u) == 16 * 14 + 20, "today's code is a variant");
// walk_variant() of all 16 masks, four bits each: what the kernel looks up with one scalar shift
constexpr unsigned long long walk_variant_table() {
  unsigned long long t = 0ull;
  for (unsigned n = 0; n < 16u; ++n) t |= (unsigned long long)walk_variant(n) << (4 * n);
  return t;
}

// ---------------------------------------------------------------------------------------------
// Box tests of the pruned solve (houv_sweep.h, prune_masks) and their cull per GROUP of queries.
//
// Per query and reference box the kernel asks: is the box, for some metric m of the set, no farther from the query than the
// query's bound ub[m]?  box_test_query restates that test for the host, instruction for instruction: the offset per axis is the
// query minus the query clamped into the box (v_med3_f32), squared and summed per metric in the order of metric_sqdist, `<=`.
//
// box_test_group is the same question for a whole group of queries at once -- the 64 queries of one k of a wave, two k-d leaves
// of a sorted cloud -- and is the code the kernel runs: the group's box [glo, ghi] (min / max of the queries' coordinates, NaN
// left out) against the reference box, with the group's LARGEST bound per metric (NaN left out).  A box that fails it fails the
// test of every query of the group, so the per-query tests run over the surviving boxes only and give the bits they gave before.
//
// Why it is exact, not merely safe in exact arithmetic:
//   * fp32 subtraction, multiplication and fma round monotonically in each operand.
//   * With L = min(lo, hi), H = max(lo, hi) of the reference box on an axis (the clamp takes its bounds in either order), a
//     query's offset is |q - med3(q, lo, hi)| = max(fl(L - q), fl(q - H), 0): fl(a - b) = -fl(b - a), and the sign is squared
//     away.  For glo <= q <= ghi, fl(L - q) >= fl(L - ghi) and fl(q - H) >= fl(glo - H): the offset is >= the group's gap
//     g = max(fl(L - ghi), fl(glo - H), 0) on every axis.
//   * The same mul / fma tree over non-negative operands, each >= the group's: s_m(query) >= s_m(group) in fp32.
//   * ub[m] of the query <= the group's bound.  So s_m(group) > bound, for every m of the set, gives s_m(query) > ub[m]: fail.
//   * NaN: a gap is never NaN (the maxima leave NaN out; Inf - Inf on one side leaves the other side or 0: a smaller gap, which
//     only lets a box survive), so neither is s_m(group).  The group box is formed per axis, and a NaN coordinate is left out
//     of its own axis only: a query with a NaN on an axis has a NaN offset there and fails every metric that reads the axis, as
//     before; a view that drops the axis reads the other two, on which the query IS inside the group box, and the argument
//     above holds for it.  A NaN bound passes nothing in either test; the group's bound is NaN only when every query's is.
// ---------------------------------------------------------------------------------------------
// v_med3_f32: the median of three numbers; with a NaN among them, the minimum of the others
HOUV_HD inline float box_med3(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_fmed3f(a, b, c);
#else
  if (a != a || b != b || c != c) return fminf(fminf(a, b), c);
  return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c));
#endif
}

// s_m of the offsets (dx, dy, dz) for the metrics of `mset` against the bounds b[m]: the expression trees of prune_masks
template <int NMET>
HOUV_HD inline bool box_within_bounds(float dx, float dy, float dz, const float* b, unsigned mset) {
  if constexpr (NMET == 4) {
    const float xx = dx * dx, yy = dy * dy;
    const float s3 = __builtin_fmaf(dy, dy, xx), s1 = __builtin_fmaf(dz, dz, yy), s2 = __builtin_fmaf(dz, dz, xx);
    const float s0 = __builtin_fmaf(dz, dz, s3);
    bool in = false;
    if (mset & 1u) in |= s0 <= b[0];
    if (mset & 2u) in |= s1 <= b[1];
    if (mset & 4u) in |= s2 <= b[2];
    if (mset & 8u) in |= s3 <= b[3];
    return in;
  } else {
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)) <= b[0];
  }
}

// the per-query test, restated (q, lo, hi: x, y, z; ub: one bound per metric, -1 = the metric's term is not computed)
template <int NMET>
HOUV_HD inline bool box_test_query(const float* q, const float* lo, const float* hi, const float* ub, unsigned mset) {
  return box_within_bounds<NMET>(q[0] - box_med3(q[0], lo[0], hi[0]), q[1] - box_med3(q[1], lo[1], hi[1]),
                                 q[2] - box_med3(q[2], lo[2], hi[2]), ub, mset);
}

// gap between the group's interval [glo, ghi] and the box's, whichever way round its bounds are; never NaN
HOUV_HD inline float box_group_gap(float glo, float ghi, float lo, float hi) {
  return fmaxf(fmaxf(fminf(lo, hi) - ghi, glo - fmaxf(lo, hi)), 0.0f);
}

// the group verdict: false = no query inside [glo, ghi] with bounds <= gub passes box_test_query on this box
template <int NMET>
HOUV_HD inline bool box_test_group(const float* glo, const float* ghi, const float* lo, const float* hi, const float* gub,
                                   unsigned mset) {
  return box_within_bounds<NMET>(box_group_gap(glo[0], ghi[0], lo[0], hi[0]), box_group_gap(glo[1], ghi[1], lo[1], hi[1]),
                                 box_group_gap(glo[2], ghi[2], lo[2], hi[2]), gub, mset);
}

// ---------------------------------------------------------------------------------------------
// 3x3 SVD by one-sided (Hestenes) Jacobi, register resident.  H = U diag(S) V^T, S sorted
// descending like torch.svd (model_utils.py:233).
// ---------------------------------------------------------------------------------------------
template <typename T>
HOUV_HD inline void svd3x3(const T H[9], T U[9], T S[3], T V[9]) {
  T B[9];
  for (int i = 0; i < 9; ++i) { B[i] = H[i]; V[i] = (i % 4 == 0) ? (T)1 : (T)0; }
  const int P[3] = {0, 0, 1}, Qi[3] = {1, 2, 2};
  for (int sweep = 0; sweep < 12; ++sweep) {
    T off = 0;
    for (int r = 0; r < 3; ++r) {
      const int p = P[r], q = Qi[r];
      const T a = B[0 * 3 + p] * B[0 * 3 + p] + B[1 * 3 + p] * B[1 * 3 + p] + B[2 * 3 + p] * B[2 * 3 + p];
      const T b = B[0 * 3 + q] * B[0 * 3 + q] + B[1 * 3 + q] * B[1 * 3 + q] + B[2 * 3 + q] * B[2 * 3 + q];
      const T g = B[0 * 3 + p] * B[0 * 3 + q] + B[1 * 3 + p] * B[1 * 3 + q] + B[2 * 3 + p] * B[2 * 3 + q];
      // converged for this pair when |g| <= eps * |b_p||b_q|
      const T eps2 = sizeof(T) == 4 ? (T)1e-14 : (T)1e-31;
      if (g * g <= eps2 * a * b) continue;
      off += (T)1;
      const T zeta = (b - a) / ((T)2 * g);
      const T az = zeta < 0 ? -zeta : zeta;
      const T t = (zeta < 0 ? (T)-1 : (T)1) / (az + tsqrt((T)1 + zeta * zeta));
      const T c = (T)1 / tsqrt((T)1 + t * t);
      const T s = c * t;
      for (int i = 0; i < 3; ++i) {
        const T bp = B[i * 3 + p], bq = B[i * 3 + q];
        B[i * 3 + p] = c * bp - s * bq;
        B[i * 3 + q] = s * bp + c * bq;
        const T vp = V[i * 3 + p], vq = V[i * 3 + q];
        V[i * 3 + p] = c * vp - s * vq;
        V[i * 3 + q] = s * vp + c * vq;
      }
    }
    if (off == (T)0) break;
  }
  for (int j = 0; j < 3; ++j)
    S[j] = tsqrt(B[0 * 3 + j] * B[0 * 3 + j] + B[1 * 3 + j] * B[1 * 3 + j] + B[2 * 3 + j] * B[2 * 3 + j]);
  // sort columns by S descending (3-element network)
  auto swapcol = [&](int x, int y) {
    T ts = S[x]; S[x] = S[y]; S[y] = ts;
    for (int i = 0; i < 3; ++i) {
      T tb = B[i * 3 + x]; B[i * 3 + x] = B[i * 3 + y]; B[i * 3 + y] = tb;
      T tv = V[i * 3 + x]; V[i * 3 + x] = V[i * 3 + y]; V[i * 3 + y] = tv;
    }
  };
  if (S[0] < S[1]) swapcol(0, 1);
  if (S[1] < S[2]) swapcol(1, 2);
  if (S[0] < S[1]) swapcol(0, 1);
  // U columns = B columns / S; rank-deficient columns are completed to a right-handed orthonormal set
  const T tiny = S[0] * (sizeof(T) == 4 ? (T)1e-6 : (T)1e-13);
  for (int j = 0; j < 2; ++j) {
    if (S[j] > tiny && S[j] > (T)0) {
      for (int i = 0; i < 3; ++i) U[i * 3 + j] = B[i * 3 + j] / S[j];
    } else if (j == 0) {
      U[0] = 1; U[3] = 0; U[6] = 0;
    } else {
      // any unit vector orthogonal to u0
      const T x = U[0], y = U[3], z = U[6];
      const T ax = x < 0 ? -x : x, ay = y < 0 ? -y : y, az = z < 0 ? -z : z;
      T e[3] = {0, 0, 0};
      if (ax <= ay && ax <= az) e[0] = 1; else if (ay <= az) e[1] = 1; else e[2] = 1;
      T w[3] = {y * e[2] - z * e[1], z * e[0] - x * e[2], x * e[1] - y * e[0]};
      const T n = tsqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
      U[1] = w[0] / n; U[4] = w[1] / n; U[7] = w[2] / n;
    }
  }
  if (S[2] > tiny && S[2] > (T)0) {
    for (int i = 0; i < 3; ++i) U[i * 3 + 2] = B[i * 3 + 2] / S[2];
  } else {
    U[2] = U[3] * U[7] - U[6] * U[4];
    U[5] = U[6] * U[1] - U[0] * U[7];
    U[8] = U[0] * U[4] - U[3] * U[1];
  }
}

template <typename T>
HOUV_HD inline T det3(const T m[9]) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// model_utils.py:232-240: r = v u^T; if det(r) < 0 flip the last column of v and recompute.
template <typename T>
HOUV_HD inline void kabsch_rotation(const T H[9], T R[9]) {
  T U[9], S[3], V[9];
  svd3x3<T>(H, U, S, V);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = V[i * 3 + 0] * U[j * 3 + 0] + V[i * 3 + 1] * U[j * 3 + 1] + V[i * 3 + 2] * U[j * 3 + 2];
  if (det3<T>(R) < (T)0) {
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) R[i * 3 + j] = V[i * 3 + 0] * U[j * 3 + 0] + V[i * 3 + 1] * U[j * 3 + 1] - V[i * 3 + 2] * U[j * 3 + 2];
  }
}

// ---- stage scheduling (houv_solve_stage, solve.hip): a stage of n_iters iterations is cut into chunks of chunk_iters (the last
// one what is left); ticket t of the persistent grid is the item (chunk = t / ninst, hypothesis = t % ninst), chunk-major ----
HOUV_HD inline int sched_chunks(int n_iters, int chunk_iters) { return (n_iters - 1) / chunk_iters + 1; }   // n_iters, chunk_iters >= 1; no overflow
// items of a stage; 64-bit on the host (the entry point refuses a stage whose tickets do not fit an int), int in the kernel
HOUV_HD inline long long sched_items64(int ninst, int n_iters, int chunk_iters) {
  return (long long)ninst * sched_chunks(n_iters, chunk_iters);
}
HOUV_HD inline int sched_items(int ninst, int n_iters, int chunk_iters) { return ninst * sched_chunks(n_iters, chunk_iters); }
// iterations of chunk `chunk`; it starts at steps_done + chunk * chunk_iters and finds the workspace valid when the stage did
// or when chunk > 0
HOUV_HD inline int sched_item_iters(int n_iters, int chunk_iters, int chunk) {
  const int left = n_iters - chunk * chunk_iters;
  return left < chunk_iters ? left : chunk_iters;
}

}  // namespace houv
