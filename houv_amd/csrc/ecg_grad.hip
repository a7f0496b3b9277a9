// ecg_grad.hip -- training support for Dense_conv (houv_dense_conv, ecg.hip):
//
//   houv_dense_conv_arg        houv_dense_conv (the unchanged forward kernel writes `out`) followed by a second comparing pass, a
//                              kernel of its own, that recomputes the three layers by the forward's chains and records for each of
//                              the 72 pooled channels the lowest edge slot that attains the maximum.
//   houv_dense_conv_backward   four steps, no float atomics, every sum in a fixed order:
//     1. edge kernel (lane = point, the k edges in a loop): recomputes y0 and s1 by the forward's chains, forms gs2, gs1, gy0 with
//        the transposed weights at wave-uniform LDS addresses, writes gy0 (channel-major) and the clamped neighbour index to the
//        workspace, keeps the per-point sum of gs1, and reduces the per-edge weight gradients inside the workgroup: the 128
//        lanes stage (gy0, gs1, gs2 | x_j - x_i, y0, s1) in LDS and every thread owns a 4 x 6 block of gW elements.
//     2. houv_scatter_points_grad sums gy0 per destination in ascending (i, e) order (the neighbour path is linear, so
//        W0[:, C:]^T is applied once per point afterwards).
//     3. point kernel (lane = point): everything that is linear in the per-point sums Gy0 = sum_e gy0, Gs1, Gs2 and D (the
//        destination sum) -- gx, the x_i columns of the three weight gradients and the biases -- again reduced through LDS.
//     4. the workgroups' partials are added in workgroup order.
#include "../../include/houv_hip.h"
#include "houv_common.h"

namespace houv {
namespace {

constexpr int kG = HOUV_DENSE_CONV_GROWTH;
constexpr int kNT = 128;                         // lanes (points) per workgroup, as in the forward
static_assert(kG == 24, "the tiles below are written for 24 output channels");

// ------------------------------------------------------------------------------------------------------------------
// where each maximum sits
// ------------------------------------------------------------------------------------------------------------------
// the first candidate that is not NaN is always taken (a true -inf included), after that only a strictly larger one: the lowest
// slot that attains the maximum, -1 when every candidate is NaN
__device__ __forceinline__ void track(float v, int e, float& m, int& a) {
  if (v > m || (a < 0 && v == v)) { m = v; a = e; }
}

template <int C>
__global__ __launch_bounds__(kNT) void dense_conv_arg_kernel(const float* __restrict__ x, int ldx, const int* __restrict__ idx, int N,
                                                             int k, const float* __restrict__ W0, const float* __restrict__ b0,
                                                             const float* __restrict__ W1, const float* __restrict__ b1,
                                                             const float* __restrict__ W2, const float* __restrict__ b2,
                                                             signed char* __restrict__ arg) {
  constexpr int L0 = 2 * C, L1 = kG + C, L2 = 2 * kG + C;
  __shared__ __attribute__((aligned(16))) float W0s[kG * L0];
  __shared__ __attribute__((aligned(16))) float W1s[kG * L1];
  __shared__ __attribute__((aligned(16))) float W2s[kG * L2];
  __shared__ float bs[3][kG];
  const int b = blockIdx.y, tid = threadIdx.x;
  for (int e = tid; e < kG * L0; e += kNT) W0s[e] = W0[e];
  for (int e = tid; e < kG * L1; e += kNT) W1s[e] = W1[e];
  for (int e = tid; e < kG * L2; e += kNT) W2s[e] = W2[e];
  if (tid < kG) { bs[0][tid] = b0[tid]; bs[1][tid] = b1[tid]; bs[2][tid] = b2[tid]; }
  __syncthreads();

  const int pi = blockIdx.x * kNT + tid;
  const bool ok = pi < N;
  const int i = min(pi, N - 1);
  const float* __restrict__ xb = x + (size_t)b * N * ldx;
  const int* __restrict__ nb = idx + ((size_t)b * N + i) * k;

  float xi[C];
#pragma unroll
  for (int c = 0; c < C; ++c) xi[c] = xb[(size_t)i * ldx + c];
  float pre0[kG], q1[kG], q2[kG];
#pragma unroll
  for (int o = 0; o < kG; ++o) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      a0 = __builtin_fmaf(W0s[o * L0 + c], xi[c], a0);
      a1 = __builtin_fmaf(W1s[o * L1 + kG + c], xi[c], a1);
      a2 = __builtin_fmaf(W2s[o * L2 + kG + c], xi[c], a2);
    }
    pre0[o] = a0;
    q1[o] = a1 + bs[1][o];
    q2[o] = a2 + bs[2][o];
  }

  float m0[kG], m1[kG], m2[kG];
  int r0[kG], r1[kG], r2[kG];
#pragma unroll
  for (int o = 0; o < kG; ++o) { m0[o] = m1[o] = m2[o] = -__builtin_inff(); r0[o] = r1[o] = r2[o] = -1; }

#pragma unroll 1
  for (int e = 0; e < k; ++e) {
    int z = 0;                                   // keeps the weight reads inside the loop, as in the forward
    asm volatile("" : "+s"(z));
    const float* __restrict__ W0e = W0s + z;
    const float* __restrict__ W1e = W1s + z;
    const float* __restrict__ W2e = W2s + z;
    const int j = min(max(nb[e], 0), N - 1);
    const float* __restrict__ xj = xb + (size_t)j * ldx;
    float y0[kG], s1[kG];
#pragma unroll
    for (int o = 0; o < kG; ++o) y0[o] = pre0[o];
#pragma unroll
    for (int c4 = 0; c4 < C; c4 += 4) {
      float t[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) t[c] = xj[c4 + c] - xi[c4 + c];
#pragma unroll
      for (int o = 0; o < kG; ++o)
#pragma unroll
        for (int c = 0; c < 4; ++c) y0[o] = __builtin_fmaf(W0e[o * L0 + C + c4 + c], t[c], y0[o]);
    }
#pragma unroll
    for (int o = 0; o < kG; ++o) {
      y0[o] = __builtin_fmaxf(y0[o] + bs[0][o], 0.f);
      track(y0[o], e, m0[o], r0[o]);
    }
#pragma unroll
    for (int o = 0; o < kG; ++o) {
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < kG; ++c) a = __builtin_fmaf(W1e[o * L1 + c], y0[c], a);
      s1[o] = __builtin_fmaxf(a + q1[o], 0.f);
      track(s1[o], e, m1[o], r1[o]);
    }
#pragma unroll
    for (int o = 0; o < kG; ++o) {
      float a = 0.f, c2 = 0.f;
#pragma unroll
      for (int c = 0; c < kG; ++c) a = __builtin_fmaf(W2e[o * L2 + c], y0[c], a);
#pragma unroll
      for (int c = 0; c < kG; ++c) c2 = __builtin_fmaf(W2e[o * L2 + kG + C + c], s1[c], c2);
      track((a + q2[o]) + c2, e, m2[o], r2[o]);
    }
  }

  if (ok) {
    signed char* __restrict__ a_ = arg + ((size_t)b * N + pi) * (3 * kG);
#pragma unroll
    for (int o = 0; o < kG; ++o) {
      a_[o] = (signed char)r0[o];
      a_[kG + o] = (signed char)r1[o];
      a_[2 * kG + o] = (signed char)r2[o];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------
// One row of partials per workgroup: [gW0 (24 x 2C) | gW1 (24 x (24 + C)) | gW2 (24 x (48 + C)) | gb0 gb1 gb2].
template <int C>
struct Bw {
  static constexpr int L0 = 2 * C, L1 = kG + C, L2 = 2 * kG + C;
  static constexpr int P0 = 0, P1 = P0 + kG * L0, P2 = P1 + kG * L1, PB = P2 + kG * L2, R = PB + 3 * kG;
  // LDS of the edge kernel, in floats (every offset a multiple of 4)
  static constexpr int oW0 = 0, oW1 = oW0 + kG * L0, oW1aT = oW1 + kG * L1, oW2aT = oW1aT + kG * kG, oW2cT = oW2aT + kG * kG,
                       oB = oW2cT + kG * kG, oStage = oB + 2 * kG;
  // a lane's staged row: [gy0 | gs1 | gs2 | x_j - x_i | y0 | s1]; the stride keeps 16-byte alignment and spreads the lanes' rows
  // over the banks (S mod 64 = 4 or 20)
  static constexpr int aGY0 = 0, aGS1 = kG, aGS2 = 2 * kG, bT = 3 * kG, bY0 = 3 * kG + C, bS1 = 4 * kG + C;
  static constexpr int S = C == 48 ? 196 : 148;
  static constexpr int ldsEdge = oStage + kNT * S;
  static constexpr int tilesA = 6 * (C / 6), tilesEdge = tilesA + 3 * 24;     // 4 x 6 blocks of gW0[:, C:], gW1[:, :24], gW2[:, :24], gW2[:, 24+C:]
  // the point kernel: [Gy0 | Gs1 | Gs2 | x_i | D - Gy0], 6 x 6 blocks of the 72 x C products
  static constexpr int S2 = C == 48 ? 148 : 132;
  static constexpr int ldsPoint = kNT * S2;
  static constexpr int tilesPoint = 12 * (C / 6);
  static_assert(5 * kG + C <= S && 4 * kG + C <= S2 && tilesEdge <= kNT && tilesPoint <= kNT && C % 6 == 0, "tiling");
};

__device__ __forceinline__ int arg_byte(const unsigned (&w)[18], int c) { return (int)((w[c >> 2] >> (8 * (c & 3))) & 0xffu); }

template <int C>
__global__ __launch_bounds__(kNT) void dense_conv_bw_edge_kernel(
    const float* __restrict__ x, int ldx, const int* __restrict__ idx, int N, int k, const float* __restrict__ W0,
    const float* __restrict__ b0, const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2,
    int relu_out, const signed char* __restrict__ arg, const float* __restrict__ out, int ldo, const float* __restrict__ gout,
    int ldg, float* __restrict__ gy0T, int* __restrict__ keys, float* __restrict__ Gs1w, float* __restrict__ part) {
  using D = Bw<C>;
  constexpr int L0 = D::L0, L1 = D::L1, L2 = D::L2, S = D::S;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* W0s = smem + D::oW0;
  float* W1s = smem + D::oW1;
  float* W1aT = smem + D::oW1aT;                 // [c][o] = W1[o][c]
  float* W2aT = smem + D::oW2aT;                 // [c][o] = W2[o][c]
  float* W2cT = smem + D::oW2cT;                 // [c][o] = W2[o][G + C + c]
  float* bs = smem + D::oB;                      // b0, b1
  float* stage = smem + D::oStage;
  const int b = blockIdx.y, tid = threadIdx.x;
  for (int e = tid; e < kG * L0; e += kNT) W0s[e] = W0[e];
  for (int e = tid; e < kG * L1; e += kNT) W1s[e] = W1[e];
  for (int e = tid; e < kG * kG; e += kNT) {
    const int c = e / kG, o = e - c * kG;
    W1aT[e] = W1[o * L1 + c];
    W2aT[e] = W2[o * L2 + c];
    W2cT[e] = W2[o * L2 + kG + C + c];
  }
  if (tid < kG) { bs[tid] = b0[tid]; bs[kG + tid] = b1[tid]; }
  __syncthreads();

  const int pi = blockIdx.x * kNT + tid;
  const bool ok = pi < N;
  const int i = min(pi, N - 1);                  // lanes past the cloud repeat its last point; they store nothing and are not summed
  const int nvalid = min(kNT, N - (int)blockIdx.x * kNT);
  const float* __restrict__ xb = x + (size_t)b * N * ldx;
  const size_t row = (size_t)b * N + i;
  const int* __restrict__ nb = idx + row * k;

  float xi[C];
#pragma unroll
  for (int c = 0; c < C; ++c) xi[c] = xb[(size_t)i * ldx + c];
  // the centre's share of the first two layers, once per point, by the forward's chains.  The loop over o stays rolled and
  // hands its results over through the lane's own staging row: unrolled, every weight of the prologue is read ahead of the
  // first fma and spills.
  float* __restrict__ st = stage + tid * S;
#pragma unroll 1
  for (int o = 0; o < kG; ++o) {
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      a0 = __builtin_fmaf(W0s[o * L0 + c], xi[c], a0);
      a1 = __builtin_fmaf(W1s[o * L1 + kG + c], xi[c], a1);
    }
    st[o] = a0;
    st[kG + o] = a1 + bs[kG + o];
  }
  float pre0[kG], q1[kG];
#pragma unroll
  for (int o = 0; o < kG; ++o) { pre0[o] = st[o]; q1[o] = st[kG + o]; }
  // the gradient of the three pooled groups (the pass-through columns belong to the point kernel) and their winners
  float g0[kG], g1[kG], g2[kG];
  {
    const float* __restrict__ gr = gout + row * ldg;
    const float* __restrict__ orow = relu_out ? out + row * ldo : nullptr;
#pragma unroll
    for (int o = 0; o < kG; ++o) {
      g0[o] = gr[o]; g1[o] = gr[kG + C + o]; g2[o] = gr[2 * kG + C + o];
      if (relu_out) {
        g0[o] = orow[o] > 0.f ? g0[o] : 0.f;
        g1[o] = orow[kG + C + o] > 0.f ? g1[o] : 0.f;
        g2[o] = orow[2 * kG + C + o] > 0.f ? g2[o] : 0.f;
      }
    }
  }
  unsigned aw[18];
  {
    const unsigned* __restrict__ ar = reinterpret_cast<const unsigned*>(arg + row * (3 * kG));   // 72-byte rows: 4-byte aligned
#pragma unroll
    for (int q = 0; q < 18; ++q) aw[q] = ar[q];
  }

  // this thread's 4 x 6 block of weight-gradient elements
  int aoff = 0, boff = 0, opos = 0, old = 0;
  {
    int t = tid;
    const int rg = t % 6;
    if (t < D::tilesA) {
      const int cg = t / 6;
      aoff = D::aGY0 + 4 * rg; boff = D::bT + 6 * cg; old = L0; opos = D::P0 + 4 * rg * L0 + C + 6 * cg;
    } else {
      t -= D::tilesA;
      const int grp = t / 24, cg = (t % 24) / 6;
      if (grp == 0) { aoff = D::aGS1 + 4 * rg; boff = D::bY0 + 6 * cg; old = L1; opos = D::P1 + 4 * rg * L1 + 6 * cg; }
      else if (grp == 1) { aoff = D::aGS2 + 4 * rg; boff = D::bY0 + 6 * cg; old = L2; opos = D::P2 + 4 * rg * L2 + 6 * cg; }
      else { aoff = D::aGS2 + 4 * rg; boff = D::bS1 + 6 * cg; old = L2; opos = D::P2 + 4 * rg * L2 + kG + C + 6 * cg; }
    }
  }
  const bool owner = tid < D::tilesEdge;
  float acc[24];
#pragma unroll
  for (int q = 0; q < 24; ++q) acc[q] = 0.f;
  float Gs1[kG];
#pragma unroll
  for (int o = 0; o < kG; ++o) Gs1[o] = 0.f;

#pragma unroll 1
  for (int e = 0; e < k; ++e) {
    int z = 0;                                   // keeps the weight reads inside the loop, as in the forward
    asm volatile("" : "+s"(z));
    const float* __restrict__ W0e = W0s + z;
    const float* __restrict__ W1e = W1s + z;
    const float* __restrict__ W1aTe = W1aT + z;
    const float* __restrict__ W2aTe = W2aT + z;
    const float* __restrict__ W2cTe = W2cT + z;
    const int j = min(max(nb[e], 0), N - 1);
    if (ok) keys[row * k + e] = j;
    const float* __restrict__ xj = xb + (size_t)j * ldx;
    float y0[kG], s1[kG];
#pragma unroll
    for (int o = 0; o < kG; ++o) y0[o] = pre0[o];
#pragma unroll
    for (int c4 = 0; c4 < C; c4 += 4) {
      float t[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) t[c] = xj[c4 + c] - xi[c4 + c];
      *reinterpret_cast<float4*>(st + D::bT + c4) = make_float4(t[0], t[1], t[2], t[3]);
#pragma unroll
      for (int o = 0; o < kG; ++o)
#pragma unroll
        for (int c = 0; c < 4; ++c) y0[o] = __builtin_fmaf(W0e[o * L0 + C + c4 + c], t[c], y0[o]);
    }
#pragma unroll
    for (int o = 0; o < kG; ++o) y0[o] = __builtin_fmaxf(y0[o] + bs[o], 0.f);
#pragma unroll
    for (int o = 0; o < kG; ++o) {
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < kG; ++c) a = __builtin_fmaf(W1e[o * L1 + c], y0[c], a);
      s1[o] = __builtin_fmaxf(a + q1[o], 0.f);
    }
#pragma unroll
    for (int q = 0; q < kG; q += 4) {
      *reinterpret_cast<float4*>(st + D::bY0 + q) = make_float4(y0[q], y0[q + 1], y0[q + 2], y0[q + 3]);
      *reinterpret_cast<float4*>(st + D::bS1 + q) = make_float4(s1[q], s1[q + 1], s1[q + 2], s1[q + 3]);
    }
    // gs2, gs1, gy0: each pooled gradient goes to the edge that won; the products with the transposed weights run o ascending
    float gs2[kG], gs1[kG], gy0[kG];
#pragma unroll
    for (int o = 0; o < kG; ++o) gs2[o] = arg_byte(aw, 2 * kG + o) == e ? g2[o] : 0.f;
#pragma unroll
    for (int c = 0; c < kG; ++c) {
      float a = 0.f;
#pragma unroll
      for (int o = 0; o < kG; ++o) a = __builtin_fmaf(W2cTe[c * kG + o], gs2[o], a);
      a += arg_byte(aw, kG + c) == e ? g1[c] : 0.f;
      gs1[c] = s1[c] > 0.f ? a : 0.f;
      Gs1[c] += gs1[c];
    }
#pragma unroll
    for (int c = 0; c < kG; ++c) {
      float a = 0.f, a2 = 0.f;
#pragma unroll
      for (int o = 0; o < kG; ++o) a = __builtin_fmaf(W1aTe[c * kG + o], gs1[o], a);
#pragma unroll
      for (int o = 0; o < kG; ++o) a2 = __builtin_fmaf(W2aTe[c * kG + o], gs2[o], a2);
      a = (a + a2) + (arg_byte(aw, c) == e ? g0[c] : 0.f);
      gy0[c] = y0[c] > 0.f ? a : 0.f;
    }
#pragma unroll
    for (int q = 0; q < kG; q += 4) {
      *reinterpret_cast<float4*>(st + D::aGY0 + q) = make_float4(gy0[q], gy0[q + 1], gy0[q + 2], gy0[q + 3]);
      *reinterpret_cast<float4*>(st + D::aGS1 + q) = make_float4(gs1[q], gs1[q + 1], gs1[q + 2], gs1[q + 3]);
      *reinterpret_cast<float4*>(st + D::aGS2 + q) = make_float4(gs2[q], gs2[q + 1], gs2[q + 2], gs2[q + 3]);
    }
    if (ok) {
      float* __restrict__ gy = gy0T + ((size_t)b * kG * N + pi) * k + e;     // [b][c][i*k + e]
#pragma unroll
      for (int c = 0; c < kG; ++c) gy[(size_t)c * N * k] = gy0[c];
    }
    __syncthreads();
    // the workgroup's share of the per-edge weight gradients: lanes ascending, the reads of several lanes in flight at once
    if (owner) {
      const float* __restrict__ sa = stage + aoff;
      const float* __restrict__ sb = stage + boff;
#pragma unroll 4
      for (int p = 0; p < nvalid; ++p) {
        const float4 a = *reinterpret_cast<const float4*>(sa + p * S);
        const float2 u0 = *reinterpret_cast<const float2*>(sb + p * S);
        const float2 u1 = *reinterpret_cast<const float2*>(sb + p * S + 2);
        const float2 u2 = *reinterpret_cast<const float2*>(sb + p * S + 4);
        const float av[4] = {a.x, a.y, a.z, a.w};
        const float bv[6] = {u0.x, u0.y, u1.x, u1.y, u2.x, u2.y};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 6; ++c) acc[r * 6 + c] = __builtin_fmaf(av[r], bv[c], acc[r * 6 + c]);
      }
    }
    __syncthreads();
  }

  if (ok) {
    float* __restrict__ gs = Gs1w + row * kG;
#pragma unroll
    for (int o = 0; o < kG; ++o) gs[o] = Gs1[o];
  }
  if (owner) {
    float* __restrict__ pr = part + ((size_t)b * gridDim.x + blockIdx.x) * D::R + opos;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) pr[r * old + c] = acc[r * 6 + c];
  }
}

template <int C>
__global__ __launch_bounds__(kNT) void dense_conv_bw_point_kernel(
    const float* __restrict__ x, int ldx, int N, int k, const float* __restrict__ W0, const float* __restrict__ W1,
    const float* __restrict__ W2, int relu_out, const signed char* __restrict__ arg, const float* __restrict__ out, int ldo,
    const float* __restrict__ gout, int ldg, const float* __restrict__ gy0T, const float* __restrict__ Dsum,
    const float* __restrict__ Gs1w, float* __restrict__ gx, int ldgx, float* __restrict__ part) {
  using D = Bw<C>;
  constexpr int L0 = D::L0, L1 = D::L1, L2 = D::L2, S2 = D::S2;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int pi = blockIdx.x * kNT + tid;
  const bool ok = pi < N;
  const int i = min(pi, N - 1);
  const int nvalid = min(kNT, N - (int)blockIdx.x * kNT);
  const size_t row = (size_t)b * N + i;

  float xi[C], gxr[C], gpass[C], Gy0[kG], Gs1[kG], Gs2[kG], dn[kG];
  const float* __restrict__ gr = gout + row * ldg;
  const float* __restrict__ orow = relu_out ? out + row * ldo : nullptr;
  const signed char* __restrict__ ar = arg + row * (3 * kG);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    xi[c] = x[row * ldx + c];
    gpass[c] = gr[kG + c];                       // the pass-through columns
    if (relu_out) gpass[c] = orow[kG + c] > 0.f ? gpass[c] : 0.f;
  }
#pragma unroll
  for (int o = 0; o < kG; ++o) {
    const float* __restrict__ gy = gy0T + (((size_t)b * kG + o) * N + i) * k;
    float s = 0.f;
    for (int e = 0; e < k; ++e) s += gy[e];      // edges ascending
    Gy0[o] = s;
    Gs1[o] = Gs1w[row * kG + o];
    float g2 = gr[2 * kG + C + o];
    if (relu_out) g2 = orow[2 * kG + C + o] > 0.f ? g2 : 0.f;
    Gs2[o] = ar[2 * kG + o] >= 0 ? g2 : 0.f;
    dn[o] = Dsum[((size_t)b * kG + o) * N + i] - s;   // what arrives over the neighbour path minus what left over the centre's
  }
  // stage [Gy0 | Gs1 | Gs2 | x_i | D - Gy0]
  float* __restrict__ st = smem + tid * S2;
#pragma unroll
  for (int q = 0; q < kG; q += 4) {
    *reinterpret_cast<float4*>(st + q) = make_float4(Gy0[q], Gy0[q + 1], Gy0[q + 2], Gy0[q + 3]);
    *reinterpret_cast<float4*>(st + kG + q) = make_float4(Gs1[q], Gs1[q + 1], Gs1[q + 2], Gs1[q + 3]);
    *reinterpret_cast<float4*>(st + 2 * kG + q) = make_float4(Gs2[q], Gs2[q + 1], Gs2[q + 2], Gs2[q + 3]);
    *reinterpret_cast<float4*>(st + 3 * kG + C + q) = make_float4(dn[q], dn[q + 1], dn[q + 2], dn[q + 3]);
  }
#pragma unroll
  for (int q = 0; q < C; q += 4) *reinterpret_cast<float4*>(st + 3 * kG + q) = make_float4(xi[q], xi[q + 1], xi[q + 2], xi[q + 3]);
  // gx: four products, each a chain of its own from 0 with o ascending (a running sum that started from the pass-through
  // gradient would round every one of the 96 terms at that magnitude), added in the order written, the pass-through columns
  // last.  The weights sit at wave-uniform addresses and arrive through the scalar cache, once per point; the per-point factor
  // of channel o comes back from the lane's own staged row, so that the loops over o stay rolled.
  auto product = [&](const float* __restrict__ W, int ld, int col, int src, bool first) {
    float t[C];
#pragma unroll
    for (int c = 0; c < C; ++c) t[c] = 0.f;
#pragma unroll 1
    for (int o = 0; o < kG; ++o) {
      const float f = st[src + o];
#pragma unroll
      for (int c = 0; c < C; ++c) t[c] = __builtin_fmaf(W[o * ld + col + c], f, t[c]);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) gxr[c] = first ? t[c] : gxr[c] + t[c];
  };
  product(W1, L1, kG, kG, true);                 // W1[:, G:]^T Gs1
  product(W2, L2, kG, 2 * kG, false);            // W2[:, G : G + C]^T Gs2
  product(W0, L0, 0, 0, false);                  // W0[:, :C]^T Gy0
  product(W0, L0, C, 3 * kG + C, false);         // W0[:, C:]^T (D - Gy0)
#pragma unroll
  for (int c = 0; c < C; ++c) gxr[c] += gpass[c];
  if (ok) {
    float* __restrict__ gxo = gx + row * ldgx;
#pragma unroll
    for (int c = 0; c < C; ++c) gxo[c] = gxr[c];
  }
  __syncthreads();

  float* __restrict__ pr = part + ((size_t)b * gridDim.x + blockIdx.x) * D::R;
  if (tid < D::tilesPoint) {
    const int rg = tid % 12, cg = tid / 12;      // rows 6 rg .. 6 rg + 5 of [Gy0; Gs1; Gs2], columns 6 cg .. 6 cg + 5 of x_i
    float acc[36];
#pragma unroll
    for (int q = 0; q < 36; ++q) acc[q] = 0.f;
    const float* __restrict__ sa = smem + 6 * rg;
    const float* __restrict__ sb = smem + 3 * kG + 6 * cg;
#pragma unroll 2
    for (int p = 0; p < nvalid; ++p) {
      float av[6], bv[6];
#pragma unroll
      for (int q = 0; q < 6; q += 2) {
        const float2 u = *reinterpret_cast<const float2*>(sa + p * S2 + q);
        const float2 w = *reinterpret_cast<const float2*>(sb + p * S2 + q);
        av[q] = u.x; av[q + 1] = u.y; bv[q] = w.x; bv[q + 1] = w.y;
      }
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[r * 6 + c] = __builtin_fmaf(av[r], bv[c], acc[r * 6 + c]);
    }
    const int grp = rg / 4, o0 = 6 * (rg % 4);   // 0: gW0[:, :C], 1: gW1[:, 24:], 2: gW2[:, 24 : 24 + C]
    const int ld = grp == 0 ? L0 : grp == 1 ? L1 : L2;
    const int base = grp == 0 ? D::P0 : grp == 1 ? D::P1 + kG : D::P2 + kG;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) pr[base + (o0 + r) * ld + 6 * cg + c] = acc[r * 6 + c];
  }
  if (tid < 3 * kG) {                            // the biases: gb0 = sum Gy0, gb1 = sum Gs1, gb2 = sum Gs2
    float s = 0.f;
    for (int p = 0; p < nvalid; ++p) s += smem[p * S2 + tid];
    pr[D::PB + tid] = s;
  }
}

// element e of the row of partials, summed over the workgroups in ascending order, to where it belongs
__global__ __launch_bounds__(256) void dense_conv_bw_fold_kernel(const float* __restrict__ part, int nwg, int R, int P1, int P2, int PB,
                                                                 float* __restrict__ gW0, float* __restrict__ gW1,
                                                                 float* __restrict__ gW2, float* __restrict__ gb0,
                                                                 float* __restrict__ gb1, float* __restrict__ gb2) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= R) return;
  float v = part[e];
  for (int w = 1; w < nwg; ++w) v += part[(size_t)w * R + e];
  if (e < P1) gW0[e] = v;
  else if (e < P2) gW1[e - P1] = v;
  else if (e < PB) gW2[e - P2] = v;
  else if (e < PB + kG) gb0[e - PB] = v;
  else if (e < PB + 2 * kG) gb1[e - PB - kG] = v;
  else gb2[e - PB - 2 * kG] = v;
}

// the checks houv_dense_conv makes, under the caller's name
bool check_shape(const char* fn, int B, int N, int C, int k, bool edges_fit_int) {
  if (C != 24 && C != 48) {
    set_error("%s: C=%d has no kernel: 24 and 48 are served", fn, C);
    return false;
  }
  if (k < 1 || k > 32) {
    set_error("%s: k=%d neighbours per point: 1..32 are served", fn, k);
    return false;
  }
  if (B < 0 || B > 65535 || N < 1) {
    set_error("%s: bad argument B=%d N=%d (0 <= B <= 65535, N >= 1)", fn, B, N);
    return false;
  }
  if (edges_fit_int && (long long)N * k > 0x7fffffffLL) {    // the backward alone: the ordered scatter indexes the edges with an int
    set_error("%s: bad argument N=%d k=%d (N * k < 2^31)", fn, N, k);
    return false;
  }
  return true;
}

inline long long up4(long long n) { return (n + 3) & ~3LL; }

struct BwLayout {                                // offsets into the workspace in 4-byte elements, each a multiple of 4
  long long gy0T, keys, dsum, gs1, scat, part, total;
  int nwgx, R;
};

BwLayout bw_layout(int B, int N, int C, int k) {
  BwLayout l;
  long long o = 0;
  const long long M = (long long)N * k;
  l.nwgx = (N + kNT - 1) / kNT;
  l.R = C == 24 ? Bw<24>::R : Bw<48>::R;
  l.gy0T = o; o += up4((long long)B * kG * M);
  l.keys = o; o += up4((long long)B * M);
  l.dsum = o; o += up4((long long)B * kG * N);
  l.gs1 = o; o += up4((long long)B * N * kG);
  l.scat = o; o += up4(houv_scatter_points_workspace_bytes(B, N, (int)M) / 4);
  l.part = o; o += up4((long long)B * l.nwgx * l.R);
  l.total = o;
  return l;
}

template <int C>
bool launch_backward(const float* x, int ldx, const int32_t* idx, int B, int N, int k, const float* W0, const float* b0,
                     const float* W1, const float* b1, const float* W2, int relu_out, const int8_t* arg, const float* out, int ldo,
                     const float* gout, int ldg, float* gx, int ldgx, float* gW0, float* gb0, float* gW1, float* gb1, float* gW2,
                     float* gb2, void* workspace, const BwLayout& l, void* stream) {
  using D = Bw<C>;
  const char* fn = "houv_dense_conv_backward";
  hipStream_t st = (hipStream_t)stream;
  float* wf = static_cast<float*>(workspace);
  float *gy0T = wf + l.gy0T, *dsum = wf + l.dsum, *gs1 = wf + l.gs1, *part = wf + l.part;
  int* keys = reinterpret_cast<int*>(wf + l.keys);
  const size_t ldsE = (size_t)D::ldsEdge * 4, ldsP = (size_t)D::ldsPoint * 4;
  hipError_t e = hipFuncSetAttribute((const void*)dense_conv_bw_edge_kernel<C>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsE);
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void*)dense_conv_bw_point_kernel<C>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsP);
  if (e != hipSuccess) {
    set_error("%s: %zu B of LDS: %s", fn, ldsE, hipGetErrorString(e));
    return false;
  }
  const dim3 grid((unsigned)l.nwgx, (unsigned)B);
  dense_conv_bw_edge_kernel<C><<<grid, kNT, ldsE, st>>>(x, ldx, idx, N, k, W0, b0, W1, b1, W2, relu_out,
                                                        reinterpret_cast<const signed char*>(arg), out, ldo, gout, ldg, gy0T, keys,
                                                        gs1, part);
  if (!check_launch(fn)) return false;
  // the neighbour path: gy0 summed per destination, sources in ascending (i, e) order
  if (!houv_scatter_points_grad(gy0T, keys, nullptr, B, kG, N, N * k, 1, dsum, wf + l.scat, stream)) return false;
  dense_conv_bw_point_kernel<C><<<grid, kNT, ldsP, st>>>(x, ldx, N, k, W0, W1, W2, relu_out, reinterpret_cast<const signed char*>(arg),
                                                         out, ldo, gout, ldg, gy0T, dsum, gs1, gx, ldgx, part);
  if (!check_launch(fn)) return false;
  dense_conv_bw_fold_kernel<<<(D::R + 255) / 256, 256, 0, st>>>(part, B * l.nwgx, D::R, D::P1, D::P2, D::PB, gW0, gW1, gW2, gb0, gb1,
                                                                gb2);
  return check_launch(fn);
}

}  // namespace
}  // namespace houv

extern "C" int houv_dense_conv_arg(const float* x, int ldx, const int32_t* idx, int B, int N, int C, int k, const float* W0,
                                   const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                                   int relu_out, float* out, int ldo, int8_t* arg, void* stream) {
  using namespace houv;
  const char* fn = "houv_dense_conv_arg";
  if (!check_shape(fn, B, N, C, k, false)) return 0;
  if (ldx < C || ldo < C + 3 * kG) {
    set_error("%s: bad argument ldx=%d ldo=%d (ldx >= C=%d, ldo >= C + 72 = %d)", fn, ldx, ldo, C, C + 3 * kG);
    return 0;
  }
  if (B == 0) return 1;
  {
    const void* req[] = {x, idx, W0, b0, W1, b1, W2, b2, out, arg};
    const char* names[] = {"x", "idx", "W0", "b0", "W1", "b1", "W2", "b2", "out", "arg"};
    for (int i = 0; i < 10; ++i)
      if (!req[i]) {
        set_error("%s: %s is a null pointer", fn, names[i]);
        return 0;
      }
  }
  if (!houv_dense_conv(x, ldx, idx, B, N, C, k, W0, b0, W1, b1, W2, b2, relu_out, out, ldo, stream)) return 0;
  dim3 grid((N + kNT - 1) / kNT, B);
  hipStream_t s = (hipStream_t)stream;
  signed char* a = reinterpret_cast<signed char*>(arg);
  if (C == 24) dense_conv_arg_kernel<24><<<grid, kNT, 0, s>>>(x, ldx, idx, N, k, W0, b0, W1, b1, W2, b2, a);
  else dense_conv_arg_kernel<48><<<grid, kNT, 0, s>>>(x, ldx, idx, N, k, W0, b0, W1, b1, W2, b2, a);
  return check_launch(fn) ? 1 : 0;
}

extern "C" long long houv_dense_conv_backward_workspace_bytes(int B, int N, int C, int k) {
  using namespace houv;
  if (B <= 0 || N < 1 || (C != 24 && C != 48) || k < 1 || k > 32 || B > 65535 || (long long)N * k > 0x7fffffffLL) return 0;
  return bw_layout(B, N, C, k).total * 4;
}

extern "C" int houv_dense_conv_backward(const float* x, int ldx, const int32_t* idx, int B, int N, int C, int k, const float* W0,
                                        const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                                        int relu_out, const int8_t* arg, const float* out_or_null, int ldo, const float* gout,
                                        int ldg, float* gx, int ldgx, float* gW0, float* gb0, float* gW1, float* gb1, float* gW2,
                                        float* gb2, void* workspace, long long workspace_bytes, void* stream) {
  using namespace houv;
  const char* fn = "houv_dense_conv_backward";
  if (!check_shape(fn, B, N, C, k, true)) return 0;
  if (ldx < C || ldg < C + 3 * kG || ldgx < C || (relu_out && ldo < C + 3 * kG)) {
    set_error("%s: bad argument ldx=%d ldo=%d ldg=%d ldgx=%d (ldx, ldgx >= C=%d; ldg, and ldo when relu_out is set, >= C + 72 = %d)",
              fn, ldx, ldo, ldg, ldgx, C, C + 3 * kG);
    return 0;
  }
  {
    const void* req[] = {gW0, gb0, gW1, gb1, gW2, gb2};
    const char* names[] = {"gW0", "gb0", "gW1", "gb1", "gW2", "gb2"};
    for (int i = 0; i < 6; ++i)
      if (!req[i]) {
        set_error("%s: %s is a null pointer", fn, names[i]);
        return 0;
      }
  }
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {                                  // no cloud: the weight gradients are zero
    const size_t n0 = (size_t)kG * 2 * C, n1 = (size_t)kG * (kG + C), n2 = (size_t)kG * (2 * kG + C);
    if (hipMemsetAsync(gW0, 0, n0 * 4, st) != hipSuccess || hipMemsetAsync(gW1, 0, n1 * 4, st) != hipSuccess ||
        hipMemsetAsync(gW2, 0, n2 * 4, st) != hipSuccess || hipMemsetAsync(gb0, 0, kG * 4, st) != hipSuccess ||
        hipMemsetAsync(gb1, 0, kG * 4, st) != hipSuccess || hipMemsetAsync(gb2, 0, kG * 4, st) != hipSuccess) {
      set_error("%s: hipMemsetAsync failed", fn);
      return 0;
    }
    return 1;
  }
  {
    const void* req[] = {x, idx, W0, b0, W1, b1, W2, b2, arg, gout, gx};
    const char* names[] = {"x", "idx", "W0", "b0", "W1", "b1", "W2", "b2", "arg", "gout", "gx"};
    for (int i = 0; i < 11; ++i)
      if (!req[i]) {
        set_error("%s: %s is a null pointer", fn, names[i]);
        return 0;
      }
    if (relu_out && !out_or_null) {
      set_error("%s: relu_out is set but out is a null pointer", fn);
      return 0;
    }
  }
  const BwLayout l = bw_layout(B, N, C, k);
  if (!workspace || workspace_bytes < l.total * 4 || ((uintptr_t)workspace & 15)) {
    set_error("%s: workspace of %lld bytes at %p, %lld are needed, 16-byte aligned (houv_dense_conv_backward_workspace_bytes)", fn,
              workspace_bytes, workspace, l.total * 4);
    return 0;
  }
  const bool ok = C == 24 ? launch_backward<24>(x, ldx, idx, B, N, k, W0, b0, W1, b1, W2, relu_out, arg, out_or_null, ldo, gout, ldg,
                                                gx, ldgx, gW0, gb0, gW1, gb1, gW2, gb2, workspace, l, stream)
                          : launch_backward<48>(x, ldx, idx, B, N, k, W0, b0, W1, b1, W2, relu_out, arg, out_or_null, ldo, gout, ldg,
                                                gx, ldgx, gW0, gb0, gW1, gb1, gW2, gb2, workspace, l, stream);
  return ok ? 1 : 0;
}
