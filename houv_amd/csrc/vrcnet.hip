// vrcnet.hip -- the device piece of the VRCNet completion network (completion/models/vrcnet.py):
//
//   houv_sa_attn   SA_module.forward (vrcnet.py:49-67) after its three input projections, in one kernel.  get_edge_features is a
//                  pure gather, so conv2(xn) and conv3(xn) are gathers of per-point projections: one houv_gemm_f32 call writes
//                  P = [x1 | x2 | x3] per point, and this kernel does the rest with lane = point: the attention MLP over
//                  cat(x1, x2 of the k neighbours), the k * m weights, the weighted sum of the neighbours' x3, conv_out, the
//                  residual.  The [B, C, k, N] edge tensor, its [B, rel, k, N] and [B, mid, k, N] projections and the
//                  [B, mid, k, N] weight tensor of the reference never exist; only out[B, N, C] is written.
//
// Every weight is read at a wave-uniform LDS address (a broadcast), as in dense_conv_kernel (ecg.hip).  One LDS buffer is
// refilled between the phases: conv_w[1] transposed to [slot][r][o] (slot 0 = the point's own x1, slot j + 1 = neighbour j), in
// chunks of whole slots where it does not fit at once (C = 512, k > 16), then conv_w[3] as it is, then conv_out in chunks of rows.
// Exact fp32 fma chains on the vector ALU: the products are [1 x K] . [K x m] per LANE with m = 2 .. 16, which has no MFMA shape,
// and conv_out per lane keeps the weighted sum in registers instead of sending it through memory to a GEMM.
//
// No atomics, no allocation, no scratch, fixed orders everywhere: results are bit-identical from call to call.
#include "../../include/houv_hip.h"
#include "houv_common.h"

namespace houv {
namespace {

constexpr int kSaNT = HOUV_SA_ATTN_BLOCK;        // points per workgroup: two waves share one LDS copy of the weights
constexpr int kSaMaxK = 32;
constexpr int kSaLdsFloats = 8704;               // the weight buffer's ceiling: 17 slots of conv_w[1] at C = 512 (34 KB)

constexpr int sa_max(int a, int b) { return a > b ? a : b; }

template <int C>
struct SaDims {
  static constexpr int rel = C / 16, mid = C / 4, m = mid / 8;
  static constexpr int slab = rel * m;                                                     // conv_w[1] weights per slot
  static constexpr int SC = (kSaMaxK + 1) * slab <= kSaLdsFloats ? kSaMaxK + 1 : kSaLdsFloats / slab;   // slots per chunk
  static constexpr int RC = C * mid <= 8192 ? C : 8192 / mid;                              // conv_out rows per chunk
  static constexpr int SW = sa_max(sa_max(SC * slab, kSaMaxK * m * m), RC * mid);
  static_assert(C % RC == 0 && RC % 4 == 0 && rel % 4 == 0 && SW <= kSaLdsFloats, "chunking");
};

template <int C>
__global__ __launch_bounds__(kSaNT) void sa_attn_kernel(const float* __restrict__ P, int ldp, const float* x, int ldx,
                                                        const int* __restrict__ idx, int N, int k,
                                                        const float* __restrict__ Ww1, const float* __restrict__ Ww2,
                                                        const float* __restrict__ bw2, const float* __restrict__ Wout,
                                                        const float* __restrict__ bout, int relu_out, float* out, int ldo) {
  using D = SaDims<C>;
  constexpr int rel = D::rel, mid = D::mid, m = D::m, slab = D::slab, SC = D::SC, RC = D::RC;
  __shared__ __attribute__((aligned(16))) float sw[D::SW];
  __shared__ float sb2[kSaMaxK * m];
  __shared__ float sbo[C];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int pi = blockIdx.x * kSaNT + tid;
  const bool ok = pi < N;
  const int i = min(pi, N - 1);                                 // lanes past the cloud repeat its last point; never stored
  const float* __restrict__ Pb = P + (size_t)b * N * ldp;
  const int* __restrict__ nb = idx + ((size_t)b * N + i) * k;
  for (int e = tid; e < k * m; e += kSaNT) sb2[e] = bw2[e];
  for (int e = tid; e < C; e += kSaNT) sbo[e] = bout[e];

  // ---- h = relu(Ww1 . relu(t)),  t = cat(x1[i], x2 of the neighbours, channel-major): slot by slot
  float h[m];
#pragma unroll
  for (int o = 0; o < m; ++o) h[o] = 0.f;
  const int ldw = rel * (k + 1);
  for (int s0 = 0; s0 <= k; s0 += SC) {
    const int ns = min(SC, k + 1 - s0);
    __syncthreads();
    for (int e = tid; e < ns * slab; e += kSaNT) {
      const int s = s0 + e / slab, r = (e % slab) / m, o = e % m;
      sw[e] = Ww1[o * ldw + (s == 0 ? r : rel + r * k + (s - 1))];
    }
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < ns; ++s) {
      const int sg = s0 + s;
      const float* __restrict__ src = sg == 0 ? Pb + (size_t)i * ldp : Pb + (size_t)min(max(nb[sg - 1], 0), N - 1) * ldp + rel;
      float t[rel];
#pragma unroll
      for (int r4 = 0; r4 < rel / 4; ++r4) {
        const float4 v = reinterpret_cast<const float4*>(src)[r4];
        t[4 * r4] = v.x; t[4 * r4 + 1] = v.y; t[4 * r4 + 2] = v.z; t[4 * r4 + 3] = v.w;
      }
      const float* __restrict__ ws = sw + s * slab;
#pragma unroll
      for (int r = 0; r < rel; ++r) {
        const float tr = __builtin_fmaxf(t[r], 0.f);
#pragma unroll
        for (int o = 0; o < m; ++o) h[o] = __builtin_fmaf(ws[r * m + o], tr, h[o]);
      }
    }
  }
#pragma unroll
  for (int o = 0; o < m; ++o) h[o] = __builtin_fmaxf(h[o], 0.f);

  // ---- w[c', j] = Ww2[c' k + j] . h + bw2[c' k + j];  o[c] = sum_j w[c mod m, j] x3[idx[j]][c]
  __syncthreads();
  for (int e = tid; e < k * m * m; e += kSaNT) sw[e] = Ww2[e];
  __syncthreads();
  float o_[mid];
#pragma unroll
  for (int c = 0; c < mid; ++c) o_[c] = 0.f;
#pragma unroll 1
  for (int j = 0; j < k; ++j) {
    float wj[m];
#pragma unroll
    for (int cp = 0; cp < m; ++cp) {
      const float* __restrict__ row = sw + (cp * k + j) * m;
      float a = 0.f;
#pragma unroll
      for (int q = 0; q < m; ++q) a = __builtin_fmaf(row[q], h[q], a);
      wj[cp] = a + sb2[cp * k + j];
    }
    const float4* __restrict__ x3 = reinterpret_cast<const float4*>(Pb + (size_t)min(max(nb[j], 0), N - 1) * ldp + 2 * rel);
#pragma unroll
    for (int c4 = 0; c4 < mid / 4; ++c4) {
      const float4 v = x3[c4];
      o_[4 * c4] = __builtin_fmaf(wj[(4 * c4) % m], v.x, o_[4 * c4]);
      o_[4 * c4 + 1] = __builtin_fmaf(wj[(4 * c4 + 1) % m], v.y, o_[4 * c4 + 1]);
      o_[4 * c4 + 2] = __builtin_fmaf(wj[(4 * c4 + 2) % m], v.z, o_[4 * c4 + 2]);
      o_[4 * c4 + 3] = __builtin_fmaf(wj[(4 * c4 + 3) % m], v.w, o_[4 * c4 + 3]);
    }
  }
#pragma unroll
  for (int c = 0; c < mid; ++c) o_[c] = __builtin_fmaxf(o_[c], 0.f);

  // ---- out = Wout . relu(o) + bout + x, four rows of Wout at a time.  x[i][c] is read by the lane that then writes out[i][c]
  // and by no other, which is what lets `out` be `x` itself.
  const float* xr = x + ((size_t)b * N + i) * ldx;
  float* orow = out + ((size_t)b * N + i) * ldo;
  for (int c0 = 0; c0 < C; c0 += RC) {
    __syncthreads();
    for (int e = tid; e < RC * mid; e += kSaNT) sw[e] = Wout[(size_t)c0 * mid + e];
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < RC; c += 4) {
      float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q4 = 0; q4 < mid / 4; ++q4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 w = *reinterpret_cast<const float4*>(sw + (c + u) * mid + 4 * q4);
          a[u] = __builtin_fmaf(w.x, o_[4 * q4], a[u]);
          a[u] = __builtin_fmaf(w.y, o_[4 * q4 + 1], a[u]);
          a[u] = __builtin_fmaf(w.z, o_[4 * q4 + 2], a[u]);
          a[u] = __builtin_fmaf(w.w, o_[4 * q4 + 3], a[u]);
        }
      }
      if (ok) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float v = (a[u] + sbo[c0 + c + u]) + xr[c0 + c + u];
          orow[c0 + c + u] = relu_out ? __builtin_fmaxf(v, 0.f) : v;
        }
      }
    }
  }
}

}  // namespace
}  // namespace houv

extern "C" int houv_sa_attn(const float* P, int ldp, const float* x, int ldx, const int32_t* idx, int B, int N, int C, int k,
                            const float* Ww1, const float* Ww2, const float* bw2, const float* Wout, const float* bout,
                            int relu_out, float* out, int ldo, void* stream) {
  using namespace houv;
  if (C != 64 && C != 128 && C != 256 && C != 512) {
    set_error("houv_sa_attn: C=%d has no kernel: 64, 128, 256 and 512 are served", C);
    return 0;
  }
  if (k < 1 || k > kSaMaxK) {
    set_error("houv_sa_attn: k=%d neighbours per point: 1..32 are served", k);
    return 0;
  }
  if (N < 1 || N > 16384 || k > N) {
    set_error("houv_sa_attn: N=%d points with k=%d: k <= N <= 16384 is served", N, k);
    return 0;
  }
  if (B < 0 || B > 65535) {
    set_error("houv_sa_attn: B=%d clouds: 0..65535 are served", B);
    return 0;
  }
  const int wp = 2 * (C / 16) + C / 4;
  if (ldp < wp || ldp % 4 != 0) {
    set_error("houv_sa_attn: ldp=%d: a multiple of 4 that is >= 2 rel + mid = %d is served", ldp, wp);
    return 0;
  }
  if (ldx < C) { set_error("houv_sa_attn: ldx=%d is less than C=%d", ldx, C); return 0; }
  if (ldo < C) { set_error("houv_sa_attn: ldo=%d is less than C=%d", ldo, C); return 0; }
  if (B == 0) return 1;
  {
    const void* req[] = {P, x, idx, Ww1, Ww2, bw2, Wout, bout, out};
    const char* names[] = {"P", "x", "idx", "Ww1", "Ww2", "bw2", "Wout", "bout", "out"};
    for (int i = 0; i < 9; ++i)
      if (!req[i]) {
        set_error("houv_sa_attn: %s is a null pointer", names[i]);
        return 0;
      }
  }
  if ((uintptr_t)P % 16 != 0) {
    set_error("houv_sa_attn: P is not aligned to 16 bytes (its rows are read four floats at a time)");
    return 0;
  }
  if (out == x && ldo != ldx) {
    set_error("houv_sa_attn: out is x but ldo=%d differs from ldx=%d: out may be x itself, element for element, and nothing else "
              "of it", ldo, ldx);
    return 0;
  }
  dim3 grid((N + kSaNT - 1) / kSaNT, B);
  hipStream_t s = (hipStream_t)stream;
#define HOUV_SA_LAUNCH(CC) \
  sa_attn_kernel<CC><<<grid, kSaNT, 0, s>>>(P, ldp, x, ldx, idx, N, k, Ww1, Ww2, bw2, Wout, bout, relu_out, out, ldo)
  if (C == 64) HOUV_SA_LAUNCH(64);
  else if (C == 128) HOUV_SA_LAUNCH(128);
  else if (C == 256) HOUV_SA_LAUNCH(256);
  else HOUV_SA_LAUNCH(512);
#undef HOUV_SA_LAUNCH
  return check_launch("houv_sa_attn") ? 1 : 0;
}
