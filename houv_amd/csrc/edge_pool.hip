// edge_pool.hip -- edge_preserve_sampling's feature half (model_utils.py:90-116) as one gather, and its backward (DESIGN.md
// section 9.15):
//
//   houv_edge_pool            out[b,s,0:C] = feat[b, p_idx[b,s]],  out[b,s,C+c] = max_j feat[b, pn_idx[b,s,j], c], with the slot of
//                             each maximum when the caller asks for it.  The [B,S,pk,C] gather is never built.
//   houv_edge_pool_backward   gfeat[b,n] = the sum, in ascending (s, slot) with the centre as slot 0, of what the forward sent to
//                             row n.  Three steps, no float atomics: a key array [B][S][pk+1] of clamped rows (slot 0 the centre),
//                             the stable counting sort of houv_scatter_points_grad (its CSR inverse), and one gather per row.
//
// Both kernels are gathers bound by memory traffic: one lane owns four consecutive channels of one sample (forward) or of one
// source row (backward), so the lanes of a row read one coalesced run of float4s (sa_attn_bw_scatter_kernel's layout).  VEC is
// that layout with 16-byte accesses; the scalar form serves any C, leading dimension and address with the same arithmetic.
#include "../../include/houv_hip.h"
#include "houv_common.h"

namespace houv {
namespace {

constexpr int kPoolNT = 256;
constexpr int kPoolMaxC = 1024;
constexpr int kPoolMaxK = 32;
constexpr int kPoolMaxN = 16384;
constexpr unsigned kPoolMaxBlocks = 65536;

// channels c0 .. c0+3 of a row; the scalar form leaves the channels past C at 0 and never touches them
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* __restrict__ row, int c0, int C) {
  if constexpr (VEC) {
    return *reinterpret_cast<const float4*>(row + c0);
  } else {
    float4 v;
    v.x = row[c0];
    v.y = c0 + 1 < C ? row[c0 + 1] : 0.f;
    v.z = c0 + 2 < C ? row[c0 + 2] : 0.f;
    v.w = c0 + 3 < C ? row[c0 + 3] : 0.f;
    return v;
  }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ row, int c0, int C, float4 v) {
  if constexpr (VEC) {
    *reinterpret_cast<float4*>(row + c0) = v;
  } else {
    row[c0] = v.x;
    if (c0 + 1 < C) row[c0 + 1] = v.y;
    if (c0 + 2 < C) row[c0 + 2] = v.z;
    if (c0 + 3 < C) row[c0 + 3] = v.w;
  }
}

// the running best of one column: a NaN never enters, a later slot enters only when strictly greater (-0 == +0: the earlier stays)
__device__ __forceinline__ void take(float v, int j, float& best, int& arg) {
  if (v == v && (arg < 0 || v > best)) {
    best = v;
    arg = j;
  }
}

template <bool VEC>
__global__ __launch_bounds__(kPoolNT) void edge_pool_kernel(const float* __restrict__ feat, int ldx, const int* __restrict__ p_idx,
                                                            const int* __restrict__ pn_idx, size_t total, int N, int S, int C, int pk,
                                                            float* __restrict__ out, int ldo, signed char* __restrict__ arg) {
  const int Q = (C + 3) >> 2;
  for (size_t e = (size_t)blockIdx.x * kPoolNT + threadIdx.x; e < total; e += (size_t)gridDim.x * kPoolNT) {
    const size_t row = e / Q;                    // b * S + s
    const int c0 = 4 * (int)(e - row * Q);
    const size_t b = row / S;
    const float* __restrict__ fb = feat + b * (size_t)N * ldx;
    const int* __restrict__ nb = pn_idx + row * pk;
    float* __restrict__ dst = out + row * ldo;
    store4<VEC>(dst, c0, C, load4<VEC>(fb + (size_t)min(max(p_idx[row], 0), N - 1) * ldx, c0, C));
    float4 best = make_float4(0.f, 0.f, 0.f, 0.f);
    int a0 = -1, a1 = -1, a2 = -1, a3 = -1;
    int j = 0;
    for (; j + 4 <= pk; j += 4) {                // the four rows are fetched ahead of the compares, which run j ascending
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = load4<VEC>(fb + (size_t)min(max(nb[j + u], 0), N - 1) * ldx, c0, C);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        take(v[u].x, j + u, best.x, a0); take(v[u].y, j + u, best.y, a1);
        take(v[u].z, j + u, best.z, a2); take(v[u].w, j + u, best.w, a3);
      }
    }
    for (; j < pk; ++j) {
      const float4 v = load4<VEC>(fb + (size_t)min(max(nb[j], 0), N - 1) * ldx, c0, C);
      take(v.x, j, best.x, a0); take(v.y, j, best.y, a1);
      take(v.z, j, best.z, a2); take(v.w, j, best.w, a3);
    }
    const float nan = __builtin_nanf("");
    best.x = a0 < 0 ? nan : best.x; best.y = a1 < 0 ? nan : best.y;
    best.z = a2 < 0 ? nan : best.z; best.w = a3 < 0 ? nan : best.w;
    store4<VEC>(dst + C, c0, C, best);
    if (arg) {
      signed char* __restrict__ ar = arg + row * C + c0;
      if constexpr (VEC) {
        *reinterpret_cast<char4*>(ar) = make_char4((signed char)a0, (signed char)a1, (signed char)a2, (signed char)a3);
      } else {
        ar[0] = (signed char)a0;
        if (c0 + 1 < C) ar[1] = (signed char)a1;
        if (c0 + 2 < C) ar[2] = (signed char)a2;
        if (c0 + 3 < C) ar[3] = (signed char)a3;
      }
    }
  }
}

// keys[b][s][0] = the clamped centre, keys[b][s][1 + j] = the clamped neighbour j: ascending position = the backward's order
__global__ __launch_bounds__(kPoolNT) void edge_pool_keys_kernel(const int* __restrict__ p_idx, const int* __restrict__ pn_idx,
                                                                 size_t total, int N, int pk, int* __restrict__ keys) {
  const int P = pk + 1;
  for (size_t e = (size_t)blockIdx.x * kPoolNT + threadIdx.x; e < total; e += (size_t)gridDim.x * kPoolNT) {
    const size_t row = e / P;
    const int slot = (int)(e - row * P);
    keys[e] = min(max(slot == 0 ? p_idx[row] : pn_idx[row * pk + slot - 1], 0), N - 1);
  }
}

// One entry of a row's list: the four gradients it brings, -0 where it brings none (x + -0 is x for every x, so an entry that
// does not land leaves the running sum's bits alone), and in `hit` a bit per channel that it landed on.
template <bool VEC>
__device__ __forceinline__ float4 pool_term(const float* __restrict__ gb, int ldg, const signed char* __restrict__ argb, int m, int P,
                                            int c0, int C, int& hit) {
  const int s = m / P, slot = m - s * P;
  const float4 none = make_float4(-0.f, -0.f, -0.f, -0.f);
  const float* __restrict__ gr = gb + (size_t)s * ldg;
  if (slot == 0) {
    hit = 15;
    return load4<VEC>(gr, c0, C);
  }
  const signed char* __restrict__ ar = argb + (size_t)s * C + c0;
  int a0, a1 = -1, a2 = -1, a3 = -1;
  if constexpr (VEC) {
    const char4 a = *reinterpret_cast<const char4*>(ar);
    a0 = a.x; a1 = a.y; a2 = a.z; a3 = a.w;
  } else {
    a0 = ar[0];
    if (c0 + 1 < C) a1 = ar[1];
    if (c0 + 2 < C) a2 = ar[2];
    if (c0 + 3 < C) a3 = ar[3];
  }
  const int j = slot - 1;
  hit = (a0 == j ? 1 : 0) | (a1 == j ? 2 : 0) | (a2 == j ? 4 : 0) | (a3 == j ? 8 : 0);
  if (!hit) return none;                         // most entries of most lanes: the gradient row is not fetched
  const float4 g = load4<VEC>(gr + C, c0, C);
  return make_float4(hit & 1 ? g.x : -0.f, hit & 2 ? g.y : -0.f, hit & 4 ? g.z : -0.f, hit & 8 ? g.w : -0.f);
}

template <bool VEC>
__global__ __launch_bounds__(kPoolNT) void edge_pool_bw_kernel(const float* __restrict__ g, int ldg, const signed char* __restrict__ arg,
                                                               const int* __restrict__ offsets, const int* __restrict__ order,
                                                               size_t total, int N, int S, int C, int pk, float* __restrict__ gfeat,
                                                               int ldgx) {
  const int Q = (C + 3) >> 2, P = pk + 1;
  for (size_t e = (size_t)blockIdx.x * kPoolNT + threadIdx.x; e < total; e += (size_t)gridDim.x * kPoolNT) {
    const size_t row = e / Q;                    // b * N + n
    const int c0 = 4 * (int)(e - row * Q);
    const size_t b = row / N;
    const int n = (int)(row - b * N);
    const int* __restrict__ off = offsets + b * ((size_t)N + 1);
    const int* __restrict__ ord = order + b * (size_t)S * P;
    const float* __restrict__ gb = g + b * (size_t)S * ldg;
    const signed char* __restrict__ argb = arg + b * (size_t)S * C;
    float4 acc = make_float4(-0.f, -0.f, -0.f, -0.f);
    int landed = 0;
    int jj = off[n];
    const int end = off[n + 1];
    for (; jj + 2 <= end; jj += 2) {             // two entries fetched ahead of the adds, which run in list order
      int h0, h1;
      const float4 t0 = pool_term<VEC>(gb, ldg, argb, ord[jj], P, c0, C, h0);
      const float4 t1 = pool_term<VEC>(gb, ldg, argb, ord[jj + 1], P, c0, C, h1);
      acc.x += t0.x; acc.y += t0.y; acc.z += t0.z; acc.w += t0.w;
      acc.x += t1.x; acc.y += t1.y; acc.z += t1.z; acc.w += t1.w;
      landed |= h0 | h1;
    }
    if (jj < end) {
      int h0;
      const float4 t0 = pool_term<VEC>(gb, ldg, argb, ord[jj], P, c0, C, h0);
      acc.x += t0.x; acc.y += t0.y; acc.z += t0.z; acc.w += t0.w;
      landed |= h0;
    }
    // a channel nothing landed on is +0; one that terms landed on keeps its sum's bits, a -0 of -0 terms included
    acc.x = landed & 1 ? acc.x : 0.f; acc.y = landed & 2 ? acc.y : 0.f;
    acc.z = landed & 4 ? acc.z : 0.f; acc.w = landed & 8 ? acc.w : 0.f;
    store4<VEC>(gfeat + row * ldgx, c0, C, acc);
  }
}

inline long long up4(long long n) { return (n + 3) & ~3LL; }

unsigned pool_grid(size_t total) {
  const size_t blocks = (total + kPoolNT - 1) / kPoolNT;
  return (unsigned)(blocks > kPoolMaxBlocks ? kPoolMaxBlocks : blocks);
}

// the shape checks both entry points share; false with the error set
bool pool_shape_ok(const char* fn, int B, int N, int S, int C, int pk) {
  if (C < 1 || C > kPoolMaxC) { set_error("%s: C=%d channels: 1..%d are served", fn, C, kPoolMaxC); return false; }
  if (pk < 1 || pk > kPoolMaxK) { set_error("%s: pk=%d neighbours per sample: 1..%d are served", fn, pk, kPoolMaxK); return false; }
  if (N < 1 || N > kPoolMaxN) { set_error("%s: N=%d points: 1..%d are served", fn, N, kPoolMaxN); return false; }
  if (S < 1) { set_error("%s: S=%d samples: S >= 1 is served", fn, S); return false; }
  if ((long long)S * (pk + 1) > 0x7fffffffLL) { set_error("%s: S=%d pk=%d: S * (pk + 1) < 2^31 is served", fn, S, pk); return false; }
  if (B < 0) { set_error("%s: B=%d clouds: B >= 0 is served", fn, B); return false; }
  return true;
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace
}  // namespace houv

extern "C" int houv_edge_pool(const float* feat, int ldx, const int32_t* p_idx, const int32_t* pn_idx, int B, int N, int S, int C,
                              int pk, float* out, int ldo, int8_t* arg_or_null, void* stream) {
  using namespace houv;
  const char* fn = "houv_edge_pool";
  if (!pool_shape_ok(fn, B, N, S, C, pk)) return 0;
  if (ldx < C) { set_error("%s: ldx=%d is less than C=%d", fn, ldx, C); return 0; }
  if (ldo < 2 * C) { set_error("%s: ldo=%d is less than 2 C = %d", fn, ldo, 2 * C); return 0; }
  if (B == 0) return 1;
  {
    const void* req[] = {feat, p_idx, pn_idx, out};
    const char* names[] = {"feat", "p_idx", "pn_idx", "out"};
    for (int i = 0; i < 4; ++i)
      if (!req[i]) {
        set_error("%s: %s is a null pointer", fn, names[i]);
        return 0;
      }
  }
  const size_t total = (size_t)B * S * ((C + 3) / 4);
  const bool vec = C % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && aligned(feat, 16) && aligned(out, 16) && aligned(arg_or_null, 4);
  signed char* arg = reinterpret_cast<signed char*>(arg_or_null);
  if (vec) edge_pool_kernel<true><<<pool_grid(total), kPoolNT, 0, (hipStream_t)stream>>>(feat, ldx, p_idx, pn_idx, total, N, S, C, pk, out, ldo, arg);
  else edge_pool_kernel<false><<<pool_grid(total), kPoolNT, 0, (hipStream_t)stream>>>(feat, ldx, p_idx, pn_idx, total, N, S, C, pk, out, ldo, arg);
  return check_launch(fn) ? 1 : 0;
}

extern "C" long long houv_edge_pool_backward_workspace_bytes(int B, int N, int S, int pk) {
  using namespace houv;
  if (B <= 0 || N < 1 || N > kPoolMaxN || S < 1 || pk < 1 || pk > kPoolMaxK || (long long)S * (pk + 1) > 0x7fffffffLL) return 0;
  const long long M = (long long)B * S * (pk + 1);           // keys[B][S][pk+1], offsets[B][N+1], order[B][S][pk+1]
  return 4 * (2 * up4(M) + up4((long long)B * (N + 1)));
}

extern "C" int houv_edge_pool_backward(const float* g, int ldg, const int32_t* p_idx, const int32_t* pn_idx, const int8_t* arg, int B,
                                       int N, int S, int C, int pk, float* gfeat, int ldgx, void* workspace, long long workspace_bytes,
                                       void* stream) {
  using namespace houv;
  const char* fn = "houv_edge_pool_backward";
  if (!pool_shape_ok(fn, B, N, S, C, pk)) return 0;
  if (ldg < 2 * C) { set_error("%s: ldg=%d is less than 2 C = %d", fn, ldg, 2 * C); return 0; }
  if (ldgx < C) { set_error("%s: ldgx=%d is less than C=%d", fn, ldgx, C); return 0; }
  if (B == 0) return 1;
  {
    const void* req[] = {g, p_idx, pn_idx, arg, gfeat};
    const char* names[] = {"g", "p_idx", "pn_idx", "arg", "gfeat"};
    for (int i = 0; i < 5; ++i)
      if (!req[i]) {
        set_error("%s: %s is a null pointer", fn, names[i]);
        return 0;
      }
  }
  const long long need = houv_edge_pool_backward_workspace_bytes(B, N, S, pk);
  if (!workspace || workspace_bytes < need || !aligned(workspace, 16)) {
    set_error("%s: workspace of %lld bytes at %p, %lld are needed, 16-byte aligned (houv_edge_pool_backward_workspace_bytes)", fn,
              workspace_bytes, workspace, need);
    return 0;
  }
  hipStream_t st = (hipStream_t)stream;
  const int P = pk + 1;
  const long long M = (long long)B * S * P;
  int* keys = static_cast<int*>(workspace);
  int* offsets = keys + up4(M);
  int* order = offsets + up4((long long)B * (N + 1));
  edge_pool_keys_kernel<<<pool_grid((size_t)M), kPoolNT, 0, st>>>(p_idx, pn_idx, (size_t)M, N, pk, keys);
  if (!check_launch(fn)) return 0;
  if (!scatter_index_launch(keys, B, N, S * P, offsets, order, st)) return 0;
  const size_t total = (size_t)B * N * ((C + 3) / 4);
  const signed char* a = reinterpret_cast<const signed char*>(arg);
  const bool vec = C % 4 == 0 && ldg % 4 == 0 && ldgx % 4 == 0 && aligned(g, 16) && aligned(gfeat, 16) && aligned(arg, 4);
  if (vec) edge_pool_bw_kernel<true><<<pool_grid(total), kPoolNT, 0, st>>>(g, ldg, a, offsets, order, total, N, S, C, pk, gfeat, ldgx);
  else edge_pool_bw_kernel<false><<<pool_grid(total), kPoolNT, 0, st>>>(g, ldg, a, offsets, order, total, N, S, C, pk, gfeat, ldgx);
  return check_launch(fn) ? 1 : 0;
}
