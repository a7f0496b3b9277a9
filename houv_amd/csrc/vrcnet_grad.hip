// vrcnet_grad.hip -- training support for SA_module (houv_sa_attn, vrcnet.hip):
//
//   houv_sa_attn_backward   the backward pass of everything houv_sa_attn computes before conv_out (conv_out's two products over all
//                           points belong on the matrix pipe and stay with the caller, who passes G = gy . Wout, the gradient of
//                           relu(o)).  Five steps, no float atomics, every sum in a fixed order:
//     1. point kernel (lane = point, 128 lanes, the forward's LDS weight scheme): recomputes t, pre, h, w and o by the forward's
//        own chains (the same source, the same flags: every ReLU mask is the forward's bits), writes ro = relu(o), and leaves per
//        point the rows go[mid], w[k m], gw[k m], relu(t)[rel (k+1)], gt[rel (k+1)], (h | gpre)[2 m] and the clamped keys.
//     2. the stable counting sort of houv_scatter_points_grad turns the keys into the CSR inverse of idx.
//     3. scatter kernel (four columns of one destination per lane): gP's x1 columns are the point's own gt; its x2 and x3 columns
//        are sums over the destination's incoming edges in ascending (i, j), the x3 sum an fma chain from 0.
//     4. reduce kernel (lane = one column of the per-point rows): gWw2 = sum gw (x) h, gbw2 = sum gw, gWw1 = sum gpre (x) relu(t)
//        over a fixed chunk of points in ascending order, one row of partials per chunk.
//     5. the chunks' partials are added in chunk order and land at the weights' own index order.
#include "../../include/houv_hip.h"
#include "houv_common.h"

namespace houv {
namespace {

constexpr int kNT = HOUV_SA_ATTN_BLOCK;          // points per workgroup of the point kernel, as in the forward
constexpr int kMaxK = 32;
constexpr int kLdsFloats = 8704;                 // the forward's ceiling: 17 slots of conv_w[1] at C = 512
constexpr int kRedNT = 128;                      // columns per workgroup of the reduce kernel
constexpr int kRedMinChunk = 128;                // points per chunk of the reduction, at least
constexpr int kRedMaxChunks = 1024;

constexpr int bw_max(int a, int b) { return a > b ? a : b; }

template <int C>
struct BwDims {
  static constexpr int rel = C / 16, mid = C / 4, m = mid / 8;
  static constexpr int slab = rel * m;                                                     // conv_w[1] weights per slot
  static constexpr int SC = (kMaxK + 1) * slab <= kLdsFloats ? kMaxK + 1 : kLdsFloats / slab;   // slots per chunk
  static constexpr int SW = bw_max(SC * slab, kMaxK * m * m);
  static constexpr int NQ = (2 * rel + mid) / 4;                                           // four-column pieces of a gP row
  static_assert(rel % 4 == 0 && SW <= kLdsFloats, "chunking");
};

// v[0 .. n) to dst, which is aligned to min(n, 4) floats
template <int n>
__device__ __forceinline__ void store_row(float* __restrict__ dst, const float (&v)[n]) {
  if constexpr (n == 2) {
    *reinterpret_cast<float2*>(dst) = make_float2(v[0], v[1]);
  } else {
#pragma unroll
    for (int q = 0; q < n; q += 4) *reinterpret_cast<float4*>(dst + q) = make_float4(v[q], v[q + 1], v[q + 2], v[q + 3]);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// step 1: everything that belongs to one point
// ------------------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(kNT) void sa_attn_bw_point_kernel(const float* __restrict__ P, int ldp, const int* __restrict__ idx, int N,
                                                               int k, const float* __restrict__ Ww1, const float* __restrict__ Ww2,
                                                               const float* __restrict__ bw2, const float* __restrict__ G, int ldg,
                                                               float* __restrict__ ro, int ldro, float* __restrict__ go_w,
                                                               float* __restrict__ w_w, float* __restrict__ gw_w,
                                                               float* __restrict__ rt_w, float* __restrict__ gt_w,
                                                               float* __restrict__ hg_w, int* __restrict__ keys) {
  using D = BwDims<C>;
  constexpr int rel = D::rel, mid = D::mid, m = D::m, slab = D::slab, SC = D::SC;
  __shared__ __attribute__((aligned(16))) float sw[D::SW];
  __shared__ float sb2[kMaxK * m];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int pi = blockIdx.x * kNT + tid;
  const bool ok = pi < N;
  const int i = min(pi, N - 1);                                 // lanes past the cloud repeat its last point; never stored
  const float* __restrict__ Pb = P + (size_t)b * N * ldp;
  const size_t row = (size_t)b * N + i;
  const int* __restrict__ nb = idx + row * k;
  const int ldt = rel * (k + 1), ldk = k * m;
  for (int e = tid; e < k * m; e += kNT) sb2[e] = bw2[e];

  // ---- h = relu(Ww1 . relu(t)) by the forward's chain, slot by slot; relu(t) leaves as the point's row [slot][r]
  float h[m];
#pragma unroll
  for (int o = 0; o < m; ++o) h[o] = 0.f;
  const int ldw = rel * (k + 1);
  for (int s0 = 0; s0 <= k; s0 += SC) {
    const int ns = min(SC, k + 1 - s0);
    __syncthreads();
    for (int e = tid; e < ns * slab; e += kNT) {
      const int s = s0 + e / slab, r = (e % slab) / m, o = e % m;
      sw[e] = Ww1[o * ldw + (s == 0 ? r : rel + r * k + (s - 1))];
    }
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < ns; ++s) {
      const int sg = s0 + s;
      const float* __restrict__ src = sg == 0 ? Pb + (size_t)i * ldp : Pb + (size_t)min(max(nb[sg - 1], 0), N - 1) * ldp + rel;
      const float* __restrict__ ws = sw + s * slab;
      float* __restrict__ rt = rt_w + row * ldt + sg * rel;
      // four rows of the slot at a time, the loop rolled: unrolled over all of rel = 32 rows the weights of the whole slot are
      // read ahead of the first fma and spill (C = 512).  The chain runs r ascending either way.
#pragma unroll 1
      for (int r4 = 0; r4 < rel / 4; ++r4) {
        const float4 v = reinterpret_cast<const float4*>(src)[r4];
        const float t[4] = {__builtin_fmaxf(v.x, 0.f), __builtin_fmaxf(v.y, 0.f), __builtin_fmaxf(v.z, 0.f), __builtin_fmaxf(v.w, 0.f)};
        if (ok) store_row<4>(rt + 4 * r4, t);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int o = 0; o < m; ++o) h[o] = __builtin_fmaf(ws[(4 * r4 + u) * m + o], t[u], h[o]);
      }
    }
  }
#pragma unroll
  for (int o = 0; o < m; ++o) h[o] = __builtin_fmaxf(h[o], 0.f);

  // ---- w and o by the forward's chains; w leaves as the point's row [j][c'], the clamped lists as the scatter's keys
  __syncthreads();
  for (int e = tid; e < k * m * m; e += kNT) sw[e] = Ww2[e];
  __syncthreads();
  float o_[mid];
#pragma unroll
  for (int c = 0; c < mid; ++c) o_[c] = 0.f;
#pragma unroll 1
  for (int j = 0; j < k; ++j) {
    float wj[m];
#pragma unroll
    for (int cp = 0; cp < m; ++cp) {
      const float* __restrict__ wr = sw + (cp * k + j) * m;
      float a = 0.f;
#pragma unroll
      for (int q = 0; q < m; ++q) a = __builtin_fmaf(wr[q], h[q], a);
      wj[cp] = a + sb2[cp * k + j];
    }
    const int n = min(max(nb[j], 0), N - 1);
    if (ok) {
      store_row<m>(w_w + row * ldk + j * m, wj);
      keys[row * k + j] = n;
    }
    const float4* __restrict__ x3 = reinterpret_cast<const float4*>(Pb + (size_t)n * ldp + 2 * rel);
#pragma unroll
    for (int c4 = 0; c4 < mid / 4; ++c4) {
      const float4 v = x3[c4];
      o_[4 * c4] = __builtin_fmaf(wj[(4 * c4) % m], v.x, o_[4 * c4]);
      o_[4 * c4 + 1] = __builtin_fmaf(wj[(4 * c4 + 1) % m], v.y, o_[4 * c4 + 1]);
      o_[4 * c4 + 2] = __builtin_fmaf(wj[(4 * c4 + 2) % m], v.z, o_[4 * c4 + 2]);
      o_[4 * c4 + 3] = __builtin_fmaf(wj[(4 * c4 + 3) % m], v.w, o_[4 * c4 + 3]);
    }
  }

  // ---- ro = relu(o);  go = G [o > 0] takes o's registers
  {
    const float* __restrict__ gr = G + row * ldg;
    float* __restrict__ rr = ro + row * ldro;
#pragma unroll
    for (int c = 0; c < mid; ++c) {
      const float g = gr[c];
      if (ok) rr[c] = __builtin_fmaxf(o_[c], 0.f);
      o_[c] = o_[c] > 0.f ? g : 0.f;
    }
    if (ok) store_row<mid>(go_w + row * mid, o_);
  }

  // ---- gw[c', j] = sum over c = c' (mod m), ascending, of go[c] x3[n_j][c];  gh = sum over (j, c') of Ww2[c' k + j] gw[c', j]
  float gh[m];
#pragma unroll
  for (int q = 0; q < m; ++q) gh[q] = 0.f;
#pragma unroll 1
  for (int j = 0; j < k; ++j) {
    const int n = min(max(nb[j], 0), N - 1);
    const float4* __restrict__ x3 = reinterpret_cast<const float4*>(Pb + (size_t)n * ldp + 2 * rel);
    float gwj[m];
#pragma unroll
    for (int cp = 0; cp < m; ++cp) gwj[cp] = 0.f;
#pragma unroll
    for (int c4 = 0; c4 < mid / 4; ++c4) {
      const float4 v = x3[c4];
      gwj[(4 * c4) % m] = __builtin_fmaf(o_[4 * c4], v.x, gwj[(4 * c4) % m]);
      gwj[(4 * c4 + 1) % m] = __builtin_fmaf(o_[4 * c4 + 1], v.y, gwj[(4 * c4 + 1) % m]);
      gwj[(4 * c4 + 2) % m] = __builtin_fmaf(o_[4 * c4 + 2], v.z, gwj[(4 * c4 + 2) % m]);
      gwj[(4 * c4 + 3) % m] = __builtin_fmaf(o_[4 * c4 + 3], v.w, gwj[(4 * c4 + 3) % m]);
    }
    if (ok) store_row<m>(gw_w + row * ldk + j * m, gwj);
#pragma unroll
    for (int cp = 0; cp < m; ++cp) {
      const float* __restrict__ wr = sw + (cp * k + j) * m;
#pragma unroll
      for (int q = 0; q < m; ++q) gh[q] = __builtin_fmaf(wr[q], gwj[cp], gh[q]);
    }
  }
  // gpre = gh [pre > 0], and pre > 0 exactly where h = relu(pre) > 0
#pragma unroll
  for (int q = 0; q < m; ++q) gh[q] = h[q] > 0.f ? gh[q] : 0.f;
  if (ok) {
    store_row<m>(hg_w + row * (2 * m), h);
    store_row<m>(hg_w + row * (2 * m) + m, gh);
  }

  // ---- gt[s] = [t[s] > 0] sum_q Ww1[q, s] gpre[q], slot by slot with the weights of the first phase; the point's row [slot][r]
  for (int s0 = 0; s0 <= k; s0 += SC) {
    const int ns = min(SC, k + 1 - s0);
    __syncthreads();
    for (int e = tid; e < ns * slab; e += kNT) {
      const int s = s0 + e / slab, r = (e % slab) / m, o = e % m;
      sw[e] = Ww1[o * ldw + (s == 0 ? r : rel + r * k + (s - 1))];
    }
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < ns; ++s) {
      const int sg = s0 + s;
      const float* __restrict__ src = sg == 0 ? Pb + (size_t)i * ldp : Pb + (size_t)min(max(nb[sg - 1], 0), N - 1) * ldp + rel;
      const float* __restrict__ ws = sw + s * slab;
      float* __restrict__ gt = gt_w + row * ldt + sg * rel;
#pragma unroll 1
      for (int r4 = 0; r4 < rel / 4; ++r4) {     // rolled, as above
        const float4 v = reinterpret_cast<const float4*>(src)[r4];
        const float t[4] = {v.x, v.y, v.z, v.w};
        float g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          float a = 0.f;
#pragma unroll
          for (int o = 0; o < m; ++o) a = __builtin_fmaf(ws[(4 * r4 + u) * m + o], gh[o], a);
          g[u] = t[u] > 0.f ? a : 0.f;
        }
        if (ok) store_row<4>(gt + 4 * r4, g);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// step 3: the neighbour path, summed per destination in ascending (i, j)
// ------------------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void sa_attn_bw_scatter_kernel(const float* __restrict__ go_w, const float* __restrict__ w_w,
                                                                 const float* __restrict__ gt_w, const int* __restrict__ offsets,
                                                                 const int* __restrict__ order, size_t total, int N, int k,
                                                                 float* __restrict__ gP, int ldgp) {
  using D = BwDims<C>;
  constexpr int rel = D::rel, mid = D::mid, m = D::m, NQ = D::NQ;
  const int ldt = rel * (k + 1), ldk = k * m;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t row = e / NQ;                   // b * N + n
    const int q = (int)(e - row * NQ);
    const size_t b = row / N;
    const int n = (int)(row - b * N);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (q < rel / 4) {                           // the point's own x1 columns
      const float4 v = *reinterpret_cast<const float4*>(gt_w + row * ldt + 4 * q);
      a0 = v.x; a1 = v.y; a2 = v.z; a3 = v.w;
    } else {
      const int* __restrict__ off = offsets + b * ((size_t)N + 1);
      const int* __restrict__ ord = order + b * (size_t)N * k;
      const int end = off[n + 1];
      if (q < rel / 2) {                         // x2: gt of the slot the edge fills
        const int r0 = 4 * q - rel;
        for (int jj = off[n]; jj < end; ++jj) {
          const int mth = ord[jj], i = mth / k, j = mth - i * k;
          const float4 v = *reinterpret_cast<const float4*>(gt_w + (b * N + i) * ldt + (j + 1) * rel + r0);
          a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w;
        }
      } else {                                   // x3: go_i[c] w_i[c mod m, j]
        const int c0 = 4 * q - 2 * rel;
        for (int jj = off[n]; jj < end; ++jj) {
          const int mth = ord[jj], i = mth / k, j = mth - i * k;
          const size_t src = b * N + i;
          const float4 g = *reinterpret_cast<const float4*>(go_w + src * mid + c0);
          const float* __restrict__ wr = w_w + src * ldk + j * m;
          float w0, w1, w2, w3;
          if constexpr (m == 2) {
            const float2 w = *reinterpret_cast<const float2*>(wr);
            w0 = w.x; w1 = w.y; w2 = w.x; w3 = w.y;
          } else {
            const float4 w = *reinterpret_cast<const float4*>(wr + c0 % m);
            w0 = w.x; w1 = w.y; w2 = w.z; w3 = w.w;
          }
          a0 = __builtin_fmaf(g.x, w0, a0); a1 = __builtin_fmaf(g.y, w1, a1);
          a2 = __builtin_fmaf(g.z, w2, a2); a3 = __builtin_fmaf(g.w, w3, a3);
        }
      }
    }
    float* __restrict__ dst = gP + row * ldgp + 4 * q;
    dst[0] = a0; dst[1] = a1; dst[2] = a2; dst[3] = a3;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// steps 4 and 5: the three weight gradients
// ------------------------------------------------------------------------------------------------------------------
// One lane owns column e of X[T, ncols] and adds X[p, e] V[p, 0 .. M) over the chunk's points in ascending p (V = the M floats
// at column `voff` of the (h | gpre) rows, a wave-uniform address), and X[p, e] alone when `with_sum`.  The chunk's partials land
// at part[chunk][poff + q ncols + e].
template <int M>
__global__ __launch_bounds__(kRedNT) void sa_attn_bw_reduce_kernel(const float* __restrict__ X, int ncols, const float* __restrict__ hg,
                                                                   int voff, long long T, long long chunk, float* __restrict__ part,
                                                                   int R, int poff, int with_sum) {
  const int e = blockIdx.x * kRedNT + threadIdx.x;
  if (e >= ncols) return;
  const long long p0 = (long long)blockIdx.y * chunk, p1 = min(T, p0 + chunk);
  float acc[M], s = 0.f;
#pragma unroll
  for (int q = 0; q < M; ++q) acc[q] = 0.f;
#pragma unroll 4
  for (long long p = p0; p < p1; ++p) {
    const float x = X[(size_t)p * ncols + e];
    const float* __restrict__ v = hg + (size_t)p * (2 * M) + voff;
#pragma unroll
    for (int q = 0; q < M; ++q) acc[q] = __builtin_fmaf(x, v[q], acc[q]);
    s += x;
  }
  float* __restrict__ pr = part + (size_t)blockIdx.y * R + poff;
#pragma unroll
  for (int q = 0; q < M; ++q) pr[q * ncols + e] = acc[q];
  if (with_sum) pr[M * ncols + e] = s;
}

// element f of the row of partials, summed over the chunks in ascending order, to where it belongs: the rows were written
// [j][c'] and [slot][r], the weights are indexed c' k + j and (x1 | r k + j)
__global__ __launch_bounds__(256) void sa_attn_bw_fold_kernel(const float* __restrict__ part, int nch, int R, int k, int m, int rel,
                                                              float* __restrict__ gWw1, float* __restrict__ gWw2,
                                                              float* __restrict__ gbw2) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= R) return;
  float v = part[f];
  for (int c = 1; c < nch; ++c) v += part[(size_t)c * R + f];
  const int KA = k * m, KB = rel * (k + 1);
  if (f < (m + 1) * KA) {
    const int q = f / KA, e = f - q * KA, j = e / m, cp = e - j * m, dst = cp * k + j;
    if (q < m) gWw2[dst * m + q] = v;
    else gbw2[dst] = v;
  } else {
    const int g = f - (m + 1) * KA, q = g / KB, sp = g - q * KB, slot = sp / rel, r = sp - slot * rel;
    gWw1[q * KB + (slot == 0 ? r : rel + r * k + (slot - 1))] = v;
  }
}

inline long long up4(long long n) { return (n + 3) & ~3LL; }

struct BwLayout {                                // offsets into the workspace in 4-byte elements, each a multiple of 4
  long long go, w, gw, rt, gt, hg, keys, offsets, order, part, total;
  long long T, chunk;
  int nch, R;
};

BwLayout bw_layout(int B, int N, int C, int k) {
  BwLayout l;
  const int rel = C / 16, mid = C / 4, m = mid / 8;
  const long long T = (long long)B * N, M = (long long)N * k;
  l.T = T;
  l.chunk = kRedMinChunk;
  if ((T + l.chunk - 1) / l.chunk > kRedMaxChunks) l.chunk = (T + kRedMaxChunks - 1) / kRedMaxChunks;
  l.nch = (int)((T + l.chunk - 1) / l.chunk);
  l.R = (m + 1) * k * m + m * rel * (k + 1);
  long long o = 0;
  l.go = o; o += up4(T * mid);
  l.w = o; o += up4(T * k * m);
  l.gw = o; o += up4(T * k * m);
  l.rt = o; o += up4(T * rel * (k + 1));
  l.gt = o; o += up4(T * rel * (k + 1));
  l.hg = o; o += up4(T * 2 * m);
  l.keys = o; o += up4(B * M);
  l.offsets = o; o += up4((long long)B * (N + 1));
  l.order = o; o += up4(B * M);
  l.part = o; o += up4((long long)l.nch * l.R);
  l.total = o;
  return l;
}

bool shape_served(int B, int N, int C, int k) {
  return (C == 64 || C == 128 || C == 256 || C == 512) && k >= 1 && k <= kMaxK && N >= 1 && N <= 16384 && k <= N && B >= 0 &&
         B <= 65535 && (long long)N * k <= 0x7fffffffLL;
}

template <int C>
bool launch_backward(const float* P, int ldp, const int32_t* idx, int B, int N, int k, const float* Ww1, const float* Ww2,
                     const float* bw2, const float* G, int ldg, float* gP, int ldgp, float* ro, int ldro, float* gWw1, float* gWw2,
                     float* gbw2, void* workspace, const BwLayout& l, void* stream) {
  using D = BwDims<C>;
  const char* fn = "houv_sa_attn_backward";
  hipStream_t st = (hipStream_t)stream;
  float* wf = static_cast<float*>(workspace);
  float *go = wf + l.go, *w = wf + l.w, *gw = wf + l.gw, *rt = wf + l.rt, *gt = wf + l.gt, *hg = wf + l.hg, *part = wf + l.part;
  int *keys = reinterpret_cast<int*>(wf + l.keys), *offsets = reinterpret_cast<int*>(wf + l.offsets),
      *order = reinterpret_cast<int*>(wf + l.order);
  const dim3 grid((unsigned)((N + kNT - 1) / kNT), (unsigned)B);
  sa_attn_bw_point_kernel<C><<<grid, kNT, 0, st>>>(P, ldp, idx, N, k, Ww1, Ww2, bw2, G, ldg, ro, ldro, go, w, gw, rt, gt, hg, keys);
  if (!check_launch(fn)) return false;
  if (!scatter_index_launch(keys, B, N, N * k, offsets, order, st)) return false;
  const size_t total = (size_t)l.T * D::NQ;
  const size_t blocks = (total + 255) / 256;
  sa_attn_bw_scatter_kernel<C><<<(unsigned)(blocks > 65536 ? 65536 : blocks), 256, 0, st>>>(go, w, gt, offsets, order, total, N, k, gP,
                                                                                          ldgp);
  if (!check_launch(fn)) return false;
  const int KA = k * D::m, KB = D::rel * (k + 1);
  sa_attn_bw_reduce_kernel<D::m><<<dim3((KA + kRedNT - 1) / kRedNT, l.nch), kRedNT, 0, st>>>(gw, KA, hg, 0, l.T, l.chunk, part, l.R, 0, 1);
  if (!check_launch(fn)) return false;
  sa_attn_bw_reduce_kernel<D::m><<<dim3((KB + kRedNT - 1) / kRedNT, l.nch), kRedNT, 0, st>>>(rt, KB, hg, D::m, l.T, l.chunk, part, l.R,
                                                                                           (D::m + 1) * KA, 0);
  if (!check_launch(fn)) return false;
  sa_attn_bw_fold_kernel<<<(l.R + 255) / 256, 256, 0, st>>>(part, l.nch, l.R, k, D::m, D::rel, gWw1, gWw2, gbw2);
  return check_launch(fn);
}

}  // namespace
}  // namespace houv

extern "C" long long houv_sa_attn_backward_workspace_bytes(int B, int N, int C, int k) {
  using namespace houv;
  if (B <= 0 || !shape_served(B, N, C, k)) return 0;
  return bw_layout(B, N, C, k).total * 4;
}

extern "C" int houv_sa_attn_backward(const float* P, int ldp, const int32_t* idx, int B, int N, int C, int k, const float* Ww1,
                                     const float* Ww2, const float* bw2, const float* G, int ldg, float* gP, int ldgp, float* ro,
                                     int ldro, float* gWw1, float* gWw2, float* gbw2, void* workspace, long long workspace_bytes,
                                     void* stream) {
  using namespace houv;
  const char* fn = "houv_sa_attn_backward";
  if (C != 64 && C != 128 && C != 256 && C != 512) {
    set_error("%s: C=%d has no kernel: 64, 128, 256 and 512 are served", fn, C);
    return 0;
  }
  if (k < 1 || k > kMaxK) {
    set_error("%s: k=%d neighbours per point: 1..32 are served", fn, k);
    return 0;
  }
  if (N < 1 || N > 16384 || k > N) {
    set_error("%s: N=%d points with k=%d: k <= N <= 16384 is served", fn, N, k);
    return 0;
  }
  if (B < 0 || B > 65535) {
    set_error("%s: B=%d clouds: 0..65535 are served", fn, B);
    return 0;
  }
  if (!shape_served(B, N, C, k)) {
    set_error("%s: N=%d k=%d: N * k < 2^31 is served", fn, N, k);
    return 0;
  }
  const int rel = C / 16, mid = C / 4, m = mid / 8, wp = 2 * rel + mid;
  if (ldp < wp || ldp % 4 != 0) {
    set_error("%s: ldp=%d: a multiple of 4 that is >= 2 rel + mid = %d is served", fn, ldp, wp);
    return 0;
  }
  if (ldg < mid) { set_error("%s: ldg=%d is less than mid=%d", fn, ldg, mid); return 0; }
  if (ldgp < wp) { set_error("%s: ldgp=%d is less than 2 rel + mid = %d", fn, ldgp, wp); return 0; }
  if (ldro < mid) { set_error("%s: ldro=%d is less than mid=%d", fn, ldro, mid); return 0; }
  {
    const void* req[] = {gWw1, gWw2, gbw2};
    const char* names[] = {"gWw1", "gWw2", "gbw2"};
    for (int i = 0; i < 3; ++i)
      if (!req[i]) {
        set_error("%s: %s is a null pointer", fn, names[i]);
        return 0;
      }
  }
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {                                  // no cloud: the weight gradients are zero
    if (hipMemsetAsync(gWw1, 0, (size_t)m * rel * (k + 1) * 4, st) != hipSuccess ||
        hipMemsetAsync(gWw2, 0, (size_t)k * m * m * 4, st) != hipSuccess || hipMemsetAsync(gbw2, 0, (size_t)k * m * 4, st) != hipSuccess) {
      set_error("%s: hipMemsetAsync failed", fn);
      return 0;
    }
    return 1;
  }
  {
    const void* req[] = {P, idx, Ww1, Ww2, bw2, G, gP, ro};
    const char* names[] = {"P", "idx", "Ww1", "Ww2", "bw2", "G", "gP", "ro"};
    for (int i = 0; i < 8; ++i)
      if (!req[i]) {
        set_error("%s: %s is a null pointer", fn, names[i]);
        return 0;
      }
  }
  if ((uintptr_t)P % 16 != 0) {
    set_error("%s: P is not aligned to 16 bytes (its rows are read four floats at a time)", fn);
    return 0;
  }
  const BwLayout l = bw_layout(B, N, C, k);
  if (!workspace || workspace_bytes < l.total * 4 || ((uintptr_t)workspace & 15)) {
    set_error("%s: workspace of %lld bytes at %p, %lld are needed, 16-byte aligned (houv_sa_attn_backward_workspace_bytes)", fn,
              workspace_bytes, workspace, l.total * 4);
    return 0;
  }
  bool ok;
#define HOUV_SA_BW_LAUNCH(CC) \
  ok = launch_backward<CC>(P, ldp, idx, B, N, k, Ww1, Ww2, bw2, G, ldg, gP, ldgp, ro, ldro, gWw1, gWw2, gbw2, workspace, l, stream)
  if (C == 64) HOUV_SA_BW_LAUNCH(64);
  else if (C == 128) HOUV_SA_BW_LAUNCH(128);
  else if (C == 256) HOUV_SA_BW_LAUNCH(256);
  else HOUV_SA_BW_LAUNCH(512);
#undef HOUV_SA_BW_LAUNCH
  return ok ? 1 : 0;
}
