// cd_loss.hip -- the gradient of the completion Chamfer loss with respect to the output cloud, as ordered sums (DESIGN.md
// section 9.17).  The loss is calc_cd(output, gt): with (dist1, dist2, idx1, idx2) = houv_chamfer_forward(gt, output),
//   cd_p = (mean sqrt(dist1) + mean sqrt(dist2)) / 2,   cd_t = mean dist1 + mean dist2        per cloud,
// and with the upstream gradients g_p[B], g_t[B] of the two, row j of cloud b receives
//   gout[j] = 2 w2[j] (out[j] - gt[idx2[j]])  +  the sum over i with idx1[i] == j, i ascending, of  2 w1[i] (out[j] - gt[i])
//   w1[i] = g_t / N + (g_p / (4 N)) / sqrt(dist1[i]),        w2[j] = g_t / M + (g_p / (4 M)) / sqrt(dist2[j]).
//
//   houv_cd_loss_backward   two launches: the stable counting sort of houv_scatter_points_grad over idx1 as it stands (its CSR
//                           inverse: offsets[B][M+1], order[B][N]), then cd_loss_bw_kernel, one lane per output row, which WRITES
//                           gout.  No float atomics, no zeroed buffer, no [B,N] / [B,M] tensor of distance gradients: the square
//                           root's and the mean's backward are the two weights above, computed where they are used.
//
// The order of a row's sum depends on its list alone.  A list of up to kCdLong = 32 entries is added by the row's lane, one
// entry after the other onto the own term.  A longer list is added by the row's whole wave: lane l adds entries l, l + 64,
// l + 128, ... of the list in that order onto -0 (x + -0 is x for every x), the 64 partial sums are added by the xor butterfly
// 32, 16, 8, 4, 2, 1 (a + b is b + a bit for bit, so every lane ends with the same value), and that sum is added to the own
// term.  Split and tree are functions of the list's length; the launch shape and the arrival of lanes decide nothing.
//
// A zero distance is NOT clamped: (g_p / (4 N)) / sqrt(0) is inf (NaN when g_p is 0), and inf times the zero difference of the
// coincident pair is NaN -- what the composition sqrt -> mean -> backward gives at the same rows.
//
// Bound by gathers, not by arithmetic.  Per cloud the kernel reads out (12 M bytes), dist2 and idx2 (8 M), offsets (4 M + 4),
// order (4 N), dist1 (4 N, gathered) and gt (12 N gathered for the lists, up to 12 M for the own terms) and writes gout (12 M):
// 36 M + 20 N + 4 bytes and at most 12 M more; the sort before it reads idx1 (8 N per pass of 8192 rows) and writes offsets
// and order.  A row's lanes run along j, so out, dist2, idx2, offsets and gout are contiguous runs per wave; order is read in
// list order (contiguous per lane, and contiguous per wave on the long path); the 12-byte rows of gt and the 4-byte dist1 are
// gathers into one cloud's 16 N bytes, which stay in cache while the cloud's workgroups run.
#include "../../include/houv_hip.h"
#include "houv_common.h"

namespace houv {
namespace {

constexpr int kCdNT = 256;
constexpr int kCdLong = 32;                // a list longer than this is summed by the row's wave
constexpr unsigned kCdMaxBlocks = 65536;

__device__ __forceinline__ float3 load3(const float* __restrict__ p) { return make_float3(p[0], p[1], p[2]); }

// 2 w (o - g) with w = a_t + a_p / sqrt(d): the one expression tree both kinds of term share
__device__ __forceinline__ float3 cd_term(float3 o, float3 g, float d, float a_t, float a_p) {
  const float s = 2.f * (a_t + a_p / __builtin_sqrtf(d));
  return make_float3(s * (o.x - g.x), s * (o.y - g.y), s * (o.z - g.z));
}

// entry jj of a list: ground-truth point i = ord[jj] against the output row o
__device__ __forceinline__ float3 cd_list_term(const float* __restrict__ gtb, const float* __restrict__ d1b,
                                               const int* __restrict__ ord, int jj, int N, float3 o, float a_t, float a_p) {
  const int i = min(max(ord[jj], 0), N - 1);
  return cd_term(o, load3(gtb + 3 * (size_t)i), d1b[i], a_t, a_p);
}

__device__ __forceinline__ void add3(float3& a, float3 t) {
  a.x = a.x + t.x; a.y = a.y + t.y; a.z = a.z + t.z;
}

__global__ __launch_bounds__(kCdNT) void cd_loss_bw_kernel(const float* __restrict__ out, const float* __restrict__ gt,
                                                           const float* __restrict__ dist1, const float* __restrict__ dist2,
                                                           const int* __restrict__ idx2, const float* __restrict__ g_p,
                                                           const float* __restrict__ g_t, const int* __restrict__ offsets,
                                                           const int* __restrict__ order, size_t tiles, int chunks, int N, int M,
                                                           float* __restrict__ gout) {
  const int lane = threadIdx.x & 63;
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {       // a tile: kCdNT consecutive rows of one cloud
    const size_t b = t / chunks;
    const int j = (int)(t - b * chunks) * kCdNT + (int)threadIdx.x;
    const bool active = j < M;
    const float* __restrict__ gtb = gt + b * (size_t)N * 3;
    const float* __restrict__ d1b = dist1 + b * (size_t)N;
    const int* __restrict__ ord = order + b * (size_t)N;
    const float gp = g_p[b], gtt = g_t[b];
    const float a_t1 = gtt / (float)N, a_p1 = gp / (4.f * (float)N);
    float3 o = make_float3(0.f, 0.f, 0.f), acc = o;
    int beg = 0, end = 0;
    if (active) {
      const size_t row = b * (size_t)M + j;
      o = load3(out + 3 * row);
      const int i2 = min(max(idx2[row], 0), N - 1);
      acc = cd_term(o, load3(gtb + 3 * (size_t)i2), dist2[row], gtt / (float)M, gp / (4.f * (float)M));
      const int* __restrict__ off = offsets + b * ((size_t)M + 1);
      beg = min(max(off[j], 0), N);
      end = min(max(off[j + 1], beg), N);
      if (end - beg <= kCdLong) {
        int jj = beg;
        for (; jj + 4 <= end; jj += 4) {         // four entries fetched ahead of the adds, which run in list order
          float3 v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = cd_list_term(gtb, d1b, ord, jj + u, N, o, a_t1, a_p1);
#pragma unroll
          for (int u = 0; u < 4; ++u) add3(acc, v[u]);
        }
        for (; jj < end; ++jj) add3(acc, cd_list_term(gtb, d1b, ord, jj, N, o, a_t1, a_p1));
      }
    }
    // the long lists of this wave's 64 rows, one after the other, each by the whole wave
    unsigned long long pend = __ballot(active && end - beg > kCdLong);
    while (pend) {
      const int l = __builtin_ctzll(pend);
      pend &= pend - 1;
      const int lb = __shfl(beg, l, kWave), le = __shfl(end, l, kWave);
      const float3 ol = make_float3(__shfl(o.x, l, kWave), __shfl(o.y, l, kWave), __shfl(o.z, l, kWave));
      float3 part = make_float3(-0.f, -0.f, -0.f);
      for (int jj = lb + lane; jj < le; jj += kWave) add3(part, cd_list_term(gtb, d1b, ord, jj, N, ol, a_t1, a_p1));
      part.x = wave_sum(part.x); part.y = wave_sum(part.y); part.z = wave_sum(part.z);
      if (lane == l) add3(acc, part);
    }
    if (active) {
      float* __restrict__ dst = gout + 3 * (b * (size_t)M + j);
      dst[0] = acc.x; dst[1] = acc.y; dst[2] = acc.z;
    }
  }
}

inline long long up4(long long n) { return (n + 3) & ~3LL; }

}  // namespace
}  // namespace houv

extern "C" long long houv_cd_loss_backward_workspace_bytes(int B, int N, int M) {
  using namespace houv;
  if (B <= 0 || N <= 0 || M <= 0) return 0;
  return 4 * (up4((long long)B * ((long long)M + 1)) + up4((long long)B * N));       // offsets[B][M+1], order[B][N]
}

extern "C" int houv_cd_loss_backward(const float* output, const float* gt, const float* dist1, const float* dist2,
                                     const int32_t* idx1, const int32_t* idx2, const float* g_p, const float* g_t, int B, int N, int M,
                                     float* gout, void* workspace, long long workspace_bytes, void* stream) {
  using namespace houv;
  const char* fn = "houv_cd_loss_backward";
  if (N <= 0) { set_error("%s: N=%d ground-truth points: N >= 1 is served", fn, N); return 0; }
  if (M <= 0) { set_error("%s: M=%d output points: M >= 1 is served", fn, M); return 0; }
  if (B < 0) { set_error("%s: B=%d clouds: B >= 0 is served", fn, B); return 0; }
  if (B == 0) return 1;
  {
    const void* req[] = {output, gt, dist1, dist2, idx1, idx2, g_p, g_t, gout};
    const char* names[] = {"output", "gt", "dist1", "dist2", "idx1", "idx2", "g_p", "g_t", "gout"};
    for (int i = 0; i < 9; ++i)
      if (!req[i]) {
        set_error("%s: %s is a null pointer", fn, names[i]);
        return 0;
      }
  }
  const long long need = houv_cd_loss_backward_workspace_bytes(B, N, M);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) != 0) {
    set_error("%s: workspace of %lld bytes at %p, %lld are needed, 16-byte aligned (houv_cd_loss_backward_workspace_bytes)", fn,
              workspace_bytes, workspace, need);
    return 0;
  }
  hipStream_t st = (hipStream_t)stream;
  int* offsets = static_cast<int*>(workspace);
  int* order = offsets + up4((long long)B * ((long long)M + 1));
  // destinations: the M output rows; sources: the N ground-truth points; a key outside [0, M) goes to the nearest end
  if (!scatter_index_launch(idx1, B, M, N, offsets, order, st, true)) return 0;
  const int chunks = (M + kCdNT - 1) / kCdNT;
  const size_t tiles = (size_t)B * chunks;
  const unsigned grid = (unsigned)(tiles > kCdMaxBlocks ? kCdMaxBlocks : tiles);
  cd_loss_bw_kernel<<<grid, kCdNT, 0, st>>>(output, gt, dist1, dist2, idx2, g_p, g_t, offsets, order, tiles, chunks, N, M, gout);
  return check_launch(fn) ? 1 : 0;
}
