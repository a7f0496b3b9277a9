// pointops_group.hip -- the rest of the utils/mm3d_pn2 point ops (ball query, three-interpolate) and the one ordered scatter
// that serves as the backward pass of gather_points, grouping_operation and three_interpolate:
//   houv_ball_query            utils/mm3d_pn2/ops/ball_query/src/ball_query_cuda.cu:11-54
//   houv_three_interpolate     utils/mm3d_pn2/ops/interpolate/src/three_interpolate_cuda.cu (forward)
//   houv_scatter_points_grad   gather_points_cuda.cu / group_points_cuda.cu / three_interpolate_cuda.cu (backward kernels): the
//                              reference scatters with global float atomicAdd, whose sum order follows the scheduler; here every
//                              destination's terms are added by ONE lane in ascending source order, so the result is the
//                              sequential host loop's, bit for bit.
// All arithmetic is fp32 with the expression trees of include/houv_hip.h (compiled with -ffp-contract=off).
#include "../../include/houv_hip.h"
#include "houv_common.h"

namespace houv {
namespace {

// ---- ball query: one wave per centre -----------------------------------------------------------------------------------
// The kBallWaves waves of a workgroup serve kBallWaves consecutive centres of one cloud and share every tile of kBallTile
// points through LDS (raw xyz triples, loaded coalesced; the stride-3 reads of a wave touch 64 distinct banks mod 32 twice, i.e.
// conflict-free per 32-lane half).  A step tests 64 consecutive points, one per lane: __ballot gives the hit mask, mbcnt the
// number of hits in lower lanes = this hit's slot after the hits so far, which keeps index order without a serial scan.  The
// count is wave-uniform, so a wave stops testing once it holds nsample hits and the workgroup leaves once all its waves did.
constexpr int kBallWaves = 8;
constexpr int kBallTile = kBallWaves * 64;

__device__ __forceinline__ int lanes_below(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

__global__ __launch_bounds__(kBallTile) void ball_query_kernel(const float* __restrict__ xyz, const float* __restrict__ center,
                                                               int N, int Mc, float min2, float max2, int nsample,
                                                               int* __restrict__ idx, int* __restrict__ cnt_out) {
  __shared__ float s_p[kBallTile * 3];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = blockIdx.x * kBallWaves + wave;
  const bool live = c < Mc;
  const float* __restrict__ p = xyz + (size_t)b * N * 3;
  float cx = 0.f, cy = 0.f, cz = 0.f;
  if (live) {
    const float* q = center + ((size_t)b * Mc + c) * 3;
    cx = q[0]; cy = q[1]; cz = q[2];
  }
  int* __restrict__ out = idx + ((size_t)b * Mc + (live ? c : 0)) * nsample;
  int cnt = 0, first = 0;                  // wave-uniform: hits so far, index of the first hit
  bool done = !live;
  for (int t0 = 0; t0 < N; t0 += kBallTile) {
    if (__syncthreads_and(done)) break;    // also: the previous tile has been read by every wave
    const int nf = min(kBallTile, N - t0) * 3;
    for (int j = tid; j < nf; j += kBallTile) s_p[j] = p[(size_t)t0 * 3 + j];
    __syncthreads();
    if (!done) {
      const int steps = (min(kBallTile, N - t0) + 63) >> 6;
      for (int s = 0; s < steps; ++s) {
        const int k = t0 + s * 64 + lane;
        bool hit = false;
        if (k < N) {
          const float x = s_p[(s * 64 + lane) * 3 + 0], y = s_p[(s * 64 + lane) * 3 + 1], z = s_p[(s * 64 + lane) * 3 + 2];
          const float d2 = ((cx - x) * (cx - x) + (cy - y) * (cy - y)) + (cz - z) * (cz - z);
          hit = d2 == 0.f || (d2 >= min2 && d2 < max2);
        }
        const unsigned long long mask = __ballot(hit);
        if (mask) {
          if (cnt == 0) first = t0 + s * 64 + __builtin_ctzll(mask);
          const int slot = cnt + lanes_below(mask);
          if (hit && slot < nsample) out[slot] = k;
          cnt += __builtin_popcountll(mask);
          if (cnt >= nsample) { done = true; break; }
        }
      }
    }
  }
  if (live) {
    cnt = min(cnt, nsample);
    if (lane >= cnt && lane < nsample) out[lane] = first;     // nsample <= 64: one lane per unused slot; no hit: first == 0
    if (cnt_out && lane == 0) cnt_out[(size_t)b * Mc + c] = cnt;
  }
}

// ---- three_interpolate forward: out[b,c,i] = (w0*f[i0] + w1*f[i1]) + w2*f[i2] ----------------------------------------------
__global__ __launch_bounds__(256) void three_interpolate_kernel(const float* __restrict__ feat, const int* __restrict__ idx,
                                                                const float* __restrict__ weight, size_t total, int C, int M,
                                                                int N, float* __restrict__ out) {
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t bc = e / N;
    const int i = (int)(e - bc * N);
    const size_t b = bc / C;
    const int* __restrict__ j = idx + (b * N + i) * 3;
    const float* __restrict__ w = weight + (b * N + i) * 3;
    const float* __restrict__ f = feat + bc * M;
    out[e] = (w[0] * f[j[0]] + w[1] * f[j[1]]) + w[2] * f[j[2]];
  }
}

// ---- ordered scatter ---------------------------------------------------------------------------------------------------
// Step 1, scatter_index_kernel, one workgroup per cloud: a STABLE counting sort of the sources m = 0..M-1 by destination
// idx[m], giving the inverse index in CSR form: offsets[k] .. offsets[k+1] delimit, in order[], the sources of destination k
// in ascending m.  Destinations are taken kScatKeys at a time so that the counters live in LDS whatever N is (one pass up to
// 8192 destinations).  Per pass: integer LDS atomics count, a workgroup scan turns counts into cursors, then the sources are
// walked in chunks of 1024 in ascending m.  Inside a wave equal keys are ranked by a readlane/ballot loop (as many turns
// as the wave holds distinct keys; ONE when all are equal); the 16 waves of a chunk then take their base from the cursor one
// after the other, the lowest lane of each key advancing it by the wave's count.  The sort is exact integer work: no atomics
// decide an order.  Keys outside [0,N) are skipped; with CLAMP they are taken as the nearest of 0 and N-1 instead (the lists
// of houv_cd_loss_backward, which must not lose a source).
constexpr int kScatThreads = 1024;
constexpr int kScatWaves = kScatThreads / 64;
constexpr int kScatKeys = 8192;            // 32 KiB of LDS cursors
constexpr int kScatPer = kScatKeys / kScatThreads;

template <bool CLAMP>
__global__ __launch_bounds__(kScatThreads) void scatter_index_kernel(const int* __restrict__ idx, int N, int M,
                                                                     int* __restrict__ offsets, int* __restrict__ order) {
  auto key_of = [&](int v) { return CLAMP ? min(max(v, 0), N - 1) : v; };
  __shared__ int s_cur[kScatKeys];
  __shared__ int s_part[kScatWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int* __restrict__ key_in = idx + (size_t)b * M;
  int* __restrict__ off = offsets + (size_t)b * (N + 1);
  int* __restrict__ ord = order + (size_t)b * M;
  int carry = 0;                           // sources placed by earlier passes (workgroup-uniform)
  for (int k0 = 0; k0 < N; k0 += kScatKeys) {
    const int nk = min(kScatKeys, N - k0);
    for (int i = tid; i < kScatKeys; i += kScatThreads) s_cur[i] = 0;
    __syncthreads();
    for (int m = tid; m < M; m += kScatThreads) {
      const int key = key_of(key_in[m]) - k0;
      if ((unsigned)key < (unsigned)nk) atomicAdd(&s_cur[key], 1);
    }
    __syncthreads();
    // exclusive scan of the counts: every thread owns kScatPer consecutive destinations
    int mine[kScatPer], t = 0;
#pragma unroll
    for (int i = 0; i < kScatPer; ++i) { mine[i] = s_cur[tid * kScatPer + i]; t += mine[i]; }
    const int incl = wave_incl_scan_i(t);
    if (lane == 63) s_part[wave] = incl;
    __syncthreads();
    int before = carry, total = 0;
#pragma unroll
    for (int w = 0; w < kScatWaves; ++w) { const int v = s_part[w]; before += w < wave ? v : 0; total += v; }
    int run = before + incl - t;
#pragma unroll
    for (int i = 0; i < kScatPer; ++i) {
      const int k = tid * kScatPer + i;
      s_cur[k] = run;
      if (k < nk) off[k0 + k] = run;
      run += mine[i];
    }
    carry += total;
    __syncthreads();
    // place the sources, 1024 at a time in ascending m
    for (int m0 = 0; m0 < M; m0 += kScatThreads) {
      const int m = m0 + tid;
      const int key = m < M ? key_of(key_in[m]) - k0 : -1;
      const bool valid = (unsigned)key < (unsigned)nk;
      int rank = 0, cnt = 0;
      unsigned long long pend = __ballot(valid);
      while (pend) {                       // wave-uniform loop: one turn per distinct key, the lowest unranked lane's first
        const int k1 = __builtin_amdgcn_readlane(key, __builtin_ctzll(pend));
        const bool same = valid && key == k1;
        const unsigned long long mask = __ballot(same);
        if (same) { rank = lanes_below(mask); cnt = __builtin_popcountll(mask); }
        pend &= ~mask;
      }
      const int waves_here = min(kScatWaves, (M - m0 + 63) >> 6);
      int base = 0;
      for (int w = 0; w < waves_here; ++w) {
        if (wave == w && valid) {
          base = s_cur[key];               // read by every lane of the key before its lowest lane advances the cursor
          if (rank == 0) s_cur[key] = base + cnt;
        }
        __syncthreads();
      }
      if (valid) ord[base + rank] = m;
    }
    __syncthreads();                       // s_cur / s_part are reused by the next pass
  }
  if (tid == 0) off[N] = carry;
}

// Step 2: one lane owns destination k of one channel and adds its list in order, starting from the first term (0 where the
// list is empty).  Lanes run along k: the offsets and the result are coalesced, the terms are gathered.  The loads of a list are
// independent of the running sum and are issued four ahead of the adds.
template <int S>   // S = 1, 3: compile-time stride; 0: run-time `stride`
__global__ __launch_bounds__(256) void scatter_sum_kernel(const float* __restrict__ grad_out, const float* __restrict__ weight,
                                                          const int* __restrict__ offsets, const int* __restrict__ order,
                                                          size_t total, int C, int N, int M, int stride,
                                                          float* __restrict__ grad_features) {
  const int st = S ? S : stride;
  const int Mo = M / st;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t bc = e / N;
    const int k = (int)(e - bc * N);
    const size_t b = bc / C;
    const int* __restrict__ off = offsets + b * (N + 1);
    const int* __restrict__ ord = order + b * M;
    const float* __restrict__ g = grad_out + bc * Mo;
    const float* __restrict__ w = weight ? weight + b * M : nullptr;
    auto term = [&](int j) {
      const int m = ord[j];
      const float v = g[m / st];
      return w ? v * w[m] : v;
    };
    int j = off[k];
    const int end = off[k + 1];
    float acc = 0.f;
    if (j < end) {
      acc = term(j);
      ++j;
      for (; j + 4 <= end; j += 4) {
        const float t0 = term(j), t1 = term(j + 1), t2 = term(j + 2), t3 = term(j + 3);
        acc = acc + t0; acc = acc + t1; acc = acc + t2; acc = acc + t3;
      }
      for (; j < end; ++j) acc = acc + term(j);
    }
    grad_features[e] = acc;
  }
}

unsigned grid_for(size_t total) {
  size_t blocks = (total + 255) / 256;
  return (unsigned)(blocks > 16384 ? 16384 : blocks);
}

}  // namespace

bool scatter_index_launch(const int* keys, int B, int N, int M, int* offsets, int* order, hipStream_t stream, bool clamp) {
  if (clamp) scatter_index_kernel<true><<<B, kScatThreads, 0, stream>>>(keys, N, M, offsets, order);
  else scatter_index_kernel<false><<<B, kScatThreads, 0, stream>>>(keys, N, M, offsets, order);
  return check_launch("scatter_index_kernel");
}

}  // namespace houv

extern "C" int houv_ball_query(const float* xyz, const float* center, int B, int N, int Mc, float min_radius, float max_radius,
                               int nsample, int32_t* idx, int32_t* cnt_or_null, void* stream) {
  using namespace houv;
  if (B < 0 || N < 1 || Mc < 0 || nsample < 1 || nsample > 64 || !(min_radius < max_radius)) {
    set_error("houv_ball_query: bad argument B=%d N=%d Mc=%d nsample=%d (1..64) min_radius=%g max_radius=%g", B, N, Mc, nsample,
              (double)min_radius, (double)max_radius);
    return 0;
  }
  if (B == 0 || Mc == 0) return 1;
  if (B > 65535) { set_error("houv_ball_query: B=%d > 65535 not supported", B); return 0; }
  if (!xyz || !center || !idx) { set_error("houv_ball_query: null pointer"); return 0; }
  const float min2 = min_radius * min_radius, max2 = max_radius * max_radius;
  dim3 grid((Mc + kBallWaves - 1) / kBallWaves, B);
  ball_query_kernel<<<grid, kBallTile, 0, (hipStream_t)stream>>>(xyz, center, N, Mc, min2, max2, nsample, idx, cnt_or_null);
  return check_launch("houv_ball_query") ? 1 : 0;
}

extern "C" int houv_three_interpolate(const float* features, const int32_t* idx, const float* weight, int B, int C, int M, int N,
                                      float* out, void* stream) {
  using namespace houv;
  if (B < 0 || C <= 0 || M <= 0 || N <= 0) { set_error("houv_three_interpolate: bad argument B=%d C=%d M=%d N=%d", B, C, M, N); return 0; }
  if (B == 0) return 1;
  if (!features || !idx || !weight || !out) { set_error("houv_three_interpolate: null pointer"); return 0; }
  const size_t total = (size_t)B * C * N;
  three_interpolate_kernel<<<grid_for(total), 256, 0, (hipStream_t)stream>>>(features, idx, weight, total, C, M, N, out);
  return check_launch("houv_three_interpolate") ? 1 : 0;
}

extern "C" long long houv_scatter_points_workspace_bytes(int B, int N, int M) {
  if (B <= 0 || N <= 0 || M <= 0) return 0;
  return 4ll * ((long long)B * ((long long)N + 1) + (long long)B * M);     // offsets[B][N+1], order[B][M]
}

extern "C" int houv_scatter_points_grad(const float* grad_out, const int32_t* idx, const float* weight_or_null, int B, int C, int N,
                                        int M, int S, float* grad_features, void* workspace, void* stream) {
  using namespace houv;
  if (B < 0 || C <= 0 || N <= 0 || M <= 0 || S <= 0 || M % S != 0) {
    set_error("houv_scatter_points_grad: bad argument B=%d C=%d N=%d M=%d S=%d (M must be a multiple of S)", B, C, N, M, S);
    return 0;
  }
  if (B == 0) return 1;
  if (!grad_out || !idx || !grad_features || !workspace) { set_error("houv_scatter_points_grad: null pointer"); return 0; }
  hipStream_t s = (hipStream_t)stream;
  int* offsets = (int*)workspace;
  int* order = offsets + (size_t)B * ((size_t)N + 1);
  scatter_index_kernel<false><<<B, kScatThreads, 0, s>>>(idx, N, M, offsets, order);
  if (!check_launch("houv_scatter_points_grad")) return 0;
  const size_t total = (size_t)B * C * N;
  if (S == 1) scatter_sum_kernel<1><<<grid_for(total), 256, 0, s>>>(grad_out, weight_or_null, offsets, order, total, C, N, M, S, grad_features);
  else if (S == 3) scatter_sum_kernel<3><<<grid_for(total), 256, 0, s>>>(grad_out, weight_or_null, offsets, order, total, C, N, M, S, grad_features);
  else scatter_sum_kernel<0><<<grid_for(total), 256, 0, s>>>(grad_out, weight_or_null, offsets, order, total, C, N, M, S, grad_features);
  return check_launch("houv_scatter_points_grad") ? 1 : 0;
}
