// solve_large.hip -- the fused HOUV optimisation loop for clouds of up to 16384 points (houv_solve_iterate_large).
//
// Same contract as solve.hip's solve_kernel: one workgroup owns one hypothesis for `n_iters` iterations of
//   pose -> moved cloud -> 4-metric bidirectional Chamfer -> top-k loss -> closed-form gradient -> Adam step,
// and only the 24-double state touches HBM between iterations.  What changes is where the clouds live: neither is
// resident in LDS (two clouds of 16384 points would need 512 KiB).
//   * queries in registers, in chunks: 1024 threads x 4 points = 4096 queries per chunk;
//   * references streamed through a double-buffered LDS tile of 1024 points (one per thread, plain loads issued before
//     the sweep of the previous tile, stored after it: one barrier per tile).  The moved cloud is built while filling the
//     tile, by solve_kernel's move_point (houv_solve.h), so its points are bit-identical.  All K hypotheses of a pair read
//     the same src / tgt: the stream is served from L2 / MALL;
//   * the sweep is houv_sweep.h's: wave-uniform ds_read_b128 broadcasts, 11 VALU ops per point pair and metric set, and the
//     16-reference tracking unit of each minimum (strict <: the lowest unit wins ties);
//   * only the full metric is parked: it needs top-k over the whole direction (k_full, usually N/2), so each query parks
//     its minimum (fp32 bits) and tracking unit (uint16) in LDS -- 6 B per query, one buffer for both directions.  After
//     the last chunk, the 4-pass radix select of houv_solve.h runs over the parked keys, read from LDS, and one pass over the
//     records accumulates the selected queries' sums.  Ties at the threshold are taken in (thread, point) order, the
//     order of solve_kernel<1024, 4>;
//   * the view metrics take every point (k_view == N == M, all the reference can do): their sums are accumulated from
//     registers at the end of each chunk;
//   * arg-min: the exact nearest neighbour is recovered by re-evaluating the winning tracking unit -- from GLOBAL memory
//     (the tile holding it is gone), with the same expression trees, hence the same point as solve_kernel's LDS rescan;
//   * G / GP are accumulated for BOTH directions of every metric (no prediction / repair as in solve_kernel: the 16-point
//     rescans are ~0.1 % of a direction's sweep at these sizes), and the scalar tail picks the winner as solve_kernel does.
//     The un-moved point of G p^T is the source point itself (loaded alongside the moved one), not R^T(p' - T).
// Deterministic: no float atomics; per-wave DPP sums, cross-wave sums in wave order, chunks in order.
#include <stddef.h>

#include "../../include/houv_hip.h"
#include "houv_common.h"
#include "houv_solve.h"

namespace houv {
namespace {

constexpr int kLBlock = 1024;              // threads per workgroup = one hypothesis
constexpr int kLQ = 4;                     // query points per lane and chunk
constexpr int kLChunk = kLBlock * kLQ;     // queries per chunk
constexpr int kLTile = 1024;               // reference points per LDS tile (one per thread)
constexpr int kLNW = kLBlock / 64;
static_assert(kLTile == kLBlock, "a tile is filled with one point per thread");
static_assert(kLTile % (2 * kTrk) == 0, "tiles hold whole pairs of tracking units");
static_assert(HOUV_LARGE_MAX_POINTS / kTrk <= 65536, "tracking units are parked as uint16");

struct LargeSmem {
  float4* tile;            // [2][kLTile] the streamed references
  double* state;           // [24]
  float* pose;             // [kPoseFloats] Pose of the current parameters: R row-major [0..8], T [9..11], intermediates
  float* acc;              // [8][kAccStride] slot = metric*2 + dir: S, G[3], GP[9]
  float* red;              // [kLNW][kRedStride]
  unsigned* hist;          // [kHistSets][256]
  int* ctl;                // [kLNW]
  unsigned* key;           // [max(N,M)] the full metric's minimum per query (fp32 bits) of the current direction
  unsigned short* unit;    // [max(N,M)] its tracking unit
};

__host__ __device__ inline size_t large_smem_bytes(int mx) {
  return (size_t)2 * kLTile * 16 + 24 * 8 + kPoseFloats * 4 + 8 * kAccStride * 4 + (size_t)kLNW * kRedStride * 4 +
         kHistSets * kHistBins * 4 + kLNW * 4 + (size_t)mx * 6;
}

__device__ inline LargeSmem large_carve(unsigned char* base, int mx) {
  LargeSmem s;
  s.tile = reinterpret_cast<float4*>(base);
  s.state = reinterpret_cast<double*>(s.tile + 2 * kLTile);
  s.pose = reinterpret_cast<float*>(s.state + 24);
  s.acc = s.pose + kPoseFloats;
  s.red = s.acc + 8 * kAccStride;
  s.hist = reinterpret_cast<unsigned*>(s.red + kLNW * kRedStride);
  s.ctl = reinterpret_cast<int*>(s.hist + kHistSets * kHistBins);
  s.key = reinterpret_cast<unsigned*>(s.ctl + kLNW);
  s.unit = reinterpret_cast<unsigned short*>(s.key + mx);
  return s;
}

// Reference j of the direction's reference cloud: DIR 1 (queries = moved points) references the target, DIR 0 (queries =
// target points) the moved source.  (sx, sy, sz) = the un-moved source point (DIR 0 only).
template <int DIR>
__device__ __forceinline__ void ref_point(const float* __restrict__ src, const float* __restrict__ tgt, int j,
                                          const float (&R)[9], const float (&T)[3], float& x, float& y, float& z,
                                          float& sx, float& sy, float& sz) {
  if constexpr (DIR == 1) {
    x = tgt[j * 3]; y = tgt[j * 3 + 1]; z = tgt[j * 3 + 2];
    sx = sy = sz = 0.f;
  } else {
    sx = src[j * 3]; sy = src[j * 3 + 1]; sz = src[j * 3 + 2];
    move_point(R, T, sx, sy, sz, x, y, z);
  }
}

// One query's share of metric MET's sums (S, G, GP) when it is selected: exact NN recovery from global memory (the lowest
// reference of tracking unit `u` at squared distance bd, solve_kernel's recover_nn rule) and the products of lane_grad_sums.
// (px, py, pz): the query's un-moved source point (DIR 1).
template <int MET, int DIR>
__device__ __forceinline__ void add_query(const float* __restrict__ src, const float* __restrict__ tgt, int nref,
                                          const float (&R)[9], const float (&T)[3], float qx, float qy, float qz, float px,
                                          float py, float pz, float bd, int u, float (&g)[kAccN]) {
  const float s = (bd < INFINITY) ? sqrtf(bd) : NAN;   // no finite distance -> NaN like torch's min/topk/sqrt chain
  g[0] += s;
  float nx = 0.f, ny = 0.f, nz = 0.f, ux = 0.f, uy = 0.f, uz = 0.f;
  bool found = false;
  const int j0 = u * kTrk;
#pragma unroll 4
  for (int j = 0; j < kTrk; ++j) {
    if (j0 + j < nref) {
      float x, y, z, sx, sy, sz;
      ref_point<DIR>(src, tgt, j0 + j, R, T, x, y, z, sx, sy, sz);
      const bool hit = metric_sqdist<MET>(x - qx, y - qy, z - qz) == bd;
      if ((hit && !found) || j == 0) {   // the unit's first point unless a match comes (solve_kernel: index 0 when none)
        nx = x; ny = y; nz = z; ux = sx; uy = sy; uz = sz;
      }
      found = found || hit;
    }
  }
  const float inv = 1.0f / s;   // d == 0 -> inf, and 0*inf = NaN below, as torch's sqrt backward gives
  float dx, dy, dz, sx, sy, sz;
  if constexpr (DIR == 1) {
    dx = qx - nx; dy = qy - ny; dz = qz - nz;
    sx = px; sy = py; sz = pz;
  } else {
    dx = nx - qx; dy = ny - qy; dz = nz - qz;
    sx = ux; sy = uy; sz = uz;
  }
  if constexpr (MET == 1) dx = 0.f;
  if constexpr (MET == 2) dy = 0.f;
  if constexpr (MET == 3) dz = 0.f;
  const float cx = dx * inv, cy = dy * inv, cz = dz * inv;
  g[1] += cx; g[2] += cy; g[3] += cz;
  g[4] += cx * sx; g[5] += cx * sy; g[6] += cx * sz;
  g[7] += cy * sx; g[8] += cy * sy; g[9] += cy * sz;
  g[10] += cz * sx; g[11] += cz * sy; g[12] += cz * sz;
}

// wave-level DPP sums of a lane's 13 sums, parked by lane 63 in red[wave][met*13 ..]
__device__ __forceinline__ void park13(const float (&g)[kAccN], float* red, int met) {
  float* dst = red + (tid_x() >> 6) * kRedStride + met * kAccN;
#pragma unroll
  for (int i = 0; i < kAccN; ++i) {
    const float v = wave_sum_to_lane63(g[i]);
    if ((tid_x() & 63) == 63) dst[i] = v;
  }
}

// Exact threshold of the `ksel` smallest of the `count` parked keys: houv_solve.h's radix select, reading the keys from LDS.
__device__ __forceinline__ void select_threshold(const LargeSmem& sm, int count, int ksel, int& hrot, RadixState& rs) {
  const int tid = tid_x(), lane = tid & 63;
  const int nj = (count + kLBlock - 1) / kLBlock;
  rs = RadixState{0u, 0u, ksel, 0};
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    unsigned* h = radix_rotate<kLBlock>(sm.hist, hrot, tid);
#pragma unroll 1
    for (int j = 0; j < nj; ++j) {
      const int q = j * kLBlock + tid;
      radix_count(h, (q < count) ? sm.key[q] : 0xFFFFFFFFu, pass, lane, rs);   // "not a point": digit 255 in pass 0, never selected
    }
    __syncthreads();
    radix_pick(h, pass, lane, rs);
  }
}

// One direction of one iteration: sweep every chunk of queries against the streamed references; the view metrics' sums
// at the end of each chunk; then the full metric's top-k and sums.  Leaves acc[(m*2 + DIR)][0..12] for every metric.
//   DIR 1 ("A"): queries = moved source points (count N), references = target.
//   DIR 0 ("B"): queries = target points (count M), references = moved source.
template <int NMET, int DIR>
__device__ __forceinline__ void large_direction(const LargeSmem& sm, const float* __restrict__ src, const float* __restrict__ tgt,
                                                int N, int M, int k_full, int& hrot) {
  const int tid = tid_x();
  const int count = DIR ? N : M, nref = DIR ? M : N;
  const int ntiles = (nref + kLTile - 1) / kLTile;
  const float4 pad4 = make_float4(INFINITY, INFINITY, INFINITY, 0.f);   // padding references never win
#pragma unroll 1
  for (int c0 = 0; c0 < count; c0 += kLChunk) {
    float qx[kLQ], qy[kLQ], qz[kLQ];
    {
      float R[9], T[3];
      load_rt(sm.pose, R, T);
#pragma unroll
    for (int k = 0; k < kLQ; ++k) {
      const int q = c0 + k * kLBlock + tid;
      qx[k] = qy[k] = qz[k] = 0.f;
      if (q < count) {
        if constexpr (DIR == 1) {
          move_point(R, T, src[q * 3], src[q * 3 + 1], src[q * 3 + 2], qx[k], qy[k], qz[k]);
        } else {
          qx[k] = tgt[q * 3]; qy[k] = tgt[q * 3 + 1]; qz[k] = tgt[q * 3 + 2];
        }
      }
    }
    }
    // ---- sweep: references streamed through the double-buffered tile ----
    float best[kLQ][NMET], other[kLQ][NMET];
    int btile[kLQ][NMET];
#pragma unroll
    for (int k = 0; k < kLQ; ++k)
#pragma unroll
      for (int m = 0; m < NMET; ++m) {
        best[k][m] = INFINITY;
        btile[k][m] = 0;
      }
    auto fetch = [&](int t) {
      const int j = t * kLTile + tid;
      float4 v = pad4;
      if (j < nref) {
        float Rf[9], Tf[3], sx, sy, sz;
        load_rt(sm.pose, Rf, Tf);   // from LDS at every fetch: R, T are not kept in registers across the sweep
        ref_point<DIR>(src, tgt, j, Rf, Tf, v.x, v.y, v.z, sx, sy, sz);
        v.w = 0.f;
      }
      return v;
    };
    sm.tile[tid] = fetch(0);
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < ntiles; ++t) {
      const bool more = t + 1 < ntiles;
      float4 nxt = pad4;
      if (more) nxt = fetch(t + 1);                       // in flight during this tile's sweep
      const float4* rp = sm.tile + (t & 1) * kLTile;
      const int len = min(kLTile, nref - t * kLTile);
      const int nunit = (len + 2 * kTrk - 1) / (2 * kTrk) * 2;   // whole pairs of tracking units (padding never wins)
      const int u0 = t * (kLTile / kTrk);
#pragma unroll 1
      for (int u = 0; u < nunit; u += 2) {
        // ping-pong of the running minimum as in sweep(): strict <, the earlier unit keeps ties
        sweep_tile<kLQ, NMET>(rp + u * kTrk, qx, qy, qz, best, other);
#pragma unroll
        for (int k = 0; k < kLQ; ++k)
#pragma unroll
          for (int m = 0; m < NMET; ++m) btile[k][m] = (other[k][m] < best[k][m]) ? u0 + u : btile[k][m];
        sweep_tile<kLQ, NMET>(rp + (u + 1) * kTrk, qx, qy, qz, other, best);
#pragma unroll
        for (int k = 0; k < kLQ; ++k)
#pragma unroll
          for (int m = 0; m < NMET; ++m) btile[k][m] = (best[k][m] < other[k][m]) ? u0 + u + 1 : btile[k][m];
      }
      if (more) sm.tile[((t + 1) & 1) * kLTile + tid] = nxt;
      __syncthreads();
    }
    // ---- park the full metric ----
#pragma unroll
    for (int k = 0; k < kLQ; ++k) {
      const int q = c0 + k * kLBlock + tid;
      if (q < count) {
        sm.key[q] = __float_as_uint(best[k][0]);
        sm.unit[q] = (unsigned short)btile[k][0];
      }
    }
    // ---- view metrics: every point takes part; sums straight from registers ----
    if constexpr (NMET == 4) {
      float R[9], T[3], px[kLQ], py[kLQ], pz[kLQ];
      load_rt(sm.pose, R, T);
#pragma unroll
      for (int k = 0; k < kLQ; ++k) {
        const int q = c0 + k * kLBlock + tid;
        px[k] = py[k] = pz[k] = 0.f;
        if (DIR == 1 && q < count) { px[k] = src[q * 3]; py[k] = src[q * 3 + 1]; pz[k] = src[q * 3 + 2]; }
      }
#define HOUV_LARGE_VIEW(MET)                                                                                         \
      {                                                                                                              \
        float g[kAccN];                                                                                             \
        _Pragma("unroll") for (int i = 0; i < kAccN; ++i) g[i] = 0.f;                                               \
        _Pragma("unroll") for (int k = 0; k < kLQ; ++k) {                                                            \
          if (c0 + k * kLBlock + tid < count)                                                                        \
            add_query<MET, DIR>(src, tgt, nref, R, T, qx[k], qy[k], qz[k], px[k], py[k], pz[k], best[k][MET],        \
                                btile[k][MET], g);                                                                   \
        }                                                                                                            \
        park13(g, sm.red, MET);                                                                                      \
      }
      HOUV_LARGE_VIEW(1)
      HOUV_LARGE_VIEW(2)
      HOUV_LARGE_VIEW(3)
#undef HOUV_LARGE_VIEW
      __syncthreads();
      if (tid < 3 * kAccN) {                          // chunk sums in wave order, added to the running sums in chunk order
        const int m = 1 + tid / kAccN, i = tid % kAccN;
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < kLNW; ++w) a += sm.red[w * kRedStride + m * kAccN + i];
        float* slot = sm.acc + (m * 2 + DIR) * kAccStride + i;
        *slot = (c0 == 0 ? 0.f : *slot) + a;
      }
    }
  }
  __syncthreads();   // every query's key is parked
  // ---- full metric: top-k over the parked keys, then the selected queries' sums ----
  const int lane = tid & 63, wave = tid >> 6;
  const int nj = (count + kLBlock - 1) / kLBlock;
  const bool all = k_full >= count;
  RadixState rs{0xFFFFFFFFu, 0u, 0, 0};
  int rank = 0;
  if (!all) {
    select_threshold(sm, count, k_full, hrot, rs);
    if (rs.neq != rs.remaining) {                            // ties at the threshold: taken in (thread, point) order
      int e = 0;
#pragma unroll 1
      for (int j = 0; j < nj; ++j) {
        const int q = j * kLBlock + tid;
        e += (q < count && sm.key[q] == rs.prefix) ? 1 : 0;
      }
      const int incl = wave_incl_scan_dpp(e);
      if (lane == 63) sm.ctl[wave] = incl;
      __syncthreads();
      rank = incl - e;
      for (int w = 0; w < wave; ++w) rank += sm.ctl[w];
    }
  }
  float R[9], T[3], g[kAccN];
  load_rt(sm.pose, R, T);
#pragma unroll
  for (int i = 0; i < kAccN; ++i) g[i] = 0.f;
#pragma unroll 1
  for (int j = 0; j < nj; ++j) {
    const int q = j * kLBlock + tid;
    if (q < count) {
      const unsigned k = sm.key[q];
      const bool eq = k == rs.prefix;
      const bool sel = all || k < rs.prefix || (eq && (rs.neq == rs.remaining || rank < rs.remaining));
      rank += eq ? 1 : 0;
      if (sel) {
        float qx, qy, qz, px = 0.f, py = 0.f, pz = 0.f;
        if constexpr (DIR == 1) {
          px = src[q * 3]; py = src[q * 3 + 1]; pz = src[q * 3 + 2];
          move_point(R, T, px, py, pz, qx, qy, qz);
        } else {
          qx = tgt[q * 3]; qy = tgt[q * 3 + 1]; qz = tgt[q * 3 + 2];
        }
        add_query<0, DIR>(src, tgt, nref, R, T, qx, qy, qz, px, py, pz, __uint_as_float(k), (int)sm.unit[q], g);
      }
    }
  }
  park13(g, sm.red, 0);
  __syncthreads();
  if (tid < kAccN) {
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < kLNW; ++w) a += sm.red[w * kRedStride + tid];
    sm.acc[DIR * kAccStride + tid] = a;
  }
  __syncthreads();   // acc complete; the parked keys and the tile may be overwritten by the next direction
}

template <int NMET>
__global__ __launch_bounds__(kLBlock) void solve_large_kernel(SolveCommon a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int N = a.N, M = a.M;
  const LargeSmem sm = large_carve(smem_raw, N > M ? N : M);
  const int tid = tid_x();
  const int ninst = a.P * a.K;
  // XCD-aware placement as in solve_kernel: the K restarts of one pair read the pair's clouds through one L2
  int inst = blockIdx.x;
  if ((ninst & 7) == 0) inst = (blockIdx.x & 7) * (ninst >> 3) + (blockIdx.x >> 3);
  const int pair = inst / a.K;
  const float* __restrict__ src = a.src + (size_t)pair * N * 3;
  const float* __restrict__ tgt = a.tgt + (size_t)pair * M * 3;

  if (tid < 24) sm.state[tid] = a.state[(size_t)inst * 24 + tid];
  if (tid < kHistBins) sm.hist[tid] = 0u;   // radix-select histogram set 0 (radix_rotate takes it from there)
  int hrot = 0;
  __syncthreads();
  if (tid == 0) {
    float p[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = (float)sm.state[k];
    Pose f;
    pose_forward(p, a.angle_base, a.trans_mode, f);
    store_pose(sm.pose, f);
  }
  __syncthreads();

#pragma unroll 1
  for (int it = 0; it < a.n_iters; ++it) {
    large_direction<NMET, 1>(sm, src, tgt, N, M, a.k_full, hrot);
    large_direction<NMET, 0>(sm, src, tgt, N, M, a.k_full, hrot);

    // ---- per-hypothesis scalar tail: loss, closed-form gradient, Adam, next pose ----
    if (tid == 0) {
      Pose f;
      load_pose(f, sm.pose);
      TailLoss r;
      solve_tail_loss<NMET>(sm.acc, kAccStride, f, a.k_full, a.k_view, a.loss_scale, a.trans_mode, r);
      if (it == a.n_iters - 1)
        store_outputs(a.out_score, a.out_loss, a.out_R, a.out_T, a.out_grad, a.out_cd, inst, f, r);
      solve_tail_step(r.g, sm.state, a.f64_params, adam_scalars(a.steps_done + it + 1, a.lr, a.beta1, a.beta2), a.beta1, a.beta2,
                      a.eps, a.angle_base, a.trans_mode, f);
      store_pose(sm.pose, f);
    }
    __syncthreads();
  }
  if (tid < 24) a.state[(size_t)inst * 24 + tid] = sm.state[tid];
}

}  // namespace
}  // namespace houv

extern "C" int houv_solve_iterate_large(const float* src, const float* tgt, int P, int N, int M, int K, double* state,
                                        int steps_done, int n_iters, int angle_base, int trans_mode, int use_views,
                                        int f64_params, int k_full, int k_view, double lr, double beta1, double beta2,
                                        double eps, float loss_scale, float* out_score, float* out_loss, float* out_R,
                                        float* out_T, float* out_grad, float* out_cd, void* stream) {
  using namespace houv;
  const char* who = "houv_solve_iterate_large";
  if (N < 1 || M < 1 || N > HOUV_LARGE_MAX_POINTS || M > HOUV_LARGE_MAX_POINTS) {
    set_error("%s: cloud sizes out of range (1 <= N, M <= %d; N=%d M=%d)", who, HOUV_LARGE_MAX_POINTS, N, M);
    return 0;
  }
  // the view terms take every point of both clouds: loss_view raises on N != M (model_utils_completion.py:158-163)
  if (use_views && (N != M || k_view != N)) {
    set_error("%s: the view terms need N == M and k_view == N (N=%d M=%d k_view=%d)", who, N, M, k_view);
    return 0;
  }
  const SolveCommon a{src, tgt, P, N, M, K, state, steps_done, n_iters, angle_base, trans_mode, f64_params, k_full, k_view,
                      lr, beta1, beta2, eps, loss_scale, out_score, out_loss, out_R, out_T, out_grad, out_cd};
  const int ok = solve_check_args(who, a, use_views);
  if (ok < 2) return ok;
  const size_t bytes = large_smem_bytes(N > M ? N : M);
  hipStream_t s = (hipStream_t)stream;
  const void* fn = use_views ? (const void*)solve_large_kernel<4> : (const void*)solve_large_kernel<1>;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) {
    set_error("%s: cannot reserve %zu B of LDS: %s", who, bytes, hipGetErrorString(e));
    return 0;
  }
  if (use_views)
    solve_large_kernel<4><<<P * K, kLBlock, bytes, s>>>(a);
  else
    solve_large_kernel<1><<<P * K, kLBlock, bytes, s>>>(a);
  return check_launch(who) ? 1 : 0;
}
