// solve_large.hip -- the fused HOUV optimisation loop for clouds of up to 16384 points (houv_solve_iterate_large).
//
// Same contract as solve.hip's solve_kernel: one workgroup owns one hypothesis for `n_iters` iterations of
//   pose -> moved cloud -> 4-metric bidirectional Chamfer -> top-k loss -> closed-form gradient -> Adam step,
// and only the 24-double state touches HBM between iterations.  What changes is where the clouds live: neither is
// resident in LDS (two clouds of 16384 points would need 512 KiB).
//   * queries in registers, in chunks: 1024 threads x 4 points = 4096 queries per chunk;
//   * references streamed through a double-buffered LDS tile of 1024 points (one per thread, plain loads issued before
//     the sweep of the previous tile, stored after it: one barrier per tile).  The moved cloud is built while filling the
//     tile, with the FMA order of solve_kernel's sm.mov, so its points are bit-identical.  All K hypotheses of a pair read
//     the same src / tgt: the stream is served from L2 / MALL;
//   * the sweep is houv_sweep.h's: wave-uniform ds_read_b128 broadcasts, 11 VALU ops per point pair and metric set, and the
//     16-reference tracking unit of each minimum (strict <: the lowest unit wins ties);
//   * only the full metric is parked: it needs top-k over the whole direction (k_full, usually N/2), so each query parks
//     its minimum (fp32 bits) and tracking unit (uint16) in LDS -- 6 B per query, one buffer for both directions.  After
//     the last chunk, solve.hip's 4-pass radix select runs over the parked keys, read from LDS, and one pass over the
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
#include "houv_sweep.h"

namespace houv {
namespace {

constexpr int kLBlock = 1024;              // threads per workgroup = one hypothesis
constexpr int kLQ = 4;                     // query points per lane and chunk
constexpr int kLChunk = kLBlock * kLQ;     // queries per chunk
constexpr int kLTile = 1024;               // reference points per LDS tile (one per thread)
constexpr int kLNW = kLBlock / 64;
constexpr int kLAccN = 13;                 // sum sqrt(d), G[3], (G p^T)[9]
constexpr int kLRed = 4 * kLAccN;          // per-wave partial sums: [metric][13]
constexpr int kLHistBins = 256;
constexpr int kLHistSets = 3;              // rotating radix-select histograms (see select_smallest in solve.hip)
constexpr int kLPoseFloats = 28;
static_assert(sizeof(Pose) <= kLPoseFloats * 4 && offsetof(Pose, T) == 36, "pose[0..11] must be R | T");
static_assert(kLTile == kLBlock, "a tile is filled with one point per thread");
static_assert(kLTile % (2 * kTrk) == 0, "tiles hold whole pairs of tracking units");
static_assert(HOUV_LARGE_MAX_POINTS / kTrk <= 65536, "tracking units are parked as uint16");

struct LargeArgs {
  const float* src;
  const float* tgt;
  int P, N, M, K;
  double* state;
  int steps_done, n_iters, angle_base, trans_mode, f64_params, k_full, k_view;
  double lr, beta1, beta2, eps;
  float loss_scale;
  float* out_score;
  float* out_loss;
  float* out_R;
  float* out_T;
  float* out_grad;
  float* out_cd;
};

struct LargeSmem {
  float4* tile;            // [2][kLTile] the streamed references
  double* state;           // [24]
  float* pose;             // [kLPoseFloats] Pose of the current parameters: R row-major [0..8], T [9..11], intermediates
  float* acc;              // [8][kAccStride] slot = metric*2 + dir: S, G[3], GP[9]
  float* red;              // [kLNW][kLRed]
  unsigned* hist;          // [kLHistSets][256]
  int* ctl;                // [kLNW]
  unsigned* key;           // [max(N,M)] the full metric's minimum per query (fp32 bits) of the current direction
  unsigned short* unit;    // [max(N,M)] its tracking unit
};

__host__ __device__ inline size_t large_smem_bytes(int mx) {
  return (size_t)2 * kLTile * 16 + 24 * 8 + kLPoseFloats * 4 + 8 * kAccStride * 4 + (size_t)kLNW * kLRed * 4 +
         kLHistSets * kLHistBins * 4 + kLNW * 4 + (size_t)mx * 6;
}

__device__ inline LargeSmem large_carve(unsigned char* base, int mx) {
  LargeSmem s;
  s.tile = reinterpret_cast<float4*>(base);
  s.state = reinterpret_cast<double*>(s.tile + 2 * kLTile);
  s.pose = reinterpret_cast<float*>(s.state + 24);
  s.acc = s.pose + kLPoseFloats;
  s.red = s.acc + 8 * kAccStride;
  s.hist = reinterpret_cast<unsigned*>(s.red + kLNW * kLRed);
  s.ctl = reinterpret_cast<int*>(s.hist + kLHistSets * kLHistBins);
  s.key = reinterpret_cast<unsigned*>(s.ctl + kLNW);
  s.unit = reinterpret_cast<unsigned short*>(s.key + mx);
  return s;
}

// src @ R^T + T (houv.py:102), the expression tree of solve_kernel's moved points
__device__ __forceinline__ void move_point(const float (&R)[9], const float (&T)[3], float sx, float sy, float sz, float& mx,
                                           float& my, float& mz) {
  mx = __builtin_fmaf(sz, R[2], __builtin_fmaf(sy, R[1], sx * R[0])) + T[0];
  my = __builtin_fmaf(sz, R[5], __builtin_fmaf(sy, R[4], sx * R[3])) + T[1];
  mz = __builtin_fmaf(sz, R[8], __builtin_fmaf(sy, R[7], sx * R[6])) + T[2];
}

__device__ __forceinline__ void load_pose_rt(const LargeSmem& sm, float (&R)[9], float (&T)[3]) {
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = sm.pose[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) T[i] = sm.pose[9 + i];
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
                                          float py, float pz, float bd, int u, float (&g)[kLAccN]) {
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
__device__ __forceinline__ void park13(const float (&g)[kLAccN], float* red, int met) {
  float* dst = red + (tid_x() >> 6) * kLRed + met * kLAccN;
#pragma unroll
  for (int i = 0; i < kLAccN; ++i) {
    const float v = wave_sum_to_lane63(g[i]);
    if ((tid_x() & 63) == 63) dst[i] = v;
  }
}

// Exact threshold of the `ksel` smallest of the `count` parked keys (fp32 bit patterns of non-negative distances): the
// 4-pass 8-bit radix select of solve.hip's select_smallest, reading the keys from LDS.  Returns the ksel-th smallest key
// (prefix), how many of the keys equal to it are still to be taken (remaining) and how many there are (neq).
__device__ __forceinline__ void select_threshold(const LargeSmem& sm, int count, int ksel, int& hrot, unsigned& prefix_out,
                                                 int& remaining_out, int& neq_out) {
  const int tid = tid_x(), lane = tid & 63;
  const int nj = (count + kLBlock - 1) / kLBlock;
  unsigned prefix = 0u, mask = 0u;
  int remaining = ksel, neq = 0;
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    unsigned* h = sm.hist + hrot * kLHistBins;
    const int nxt = (hrot == kLHistSets - 1) ? 0 : hrot + 1;
    if (tid < kLHistBins) sm.hist[nxt * kLHistBins + tid] = 0u;
#pragma unroll 1
    for (int j = 0; j < nj; ++j) {
      const int q = j * kLBlock + tid;
      const unsigned k = (q < count) ? sm.key[q] : 0xFFFFFFFFu;   // "not a point": digit 255 in pass 0, never selected
      if (pass == 0) {
        const unsigned digit = k >> 24;
        unsigned long long todo = __ballot(1);
        while (todo) {                                           // wave-uniform loop over the distinct digits
          const int leader = __ffsll((long long)todo) - 1;
          const unsigned d = (unsigned)__builtin_amdgcn_readlane((int)digit, leader);
          const unsigned long long m = __ballot(digit == d);
          if (lane == leader) atomicAdd(&h[d], (unsigned)__popcll(m));
          todo &= ~m;
        }
      } else if ((k & mask) == prefix) {
        atomicAdd(&h[(k >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    {
      const uint4 hv = *reinterpret_cast<const uint4*>(h + 4 * lane);
      const int hh[4] = {(int)hv.x, (int)hv.y, (int)hv.z, (int)hv.w};
      const int tot = hh[0] + hh[1] + hh[2] + hh[3];
      int c = wave_incl_scan_dpp(tot) - tot;
      int fbin = 0, fc = 0, fn = 0;
      bool found = false;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const bool hit = c < remaining && remaining <= c + hh[b];
        fbin = hit ? 4 * lane + b : fbin;
        fc = hit ? c : fc;
        fn = hit ? hh[b] : fn;
        found = found || hit;
        c += hh[b];
      }
      const int src_lane = __ffsll((long long)__ballot(found)) - 1;   // exactly one lane holds the bin
      const int bin = __builtin_amdgcn_readlane(fbin, src_lane);
      prefix |= (unsigned)bin << shift;
      mask |= 255u << shift;
      remaining -= __builtin_amdgcn_readlane(fc, src_lane);
      neq = __builtin_amdgcn_readlane(fn, src_lane);
    }
    hrot = nxt;
  }
  prefix_out = prefix;
  remaining_out = remaining;
  neq_out = neq;
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
      load_pose_rt(sm, R, T);
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
        load_pose_rt(sm, Rf, Tf);   // from LDS at every fetch: R, T are not kept in registers across the sweep
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
      load_pose_rt(sm, R, T);
#pragma unroll
      for (int k = 0; k < kLQ; ++k) {
        const int q = c0 + k * kLBlock + tid;
        px[k] = py[k] = pz[k] = 0.f;
        if (DIR == 1 && q < count) { px[k] = src[q * 3]; py[k] = src[q * 3 + 1]; pz[k] = src[q * 3 + 2]; }
      }
#define HOUV_LARGE_VIEW(MET)                                                                                         \
      {                                                                                                              \
        float g[kLAccN];                                                                                             \
        _Pragma("unroll") for (int i = 0; i < kLAccN; ++i) g[i] = 0.f;                                               \
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
      if (tid < 3 * kLAccN) {                          // chunk sums in wave order, added to the running sums in chunk order
        const int m = 1 + tid / kLAccN, i = tid % kLAccN;
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < kLNW; ++w) a += sm.red[w * kLRed + m * kLAccN + i];
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
  unsigned prefix = 0xFFFFFFFFu;
  int remaining = 0, neq = 0, rank = 0;
  if (!all) {
    select_threshold(sm, count, k_full, hrot, prefix, remaining, neq);
    if (neq != remaining) {                            // ties at the threshold: taken in (thread, point) order
      int e = 0;
#pragma unroll 1
      for (int j = 0; j < nj; ++j) {
        const int q = j * kLBlock + tid;
        e += (q < count && sm.key[q] == prefix) ? 1 : 0;
      }
      const int incl = wave_incl_scan_dpp(e);
      if (lane == 63) sm.ctl[wave] = incl;
      __syncthreads();
      rank = incl - e;
      for (int w = 0; w < wave; ++w) rank += sm.ctl[w];
    }
  }
  float R[9], T[3], g[kLAccN];
  load_pose_rt(sm, R, T);
#pragma unroll
  for (int i = 0; i < kLAccN; ++i) g[i] = 0.f;
#pragma unroll 1
  for (int j = 0; j < nj; ++j) {
    const int q = j * kLBlock + tid;
    if (q < count) {
      const unsigned k = sm.key[q];
      const bool eq = k == prefix;
      const bool sel = all || k < prefix || (eq && (neq == remaining || rank < remaining));
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
  if (tid < kLAccN) {
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < kLNW; ++w) a += sm.red[w * kLRed + tid];
    sm.acc[DIR * kAccStride + tid] = a;
  }
  __syncthreads();   // acc complete; the parked keys and the tile may be overwritten by the next direction
}

template <int NMET>
__global__ __launch_bounds__(kLBlock) void solve_large_kernel(LargeArgs a) {
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
  if (tid < kLHistBins) sm.hist[tid] = 0u;   // radix-select histogram set 0 (select_threshold rotates)
  int hrot = 0;
  __syncthreads();
  if (tid == 0) {
    float p[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = (float)sm.state[k];
    Pose f;
    pose_forward(p, a.angle_base, a.trans_mode, f);
    const float* fs = reinterpret_cast<const float*>(&f);
    for (int i = 0; i < (int)(sizeof(Pose) / 4); ++i) sm.pose[i] = fs[i];
  }
  __syncthreads();

#pragma unroll 1
  for (int it = 0; it < a.n_iters; ++it) {
    large_direction<NMET, 1>(sm, src, tgt, N, M, a.k_full, hrot);
    large_direction<NMET, 0>(sm, src, tgt, N, M, a.k_full, hrot);

    // ---- per-hypothesis scalar tail (solve_kernel's): loss, closed-form gradient, Adam, next pose ----
    if (tid == 0) {
      Pose f;
      float* fs = reinterpret_cast<float*>(&f);
      for (int i = 0; i < (int)(sizeof(Pose) / 4); ++i) fs[i] = sm.pose[i];
      float cd[NMET][2], val[NMET];
      int pick[NMET];
      float gT[3] = {0.f, 0.f, 0.f}, Mm[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      bool bad = false;
#pragma unroll
      for (int m = 0; m < NMET; ++m) {
        const float kk = (float)((m == 0) ? a.k_full : a.k_view);
        cd[m][0] = sm.acc[(m * 2 + 0) * kAccStride] / kk;   // over target points   (calc_cd_percent's 1st output)
        cd[m][1] = sm.acc[(m * 2 + 1) * kAccStride] / kk;   // over moved points    (2nd output)
        // torch.min(cat([first, second])): first wins ties; NaN propagates
        pick[m] = (cd[m][0] <= cd[m][1]) ? 0 : 1;
        val[m] = cd[m][pick[m]];
        if (cd[m][0] != cd[m][0] || cd[m][1] != cd[m][1]) { val[m] = NAN; bad = true; }
        const float w = ((m == 0) ? 6.0f : 1.0f) * a.loss_scale / kk;
        const float* ac = sm.acc + (m * 2 + pick[m]) * kAccStride;
#pragma unroll
        for (int i = 0; i < 3; ++i) gT[i] += w * ac[1 + i];
#pragma unroll
        for (int i = 0; i < 9; ++i) Mm[i] += w * ac[4 + i];
      }
      float loss = val[0] * 6.0f;                            // houv.py:222 / train_utils.py:433
      if constexpr (NMET == 4) loss = loss + (val[1] + val[2] + val[3]);
      if (bad) {
#pragma unroll
        for (int i = 0; i < 3; ++i) gT[i] = NAN;
#pragma unroll
        for (int i = 0; i < 9; ++i) Mm[i] = NAN;
      }
      float g[8];
      pose_backward(f, a.trans_mode, gT, Mm, g);
      if (it == a.n_iters - 1) {
        // outputs of the LAST forward (houv.py:134-136: the final step is never observed)
        if (a.out_score) a.out_score[inst] = val[0];
        if (a.out_loss) a.out_loss[inst] = loss;
        if (a.out_R)
          for (int k = 0; k < 9; ++k) a.out_R[(size_t)inst * 9 + k] = f.R[k];
        if (a.out_T)
          for (int k = 0; k < 3; ++k) a.out_T[(size_t)inst * 3 + k] = f.T[k];
        if (a.out_grad)
          for (int k = 0; k < 8; ++k) a.out_grad[(size_t)inst * 8 + k] = g[k];
        if (a.out_cd)
          for (int m = 0; m < 4; ++m)
            for (int d = 0; d < 2; ++d) a.out_cd[(size_t)inst * 8 + m * 2 + d] = (m < NMET) ? cd[m < NMET ? m : 0][d] : 0.f;
      }
      const int step = a.steps_done + it + 1;
      const AdamScalars asc = adam_scalars(step, a.lr, a.beta1, a.beta2);
      if (a.f64_params) {
        for (int k = 0; k < 8; ++k)
          adam_step<double>(sm.state[k], sm.state[8 + k], sm.state[16 + k], (double)g[k], asc, a.beta1, a.beta2, a.eps);
      } else {
        for (int k = 0; k < 8; ++k) {
          float pp = (float)sm.state[k], mm = (float)sm.state[8 + k], vv = (float)sm.state[16 + k];
          adam_step<float>(pp, mm, vv, g[k], asc, a.beta1, a.beta2, a.eps);
          sm.state[k] = pp; sm.state[8 + k] = mm; sm.state[16 + k] = vv;
        }
      }
      float p[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) p[k] = (float)sm.state[k];
      pose_forward(p, a.angle_base, a.trans_mode, f);
      for (int i = 0; i < (int)(sizeof(Pose) / 4); ++i) sm.pose[i] = fs[i];
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
  if (P < 0 || K <= 0 || n_iters <= 0 || steps_done < 0 || angle_base < 0 || angle_base > 3 || trans_mode < 0 ||
      trans_mode > 1) {
    set_error("%s: bad argument P=%d N=%d M=%d K=%d n_iters=%d steps_done=%d base=%d trans_mode=%d", who, P, N, M, K,
              n_iters, steps_done, angle_base, trans_mode);
    return 0;
  }
  // the view terms take every point of both clouds: loss_view raises on N != M (model_utils_completion.py:158-163)
  if (use_views && (N != M || k_view != N)) {
    set_error("%s: the view terms need N == M and k_view == N (N=%d M=%d k_view=%d)", who, N, M, k_view);
    return 0;
  }
  const int kv = use_views ? k_view : 1;
  if (k_full < 1 || k_full > N || k_full > M || kv < 1 || kv > N || kv > M) {
    set_error("%s: top-k size out of range (k_full=%d k_view=%d N=%d M=%d)", who, k_full, k_view, N, M);
    return 0;
  }
  if ((long long)P * K > 0x7fffffffLL) {
    set_error("%s: too many hypotheses", who);
    return 0;
  }
  if (P == 0) return 1;
  if (!src || !tgt || !state) {
    set_error("%s: null pointer", who);
    return 0;
  }
  LargeArgs a{src, tgt, P, N, M, K, state, steps_done, n_iters, angle_base, trans_mode, f64_params, k_full, k_view,
              lr, beta1, beta2, eps, loss_scale, out_score, out_loss, out_R, out_T, out_grad, out_cd};
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
