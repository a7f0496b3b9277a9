// solve_seed.hip -- first-guess neighbour records for the pruned solve (houv_solve_seed; DESIGN.md 3.1b, Seeded first iteration).
//
// A stage of the pruned solve starts with an empty workspace, so its first iteration has no remembered neighbours to bound the
// search with and runs the brute-force sweep: 2 x N x M point pairs per hypothesis, against ~1/8 of that in the steady state.
// Any in-range record whose reference lies at a finite distance is an attained upper bound ("costs visits, not correctness",
// solve.hip), so a cheap guess is enough to let that iteration run the pruned search too: this kernel writes one.
//
// One workgroup per hypothesis, both clouds in LDS.  Per query and metric: the 32-point run whose box is nearest to the query in
// the metric's projection, then the nearest point of that run.  The per-metric choice of the box is what makes the guess good: the
// view metrics search in projections, where the nearest box of the 3-D metric is often far from the nearest point (the replay
// scripts/sim_solve_seed.py: 9.4 sub-tiles asked per query with this rule, 14.1 with the 3-D box for all metrics, 6.3 with exact
// neighbours).  ~0.2 M wave-instructions per hypothesis at 2048 points, against 1.5 M of the brute-force iteration it replaces.
// The kernel has no float atomics and no scratch; solve_kernel is not touched.
#include <stdint.h>

#include "../../include/houv_hip.h"
#include "houv_common.h"
#include "houv_solve.h"

namespace houv {
namespace {

constexpr int kSeedMinPoints = 257;    // houv_solve_variant: up to 256 points the brute-force kernel runs
constexpr int kSeedMaxPoints = 4096;

struct SeedArgs {
  const float* src;
  const float* tgt;
  int N, M, K;
  const double* state;
  int angle_base, trans_mode;
  short* nn_ws;
  int ws_stride;
};

__host__ __device__ inline int seed_pad(int n) { return (n + kSub - 1) / kSub * kSub; }
// both clouds, the boxes of their runs (lo, hi per run), R | T
__host__ __device__ inline size_t seed_smem_bytes(int N, int M) {
  return (size_t)(seed_pad(N) + seed_pad(M)) * 16 + (size_t)(seed_pad(N) + seed_pad(M)) / kSub * 32 + 12 * 4;
}

// boxes of the 32-point runs of `pts` (count points): run t by thread first + t, from its existing points only; fminf / fmaxf leave
// a NaN coordinate out, and a run with no number on an axis keeps lo = +inf, hi = -inf there (at infinite distance from any query)
__device__ __forceinline__ void seed_boxes(const float4* pts, int count, int ntile, int first, float4* box) {
  const int t = (int)threadIdx.x - first;
  if (t < 0 || t >= ntile) return;
  float lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
  for (int i = 0; i < kSub; ++i) {
    const int j = t * kSub + ((i + t) & (kSub - 1));   // rotated per run: the runs are 512 B apart in LDS
    if (j < count) {
      const float4 p = pts[j];
      lx = fminf(lx, p.x); ly = fminf(ly, p.y); lz = fminf(lz, p.z);
      hx = fmaxf(hx, p.x); hy = fmaxf(hy, p.y); hz = fmaxf(hz, p.z);
    }
  }
  box[2 * t] = make_float4(lx, ly, lz, 0.f);
  box[2 * t + 1] = make_float4(hx, hy, hz, 0.f);
}

// the point of run `tile` nearest to the query in metric MET: strict < from +inf, the lowest index among equals (the scan order is
// rotated per lane -- lanes read different runs, 512 B apart -- so the index takes part in the comparison).  No reference of the run
// at a finite distance: the first one of the whole cloud that is; none: 0.
template <int MET>
__device__ __forceinline__ int seed_nearest(const float4* refs, int count, int tile, float qx, float qy, float qz) {
  float best = INFINITY;
  int bi = 0;
  const int rot = (int)threadIdx.x & (kSub - 1);
#pragma unroll 4
  for (int i = 0; i < kSub; ++i) {
    const int j = tile * kSub + ((i + rot) & (kSub - 1));
    const float4 r = refs[j];                           // in the padded cloud (+inf past the end)
    const float d = metric_sqdist<MET>(r.x - qx, r.y - qy, r.z - qz);
    const bool take = j < count && (d < best || (d == best && d < INFINITY && j < bi));
    best = take ? d : best;
    bi = take ? j : bi;
  }
  if (!(best < INFINITY)) {   // rare: a run of NaN points, a query at NaN or Inf
    bi = 0;
    for (int j = 0; j < count; ++j) {
      const float4 r = refs[j];
      if (metric_sqdist<MET>(r.x - qx, r.y - qy, r.z - qz) < INFINITY) {
        bi = j;
        break;
      }
    }
  }
  return bi;
}

// records of one direction: the queries `qpts` (nq of them) against the references `refs` (count, in runs with boxes `box`)
template <int BLOCK, int NMET>
__device__ __forceinline__ void seed_direction(const float4* qpts, int nq, const float4* refs, int count, const float4* box,
                                               short* rec) {
  const int ntile = (count + kSub - 1) / kSub;
  for (int q = (int)threadIdx.x; q < nq; q += BLOCK) {
    const float4 qp = qpts[q];
    float bd[NMET];
    int bt[NMET];
#pragma unroll
    for (int m = 0; m < NMET; ++m) { bd[m] = INFINITY; bt[m] = 0; }
    for (int t = 0; t < ntile; ++t) {                   // wave-uniform box: LDS broadcasts
      const float4 lo = box[2 * t], hi = box[2 * t + 1];
      // the box point nearest to the query is the query clamped into the box; squares shared across the metrics
      const float dx = qp.x - fminf(fmaxf(qp.x, lo.x), hi.x);
      const float dy = qp.y - fminf(fmaxf(qp.y, lo.y), hi.y);
      const float dz = qp.z - fminf(fmaxf(qp.z, lo.z), hi.z);
      float s[4];
      const float xx = dx * dx, yy = dy * dy;
      s[3] = __builtin_fmaf(dy, dy, xx);
      s[1] = __builtin_fmaf(dz, dz, yy);
      s[2] = __builtin_fmaf(dz, dz, xx);
      s[0] = __builtin_fmaf(dz, dz, s[3]);
#pragma unroll
      for (int m = 0; m < NMET; ++m) {
        const bool lt = s[m] < bd[m];                   // strict: the lowest run wins ties, a NaN never wins
        bd[m] = lt ? s[m] : bd[m];
        bt[m] = lt ? t : bt[m];
      }
    }
    const int i0 = seed_nearest<0>(refs, count, bt[0], qp.x, qp.y, qp.z);
    if constexpr (NMET == 4) {
      const int i1 = seed_nearest<1>(refs, count, bt[1], qp.x, qp.y, qp.z);
      const int i2 = seed_nearest<2>(refs, count, bt[2], qp.x, qp.y, qp.z);
      const int i3 = seed_nearest<3>(refs, count, bt[3], qp.x, qp.y, qp.z);
      uint2 w;
      w.x = (unsigned)i0 | ((unsigned)i1 << 16);
      w.y = (unsigned)i2 | ((unsigned)i3 << 16);
      *reinterpret_cast<uint2*>(rec + (size_t)q * (kNnRec / 2)) = w;
    } else {
      rec[(size_t)q * (kNnRec / 2)] = (short)i0;
    }
  }
}

template <int BLOCK, int NMET>
__global__ __launch_bounds__(BLOCK) void solve_seed_kernel(SeedArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char seed_smem[];
  const int N = a.N, M = a.M, npad = seed_pad(N), mpad = seed_pad(M);
  const int ntn = npad / kSub, ntm = mpad / kSub;
  float4* s_tgt = reinterpret_cast<float4*>(seed_smem);
  float4* s_mov = s_tgt + mpad;
  float4* s_tbox = s_mov + npad;
  float4* s_mbox = s_tbox + 2 * ntm;
  float* s_pose = reinterpret_cast<float*>(s_mbox + 2 * ntn);
  const int inst = blockIdx.x, tid = threadIdx.x;
  const int pair = inst / a.K;
  const float* __restrict__ src = a.src + (size_t)pair * N * 3;
  const float* __restrict__ tgt = a.tgt + (size_t)pair * M * 3;
  if (tid == 0) {   // the pose as the solve's prologue forms it: fp32 parameters, pose_forward
    float p[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = (float)a.state[(size_t)inst * 24 + k];
    Pose f;
    pose_forward(p, a.angle_base, a.trans_mode, f);
#pragma unroll
    for (int i = 0; i < 9; ++i) s_pose[i] = f.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) s_pose[9 + i] = f.T[i];
  }
  const float4 pad4 = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
  for (int j = tid; j < mpad; j += BLOCK)
    s_tgt[j] = (j < M) ? make_float4(tgt[j * 3], tgt[j * 3 + 1], tgt[j * 3 + 2], 0.f) : pad4;
  __syncthreads();
  float R[9], T[3];
  load_rt(s_pose, R, T);
  for (int j = tid; j < npad; j += BLOCK) {
    float4 v = pad4;
    if (j < N) {
      move_point(R, T, src[j * 3], src[j * 3 + 1], src[j * 3 + 2], v.x, v.y, v.z);
      v.w = 0.f;
    }
    s_mov[j] = v;
  }
  __syncthreads();
  static_assert(BLOCK >= 2 * (kSeedMaxPoints / kSub), "one thread per run of either cloud");
  seed_boxes(s_tgt, M, ntm, 0, s_tbox);
  seed_boxes(s_mov, N, ntn, BLOCK / 2, s_mbox);
  __syncthreads();
  short* ws = a.nn_ws + (size_t)inst * 16 * a.ws_stride;
  // direction B: queries = target points, indices into the moved cloud; direction A: queries = moved points, indices into the target
  seed_direction<BLOCK, NMET>(s_tgt, M, s_mov, N, s_mbox, ws);
  seed_direction<BLOCK, NMET>(s_mov, N, s_tgt, M, s_tbox, ws + (size_t)a.ws_stride * (kNnRec / 2));
}

template <int BLOCK>
int seed_launch(const SeedArgs& a, int P, int use_views, hipStream_t s) {
  const size_t bytes = seed_smem_bytes(a.N, a.M);
  auto go = [&](auto kernel) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
      set_error("houv_solve_seed: cannot reserve %zu B of LDS: %s", bytes, hipGetErrorString(e));
      return 0;
    }
    kernel<<<P * a.K, BLOCK, bytes, s>>>(a);
    return check_launch("houv_solve_seed") ? 1 : 0;
  };
  return use_views ? go(solve_seed_kernel<BLOCK, 4>) : go(solve_seed_kernel<BLOCK, 1>);
}

}  // namespace
}  // namespace houv

extern "C" int houv_solve_seed(const float* src, const float* tgt, int P, int N, int M, int K, const double* state,
                               int angle_base, int trans_mode, int use_views, int16_t* nn_ws, int ws_stride, void* stream) {
  using namespace houv;
  if (P < 0 || N <= 0 || M <= 0 || K <= 0 || angle_base < 0 || angle_base > 3 || trans_mode < 0 || trans_mode > 1) {
    set_error("houv_solve_seed: bad argument P=%d N=%d M=%d K=%d base=%d trans_mode=%d", P, N, M, K, angle_base, trans_mode);
    return 0;
  }
  const int mx = N > M ? N : M;
  if (mx < kSeedMinPoints || mx > kSeedMaxPoints) {
    set_error("houv_solve_seed: the pruned kernels serve clouds of %d..%d points (N=%d M=%d)", kSeedMinPoints, kSeedMaxPoints, N, M);
    return 0;
  }
  if (P == 0) return 1;
  if (!src || !tgt || !state) {
    set_error("houv_solve_seed: null pointer");
    return 0;
  }
  if ((long long)P * K > 0x7fffffffLL) {
    set_error("houv_solve_seed: too many hypotheses");
    return 0;
  }
  if (!nn_ws || ws_stride < mx || (ws_stride & 7)) {
    set_error("houv_solve_seed: needs a workspace of 16 x ws_stride int16 per hypothesis, ws_stride >= max(N,M) and a multiple of 8");
    return 0;
  }
  if ((uintptr_t)nn_ws & 15) {
    set_error("houv_solve_seed: the pruned-mode workspace must be 16-byte aligned");
    return 0;
  }
  const SeedArgs a{src, tgt, N, M, K, state, angle_base, trans_mode, (short*)nn_ws, ws_stride};
  // two 512-thread workgroups share a CU up to 2048 points (68 KiB of LDS each); above, one 1024-thread workgroup has it alone
  if (mx <= 2048) return seed_launch<512>(a, P, use_views, (hipStream_t)stream);
  return seed_launch<1024>(a, P, use_views, (hipStream_t)stream);
}
